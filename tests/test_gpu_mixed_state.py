"""Float32 results from the float32-field grad, div and face-mass kernels (transform ``"mixed_state"``, csrc/fe_mixed.h with
OUT = float).  The contract: every output entry is float32(x), x the float64 value the ``"mixed_family"``
kernel of the same launch stores for that entry, rounded once to nearest-even -- so the results are bitwise
``mixed_family_output.astype(np.float32)``, whatever the load form, the store form and the placement of the arrays."""

import sys
from pathlib import Path

import numpy as np
import pytest

import feinsum_amd as f
from feinsum_amd import _hip
from feinsum_amd.diagnostics import InvalidParameterError
from oracle import einsum_ref as R
from test_gpu_dg_mixed import (BASE, CASES, E_AXIS, E_LIST, IDS, SCALES, TEL, TETS, Data, banded, bands_intact, base_shapes, cut,
                               expr_of, in_layout, layouts, n_terms, subscripts)

pytestmark = pytest.mark.gpu

BS = {"grad": (1, 3), "div": (1, 3), "facemass": (1, 2, 4)}


@pytest.fixture(scope="module")
def torch():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    yield torch
    import gc

    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def launch(torch, d, layout, E, b, transform="mixed_state", place=None, outs=None, **kw):
    """The first *E* elements and *b* fields of *d* (J, op, fields in the base layout) under *transform*."""
    ax = E_AXIS[d.fam]
    place = place or (lambda name, t: t)
    J, op = in_layout(torch, d.fam, layout, cut(d.J, ax[0], E), d.op)
    args = {"J": place("J", J), "R": place("R", op)}
    for k in range(b):
        args[f"u{k}"] = place(f"u{k}", cut(d.fields[k], ax[2], E))
    expr = expr_of(d.fam, d.Np, layout, b)
    got = f.evaluate(expr, 0, args, out_dict=outs, transform=transform, wait=True, **kw)
    return [got[n] for n in expr.output_names], args


def same_bits(torch, got, want):
    """Bitwise, NaN positions compared and not payloads (-0.0 and 0.0 differ here: one rounding of one value has one sign)."""
    if got.dtype != want.dtype or got.shape != want.shape:
        return False
    nan = torch.isnan(want)
    return bool((torch.isnan(got) == nan).all()) and bool((got.view(torch.int32)[~nan] == want.view(torch.int32)[~nan]).all())


def rounded(torch, t64):
    """A float64 device array rounded to float32 by numpy on the host."""
    with np.errstate(over="ignore"):
        return torch.from_numpy(t64.cpu().numpy().astype(np.float32)).cuda()


class Exact24:
    """Operands whose every partial sum fits 24 bits, with the integer einsum cast to float32 (exact) as the reference."""

    def __init__(self, torch, fam, Np, E, b, seed):
        rng = np.random.default_rng(seed)
        sj, so, sf, _ = base_shapes(fam, Np, E)
        dts = [np.dtype("float64"), np.dtype("float64"), np.dtype("float32")]
        self.fam, self.Np, self.E, self.b = fam, Np, E, b
        bits = R.exact_bits(3, dts, n_terms(fam, Np), 24, rng)
        assert R.bits_fit(bits, n_terms(fam, Np), 24)
        mants, arrs = R.exact_operands([sj, so] + [sf] * b, dts[:2] + [dts[2]] * b, bits[:2] + [bits[2]] * b,
                                       list(SCALES[:2]) + [SCALES[2]] * b, rng)
        self.ref = [torch.from_numpy(R.exact_reference(BASE[fam], [mants[0], mants[1], mants[2 + k]], SCALES, np.float32, 24)).cuda()
                    for k in range(b)]
        self.J, self.op = (torch.from_numpy(a).cuda() for a in arrs[:2])
        self.fields = [torch.from_numpy(a).cuda() for a in arrs[2:]]


@pytest.fixture(scope="module")
def exact24(torch):
    cache = {}

    def get(fam, Np):
        if (fam, Np) not in cache:
            cache[fam, Np] = Exact24(torch, fam, Np, 2648, max(BS[fam]), seed=4000 + Np)
        return cache[fam, Np]
    return get


def _check_exact(torch, d, layout, E, b):
    outs, _ = launch(torch, d, layout, E, b)
    for k, out in enumerate(outs):
        ref = cut(d.ref[k], E_AXIS[d.fam][3], E)
        assert out.dtype == torch.float32 and out.shape == ref.shape, (layout, E, b, k)
        assert R.differing_entries(out, ref) == 0, (d.fam, d.Np, layout, E, b, k, R.differing_entries(out, ref))


# ---- 1. exact data ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fam,Np", CASES, ids=IDS)
def test_exact_data_is_bitwise_the_integer_einsum_cast_to_float32(torch, exact24, fam, Np):
    """Results that fit 24 bits: below, at and above one wave tile, with and without a remainder, odd and even E (both load forms,
    and for grad both store forms), the layouts in turn, every b of the case."""
    d = exact24(fam, Np)
    lay, n = layouts(fam), 0
    for E in E_LIST:
        for b in (BS[fam] if E in (163, 1003) else (BS[fam][n % len(BS[fam])],)):
            _check_exact(torch, d, lay[n % len(lay)], E, b)
            n += 1
            if E:
                info = _hip.last_launch_info()
                assert info["mixed_fields"] and info["float32_results"], info
                assert info["dword_stores"] == (fam == "grad" and (E * Np) % 2 == 1), (E, info)
    for layout in lay:                                    # every layout once, with a remainder
        _check_exact(torch, d, layout, 81, BS[fam][-1])


@pytest.mark.parametrize("fam,Np", CASES, ids=IDS)
def test_exact_data_on_one_cu_many_rounds(torch, exact24, fam, Np):
    """E = 2647 and 2648 on a grid sized for one CU: eight waves walk at least four rounds each -- the ring of two slots, the
    counted waits with the new store counts and, at div p = 4, the float out tile over the consumed u planes."""
    d = exact24(fam, Np)
    assert 2647 // TEL[fam][Np] >= 4 * 8
    before = _hip.set_cu_limit(1)
    try:
        for layout in (layouts(fam)[0], layouts(fam)[-1]):
            for E in (2647, 2648):
                _check_exact(torch, d, layout, E, d.b if E == 2648 else 1)
                info = _hip.last_launch_info()
                assert info["blocks"] == 2 and info["float32_results"], info
    finally:
        _hip.set_cu_limit(before)


# ---- 2. signed data: bitwise the float64 results of "mixed_family", rounded on the host ----------------------------------------

@pytest.mark.parametrize("fam,Np", CASES, ids=IDS)
def test_signed_data_is_bitwise_the_rounded_mixed_family_result(torch, fam, Np):
    d = Data(torch, fam, Np, 2647, max(BS[fam]), "signed", seed=5000 + Np)
    for E, layout in ((2647, layouts(fam)[0]), (1003, layouts(fam)[-1]), (1004, layouts(fam)[1]), (17, layouts(fam)[0])):
        for b in BS[fam]:
            want, _ = launch(torch, d, layout, E, b, transform="mixed_family")
            got, _ = launch(torch, d, layout, E, b)
            for k in range(b):
                assert want[k].dtype == torch.float64
                assert same_bits(torch, got[k], rounded(torch, want[k])), (fam, Np, layout, E, b, k)


@pytest.mark.parametrize("fam", ["grad", "div", "facemass"])
@pytest.mark.parametrize("what,exponent", [("subnormal", -135), ("overflow", 127)])
def test_scaled_data_rounds_into_the_subnormal_range_and_to_infinity(torch, fam, what, exponent):
    """J scaled by a power of two (exact in float64): results in the float32 subnormal range (below 2^-126, down to half an ulp of
    2^-149, which rounds to even: 0) and beyond FLT_MAX (+-Inf), bitwise what numpy's float64 -> float32 conversion gives."""
    Np, E, b = 35, 163, BS[fam][-1]
    d = Data(torch, fam, Np, E, b, "signed", seed=6000)
    d.J = d.J * float(2.0 ** exponent)
    want, _ = launch(torch, d, layouts(fam)[0], E, b, transform="mixed_family")
    got, _ = launch(torch, d, layouts(fam)[0], E, b)
    tiny = float(np.finfo(np.float32).tiny)
    for k in range(b):
        ref = rounded(torch, want[k])
        if what == "subnormal":
            assert bool((ref.abs() < tiny).all()) and bool(((ref != 0) & (ref.abs() < tiny)).any())
            assert float(want[k].abs().max()) < tiny
        else:
            assert bool(torch.isinf(ref).any()) and bool(torch.isfinite(want[k]).all())
        print(f"{fam} {what}: field {k}, {int((got[k].view(torch.int32) != ref.view(torch.int32)).sum())} of {ref.numel()} entries differ")
        assert same_bits(torch, got[k], ref), (fam, what, k)


# ---- 3. both store forms, every placement -------------------------------------------------------------------------------------

def dword_rule(fam, Np, E, out_ptrs):
    """The launcher's rule: 16-byte stores when every output plane starts on an 8-byte boundary."""
    odd_planes = fam == "grad" and (E * Np) % 2 == 1
    return odd_planes or any(p % 8 for p in out_ptrs)


@pytest.mark.parametrize("fam,Np", CASES, ids=IDS)
def test_every_placement_of_the_outputs_gives_the_same_bits(torch, fam, Np):
    SENT = -7.25
    d = Data(torch, fam, Np, 164, 2, "signed", seed=7000 + Np)
    forms = set()
    for E in (163, 164):
        layout = layouts(fam)[E % 2]
        want64, _ = launch(torch, d, layout, E, 2, transform="mixed_family")
        want = [rounded(torch, t) for t in want64]
        for shift in ({}, {"out0": 4}, {"out1": 8}, {"out0": 12, "out1": 4}, {"out0": 8, "out1": 8, "u0": 4}, {"out0": 4, "u1": 12, "J": 8}):
            kept, before = {}, {}

            def place(name, t):
                view, buf, sl = banded(torch, t, SENT if name.startswith("out") else float("nan"), shift.get(name, 0))
                kept[name] = (view, buf, sl)
                before[name] = view.clone()
                return view
            expr = expr_of(fam, Np, layout, 2)
            outs = {name: place(f"out{k}", torch.empty_like(want[k])) for k, name in enumerate(expr.output_names)}
            got, args = launch(torch, d, layout, E, 2, place=place, outs=outs)
            info = _hip.last_launch_info()
            dwords = dword_rule(fam, Np, E, [t.data_ptr() for t in got])
            assert info["float32_results"] and info["dword_stores"] == dwords, (fam, Np, E, shift, info)
            forms.add(dwords)
            for k in range(2):
                assert got[k].data_ptr() % 256 == shift.get(f"out{k}", 0)
                assert same_bits(torch, got[k], want[k]), (fam, Np, layout, E, shift, k)
                view, buf, sl = kept[f"out{k}"]
                assert bands_intact(torch, buf, sl, SENT), (fam, Np, E, shift, "output band", k)
            for n in ("J", "R", "u0", "u1"):             # the inputs and their bands are as they were
                view, buf, sl = kept[n]
                assert torch.equal(view, before[n]) and bands_intact(torch, buf, sl, float("nan")), (fam, Np, E, shift, n)
    assert forms == {True, False}


# ---- 4. non-finite values -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fam,Np", CASES, ids=IDS)
def test_nonfinite_values_reach_exactly_their_dependency_sets(torch, exact24, fam, Np):
    d = exact24(fam, Np)
    E, tel = 163, TEL[fam][Np]
    layout = layouts(fam)[Np % len(layouts(fam))]
    ax = E_AXIS[fam]
    sites_e = (3, (E // tel) * tel - 2, E - 1)                  # first tile, last full tile, remainder
    rng = np.random.default_rng(Np)
    subs = subscripts(fam, layout)
    expr = expr_of(fam, Np, layout, 2)
    for operand in (0, 1, 2):
        for value in (float("nan"), float("inf"), float("-inf")):
            site = int(rng.integers(0, 3))
            J, op = in_layout(torch, fam, layout, cut(d.J, ax[0], E), d.op)
            arrays = [J, op, cut(d.fields[1], ax[2], E)]
            idx = [int(rng.integers(0, s)) for s in arrays[operand].shape]
            sub = subs.split("->")[0].split(",")[operand]
            if "e" in sub:
                idx[sub.index("e")] = sites_e[site]
            planted = arrays[operand].clone()
            planted[tuple(idx)] = value
            args = {"J": planted if operand == 0 else J, "R": planted if operand == 1 else op,
                    "u0": cut(d.fields[0], ax[2], E), "u1": planted if operand == 2 else arrays[2]}
            got = f.evaluate(expr, 0, args, transform="mixed_state", wait=True)
            dep = torch.from_numpy(R.dependency_set(subs, [tuple(a.shape) for a in arrays], operand, tuple(idx))).cuda()
            for k, name in enumerate(expr.output_names):
                hit = dep if (operand < 2 or k == 1) else torch.zeros_like(dep)
                bad = R.nonfinite_violations(got[name], cut(d.ref[k], ax[3], E), hit, value)
                assert got[name].dtype == torch.float32 and bad == 0, (fam, Np, layout, operand, value, idx, k, bad)


# ---- 5. the entry points, called directly --------------------------------------------------------------------------------------

@pytest.mark.parametrize("fam", ["grad", "div", "facemass"])
def test_direct_calls_refuse_by_code_and_record_the_new_kernel(torch, fam):
    Np, E, b = 35, 163, 2
    d = Data(torch, fam, Np, E, b, "signed", seed=8000)
    SENT = -3.5
    outs = [torch.full(base_shapes(fam, Np, E)[3], SENT, dtype=torch.float32, device="cuda") for _ in range(b)]
    lib = _hip.load_library()
    entry = getattr(lib, {"grad": "fe_grad3d_mixed_state_f64", "div": "fe_div3d_mixed_state_f64", "facemass": "fe_facemass_mixed_state_f64"}[fam])

    def call(J=None, op=None, v=None, o=None, Np_=Np, Nfp=15, flags=0):
        va = _hip._ptr_array([t.data_ptr() for t in d.fields] if v is None else v)
        oa = _hip._ptr_array([t.data_ptr() for t in outs] if o is None else o)
        J, op = d.J.data_ptr() if J is None else J, d.op.data_ptr() if op is None else op
        if fam == "facemass":
            return entry(J, op, va, oa, E, Np_, 4, Nfp, b, flags, None)
        return entry(J, op, va, oa, E, Np_, b, flags, None)

    o0, u0 = outs[0].data_ptr(), d.fields[0].data_ptr()
    refusals = [(dict(Np_=56, Nfp=21), _hip.FE_EUNSUPPORTED), (dict(Np_=10), _hip.FE_EUNSUPPORTED if fam == "facemass" else None),
                (dict(o=[o0 + 2, o0]), _hip.FE_EINVAL), (dict(v=[u0, u0 + 1]), _hip.FE_EINVAL),
                (dict(J=d.J.data_ptr() + 4), _hip.FE_EINVAL), (dict(op=d.op.data_ptr() + 4), _hip.FE_EINVAL),
                (dict(flags=8), _hip.FE_EINVAL), (dict(J=0), _hip.FE_EINVAL)]
    for kw, code in refusals:
        if code is None:
            continue
        assert call(**kw) == code, (fam, kw, lib.fe_last_error())
        torch.cuda.synchronize()
        assert all(bool((t == SENT).all()) for t in outs), (fam, kw)
        assert _hip.last_launch_info() == {}
    assert call() == _hip.FE_OK
    torch.cuda.synchronize()
    info = _hip.last_launch_info()
    assert info["mixed_fields"] and info["float32_results"] and info["tiles"] == E // 16 and not info["dynamic_walk"], info
    assert info["dword_stores"] == (fam == "grad")        # 163 * 35 is odd
    assert f"{'face-mass' if fam == 'facemass' else fam} float32 fields+results Np=35" in _hip.kernel_resources()
    want, _ = launch(torch, d, layouts(fam)[0], E, b, transform="mixed_family")
    for k in range(b):
        assert same_bits(torch, outs[k], rounded(torch, want[k]))


# ---- 6. alpha, beta -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fam", ["grad", "div", "facemass"])
def test_alpha_beta_take_the_axpby_route_in_float32(torch, fam):
    from feinsum_amd.measure import _bind

    Np, E, b = 20, 163, 2
    d = Data(torch, fam, Np, E, b, "signed", seed=9000)
    layout = layouts(fam)[0]
    plain, args = launch(torch, d, layout, E, b)
    expr = expr_of(fam, Np, layout, b)
    rng = np.random.default_rng(5)
    for alpha, beta in ((0.5, -2.0), (1.7, 0.3), (-0.37, 1.0)):
        old = {n: torch.from_numpy(rng.uniform(-1, 1, tuple(plain[0].shape)).astype(np.float32)).cuda() for n in expr.output_names}
        before = {n: t.cpu().numpy() for n, t in old.items()}
        _, bound, _ = _bind(expr, 0, args, old, "mixed_state", alpha=alpha, beta=beta)
        assert bound.accumulate == "axpby" and all(t.dtype == torch.float32 for t in bound.temps)
        f.evaluate(expr, 0, args, out_dict=old, transform="mixed_state", alpha=alpha, beta=beta, wait=True)
        for k, n in enumerate(expr.output_names):
            # float32 fma(alpha, E32, beta * old): the product beta * old rounded to float32, then one rounding of the sum
            a32, b32 = np.float32(alpha), np.float32(beta)
            t = (b32 * before[n]).astype(np.float32)
            want = (np.longdouble(a32) * plain[k].cpu().numpy().astype(np.longdouble) + t.astype(np.longdouble)).astype(np.float32)
            assert np.array_equal(old[n].cpu().numpy(), want), (fam, alpha, beta, k)
    # beta = 0 does not read the outputs
    nan = {n: torch.full_like(plain[0], float("nan")) for n in expr.output_names}
    f.evaluate(expr, 0, args, out_dict=nan, transform="mixed_state", alpha=2.0, beta=0.0, wait=True)
    for k, n in enumerate(expr.output_names):
        assert torch.equal(nan[n], 2.0 * plain[k])
    with pytest.raises(InvalidParameterError, match="beta"):
        f.evaluate(expr, 0, args, out_dict={expr.output_names[0]: nan[expr.output_names[0]]}, transform="mixed_state", beta=1.0)
    for forced in ("kernel", "epilogue"):
        with pytest.raises(NotImplementedError):
            f.evaluate(expr, 0, args, transform={"variant": "mixed_state", "accumulate": forced}, alpha=2.0)
    # a float64 output is refused, an element slice too, and the differentiable entry point as for "mixed_family"
    with pytest.raises(InvalidParameterError, match="has dtype torch.float64, expected float32"):
        f.evaluate(expr, 0, args, out_dict={expr.output_names[0]: plain[0].double()}, transform="mixed_state")
    name, axis = ("J", 2) if fam == "grad" else ("u0", 1)      # an element axis that is not the leading one
    shape = list(args[name].shape)
    shape[axis] *= 2
    sliced = dict(args, **{name: torch.zeros(shape, dtype=args[name].dtype, device="cuda").narrow(axis, 0, E)})
    with pytest.raises(InvalidParameterError, match="C-contiguous"):
        f.evaluate(expr, 0, sliced, transform="mixed_state")


# ---- 7. the other entry points of the package ---------------------------------------------------------------------------------

@pytest.mark.parametrize("make", [lambda: expr_of("grad", 35, "rij", 1), lambda: expr_of("div", 35, "rji", 3),
                                  lambda: expr_of("facemass", 35, ("ef", "fij"), 4)], ids=["grad", "div-x3", "facemass-x4"])
def test_validate_and_timeit(torch, make):
    f.validate_batched_einsum_transform(make(), 0, "mixed_state")
    f.validate_batched_einsum_transform(make(), 0, {"variant": "mixed_state", "placement": "separate"})
    # (10 000 elements: the outputs stay below the 8 MiB from which timeit takes them from the split allocator, whose searches
    #  for a second class of memory share one time budget per process with every later test)
    assert f.timeit(make(), cq=0, transform="mixed_state", long_dim_length=10_000) > 0
    info = _hip.last_launch_info()
    assert info["mixed_fields"] and info["float32_results"]


def test_outputs_are_allocated_as_float32_and_placement_separate_is_honoured(torch):
    from feinsum_amd import placement
    from feinsum_amd.measure import _bind

    E = 20_000
    expr = expr_of("grad", 35, "rij", 1)
    d = Data(torch, "grad", 35, E, 1, "signed", seed=12)
    args = {"J": d.J, "R": d.op, "u0": d.fields[0]}
    assert 3 * E * 35 * 4 >= placement.SPLIT_MIN_BYTES              # large enough for the split allocator, were it asked
    _, bound, outs = _bind(expr, 0, args, None, {"variant": "mixed_state", "placement": "separate"})
    assert outs[0].dtype == torch.float32 and tuple(outs[0].shape) == (3, E, 35)
    assert dict(bound.output_allocations) == {expr.output_names[0]: "torch (placement: separate)"}
    bound.launch(int(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    want = f.evaluate(expr, 0, args, transform={"variant": "mixed_family", "placement": "separate"}, wait=True)[expr.output_names[0]]
    assert same_bits(torch, outs[0], rounded(torch, want))


@pytest.mark.parametrize("fam", ["grad", "div", "facemass"])
def test_a_side_stream_queue_and_a_captured_bound_launch(torch, fam):
    from feinsum_amd.measure import _bind, _MixedStateLaunch

    b = 4 if fam == "facemass" else 1
    expr = expr_of(fam, 35, layouts(fam)[0], b)
    d = Data(torch, fam, 35, 4099, b, "signed", seed=7)
    eager, args = launch(torch, d, layouts(fam)[0], 4099, b)
    want, _ = launch(torch, d, layouts(fam)[0], 4099, b, transform="mixed_family")
    for k in range(b):
        assert same_bits(torch, eager[k], rounded(torch, want[k]))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    q = f.DeviceQueue(0, side)
    got = f.evaluate(expr, q, args, transform={"variant": "mixed_state", "placement": "separate"}, wait=True)   # allocated on the queue's stream
    for k, n in enumerate(expr.output_names):
        assert got[n].dtype == torch.float32 and torch.equal(got[n], eager[k])
    outs = {n: torch.full_like(eager[k], float("nan")) for k, n in enumerate(expr.output_names)}
    torch.cuda.synchronize()
    _, bound, _ = _bind(expr, q, args, outs, "mixed_state")
    assert isinstance(bound, _MixedStateLaunch) and bound.accumulate is None and len(bound.calls) == 1
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        bound.launch(int(torch.cuda.current_stream().cuda_stream))
    for _ in range(2):
        for t in outs.values():
            t.fill_(float("nan"))
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        for k, n in enumerate(expr.output_names):
            assert torch.equal(outs[n], eager[k])


def test_stages_of_an_operator_stay_launches_of_their_own(torch):
    """div, grad and lift x 4 that share J and D: under "mixed_state" they are not merged, are named by their entry points, and a
    captured and replayed operator gives the bits of the single evaluations."""
    E = 1003
    d = {fam: Data(torch, fam, 35, E, 4 if fam == "facemass" else 1, "signed", seed=11) for fam in ("div", "grad", "facemass")}
    d["grad"].J, d["grad"].op = d["div"].J, d["div"].op          # shared geometry factors and operator
    stages, single = [], []
    for fam in ("div", "grad", "facemass"):
        outs, args = launch(torch, d[fam], layouts(fam)[0], E, d[fam].b)
        stages.append((expr_of(fam, 35, layouts(fam)[0], d[fam].b), args))
        single.append(outs)
    op = f.bind_operator(stages, 0, transform="mixed_state")
    assert op.entry_points == ("fe_div_mixed_state", "fe_grad_mixed_state", "fe_facemass_mixed_state")
    op.launch()
    torch.cuda.synchronize()
    for (expr, _), outs, want in zip(stages, op.outputs, single):
        for k, n in enumerate(expr.output_names):
            assert outs[n].dtype == torch.float32 and torch.equal(outs[n], want[k])
    op.capture()
    for outs in op.outputs:
        for t in outs.values():
            t.fill_(float("nan"))
    op.replay()
    torch.cuda.synchronize()
    for (expr, _), outs, want in zip(stages, op.outputs, single):
        for k, n in enumerate(expr.output_names):
            assert torch.equal(outs[n], want[k])


# ---- speed --------------------------------------------------------------------------------------------------------------------
# Measured on MI355X with tools/bench_mixed_state.py (profiles/mixed_state/bench_mixed_state.jsonl) at
# p = 4, E = 2 10^5, face-mass x 4; microseconds per launch, alternating windows:
#              (a) mixed_state   (b) mixed_family + copy   (c) mixed_family   (d) float64   (b) / (a)
#   grad            36.8               100.5                    43.4              40.6         2.73
#   div             35.3                58.4                    38.1              38.8         1.65
#   face-mass       75.3               161.0                    80.9             104.1         2.14
SPEED_MEASURED = {"grad": 2.73, "div": 1.65, "facemass": 2.14}     # (b) / (a) at E = 2 10^5


@pytest.fixture(scope="module")
def speed(torch):
    """Seconds per launch of the four forms of one family at E = 2 10^5, measured once per family in alternating windows."""
    sys.path.insert(0, str(Path(__file__).resolve().parents[1] / "tools"))
    import bench_mixed_state as B

    cache = {}

    def get(fam):
        if fam not in cache:
            forms, keep = B.bound_forms(fam, 2 * 10 ** 5)
            cache[fam] = B.alternating(forms, B.FORMS, 0.1)
            del keep
        return cache[fam]
    return get


@pytest.mark.parametrize("fam", ["grad", "div", "facemass"])
def test_faster_than_mixed_family_and_a_downcast_pass(speed, fam):
    """(b) / (a): "mixed_family" followed by Tensor.copy_ of every output into a float32 array, over "mixed_state"; asserted above
    the midpoint between 1.0 and the ratio measured at E = 2 10^5 (measured 2.73 / 1.65 / 2.14 for grad / div / face-mass x 4: floors
    1.865, 1.325, 1.57).  (c) "mixed_family" alone and (d) the all-float64 kernel
    are reported."""
    t = speed(fam)
    ratio = t["mixed_family+copy"] / t["mixed_state"]
    print(f"{fam}: (a) mixed_state {t['mixed_state'] * 1e6:.1f} us, (b) mixed_family + copy {t['mixed_family+copy'] * 1e6:.1f} us, "
          f"(c) mixed_family {t['mixed_family'] * 1e6:.1f} us, (d) float64 {t['f64'] * 1e6:.1f} us; (b)/(a) {ratio:.2f}")
    floor = (1.0 + SPEED_MEASURED[fam]) / 2
    assert ratio > floor, (t, floor)
