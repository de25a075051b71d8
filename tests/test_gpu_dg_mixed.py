"""Float32 fields in float64 grad, div and face-mass on the matrix cores (transform ``"mixed_family"``, csrc/fe_mixed.h,
DESIGN.md section 3j) against the references of oracle/einsum_ref.py: exact data bitwise, signed data within the float64
bound, planted non-finite values in exactly their dependency sets, every accepted placement bitwise the aligned launch (which
holds the two forms of the field loads to the same arithmetic), and the route."""

import numpy as np
import pytest

import feinsum_amd as f
from feinsum_amd import _hip
from oracle import einsum_ref as R

pytestmark = pytest.mark.gpu

TETS = {4: 3, 10: 6, 20: 10, 35: 15}                  # Np -> Nfp
TEL = {"grad": {35: 16, 20: 32, 10: 48, 4: 80}, "div": {35: 16, 20: 16, 10: 48, 4: 80},
       "facemass": {35: 16, 20: 16, 10: 32, 4: 64}}   # elements per wave tile
BASE = {"grad": "xre,rij,ej->xei", "div": "xre,rij,xej->ei", "facemass": "ef,fij,fej->ei"}
OP_LAYOUTS = ("rij", "rji")
FM_LAYOUTS = tuple((j, r) for j in ("ef", "fe") for r in ("fij", "ifj", "fji", "jfi"))
CASES = [(fam, Np) for fam in ("grad", "div", "facemass") for Np in (35, 20, 10, 4)]
IDS = [f"{fam}-Np{Np}" for fam, Np in CASES]
E_LIST = (0, 1, 5, 15, 16, 17, 31, 33, 79, 80, 81, 163, 1003)
SCALES = (-3, 5, -7)


@pytest.fixture(scope="module")
def torch():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    yield torch
    import gc

    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def layouts(fam):
    return OP_LAYOUTS if fam != "facemass" else FM_LAYOUTS


def base_shapes(fam, Np, E):
    """Shapes of (J, operator, field, out) in the base layout."""
    Nfp = TETS[Np]
    if fam == "facemass":
        return (E, 4), (4, Np, Nfp), (4, E, Nfp), (E, Np)
    return (3, 3, E), (3, Np, Np), ((E, Np) if fam == "grad" else (3, E, Np)), ((3, E, Np) if fam == "grad" else (E, Np))


E_AXIS = {"grad": (2, None, 0, 1), "div": (2, None, 1, 0), "facemass": (0, None, 1, 0)}   # of J, operator, field, out


def n_terms(fam, Np):
    return 4 * TETS[Np] if fam == "facemass" else 9 * Np


def subscripts(fam, layout):
    if fam == "facemass":
        return f"{layout[0]},{layout[1]},fej->ei"
    return BASE[fam].replace("rij", layout)


def in_layout(torch, fam, layout, J, op):
    """J and the operator of the base layout, stored as *layout* says."""
    if fam != "facemass":
        return J, (op if layout == "rij" else op.permute(0, 2, 1).contiguous())
    perm = {"fij": (0, 1, 2), "ifj": (1, 0, 2), "fji": (0, 2, 1), "jfi": (2, 0, 1)}[layout[1]]
    return (J if layout[0] == "ef" else J.t().contiguous()), op.permute(*perm).contiguous()


def expr_of(fam, Np, layout, b):
    ext = {"e": "E", "x": 3, "r": 3, "f": 4, "i": Np, "j": TETS[Np] if fam == "facemass" else Np}
    subs = subscripts(fam, layout)
    ins = subs.split("->")[0].split(",")
    shape = lambda s: tuple(ext[c] for c in s)   # noqa: E731
    return f.batched_einsum(subs, [[f.array("J", shape(ins[0]), "float64"), f.array("R", shape(ins[1]), "float64"),
                                    f.array(f"u{k}", shape(ins[2]), "float32")] for k in range(b)])


def cut(t, axis, E):
    return t if axis is None else t.narrow(axis, 0, E).contiguous()


class Data:
    """Operands of one (family, Np) at E elements and b fields in the base layout, on the device, with the reference of
    every field (kind "exact": the int64 einsum of the mantissas; "bounded": longdouble ref and absref of signed uniform data;
    "signed": the same data without a reference).  An element's results depend
    on that element alone, so a launch at E' <= E is checked against the first E' elements."""

    def __init__(self, torch, fam, Np, E, b, kind, seed):
        rng = np.random.default_rng(seed)
        sj, so, sf, _ = base_shapes(fam, Np, E)
        dts = [np.dtype("float64"), np.dtype("float64"), np.dtype("float32")]
        self.fam, self.Np, self.E, self.b, self.subs = fam, Np, E, b, BASE[fam]
        if kind == "exact":
            bits = R.exact_bits(3, dts, n_terms(fam, Np), 53, rng)
            assert bits[2] <= 24 and R.bits_fit(bits, n_terms(fam, Np), 53)
            mants, arrs = R.exact_operands([sj, so] + [sf] * b, dts[:2] + [dts[2]] * b, bits[:2] + [bits[2]] * b,
                                           list(SCALES[:2]) + [SCALES[2]] * b, rng)
            self.host = arrs
            self.ref = [torch.from_numpy(R.exact_reference(self.subs, [mants[0], mants[1], mants[2 + k]], SCALES, np.float64, 53)).cuda()
                        for k in range(b)]
        else:
            self.host = [rng.uniform(-1, 1, sj), rng.uniform(-1, 1, so)] + [rng.uniform(-1, 1, sf).astype(np.float32) for _ in range(b)]
            if kind == "bounded":
                self.bounded = [R.bounded_reference(self.subs, [self.host[0], self.host[1], self.host[2 + k]]) for k in range(b)]
        self.J, self.op = (torch.from_numpy(a).cuda() for a in self.host[:2])
        self.fields = [torch.from_numpy(a).cuda() for a in self.host[2:]]

    def launch(self, torch, layout, E, b, place=None, outs=None):
        """The first *E* elements and *b* fields under "mixed_family"; *place* maps an array to where it lies."""
        ax = E_AXIS[self.fam]
        place = place or (lambda name, t: t)
        J, op = in_layout(torch, self.fam, layout, cut(self.J, ax[0], E), self.op)
        args = {"J": place("J", J), "R": place("R", op)}
        for k in range(b):
            args[f"u{k}"] = place(f"u{k}", cut(self.fields[k], ax[2], E))
        expr = expr_of(self.fam, self.Np, layout, b)
        got = f.evaluate(expr, 0, args, out_dict=outs, transform="mixed_family", wait=True)
        return [got[n] for n in expr.output_names], args


@pytest.fixture(scope="module")
def exact_data(torch):
    cache = {}

    def get(fam, Np):
        if (fam, Np) not in cache:
            cache[fam, Np] = Data(torch, fam, Np, 2648, 9 if fam == "facemass" else 3, "exact", seed=1000 + Np)
        return cache[fam, Np]
    return get


def _check_exact(torch, d, layout, E, b):
    outs, _ = d.launch(torch, layout, E, b)
    ax = E_AXIS[d.fam][3]
    for k, out in enumerate(outs):
        ref = cut(d.ref[k], ax, E)
        assert out.dtype == torch.float64 and out.shape == ref.shape, (layout, E, b, k)
        assert R.differing_entries(out, ref) == 0, (d.fam, d.Np, layout, E, b, k, R.differing_entries(out, ref))


@pytest.mark.parametrize("fam,Np", CASES, ids=IDS)
def test_exact_data_is_bitwise_the_integer_einsum(torch, exact_data, fam, Np):
    """24-bit fields, the rest of the 53 bits on J and the operator: below, at and above one wave tile of every geometry, with
    and without a remainder, odd E (fields through registers) and even (LDS-DMA), every layout, every b."""
    d = exact_data(fam, Np)
    bs = (1, 2, 4, 9) if fam == "facemass" else (1, 3)
    n = 0
    for layout in layouts(fam):
        for E in E_LIST:
            for b in (bs if E in (163, 1003) else (bs[n % len(bs)],)):
                _check_exact(torch, d, layout, E, b)
                n += 1
    info = _hip.last_launch_info()
    assert info["mixed_fields"]


@pytest.mark.parametrize("fam,Np", CASES, ids=IDS)
def test_exact_data_on_one_cu_many_rounds(torch, exact_data, fam, Np):
    """E = 2647 and 2648 on a grid sized for one CU: eight waves walk at least four rounds each at every geometry, which is what
    the ring of two and the counted waits need to go wrong."""
    d = exact_data(fam, Np)
    assert 2647 // TEL[fam][Np] >= 4 * 8
    before = _hip.set_cu_limit(1)
    try:
        for layout in (layouts(fam)[0], layouts(fam)[-1]):
            for E in (2647, 2648):
                _check_exact(torch, d, layout, E, d.b if E == 2648 else 1)
                info = _hip.last_launch_info()
                assert info["blocks"] == 2 and info["mixed_fields"]
    finally:
        _hip.set_cu_limit(before)


@pytest.mark.parametrize("fam,Np", CASES, ids=IDS)
def test_signed_data_within_the_float64_bound(torch, fam, Np):
    d = Data(torch, fam, Np, 2647, 2, "bounded", seed=2000 + Np)
    ext = {"e": 2647, "x": 3, "r": 3, "f": 4, "i": Np, "j": TETS[Np] if fam == "facemass" else Np}
    n = R.bound_terms(BASE[fam], ext, 3)
    ax = E_AXIS[fam][3]
    for E, layout in ((2647, layouts(fam)[0]), (1003, layouts(fam)[-1])):
        outs, _ = d.launch(torch, layout, E, 2)
        for k, out in enumerate(outs):
            ref, absref = (np.take(a, range(E), axis=ax) for a in d.bounded[k])
            got = out.cpu().numpy()
            print(f"{fam} Np={Np} E={E} field {k}: bound ratio {R.bound_ratio(got, ref, absref, n, R.U64):.3f}")
            assert R.bound_violations(got, ref, absref, n, R.U64) == 0


@pytest.mark.parametrize("make", [lambda: expr_of("grad", 35, "rij", 1), lambda: expr_of("div", 35, "rij", 1),
                                  lambda: expr_of("facemass", 35, ("ef", "fij"), 4)], ids=["grad", "div", "facemass-x4"])
def test_validate_batched_einsum_transform(torch, make):
    f.validate_batched_einsum_transform(make(), 0, "mixed_family")


# ---- non-finite values, NaN bands around the inputs, sentinel bands around the outputs -------------------------------------

BAND = 4096   # bytes on either side


def banded(torch, t, fill, shift=0):
    """A copy of *t* that starts *shift* bytes behind a 256-byte boundary, with at least BAND bytes of *fill* on either side;
    ``(view, whole buffer, slice of the view in the buffer)``."""
    item = t.element_size()
    pad = (BAND + 512) // item
    buf = torch.full((t.numel() + 2 * pad,), fill, dtype=t.dtype, device="cuda")
    first = BAND // item + (-(buf.data_ptr() + BAND) % 256) // item + shift // item
    assert (buf.data_ptr() + first * item) % 256 == shift
    view = buf[first:first + t.numel()].view(t.shape)
    view.copy_(t)
    return view, buf, slice(first, first + t.numel())


def bands_intact(torch, buf, sl, fill):
    outside = torch.cat([buf[:sl.start], buf[sl.stop:]])
    return bool(torch.isnan(outside).all()) if fill != fill else bool((outside == fill).all())


@pytest.mark.parametrize("fam,Np", CASES, ids=IDS)
def test_nonfinite_values_reach_exactly_their_dependency_sets(torch, exact_data, fam, Np):
    d = exact_data(fam, Np)
    E, tel = 163, TEL[fam][Np]
    layout = layouts(fam)[Np % len(layouts(fam))]
    b = 2
    ax = E_AXIS[fam]
    sites_e = (3, (E // tel) * tel - 2, E - 1)                  # first tile, last full tile, remainder
    assert sites_e[1] >= (E // tel - 1) * tel >= 0 and sites_e[2] >= (E // tel) * tel
    rng = np.random.default_rng(Np)
    subs = subscripts(fam, layout)
    SENT = -7.25
    for operand in (0, 1, 2):
        for value in (float("nan"), float("inf"), float("-inf")):
            for site in range(3):
                kept = {}

                def place(name, t):
                    view, buf, sl = banded(torch, t, float("nan"))
                    kept[name] = (view, buf, sl)
                    return view
                J, op = in_layout(torch, fam, layout, cut(d.J, ax[0], E), d.op)
                arrays = [J, op, cut(d.fields[1], ax[2], E)]
                # the planted entry: a random index whose element coordinate is the site's
                shape = tuple(arrays[operand].shape)
                idx = [int(rng.integers(0, s)) for s in shape]
                sub = subs.split("->")[0].split(",")[operand]
                if "e" in sub:
                    idx[sub.index("e")] = sites_e[site]
                planted = arrays[operand].clone()
                planted[tuple(idx)] = value
                args = {"J": place("J", planted if operand == 0 else J), "R": place("R", planted if operand == 1 else op),
                        "u0": place("u0", cut(d.fields[0], ax[2], E)), "u1": place("u1", planted if operand == 2 else arrays[2])}
                before = {n: v[0].clone() for n, v in kept.items()}
                outs = {}
                expr = expr_of(fam, Np, layout, b)
                for k, name in enumerate(expr.output_names):
                    o = torch.empty(base_shapes(fam, Np, E)[3], dtype=torch.float64, device="cuda")
                    outs[name] = banded(torch, o, SENT)
                f.evaluate(expr, 0, args, out_dict={n: v[0] for n, v in outs.items()}, transform="mixed_family", wait=True)
                shapes = [tuple(a.shape) for a in arrays]
                dep = torch.from_numpy(R.dependency_set(subs, shapes, operand, tuple(idx))).cuda()
                for k, name in enumerate(expr.output_names):
                    got, ref = outs[name][0], cut(d.ref[k], ax[3], E)
                    hit = dep if (operand < 2 or k == 1) else torch.zeros_like(dep)
                    bad = R.nonfinite_violations(got, ref, hit, value)
                    assert bad == 0, (fam, Np, layout, operand, value, idx, k, bad)
                    assert bands_intact(torch, outs[name][1], outs[name][2], SENT), (fam, Np, "output band", name)
                for n, (view, buf, sl) in kept.items():
                    same = (view == before[n]) | (torch.isnan(view) & torch.isnan(before[n]))
                    assert bool(same.all()) and bands_intact(torch, buf, sl, float("nan")), (fam, Np, "input", n)


# ---- placement: the two load forms, bitwise ----------------------------------------------------------------------------------

def field_planes_aligned(fam, Np, E, ptr):
    """The launcher's rule: every field plane (div) / face slab (face-mass) / the field (grad) on an 8-byte boundary."""
    if fam == "grad":
        return ptr % 8 == 0
    n, per = (3, E * Np * 4) if fam == "div" else (4, E * TETS[Np] * 4)
    return all((ptr + k * per) % 8 == 0 for k in range(n))


@pytest.mark.parametrize("fam,Np", CASES, ids=IDS)
def test_every_accepted_placement_gives_the_aligned_bits(torch, fam, Np):
    d = Data(torch, fam, Np, 164, 2, "signed", seed=3000 + Np)
    forms = set()
    for E in (163, 164):
        for layout in (layouts(fam)[0], layouts(fam)[-1]):
            want, args0 = d.launch(torch, layout, E, 2)
            info = _hip.last_launch_info()
            assert info["plain_field_loads"] == (not all(field_planes_aligned(fam, Np, E, args0[u].data_ptr()) for u in ("u0", "u1")))
            shifts = [{"u0": 4}, {"u0": 8}, {"u1": 12}, {"J": 8}, {"R": 8}, {"out0": 8}, {"out1": 8},
                      {"u0": 4, "u1": 4, "J": 8, "R": 8, "out0": 8, "out1": 8}, {"u0": 12, "u1": 8, "J": 8, "out1": 8}]
            for shift in shifts:
                keep = []

                def place(name, t):
                    view, buf, sl = banded(torch, t, float("nan"), shift.get(name, 0))
                    keep.append(buf)
                    return view
                expr = expr_of(fam, Np, layout, 2)
                outs = {name: place(f"out{k}", torch.empty_like(want[k])) for k, name in enumerate(expr.output_names)}
                got, args = d.launch(torch, layout, E, 2, place=place, outs=outs)
                info = _hip.last_launch_info()
                plain = not all(field_planes_aligned(fam, Np, E, args[u].data_ptr()) for u in ("u0", "u1"))
                assert info["mixed_fields"] and info["plain_field_loads"] == plain, (fam, Np, E, shift, info)
                forms.add(plain)
                for k in range(2):
                    assert got[k].data_ptr() % 256 == shift.get(f"out{k}", 0)
                    assert R.differing_entries(got[k], want[k]) == 0, (fam, Np, layout, E, shift, k)
    assert forms == {True, False}


# ---- the route ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fam", ["grad", "div", "facemass"])
def test_the_route_is_the_new_entry_point(torch, fam):
    from feinsum_amd.measure import _bind, launch_kind

    b = 4 if fam == "facemass" else 1
    expr = expr_of(fam, 35, layouts(fam)[0], b)
    assert launch_kind(expr, "mixed_family", {"E": 4096}) == "mixed_family" and launch_kind(expr, "auto", {"E": 4096}) == "generic"
    d = Data(torch, fam, 35, 4099, b, "signed", seed=7)
    eager, args = d.launch(torch, layouts(fam)[0], 4099, b)
    info = _hip.last_launch_info()
    assert info["mixed_fields"] and info["tiles"] == 4099 // 16 and not info["dynamic_walk"]
    assert f"{'face-mass' if fam == 'facemass' else fam} float32 fields Np=35" in _hip.kernel_resources()
    # a bound launch, captured on a side stream and replayed twice, gives the eager bits
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    q = f.DeviceQueue(0, side)
    outs = {n: torch.full_like(eager[k], float("nan")) for k, n in enumerate(expr.output_names)}
    torch.cuda.synchronize()
    _, bound, _ = _bind(expr, q, args, outs, "mixed_family")
    assert bound.family_code & _hip.FAMILY_FIELDS_F32 and bound.accumulate is None
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
    # alpha, beta: the "axpby" route, bitwise fma(alpha, E, beta * old) for powers of two
    old = {n: torch.ones_like(t) for n, t in outs.items()}
    f.evaluate(expr, 0, args, out_dict=old, transform="mixed_family", alpha=0.5, beta=-2.0, wait=True)
    for k, n in enumerate(expr.output_names):
        assert torch.equal(old[n], 0.5 * eager[k] - 2.0)


@pytest.mark.parametrize("fam", ["grad", "div", "facemass"])
def test_timeit_times_the_new_kernels(torch, fam):
    expr = expr_of(fam, 35, layouts(fam)[0], 4 if fam == "facemass" else 1)
    assert f.timeit(expr, cq=0, transform="mixed_family", long_dim_length=20_000) > 0
    assert _hip.last_launch_info()["mixed_fields"]


# ---- speed --------------------------------------------------------------------------------------------------------------
# Measured on MI355X with tools/bench_mixed_dg.py (profiles/mixed_family/bench_mixed_dg.jsonl) at p = 4,
# E = 2 10^5, face-mass x 4; microseconds per launch:
#              "mixed_family"   "auto" (generic)   cast + float64   auto / mixed   cast / mixed
#   grad            44.0           10282.8              64.1           233.7           1.46
#   div             37.6           10682.9              92.8           284.5           2.47
#   face-mass       81.1            8987.5             258.8           110.8           3.19
SPEED_MEASURED = {"grad": (233.7, 1.46), "div": (284.5, 2.47), "facemass": (110.8, 3.19)}


@pytest.fixture(scope="module")
def speed(torch):
    """Seconds per launch of the three forms of one family at E = 2 10^5, measured once per family in alternating windows."""
    import sys
    from pathlib import Path

    sys.path.insert(0, str(Path(__file__).resolve().parents[1] / "tools"))
    import bench_mixed_dg as B

    cache = {}

    def window(launch, min_seconds):
        reps = 4
        while True:
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(reps):
                launch()
            t1.record()
            t1.synchronize()
            total = t0.elapsed_time(t1) * 1e-3
            if total >= min_seconds:
                return total / reps
            reps *= 4

    def get(fam):
        if fam not in cache:
            forms, keep = B.bound_forms(fam, 2 * 10 ** 5)
            names = ("mixed_family", "auto", "cast+f64")
            for n in names:
                forms[n]()
            torch.cuda.synchronize()
            best = {n: float("inf") for n in names}
            for _ in range(3):
                for n in names:
                    best[n] = min(best[n], window(forms[n], 0.1))
            del keep
            cache[fam] = best
        return cache[fam]
    return get


@pytest.mark.parametrize("fam", ["grad", "div", "facemass"])
def test_faster_than_the_route_auto_takes(speed, fam):
    """(b) / (a): "auto" on the same mixed einsum over "mixed_family".  Measured 233.7 (grad), 284.5 (div), 110.8 (face-mass x 4);
    asserted above half of that: 116.8, 142.2, 55.4."""
    t = speed(fam)
    floor = SPEED_MEASURED[fam][0] / 2
    ratio = t["auto"] / t["mixed_family"]
    print(f"{fam}: auto {t['auto'] * 1e6:.1f} us, mixed_family {t['mixed_family'] * 1e6:.1f} us, ratio {ratio:.1f} (floor {floor:.1f})")
    assert ratio > floor, t


@pytest.mark.parametrize("fam", ["grad", "div", "facemass"])
def test_faster_than_a_conversion_pass_and_the_float64_kernel(speed, fam):
    """(c) / (a): a float32 -> float64 pass of the fields, then the float64 einsum under "auto", over "mixed_family".  Measured 1.46
    (grad), 2.47 (div), 3.19 (face-mass x 4); asserted above the midpoint between 1.0 and that: 1.23, 1.735, 2.095."""
    t = speed(fam)
    floor = (1.0 + SPEED_MEASURED[fam][1]) / 2
    ratio = t["cast+f64"] / t["mixed_family"]
    print(f"{fam}: cast + float64 {t['cast+f64'] * 1e6:.1f} us, mixed_family {t['mixed_family'] * 1e6:.1f} us, ratio {ratio:.2f} (floor {floor:.3f})")
    assert ratio > floor, t


def test_stages_of_an_operator_stay_launches_of_their_own(torch):
    """div, grad and lift x 4 that share J and D would be ONE fused float64 launch; under "mixed_family" they are not merged
    (the fused kernels read float64 fields) and give the bits of the single evaluations."""
    E = 1003
    d = {fam: Data(torch, fam, 35, E, 4 if fam == "facemass" else 1, "signed", seed=11) for fam in ("div", "grad", "facemass")}
    d["grad"].J, d["grad"].op = d["div"].J, d["div"].op          # shared geometry factors and operator
    stages, single = [], []
    for fam in ("div", "grad", "facemass"):
        outs, args = d[fam].launch(torch, layouts(fam)[0], E, d[fam].b)
        stages.append((expr_of(fam, 35, layouts(fam)[0], d[fam].b), args))
        single.append(outs)
    op = f.bind_operator(stages, 0, transform="mixed_family")
    assert op.entry_points == ("fe_div_mixed", "fe_grad_mixed", "fe_facemass_mixed")
    op.launch()
    torch.cuda.synchronize()
    for (expr, _), outs, want in zip(stages, op.outputs, single):
        for k, n in enumerate(expr.output_names):
            assert torch.equal(outs[n], want[k])
