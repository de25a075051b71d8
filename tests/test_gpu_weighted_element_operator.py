"""The weighted element operator 'iq,eq,qj,ej->ei' in one matrix-core kernel (transform "weighted_element_operator",
fe_weightedop_f64), on the device:

- exact data at every size where the kernel takes another path -- row tiles and k steps of both products with and without
  padding, one and several tiles, a partial last tile, fewer elements than a tile, more than two rounds of the persistent
  grid -- all four templates, one, three and nine fields, through ``evaluate`` and through the C entry point: bitwise the
  int64 einsum;
- signed random data within gamma(n, u) absref; results that do not depend on where an element sits in its array;
- every array between guard bands, 0 and 8 bytes past a 256-byte boundary; a planted NaN / Inf stays in its dependency set;
- refusals, the launch record, accumulation through fe_axpby, a captured stage, a side-stream queue, and one speed floor."""

import math
import sys
from pathlib import Path

import numpy as np
import pytest

import feinsum_amd as f
from feinsum_amd import _hip
from feinsum_amd.diagnostics import InvalidParameterError
from feinsum_amd.family import (WEIGHTED_ELEMENT_OPERATOR_RULE, WO_A_T, WO_P_T, weighted_element_operator_lds_bytes,
                                weighted_element_operator_supported)
from oracle import einsum_ref as R

sys.path.insert(0, str(Path(__file__).resolve().parents[1] / "tools"))
import fuzz_dg as D  # noqa: E402

pytestmark = pytest.mark.gpu

F64 = np.float64
NAME = "weighted_element_operator"
SUBS = "iq,eq,qj,ej->ei"
MUST_HAVE = ((35, 56, 35), (20, 35, 20), (10, 20, 10), (4, 10, 4), (20, 56, 35), (35, 56, 20), (35, 35, 35))
_ok = weighted_element_operator_supported
#: the largest Nj the rule admits beside the largest (Ni, Nq) of every pair of row-tile counts (RI, RQ)
TILE_MAX = tuple((16 * ri, 16 * rq, max(nj for nj in range(1, 65) if _ok(16 * ri, 16 * rq, nj))) for ri in (1, 2, 3) for rq in (1, 2, 3, 4))
#: the shape of the rule that needs the most LDS
LARGEST = max(((ni, nq, nj) for ni in range(1, 49) for nq in range(1, 65) for nj in range(1, 49) if _ok(ni, nq, nj)),
              key=lambda s: (weighted_element_operator_lds_bytes(*s), s))
SHAPES = tuple(s for s in dict.fromkeys(
    [(ni, nq, nj) for ni in (1, 16, 17, 35) for nq in (1, 4, 5, 16, 17, 56, 64) for nj in (1, 4, 5, 35)] + list(MUST_HAVE)
    + list(TILE_MAX)) if _ok(*s))
SIZES = (1, 15, 16, 17, 63, 65, 1003)
#: (subscripts, FE_WO_P_T | FE_WO_A_T)
TEMPLATES = ((SUBS, 0), ("qi,eq,qj,ej->ei", WO_P_T), ("iq,eq,jq,ej->ei", WO_A_T), ("qi,eq,jq,ej->ei", WO_P_T | WO_A_T))
TILE = 16     # elements of a wave tile
_id = lambda s: "x".join(map(str, s))   # noqa: E731


@pytest.fixture(scope="module")
def torch():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


@pytest.fixture(scope="module", autouse=True)
def _leave_the_device_as_found(torch):
    yield
    import gc

    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def two_rounds(torch):
    """Elements of a launch just above two rounds of the persistent grid: two blocks of four waves per CU, a tile per wave."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    return 2 * (2 * cus * 4) * TILE + 21


def test_the_shapes_cross_every_boundary_inside_the_rule():
    assert TILE_MAX == ((16, 16, 48), (16, 32, 48), (16, 48, 48), (16, 64, 48), (32, 16, 48), (32, 32, 48), (32, 48, 48),
                        (32, 64, 48), (48, 16, 48), (48, 32, 48), (48, 48, 48), (48, 64, 44))
    assert LARGEST == (48, 63, 48) and weighted_element_operator_lds_bytes(*LARGEST) == 81472
    assert len(SHAPES) == 4 * 7 * 4 + len(MUST_HAVE) + len(TILE_MAX) - 1      # nothing was filtered out; (35, 56, 35) is in two lists
    assert all(s in SHAPES for s in MUST_HAVE)


class Exact:
    """Exact data of one shape for up to *E* elements and *b* fields: integer mantissas of four operands whose every partial
    sum of Nq Nj terms fits 53 bits (``bits_fit``), the int64 einsum computed once; a smaller launch takes the leading elements
    (an element's result depends on its own rows only)."""

    def __init__(self, shape, E, b, seed):
        Ni, Nq, Nj = shape
        rng = np.random.default_rng(seed)
        bits = R.exact_bits(4, [F64] * 4, Nq * Nj, 53, rng)
        assert R.bits_fit(bits, Nq * Nj, 53)
        mants, arrays = R.exact_operands([(Ni, Nq), (E, Nq), (Nq, Nj)] + [(E, Nj)] * b, [F64] * (3 + b), bits[:3] + [bits[3]] * b,
                                         [0] * (3 + b), rng)
        (self.mP, self.mW, self.mA, *self.mu), (self.P, self.W, self.A, *self.u) = mants, arrays
        self.ref = [R.int_reference(SUBS, [self.mP, self.mW, self.mA, m], 0, F64, 53) for m in self.mu]
        self.shape, self.E, self.b = shape, E, b

    def stored(self, flags):
        return (np.ascontiguousarray(self.P.T) if flags & WO_P_T else self.P, np.ascontiguousarray(self.A.T) if flags & WO_A_T else self.A)


def _expr(subs, shape, b, same=False):
    """*same*: one array in both operator positions (the caller's shapes must allow it)."""
    Ni, Nq, Nj = shape
    dims = {"iq": (Ni, Nq), "qi": (Nq, Ni), "eq": ("E", Nq), "qj": (Nq, Nj), "jq": (Nj, Nq), "ej": ("E", Nj)}
    name = {"iq": "P", "qi": "P", "eq": "W", "qj": "P" if same else "A", "jq": "P" if same else "A"}
    return f.batched_einsum(subs, [[f.array(name.get(s, f"u{k}"), dims[s]) for s in subs.split("->")[0].split(",")] for k in range(b)])


def _launch(torch, shape, E, P, W, A, us, flags=0, shifts=(0, 0, 0, 0, 0), stream=0):
    """One fe_weightedop_f64 call on embedded arrays (tools/fuzz_dg.py: inputs between NaN bands, outputs between sentinel
    bands, *shifts* doubles past a 256-byte boundary: P, W, A, every u, every out); returns the outputs after checking that
    the inputs are bitwise what they were, the bands intact."""
    Ni, Nq, Nj = shape
    as_t = lambda a: a if torch.is_tensor(a) else torch.from_numpy(a)   # noqa: E731
    eP = D.embed(torch, tuple(P.shape), torch.float64, shifts[0], "in", as_t(P))
    eW = D.embed(torch, (E, Nq), torch.float64, shifts[1], "in", as_t(W))
    eA = D.embed(torch, tuple(A.shape), torch.float64, shifts[2], "in", as_t(A))
    eu = [D.embed(torch, (E, Nj), torch.float64, shifts[3], "in", as_t(u)) for u in us]
    eo = [D.embed(torch, (E, Ni), torch.float64, shifts[4], "out") for _ in us]
    ins = [eP, eW, eA, *eu]
    snaps = [e.snapshot() for e in ins]
    torch.cuda.synchronize()
    _hip.weightedop(eP.view.data_ptr(), eW.view.data_ptr(), eA.view.data_ptr(), [e.view.data_ptr() for e in eu],
                    [e.view.data_ptr() for e in eo], E, Ni, Nq, Nj, flags, stream)
    torch.cuda.synchronize()
    for e, s in zip(ins, snaps):
        assert e.unchanged(s), ("an input changed", shape, E, e.first_change(s))
    for e in eo:
        assert e.guards_intact(), ("a store outside the output", shape, E)
    return [e.view.clone() for e in eo]


def _bits(t):
    import torch

    return t.contiguous().view(torch.int64)


def _rnd(torch, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return lambda *s: torch.rand(*s, generator=g, device="cuda", dtype=torch.float64) * 2 - 1


# ---- 1. exact data -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_exact_data_bitwise_the_int64_einsum(torch, shape):
    """Every size x every template; the field count (1, 3) and the path (``evaluate``, the C entry point) alternate over them so
    that every template meets both counts on both paths in every shape."""
    d = Exact(shape, max(SIZES), 3, 1000 * shape[0] + 100 * shape[1] + shape[2])
    dev = {"W": torch.from_numpy(d.W).cuda(), **{f"u{k}": torch.from_numpy(u).cuda() for k, u in enumerate(d.u)}}
    for n, E in enumerate(SIZES):
        for t, (subs, flags) in enumerate(TEMPLATES):
            b = (1, 3)[(n + t) % 2]
            direct = ((n + t) // 2) % 2 == 1
            P, A = d.stored(flags)
            if direct:
                outs = _launch(torch, shape, E, P, d.W[:E], A, [u[:E] for u in d.u[:b]], flags)
            else:
                expr = _expr(subs, shape, b)
                arrays = {"P": torch.from_numpy(P).cuda(), "A": torch.from_numpy(A).cuda(), **{nm: dev[nm][:E].contiguous() for nm in dev}}
                got = f.evaluate(expr, 0, {nm: arrays[nm] for nm in expr.all_args}, transform=NAME, wait=True)
                outs = [got[nm] for nm in expr.output_names]
            info = _hip.last_launch_info()
            assert info.get(NAME) and not info.get("element_operator"), info
            assert info["tiles"] == -(-E // TILE) and not info["dynamic_walk"], info     # per launch: a tile carries every field
            for k in range(b):
                bad = R.differing_entries(outs[k].cpu().numpy(), d.ref[k][:E])
                assert bad == 0, (shape, E, subs, b, "direct" if direct else "evaluate", k, bad)


def test_nine_fields_take_two_kernel_launches_and_one_array_may_be_both_operators(torch):
    shape, E = (35, 56, 35), 1003
    d = Exact(shape, E, 9, 99)
    for flags in (0, WO_P_T | WO_A_T):
        P, A = d.stored(flags)
        outs = _launch(torch, shape, E, P, d.W, A, d.u, flags)
        info = _hip.last_launch_info()          # the record of the second launch: one field, the same tiles
        assert info.get(NAME) and info["tiles"] == -(-E // TILE), info
        assert [R.differing_entries(o.cpu().numpy(), r) for o, r in zip(outs, d.ref)] == [0] * 9, flags
    expr = _expr(SUBS, shape, 9)
    arrays = {"P": d.P, "W": d.W, "A": d.A, **{f"u{k}": u for k, u in enumerate(d.u)}}
    got = f.evaluate(expr, 0, {nm: torch.from_numpy(a).cuda() for nm, a in arrays.items()}, transform=NAME, wait=True)
    assert [R.differing_entries(got[nm].cpu().numpy(), r) for nm, r in zip(expr.output_names, d.ref)] == [0] * 9
    # the Galerkin form qi,eq,qj,ej->ei: one array in both operator positions (it gets the smaller of the two shares of bits)
    rng = np.random.default_rng(7)
    bits = R.exact_bits(4, [F64] * 4, 56 * 35, 53, rng)
    bits = [min(bits[0], bits[2]), bits[1], min(bits[0], bits[2]), bits[3]]
    (mS, mW, *mu), (S, W, *us) = R.exact_operands([(56, 35), (E, 56)] + [(E, 35)] * 3, [F64] * 5, bits[:2] + [bits[3]] * 3, [0] * 5, rng)
    gal = _expr("qi,eq,qj,ej->ei", shape, 3, same=True)
    dev = {"P": torch.from_numpy(S).cuda(), "W": torch.from_numpy(W).cuda(), **{f"u{k}": torch.from_numpy(us[k]).cuda() for k in range(3)}}
    assert sorted(gal.all_args) == sorted(dev)
    got = f.evaluate(gal, 0, dev, transform=NAME, wait=True)
    for k, nm in enumerate(gal.output_names):
        ref = R.int_reference("qi,eq,qj,ej->ei", [mS, mW, mS, mu[k]], 0, F64, 53)
        assert R.differing_entries(got[nm].cpu().numpy(), ref) == 0, k


# ---- 2. beyond the first rounds of the grid ------------------------------------------------------------------------

@pytest.mark.parametrize("shape", ((35, 56, 35), (17, 5, 5), LARGEST), ids=_id)
def test_exact_data_above_two_rounds_of_the_grid(torch, two_rounds, shape):
    """The int64 einsum is computed for 2053 elements and element e of the launch is element e mod 2053 of them (an odd
    period: a repeated element meets other lanes and other neighbours in every tile) -- an element's result depends on its own
    rows only, so the int64 einsum of the whole launch is that gather."""
    E = two_rounds
    d = Exact(shape, 2053, 3, 77 + shape[0])
    rows = np.arange(E) % 2053
    W, us, refs = d.W[rows], [u[rows] for u in d.u], [r[rows] for r in d.ref]
    for subs, flags in (TEMPLATES[3], TEMPLATES[0]):
        P, A = d.stored(flags)
        (out,) = _launch(torch, shape, E, P, W, A, us[:1], flags)
        info = _hip.last_launch_info()
        assert info["tiles"] == -(-E // TILE) and info["blocks"] * info["waves_per_block"] * 2 < info["tiles"], info
        assert R.differing_entries(out.cpu().numpy(), refs[0]) == 0, (shape, subs)
    three = _launch(torch, shape, E, d.P, W, d.A, us)           # three fields in one launch: fields innermost in the walk
    for k in range(3):
        (alone,) = _launch(torch, shape, E, d.P, W, d.A, [us[k]])
        assert torch.equal(_bits(three[k]), _bits(alone)), (shape, k)      # independent of b
        assert R.differing_entries(three[k].cpu().numpy(), refs[k]) == 0, (shape, k)


# ---- 3. signed random data within the project's bound --------------------------------------------------------------

@pytest.mark.parametrize("shape", MUST_HAVE + TILE_MAX + ((17, 5, 5), (1, 1, 1), (13, 17, 13)), ids=_id)
def test_signed_random_data_within_the_bound(torch, shape):
    """n = 3 + Nq Nj, the project's count for a four-operand einsum; the kernel's own chain has Nj + Nq + 1 roundings per
    entry (the first sum, the weight, the second sum), which never exceeds it: the bound is derived, not measured."""
    Ni, Nq, Nj = shape
    E = 1003
    rng = np.random.default_rng(5 * Ni + 3 * Nq + Nj)
    P, W, A, u = (rng.random(s) * 2 - 1 for s in ((Ni, Nq), (E, Nq), (Nq, Nj), (E, Nj)))
    ref, absref = R.bounded_reference(SUBS, [P, W, A, u])
    n = R.bound_terms(SUBS, {"e": E, "i": Ni, "q": Nq, "j": Nj}, 4)
    assert n == 3 + Nq * Nj >= Nj + Nq + 1
    for subs, flags in TEMPLATES:
        (out,) = _launch(torch, shape, E, np.ascontiguousarray(P.T) if flags & WO_P_T else P, W,
                         np.ascontiguousarray(A.T) if flags & WO_A_T else A, [u], flags)
        assert R.bound_violations(out.cpu().numpy(), ref, absref, n, R.U64) == 0, (shape, subs)


# ---- 4. an element's result does not depend on where it sits -------------------------------------------------------

@pytest.mark.parametrize("shape", ((35, 56, 35), (17, 5, 5), (20, 56, 35)), ids=_id)
def test_position_independence(torch, two_rounds, shape):
    Ni, Nq, Nj = shape
    rnd = _rnd(torch, 11 + Ni)
    P, A, W, u = rnd(Ni, Nq), rnd(Nq, Nj), rnd(two_rounds, Nq), rnd(two_rounds, Nj)
    n = 37
    (small,) = _launch(torch, shape, n, P, W[:n], A, [u[:n]])
    assert bool(torch.isfinite(small).all())
    (mid,) = _launch(torch, shape, 1003, P, W[:1003], A, [u[:1003]])
    (big,) = _launch(torch, shape, two_rounds, P, W, A, [u])
    assert torch.equal(_bits(mid[:n]), _bits(small)) and torch.equal(_bits(big[:n]), _bits(small))
    W2, u2 = W.clone(), u.clone()
    W2[5000:5000 + n], u2[5000:5000 + n] = W[:n], u[:n]       # 5000 = 312 tiles + 8: other lanes, another tile boundary
    moved = _launch(torch, shape, two_rounds, P, W2, A, [u, u2])      # ... and as the second field of its tile
    assert torch.equal(_bits(moved[1][5000:5000 + n]), _bits(small)) and torch.equal(_bits(moved[1][:n]), _bits(small))
    assert torch.equal(_bits(moved[0][:5000]), _bits(big[:5000])) and torch.equal(_bits(moved[0][5000 + n:]), _bits(big[5000 + n:]))


# ---- 5. guard bands and placement ----------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", ((17, 5, 5), (35, 56, 35), (4, 10, 4), LARGEST), ids=_id)
@pytest.mark.parametrize("E", (1, 17, 1003))
def test_guard_bands_and_placement(torch, shape, E):
    Ni, Nq, Nj = shape
    rnd = _rnd(torch, 3 * Ni + E)
    P, A, W, us = rnd(Ni, Nq), rnd(Nq, Nj), rnd(E, Nq), [rnd(E, Nj), rnd(E, Nj)]
    for flags in (0, WO_P_T | WO_A_T):
        sP, sA = (P.T.contiguous(), A.T.contiguous()) if flags else (P, A)
        base = _launch(torch, shape, E, sP, W, sA, us, flags)
        assert all(bool(torch.isfinite(o).all()) for o in base)
        for shifts in ((1, 0, 0, 0, 0), (0, 1, 0, 0, 0), (0, 0, 1, 0, 0), (0, 0, 0, 1, 0), (0, 0, 0, 0, 1), (0, 1, 0, 1, 0),
                       (1, 1, 1, 1, 1)):
            outs = _launch(torch, shape, E, sP, W, sA, us, flags, shifts)
            for o, ref in zip(outs, base):
                assert bool(torch.isfinite(o).all()) and torch.equal(_bits(o), _bits(ref)), (shape, E, flags, shifts)


# ---- 6. a planted non-finite value reaches exactly its dependency set ----------------------------------------------

@pytest.mark.parametrize("shape", ((35, 56, 35), (17, 5, 5)), ids=_id)
def test_a_planted_non_finite_value_stays_in_its_dependency_set(torch, shape):
    Ni, Nq, Nj = shape
    E = 1003                      # 62 full tiles and one of 11 elements: element 1002 is the partial tile's last one
    d = Exact(shape, E, 1, 31 + Ni)
    shapes = [(Ni, Nq), (E, Nq), (Nq, Nj), (E, Nj)]
    spots = [(3, (E - 1, Nj - 1)), (3, (31, 0)),           # u: the partial tile's last element, a full tile's last one
             (1, (E - 1, Nq - 1)), (1, (31, 0)),           # W: likewise; the last column lies in the padded fragments
             (2, (Nq - 1, Nj - 1)), (0, (Ni - 1, Nq - 1)), (0, (0, 0))]
    for operand, index in spots:
        dep = R.dependency_set(SUBS, shapes, operand, index)
        for planted in (math.nan, math.inf):
            host = [d.P.copy(), d.W.copy(), d.A.copy(), d.u[0].copy()]
            host[operand][index] = planted
            for flags in (0, WO_P_T | WO_A_T):
                P = np.ascontiguousarray(host[0].T) if flags else host[0]
                A = np.ascontiguousarray(host[2].T) if flags else host[2]
                (out,) = _launch(torch, shape, E, P, host[1], A, [host[3]], flags)
                assert R.nonfinite_violations(out.cpu().numpy(), d.ref[0], dep, planted) == 0, (shape, operand, index, planted, flags)


# ---- 7. refusals on the device -------------------------------------------------------------------------------------

def test_an_unsupported_size_is_refused_before_anything_is_written(torch):
    E = 100
    for shape in ((35, 84, 35), (48, 64, 48), (49, 4, 4)):
        Ni, Nq, Nj = shape
        expr = _expr(SUBS, shape, 1)
        ones = lambda *s: torch.ones(*s, dtype=torch.float64, device="cuda")   # noqa: E731
        arrays = {"P": ones(Ni, Nq), "W": ones(E, Nq), "A": ones(Nq, Nj), "u0": ones(E, Nj)}
        out = torch.full((E, Ni), D.SENTINEL, dtype=torch.float64, device="cuda")
        count = lambda: torch.cuda.memory_stats().get("allocation.all.allocated", 0)   # noqa: E731  (allocations so far)
        before = count()
        with pytest.raises(NotImplementedError) as exc:
            f.evaluate(expr, 0, arrays, out_dict={expr.output_names[0]: out}, transform=NAME, wait=True)
        assert WEIGHTED_ELEMENT_OPERATOR_RULE in str(exc.value)
        with pytest.raises(NotImplementedError):
            f.evaluate(expr, 0, arrays, transform=NAME, wait=True)          # ... nor allocated
        assert count() == before
        with pytest.raises(NotImplementedError, match="size rule"):
            _hip.weightedop(arrays["P"].data_ptr(), arrays["W"].data_ptr(), arrays["A"].data_ptr(), [arrays["u0"].data_ptr()],
                            [out.data_ptr()], E, Ni, Nq, Nj)
        torch.cuda.synchronize()
        assert bool((out == D.SENTINEL).all())
    assert f.evaluate(expr, 0, arrays, transform="auto", wait=True)[expr.output_names[0]].shape == (E, Ni)   # other routes still run it


def test_aliasing_slices_other_dtypes_and_differentiation_are_refused(torch):
    shape, E = (20, 35, 20), 64
    Ni, Nq, Nj = shape
    expr = _expr(SUBS, shape, 1)
    ones = lambda *s: torch.ones(*s, dtype=torch.float64, device="cuda")   # noqa: E731
    arrays = {"P": ones(Ni, Nq), "W": ones(E, Nq), "A": ones(Nq, Nj), "u0": ones(E, Nj)}
    name = expr.output_names[0]
    with pytest.raises(InvalidParameterError, match="shares memory"):
        f.evaluate(expr, 0, arrays, out_dict={name: arrays["u0"]}, transform=NAME)
    for sliced in ("u0", "W"):
        base = ones(2 * E, arrays[sliced].shape[1])
        with pytest.raises(InvalidParameterError, match="C-contiguous"):
            f.evaluate(expr, 0, {**arrays, sliced: base[::2]}, transform=NAME)
    with pytest.raises(InvalidParameterError, match="C-contiguous"):
        f.evaluate(expr, 0, arrays, out_dict={name: ones(E, 2 * Ni)[:, :Ni]}, transform=NAME)
    dims = {"P": (Ni, Nq), "W": ("E", Nq), "A": (Nq, Nj), "u0": ("E", Nj)}
    f32 = f.einsum(SUBS, *[f.array(nm, dims[nm], "float32") for nm in ("P", "W", "A", "u0")])
    with pytest.raises(NotImplementedError, match=NAME):
        f.evaluate(f32, 0, {nm: t.float() for nm, t in arrays.items()}, transform=NAME)
    mixed = f.einsum(SUBS, *[f.array(nm, dims[nm], "float32" if nm == "u0" else "float64") for nm in ("P", "W", "A", "u0")])
    with pytest.raises(NotImplementedError, match=NAME):
        f.evaluate(mixed, 0, {**arrays, "u0": arrays["u0"].float()}, transform=NAME)
    with pytest.raises(NotImplementedError, match=NAME):
        f.evaluate_differentiable(expr, 0, arrays, transform=NAME)
    for forced in ("kernel", "epilogue"):
        with pytest.raises(NotImplementedError):
            f.evaluate(expr, 0, arrays, out_dict={name: torch.zeros(E, Ni, dtype=torch.float64, device="cuda")},
                       transform={"variant": NAME, "accumulate": forced}, alpha=2.0, beta=1.0)


# ---- 8. the host features ------------------------------------------------------------------------------------------

def test_accumulation_through_axpby_is_the_fused_multiply_add(torch):
    shape, E = (35, 56, 35), 1003
    Ni, Nq, Nj = shape
    rnd = _rnd(torch, 9)
    expr = _expr("qi,eq,jq,ej->ei", shape, 2)
    arrays = {"P": rnd(Nq, Ni), "W": rnd(E, Nq), "A": rnd(Nj, Nq), "u0": rnd(E, Nj), "u1": rnd(E, Nj)}
    plain = f.evaluate(expr, 0, arrays, transform=NAME, wait=True)
    assert f.accumulate_route(expr, NAME) == "axpby"
    for alpha, beta in ((2.0, -0.5), (-0.25, 4.0), (0.5, 0.0)):
        old = {nm: rnd(E, Ni) for nm in expr.output_names}
        outs = {nm: t.clone() for nm, t in old.items()}
        f.evaluate(expr, 0, arrays, out_dict=outs, transform=NAME, alpha=alpha, beta=beta, wait=True)
        for nm in expr.output_names:
            # powers of two: both products are exact, so the combine is one correctly rounded sum
            want = alpha * plain[nm] + beta * old[nm]
            assert torch.equal(_bits(outs[nm]), _bits(want)), (alpha, beta, nm)


def test_a_bound_stage_is_a_launch_of_its_own_and_replays_to_the_same_bits(torch):
    from dg import div, grad

    Np, E = 35, 1003
    rnd = _rnd(torch, 21)
    geo = {"J": rnd(3, 3, E), "R": rnd(3, Np, Np)}
    mass = _expr(SUBS, (35, 56, 35), 4)
    arrays = {"P": rnd(35, 56), "W": rnd(E, 56), "A": rnd(56, 35), **{f"u{k}": rnd(E, 35) for k in range(4)}}
    eager = {nm: t.clone() for nm, t in f.evaluate(mass, 0, arrays, transform=NAME, wait=True).items()}
    op = f.bind_operator([(mass, arrays)], 0, transform=NAME)
    assert op.entry_points == ("fe_weightedop_f64",), op.entry_points
    fused = f.bind_operator([(div(), {**geo, "u": rnd(3, E, Np)}), (grad(), {**geo, "u": rnd(E, Np)})], 0)
    assert len(fused.entry_points) == 1          # (untouched: div + grad still share a launch)
    op.launch()
    torch.cuda.synchronize()
    info = _hip.last_launch_info()
    assert info.get(NAME) and info["tiles"] == -(-E // TILE) and info["bodies"] == 1, info
    outs = op.outputs[0]
    assert all(torch.equal(_bits(outs[nm]), _bits(eager[nm])) for nm in mass.output_names)
    side = torch.cuda.Stream(priority=-1)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        op.launch(int(torch.cuda.current_stream().cuda_stream))
    for nm in mass.output_names:
        outs[nm].fill_(math.nan)
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(_bits(outs[nm]), _bits(eager[nm])) for nm in mass.output_names)
    graph.reset()


def test_a_queue_on_another_stream_matches_the_default_stream(torch):
    shape, E = (20, 56, 35), 1003
    Ni, Nq, Nj = shape
    rnd = _rnd(torch, 4)
    expr = _expr(SUBS, shape, 1)
    arrays = {"P": rnd(Ni, Nq), "W": rnd(E, Nq), "A": rnd(Nq, Nj), "u0": rnd(E, Nj)}
    name = expr.output_names[0]
    here = f.evaluate(expr, 0, arrays, transform=NAME, wait=True)[name]
    torch.cuda.synchronize()
    side = torch.cuda.Stream(priority=-1)
    q = f.DeviceQueue(0, side)
    there = f.evaluate(expr, q, arrays, transform=NAME, wait=True)[name]
    assert torch.equal(_bits(there), _bits(here))
    f.validate_batched_einsum_transform(expr, q, NAME)
    assert f.timeit_details(expr, transform=NAME, cq=q, long_dim_length=1003, min_rounds=5, min_secs=0.0).rounds >= 5


# ---- 9. speed: one floor -------------------------------------------------------------------------------------------

#: halfway between 1.0 and the ratio tools/bench_weighted_element_operator.py measured at this shape and size on the MI355X
#: (c / d = 1.849 [1.823, 1.877] at (35, 56, 35), b = 1, E = 2e5): the convention of section 3m
SPEED_FLOOR = 1.4245


def test_faster_than_the_three_pass_route(torch):
    """Against what a caller can chain by hand, unchanged by this kernel's arrival: "element_operator" 35 -> 56, an in-place
    ``torch.mul`` by W, "element_operator" 56 -> 35, the E x 56 temporary allocated once."""
    from feinsum_amd.measure import _bind

    shape, E = (35, 56, 35), 200_000
    Ni, Nq, Nj = shape
    rnd = _rnd(torch, 1)
    arrays = {"P": rnd(Ni, Nq), "W": rnd(E, Nq), "A": rnd(Nq, Nj), "u0": rnd(E, Nj)}
    q = f.DeviceQueue(0)
    expr = _expr(SUBS, shape, 1)
    out = torch.empty(E, Ni, dtype=torch.float64, device="cuda")
    fused = _bind(expr, q, arrays, {expr.output_names[0]: out}, NAME)[1]
    up = f.einsum("ij,ej->ei", f.array("A", (Nq, Nj)), f.array("u0", ("E", Nj)))
    down = f.einsum("ij,ej->ei", f.array("P", (Ni, Nq)), f.array("t", ("E", Nq)))
    t, out3 = torch.empty(E, Nq, dtype=torch.float64, device="cuda"), torch.empty_like(out)
    first = _bind(up, q, {"A": arrays["A"], "u0": arrays["u0"]}, {up.output_names[0]: t}, "element_operator")[1]
    second = _bind(down, q, {"P": arrays["P"], "t": t}, {down.output_names[0]: out3}, "element_operator")[1]

    def three_pass(stream_ptr):
        first.launch(stream_ptr)
        torch.mul(t, arrays["W"], out=t)
        second.launch(stream_ptr)

    launch = {"c": three_pass, "d": fused.launch}
    times = {"c": [], "d": []}
    for form in launch:
        _hip.time_with_events(launch[form], 10, q.stream_ptr)          # warm-up
    # (the two routes round differently -- the three-pass one rounds t before the weight is applied as well -- so they agree
    # within the bound of either, not bitwise)
    assert torch.allclose(out, out3, rtol=1e-12, atol=1e-12)
    for _ in range(5):                                     # the forms take turns
        for form in ("c", "d"):
            times[form].append(_hip.time_with_events(launch[form], 20, q.stream_ptr) / 20)
    c, d = (float(np.median(times[form])) for form in ("c", "d"))
    print(f"c (three passes) {c * 1e6:.1f} us, d (weighted_element_operator) {d * 1e6:.1f} us, c / d = {c / d:.3f}, floor {SPEED_FLOOR}")
    # measured c / d = 1.849 [1.823, 1.877]; the floor is (1 + 1.849) / 2
    assert c / d > SPEED_FLOOR, (c, d, c / d)
