"""The element-local operator of any shape on the matrix cores (transform "element_operator", fe_elemop_f64; DESIGN.md
section 3q), on the device:

- exact data at every size where the kernel takes another path -- row tiles and k steps with and without padding, one and
  several tiles, a partial last tile, fewer elements than a tile, more than two rounds of the persistent grid -- all four
  templates, one and three fields, through ``evaluate`` and through the C entry point: bitwise the int64 einsum;
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
from feinsum_amd.family import ELEMENT_OPERATOR_RULE, element_operator_supported
from oracle import einsum_ref as R

sys.path.insert(0, str(Path(__file__).resolve().parents[1] / "tools"))
import fuzz_dg as D  # noqa: E402

pytestmark = pytest.mark.gpu

F64 = np.float64
DG_PAIRS = ((56, 35), (35, 56), (84, 35), (35, 84), (60, 35), (35, 60), (20, 35), (35, 20), (10, 20), (20, 10))
#: the largest accepted (Ni, Nj) of every row-tile count: Ni = 16 RT, Nj the most the rule allows beside it
RT_MAX = tuple((16 * rt, max(nj for nj in range(1, 129) if element_operator_supported(16 * rt, nj))) for rt in range(1, 7))
SHAPES = tuple(dict.fromkeys([(ni, nj) for ni in (1, 16, 17, 35, 64) for nj in (1, 4, 5, 35, 64)] + list(DG_PAIRS) + list(RT_MAX)))
SIZES = (1, 15, 16, 17, 63, 65, 1003)
#: (subscripts, FE_OP_TRANSPOSED, with J)
TEMPLATES = (("ij,ej->ei", 0, False), ("ji,ej->ei", 1, False), ("e,ij,ej->ei", 0, True), ("e,ji,ej->ei", 1, True))
TILE = 16     # elements of a wave tile (M = 1)


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


def test_the_rule_accepts_the_largest_pair_of_every_row_tile_count():
    assert RT_MAX == ((16, 96), (32, 96), (48, 84), (64, 64), (80, 48), (96, 40))
    assert all(element_operator_supported(*s) for s in SHAPES) and len(SHAPES) == 25 + 10 + 6 - 1   # (64, 64) is in both lists


class Exact:
    """Exact data of one shape for up to *E* elements and *b* fields: integer mantissas whose every partial sum of Nj terms
    fits 53 bits (``bits_fit``), the int64 einsums with and without J computed once; a smaller launch takes the leading
    elements (an element's result depends on its own rows only)."""

    def __init__(self, Ni, Nj, E, b, seed):
        rng = np.random.default_rng(seed)
        bits = R.exact_bits(3, [F64] * 3, Nj, 53, rng)
        assert R.bits_fit(bits, Nj, 53)
        mants, arrays = R.exact_operands([(E,), (Ni, Nj)] + [(E, Nj)] * b, [F64] * (2 + b), [bits[0], bits[1]] + [bits[2]] * b,
                                         [0] * (2 + b), rng)
        (self.mJ, self.mA, *self.mu), (self.J, self.A, *self.u) = mants, arrays
        self.ref = {True: [R.int_reference("e,ij,ej->ei", [self.mJ, self.mA, m], 0, F64, 53) for m in self.mu],
                    False: [R.int_reference("ij,ej->ei", [self.mA, m], 0, F64, 53) for m in self.mu]}
        self.Ni, self.Nj, self.E, self.b = Ni, Nj, E, b

    def stored(self, opT):
        return np.ascontiguousarray(self.A.T) if opT else self.A


def _expr(subs, Ni, Nj, b):
    shape = {"e": ("E",), "ij": (Ni, Nj), "ji": (Nj, Ni), "ej": ("E", Nj)}
    name = {"e": "J", "ij": "A", "ji": "A"}
    return f.batched_einsum(subs, [[f.array(name.get(s, f"u{k}"), shape[s]) for s in subs.split("->")[0].split(",")] for k in range(b)])


def _launch(torch, Ni, Nj, E, J, A, us, opT=0, shifts=(0, 0, 0, 0), stream=0):
    """One fe_elemop_f64 call on embedded arrays (tools/fuzz_dg.py: inputs between NaN bands, outputs between sentinel bands,
    *shifts* doubles past a 256-byte boundary: J, A, every u, every out); returns the outputs after checking that the inputs
    are bitwise what they were, the bands intact."""
    as_t = lambda a: a if torch.is_tensor(a) else torch.from_numpy(a)   # noqa: E731
    eJ = None if J is None else D.embed(torch, (E,), torch.float64, shifts[0], "in", as_t(J))
    eA = D.embed(torch, tuple(A.shape), torch.float64, shifts[1], "in", as_t(A))
    eu = [D.embed(torch, (E, Nj), torch.float64, shifts[2], "in", as_t(u)) for u in us]
    eo = [D.embed(torch, (E, Ni), torch.float64, shifts[3], "out") for _ in us]
    ins = [e for e in (eJ, eA, *eu) if e is not None]
    snaps = [e.snapshot() for e in ins]
    torch.cuda.synchronize()
    _hip.elemop(None if eJ is None else eJ.view.data_ptr(), eA.view.data_ptr(), [e.view.data_ptr() for e in eu],
                [e.view.data_ptr() for e in eo], E, Ni, Nj, opT, stream)
    torch.cuda.synchronize()
    for e, s in zip(ins, snaps):
        assert e.unchanged(s), ("an input changed", Ni, Nj, E, e.first_change(s))
    for e in eo:
        assert e.guards_intact(), ("a store outside the output", Ni, Nj, E)
    return [e.view.clone() for e in eo]


def _bits(t):
    import torch

    return t.contiguous().view(torch.int64)


# ---- 1. exact data -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", SHAPES, ids=[f"{a}x{b}" for a, b in SHAPES])
def test_exact_data_bitwise_the_int64_einsum(torch, shape):
    """Every size x every template; the field count (1, 3) and the path (``evaluate``, the C entry point) alternate over them so
    that every template meets both counts on both paths in every shape."""
    Ni, Nj = shape
    d = Exact(Ni, Nj, max(SIZES), 3, 1000 * Ni + Nj)
    dev = {"J": torch.from_numpy(d.J).cuda(), **{f"u{k}": torch.from_numpy(u).cuda() for k, u in enumerate(d.u)}}
    for n, E in enumerate(SIZES):
        for t, (subs, opT, with_j) in enumerate(TEMPLATES):
            b = (1, 3)[(n + t) % 2]
            direct = ((n + t) // 2) % 2 == 1
            if direct:
                outs = _launch(torch, Ni, Nj, E, d.J[:E] if with_j else None, d.stored(opT), [u[:E] for u in d.u[:b]], opT)
            else:
                expr = _expr(subs, Ni, Nj, b)
                arrays = {"A": torch.from_numpy(d.stored(opT)).cuda(), **{nm: dev[nm][:E].contiguous() for nm in dev}}
                got = f.evaluate(expr, 0, {nm: arrays[nm] for nm in expr.all_args}, transform="element_operator", wait=True)
                outs = [got[nm] for nm in expr.output_names]
            info = _hip.last_launch_info()
            assert info.get("element_operator") and info["tiles"] == -(-E // TILE) and not info["dynamic_walk"], info
            for k in range(b):
                bad = R.differing_entries(outs[k].cpu().numpy(), d.ref[with_j][k][:E])
                assert bad == 0, (shape, E, subs, b, "direct" if direct else "evaluate", k, bad)


@pytest.mark.parametrize("shape", ((56, 35), (35, 56), (17, 5), (96, 40)), ids=lambda s: f"{s[0]}x{s[1]}")
def test_exact_data_above_two_rounds_of_the_grid(torch, two_rounds, shape):
    Ni, Nj = shape
    E = two_rounds
    d = Exact(Ni, Nj, E, 1, 77 + Ni)
    for subs, opT, with_j in (TEMPLATES[3], TEMPLATES[0]):
        (out,) = _launch(torch, Ni, Nj, E, d.J if with_j else None, d.stored(opT), d.u, opT)
        info = _hip.last_launch_info()
        assert info["tiles"] == -(-E // TILE) and info["blocks"] * info["waves_per_block"] * 2 < info["tiles"], info
        assert R.differing_entries(out.cpu().numpy(), d.ref[with_j][0]) == 0, (shape, subs)
    expr = _expr("e,ij,ej->ei", Ni, Nj, 3)       # three fields in one launch: fields outermost in the walk
    us = [torch.from_numpy(np.roll(d.u[0], k, axis=0)).cuda() for k in range(3)]
    arrays = {"J": torch.from_numpy(d.J).cuda(), "A": torch.from_numpy(d.A).cuda(), "u0": us[0], "u1": us[1], "u2": us[2]}
    got = f.evaluate(expr, 0, arrays, transform="element_operator", wait=True)
    one = _expr("e,ij,ej->ei", Ni, Nj, 1)
    for k, nm in enumerate(expr.output_names):
        alone = f.evaluate(one, 0, {"J": arrays["J"], "A": arrays["A"], "u0": us[k]}, transform="element_operator", wait=True)
        assert torch.equal(_bits(got[nm]), _bits(alone[one.output_names[0]])), (shape, k)     # independent of b
    assert R.differing_entries(got[expr.output_names[0]].cpu().numpy(), d.ref[True][0]) == 0


# ---- 2. signed random data within the project's bound --------------------------------------------------------------

@pytest.mark.parametrize("shape", DG_PAIRS + RT_MAX + ((17, 5), (1, 1), (13, 13)), ids=lambda s: f"{s[0]}x{s[1]}")
def test_signed_random_data_within_the_bound(torch, shape):
    Ni, Nj = shape
    E = 1003
    rng = np.random.default_rng(5 * Ni + Nj)
    J, A, u = (rng.random(s) * 2 - 1 for s in ((E,), (Ni, Nj), (E, Nj)))
    for subs, opT, with_j in TEMPLATES:
        host = ([J] if with_j else []) + [A, u]
        ref, absref = R.bounded_reference("e,ij,ej->ei" if with_j else "ij,ej->ei", host)
        # the J rounding is one more than the einsum's own count (the factor multiplies the finished sum)
        n = R.bound_terms(subs, {"e": E, "i": Ni, "j": Nj}, len(host)) + 1
        (out,) = _launch(torch, Ni, Nj, E, J if with_j else None, np.ascontiguousarray(A.T) if opT else A, [u], opT)
        assert R.bound_violations(out.cpu().numpy(), ref, absref, n, R.U64) == 0, (shape, subs)


# ---- 3. an element's result does not depend on where it sits -------------------------------------------------------

@pytest.mark.parametrize("shape", ((56, 35), (35, 56), (17, 5), (64, 64)), ids=lambda s: f"{s[0]}x{s[1]}")
def test_position_independence(torch, two_rounds, shape):
    Ni, Nj = shape
    g = torch.Generator(device="cuda").manual_seed(11 + Ni)
    rnd = lambda *s: torch.rand(*s, generator=g, device="cuda", dtype=torch.float64) * 2 - 1   # noqa: E731
    A, J, u = rnd(Ni, Nj), rnd(two_rounds), rnd(two_rounds, Nj)
    n = 37
    (small,) = _launch(torch, Ni, Nj, n, J[:n], A, [u[:n]])
    assert bool(torch.isfinite(small).all())
    (mid,) = _launch(torch, Ni, Nj, 1003, J[:1003], A, [u[:1003]])
    (big,) = _launch(torch, Ni, Nj, two_rounds, J, A, [u])
    assert torch.equal(_bits(mid[:n]), _bits(small)) and torch.equal(_bits(big[:n]), _bits(small))
    J2, u2 = J.clone(), u.clone()
    J2[5000:5000 + n], u2[5000:5000 + n] = J[:n], u[:n]       # 5000 = 312 tiles + 8: other lanes, another tile boundary
    (moved,) = _launch(torch, Ni, Nj, two_rounds, J2, A, [u2])
    assert torch.equal(_bits(moved[5000:5000 + n]), _bits(small))
    assert torch.equal(_bits(moved[:5000]), _bits(big[:5000])) and torch.equal(_bits(moved[5000 + n:]), _bits(big[5000 + n:]))


# ---- 4. guard bands and placement ----------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", ((17, 5), (35, 56), (56, 35), (64, 64)), ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("E", (1, 17, 1003))
def test_guard_bands_and_placement(torch, shape, E):
    Ni, Nj = shape
    g = torch.Generator(device="cuda").manual_seed(3 * Ni + E)
    rnd = lambda *s: torch.rand(*s, generator=g, device="cuda", dtype=torch.float64) * 2 - 1   # noqa: E731
    A, J, us = rnd(Ni, Nj), rnd(E), [rnd(E, Nj), rnd(E, Nj)]
    for opT in (0, 1):
        stored = A.T.contiguous() if opT else A
        base = _launch(torch, Ni, Nj, E, J, stored, us, opT)
        assert all(bool(torch.isfinite(o).all()) for o in base)
        for shifts in ((1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 0), (0, 0, 0, 1), (1, 1, 1, 1)):
            outs = _launch(torch, Ni, Nj, E, J, stored, us, opT, shifts)
            for o, ref in zip(outs, base):
                assert bool(torch.isfinite(o).all()) and torch.equal(_bits(o), _bits(ref)), (shape, E, opT, shifts)
        (nj,) = _launch(torch, Ni, Nj, E, None, stored, us[:1], opT, (0, 1, 1, 1))
        (nj0,) = _launch(torch, Ni, Nj, E, None, stored, us[:1], opT)
        assert bool(torch.isfinite(nj).all()) and torch.equal(_bits(nj), _bits(nj0))


# ---- 5. a planted non-finite value reaches exactly its dependency set ----------------------------------------------

@pytest.mark.parametrize("shape", ((35, 56), (17, 5)), ids=lambda s: f"{s[0]}x{s[1]}")
def test_a_planted_non_finite_value_stays_in_its_dependency_set(torch, shape):
    Ni, Nj = shape
    E = 1003
    d = Exact(Ni, Nj, E, 1, 31 + Ni)
    subs = "e,ij,ej->ei"
    shapes = [(E,), (Ni, Nj), (E, Nj)]
    spots = {0: (E - 2,), 1: (Ni - 1, Nj - 2 if Nj > 1 else 0), 2: (E - 5, Nj - 1)}     # in the partial last tile, the padded fragments
    for operand, index in list(spots.items()) + [(2, (16, 0)), (1, (0, 0))]:
        dep = R.dependency_set(subs, shapes, operand, index)
        for planted in (math.nan, math.inf, -math.inf):
            host = [d.J.copy(), d.A.copy(), d.u[0].copy()]
            host[operand][index] = planted
            for opT in (0, 1):
                (out,) = _launch(torch, Ni, Nj, E, host[0], np.ascontiguousarray(host[1].T) if opT else host[1], [host[2]], opT)
                assert R.nonfinite_violations(out.cpu().numpy(), d.ref[True][0], dep, planted) == 0, (shape, operand, index, planted, opT)
            if operand:     # the forms without J
                dep2 = R.dependency_set("ij,ej->ei", shapes[1:], operand - 1, index)
                (out,) = _launch(torch, Ni, Nj, E, None, host[1], [host[2]])
                assert R.nonfinite_violations(out.cpu().numpy(), d.ref[False][0], dep2, planted) == 0, (shape, operand, index, planted)


# ---- 6. refusals on the device -------------------------------------------------------------------------------------

def test_an_unsupported_size_is_refused_before_anything_is_written(torch):
    E = 100
    for Ni, Nj in ((97, 4), (96, 41), (65, 64)):
        expr = _expr("ij,ej->ei", Ni, Nj, 1)
        arrays = {"A": torch.ones(Ni, Nj, dtype=torch.float64, device="cuda"), "u0": torch.ones(E, Nj, dtype=torch.float64, device="cuda")}
        out = torch.full((E, Ni), D.SENTINEL, dtype=torch.float64, device="cuda")
        count = lambda: torch.cuda.memory_stats().get("allocation.all.allocated", 0)   # noqa: E731  (allocations so far)
        before = count()
        with pytest.raises(NotImplementedError) as exc:
            f.evaluate(expr, 0, arrays, out_dict={expr.output_names[0]: out}, transform="element_operator", wait=True)
        assert ELEMENT_OPERATOR_RULE in str(exc.value)
        with pytest.raises(NotImplementedError):
            f.evaluate(expr, 0, arrays, transform="element_operator", wait=True)          # ... nor allocated
        assert count() == before
        with pytest.raises(NotImplementedError, match="size rule"):
            _hip.elemop(None, arrays["A"].data_ptr(), [arrays["u0"].data_ptr()], [out.data_ptr()], E, Ni, Nj)
        torch.cuda.synchronize()
        assert bool((out == D.SENTINEL).all())
        assert f.evaluate(expr, 0, arrays, transform="auto", wait=True)[expr.output_names[0]].shape == (E, Ni)   # other routes still run it


def test_aliasing_slices_and_other_dtypes_are_refused(torch):
    Ni, Nj, E = 35, 35, 64
    expr = _expr("ij,ej->ei", Ni, Nj, 1)
    A = torch.ones(Ni, Nj, dtype=torch.float64, device="cuda")
    u = torch.ones(E, Nj, dtype=torch.float64, device="cuda")
    name = expr.output_names[0]
    with pytest.raises(InvalidParameterError, match="shares memory"):
        f.evaluate(expr, 0, {"A": A, "u0": u}, out_dict={name: u}, transform="element_operator")
    base = torch.ones(2 * E, Nj, dtype=torch.float64, device="cuda")
    with pytest.raises(InvalidParameterError, match="C-contiguous"):
        f.evaluate(expr, 0, {"A": A, "u0": base[::2]}, transform="element_operator")
    big = torch.ones(E, 2 * Ni, dtype=torch.float64, device="cuda")
    with pytest.raises(InvalidParameterError, match="C-contiguous"):
        f.evaluate(expr, 0, {"A": A, "u0": u}, out_dict={name: big[:, :Ni]}, transform="element_operator")
    f32 = f.einsum("ij,ej->ei", f.array("A", (Ni, Nj), "float32"), f.array("u0", ("E", Nj), "float32"))
    with pytest.raises(NotImplementedError, match="element_operator"):
        f.evaluate(f32, 0, {"A": A.float(), "u0": u.float()}, transform="element_operator")
    for forced in ("kernel", "epilogue"):
        with pytest.raises(NotImplementedError):
            f.evaluate(expr, 0, {"A": A, "u0": u}, out_dict={name: torch.zeros(E, Ni, dtype=torch.float64, device="cuda")},
                       transform={"variant": "element_operator", "accumulate": forced}, alpha=2.0, beta=1.0)


# ---- 7. the launch record and the host features --------------------------------------------------------------------

def test_accumulation_through_axpby_is_the_fused_multiply_add(torch):
    Ni, Nj, E = 56, 35, 1003
    g = torch.Generator(device="cuda").manual_seed(9)
    rnd = lambda *s: torch.rand(*s, generator=g, device="cuda", dtype=torch.float64) * 2 - 1   # noqa: E731
    expr = _expr("e,ji,ej->ei", Ni, Nj, 2)
    arrays = {"J": rnd(E), "A": rnd(Nj, Ni), "u0": rnd(E, Nj), "u1": rnd(E, Nj)}
    plain = f.evaluate(expr, 0, arrays, transform="element_operator", wait=True)
    assert f.accumulate_route(expr, "element_operator") == "axpby"
    for alpha, beta in ((2.0, -0.5), (-0.25, 4.0), (0.5, 0.0)):
        old = {nm: rnd(E, Ni) for nm in expr.output_names}
        outs = {nm: t.clone() for nm, t in old.items()}
        f.evaluate(expr, 0, arrays, out_dict=outs, transform="element_operator", alpha=alpha, beta=beta, wait=True)
        for nm in expr.output_names:
            # powers of two: both products are exact, so the combine is one correctly rounded sum
            want = alpha * plain[nm] + beta * old[nm]
            assert torch.equal(_bits(outs[nm]), _bits(want)), (alpha, beta, nm)


def test_a_bound_stage_is_a_launch_of_its_own_and_replays_to_the_same_bits(torch):
    from dg import div, grad

    Np, E = 35, 1003
    g = torch.Generator(device="cuda").manual_seed(21)
    rnd = lambda *s: torch.rand(*s, generator=g, device="cuda", dtype=torch.float64) * 2 - 1   # noqa: E731
    geo = {"J": rnd(3, 3, E), "R": rnd(3, Np, Np)}
    proj = _expr("e,ij,ej->ei", 20, 35, 2)
    arrays = {"J": rnd(E), "A": rnd(20, 35), "u0": rnd(E, 35), "u1": rnd(E, 35)}
    eager = {nm: t.clone() for nm, t in f.evaluate(proj, 0, arrays, transform="element_operator", wait=True).items()}
    op = f.bind_operator([(proj, arrays)], 0, transform="element_operator")
    assert op.entry_points == ("fe_elemop_f64",), op.entry_points
    # beside stages that fuse: the element operator of a square size stays outside the fused launch
    sq = _expr("ij,ej->ei", Np, Np, 1)
    mixed = f.bind_operator([(sq, {"A": rnd(Np, Np), "u0": rnd(E, Np)})], 0, transform="element_operator")
    assert mixed.entry_points == ("fe_elemop_f64",)
    fused = f.bind_operator([(div(), {**geo, "u": rnd(3, E, Np)}), (grad(), {**geo, "u": rnd(E, Np)})], 0)
    assert len(fused.entry_points) == 1          # (untouched: div + grad still share a launch)
    op.launch()
    torch.cuda.synchronize()
    info = _hip.last_launch_info()
    assert info.get("element_operator") and info["tiles"] == -(-E // TILE) and info["bodies"] == 1, info
    outs = op.outputs[0]
    assert all(torch.equal(_bits(outs[nm]), _bits(eager[nm])) for nm in proj.output_names)
    side = torch.cuda.Stream(priority=-1)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        op.launch(int(torch.cuda.current_stream().cuda_stream))
    for nm in proj.output_names:
        outs[nm].fill_(math.nan)
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(_bits(outs[nm]), _bits(eager[nm])) for nm in proj.output_names)
    graph.reset()


def test_a_queue_on_another_stream_matches_the_default_stream(torch):
    Ni, Nj, E = 35, 56, 1003
    g = torch.Generator(device="cuda").manual_seed(4)
    rnd = lambda *s: torch.rand(*s, generator=g, device="cuda", dtype=torch.float64) * 2 - 1   # noqa: E731
    expr = _expr("ij,ej->ei", Ni, Nj, 1)
    arrays = {"A": rnd(Ni, Nj), "u0": rnd(E, Nj)}
    name = expr.output_names[0]
    here = f.evaluate(expr, 0, arrays, transform="element_operator", wait=True)[name]
    torch.cuda.synchronize()
    side = torch.cuda.Stream(priority=-1)
    q = f.DeviceQueue(0, side)
    there = f.evaluate(expr, q, arrays, transform="element_operator", wait=True)[name]
    assert torch.equal(_bits(there), _bits(here))
    f.validate_batched_einsum_transform(expr, q, "element_operator")
    assert f.timeit_details(expr, transform="element_operator", cq=q, long_dim_length=1003, min_rounds=5, min_secs=0.0).rounds >= 5


# ---- 8. speed: one floor -------------------------------------------------------------------------------------------

#: halfway between 1.0 and the ratio tools/bench_element_operator.py measured at this shape and size on the MI355X
#: (a / c = 3.368 [3.358, 3.395] at (56, 35), b = 1, E = 2e5, no J): the convention of section 3m
SPEED_FLOOR = 2.184


def test_faster_than_the_route_auto_takes(torch):
    from feinsum_amd.measure import _bind, launch_kind

    Ni, Nj, E = 56, 35, 200_000
    g = torch.Generator(device="cuda").manual_seed(1)
    rnd = lambda *s: torch.rand(*s, generator=g, device="cuda", dtype=torch.float64) * 2 - 1   # noqa: E731
    expr = _expr("ij,ej->ei", Ni, Nj, 1)
    arrays = {"A": rnd(Ni, Nj), "u0": rnd(E, Nj)}
    outs = {expr.output_names[0]: torch.empty(E, Ni, dtype=torch.float64, device="cuda")}
    q = f.DeviceQueue(0)
    assert launch_kind(expr, "auto", {"E": E}) == "contraction"
    bound = {form: _bind(expr, q, arrays, outs, transform)[1] for form, transform in (("a", "auto"), ("c", "element_operator"))}
    times = {"a": [], "c": []}
    for form in bound:
        bound[form].time_batch(10, q.stream_ptr)           # warm-up
    for _ in range(5):                                     # the forms take turns
        for form in ("a", "c"):
            times[form].append(bound[form].time_batch(20, q.stream_ptr) / 20)
    a, c = (float(np.median(times[form])) for form in ("a", "c"))
    print(f"a (auto: contraction) {a * 1e6:.1f} us, c (element_operator) {c * 1e6:.1f} us, a / c = {a / c:.3f}, floor {SPEED_FLOOR}")
    # measured a / c = 3.368 [3.358, 3.395]; the floor is (1 + 3.368) / 2
    assert a / c > SPEED_FLOOR, (a, c, a / c)
