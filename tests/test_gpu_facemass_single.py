"""Face-mass of ONE field (b = 1) on the matrix cores: every (Np, nf, Nfp) the launcher knows, both J
layouts, the four operator layouts.

- a forced ``transform="mfma"`` returns (it raised NotImplementedError before) and leaves a launch record;
- exact data on a grid of 16 waves at the element counts where a ring of two slabs and one J buffer can go wrong: one tile, a
  remainder beside one tile, every wave walking 1, 2, 3 and 5 tiles, one wave a tile ahead of the rest -- every output bitwise
  the int64 einsum, outputs between sentinel bands, inputs between NaN bands, all compared bitwise after the launch;
- signed data: the result of a field is bitwise what it is as a member of a launch of two and of three fields;
- the dynamic walk: set, bitwise the static walk and the exact reference, its counters clean, two streams alike;
- a planted NaN / +Inf / -Inf stays in its dependency set (triangles: K = 3 Nfp is padded to a multiple of 4);
- every operand 8 bytes past a 256-byte boundary: bitwise the aligned launch;
- "tiled" and "generic" still run one field and agree within the gamma(n, u) bound; a bound operator with a lift of one field
  runs it as a launch of its own on the new kernel; a captured graph replays the eager bits."""

import math
import sys
from pathlib import Path

import numpy as np
import pytest

import feinsum_amd as f
from feinsum_amd import _hip
from feinsum_amd.family import FM_J_FE, FM_R_IFJ, FM_R_T
from oracle import einsum_ref as R

sys.path.insert(0, str(Path(__file__).resolve().parents[1] / "tools"))
import fuzz_dg as D  # noqa: E402

pytestmark = pytest.mark.gpu

#: (Np, nf, Nfp, M): tetrahedra p = 1..5, triangles p = 1..5; a wave tile is 16 M elements
SHAPES = ((4, 4, 3, 4), (10, 4, 6, 2), (20, 4, 10, 1), (35, 4, 15, 1), (56, 4, 21, 1),
          (3, 3, 2, 8), (6, 3, 3, 6), (10, 3, 4, 5), (15, 3, 5, 4), (21, 3, 6, 3))
IDS = [f"Np{s[0]}nf{s[1]}" for s in SHAPES]
REGISTER_SHAPES = tuple(s for s in SHAPES if s[0] != 56)       # the kernels with a dynamic walk
J_LAYOUTS = ("ef", "fe")
R_LAYOUTS = {"fij": 0, "ifj": FM_R_IFJ, "fji": FM_R_T, "jfi": FM_R_IFJ | FM_R_T}
#: axes of the operator stored [f][i][j] in each layout
R_AXES = {"fij": (0, 1, 2), "ifj": (1, 0, 2), "fji": (0, 2, 1), "jfi": (2, 0, 1)}
W = 16    # waves of a grid sized for two CUs: two blocks of four waves per CU, or one of eight (p = 5)


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
def own_streams(torch):
    """Two streams from torch's high-priority pool (tests/test_gpu_reduction.py: the other modules take theirs from the
    default-priority pool, round robin, so the streams they get stay what they were without this module); the ticket-counter
    groups their launches took go back to the library when the module ends."""
    streams = [torch.cuda.Stream(priority=-1) for _ in range(2)]
    yield streams
    torch.cuda.synchronize()
    for s in streams:
        _hip.stream_retired(int(s.cuda_stream))


def _flags(jl, rl):
    return (FM_J_FE if jl == "fe" else 0) | R_LAYOUTS[rl]


class Exact:
    """Exact data of one shape for up to *E* elements: integer mantissas whose every partial sum fits 53 bits, the int64
    einsum of all of them computed once; a smaller launch takes the leading elements."""

    def __init__(self, shape, E, seed):
        Np, nf, Nfp, _ = shape
        rng = np.random.default_rng(seed)
        bits = R.exact_bits(3, [np.float64] * 3, nf * Nfp, 53, rng)
        (self.mJ, self.mR, self.mv), (self.J, self.R, self.v) = R.exact_operands(
            [(E, nf), (nf, Np, Nfp), (nf, E, Nfp)], [np.float64] * 3, bits, [0, 0, 0], rng)
        self.ref = R.int_reference("ef,fij,fej->ei", [self.mJ, self.mR, self.mv], 0, np.float64, 53)
        self.shape, self.E = shape, E

    def host(self, E, jl, rl):
        J = self.J[:E] if jl == "ef" else np.ascontiguousarray(self.J[:E].T)
        return J, np.ascontiguousarray(self.R.transpose(R_AXES[rl])), np.ascontiguousarray(self.v[:, :E])


def _launch(torch, shape, E, jl, rl, J, Rm, vs, shifts=(0, 0, 0, 0), variant="mfma", stream=0):
    """One face-mass call on embedded arrays (tools/fuzz_dg.py: inputs between NaN bands, outputs between sentinel bands);
    returns the outputs after checking that nothing but them changed."""
    Np, nf, Nfp, _ = shape
    as_t = lambda a: a if torch.is_tensor(a) else torch.from_numpy(a)   # noqa: E731
    eJ = D.embed(torch, tuple(J.shape), torch.float64, shifts[0], "in", as_t(J))
    eR = D.embed(torch, tuple(Rm.shape), torch.float64, shifts[1], "in", as_t(Rm))
    ev = [D.embed(torch, tuple(v.shape), torch.float64, shifts[2], "in", as_t(v)) for v in vs]
    eo = [D.embed(torch, (E, Np), torch.float64, shifts[3], "out") for _ in vs]
    snaps = [e.snapshot() for e in (eJ, eR, *ev)]
    torch.cuda.synchronize()
    _hip.facemass(eJ.view.data_ptr(), eR.view.data_ptr(), [e.view.data_ptr() for e in ev], [e.view.data_ptr() for e in eo],
                  E, Np, nf, Nfp, _flags(jl, rl), variant, stream)
    torch.cuda.synchronize()
    for e, s in zip((eJ, eR, *ev), snaps):
        assert e.unchanged(s), ("an input changed", shape, E, jl, rl, e.first_change(s))
    for e in eo:
        assert e.guards_intact(), ("a store outside the output", shape, E, jl, rl)
    return [e.view.clone() for e in eo]


def _bits(t):
    import torch

    return t.contiguous().view(torch.int64)


# ---- 1. fails without the feature ----------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_a_forced_mfma_launch_of_one_field_returns(torch, shape):
    from dg import face_mass

    Np, nf, Nfp, M = shape
    E = 3 * 16 * M + 5
    d = Exact(shape, E, 100 + Np)
    expr = face_mass(1, Np, nf, Nfp)
    dev = {"J": torch.from_numpy(d.J).cuda(), "R": torch.from_numpy(d.R).cuda(), "v0": torch.from_numpy(d.v).cuda()}
    for transform in ("mfma", "auto"):
        out = f.evaluate(expr, 0, dev, transform=transform, wait=True)[expr.output_names[0]]
        info = _hip.last_launch_info()
        assert info.get("valid") and info["tiles"] == 3 and info["bodies"] == 1, (transform, info)
        assert R.differing_entries(out.cpu().numpy(), d.ref) == 0, transform


# ---- 2. exact data, static walk, the sizes where the ring can go wrong ---------------------------------------------

def _ring_sizes(tel):
    return [tel, tel + 1, 2 * tel - 1] + [tel * W * k + 7 for k in (1, 2, 3, 5)] + [tel * (3 * W + 1)]


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_exact_data_on_sixteen_waves(torch, shape):
    Np, nf, Nfp, M = shape
    tel = 16 * M
    sizes = _ring_sizes(tel)
    d = Exact(shape, max(sizes), 200 + Np)
    before = _hip.set_cu_limit(2)
    try:
        for E in sizes:
            for jl in J_LAYOUTS:
                for rl in R_LAYOUTS:
                    J, Rm, v = d.host(E, jl, rl)
                    (out,) = _launch(torch, shape, E, jl, rl, J, Rm, [v])
                    info = _hip.last_launch_info()
                    assert info.get("valid") and not info["dynamic_walk"] and info["tiles"] == E // tel, info
                    waves = info["blocks"] * info["waves_per_block"]
                    assert waves <= W and (waves == W or E // tel < W), info
                    bad = R.differing_entries(out.cpu().numpy(), d.ref[:E])
                    assert bad == 0, (shape, E, jl, rl, bad)
    finally:
        _hip.set_cu_limit(before)


# ---- 3. bitwise against the launches of two and of three fields ----------------------------------------------------

@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_bitwise_the_field_of_a_launch_of_two_and_of_three(torch, shape):
    Np, nf, Nfp, M = shape
    E = 16 * M * W * 3 + 7
    g = torch.Generator(device="cuda").manual_seed(300 + Np)
    rnd = lambda *s: torch.rand(*s, generator=g, device="cuda", dtype=torch.float64) * 2 - 1   # noqa: E731
    before = _hip.set_cu_limit(2)
    try:
        for jl, rl in (("ef", "fij"), ("fe", "ifj"), ("ef", "jfi"), ("fe", "fji")):
            J = rnd(E, nf) if jl == "ef" else rnd(nf, E)
            Rm = rnd(*[(nf, Np, Nfp)[a] for a in R_AXES[rl]])
            v, w, x = rnd(nf, E, Nfp), rnd(nf, E, Nfp), rnd(nf, E, Nfp)
            (alone,) = _launch(torch, shape, E, jl, rl, J, Rm, [v])
            assert bool(torch.isfinite(alone).all())
            for fields in ([v, w], [w, v], [v, w, x], [w, v, x], [w, x, v]):
                outs = _launch(torch, shape, E, jl, rl, J, Rm, fields)
                k = next(k for k, t in enumerate(fields) if t is v)
                assert torch.equal(_bits(outs[k]), _bits(alone)), (shape, jl, rl, len(fields), k)
    finally:
        _hip.set_cu_limit(before)


# ---- 4. the dynamic walk -------------------------------------------------------------------------------------------

def _device_exact(torch, shape, E, seed):
    """Exact data of a large launch and its reference: the whole-array int64 einsum (numpy, on the host)."""
    d = Exact(shape, E, seed)
    return d, torch.from_numpy(d.ref).cuda()


@pytest.mark.parametrize("shape", REGISTER_SHAPES, ids=[i for i, s in zip(IDS, SHAPES) if s[0] != 56])
def test_the_dynamic_walk(torch, own_streams, shape):
    Np, nf, Nfp, M = shape
    tel = 16 * M
    E = tel * 512 * 4 + 3
    d, ref = _device_exact(torch, shape, E, 400 + Np)
    jl, rl = ("fe", "ifj") if Np % 2 else ("ef", "fij")
    J, Rm, v = d.host(E, jl, rl)
    cu, mr = _hip.set_cu_limit(64), _hip.set_tail_min_rounds(2)
    try:
        (dyn,) = _launch(torch, shape, E, jl, rl, J, Rm, [v])
        info = _hip.last_launch_info()
        assert info.get("valid") and info["dynamic_walk"], info
        assert info["blocks"] == 128 and info["static_tiles"] == 2 * 512 and info["tiles"] == 4 * 512, info
        assert _hip.tail_check()["dirty_words"] == 0
        tr = _hip.set_tail_rounds(-1)
        try:
            (static,) = _launch(torch, shape, E, jl, rl, J, Rm, [v])
            assert not _hip.last_launch_info()["dynamic_walk"]
        finally:
            _hip.set_tail_rounds(tr)
        assert torch.equal(_bits(dyn), _bits(static))
        assert R.differing_entries(dyn, ref) == 0
        # two launches back to back on two streams
        dJ, dR, dv = (torch.from_numpy(a).cuda() for a in (J, Rm, v))
        outs = [torch.full((E, Np), math.nan, dtype=torch.float64, device="cuda") for _ in range(2)]
        torch.cuda.synchronize()
        for s, o in zip(own_streams, outs):
            _hip.facemass(dJ.data_ptr(), dR.data_ptr(), [dv.data_ptr()], [o.data_ptr()], E, Np, nf, Nfp, _flags(jl, rl), "mfma",
                          s.cuda_stream)
            assert _hip.last_launch_info()["dynamic_walk"]
        torch.cuda.synchronize()
        assert torch.equal(_bits(outs[0]), _bits(dyn)) and torch.equal(_bits(outs[1]), _bits(dyn))
        assert _hip.tail_check()["dirty_words"] == 0
    finally:
        _hip.set_cu_limit(cu)
        _hip.set_tail_min_rounds(mr)


def test_the_dynamic_walk_on_the_devices_own_grid(torch):
    shape, E = SHAPES[3], 170_003
    d, ref = _device_exact(torch, shape, E, 435)
    J, Rm, v = d.host(E, "ef", "fij")
    (out,) = _launch(torch, shape, E, "ef", "fij", J, Rm, [v], variant="auto")
    info = _hip.last_launch_info()
    assert info.get("valid") and info["tiles"] == E // 16, info
    rounds = info["tiles"] // (info["blocks"] * info["waves_per_block"])
    assert bool(info["dynamic_walk"]) == (rounds >= 5 and info["blocks"] >= 128), info   # (the rule of single launches)
    assert R.differing_entries(out, ref) == 0
    assert _hip.tail_check()["dirty_words"] == 0


# ---- 5. non-finite values stay in their dependency sets ------------------------------------------------------------

@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_planted_non_finite_values_stay_in_their_dependency_sets(torch, shape):
    Np, nf, Nfp, M = shape
    tel = 16 * M
    E = 3 * tel + 5
    d = Exact(shape, E, 500 + Np)
    shapes = [(E, nf), (nf, Np, Nfp), (nf, E, Nfp)]
    e1, e2 = tel + 3, 3 * tel - 1          # in the second and in the third tile
    # (f, j) = (0, 0) is what the padded k-steps of the triangles read again
    sites = [(2, (0, e1, 0)), (2, (nf - 1, e2, Nfp - 1)), (0, (e1, 0)), (0, (e2, nf - 1)), (1, (nf - 1, Np - 1, Nfp // 2))]
    for jl, rl in (("ef", "fij"), ("fe", "jfi")):
        for operand, index in sites:
            dep = R.dependency_set("ef,fij,fej->ei", shapes, operand, index)
            for value in (math.nan, math.inf, -math.inf):
                J, Rm, v = (a.copy() for a in (d.J, d.R, d.v))
                (J, Rm, v)[operand][index] = value
                Jh = J if jl == "ef" else np.ascontiguousarray(J.T)
                Rh = np.ascontiguousarray(Rm.transpose(R_AXES[rl]))
                (out,) = _launch(torch, shape, E, jl, rl, Jh, Rh, [v])
                bad = R.nonfinite_violations(out.cpu().numpy(), d.ref, dep, value)
                assert bad == 0, (shape, jl, rl, operand, index, value, bad)


# ---- 6. placement --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", (SHAPES[3], SHAPES[1], SHAPES[7]), ids=(IDS[3], IDS[1], IDS[7]))
def test_operands_eight_bytes_past_a_boundary(torch, shape):
    Np, nf, Nfp, M = shape
    E = 16 * M * W * 3 + 7
    g = torch.Generator(device="cuda").manual_seed(600 + Np)
    rnd = lambda *s: torch.rand(*s, generator=g, device="cuda", dtype=torch.float64) * 2 - 1   # noqa: E731
    before = _hip.set_cu_limit(2)
    try:
        for jl, rl in (("ef", "fij"), ("fe", "ifj")):
            J = rnd(E, nf) if jl == "ef" else rnd(nf, E)
            Rm = rnd(*[(nf, Np, Nfp)[a] for a in R_AXES[rl]])
            v = rnd(nf, E, Nfp)
            (aligned,) = _launch(torch, shape, E, jl, rl, J, Rm, [v])
            for shifts in ((1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 0), (0, 0, 0, 1), (1, 1, 1, 1)):
                (out,) = _launch(torch, shape, E, jl, rl, J, Rm, [v], shifts)
                assert torch.equal(_bits(out), _bits(aligned)), (shape, jl, rl, shifts)
    finally:
        _hip.set_cu_limit(before)


# ---- 7. the variants agree; bound operators; graphs ----------------------------------------------------------------

@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_tiled_and_generic_still_run_one_field_and_agree(torch, shape):
    from dg import face_mass

    Np, nf, Nfp, M = shape
    E = 5 * 16 * M + 3
    rng = np.random.default_rng(700 + Np)
    host = {"J": rng.uniform(-1, 1, (E, nf)), "R": rng.uniform(-1, 1, (nf, Np, Nfp)), "v0": rng.uniform(-1, 1, (nf, E, Nfp))}
    ref, absref = R.bounded_reference("ef,fij,fej->ei", [host["J"], host["R"], host["v0"]])
    n = R.bound_terms("ef,fij,fej->ei", {"e": E, "f": nf, "i": Np, "j": Nfp}, 3)
    expr = face_mass(1, Np, nf, Nfp)
    dev = {k: torch.from_numpy(a).cuda() for k, a in host.items()}
    for transform in ("mfma", "tiled", "generic"):
        out = f.evaluate(expr, 0, dev, transform=transform, wait=True)[expr.output_names[0]]
        assert bool(_hip.last_launch_info().get("valid")) == (transform == "mfma"), transform
        assert R.bound_violations(out.cpu().numpy(), ref, absref, n, R.U64) == 0, (shape, transform)


def test_a_bound_operator_runs_a_lift_of_one_field_on_its_own(torch, own_streams):
    from dg import div, face_mass, grad

    Np, nf, Nfp = 35, 4, 15
    E = 16 * 40 + 9
    g = torch.Generator(device="cuda").manual_seed(77)
    rnd = lambda *s: torch.rand(*s, generator=g, device="cuda", dtype=torch.float64) * 2 - 1   # noqa: E731
    geo = {"J": rnd(3, 3, E), "R": rnd(3, Np, Np)}
    lift_arrays = {"J": rnd(E, nf), "R": rnd(nf, Np, Nfp), "v0": rnd(nf, E, Nfp)}
    lift = face_mass(1, Np, nf, Nfp)
    eager = f.evaluate(lift, 0, lift_arrays, transform="mfma", wait=True)[lift.output_names[0]].clone()
    op = f.bind_operator([(div(), {**geo, "u": rnd(3, E, Np)}), (grad(), {**geo, "u": rnd(E, Np)}), (lift, lift_arrays)], 0)
    assert len(op.entry_points) == 2 and op.entry_points[-1] == "fe_facemass", op.entry_points   # div + grad fused, the lift alone
    op.launch()
    info = _hip.last_launch_info()
    torch.cuda.synchronize()
    assert info.get("valid") and info["bodies"] == 1 and info["tiles"] == E // 16, info
    out = op.outputs[2][lift.output_names[0]]
    assert torch.equal(_bits(out), _bits(eager))
    # one capture and one replay: as BoundOperator.capture() does it, but on a stream of this module (capture() takes one from
    # the default-priority pool)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=own_streams[0]):
        s = int(torch.cuda.current_stream().cuda_stream)
        cid = _hip.capture_id(s)
        op.launch(s)
    out.fill_(math.nan)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(_bits(out), _bits(eager))
    assert _hip.tail_check()["dirty_words"] == 0
    graph.reset()
    if cid:
        _hip.graph_retired(cid)       # (these launches walk statically and own no counters; should they ever, give them back)
