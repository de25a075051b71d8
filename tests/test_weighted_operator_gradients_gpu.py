"""Differentiating the element operators on the device (``evaluate_differentiable(element_gradients="kernel")``, the weight
gradient fe_weightgrad_f64 'iq,qj,ej,ei->eq'):

- exact data at every size where the kernel takes another path -- row tiles and k steps of both chains with and without
  padding, one and several tiles, a partial last tile, fewer elements than a tile -- all four storage templates, one and three
  fields, through the C entry point and through ``evaluate_differentiable``: bitwise the int64 einsum summed over the rows;
- signed random data within gamma(n, u) absref; results that do not depend on where an element sits in its array;
- every array between guard bands, 0 and 8 bytes past a 256-byte boundary; a planted NaN / Inf stays in its dependency set;
- the whole backward pass: what runs where (``autograd.launch_counts``), bitwise against the kernels called by hand, within
  the bound of every adjoint einsum; the fallbacks; a side-stream queue; ``"auto"`` unchanged; one speed floor.

(The file sorts behind tests/test_placement.py on purpose: that test's search for a second class of physical memory depends on
what the process allocated before it, and these tests leave all that as it was.)"""

import math
import sys
from collections import Counter
from pathlib import Path

import numpy as np
import pytest

import feinsum_amd as f
from feinsum_amd import _hip, autograd
from feinsum_amd.autograd import adjoint_terms, output_grad_name
from feinsum_amd.family import (WO_A_T, WO_P_T, weighted_element_operator_supported, weighted_weight_adjoint_lds_bytes,
                                weighted_weight_adjoint_supported)
from oracle import einsum_ref as R
from test_gpu_weighted_element_operator import TEMPLATES, _bits, _expr, _id, _rnd

sys.path.insert(0, str(Path(__file__).resolve().parents[1] / "tools"))
import fuzz_dg as D  # noqa: E402

pytestmark = pytest.mark.gpu

F64 = np.float64
FWD = "weighted_element_operator"
WSUBS = "iq,qj,ej,ei->eq"          # the weight gradient of one row, P and A as the forward's first template stores them
MUST_HAVE = ((35, 56, 35), (20, 35, 20), (10, 20, 10), (4, 10, 4), (20, 56, 35), (35, 56, 20))
_ok = weighted_weight_adjoint_supported
_lds = weighted_weight_adjoint_lds_bytes
#: per RQ = ceil(Nq / 16) the shape of the rule that needs the most LDS
RQ_MAX = tuple(max(((ni, nq, nj) for ni in range(1, 49) for nq in range(16 * rq - 15, 16 * rq + 1) for nj in range(1, 49) if _ok(ni, nq, nj)),
                   key=lambda s: (_lds(*s), s)) for rq in (1, 2, 3, 4))
LARGEST = (48, 63, 48)
SHAPES = tuple(s for s in dict.fromkeys(
    [(ni, nq, nj) for ni in (1, 16, 17, 35) for nq in (1, 4, 5, 16, 17, 56, 64) for nj in (1, 4, 5, 35)] + list(MUST_HAVE)
    + list(RQ_MAX) + [LARGEST]) if _ok(*s))
SIZES = (1, 15, 16, 17, 63, 65, 1003)
TILE = 16     # elements of a wave tile


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
    assert RQ_MAX == ((48, 16, 48), (48, 32, 48), (48, 48, 48), (48, 63, 48)), RQ_MAX
    assert [_lds(*s) for s in RQ_MAX] == [36928, 49216, 61952, 81408]
    assert len(SHAPES) == 4 * 7 * 4 + len(MUST_HAVE) + len(RQ_MAX) - 1      # nothing was filtered out; (35, 56, 35) is in two lists
    assert all(s in SHAPES for s in MUST_HAVE) and LARGEST in SHAPES


class Exact:
    """Exact data of one shape for up to *E* elements and *b* fields: integer mantissas of four operands whose every partial
    sum of b Ni Nj terms fits 53 bits (``bits_fit``), the int64 einsum of every row computed once; a smaller launch takes the
    leading elements (an element's result depends on its own rows only) and the leading rows."""

    def __init__(self, shape, E, b, seed):
        Ni, Nq, Nj = shape
        rng = np.random.default_rng(seed)
        bits = R.exact_bits(4, [F64] * 4, b * Ni * Nj, 53, rng)
        assert R.bits_fit(bits, b * Ni * Nj, 53)
        mants, arrays = R.exact_operands([(Ni, Nq), (Nq, Nj)] + [(E, Nj)] * b + [(E, Ni)] * b, [F64] * (2 + 2 * b),
                                         bits[:2] + [bits[2]] * b + [bits[3]] * b, [0] * (2 + 2 * b), rng)
        self.mP, self.mA, self.mu, self.mg = mants[0], mants[1], mants[2:2 + b], mants[2 + b:]
        self.P, self.A, self.u, self.g = arrays[0], arrays[1], arrays[2:2 + b], arrays[2 + b:]
        self.rows = [R.int_reference(WSUBS, [self.mP, self.mA, mu, mg], 0, F64, 53) for mu, mg in zip(self.mu, self.mg)]
        self.shape, self.E, self.b = shape, E, b

    def ref(self, b):
        """The rows summed: integers below 2^53 in every partial sum, so the float64 sum is the int64 sum."""
        total = self.rows[0].copy()
        for row in self.rows[1:b]:
            total += row
        return total

    def stored(self, flags):
        return (np.ascontiguousarray(self.P.T) if flags & WO_P_T else self.P, np.ascontiguousarray(self.A.T) if flags & WO_A_T else self.A)


def _launch(torch, shape, E, P, A, us, gs, flags=0, shifts=(0, 0, 0, 0, 0), stream=0):
    """One fe_weightgrad_f64 call on embedded arrays (tools/fuzz_dg.py: inputs between NaN bands, the output between sentinel
    bands, *shifts* doubles past a 256-byte boundary: P, A, every u, every g, dW); returns dW after checking that the inputs
    are bitwise what they were, the bands intact."""
    Ni, Nq, Nj = shape
    as_t = lambda a: a if torch.is_tensor(a) else torch.from_numpy(a)   # noqa: E731
    eP = D.embed(torch, tuple(P.shape), torch.float64, shifts[0], "in", as_t(P))
    eA = D.embed(torch, tuple(A.shape), torch.float64, shifts[1], "in", as_t(A))
    eu = [D.embed(torch, (E, Nj), torch.float64, shifts[2], "in", as_t(u)) for u in us]
    eg = [D.embed(torch, (E, Ni), torch.float64, shifts[3], "in", as_t(g)) for g in gs]
    eo = D.embed(torch, (E, Nq), torch.float64, shifts[4], "out")
    ins = [eP, eA, *eu, *eg]
    snaps = [e.snapshot() for e in ins]
    torch.cuda.synchronize()
    _hip.weightgrad(eP.view.data_ptr(), eA.view.data_ptr(), [e.view.data_ptr() for e in eu], [e.view.data_ptr() for e in eg],
                    eo.view.data_ptr(), E, Ni, Nq, Nj, flags, stream)
    torch.cuda.synchronize()
    for e, s in zip(ins, snaps):
        assert e.unchanged(s), ("an input changed", shape, E, e.first_change(s))
    assert eo.guards_intact(), ("a store outside the output", shape, E)
    return eo.view.clone()


def _through_autograd(torch, subs, shape, E, P, A, us, gs, q=0, **requires):
    """dW (and with ``u=True`` every du_k) of the forward einsum *subs* through ``evaluate_differentiable``: the forward on the
    kernel, ``element_gradients="kernel"``.  Returns (outputs, W.grad, [u_k.grad])."""
    Ni, Nq, Nj = shape
    expr = _expr(subs, shape, len(us))
    dev = lambda a: (a if torch.is_tensor(a) else torch.from_numpy(a).cuda()).clone()   # noqa: E731
    W = requires.get("W_values")
    W = torch.ones(E, Nq, dtype=torch.float64, device="cuda") if W is None else dev(W)
    W.requires_grad_(requires.get("W", True))
    fields = [dev(u).requires_grad_(requires.get("u", False)) for u in us]
    arrays = {"P": dev(P), "A": dev(A), "W": W, **{f"u{k}": t for k, t in enumerate(fields)}}
    outs = f.evaluate_differentiable(expr, q, arrays, transform=FWD, element_gradients="kernel")
    torch.autograd.backward([outs[nm] for nm in expr.output_names], [dev(g) for g in gs])
    torch.cuda.synchronize()
    return outs, W.grad, [t.grad for t in fields]


# ---- 1. exact data -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_exact_data_bitwise_the_int64_einsum(torch, shape):
    """Every size x every storage template; the field count (1, 3) and the path (the C entry point, the backward pass of
    ``evaluate_differentiable``) alternate over them so that every template meets both counts on both paths in every shape."""
    d = Exact(shape, max(SIZES), 3, 1000 * shape[0] + 100 * shape[1] + shape[2])
    for n, E in enumerate(SIZES):
        for t, (subs, flags) in enumerate(TEMPLATES):
            b = (1, 3)[(n + t) % 2]
            direct = ((n + t) // 2) % 2 == 1
            P, A = d.stored(flags)
            us, gs = [u[:E] for u in d.u[:b]], [g[:E] for g in d.g[:b]]
            autograd.launch_counts.clear()
            if direct:
                dW = _launch(torch, shape, E, P, A, us, gs, flags)
                info = _hip.last_launch_info()
                assert info.get("weighted_weight_adjoint") and not info.get(FWD) and not info.get("element_operator"), info
                assert info["tiles"] == -(-E // TILE) and not info["dynamic_walk"], info
            else:   # (the launch record is per thread, and the backward pass runs on autograd's: the route is what is counted)
                _, dW, _ = _through_autograd(torch, subs, shape, E, P, A, us, gs)
                assert autograd.launch_counts == Counter({"weighted_w": 1}), autograd.launch_counts
            bad = R.differing_entries(dW.cpu().numpy(), d.ref(b)[:E])
            assert bad == 0, (shape, E, subs, b, "direct" if direct else "autograd", bad)


# ---- 2. signed random data within the project's bound --------------------------------------------------------------

@pytest.mark.parametrize("shape", MUST_HAVE + RQ_MAX + ((17, 5, 5), (1, 1, 1), (13, 17, 13), (45, 64, 33)), ids=_id)
def test_signed_random_data_within_the_bound(torch, shape):
    """n = b (3 + Ni Nj): the project's count for a four-operand einsum is 3 + Ni Nj per row (``bound_terms``), the kernel's
    own chain has Ni + Nj + 1 roundings per row (the two sums, the fused multiply-add), which never exceeds it, and b rows
    are summed: the bound is derived, not measured.  absref is the sum of the rows' absolute einsums."""
    Ni, Nq, Nj = shape
    E = 1003
    rng = np.random.default_rng(5 * Ni + 3 * Nq + Nj)
    P, A = rng.random((Ni, Nq)) * 2 - 1, rng.random((Nq, Nj)) * 2 - 1
    us, gs = [rng.random((E, Nj)) * 2 - 1 for _ in range(3)], [rng.random((E, Ni)) * 2 - 1 for _ in range(3)]
    rows = [R.bounded_reference(WSUBS, [P, A, u, g]) for u, g in zip(us, gs)]
    per_row = R.bound_terms(WSUBS, {"e": E, "i": Ni, "q": Nq, "j": Nj}, 4)
    assert per_row == 3 + Ni * Nj >= Ni + Nj + 1
    for b in (1, 3):
        ref, absref = sum(r for r, _ in rows[:b]), sum(a for _, a in rows[:b])
        for subs, flags in TEMPLATES:
            dW = _launch(torch, shape, E, np.ascontiguousarray(P.T) if flags & WO_P_T else P,
                         np.ascontiguousarray(A.T) if flags & WO_A_T else A, us[:b], gs[:b], flags)
            assert R.bound_violations(dW.cpu().numpy(), ref, absref, b * per_row, R.U64) == 0, (shape, subs, b)


# ---- 3. an element's result does not depend on where it sits -------------------------------------------------------

@pytest.mark.parametrize("shape", ((35, 56, 35), (17, 5, 5), (20, 56, 35)), ids=_id)
def test_position_independence(torch, two_rounds, shape):
    Ni, Nq, Nj = shape
    rnd = _rnd(torch, 11 + Ni)
    P, A, u, g = rnd(Ni, Nq), rnd(Nq, Nj), rnd(two_rounds, Nj), rnd(two_rounds, Ni)
    n = 37
    small = _launch(torch, shape, n, P, A, [u[:n]], [g[:n]])
    assert bool(torch.isfinite(small).all())
    mid = _launch(torch, shape, 1003, P, A, [u[:1003]], [g[:1003]])
    big = _launch(torch, shape, two_rounds, P, A, [u], [g])
    info = _hip.last_launch_info()
    assert info["tiles"] == -(-two_rounds // TILE) and info["blocks"] * info["waves_per_block"] * 2 < info["tiles"], info
    assert torch.equal(_bits(mid[:n]), _bits(small)) and torch.equal(_bits(big[:n]), _bits(small))
    u2, g2 = u.clone(), g.clone()
    u2[5000:5000 + n], g2[5000:5000 + n] = u[:n], g[:n]       # 5000 = 312 tiles + 8: other lanes, another tile boundary
    moved = _launch(torch, shape, two_rounds, P, A, [u2], [g2])
    assert torch.equal(_bits(moved[5000:5000 + n]), _bits(small)) and torch.equal(_bits(moved[:n]), _bits(small))
    assert torch.equal(_bits(moved[:5000]), _bits(big[:5000])) and torch.equal(_bits(moved[5000 + n:]), _bits(big[5000 + n:]))
    # ... and as the second field of its tile: a first field of zeros adds +0 to every entry
    zu, zg = torch.zeros_like(u2), torch.zeros_like(g2)
    second = _launch(torch, shape, two_rounds, P, A, [zu, u2], [zg, g2])
    assert torch.equal(_bits(second), _bits(moved))


# ---- 4. guard bands and placement ----------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", ((17, 5, 5), (35, 56, 35), (4, 10, 4), LARGEST), ids=_id)
@pytest.mark.parametrize("E", (1, 17, 1003))
def test_guard_bands_and_placement(torch, shape, E):
    Ni, Nq, Nj = shape
    rnd = _rnd(torch, 3 * Ni + E)
    P, A, us, gs = rnd(Ni, Nq), rnd(Nq, Nj), [rnd(E, Nj), rnd(E, Nj)], [rnd(E, Ni), rnd(E, Ni)]
    for flags in (0, WO_P_T | WO_A_T):
        sP, sA = (P.T.contiguous(), A.T.contiguous()) if flags else (P, A)
        base = _launch(torch, shape, E, sP, sA, us, gs, flags)
        assert bool(torch.isfinite(base).all())
        for shifts in ((1, 0, 0, 0, 0), (0, 1, 0, 0, 0), (0, 0, 1, 0, 0), (0, 0, 0, 1, 0), (0, 0, 0, 0, 1), (1, 1, 1, 1, 1)):
            dW = _launch(torch, shape, E, sP, sA, us, gs, flags, shifts)
            assert bool(torch.isfinite(dW).all()) and torch.equal(_bits(dW), _bits(base)), (shape, E, flags, shifts)


# ---- 5. a planted non-finite value reaches exactly its dependency set ----------------------------------------------

@pytest.mark.parametrize("shape", ((35, 56, 35), (17, 5, 5)), ids=_id)
def test_a_planted_non_finite_value_stays_in_its_dependency_set(torch, shape):
    Ni, Nq, Nj = shape
    E = 1003                      # 62 full tiles and one of 11 elements: element 1002 is the partial tile's last one
    d = Exact(shape, E, 1, 31 + Ni)
    shapes = [(Ni, Nq), (Nq, Nj), (E, Nj), (E, Ni)]
    spots = [(2, (E - 1, Nj - 1)), (2, (31, 0)),           # u: the partial tile's last element, a full tile's last one
             (3, (E - 1, Ni - 1)), (3, (31, 0)),           # g: likewise
             (0, (Ni - 1, Nq - 1)), (0, (0, 0)), (1, (Nq - 1, Nj - 1)), (1, (0, 0))]
    for operand, index in spots:
        dep = R.dependency_set(WSUBS, shapes, operand, index)
        for planted in (math.nan, math.inf):
            host = [d.P.copy(), d.A.copy(), d.u[0].copy(), d.g[0].copy()]
            host[operand][index] = planted
            for flags in (0, WO_P_T | WO_A_T):
                P = np.ascontiguousarray(host[0].T) if flags else host[0]
                A = np.ascontiguousarray(host[1].T) if flags else host[1]
                dW = _launch(torch, shape, E, P, A, [host[2]], [host[3]], flags)
                assert R.nonfinite_violations(dW.cpu().numpy(), d.ref(1), dep, planted) == 0, (shape, operand, index, planted, flags)


# ---- 6. the whole backward pass ------------------------------------------------------------------------------------

def _within(got, subs, operands, rows=1):
    """*got* against the summed bounded references of the rows *operands* (a list of operand lists)."""
    refs = [R.bounded_reference(subs, [o.cpu().numpy() for o in ops]) for ops in operands]
    ref, absref = sum(r for r, _ in refs), sum(a for _, a in refs)
    letters = subs.split("->")[0].split(",")
    extent = {ch: int(o.shape[k]) for s, o in zip(letters, operands[0]) for k, ch in enumerate(s)}
    n = len(operands) * R.bound_terms(subs, extent, len(letters))
    return R.bound_violations(got.cpu().numpy(), ref, absref, n, R.U64) == 0


_PASSES = {}


def _backward_pass(torch, shape, b):
    """One backward pass of (shape, b) at E = 1003 with W and every u_k asking for a gradient, computed once and shared by
    the tests below (nobody changes it): the operands, the results and the routes."""
    if (shape, b) not in _PASSES:
        Ni, Nq, Nj = shape
        E = 1003
        rnd = _rnd(torch, 7 * Ni + b)
        P, A, W = rnd(Ni, Nq), rnd(Nq, Nj), rnd(E, Nq)
        us, gs = [rnd(E, Nj) for _ in range(b)], [rnd(E, Ni) for _ in range(b)]
        autograd.launch_counts.clear()
        outs, dW, dus = _through_autograd(torch, TEMPLATES[0][0], shape, E, P, A, us, gs, u=True, W_values=W)
        _PASSES[shape, b] = dict(E=E, P=P, A=A, W=W, us=us, gs=gs, outs=outs, dW=dW, dus=dus, counts=Counter(autograd.launch_counts))
    return _PASSES[shape, b]


BACKWARD_CASES = [(shape, b) for shape in ((35, 56, 35), (17, 5, 5), (20, 56, 35)) for b in (1, 4)]
_case_id = lambda c: f"{_id(c[0])}-b{c[1]}"   # noqa: E731


@pytest.mark.parametrize("case", BACKWARD_CASES, ids=_case_id)
def test_the_whole_backward_pass_of_the_weighted_operator(torch, case):
    shape, b = case
    Ni, Nq, Nj = shape
    r = _backward_pass(torch, shape, b)
    E, P, A, W, us, gs = (r[k] for k in ("E", "P", "A", "W", "us", "gs"))
    # one call for dW, one for every du_k together; nothing on the one-thread-per-entry kernel
    assert r["counts"] == Counter({"weighted_w": 1, "weighted_u": 1}), r["counts"]
    expr = _expr(TEMPLATES[0][0], shape, b)
    arrays = {"P": P, "A": A, "W": W, **{f"u{k}": u for k, u in enumerate(us)}}
    plain = f.evaluate(expr, 0, arrays, transform=FWD, wait=True)
    for nm in expr.output_names:
        assert torch.equal(_bits(r["outs"][nm]), _bits(plain[nm])), nm
    grads = {output_grad_name(nm): g for nm, g in zip(expr.output_names, gs)}
    for k in range(b):
        (term,) = adjoint_terms(expr, f"u{k}")
        by_hand = f.evaluate(term.einsum, 0, {**arrays, **grads}, transform=FWD, wait=True)[term.einsum.output_names[0]]
        assert torch.equal(_bits(r["dus"][k]), _bits(by_hand)), k
    by_hand = torch.empty(E, Nq, dtype=torch.float64, device="cuda")
    _hip.weightgrad(P.data_ptr(), A.data_ptr(), [u.data_ptr() for u in us], [g.data_ptr() for g in gs], by_hand.data_ptr(), E, Ni, Nq, Nj)
    torch.cuda.synchronize()
    assert torch.equal(_bits(r["dW"]), _bits(by_hand))
    # only W asks for a gradient: no u-adjoint runs
    autograd.launch_counts.clear()
    _, dW_alone, dus = _through_autograd(torch, TEMPLATES[0][0], shape, E, P, A, us, gs, W_values=W)
    assert autograd.launch_counts == Counter({"weighted_w": 1}) and dus == [None] * b
    assert torch.equal(_bits(dW_alone), _bits(r["dW"]))


@pytest.mark.parametrize("wrt", ("W", "u"))
@pytest.mark.parametrize("case", BACKWARD_CASES, ids=_case_id)
def test_the_gradients_are_within_the_bound_of_their_adjoint_einsums(torch, case, wrt):
    shape, b = case
    r = _backward_pass(torch, shape, b)
    P, A, W, us, gs = (r[k] for k in ("P", "A", "W", "us", "gs"))
    if wrt == "W":
        assert _within(r["dW"], WSUBS, [[P, A, u, g] for u, g in zip(us, gs)])
    else:
        for k in range(b):
            assert _within(r["dus"][k], "iq,eq,qj,ei->ej", [[P, W, A, gs[k]]]), k


def test_a_field_of_two_forward_rows_is_not_batched(torch):
    """Every term on its own, its rows summed as before: one term of two rows, one call."""
    shape, E = (17, 5, 5), 1003
    Ni, Nq, Nj = shape
    rnd = _rnd(torch, 2)
    P, A, W, gs = rnd(Ni, Nq), rnd(Nq, Nj), rnd(E, Nq), [rnd(E, Ni) for _ in range(2)]
    twice = f.batched_einsum(TEMPLATES[0][0], [[f.array("P", (Ni, Nq)), f.array("W", ("E", Nq)), f.array("A", (Nq, Nj)),
                                               f.array("u0", ("E", Nj))] for _ in range(2)])
    u0 = rnd(E, Nj).requires_grad_(True)
    autograd.launch_counts.clear()
    outs = f.evaluate_differentiable(twice, 0, {"P": P, "W": W, "A": A, "u0": u0}, transform=FWD, element_gradients="kernel")
    torch.autograd.backward([outs[nm] for nm in twice.output_names], gs)
    torch.cuda.synchronize()
    assert autograd.launch_counts == Counter({"weighted_u": 1}), autograd.launch_counts
    assert _within(u0.grad, "iq,eq,qj,ei->ej", [[P, W, A, gs[0]], [P, W, A, gs[1]]])


@pytest.mark.parametrize("with_j", (False, True), ids=("ij,ej->ei", "e,ij,ej->ei"))
@pytest.mark.parametrize("shape", ((56, 35), (20, 35)), ids=_id)
def test_the_whole_backward_pass_of_the_element_operator(torch, shape, with_j):
    Ni, Nj = shape
    E, b = 1003, 2
    rnd = _rnd(torch, 5 * Ni + with_j)
    A, J, us, gs = rnd(Ni, Nj), rnd(E), [rnd(E, Nj) for _ in range(b)], [rnd(E, Ni) for _ in range(b)]
    subs = "e,ij,ej->ei" if with_j else "ij,ej->ei"
    row = lambda k: ([f.array("J", ("E",))] if with_j else []) + [f.array("A", (Ni, Nj)), f.array(f"u{k}", ("E", Nj))]   # noqa: E731
    expr = f.batched_einsum(subs, [row(k) for k in range(b)])

    def run(transform, element_gradients):
        leaves = {"A": A.clone(), **({"J": J.clone().requires_grad_(True)} if with_j else {}),
                  **{f"u{k}": u.clone().requires_grad_(True) for k, u in enumerate(us)}}
        autograd.launch_counts.clear()
        outs = f.evaluate_differentiable(expr, 0, leaves, transform=transform, element_gradients=element_gradients)
        torch.autograd.backward([outs[nm] for nm in expr.output_names], [g.clone() for g in gs])
        torch.cuda.synchronize()
        return outs, leaves, Counter(autograd.launch_counts)

    old_outs, old, old_counts = run("auto", "auto")
    outs, new, counts = run("element_operator", "kernel")
    arrays = {"A": A, "J": J, **{f"u{k}": u for k, u in enumerate(us)}}
    plain = f.evaluate(expr, 0, {nm: arrays[nm] for nm in expr.all_args}, transform="element_operator", wait=True)
    assert all(torch.equal(_bits(outs[nm]), _bits(plain[nm])) for nm in expr.output_names)
    # every du_k on the kernel with the transposed operator; dJ where it was
    j_terms = 1 if with_j else 0
    assert sum(old_counts.values()) == b + j_terms and "elemop_u" not in old_counts, old_counts
    assert counts["elemop_u"] == b and sum(counts.values()) == b + j_terms, counts
    grads = {output_grad_name(nm): g for nm, g in zip(expr.output_names, gs)}
    for k in range(b):
        (term,) = adjoint_terms(expr, f"u{k}")
        by_hand = f.evaluate(term.einsum, 0, {**{nm: arrays[nm] for nm in expr.all_args}, **grads}, transform="element_operator",
                             wait=True)[term.einsum.output_names[0]]
        assert torch.equal(_bits(new[f"u{k}"].grad), _bits(by_hand)), k
        assert _within(new[f"u{k}"].grad, "e,ij,ei->ej" if with_j else "ij,ei->ej", [([J] if with_j else []) + [A, gs[k]]]), k
    if with_j:
        assert torch.equal(_bits(new["J"].grad), _bits(old["J"].grad))
    # (a rectangular operator: no family kernel knows its adjoints, so the old route of every term is "auto")
    assert old_counts == Counter({"auto": b + j_terms}) and counts == Counter({"elemop_u": b, **({"auto": 1} if with_j else {})})


# ---- 7. fallbacks --------------------------------------------------------------------------------------------------

def test_a_u_adjoint_outside_the_rule_keeps_its_route(torch):
    shape, E = (45, 64, 33), 1003
    Ni, Nq, Nj = shape
    assert weighted_element_operator_supported(Ni, Nq, Nj) and not weighted_element_operator_supported(Nj, Nq, Ni)
    assert weighted_weight_adjoint_supported(Ni, Nq, Nj)
    rnd = _rnd(torch, 45)
    P, A, W, u, g = rnd(Ni, Nq), rnd(Nq, Nj), rnd(E, Nq), rnd(E, Nj), rnd(E, Ni)
    autograd.launch_counts.clear()
    outs, dW, (du,) = _through_autograd(torch, TEMPLATES[0][0], shape, E, P, A, [u], [g], u=True, W_values=W)
    assert autograd.launch_counts == Counter({"weighted_w": 1, "auto": 1}), autograd.launch_counts
    expr = _expr(TEMPLATES[0][0], shape, 1)
    plain = f.evaluate(expr, 0, {"P": P, "A": A, "W": W, "u0": u}, transform=FWD, wait=True)
    assert torch.equal(_bits(outs[expr.output_names[0]]), _bits(plain[expr.output_names[0]]))
    assert _within(dW, WSUBS, [[P, A, u, g]]) and _within(du, "iq,eq,qj,ei->ej", [[P, W, A, g]])


def test_nine_fields_take_two_calls(torch):
    shape, E, b = (20, 35, 20), 1003, 9
    Ni, Nq, Nj = shape
    rnd = _rnd(torch, 9)
    P, A = rnd(Ni, Nq), rnd(Nq, Nj)
    us, gs = [rnd(E, Nj) for _ in range(b)], [rnd(E, Ni) for _ in range(b)]
    autograd.launch_counts.clear()
    _, dW, _ = _through_autograd(torch, "qi,eq,jq,ej->ei", shape, E, P.T.contiguous(), A.T.contiguous(), us, gs)
    assert autograd.launch_counts == Counter({"weighted_w": 2}), autograd.launch_counts
    assert _within(dW, WSUBS, [[P, A, u, g] for u, g in zip(us, gs)])
    # bitwise: the first eight rows in one call, the ninth in another, added
    first, ninth = _launch(torch, shape, E, P, A, us[:8], gs[:8]), _launch(torch, shape, E, P, A, us[8:], gs[8:])
    assert torch.equal(_bits(dW), _bits(first + ninth))


# ---- 8. a queue on a side stream -----------------------------------------------------------------------------------

def test_a_queue_on_another_stream_gives_the_default_streams_bits(torch):
    shape, E, b = (20, 56, 35), 1003, 2
    Ni, Nq, Nj = shape
    rnd = _rnd(torch, 4)
    P, A, W = rnd(Ni, Nq), rnd(Nq, Nj), rnd(E, Nq)
    us, gs = [rnd(E, Nj) for _ in range(b)], [rnd(E, Ni) for _ in range(b)]
    outs, dW, dus = _through_autograd(torch, TEMPLATES[0][0], shape, E, P, A, us, gs, u=True, W_values=W)
    torch.cuda.synchronize()
    q = f.DeviceQueue(0, torch.cuda.Stream(priority=-1))
    outs_q, dW_q, dus_q = _through_autograd(torch, TEMPLATES[0][0], shape, E, P, A, us, gs, q=q, u=True, W_values=W)
    assert torch.equal(_bits(dW_q), _bits(dW)) and all(torch.equal(_bits(a), _bits(c)) for a, c in zip(dus_q, dus))
    assert all(torch.equal(_bits(outs_q[nm]), _bits(outs[nm])) for nm in outs)


# ---- 9. "auto" is unchanged ----------------------------------------------------------------------------------------

#: (forward einsum, its extents, b) -> launch_counts of the backward pass under element_gradients="auto", transform="auto", with
#: every field and (where there is one) W or J asking for a gradient.  The routes of the parent commit, whose ``_run_term`` this
#: change leaves as it was below the new branch: a term no family matcher knows is "auto", a square element-local operator's
#: u-adjoint is the MATAPPLY family with the transposed operator.
PARENT_ROUTES = (
    ("iq,eq,qj,ej->ei", (35, 56, 35), 1, {"auto": 2}),
    ("iq,eq,qj,ej->ei", (20, 56, 35), 4, {"auto": 5}),
    ("ij,ej->ei", (56, 35), 2, {"auto": 2}),
    ("e,ij,ej->ei", (56, 35), 2, {"auto": 3}),
    ("ij,ej->ei", (35, 35), 2, {"family": 2}),
)


@pytest.mark.parametrize("subs,shape,b,routes", PARENT_ROUTES, ids=[f"{s}-{_id(e)}-b{b}" for s, e, b, _ in PARENT_ROUTES])
def test_auto_routes_and_computes_as_before(torch, subs, shape, b, routes):
    E = 1003
    rnd = _rnd(torch, sum(shape) + b)
    weighted = len(shape) == 3
    Ni, Nj = shape[0], shape[-1]
    ops = {"P": rnd(Ni, shape[1]), "W": rnd(E, shape[1]), "A": rnd(shape[1], Nj)} if weighted else {"A": rnd(Ni, Nj), "J": rnd(E)}
    dims = {"iq": "P", "eq": "W", "qj": "A", "ij": "A", "e": "J"}
    ins = subs.split("->")[0].split(",")
    leaves = {nm: t.clone().requires_grad_(nm in ("W", "J")) for nm, t in ops.items() if nm in {dims.get(s) for s in ins}}
    leaves.update({f"u{k}": rnd(E, Nj).requires_grad_(True) for k in range(b)})
    size = {"i": Ni, "j": Nj, "q": shape[1], "e": "E"}
    expr = f.batched_einsum(subs, [[f.array(dims.get(s, f"u{k}"), tuple(size[ch] for ch in s)) for s in ins] for k in range(b)])
    gs = [rnd(E, Ni) for _ in range(b)]
    autograd.launch_counts.clear()
    outs = f.evaluate_differentiable(expr, 0, leaves, transform="auto")
    torch.autograd.backward([outs[nm] for nm in expr.output_names], gs)
    torch.cuda.synchronize()
    assert autograd.launch_counts == Counter(routes), autograd.launch_counts
    grads = {output_grad_name(nm): g for nm, g in zip(expr.output_names, gs)}
    detached = {nm: t.detach() for nm, t in leaves.items()}
    for nm, leaf in leaves.items():
        if not leaf.requires_grad:
            continue
        total = None
        for term in adjoint_terms(expr, nm):      # what the parent commit computes: every term under "auto", rows added in order
            got = f.evaluate(term.einsum, 0, {**detached, **grads}, wait=True)
            for out_name in term.einsum.output_names:
                total = got[out_name] if total is None else total.add_(got[out_name])
        assert torch.equal(_bits(leaf.grad), _bits(total)), nm


# ---- 10. speed: one floor ------------------------------------------------------------------------------------------

#: halfway between 1.0 and the ratio tools/bench_weighted_operator_gradients.py measured at this shape and size on the MI355X
#: (c / d = 1.915 [1.906, 1.924] at (35, 56, 35), b = 1, E = 2e5): the convention of section 3m
SPEED_FLOOR = 1.4575


def test_faster_than_the_two_pass_route(torch):
    """Against what a caller can chain by hand from kernels older than fe_weightgrad_f64: "element_operator" 35 -> 56 of u and
    of g (the latter with the transposed operator) and one ``torch.mul``, the two E x 56 temporaries allocated once."""
    from feinsum_amd.family import match_weighted_operator_weight_adjoint
    from feinsum_amd.measure import _bind, _WeightGradLaunch

    shape, E = (35, 56, 35), 200_000
    Ni, Nq, Nj = shape
    rnd = _rnd(torch, 1)
    P, A, u, g = rnd(Ni, Nq), rnd(Nq, Nj), rnd(E, Nj), rnd(E, Ni)
    q = f.DeviceQueue(0)
    (term,) = adjoint_terms(_expr(TEMPLATES[0][0], shape, 1), "W")
    dW, dW2 = torch.empty(E, Nq, dtype=torch.float64, device="cuda"), torch.empty(E, Nq, dtype=torch.float64, device="cuda")
    fused = _WeightGradLaunch(match_weighted_operator_weight_adjoint(term.einsum), term.einsum,
                              {"P": P, "A": A, "u0": u, output_grad_name("_fe_out"): g}, [dW])
    up = f.einsum("ij,ej->ei", f.array("A", (Nq, Nj)), f.array("u", ("E", Nj)))
    gup = f.einsum("ji,ej->ei", f.array("P", (Ni, Nq)), f.array("g", ("E", Ni)))
    t, s = torch.empty_like(dW), torch.empty_like(dW)
    first = _bind(up, q, {"A": A, "u": u}, {up.output_names[0]: t}, "element_operator")[1]
    second = _bind(gup, q, {"P": P, "g": g}, {gup.output_names[0]: s}, "element_operator")[1]

    def two_pass(stream_ptr):
        first.launch(stream_ptr)
        second.launch(stream_ptr)
        torch.mul(t, s, out=dW2)

    launch = {"c": two_pass, "d": fused.launch}
    times = {"c": [], "d": []}
    for form in launch:
        _hip.time_with_events(launch[form], 10, q.stream_ptr)          # warm-up
    # (one field: both routes round the two sums, then one product)
    assert torch.allclose(dW, dW2, rtol=1e-12, atol=1e-12)
    for _ in range(5):                                     # the forms take turns
        for form in ("c", "d"):
            times[form].append(_hip.time_with_events(launch[form], 20, q.stream_ptr) / 20)
    c, d = (float(np.median(times[form])) for form in ("c", "d"))
    print(f"c (two passes and a product) {c * 1e6:.1f} us, d (fe_weightgrad_f64) {d * 1e6:.1f} us, c / d = {c / d:.3f}, floor {SPEED_FLOOR}")
    # measured c / d = 1.915 [1.906, 1.924]; the floor is (1 + 1.915) / 2
    assert c / d > SPEED_FLOOR, (c, d, c / d)
