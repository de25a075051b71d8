"""The references of the backward-pass sweep (tools/fuzz_autograd.py) and its case lists, without a GPU: the shared bit
budgets hold for every forward and adjoint row and are spent, the int64 gradient reference is the numpy sum of the
adjoint einsums and torch's CPU autograd, gradient dependency sets match hand-checked ones, the checkers reject
planted errors, and the host-predicted routes of the fixed-seed case list reach every coverage minimum."""

import math
import sys
from pathlib import Path

import numpy as np
import pytest

import autograd_cases as C
from feinsum_amd import autograd as AG
from oracle import einsum_ref as R

sys.path.insert(0, str(Path(__file__).resolve().parents[1] / "tools"))
import fuzz_autograd as A  # noqa: E402
import fuzz_dg as D  # noqa: E402

SEED = 20261016   # tests/test_gpu_autograd_fuzz.py sweeps the same cases
N_EXACT, N_EINSUM, N_BOUNDED, N_NONFINITE = 60, 16, 30, 12


def _cases():
    return A.gen_cases(N_EXACT, SEED, N_EINSUM)


def _worst(bits, names, n):
    w = max(int(n), 1)
    for nm in names:
        w *= (1 << bits[nm]) - 1
    return w


def _small(cases, max_e=200):
    return [c for c in cases if c.E <= max_e and (c.dg is None or c.dg.Np <= 35)]


# --------------------------------------------------------------------------
# bit budgets
# --------------------------------------------------------------------------

def test_budgets_hold_for_every_adjoint_row_and_are_spent():
    """Every row of every adjoint term of every input (counted with all the products summed into one gradient entry)
    and every forward row fits its significand -- 24 bits for float32 einsums and for the gradient of a float32
    operand; one more bit in any array below its cap breaks some row."""
    n_f32_rows = 0
    for case in _cases():
        bits, scales, dtypes, S = A.plan_data(case, np.random.default_rng(case.seed))
        rows = A.budget_rows(case.expr(), case.drop, case.E)
        sub = 4 if case.scale == "subnormal" else 0
        for names, n, sig in rows:
            assert _worst(bits, names, n) <= 1 << (sig - sub), (case.repro(), names)
            n_f32_rows += sig == 24
        scaled = [(names, n << (53 - sig)) for names, n, sig in rows]
        for k, b in bits.items():
            cap = 24 if dtypes[k] == np.dtype("float32") else S
            assert 1 <= b <= cap
            if b < cap:
                assert not R.rows_fit(scaled, {**bits, k: b + 1}, S), (case.repro(), k)
    assert n_f32_rows > 100


def test_gradient_of_a_float32_operand_fits_float32():
    """Mixed face-mass (float32 fields): the v-gradient rows use 24 bits, so rounding the float64 sum is exact."""
    case = A.AGCase(D.DGCase("fm", 35, 15, 3, "rij", "mixed", 17, "ragged", 5), None, "auto")
    rows = A.budget_rows(case.expr(), (), 17)
    vrows = [(names, n, sig) for names, n, sig in rows if AG.output_grad_name("_fe_out_0") in names and "R" in names
             and "J" in names]
    assert vrows and all(sig == 24 for _, _, sig in vrows)
    arrays, mants, scales = A.host_data(case)
    _, grads = A.host_references(case, mants, scales)
    assert grads["v1"].dtype == np.float32
    assert np.array_equal(grads["v1"].astype(np.float64), C.numpy_adjoint_grad(case.expr(), "v1", _in(case, arrays),
                                                                               _g(case, arrays)))


def test_range_cases_keep_one_scale_per_gradient():
    for case in [c for c in _cases() if c.scale != "normal"]:
        arrays, mants, scales = A.host_data(case)
        for k, a in arrays.items():
            assert np.isfinite(a).all()
            assert np.array_equal(np.ldexp(a.astype(np.float64), -scales[k]), mants[k].astype(np.float64))
        fwd, grads = A.host_references(case, mants, scales)   # asserts one total scale per gradient
        assert all(np.isfinite(g).all() for g in grads.values() if g is not None)
        if case.scale == "subnormal":
            tiny = np.finfo(np.float32 if case.dtype == "float32" else np.float64).tiny
            for g in grads.values():
                assert g is None or (np.abs(g) < tiny).all()
                assert g is None or not g.any() or (g != 0).sum() > 0.5 * g.size
        else:
            top, _ = R.RANGE[np.dtype("float32") if case.dtype == "float32" else np.dtype("float64")]
            edge = 2.0 ** (top - (24 if case.dtype == "float32" else 53))
            for g in grads.values():   # every nonzero gradient entry at least 2^(top - significand)
                assert g is None or (np.abs(g[g != 0]) >= edge).all() and (np.abs(g) < 2.0 ** top).all()


# --------------------------------------------------------------------------
# the references
# --------------------------------------------------------------------------

def _in(case, arrays):
    return {n: arrays[n] for n in case.expr().all_args}


def _g(case, arrays):
    """Output gradients for every output: zeros for the rows that get none."""
    expr = case.expr()
    shape = C.concrete(expr.shape, case.E)
    return {n: arrays[AG.output_grad_name(n)] if k not in case.drop else np.zeros(shape)
            for k, n in enumerate(expr.output_names)}


def test_int64_reference_is_numpy_adjoint_sum_and_torch_autograd():
    torch = pytest.importorskip("torch")
    checked = 0
    for case in _small(_cases(), 64)[::2]:
        if case.scale != "normal":
            continue
        expr = case.expr()
        arrays, mants, scales = A.host_data(case)
        fwd, grads = A.host_references(case, mants, scales)
        ins, gb = _in(case, arrays), _g(case, arrays)
        tref = C.torch_reference_grads(expr, ins, gb)
        for name in expr.output_names:
            assert R.bitwise_equal(fwd[name], C.numpy_forward(expr, ins)[name].astype(fwd[name].dtype))
        for w, g in grads.items():
            if g is None:
                assert not np.any(tref[w])
                continue
            want = C.numpy_adjoint_grad(expr, w, ins, gb)
            assert R.bitwise_equal(g, want.astype(g.dtype)), (case.repro(), w)
            assert R.bitwise_equal(g, tref[w].astype(g.dtype)), (case.repro(), w)
            checked += 1
    assert checked > 60
    del torch


def test_expand_to_operand_of_a_zero_dim_operand():
    torch = pytest.importorskip("torch")
    t = AG.expand_to_operand(torch.tensor(3.0), (), (), ())
    assert t.shape == () and float(t) == 3.0
    assert tuple(AG.expand_to_operand(torch.ones(3), ("i",), ("e", "i"), (4, 3)).shape) == (4, 3)


# --------------------------------------------------------------------------
# dependency sets
# --------------------------------------------------------------------------

def test_gradient_dependency_sets_by_hand():
    """A NaN in grad's output gradient at (x, e, i) reaches dJ[x, :, e], du[e, :] and dD[:, i, :]; one in u[e, j]
    reaches dJ[:, :, e], dD[:, :, j] and the output gradient's own... (nothing: it is no input)."""
    torch = pytest.importorskip("torch")
    E, Np = 5, 4
    expr = C.grad(3, Np)
    g = AG.output_grad_name("_fe_out")
    shapes = {"J": (3, 3, E), "D": (3, Np, Np), "u": (E, Np), g: (3, E, Np)}
    dep = A.dependency(torch, expr, (), shapes, g, (2, 1, 3), E, "cpu")
    want = np.zeros((3, 3, E), bool)
    want[2, :, 1] = True
    assert np.array_equal(dep["J"].numpy(), want)
    want = np.zeros((E, Np), bool)
    want[1, :] = True
    assert np.array_equal(dep["u"].numpy(), want)
    want = np.zeros((3, Np, Np), bool)
    want[:, 3, :] = True
    assert np.array_equal(dep["D"].numpy(), want)
    assert not dep["_fe_out"].any()
    dep = A.dependency(torch, expr, (), shapes, "u", (1, 2), E, "cpu")
    want = np.zeros((3, 3, E), bool)
    want[:, :, 1] = True
    assert np.array_equal(dep["J"].numpy(), want)
    want = np.zeros((3, Np, Np), bool)
    want[:, :, 2] = True
    assert np.array_equal(dep["D"].numpy(), want)
    assert not dep["u"].any()
    # face-mass x 2: a NaN in J[e, f] reaches dv_k[f, e, :] of every field and dR of nothing... but dR[f] (all i, j)
    fm = C.face_mass(Np, 4, 3, 2)
    shapes = {"J": (E, 4), "R": (4, Np, 3), "v0": (4, E, 3), "v1": (4, E, 3),
              **{AG.output_grad_name(n): (E, Np) for n in fm.output_names}}
    dep = A.dependency(torch, fm, (), shapes, "J", (3, 2), E, "cpu")
    want = np.zeros((4, E, 3), bool)
    want[2, 3, :] = True
    assert np.array_equal(dep["v0"].numpy(), want) and np.array_equal(dep["v1"].numpy(), want)
    want = np.zeros((4, Np, 3), bool)
    want[2] = True
    assert np.array_equal(dep["R"].numpy(), want)
    assert not dep["J"].any()
    # the same, union of the per-term dependency_set, broadcast with expand_to_operand
    for wrt, _, sub, term in A.plan_backward(fm):
        for row in sub.args:
            for p, a in enumerate(row):
                if a.name == "J":
                    ds = R.dependency_set(sub.get_subscripts(), [shapes[b.name] for b in row], p, (3, 2))
                    assert not (AG.expand_to_operand(ds, sub.out_idx_set, term.wrt_subscripts, shapes[wrt])
                                & ~dep[wrt].numpy()).any()


# --------------------------------------------------------------------------
# the checkers reject planted errors
# --------------------------------------------------------------------------

def _fm9():
    case = A.AGCase(D.DGCase("fm", 10, 6, 9, "rij", "float64", 33, "ragged", 11), None, "auto")
    arrays, mants, scales = A.host_data(case)
    return case, arrays, mants, scales


def test_checkers_reject_planted_errors():
    case, arrays, mants, scales = _fm9()
    expr = case.expr()
    ref = A.grad_reference(expr, (), mants, scales, "J", case.E)
    assert R.differing_entries(ref.copy(), ref) == 0
    ulp = ref.copy()
    k = int(np.argmax(np.abs(ulp)))
    ulp.flat[k] = np.nextafter(ulp.flat[k], np.inf)                       # a single ulp
    assert R.differing_entries(ulp, ref) == 1
    dropped = A.grad_reference(expr, (), mants, scales, "J", case.E, skip=(0, 4))    # a dropped term row
    assert R.differing_entries(dropped, ref) > 0
    doubled = A.grad_reference(expr, (), mants, scales, "J", case.E, extra=(0, 8))   # the b > 8 chunk added twice
    assert R.differing_entries(doubled, ref) > 0
    # the second chunk overwriting dJ instead of adding to it: only the fields 8.. survive
    only_last = sum(A.grad_reference(expr, (), mants, scales, "J", case.E, skip=(0, r)) - ref for r in range(8)) + ref
    assert R.differing_entries(only_last, ref) > 0
    f32 = ref.astype(np.float32).astype(np.float64)                      # rounded through float32 in the middle
    assert R.differing_entries(f32, ref) > 0
    # a transposed operator: grad's u-gradient with D^T
    g = A.AGCase(D.DGCase("grad", 10, 6, 1, "rij", "float64", 17, "ragged", 3), None, "auto")
    _, m, s = A.host_data(g)
    uref = A.grad_reference(g.expr(), (), m, s, "u0", 17)
    mt = dict(m, R=np.ascontiguousarray(np.swapaxes(m["R"], 1, 2)))
    assert R.differing_entries(A.grad_reference(g.expr(), (), mt, s, "u0", 17), uref) > 0
    # a NaN outside its dependency set
    torch = pytest.importorskip("torch")
    gname = AG.output_grad_name("_fe_out")
    shapes = {"J": (3, 3, 17), "R": (3, 10, 10), "u0": (17, 10), gname: (3, 17, 10)}
    dep = A.dependency(torch, g.expr(), (), shapes, gname, (0, 16, 9), 17, "cpu")["u0"]
    r = torch.from_numpy(uref)
    good = torch.where(dep, torch.tensor(math.nan, dtype=torch.float64), r)
    assert R.nonfinite_violations(good, r, dep, math.nan) == 0
    stray = good.clone()
    stray[15, 0] = math.nan                                               # the element next to it, same tile
    assert R.nonfinite_violations(stray, r, dep, math.nan) >= 1


def test_bound_rejects_a_float32_intermediate_and_a_lost_term():
    case = A.AGCase(D.DGCase("grad", 20, 10, 1, "rij", "float64", 65, "ragged", 9), None, "auto")
    expr = case.expr()
    host = A.bounded_data(case)
    n, u, rounded = A.bound_of(expr, (), "J", case.E)
    ref, absref = A.bounded_grad(expr, (), host, "J")
    got = np.asarray(ref, dtype=np.float64)
    assert A.grad_bound_ratio(got, ref, absref, n, u, rounded) <= 1
    assert A.grad_bound_ratio(got.astype(np.float32).astype(np.float64), ref, absref, n, u, rounded) > 1
    # a float32 operand of a float64 einsum: one float32 rounding is allowed, two are not
    mixed = A.AGCase(D.DGCase("grad", 20, 10, 1, "rij", "mixed", 65, "ragged", 9), None, "auto")
    hm = A.bounded_data(mixed)
    n, u, rounded = A.bound_of(mixed.expr(), (), "u0", mixed.E)
    assert rounded and u == R.U64
    ref, absref = A.bounded_grad(mixed.expr(), (), hm, "u0")
    once = np.asarray(ref, dtype=np.float64).astype(np.float32)
    assert A.grad_bound_ratio(once, ref, absref, n, u, rounded) <= 1
    assert A.grad_bound_ratio(once + np.float32(2 ** -20) * np.abs(once), ref, absref, n, u, rounded) > 1


# --------------------------------------------------------------------------
# routes and coverage
# --------------------------------------------------------------------------

def test_routes_match_the_backward_logic():
    """Hand-checked routes: grad (geomadj, family, auto), face-mass x 9 (facemass_v per field, one facemass_j, auto),
    tetrahedra p = 5 and the tiled-only orders (the J-adjoint on auto), a mixed einsum (auto for J)."""
    def routes(kind, Np, Nfp, b, dtype):
        return A.predicted_launches(A.AGCase(D.DGCase(kind, Np, Nfp, b, "rij", dtype, 17, "ragged", 1), None, "auto"))
    assert routes("grad", 35, 15, 1, "float64") == {"geomadj": 1, "family": 1, "auto": 1}
    assert routes("fm", 35, 15, 9, "float64") == {"facemass_v": 9, "facemass_j": 1, "auto": 1}
    for Np, Nfp in ((56, 21), (7, 4), (13, 5)):
        assert routes("grad", Np, Nfp, 1, "float64") == {"family": 1, "auto": 2}
        assert routes("fm", Np, Nfp, 2, "float64") == {"auto": 4}
    assert routes("grad", 35, 15, 1, "mixed") == {"family": 1, "auto": 2}
    assert routes("cross", 10, 6, 1, "float64") == {"geomadj": 3, "family": 4, "auto": 1}
    dropped = A.AGCase(D.DGCase("fm", 35, 15, 9, "rij", "float64", 17, "ragged", 1), None, "auto", drop=(0, 3))
    assert A.predicted_launches(dropped) == {"facemass_v": 7, "facemass_j": 1, "auto": 1}


def test_case_lists_reach_every_minimum():
    cases = _cases()
    cnt = A.coverage(cases)
    assert not A.missing_buckets(cnt, A.MINIMUMS), A.missing_buckets(cnt, A.MINIMUMS)
    assert {c.dg.Np for c in cases if c.dg is not None} >= {n for n, _ in D.ORDERS3} | {n for n, _ in D.ORDERS2}
    assert {c.dg.b for c in cases if c.dg is not None and c.kind in ("fm", "bgrad")} >= {9, 17}
    for c in cases:
        if c.ein is not None:
            ins = c.ein.subs.split("->")[0].split(",")
            assert all(len(set(o)) == len(o) for o in ins)
        assert A.AGCase.from_repro(c.repro()) == c


def test_other_passes_reach_every_route():
    nf = Counter_of(A.nonfinite_cases(N_NONFINITE, SEED))
    large = Counter_of(A.large_cases(SEED))
    for r in A.ROUTES:
        assert nf[f"route:{r}"] >= 3 and large[f"route:{r}"] >= 3, r
    assert large["route:facemass_j:b>8"] >= 3
    assert {c.E for c in A.large_cases(SEED)} >= {98_304, 100_007, 1_000_003}
    assert Counter_of(A.bounded_cases(N_BOUNDED, SEED))["b:>8"] >= 2


def Counter_of(cases):
    return A.coverage(cases)


# --------------------------------------------------------------------------
# operator gradients on the matrix cores (operator_gradients="kernel")
# --------------------------------------------------------------------------

def test_kernel_mode_routes_follow_match_operator_adjoint():
    """Hand-checked routes, then every case of the list: a term takes "opgrad_d" / "opgrad_r" exactly where
    ``match_operator_adjoint`` accepts it under "kernel", and today's route everywhere else (p = 5, the tiled-only orders,
    float32, mixed, rows with different J)."""
    from feinsum_amd.family import match_operator_adjoint

    def routes(kind, Np, Nfp, b, dtype, **kw):
        return A.predicted_launches(A.AGCase(D.DGCase(kind, Np, Nfp, b, "rij", dtype, 17, "ragged", 1), None, "auto",
                                             operator_gradients="kernel", **kw))
    assert routes("grad", 35, 15, 1, "float64") == {"geomadj": 1, "family": 1, "opgrad_d": 1}
    assert routes("fm", 35, 15, 9, "float64") == {"facemass_v": 9, "facemass_j": 1, "opgrad_r": 1}
    assert routes("bgrad", 20, 10, 9, "float64") == {"geomadj": 1, "family": 9, "opgrad_d": 1}
    assert routes("grad", 56, 21, 1, "float64") == {"family": 1, "auto": 2}             # the fall-backs: today's routes
    assert routes("grad", 35, 15, 1, "float32") == routes("grad", 35, 15, 1, "mixed") == {"family": 1, "auto": 2}
    assert routes("fm", 7, 4, 2, "float64") == {"auto": 4}
    assert routes("cross", 10, 6, 1, "float64") == {"geomadj": 3, "family": 4, "auto": 1}
    assert routes("fm", 35, 15, 9, "float64", drop=(0, 3)) == {"facemass_v": 7, "facemass_j": 1, "opgrad_r": 1}
    assert routes("fm", 35, 15, 3, "float64", frozen=("R",)) == {"facemass_v": 3, "facemass_j": 1}      # no opgrad launch
    assert routes("grad", 35, 15, 1, "float64", frozen=("R",)) == {"geomadj": 1, "family": 1}
    kernel = [c for c in _cases() if c.operator_gradients == "kernel"]
    assert len(kernel) >= 60 and all(c.dg is not None for c in kernel)
    n_op = 0
    for c in kernel:
        for wrt, route, sub, _ in A.plan_backward(c.expr(), c.drop, "kernel", c.frozen):
            plan = match_operator_adjoint(sub)
            assert (route in A.OPGRAD_ROUTES) == (plan is not None) and (plan is None or route == plan.kind)
            assert plan is None or wrt in A.operator_names(c.expr())
            assert route == A.route_of(sub, "kernel") and (plan is not None or route == A.route_of(sub))
            n_op += plan is not None
        assert not set(c.frozen) & {w for w, *_ in A.plan_backward(c.expr(), c.drop, "kernel", c.frozen)}
        assert A.AGCase.from_repro(c.repro()) == c and '"operator_gradients":"kernel"' in c.repro()
    assert n_op >= 30
    # "auto" never predicts them, and a line written before the field existed replays as "auto"
    assert all(r not in A.OPGRAD_ROUTES for c in _cases() if c.operator_gradients == "auto" for r in A.predicted_launches(c))
    old = A.AGCase(D.DGCase("grad", 10, 6, 1, "rij", "float64", 17, "ragged", 3), None, "auto")
    import json
    line = json.dumps({k: v for k, v in json.loads(old.repro()).items() if k not in ("operator_gradients", "frozen")})
    assert A.AGCase.from_repro(line) == old


def test_kernel_mode_reaches_every_pass():
    nf = Counter_of(A.nonfinite_cases(N_NONFINITE, SEED))
    bounded = Counter_of(A.bounded_cases(N_BOUNDED, SEED))
    large = [c for c in A.large_cases(SEED) if c.operator_gradients == "kernel"]
    for cnt in (nf, bounded, Counter_of(large)):
        assert cnt["route:opgrad_d"] >= 3 and cnt["route:opgrad_r"] >= 3
    assert bounded["opgrad:b>8"] >= 2 and nf["opgrad:b>8"] >= 1
    assert {(c.kind, c.dg.b) for c in large} >= {("grad", 1), ("div", 1), ("fm", 9)} and all(c.E == A.MULTI_TRIP_E for c in large)
    from feinsum_amd import _hip
    assert A.MULTI_TRIP_E > 64 * 1023 and _hip.opgrad_plan(A.MULTI_TRIP_E, 48)[0] == 1024      # past the slice cap
    # no other large case was added
    assert len(A.large_cases(SEED)) == 10 + len(large) and len(large) == 6


def test_bound_of_a_kernel_term_is_the_one_derived_from_the_plan():
    from feinsum_amd import _hip

    case = A.AGCase(D.DGCase("grad", 35, 15, 1, "rij", "float64", 1003, "ragged", 9), None, "auto", operator_gradients="kernel")
    n, u, rounded = A.bound_of(case.expr(), (), "R", 1003, "kernel")
    assert (n, u, rounded) == (2 + 3 * 1003 + 6 + -(-_hip.opgrad_plan(1003, 3 * 35 * 35)[0] // 64), R.U64, False)
    assert A.bound_of(case.expr(), (), "R", 1003)[0] < n                    # (today's route: a shorter chain)
    assert A.bound_of(case.expr(), (), "J", 1003, "kernel") == A.bound_of(case.expr(), (), "J", 1003)
    fm = A.AGCase(D.DGCase("fm", 35, 15, 9, "rij", "float64", 129, "ragged", 9), None, "auto", operator_gradients="kernel")
    n, _, _ = A.bound_of(fm.expr(), (), "R", 129, "kernel")
    assert n == 2 + 129 + 6 + 1 + 8                                         # nine rows summed in the kernel: eight additions


def test_checker_rejects_a_slice_of_an_operator_gradient_summed_twice():
    """dR of face-mass x 9 at E = 133 (three slices of 64 elements): the elements of one slice added once more -- a
    second launch that adds to its slice twice, or a combine that reads a slice twice."""
    case = A.AGCase(D.DGCase("fm", 10, 6, 9, "rij", "float64", 133, "ragged", 11), None, "auto", operator_gradients="kernel")
    arrays, mants, scales = A.host_data(case)
    expr = case.expr()
    ref = A.grad_reference(expr, (), mants, scales, "R", case.E)
    assert A.predicted_launches(case)["opgrad_r"] == 1
    sl = {k: (np.take(m, range(64, 128), axis=m.shape.index(case.E)) if case.E in m.shape else m) for k, m in mants.items()}
    assert sum(v.shape != mants[k].shape for k, v in sl.items()) == 1 + 9 + 9          # J, the fields, the output gradients
    twice = ref + A.grad_reference(expr, (), sl, scales, "R", 64)
    assert R.differing_entries(ref.copy(), ref) == 0 and R.differing_entries(twice, ref) > 0
    # one field's rows of the second launch (fields 8..) summed twice, and left out
    assert R.differing_entries(A.grad_reference(expr, (), mants, scales, "R", case.E, extra=(0, 8)), ref) > 0
    assert R.differing_entries(A.grad_reference(expr, (), mants, scales, "R", case.E, skip=(0, 8)), ref) > 0
    st = A.Stats("planted")
    st.fail = lambda line: setattr(st, "failures", st.failures + 1)
    assert not A._compare(st, "planted", case, {}, {"R": twice}, {}, {"R": ref}) and st.failures == 1
    assert A._compare(st, "planted", case, {}, {"R": ref.copy()}, {}, {"R": ref}) and st.failures == 1
    # a frozen operator: a gradient that shows up anyway is a failure
    frozen = A.with_kernel(case, frozen=("R",))
    assert not A._compare(st, "planted", frozen, {}, {"R": ref}, {}, {"R": None}) and st.failures == 2


def test_direct_operator_gradient_runs_and_references():
    from feinsum_amd.family import FACEMASS_ADJ_SHAPES, GEOMADJ_NP

    og = A.opgrad_runs(SEED)
    assert {(Np, lay, ol) for Np, _, _, lay, ol, _, _, _ in og} == {(Np, lay, ol) for Np in GEOMADJ_NP for lay in A.GEOM_LAYOUTS
                                                                    for ol in A.OPGRAD_OUT_LAYOUTS}
    assert {E for *_, E, _ in og} == set(A.OPGRAD_E) == set(A.KERNEL_E) | {65, 66}
    assert {X for _, X, *_ in og} == {R_ for _, _, R_, *_ in og} == {1, 2, 3} and {nk for *_, nk, _, _ in og} == {1, 2}
    assert all((lay == "xre" or X == 1) and (lay != "e" or R_ == 1) for _, X, R_, lay, *_ in og)
    fm = A.facemass_opgrad_runs(SEED)
    assert {(s, lay[2]) for s, lay, *_ in fm} == {(s, fl) for s in FACEMASS_ADJ_SHAPES for _, _, fl in A.FM_LAYOUT_FLAGS}
    assert len({fl for _, _, fl in A.FM_LAYOUT_FLAGS}) == 8
    assert {(lay[2], b) for s, lay, b, *_ in fm} >= {(fl, b) for _, _, fl in A.FM_LAYOUT_FLAGS for b in (1, 2, 4, 9)}
    assert {E for *_, E, _ in fm} == set(A.OPGRAD_E)
    pog, pfm = A.placement_opgrad_runs(SEED)
    assert set(pog) <= set(og) and set(pfm) <= set(fm)
    assert {(lay, ol) for _, _, _, lay, ol, *_ in pog} == {(lay, ol) for lay in A.GEOM_LAYOUTS for ol in A.OPGRAD_OUT_LAYOUTS}
    assert {lay[2] for _, lay, *_ in pfm} == set(range(8)) and {b for _, _, b, *_ in pfm} == {1, 2, 4, 9}
    assert {E for *_, E, _ in pog} | {E for *_, E, _ in pfm} <= set(A.OPGRAD_E)
    # the references against the einsum definitions of tests/test_gpu_opgrad.py (small integers)
    rng = np.random.default_rng(3)
    X, R_, E, Np = 2, 3, 5, 4
    J, a, b = rng.integers(-3, 4, size=(X, R_, E)), rng.integers(-3, 4, size=(2, E, Np)), rng.integers(-3, 4, size=(2, X, E, Np))
    want = sum(np.einsum("xre,eq,xep->rpq", J, a[k], b[k]) for k in range(2))
    assert np.array_equal(A.opgrad_reference(J, list(a), list(b), "xre", "rpq"), want)
    assert np.array_equal(A.opgrad_reference(J, list(a), list(b), "xre", "rqp"), want.transpose(0, 2, 1))
    one = np.einsum("xre,eq,xep->rpq", J[:1], a[0], b[0][:1])
    assert np.array_equal(A.opgrad_reference(np.ascontiguousarray(J[0].T), [a[0]], [b[0][:1]], "er", "rpq"), one)
    assert np.array_equal(A.opgrad_reference(J[0], [a[0]], [b[0][:1]], "re", "rpq"), one)
    assert np.array_equal(A.opgrad_reference(J[0, 0], [a[0]], [b[0][:1]], "e", "rpq"), one[:1])
    nf, Nfp = 4, 3
    Jf, g, v = rng.integers(-3, 4, size=(nf, E)), rng.integers(-3, 4, size=(2, E, Np)), rng.integers(-3, 4, size=(2, nf, E, Nfp))
    dR = np.einsum("kei,fe,kfej->fij", g, Jf, v)
    assert np.array_equal(A.facemass_opgrad_reference(Jf, list(g), list(v), "fe", "jfi"), dR.transpose(2, 0, 1))
    assert A.facemass_opgrad_reference(Jf, list(g), list(v), "fe", "jfi").shape == A._r_shape("jfi", nf, Np, Nfp)
    assert np.array_equal(A.facemass_opgrad_reference(Jf.T, list(g), list(v), "ef", "ifj"), dR.transpose(1, 0, 2))
    # the workspace is an output of exactly the planned bytes
    from feinsum_amd import _hip
    outs, nbytes = A._with_workspace({"out": (3, 4, 4)}, 1003, 48)
    assert nbytes == _hip.opgrad_plan(1003, 48)[1] > 0 and outs["ws"] == (nbytes // 8,) and list(outs) == ["out", "ws"]


def test_plant_sites_reach_tile_ends_and_every_role():
    import random

    case = A.AGCase(D.DGCase("fm", 35, 15, 2, "rij", "float64", 1003, "ragged", 1), None, "auto")
    expr = case.expr()
    shapes = {n: A._shape(expr, n, 1003) for n in expr.all_args}
    shapes.update({g: (1003, 35) for g in A.grad_names(expr)})
    rng = random.Random(SEED)
    elems, roles = set(), set()
    for _ in range(12):
        for role, nm, idx in A.plant_sites(case, rng, shapes):
            roles.add(role)
            spec = expr.arg_to_shape.get(nm, expr.shape)
            elems |= {i for i, d in zip(idx, spec) if not isinstance(d, int)}
    assert roles == {"field", "geometry", "operator", "output-grad"}
    assert {15, 16, 1002} <= elems


def test_kernel_runs_cover_every_shape_and_layout():
    from feinsum_amd.family import FACEMASS_ADJ_SHAPES, GEOMADJ_NP

    g = A.geomadj_runs(SEED)
    assert {(Np, lay, op) for Np, _, _, op, lay, _, _ in g} == {(Np, lay, op) for Np in GEOMADJ_NP
                                                                 for lay in A.GEOM_LAYOUTS for op in (0, 1)}
    assert {(X, R) for _, X, R, _, lay, _, _ in g if lay == "xre"} == {(x, r) for x in (1, 2, 3) for r in (1, 2, 3)}
    assert any(E == A.MULTI_TRIP_E for *_, E, _ in g)
    fm = A.facemass_runs(SEED)
    assert {(s, lay[2], b, w) for s, lay, b, w, E, _ in fm if E != A.MULTI_TRIP_E} == {(s, fl, b, w) for s in FACEMASS_ADJ_SHAPES
                                                               for _, _, fl in A.FM_LAYOUT_FLAGS for b in (1, 8, 9, 17)
                                                               for w in ("dv", "dJ", "both")}
    assert {E for *_, E, _ in fm} >= set(A.KERNEL_E) | {A.MULTI_TRIP_E}


def test_kernel_references_by_hand():
    """geomadj and the face-mass adjoint references against the einsum definitions in float64 (small integers)."""
    rng = np.random.default_rng(3)
    Dm, a, b = (rng.integers(-3, 4, size=s) for s in ((2, 4, 4), (5, 4), (3, 5, 4)))
    got = A.geomadj_reference(Dm, a, b, 1, "xre")
    want = np.einsum("rji,ej,xei->xre", Dm, a, b)
    assert np.array_equal(got, want)
    assert np.array_equal(A.geomadj_reference(Dm[:1], a, b[:1], 0, "e"), np.einsum("rij,ej,xei->e", Dm[:1], a, b[:1]))
    J, Rm = rng.integers(-3, 4, size=(4, 5)), rng.integers(-3, 4, size=(3, 4, 10))   # J 'fe', R 'jfi' (Nfp, nf, Np)
    g = [rng.integers(-3, 4, size=(5, 10)) for _ in range(2)]
    v = [rng.integers(-3, 4, size=(4, 5, 3)) for _ in range(2)]
    dv, dJ = A.facemass_references(J, Rm, g, v, "fe", "jfi")
    Rf = np.transpose(Rm, (1, 2, 0))   # (f, i, j)
    assert np.array_equal(dv[1], np.einsum("fe,fij,ei->fej", J, Rf, g[1]))
    assert np.array_equal(dJ, sum(np.einsum("fij,ei,fej->fe", Rf, gk, vk) for gk, vk in zip(g, v)))
