"""The references of the DG sweep (oracle/einsum_ref.py) and its case lists (tools/fuzz_dg.py), without a GPU: the bit
budgets per array name hold for every row and stage that reads the array, the range cases stay inside their exponent
windows, dependency sets match hand-checked ones, the checkers reject planted errors, and the fixed-seed case lists
reach every coverage minimum."""

import math
import sys
from pathlib import Path

import numpy as np
import pytest

from oracle import einsum_ref as R

sys.path.insert(0, str(Path(__file__).resolve().parents[1] / "tools"))
import fuzz_dg as D  # noqa: E402

SEED = 20261016   # tests/test_gpu_dg_exact.py sweeps the same cases
N_EXACT, N_BOUNDED, N_NONFINITE, N_POISON = 120, 60, 24, 16


def _rows(case):
    """(keys, terms per entry, significand) of every row of every stage."""
    out = []
    for expr, keys in case.stages():
        for row in expr.args:
            out.append(([keys[a.name] for a in row], D._terms(expr)))
    return out


def _worst(bits, names, n_terms):
    w = max(int(n_terms), 1)
    for nm in names:
        w *= (1 << bits[nm]) - 1
    return w


# --------------------------------------------------------------------------
# bit budgets per array name
# --------------------------------------------------------------------------

def test_shared_array_budgets_hold_for_every_row_and_stage():
    """Every case of the exact sweep: for each row of each stage, the worst absolute sum of mantissa products (Python
    integers) fits the significand; float32 arrays fit float32; the budget is spent (one more bit in any array
    breaks some row); and arrays shared by several rows or stages exist among the cases."""
    shared = 0
    for case in D.gen_cases(N_EXACT, SEED):
        rng = np.random.default_rng(case.seed)
        bits, scales, dtypes, sig = D.plan_data(case, rng)
        rows = _rows(case)
        for names, n_terms in rows:
            assert _worst(bits, names, n_terms) <= (1 << sig), (case, names)
        for k, b in bits.items():
            assert 1 <= b <= (24 if dtypes[k] == np.dtype("float32") else sig)
            if b < (24 if dtypes[k] == np.dtype("float32") else sig):
                more = {**bits, k: b + 1}
                assert not R.rows_fit(rows, more, sig), (case, k)
        uses = {}
        for names, _ in rows:
            for nm in names:
                uses[nm] = uses.get(nm, 0) + 1
        shared += any(v > 1 for v in uses.values())
    assert shared >= 40


def test_shared_budget_small_hand_case():
    """Two stages reading J and R: one sums 9 terms, the other 3; J and R fit the 9-term row, u1 may be wider."""
    rows = [(["J", "R", "u0"], 9), (["J", "R", "u1"], 3)]
    bits = R.shared_exact_bits(rows, [], 20, np.random.default_rng(1))
    assert ((1 << bits["J"]) - 1) * ((1 << bits["R"]) - 1) * ((1 << bits["u0"]) - 1) * 9 <= 1 << 20
    assert ((1 << bits["J"]) - 1) * ((1 << bits["R"]) - 1) * ((1 << bits["u1"]) - 1) * 3 <= 1 << 20
    assert bits["u1"] >= bits["u0"]
    f32 = R.shared_exact_bits([(["a", "b"], 1)], ["a", "b"], 53, np.random.default_rng(2))
    assert max(f32.values()) <= 24


def test_exact_reference_is_the_float64_einsum_and_leaves_float32_behind():
    """On the generated data the int64 reference equals numpy's float64 einsum (exact data: every partial sum fits),
    and most float64 cases have an entry wider than 24 bits."""
    wide = total = 0
    for case in D.gen_cases(N_EXACT, SEED)[:60]:
        if case.E > 1100 or case.scale != "normal":
            continue
        arrays, mants, scales, sig = D.host_data(case)
        for expr, keys in case.stages():
            for row in expr.args:
                ks = [keys[a.name] for a in row]
                out_dt = np.float32 if case.dtype == "float32" else np.float64
                ref = R.int_reference(expr.get_subscripts(), [mants[k] for k in ks], sum(scales[k] for k in ks),
                                      out_dt, sig)
                f64 = np.einsum(expr.get_subscripts(), *[arrays[k].astype(np.float64) for k in ks], optimize=True)
                assert R.bitwise_equal(ref, f64.astype(out_dt))
        if sig == 53:
            total += 1
            wide += R.needs_more_than_f32(D._host_probe(case, mants, scales, sig))
    assert total >= 10 and wide >= 0.8 * total


# --------------------------------------------------------------------------
# range cases
# --------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("kind", ["overflow", "subnormal"])
def test_range_case_budgets(dtype, kind):
    """Scales of one sign; overflow totals stay below 2^900 / 2^100 and above half of that; subnormal totals are the
    subnormal quantum and every sum stays below the smallest normal (fixed-point arithmetic: exact)."""
    top, quantum = R.RANGE[np.dtype(dtype)]
    for seed in range(20):
        rng = np.random.default_rng(seed)
        case = D.DGCase("bdiv", 20, 10, 3, "rij", dtype, 33, "ragged", seed, kind)
        bits, scales, dtypes, sig = D.plan_data(case, rng)
        assert all((s >= 0) if kind == "overflow" else (s <= 0) for s in scales.values())
        for names, n_terms in _rows(case):
            total = sum(scales[nm] for nm in names)
            worst = _worst(bits, names, n_terms)
            if kind == "overflow":
                assert total + worst.bit_length() <= top and total >= top - (53 if dtype == "float64" else 24)
            else:
                assert total == quantum
                min_normal = -1022 if dtype == "float64" else -126
                assert worst < (1 << (min_normal - quantum))
        arrays, mants, scales, sig = D.host_data(case)
        for k, a in arrays.items():   # every operand exact in its dtype
            assert np.array_equal(np.ldexp(a.astype(np.float64), -scales[k]), mants[k].astype(np.float64))
            assert np.isfinite(a).all()


def test_subnormal_reference_is_subnormal_and_exact():
    case = D.DGCase("grad", 10, 6, 1, "rij", "float64", 17, "ragged", 5, "subnormal")
    arrays, mants, scales, sig = D.host_data(case)
    expr, keys = case.stages()[0]
    ks = [keys[a.name] for a in expr.args[0]]
    ref = R.int_reference(expr.get_subscripts(), [mants[k] for k in ks], sum(scales[k] for k in ks), np.float64, sig)
    nz = ref[ref != 0]
    assert nz.size and (np.abs(nz) < np.finfo(np.float64).tiny).all()
    assert R.bitwise_equal(ref, np.einsum(expr.get_subscripts(), *[arrays[k] for k in ks], optimize=True))


# --------------------------------------------------------------------------
# dependency sets
# --------------------------------------------------------------------------

def test_dependency_sets_by_hand():
    E, Np = 5, 4
    grad = ("xre,rij,ej->xei", [(3, 3, E), (3, Np, Np), (E, Np)])
    dep = R.dependency_set(*grad, 2, (1, 2))               # u[e=1, j=2]: every x, i of element 1
    want = np.zeros((3, E, Np), bool)
    want[:, 1, :] = True
    assert np.array_equal(dep, want)
    dep = R.dependency_set(*grad, 1, (0, 3, 1))            # R[r=0, i=3, j=1]: row i = 3 of every element
    want = np.zeros((3, E, Np), bool)
    want[:, :, 3] = True
    assert np.array_equal(dep, want)
    dep = R.dependency_set(*grad, 0, (2, 1, 4))            # J[x=2, r=1, e=4]: direction 2 of element 4
    want = np.zeros((3, E, Np), bool)
    want[2, 4, :] = True
    assert np.array_equal(dep, want)
    fm = ("ef,fij,fej->ei", [(E, 4), (4, Np, 3), (4, E, 3)])
    dep = R.dependency_set(*fm, 1, (2, 0, 1))              # R[f, i=0, j]: column 0 of every element
    want = np.zeros((E, Np), bool)
    want[:, 0] = True
    assert np.array_equal(dep, want)
    dep = R.dependency_set("e,ij,ej->ei", [(E,), (Np, Np), (E, Np)], 0, (3,))
    want = np.zeros((E, Np), bool)
    want[3] = True
    assert np.array_equal(dep, want)


# --------------------------------------------------------------------------
# the checkers reject planted errors
# --------------------------------------------------------------------------

def _small_exact():
    case = D.DGCase("grad", 10, 6, 1, "rij", "float64", 17, "ragged", 3)
    arrays, mants, scales, sig = D.host_data(case)
    expr, keys = case.stages()[0]
    ks = [keys[a.name] for a in expr.args[0]]
    ref = R.int_reference(expr.get_subscripts(), [mants[k] for k in ks], sum(scales[k] for k in ks), np.float64, sig)
    return expr, ks, ref


def test_checkers_reject_planted_errors():
    expr, ks, ref = _small_exact()
    assert R.bitwise_equal(ref.copy(), ref)
    ulp = ref.copy()
    k = int(np.argmax(np.abs(ulp)))
    ulp.flat[k] = np.nextafter(ulp.flat[k], np.inf)
    assert not R.bitwise_equal(ulp, ref)
    swapped = ref.copy()
    a, b = swapped[0, 3].copy(), swapped[0, 4].copy()
    assert not np.array_equal(a, b)
    swapped[0, 3], swapped[0, 4] = b, a
    assert not R.bitwise_equal(swapped, ref)
    # non-finite rule: R[0, 2, 0] = NaN reaches row i = 2 of every element
    shapes = [(3, 3, 17), (3, 10, 10), (17, 10)]
    dep = R.dependency_set(expr.get_subscripts(), shapes, 1, (0, 2, 0))
    good = np.where(dep, np.nan, ref)
    assert R.nonfinite_violations(good, ref, dep, math.nan) == 0
    stray = good.copy()
    stray[1, 5, 1] = np.nan                                   # a NaN outside the set (row 1: a padded neighbour)
    assert R.nonfinite_violations(stray, ref, dep, math.nan) >= 1
    finite = good.copy()
    finite[0, 0, 2] = 0.0                                     # a finite entry inside the set
    assert R.nonfinite_violations(finite, ref, dep, math.nan) >= 1
    inf = np.where(dep, np.inf, ref)
    inf[2, 3, 2] = np.nan                                     # for an Inf: NaN or either infinity inside the set
    assert R.nonfinite_violations(inf, ref, dep, math.inf) == 0
    off = inf.copy()
    off[2, 3, 1] = np.nextafter(off[2, 3, 1], -np.inf)        # one ulp outside the set
    assert R.nonfinite_violations(off, ref, dep, math.inf) >= 1


def test_tensor_checkers_the_sweep_uses():
    """The GPU sweep decides with ``differing_entries`` and ``nonfinite_violations`` on torch tensors: the same
    rejections as on numpy arrays."""
    torch = pytest.importorskip("torch")
    expr, ks, ref = _small_exact()
    r = torch.from_numpy(ref)
    assert R.differing_entries(r.clone(), r) == 0
    z = r.clone()
    z[z == 0] = -0.0
    assert R.differing_entries(z, r) == 0
    ulp = r.clone()
    ulp[0, 0, 0] = torch.nextafter(ulp[0, 0, 0], torch.tensor(math.inf, dtype=torch.float64))
    assert R.differing_entries(ulp, r) == 1
    sw = r.clone()
    sw[0, 3], sw[0, 4] = r[0, 4].clone(), r[0, 3].clone()
    assert R.differing_entries(sw, r) > 0
    assert R.differing_entries(r.float(), r) == r.numel()
    nan = r.clone()
    nan[1, 1, 1] = math.nan
    assert R.differing_entries(nan, r) == 1
    dep = torch.from_numpy(R.dependency_set(expr.get_subscripts(), [(3, 3, 17), (3, 10, 10), (17, 10)], 1, (0, 2, 0)))
    good = torch.where(dep, torch.tensor(math.nan, dtype=torch.float64), r)
    assert R.nonfinite_violations(good, r, dep, math.nan) == 0
    stray = good.clone()
    stray[1, 5, 1] = math.nan                                 # a NaN in row 1: next to the planted row's start
    assert R.nonfinite_violations(stray, r, dep, math.nan) >= 1
    finite = good.clone()
    finite[0, 0, 2] = 0.0
    assert R.nonfinite_violations(finite, r, dep, math.nan) >= 1
    inf = torch.where(dep, torch.tensor(-math.inf, dtype=torch.float64), r)
    inf[2, 3, 2] = math.nan
    assert R.nonfinite_violations(inf, r, dep, -math.inf) == 0
    inf[2, 3, 1] = math.inf
    assert R.nonfinite_violations(inf, r, dep, -math.inf) >= 1


def test_padding_sites_cover_the_reads_past_a_row_end():
    """grad's padding column j = Np and div's asmall build read the next row's first entries (or the next plane's):
    those entries are planted for every padded order, both layouts, grad and div."""
    for Np in D.PADDED_ORDERS:
        rij = set(D.padding_sites(Np, "rij"))
        assert {(r, i, 0) for r in range(3) for i in (1, Np - 1)} <= rij          # R[r, i + 1, 0] behind row i
        assert {(1, 0, 0), (2, 0, 0), (1, 0, 2)} <= rij                          # R[r + 1, 0, 0] behind the plane
        rji = set(D.padding_sites(Np, "rji"))
        assert {(r, c, i) for r in (1, 2) for c in range(min(3, Np)) for i in (0, Np - 1)} <= rji
    cases = D.padding_cases(SEED)
    assert {(c.kind, c.Np, c.op) for c in cases} == {(k, n, o) for k in ("grad", "div") for n in D.PADDED_ORDERS
                                                      for o in ("rij", "rji")}
    assert all(c.dtype == "float64" and c.E >= 16 for c in cases)


def test_large_cases_force_the_quarter_tail():
    forced = [(c, k) for c, k in D.large_cases(SEED) if k.get("quarter_tail") and k.get("tail_rounds") == -1
              and not k.get("prepared") and k.get("staggered_start") is False]
    assert {(c.kind, c.op, c.E) for c, _ in forced} >= {(k, o, E) for E in D.QUARTER_E
                                                         for k, o in (("grad", "rij"), ("grad", "rji"), ("div", "rij"))}


def test_bound_rejects_a_lost_term_on_signed_data():
    rng = np.random.default_rng(7)
    subs = "xre,rij,xej->ei"
    ops = [(rng.random(s) * 2 - 1) for s in [(3, 3, 40), (3, 35, 35), (3, 40, 35)]]
    ref, absref = R.bounded_reference(subs, ops)
    n = R.bound_terms(subs, {"x": 3, "r": 3, "e": 40, "i": 35, "j": 35}, 3)
    got = np.einsum(subs, *ops, optimize=True)
    assert R.bound_ratio(got, ref, absref, n, R.U64) <= 1
    assert R.bound_ratio(got.astype(np.float32).astype(np.float64), ref, absref, n, R.U64) > 1
    lost = got - np.outer(ops[0][0, 0] * ops[2][0, :, 0], ops[1][0, :, 0])   # the term x = r = j = 0 dropped
    assert R.bound_ratio(lost, ref, absref, n, R.U64) > 1


# --------------------------------------------------------------------------
# coverage of the fixed-seed case lists
# --------------------------------------------------------------------------

def test_case_lists_reach_every_minimum():
    cnt = D.coverage(D.gen_cases(N_EXACT, SEED))
    assert not D.missing_buckets(cnt, D.MINIMUMS), D.missing_buckets(cnt, D.MINIMUMS)
    classes = {c: 0 for c in D.E_CLASSES}
    for case in D.gen_cases(N_EXACT, SEED):
        classes[case.eclass] = classes.get(case.eclass, 0) + 1
    assert all(v >= 2 for v in classes.values()), classes


def test_large_cases_cover_every_launch_and_knob():
    cases = D.large_cases(SEED)
    kinds = {(c.kind, c.op) for c, _ in cases if c.dtype == "float64"}
    assert {("grad", "rij"), ("grad", "rji"), ("div", "rij"), ("fm", "rij"), ("fm_ifj", "rij"), ("fm_jfi", "rij"),
            ("fm_fji", "rij"), ("bgrad", "rij"), ("bdiv", "rij"), ("pipeline", "rij")} <= kinds
    assert {c.E for c, _ in cases} >= set(D.LARGE_E) | {70_004, 1_000_004}
    seen = {(k, repr(v)) for _, kn in cases for k, v in kn.items()}
    for want in [("tail_rounds", "-1"), ("tail_rounds", "None"), ("quarter_tail", "True"), ("quarter_tail", "False"),
                 ("staggered_start", "True"), ("staggered_start", "False"), ("temporal_loads", "0"),
                 ("temporal_loads", "248"), ("write_through", "4096"), ("prepared", "True"), ("alloc", "'split'"),
                 ("alloc", "'torch'")]:
        assert want in seen, want


def test_plant_sites_reach_tile_ends_and_the_last_element():
    import random

    rng = random.Random(SEED)
    case = D.DGCase("grad", 35, 15, 1, "rij", "float64", 100_007, "quarter-tail", 1)
    sites = D.plant_sites(case, rng)
    roles = {r for r, _, _ in sites}
    assert roles == {"field", "geometry", "operator"}
    elems = {idx[0] for r, k, idx in sites if r == "field"}
    assert {0, 15, 63, 100_006} <= elems and any(90_000 < e < 100_006 for e in elems)
