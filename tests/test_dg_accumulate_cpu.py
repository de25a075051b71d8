"""The accumulating pass of the DG sweep (tools/fuzz_dg.py ``run_accumulate``: ``out <- alpha E + beta out`` on the routes
"kernel", "epilogue" and "axpby") without a GPU: the case lists reach every coverage minimum, every ``REPRO`` line
round-trips, the host route prediction is ``measure.accumulate_route``, the combine references agree with ``Fraction``
arithmetic, the bit budget keeps power-of-two pairs exact and the range cases finite, and the checkers reject planted
errors."""

import math
import sys
from fractions import Fraction
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parents[1] / "tools"))
import fuzz_dg as D  # noqa: E402
from feinsum_amd.measure import accumulate_route  # noqa: E402

SEED = 20261019   # tests/test_gpu_dg_accumulate.py sweeps the same cases

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def cases():
    return D.acc_cases(SEED)


# --------------------------------------------------------------------------
# the case lists
# --------------------------------------------------------------------------

def test_case_list_reaches_every_minimum(cases):
    missing = D.missing_buckets(D.acc_coverage(cases), D.ACC_MINIMUMS)
    assert not missing, missing
    bounded = D.acc_coverage(D.acc_bounded_cases(SEED))
    for r in ("axpby", "kernel", "epilogue"):
        assert bounded[f"route:{r}"] >= 40
    assert bounded["factors:pow2"] >= 100 and bounded["factors:general"] >= 30
    assert all(ac.case.E <= 1100 and ac.case.scale == "normal" for ac in D.acc_bounded_cases(SEED))


def test_minimums_name_what_the_pass_is_meant_to_run():
    m = D.ACC_MINIMUMS
    assert {f"family:{k}" for k in D.KINDS} <= set(m) and "family:pipeline" not in m
    assert {f"route:{r}:3d-{n}" for r in ("kernel", "epilogue") for n in (4, 10, 20, 35)} <= set(m)
    assert {f"route:axpby:3d-{n}" for n, _ in D.ORDERS3} <= set(m)
    assert len(D.ACC_FM_KINDS) == 8
    assert {f"fm-layout:{jl}:{rl}:p{p}" for jl in ("ef", "fe") for rl in ("fij", "ifj", "fji", "jfi") for p in (1, 2, 3, 4)} <= set(m)
    assert {f"op:{fam}:{op}:p{p}" for fam in ("grad", "div") for op in ("rij", "rji") for p in (1, 2, 3, 4)} <= set(m)
    assert D.ACC_PAIRS[:6] == ((1.0, 1.0), (-1.0, 1.0), (2.0, -0.5), (0.5, 0.0), (0.0, 1.0), (0.0, 0.0))      # AB of test_gpu_accumulate.py
    assert (0.3, -1.7) in D.ACC_PAIRS and any(abs(a) < 1 < abs(b) and not D.is_pow2(a) for a, b in D.ACC_PAIRS)
    assert any(D.is_pow2(a) and D.is_pow2(b) and abs(b) >= 32 and a < 0 for a, b in D.ACC_PAIRS)
    assert {f"pair:{a:g},{b:g}:{r}" for a, b in D.ACC_PAIRS for r in ("axpby", "kernel", "epilogue")} <= set(m)
    assert {"dtype:float64", "dtype:float32", "dtype:mixed", "range:overflow", "range:subnormal"} <= set(m)
    assert {f"transform:{t}:axpby" for t in D.TRANSFORMS} <= set(m)
    assert {f"fm-fields:{b}" for b in (1, 2, 3, 4, 5, 8, 9)} <= set(m)
    assert {f"size:{fam}:p{p}:{s}" for fam in ("fm", "grad", "div") for p in (1, 2, 3, 4) for s in D.TEL_SIZES} <= set(m)
    assert {f"planted:{r}:{v}:{b}" for r in ("field", "geometry", "operator", "old") for v in (math.nan, math.inf, -math.inf)
            for b in ("beta=0", "beta!=0")} <= set(D.ACC_PLANT_MINIMUMS)
    assert {f"accplace:{fam}:p{p}:{pl}" for fam in ("fm", "grad", "div") for p in (1, 2, 3, 4)
            for pl in ("only:field", "only:output")} <= set(D.ACC_PLACEMENT_MINIMUMS)
    assert all(v >= 1 for mm in (m, D.ACC_PLANT_MINIMUMS, D.ACC_PLACEMENT_MINIMUMS) for v in mm.values())


def test_no_case_exceeds_the_second_tile_size(cases):
    named = [ac for ac in cases if ac.case.E < 0]
    assert named and all(ac.case.eclass in D.TEL_SIZES + ("second-tile",) and ac.family() for ac in named)
    assert {(ac.family(), ac.case.Np) for ac in named if ac.case.eclass == "second-tile"} == {("fm", 35), ("grad", 35), ("div", 35)}
    assert max(ac.case.E for ac in cases) == 20_004
    assert all(ac.case.E <= 4099 for ac in cases if ac.case.scale != "normal" or ac.case.E != 20_004)
    assert all(ac.case.kind != "pipeline" for ac in cases)


def test_plants_and_placements_reach_their_minimums():
    from collections import Counter

    cnt = Counter()
    for ac, role, value in D.acc_plants(SEED):
        assert D.predicted_route(ac) is not None
        cnt.update(D.acc_plant_buckets(ac, role, value))
    assert not D.missing_buckets(cnt, D.ACC_PLANT_MINIMUMS)
    for part in ("exact", "signed"):
        assert not D.missing_buckets(D.acc_placement_coverage(SEED, part), D.ACC_PLACEMENT_MINIMUMS)
        for runs in D.acc_placement_runs(SEED, part):
            ac = D._acc_of(runs[0])
            route = D.predicted_route(ac)
            assert route == (ac.route or route) and route is not None and runs[0].placement == "aligned"
            assert ac.case.E <= 1003 and (part == "signed") == (not ac.pow2())
            names = [r.placement for r in runs]
            assert set(names) >= ({"aligned", "all", "mixed", "only:field", "only:output", "only:geometry", "only:operator"}
                                  if route != "axpby" else {"aligned", "all"})
    # "only:field" leaves every output aligned, "only:output" every field
    for runs in D.acc_placement_runs(SEED, "exact"):
        for r in runs:
            if r.placement == "only:field":
                assert len(r.shifts) == 1 and not r.shifts[0][0].startswith("out:")
            if r.placement == "only:output":
                assert len(r.shifts) == 1 and r.shifts[0][0].startswith("out:")


def test_every_repro_line_round_trips(cases):
    for ac in cases:
        back = D.AccCase.from_repro(ac.repro())
        assert back == ac and back.repro() == ac.repro()
        assert (back.alpha, back.beta, back.route, back.transform, back.old_shift) == \
            (ac.alpha, ac.beta, ac.route, ac.transform, ac.old_shift)
        assert D.acc_transform(back) == D.acc_transform(ac)
    n = 0
    for part in ("exact", "signed"):
        for runs in D.acc_placement_runs(SEED, part):
            for run in runs:
                back = D.PlacedRun.from_repro(run.repro())
                assert back == run and back.repro() == run.repro() and back.acc == run.acc and dict(back.shifts) == dict(run.shifts)
                assert D._acc_of(back) == D._acc_of(run)
                n += 1
    assert n > 250
    # a run of the plain placement pass keeps its line
    plain = D.PlacedRun(cases[0].case, "exact", "auto", "aligned")
    assert "accumulate" not in plain.repro() and D.PlacedRun.from_repro(plain.repro()) == plain


def test_route_prediction_is_accumulate_route(cases):
    seen = set()
    for ac in cases:
        expr, _ = ac.case.stages()[0]
        t = D.acc_transform(ac)
        assert (t or {}).get("accumulate") == ac.route
        try:
            D.launch_kind(expr, t, {"E": max(ac.case.E, 1)})
            want = accumulate_route(expr, t)
        except NotImplementedError:
            want = None
        assert D.predicted_route(ac) == want
        if ac.route is not None and want is not None:
            assert want == ac.route
        seen.add((ac.route, want))
    assert seen >= {(None, "kernel"), (None, "axpby"), ("axpby", "axpby"), ("kernel", "kernel"), ("epilogue", "epilogue"),
                    ("kernel", None), ("epilogue", None)}
    # face-mass of tetrahedra: a single field takes the fallback by default, nine go to the kernel in several groups
    by_b = {ac.case.b: D.predicted_route(ac) for ac in cases if ac.case.kind == "fm" and ac.route is None
            and ac.case.dtype == "float64" and (ac.case.Np, ac.case.Nfp) in D.TET_ORDERS}
    assert by_b[1] == "axpby" and all(by_b[b] == "kernel" for b in (2, 3, 4, 5, 8, 9))


# --------------------------------------------------------------------------
# the combine reference
# --------------------------------------------------------------------------

def _fraction_combine(ms, t, alpha, beta, old, dtype):
    """fl(alpha E + fl(beta old)) by Fractions; float64 only (``float(Fraction)`` rounds correctly)."""
    p = float(Fraction(beta) * Fraction(old)) if beta != 0 else 0.0
    return float(Fraction(alpha) * Fraction(ms) * Fraction(2) ** t + Fraction(p))


def test_combine_entry_agrees_with_fractions_on_hand_made_entries():
    tiny = 2.0 ** -1074
    entries = [(3, 0, 0.3, -1.7, 5.0), (-(2 ** 44) + 1, -7, 0.3, -1.7, 1234.5678), ((1 << 45) - 1, 3, -0.7, 2.3, -9.75e4),
               (12345, -1074, 0.5, -0.5, 3 * tiny),          # subnormal: beta old = 1.5 quanta rounds to 2, the sum rounds again
               (7, -1074, -0.125, 32.0, 5 * tiny), (1, -1074, 0.5, 0.0, math.nan), (0, 0, 0.3, -1.7, 0.1),
               (2 ** 30 + 1, 850, 2.0, -0.5, 2.0 ** 880 * 3)]
    for ms, t, alpha, beta, old in entries:
        assert D.combine_entry(ms, t, alpha, beta, old, np.float64) == _fraction_combine(ms, t, alpha, beta, old, np.float64), (ms, t)
    # the subnormal entry by hand: p = fl(-0.5 * 3 q) = -2 q (tie to even), 0.5 * 12345 q - 2 q = 6170.5 q -> 6170 q
    assert D.combine_entry(12345, -1074, 0.5, -0.5, 3 * tiny, np.float64) == 6170 * tiny
    # float32: one rounding from the exact value, not through float64 -- a value that double rounding gets wrong
    ms = (1 << 24) + 1                                # 2^24 + 1 + 2^-30: just above a float32 tie
    got = D.combine_entry(ms, 0, 1.0, 1.0, 2.0 ** -30, np.float32)
    assert got == float(2 ** 24 + 2) and float(np.float32(np.float64(ms) + 2.0 ** -30)) == float(2 ** 24)
    assert D.combine_entry(3, -149, 0.5, 0.0, 0.0, np.float32) == 2 * 2.0 ** -149          # 1.5 quanta of float32: to even
    assert D.fl_int(1, 1024, np.float64) == math.inf and D.fl_int(-1, 128, np.float32) == -math.inf


def test_whole_array_reference_agrees_with_the_entrywise_one():
    rng = np.random.default_rng(5)
    for dt, sig in ((np.float64, 53), (np.float32, 24)):
        ops = sig - D.ACC_HEADROOM
        ob = D.acc_old_bits(ops)
        quantum = D.FORMAT[np.dtype(dt)][1]
        for t in (0, -9, quantum, quantum + 2, 60):
            for sh in D.ACC_OLD_SHIFTS:
                ms = rng.integers(-(1 << ops) + 1, 1 << ops, size=40)
                mo = rng.integers(-(1 << ob) + 1, 1 << ob, size=40)
                old = np.ldexp(mo.astype(np.float64), t + sh).astype(dt)
                for alpha, beta in [p for p in D.ACC_PAIRS if D.is_pow2(p[0]) and D.is_pow2(p[1])]:
                    whole = D.combine_pow2(ms, t, alpha, beta, mo, t + sh, dt)
                    each = [D.combine_entry(int(m), t, alpha, beta, float(o), dt) for m, o in zip(ms, old)]
                    assert whole.dtype == np.dtype(dt) and np.array_equal(whole, np.array(each, dtype=dt)), (dt, t, sh, alpha, beta)
                    if t > quantum + 4:      # the normal range: the budget makes plain arithmetic exact
                        plain = dt(alpha) * np.ldexp(ms.astype(np.float64), t).astype(dt) + dt(beta) * old
                        assert np.array_equal(whole, plain)
    # in the subnormal range beta * old rounds, and the reference applies it (IEEE product as a second witness)
    mo = np.arange(-9, 10)
    old = np.ldexp(mo.astype(np.float64), -1074)
    p = D.round_to_format(-mo, -1075, np.float64)
    assert np.array_equal(p, -0.5 * old) and not np.array_equal(p * 2, -old)


def test_bit_budget_keeps_power_of_two_pairs_exact_and_the_range_cases_finite(cases):
    for out_sig in (53, 24):
        for sub in (0, 4):
            assert D.acc_budget_ok(out_sig - D.ACC_HEADROOM - sub, out_sig)
    assert not D.acc_budget_ok(53, 53)
    done = set()
    for ac in cases:
        if ac.case.scale == "normal" or ac.case in done:
            continue
        done.add(ac.case)
        case = ac.case
        arrays, mants, scales, sig = D.host_data(case, headroom=D.ACC_HEADROOM)
        expr, keys = case.stages()[0]
        t = sum(scales[keys[a.name]] for a in expr.args[0])
        ms = np.einsum(expr.get_subscripts(), *[mants[keys[a.name]] for a in expr.args[0]], optimize=True)
        dt = ac.out_dtype()
        for sh in D.ACC_OLD_SHIFTS:
            mo, old = D.acc_old(case, sig, t, sh, dt)[0]
            assert np.isfinite(old).all()
            for other in [a for a in cases if a.case == case]:
                alpha, beta = other.factors()
                if other.pow2():
                    want = D.combine_pow2(ms, t, alpha, beta, mo, t + sh, dt)
                else:
                    want = D.acc_general_reference(other, ms.reshape(-1)[:64], t, old.reshape(-1)[:64])
                assert np.isfinite(want).all() and want.dtype == dt
                if case.scale == "overflow" and alpha:
                    assert np.abs(want).max() > (2.0 ** 800 if dt == np.float64 else 2.0 ** 60)
                if case.scale == "subnormal":
                    assert np.abs(want).max() < (2.0 ** -1022 if dt == np.float64 else 2.0 ** -126)
    assert {(c.dtype, c.scale) for c in done} == {(d, s) for d in ("float64", "float32") for s in ("overflow", "subnormal")}


def test_sample_index():
    case = D.DGCase("grad", 10, 6, 1, "rij", "float64", 1003, "ragged", 3)
    expr, _ = case.stages()[0]
    idx = D._sample_index(case, expr, (3, 1003, 10))
    e = (idx // 10) % 1003
    assert set(range(D.ACC_EDGE)) | set(range(1003 - D.ACC_EDGE, 1003)) <= set(e.tolist())
    assert 3 * 2 * D.ACC_EDGE * 10 <= len(idx) <= 3 * 2 * D.ACC_EDGE * 10 + D.ACC_SAMPLE and len(set(idx.tolist())) == len(idx)
    small = D.DGCase("grad", 10, 6, 1, "rij", "float64", 129, "ragged", 3)
    assert len(D._sample_index(small, expr, (3, 129, 10))) == 3 * 129 * 10


# --------------------------------------------------------------------------
# the checkers reject planted errors
# --------------------------------------------------------------------------

class _Quiet(D.Stats):
    def __init__(self):
        super().__init__("planted")
        self.lines = []

    def fail(self, line):
        self.failures += 1
        self.lines.append(line)


@pytest.fixture()
def cpu_cuda(monkeypatch):
    monkeypatch.setattr(torch.Tensor, "cuda", lambda self, *a, **k: self)
    return torch


def _problem(alpha, beta, E=17, dtype="float64"):
    case = D.DGCase("grad", 10, 6, 1, "rij", dtype, E, "ragged", 11)
    ac = D.AccCase(case, alpha, beta, "epilogue")
    arrays, mants, scales, sig = D.host_data(case, headroom=D.ACC_HEADROOM)
    expr, keys = case.stages()[0]
    t = sum(scales[keys[a.name]] for a in expr.args[0])
    name = expr.output_names[0]
    sums = {name: np.einsum(expr.get_subscripts(), *[mants[keys[a.name]] for a in expr.args[0]], optimize=True)}
    olds = D.acc_old(case, sig, t, 0, ac.out_dtype())
    return ac, name, sums, t, olds


def _check(ac, name, got, sums, t, olds):
    st = _Quiet()
    D.acc_check_exact(torch, st, ac, "planted", {name: torch.from_numpy(got)}, None, sums, t, olds)
    return st


def test_checker_rejects_an_unfused_combine(cpu_cuda):
    """mul, mul, add where that is one ulp off the contract's fma(alpha, E, fl(beta old))."""
    ac, name, sums, t, olds = _problem(0.3, -1.7)
    E = np.ldexp(sums[name].astype(np.float64), t)
    old = olds[0][1]
    right = np.array([D.combine_entry(int(m), t, 0.3, -1.7, float(o), np.float64)
                      for m, o in zip(sums[name].reshape(-1), old.reshape(-1))]).reshape(E.shape)
    unfused = 0.3 * E + -1.7 * old
    differ = unfused != right
    one_ulp = differ & ((unfused == np.nextafter(right, np.inf)) | (unfused == np.nextafter(right, -np.inf)))
    assert one_ulp.any()          # (more than one ulp only where the two terms cancel)
    assert _check(ac, name, right, sums, t, olds).failures == 0
    st = _check(ac, name, unfused, sums, t, olds)
    assert st.failures == 1 and st.exact_equal == 0 and f"{int(differ.sum())} entries differ" in st.lines[0] and ac.repro() in st.lines[0]
    one = right.copy()
    at = tuple(np.argwhere(one_ulp)[0])
    one[at] = unfused[at]
    assert _check(ac, name, one, sums, t, olds).failures == 1


def test_checker_rejects_beta_applied_to_a_neighbouring_entry(cpu_cuda):
    ac, name, sums, t, olds = _problem(2.0, -0.5)
    mo, old = olds[0]
    right = D.combine_pow2(sums[name], t, 2.0, -0.5, mo, t, np.float64)
    assert _check(ac, name, right, sums, t, olds).failures == 0
    E = np.ldexp(sums[name].astype(np.float64), t)
    shifted = np.roll(old.reshape(-1), -1).reshape(old.shape)          # the 8 bytes behind each entry
    wrong = 2.0 * E - 0.5 * shifted
    assert (wrong != right).any()
    assert _check(ac, name, wrong, sums, t, olds).failures == 1
    # one chunk only
    one = right.copy()
    one.reshape(-1)[34:36] = wrong.reshape(-1)[34:36]
    assert (one != right).any() and _check(ac, name, one, sums, t, olds).failures == 1


def test_checker_rejects_an_old_value_that_shows_through_with_beta_zero(cpu_cuda):
    ac, name, sums, t, olds = _problem(0.5, 0.0)
    mo, old = olds[0]
    right = D.combine_pow2(sums[name], t, 0.5, 0.0, mo, t, np.float64)
    assert np.array_equal(right, 0.5 * np.ldexp(sums[name].astype(np.float64), t))
    assert _check(ac, name, right, sums, t, olds).failures == 0
    at = tuple(np.argwhere(old != 0)[0])
    leak = right.copy()
    leak[at] += old[at]
    assert _check(ac, name, leak, sums, t, olds).failures == 1
    # the non-finite pass: poison that shows in one entry breaks the rule, there and nowhere else
    clean = torch.from_numpy(right)
    dep = torch.zeros(clean.shape, dtype=torch.bool)
    for poison in (math.nan, math.inf):
        got = clean.clone()
        got[at] = poison
        assert D.acc_check_plant(ac, "old", math.nan, clean, clean, dep) == 0
        assert D.acc_check_plant(ac, "old", math.nan, got, clean, dep) >= 1


def test_alpha_zero_rule_asks_for_nan():
    """alpha = 0 and a planted Inf in an input: the dependency set must be NaN (0 * Inf); +-Inf there breaks the rule."""
    ac = D.AccCase(D.DGCase("grad", 10, 6, 1, "rij", "float64", 5, "sub-tile", 1), 0.0, 1.0, "epilogue")
    clean = torch.ones(3, 5, 10, dtype=torch.float64)
    dep = torch.zeros(3, 5, 10, dtype=torch.bool)
    dep[:, 2, :] = True
    got = clean.clone()
    got[dep] = math.nan
    assert D.acc_check_plant(ac, "field", math.inf, got, clean, dep) == 0
    got[dep] = math.inf
    assert D.acc_check_plant(ac, "field", math.inf, got, clean, dep) == 30
    assert D.acc_check_plant(D.AccCase(ac.case, 1.0, 1.0, "epilogue"), "field", math.inf, got, clean, dep) == 0
    assert D.acc_check_plant(ac, "geometry", math.inf, clean, clean, dep) == 30          # alpha = 0 that skips the product: finite entries
    assert D.acc_check_plant(ac, "old", math.inf, got, clean, dep) == 0                  # beta * Inf in an old output stays an infinity
