"""The references of the einsum fuzz (oracle/einsum_ref.py) and its case list (tools/fuzz_einsum.py), without a GPU:
the exact-data bit budgets hold over the actual summation lengths, the error bound catches planted errors and accepts
numpy's own float64 result, and the generated cases reach every path of the "auto" rules often enough."""

import sys
from pathlib import Path

import numpy as np
import pytest

from oracle import einsum_ref as R

sys.path.insert(0, str(Path(__file__).resolve().parents[1] / "tools"))
import fuzz_einsum as F  # noqa: E402

SEED = 20261016   # tests/test_gpu_einsum_fuzz.py sweeps the same cases
N_EXACT, N_BOUNDED, N_DESC = 500, 500, 300


def _cases():
    return F.gen_cases(N_EXACT, SEED)


# --------------------------------------------------------------------------
# exact data
# --------------------------------------------------------------------------

def test_exact_budgets_hold_over_the_actual_summation_lengths():
    """For every generated case: the worst absolute sum of the mantissa products, computed with Python integers over
    the case's own summation length, fits the significand of the dtype it computes in (24 bits when a schedule step can
    be float32), float32-stored operands fit float32, and float64 cases leave float32 behind (> 24 bits)."""
    wide = 0
    for case in _cases():
        n = len(case.shapes)
        sig = R.compute_significand(case.dtypes, R.f32_step_possible(case.dtypes, n))
        terms = R.summed_points(case.subs, case.extent())
        bits = R.exact_bits(n, case.dtypes, terms, sig, np.random.default_rng(case.seed))
        worst = max(terms, 1)
        for b in bits:
            assert b >= 1
            worst *= (1 << b) - 1
        assert worst <= 1 << sig, (case.subs, bits, terms)
        for b, dt in zip(bits, case.dtypes):
            if dt == "float32":
                assert b <= 24
        if sig == 53 and terms < 1 << 20:
            assert sum(bits) > 24, (case.subs, bits, terms)
            wide += 1
    assert wide >= 40


def test_exact_data_round_trips_and_matches_numpy_where_numpy_is_exact():
    rng = np.random.default_rng(0)
    subs, shapes = "eij,ej->ei", [(33, 7, 5), (33, 5)]
    bits = R.exact_bits(2, ["float64", "float32"], 5, 53, rng)
    assert sum(bits) > 24 and bits[1] <= 24
    mants, arrs = R.exact_operands(shapes, ["float64", "float32"], bits, [-3, 5], rng)
    assert arrs[1].dtype == np.float32
    ref = R.exact_reference(subs, mants, [-3, 5], np.float64, 53)
    assert R.needs_more_than_f32(ref)
    # every partial sum is exact: numpy's float64 einsum, in whatever order it sums, is the same bits
    assert R.bitwise_equal(np.einsum(subs, arrs[0], arrs[1].astype(np.float64)), ref)
    # an accumulator or product rounded to float32 anywhere is not
    rounded = np.einsum(subs, arrs[0].astype(np.float32), arrs[1]).astype(np.float64)
    assert not R.bitwise_equal(rounded, ref)


@pytest.mark.parametrize("plant", ["dropped", "duplicated", "sign", "transposed", "f32_accumulator"])
def test_exact_reference_catches_planted_errors(plant):
    rng = np.random.default_rng(1)
    subs, shapes = "ei,ej->ij", [(65, 16), (65, 16)]
    bits = R.exact_bits(2, ["float64"] * 2, 65, 53, rng)
    mants, arrs = R.exact_operands(shapes, ["float64"] * 2, bits, [2, -7], rng)
    ref = R.exact_reference(subs, mants, [2, -7], np.float64, 53)
    a, b = arrs
    if plant == "dropped":
        got = np.einsum(subs, a[1:], b[1:])
    elif plant == "duplicated":
        got = np.einsum(subs, a, b) + np.einsum("i,j->ij", a[17], b[17])
    elif plant == "sign":
        got = np.einsum(subs, a, b)
        got[3, 5] = -got[3, 5]
    elif plant == "transposed":
        got = np.einsum(subs, a, b).T.copy()
    else:
        got = np.einsum(subs, a.astype(np.float32), b.astype(np.float32)).astype(np.float64)
    assert not R.bitwise_equal(got, ref)
    assert R.bitwise_equal(np.einsum(subs, a, b), ref)


# --------------------------------------------------------------------------
# error bound
# --------------------------------------------------------------------------

def _bounded(subs, shapes, seed=0, dtype=np.float64):
    rng = np.random.default_rng(seed)
    arrs = [(rng.random(s) * 2 - 1).astype(dtype) for s in shapes]
    ref, absref = R.bounded_reference(subs, arrs)
    ext = {}
    for idx, s in zip(subs.split("->")[0].split(","), shapes):
        ext.update(zip(idx, s))
    return arrs, ref, absref, R.bound_terms(subs, ext, len(shapes))


def test_bound_accepts_numpys_own_float64_result():
    for subs, shapes in (("ei,ei->", [(4000, 3), (4000, 3)]), ("ej,ej->j", [(9999, 1), (9999, 1)]),
                         ("e,ij,ei,ej->", [(50,), (7, 7), (50, 7), (50, 7)]), ("ik,kj->ij", [(31, 129), (129, 17)])):
        arrs, ref, absref, n = _bounded(subs, shapes)
        got = np.einsum(subs, *arrs, optimize="optimal")
        assert R.bound_violations(got, ref, absref, n + len(shapes), R.U64) == 0, subs
        assert R.bound_ratio(got, ref, absref, n + len(shapes), R.U64) <= 1


def test_bound_rejects_a_planted_single_term_error():
    subs, shapes = "ei,ej->ij", [(3000, 8), (3000, 8)]
    arrs, ref, absref, n = _bounded(subs, shapes, seed=2)
    a, b = arrs
    got = np.einsum(subs, a, b)
    got[2, 5] -= a[1234, 2] * b[1234, 5]   # one term missing from one entry, hidden among 3000
    assert R.bound_violations(got, ref, absref, n, R.U64) == 1
    # an error in a small entry that hides behind the large ones normwise (max|got - ref| / max|ref| ~ 1e-17)
    a = a.copy()
    a[:, 0] *= 1e-6
    ref, absref = R.bounded_reference(subs, [a, b])
    tiny = np.einsum(subs, a, b)
    tiny[0, 3] += 50 * R.gamma(n, R.U64) * float(absref[0, 3])
    assert R.bound_violations(tiny, ref, absref, n, R.U64) == 1
    assert np.max(np.abs(tiny - np.einsum(subs, a, b))) / float(np.max(np.abs(ref))) < 1e-14


def test_bound_rejects_a_float64_result_rounded_through_float32():
    subs, shapes = "ej,ej->j", [(500, 7), (500, 7)]
    arrs, ref, absref, n = _bounded(subs, shapes, seed=3)
    got = np.einsum(subs, *arrs).astype(np.float32).astype(np.float64)
    assert R.bound_violations(got, ref, absref, n, R.U64) > 0
    # float32 data computed in float32 passes its own bound
    arrs32, ref32, absref32, _ = _bounded(subs, shapes, seed=3, dtype=np.float32)
    assert R.bound_violations(np.einsum(subs, *arrs32), ref32, absref32, n, R.U32) == 0


def test_bound_rejects_a_transposed_operand():
    subs, shapes = "ij,jk->ik", [(16, 16), (16, 16)]
    arrs, ref, absref, n = _bounded(subs, shapes, seed=4)
    got = np.einsum(subs, arrs[0].T, arrs[1])
    assert R.bound_violations(got, ref, absref, n, R.U64) > 0
    assert R.bound_ratio(got, ref, absref, n, R.U64) > 1


def test_bound_rejects_nan_and_shape_mismatch():
    arrs, ref, absref, n = _bounded("ei->i", [(10, 3)])
    got = np.einsum("ei->i", arrs[0])
    got[1] = np.nan
    assert R.bound_violations(got, ref, absref, n, R.U64) == 1
    assert R.bound_ratio(got[:2], ref, absref, n, R.U64) == np.inf


def test_unit_roundoff_follows_validation_dtype():
    import feinsum_amd as f
    from feinsum_amd.measure import validation_dtype

    for dts in (("float64",) * 3, ("float32",) * 3, ("float32", "float64", "float64"), ("float32", "float32", "float64"),
                ("float32", "float64"), ("float32",), ("float64", "float32", "float32", "float64")):
        expr = f.einsum(",".join("e" * len(dts)) + "->e", *[f.array(f"A{k}", ("E",), dt) for k, dt in enumerate(dts)])
        want = R.U32 if validation_dtype(expr) == np.dtype("float32") else R.U64
        assert R.unit_roundoff(dts, len(dts)) == want, dts


# --------------------------------------------------------------------------
# coverage of the case lists (host only: launch_kind and einsum_reduce_plan need no device)
# --------------------------------------------------------------------------

def test_transform_sweep_covers_every_bucket():
    cov = F.coverage(_cases())
    assert not F.missing_buckets(cov, F.MINIMUMS), (F.missing_buckets(cov, F.MINIMUMS), dict(cov))
    # the "reduction" transform refuses some (more than REDUCE_MAX_OUT entries) and "auto" never leaves a case out
    assert cov["not-accepted:reduction"] > 0
    assert cov["not-accepted:auto"] == cov["not-accepted:generic"] == 0


def test_bounded_sweep_stays_within_its_summation_cap():
    cases = F.gen_cases(N_BOUNDED, SEED, max_points=1_000_000, max_sum=10_000, max_elems=2_000_000, edges=False)
    for c in cases:
        assert R.summed_points(c.subs, c.extent()) <= 10_000
    cov = F.coverage(cases)
    for k in ("dtype:float32", "dtype:mixed", "dtype:float64", "ops:1", "ops:2", "ops:3+", "path:contraction",
              "path:reduction-valu-Esummed", "path:reduction-valu-Ekept"):
        assert cov[k] >= 5, (k, dict(cov))


def test_descriptor_sweep_covers_every_layout_and_entry_point():
    cov = F.desc_coverage(F.gen_desc_cases(N_DESC, SEED))
    assert not F.missing_buckets(cov, F.DESC_MINIMUMS), (F.missing_buckets(cov, F.DESC_MINIMUMS), dict(cov))


def test_threshold_cases_straddle_the_auto_rules():
    from feinsum_amd.measure import launch_kind

    by = {(c.subs, c.shapes, c.E): c for c in F.threshold_cases(SEED)}
    kinds = {k: launch_kind(c.expr(), "auto", {"E": c.E}) for k, c in by.items()}
    m = F.REDUCE_MIN_SUM
    assert kinds[("e,e->", (("E",), ("E",)), m - 1)] == "generic"
    assert kinds[("e,e->", (("E",), ("E",)), m)] == "reduction"
    assert kinds[("e,j->j", (("E",), (F.REDUCE_MAX_OUT,)), m + 1)] == "reduction"
    assert kinds[("e,j->j", (("E",), (F.REDUCE_MAX_OUT + 1,)), m + 1)] == "generic"
    paths = {k: F.paths_of(c, "auto", None) for k, c in by.items()}
    assert paths[("ei,ej,e->", (("E", 4), ("E", 5), ("E",)), 16_001)] == ["reduction-valu-Esummed"]   # one launch
    assert paths[("ei,ej,e->", (("E", 5), ("E", 5), ("E",)), 16_001)] == ["generic", "reduction-valu-Esummed"]
    assert paths[("ei,ej->ij", (("E", 64), ("E", 64)), m + 1)] == ["reduction-mfma"]


def test_tile_limit_cannot_bind_under_the_output_limit():
    """REDUCE_MAX_TILES: a two-operand launch the matrix-core path takes (M >= 16, N >= 8, M N >= 512) with at most
    REDUCE_MAX_OUT entries has few tiles of 64 x 64 -- far below the limit, so no case can sit at 255 / 256 tiles."""
    from feinsum_amd.reduction import REDUCE_MAX_OUT, REDUCE_MAX_TILES

    most = 0
    for M in range(16, REDUCE_MAX_OUT + 1):
        for N in range(8, REDUCE_MAX_OUT // M + 1):
            if M * N < 512:
                continue
            per = -(-M // 64) * -(-N // 64)
            most = max(most, per * (REDUCE_MAX_OUT // (M * N)))
    assert most < REDUCE_MAX_TILES
