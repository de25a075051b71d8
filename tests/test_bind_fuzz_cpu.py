"""The bindings sweep (tools/fuzz_bind.py) without a GPU: its fixed-seed case list reaches every coverage minimum and
the 90 % condition on refusals, the bit budgets hold for every row, the per-row int64 reference is numpy's float64
einsum, ``match_family`` finds every spelling (with the roles on the right operands, for every template and every
operand order) and none of the near misses, the launch-shape prediction agrees with hand-written tables, and the
checkers reject swapped outputs and swapped geometry factors."""

import sys
from itertools import permutations
from pathlib import Path

import numpy as np

from feinsum_amd import family
from feinsum_amd.family import match_family
from oracle import einsum_ref as R

sys.path.insert(0, str(Path(__file__).resolve().parents[1] / "tools"))
import fuzz_bind as B  # noqa: E402
import fuzz_dg as D  # noqa: E402

SEED = 20261017   # tests/test_gpu_bind_fuzz.py sweeps the same cases
N_BIND = 12


def _cases():
    return B.gen_bind_cases(N_BIND, SEED)


def test_case_list_reaches_every_minimum_and_nine_tenths_run():
    cnt, run, total = B.coverage(_cases())
    assert not B.missing_buckets(cnt, B.MINIMUMS), B.missing_buckets(cnt, B.MINIMUMS)
    assert run >= 0.9 * total, (run, total)
    for c in _cases():   # nothing is refused under "auto" or "generic", and only a forced transform ever is
        for t in c.transforms():
            assert B.accepted_on_host(c, t) or D.tname(t) == "mfma", (c, t)
    assert {c.E for c in _cases() if c.eclass == "static-rounds"} == {20_004}
    assert all(B.BindCase.from_repro(c.repro()) == c for c in _cases())


def test_tool_templates_are_the_library_templates():
    assert sorted(t[0] for t in B.TEMPLATES) == sorted(t[2] for t in family._TEMPLATES)
    assert len(B.TEMPLATES) == 20 and len(B.SHAPES) == 24


def test_budgets_hold_for_every_row_of_every_case():
    shared = 0
    for case in _cases():
        bits, scales, dtypes, sig = D.plan_data(case, np.random.default_rng(case.seed))
        expr, keys = case.stages()[0]
        rows = [([keys[a.name] for a in row], D._terms(expr)) for row in expr.args]
        assert sig == (24 if case.dtype == "float32" else 53)
        for names, n_terms in rows:
            worst = max(int(n_terms), 1)
            for nm in names:
                worst *= (1 << bits[nm]) - 1
            assert worst <= (1 << sig), (case, names)
        for k, b in bits.items():
            cap = 24 if dtypes[k] == np.dtype("float32") else sig
            assert 1 <= b <= cap
            if b < cap:
                assert not R.rows_fit(rows, {**bits, k: b + 1}, sig), (case, k)
        shared += len({nm for names, _ in rows for nm in names}) < sum(len(names) for names, _ in rows)
    assert shared >= 50


def test_row_reference_is_the_float64_einsum_of_the_rows_own_arrays():
    done = 0
    for case in _cases():
        if case.E > 300:
            continue
        arrays, mants, scales, sig = D.host_data(case)
        expr, keys = case.stages()[0]
        out_dt = np.dtype(case.dtype)
        for row in expr.args:
            ks = [keys[a.name] for a in row]
            ref = R.int_reference(expr.get_subscripts(), [mants[k] for k in ks], sum(scales[k] for k in ks), out_dt, sig)
            f64 = np.einsum(expr.get_subscripts(), *[arrays[k].astype(np.float64) for k in ks], optimize=True)
            assert R.bitwise_equal(ref, f64.astype(out_dt)), case
            done += 1
    assert done >= 300


def test_match_family_puts_every_role_on_the_right_operand():
    """All 20 templates (and the triangle shapes), every operand order, renamed and not: ``roles[r]`` is the position
    of the operand the spelling put role r on, the long index is the spelling's element letter, the family is the
    template's."""
    rng_seed = 0
    for subs, fam, roles in B.TEMPLATES:
        for nd in (3, 2) if (subs, 2) in B.SHAPES else (3,):
            n = len(roles)
            for order, perm in enumerate(permutations(range(n))):
                for renamed in (False, True):
                    for concrete in (False, True):
                        rng_seed += 1
                        Np, Nfp = (10, 4) if nd == 2 else (10, 6)
                        case = B.BindCase("spell", subs, nd, Np, Nfp, "float64", 17, "ragged", rng_seed, order, renamed,
                                          concrete)
                        b = B.build(case)
                        p = match_family(b.expr)
                        assert p is not None and p.name == fam, (case, b.expr.get_subscripts())
                        assert p.long_index == b.e_letter
                        assert set(p.roles) == set(roles)
                        for pos, role in enumerate(roles):    # operand p.roles[role] of the einsum is operand pos of the template
                            assert perm[p.roles[role]] == pos, (case, role)
                        jname, opname, fname = b.rows[0]
                        row = b.expr.args[0]
                        assert row[p.roles[roles[-1]]].name == fname and row[p.roles[roles[-2]]].name == opname
                        assert jname is None or row[p.roles["J"]].name == jname
                        assert p.params["Np"] == Np and p.params.get("ndim", nd) == nd


def test_every_generated_spelling_matches_and_no_near_miss_does():
    kinds = set()
    for case in _cases():
        plan = match_family(B.build(case).expr)
        if case.mode == "near":
            assert plan is None, (case, B.build(case).expr.get_subscripts())
            kinds.add(case.near)
        else:
            assert plan is not None and plan.name == B.FAMILY_OF[case.subs], case
            assert bool(plan.params.get("f32")) == (case.dtype == "float32")
    assert kinds == set(B.NEAR)


def test_launch_shape_prediction_by_hand():
    g = lambda subs, rows, dt="float64", nd=3: B.groups_of(subs, nd, dt, rows)   # noqa: E731
    grad = "xre,rij,ej->xei"
    # consecutive rows with the same J and operator share a launch; the same pair further down does not join them
    assert g(grad, [("J", "D", "a"), ("J", "D", "b"), ("K", "D", "c"), ("J", "D", "d")]) == ("fe_grad", [2, 1, 1])
    assert g(grad, [("J", "D", "a"), ("J", "R", "a"), ("J", "R", "b")]) == ("fe_grad", [1, 2])
    assert g("ef,fij,fej->ei", [("J", "R", f"v{k}") for k in range(19)], "float32") == ("fe_facemass", [19])
    comp = "re,rij,ej->ei"
    cross = [(j, "D", u) for u, js in (("ux", ("Jy", "Jz")), ("uy", ("Jx", "Jz")), ("uz", ("Jx", "Jy"))) for j in js]
    assert g(comp, cross) == ("fe_gradplanes", [6])
    assert g(comp, cross[::-1]) == ("fe_gradplanes", [6])                      # any row order
    assert g(comp, cross, "float32") == ("fe_divcomp", [1] * 6)
    assert g(comp, cross, nd=2) == ("fe_divcomp", [1] * 6)
    assert g("er,rij,ej->ei", cross) == ("fe_divcomp", [1] * 6)
    assert g(comp, cross + [("Jx", "D", "ux")]) == ("fe_divcomp", [1] * 7)      # ux has three planes, the others two
    assert g(comp, cross + [("Jy", "D", "ux")]) == ("fe_divcomp", [1] * 7)      # (ux, Jy) twice
    assert g(comp, cross[:5] + [("Jx", "D2", "uz")]) == ("fe_divcomp", [1] * 6)  # two operators
    assert g(comp, [("Ja", "D", "u"), ("Jb", "D", "u"), ("Jc", "D", "v"), ("Jd", "D", "v")]) == ("fe_divcomp", [1] * 4)
    assert g(comp, [("Ja", "D", "u"), ("Jb", "D", "v"), ("Jc", "D", "w")]) == ("fe_divcomp", [1] * 3)   # one plane each
    assert g(comp, [("Ja", "D", "u"), ("Jb", "D", "u")]) == ("fe_gradplanes", [2])


def _two_factor_case():
    case = B.BindCase("rows", "re,rij,ej->ei", 3, 10, 6, "float64", 17, "ragged", 5, 3, True, table="planes-2j")
    arrays, mants, scales, sig = D.host_data(case)
    expr, keys = case.stages()[0]
    refs = []
    for row in expr.args:
        ks = [keys[a.name] for a in row]
        refs.append(R.int_reference(expr.get_subscripts(), [mants[k] for k in ks], sum(scales[k] for k in ks),
                                    np.float64, sig))
    return case, expr, keys, mants, scales, sig, refs


def test_checkers_reject_swapped_outputs_and_swapped_factors():
    case, expr, keys, mants, scales, sig, refs = _two_factor_case()
    b = B.build(case)
    # two rows of one field: they differ in the geometry factor only
    k0, k1 = next((a, c) for a in range(len(b.rows)) for c in range(len(b.rows))
                  if a < c and b.rows[a][2] == b.rows[c][2] and b.rows[a][0] != b.rows[c][0])
    assert R.differing_entries(refs[k0], refs[k0]) == 0
    assert R.differing_entries(refs[k1], refs[k0]) > 0          # the outputs of the two rows, swapped
    # J and J' swapped: row k0 computed with the factor of row k1
    jpos = next(p for p, a in enumerate(expr.args[k0]) if a.name == b.rows[k0][0])
    ks = [keys[a.name] for a in expr.args[k0]]
    ks[jpos] = keys[b.rows[k1][0]]
    wrong = R.int_reference(expr.get_subscripts(), [mants[k] for k in ks], sum(scales[k] for k in ks), np.float64, sig)
    assert R.differing_entries(wrong, refs[k0]) > 0


def test_aliased_names_share_their_data_key():
    seen = 0
    for case in _cases():
        b = B.build(case)
        if b.pair is None:
            continue
        seen += 1
        assert case.alias in ("same", "copies") and b.pair[0] != b.pair[1]
        assert b.keys[b.pair[0]] == b.keys[b.pair[1]]
    assert seen >= 20


def test_overlap_predicate():
    from feinsum_amd.measure import _overlap
    from feinsum_amd.operator import _conflict  # noqa: F401  (operator.py uses the same predicate)

    assert _overlap([(100, 8)], [(107, 8)]) and _overlap([(107, 8)], [(100, 8)])
    assert not _overlap([(100, 8)], [(108, 8)]) and not _overlap([(108, 8)], [(100, 8)])   # touching
    assert not _overlap([(100, 0)], [(96, 16)]) and not _overlap([(96, 16)], [(100, 0)])   # no bytes: no overlap
    assert _overlap([(0, 4), (100, 8)], [(50, 4), (104, 1)])
