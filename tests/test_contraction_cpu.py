"""The "contraction" transform without a GPU: index classification, the steps a schedule plans, the "auto"
rule, and the C ABI symbol."""

import numpy as np
import pytest

import feinsum_amd as f
from feinsum_amd import _hip
from feinsum_amd.contraction import (AUTO_MIN_K, AUTO_MIN_M, AUTO_MIN_MN, AUTO_MIN_N, IndexGroups, auto_picks_contraction,
                                     classify_indices, contraction_sizes, intermediate_shapes, plan_steps)
from feinsum_amd.contraction_schedule import (ContractionSchedule, EinsumOperand, IntermediateResult,
                                              get_opt_einsum_contraction_schedule)
from feinsum_amd.diagnostics import InvalidParameterError
from feinsum_amd.measure import launch_kind

import dg


@pytest.mark.parametrize("subs, groups", [
    ("ik,kj->ij", ("", "i", "j", "k")),
    ("bij,bjk->bik", ("b", "i", "k", "j")),
    ("abcd,ea->ebcd", ("", "bcd", "e", "a")),
    ("abc,bda->dc", ("", "c", "d", "ab")),
    ("ijkl,klmn->ijmn", ("", "ij", "mn", "kl")),
    ("erj,rij->ei", ("", "e", "i", "rj")),
    ("ej,ej->j", ("j", "", "", "e")),
    ("ij,k->i", ("", "i", "", "jk")),          # k summed, present in one operand only
    ("iij,jk->ik", ("", "i", "k", "j")),       # repeated index in one operand
    ("ij,jk->ijk", ("j", "i", "k", "")),       # no summation at all
])
def test_classification(subs, groups):
    assert classify_indices(subs) == IndexGroups(*(tuple(g) for g in groups))


def _groups(shapes, strides, out, sums):
    """What fe_einsum_contract forms (host-only query) for operands of the given per-axis strides."""
    class T:
        def __init__(self, st):
            self._st = st

        def stride(self):
            return self._st

    ins = [s for s, _ in shapes]
    extent = {c: e for s, ext in shapes for c, e in zip(s, ext)}
    d = _hip.einsum_desc(ins, out, sums, extent, [T(st) for st in strides], True)
    return _hip.einsum_contract_groups(d)


def test_classification_by_strides_in_the_library():
    # plain GEMM and a batch index
    assert _groups([("ik", (5, 7)), ("kj", (7, 3))], [(7, 1), (3, 1)], "ij", "k") == (("m", "n"), ("k",))
    assert _groups([("bij", (4, 5, 7)), ("bjk", (4, 7, 3))], [(35, 7, 1), (21, 3, 1)], "bik", "j") == \
        (("batch", "m", "n"), ("k",))
    # B = w expanded along i (stride 0): i is carried by A only -> m, although the subscripts name it in both
    assert _groups([("ij", (5, 6)), ("ij", (5, 6))], [(6, 1), (0, 1)], "ij", "") == (("m", "batch"), ())
    # neither operand carries i: a broadcast output index is a batch index
    assert _groups([("ij", (5, 6)), ("ij", (5, 6))], [(0, 1), (0, 1)], "ij", "") == (("batch", "batch"), ())
    # a summed index in one operand only: k, with stride 0 in the other
    assert _groups([("ij", (5, 6)), ("k", (9,))], [(6, 1), (1,)], "i", "jk") == (("m",), ("k", "k"))
    # a repeated index adds its strides: the diagonal of A (strides 4 + 1) is carried
    assert _groups([("iij", (4, 4, 3)), ("jk", (3, 2))], [(4, 1, 0), (2, 1)], "ik", "j") == (("m", "n"), ("k",))
    # an extent of 1 adds nothing to any offset: dropped
    assert _groups([("ik", (1, 7)), ("kj", (7, 3))], [(7, 1), (3, 1)], "ij", "k") == (("dropped", "n"), ("k",))
    with pytest.raises(NotImplementedError):   # three operands
        d = _hip.EinsumDesc()
        d.n_operands = 3
        _hip.einsum_contract_groups(d)


def test_contraction_sizes():
    assert contraction_sizes("bij,bjk->bik", {"b": 64, "i": 5, "j": 7, "k": 3}) == (64, 5, 3, 7)
    assert contraction_sizes("abcd,ea->ebcd", {"a": 2, "b": 3, "c": 4, "d": 5, "e": 6}) == (1, 60, 6, 2)
    assert contraction_sizes("ej,ej->j", {"e": 10, "j": 4}) == (4, 1, 1, 10)


def _chain():
    return f.einsum("ij,jk,kl->il", f.array("A", (6, 7)), f.array("B", (7, 8)), f.array("C", (8, 2)))


def test_steps_of_the_optimal_schedule():
    expr = dg.grad()
    steps = plan_steps(expr)
    sched = get_opt_einsum_contraction_schedule(expr)
    assert [st.subscripts for st in steps] == list(sched.subscripts) == ["rij,ej->rie", "xre,rie->xei"]
    assert steps[0].inputs == (("op", 1), ("op", 2)) and steps[0].result == "_fe_tmp"
    assert steps[1].inputs == (("op", 0), ("tmp", "_fe_tmp")) and steps[1].result is None
    assert intermediate_shapes(steps, {"e": 11, "r": 3, "i": 35, "j": 35, "x": 3}) == {"_fe_tmp": (3, 35, 11)}
    # two operands: one step, the einsum itself
    two = f.einsum("ik,kj->ij", f.array("A", (3, 4)), f.array("B", (4, 5)))
    assert [(st.subscripts, st.result) for st in plan_steps(two)] == [("ik,kj->ij", None)]


def test_steps_of_an_explicit_schedule():
    expr = _chain()
    # not the optimal order: (B C) first, then A
    sched = ContractionSchedule(("jk,kl->jl", "ij,jl->il"), ("t", "_fe_out"),
                                ((EinsumOperand(1), EinsumOperand(2)), (EinsumOperand(0), IntermediateResult("t"))))
    steps = plan_steps(expr, sched)
    assert [st.subscripts for st in steps] == ["jk,kl->jl", "ij,jl->il"]
    assert intermediate_shapes(steps, {"i": 6, "j": 7, "k": 8, "l": 2}) == {"t": (7, 2)}
    # a three-operand step is split into two-operand steps
    trivial = ContractionSchedule(("ij,jk,kl->il",), ("_fe_out",), ((EinsumOperand(0), EinsumOperand(1), EinsumOperand(2)),))
    steps = plan_steps(expr, trivial)
    assert [st.subscripts for st in steps] == ["ij,jk->ik", "ik,kl->il"]
    assert intermediate_shapes(steps, {"i": 6, "j": 7, "k": 8, "l": 2}) == {"_fe_out_part0": (6, 8)}
    bad = ContractionSchedule(("ij,jk,kl->li",), ("_fe_out",), ((EinsumOperand(0), EinsumOperand(1), EinsumOperand(2)),))
    with pytest.raises(InvalidParameterError):   # the last step must write the einsum's own output order
        plan_steps(expr, bad)


def _run_steps(expr, steps, host):
    env = {}
    row = expr.args[0]
    out = None
    for st in steps:
        ops = [host[row[x].name] if kind == "op" else env[x] for kind, x in st.inputs]
        res = np.einsum(st.subscripts, *ops)
        if st.result is None:
            out = res
        else:
            env[st.result] = res
    return out


@pytest.mark.parametrize("make", [_chain, dg.grad, dg.div, lambda: dg.face_mass(1),
                                  lambda: f.einsum("xre,rij,ej->xie", f.array("J", (3, 3, "E")),
                                                   f.array("R", (3, 4, 5)), f.array("u", ("E", 5)))])
def test_planned_steps_reproduce_the_einsum(make):
    from feinsum_amd.measure import generate_host_input_arrays

    expr = make()
    host = generate_host_input_arrays(expr, 9)
    ref = np.einsum(expr.get_subscripts(), *[host[a.name] for a in expr.args[0]])
    scheds = [None]
    if expr.n == 3:
        scheds.append(ContractionSchedule((expr.get_subscripts(),), ("_fe_out",),
                                          (tuple(EinsumOperand(i) for i in range(3)),)))
    for sched in scheds:
        got = _run_steps(expr, plan_steps(expr, sched), host)
        np.testing.assert_allclose(got, ref, rtol=1e-12, atol=0)


def test_contract_symbol_is_exported():
    lib = _hip.load_library()
    assert hasattr(lib, "fe_einsum_contract")
    assert "fe_einsum_contract" in _hip.EXPORTED_SYMBOLS
    # a three-operand descriptor is refused before anything touches a device
    d = _hip.EinsumDesc()
    d.n_operands, d.n_out, d.n_sum = 3, 1, 1
    d.out_extent[0], d.sum_extent[0] = 4, 4
    with pytest.raises(NotImplementedError):
        _hip.einsum_contract(d, [0, 0, 0], 0, 0)


def test_contraction_is_an_accepted_transform():
    gemm = f.einsum("ik,kj->ij", f.array("A", (2, 3)), f.array("B", (3, 4)))
    for transform in ("contraction", {"variant": "contraction"}):
        assert launch_kind(gemm, transform, {}) == "contraction"
        assert launch_kind(dg.grad(), transform, {"E": 10}) == "contraction"   # the DG families too
    assert launch_kind(dg.grad(), "auto", {"E": 10}) == "family"
    assert launch_kind(gemm, "generic", {}) == "generic"
    with pytest.raises(NotImplementedError):
        launch_kind(gemm, "mfma", {})


def _gemm(M, N, K, dtype="float64"):
    return f.einsum("ik,kj->ij", f.array("A", (M, K), dtype), f.array("B", (K, N), dtype))


def test_auto_rule_thresholds():
    M, N, K, MN = AUTO_MIN_M, AUTO_MIN_N, AUTO_MIN_K, AUTO_MIN_MN
    # (N != K throughout: 'ik,kj->ij' with a square B is the DG operator-apply family)
    for at in (_gemm(MN // N, N, K + 1), _gemm(M, MN // M, K + 1), _gemm(MN // N, N, K + 1, "float32")):
        assert launch_kind(at, "auto", {}) == "contraction"
        assert launch_kind(at, None, {}) == "contraction"
    for below in (_gemm(M - 1, 2 * MN // M, K + 1),    # M
                  _gemm(2 * MN // N, N - 1, K + 1),    # N
                  _gemm(MN // N, 2 * N, K - 1),        # K
                  _gemm(M, MN // M - 1, K + 1)):       # M N: too little of a tile
        assert launch_kind(below, "auto", {}) == "generic"
    # batch-heavy: the per-batch M N decides
    small = f.einsum("bij,bjk->bik", f.array("A", ("E", 16, 8)), f.array("B", ("E", 8, 8)))
    fuller = f.einsum("bij,bjk->bik", f.array("A", ("E", 32, 16)), f.array("B", ("E", 16, 16)))
    assert launch_kind(small, "auto", {"E": 100000}) == "generic"
    assert launch_kind(fuller, "auto", {"E": 100000}) == "contraction"
    assert launch_kind(_gemm(4096, 4000, 4096), "generic", {}) == "generic"   # explicit "generic" stays
    # matrix-vector, reduction, pointwise, one operand, three operands, mixed dtypes: the generic kernel
    mv = f.einsum("ij,j->i", f.array("A", (4096, 4096)), f.array("x", (4096,)))
    red = f.einsum("ej->e", f.array("A", ("E", 64)))
    pw = f.einsum("ej,ej->ej", f.array("A", ("E", 64)), f.array("B", ("E", 64)))
    chain = f.einsum("ij,jk,kl->il", f.array("A", (512, 512)), f.array("B", (512, 512)), f.array("C", (512, 512)))
    mixed = f.einsum("ik,kj->ij", f.array("A", (512, 512), "float32"), f.array("B", (512, 512), "float64"))
    for expr in (mv, red, pw, chain, mixed):
        assert launch_kind(expr, "auto", {"E": 100000}) == "generic", expr.get_subscripts()
        assert not auto_picks_contraction(expr, {"E": 100000})
    # the long axis decides: erj,rij->ei has N = 35, K = 105 and M = E
    erj = f.einsum("erj,rij->ei", f.array("u", ("E", 3, 35)), f.array("D", (3, 35, 35)))
    assert launch_kind(erj, "auto", {"E": 100000}) == "contraction"
    assert launch_kind(erj, "auto", {"E": AUTO_MIN_M - 1}) == "generic"
    assert launch_kind(erj, "auto", {"E": AUTO_MIN_M}) == "contraction"   # M N = 16 x 35
