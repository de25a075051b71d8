"""Accumulation inside the contraction and the split-reduction kernels (``{"variant": "contraction" | "reduction",
"accumulate": "kernel"}``) without a device: the routing table -- the two new cells and every default
where it was --, the two entry points' argument checks before any device work, and the bind-time refusal of a schedule
whose last step has no accumulating kernel."""

import ctypes as C
import math
import re
from pathlib import Path

import numpy as np
import pytest

import autograd_cases as cases
import feinsum_amd as f
from feinsum_amd import _hip, measure
from feinsum_amd.contraction import _desc, _extents, check_accumulating_steps, plan_steps
from feinsum_amd.contraction_schedule import ContractionSchedule, EinsumOperand, IntermediateResult
from feinsum_amd.diagnostics import InvalidParameterError
from feinsum_amd.reduction import check_accumulating_plan, plan_reduction

ROOT = Path(__file__).resolve().parents[1]
CONTRACT = {"variant": "contraction", "accumulate": "kernel"}
REDUCE = {"variant": "reduction", "accumulate": "kernel"}
FAKE = 1 << 40    # a pointer that is never dereferenced: the checks come before any device work


class _Strides:
    """C-contiguous strides of a tensor of this shape, without allocating it."""

    def __init__(self, shape):
        self._st = tuple(int(np.prod(shape[k + 1:], dtype=np.int64)) for k in range(len(shape)))

    def stride(self):
        return self._st


def _descriptor(subs, shapes, dtype="float64"):
    expr = f.einsum(subs, *[f.array(n, s, dtype) for n, s in zip("ABCD", shapes)])
    ext = _extents(expr, {})
    ts = [_Strides([ext[c] for c in idx]) for idx in expr.in_idx_sets]
    return _desc(subs, ts, ext, [np.dtype(dtype)] * expr.n)


def test_both_symbols_are_declared_exported_and_wrapped():
    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "feinsum_hip.h").read_text(), flags=re.S)
    lib = _hip.load_library()
    for sym in ("fe_einsum_contract_acc", "fe_einsum_reduce_acc"):
        assert re.search(rf"\bint {sym}\s*\(", header), sym
        assert sym in _hip.EXPORTED_SYMBOLS and hasattr(lib, sym)
    assert callable(_hip.einsum_contract_acc) and callable(_hip.einsum_reduce_acc)


def test_routing_table():
    gemm = f.einsum("ik,kj->ij", f.array("A", (20, 30)), f.array("B", (30, 40)))
    gemm32 = f.einsum("ik,kj->ij", f.array("A", (20, 30), "float32"), f.array("B", (30, 40), "float32"))
    mixed = f.einsum("ik,kj->ij", f.array("A", (20, 30), "float32"), f.array("B", (30, 40)))
    chain = f.einsum("ij,jk,kl->il", f.array("A", (5, 6)), f.array("B", (6, 7)), f.array("C", (7, 8)))
    dot = f.einsum("ei,ei->", f.array("A", ("E", 5)), f.array("B", ("E", 5)))
    rowsum = f.einsum("ij->i", f.array("A", ("E", 6)))
    energy = f.einsum("e,ei,ei->", f.array("w", ("E",), "float32"), f.array("A", ("E", 5)), f.array("B", ("E", 5)))
    # the new cells
    for e in (gemm, gemm32, mixed, chain, dot, energy, cases.grad(3, 10), cases.face_mass(35, 4, 15, 4)):
        assert measure.accumulate_route(e, CONTRACT) == "kernel"
    for e in (gemm, gemm32, mixed, chain, dot, energy, rowsum):
        assert measure.accumulate_route(e, REDUCE) == "kernel"
    # one operand has no contraction; complex operands have neither kernel
    with pytest.raises(NotImplementedError, match="no accumulating kernel"):
        measure.accumulate_route(rowsum, CONTRACT)
    cplx = f.einsum("ik,kj->ij", f.array("A", (20, 30), "complex128"), f.array("B", (30, 40), "complex128"))
    for transform in (CONTRACT, REDUCE):
        with pytest.raises(NotImplementedError, match="no accumulating kernel"):
            measure.accumulate_route(cplx, transform)
    # every default is what it was
    assert measure.ACCUMULATE_ROUTES == ("kernel", "axpby", "epilogue")
    for name, e in cases.other_cases():
        assert measure.accumulate_route(e) == "axpby", name
        for variant in ("contraction", "reduction"):
            assert measure.accumulate_route(e, variant) == "axpby", (name, variant)
            assert measure.accumulate_route(e, {"variant": variant}) == "axpby", (name, variant)
            assert measure.accumulate_route(e, {"variant": variant, "accumulate": "axpby"}) == "axpby", (name, variant)
    for name, e in cases.dg_cases():
        want = "kernel" if name.startswith("facemass_") and "_b4_tet" in name and not name.endswith("5") else "axpby"
        assert measure.accumulate_route(e) == want, name
        for variant in ("contraction", "reduction"):
            assert measure.accumulate_route(e, {"variant": variant}) == "axpby", (name, variant)
    # "kernel" without a variant stays what it was on a GEMM, and "epilogue" with either variant raises
    with pytest.raises(NotImplementedError, match="no accumulating kernel"):
        measure.accumulate_route(gemm, {"accumulate": "kernel"})
    for e in (gemm, dot, cases.grad(3, 35)):
        for variant in ("contraction", "reduction"):
            with pytest.raises(NotImplementedError, match="no accumulating epilogue"):
                measure.accumulate_route(e, {"variant": variant, "accumulate": "epilogue"})
    assert "bind" in measure.accumulate_route.__doc__


def test_contract_acc_checks_its_arguments_without_a_device():
    d = _descriptor("ik,kj->ij", [(20, 30), (30, 40)])
    lib = _hip.load_library()
    for bad in (math.nan, math.inf, -math.inf):
        for alpha, beta in ((bad, 1.0), (1.0, bad)):
            with pytest.raises(InvalidParameterError, match="finite"):
                _hip.einsum_contract_acc(d, [FAKE, FAKE], FAKE, alpha, beta, 0)
            rc = lib.fe_einsum_contract_acc(C.byref(d), _hip._ptr_array([FAKE, FAKE]), FAKE, alpha, beta, None)
            assert rc == _hip.FE_EINVAL and b"finite" in lib.fe_last_error()
    three = _hip.EinsumDesc()
    three.n_operands, three.n_out, three.n_sum = 3, 1, 1
    three.out_extent[0], three.sum_extent[0] = 4, 4
    with pytest.raises(NotImplementedError, match="exactly 2"):
        _hip.einsum_contract_acc(three, [FAKE, FAKE, FAKE], FAKE, 1.0, 1.0, 0)
    assert lib.fe_einsum_contract_acc(C.byref(three), _hip._ptr_array([FAKE] * 3), FAKE, 1.0, 1.0, None) == _hip.FE_EUNSUPPORTED
    # the parent's checks: a null or misaligned output
    with pytest.raises(InvalidParameterError, match="null output"):
        _hip.einsum_contract_acc(d, [FAKE, FAKE], 0, 1.0, 1.0, 0)
    with pytest.raises(InvalidParameterError, match="aligned"):
        _hip.einsum_contract_acc(d, [FAKE, FAKE], FAKE + 4, 1.0, 1.0, 0)
    # an empty output: FE_OK without a HIP call (no device here)
    empty = _descriptor("ik,kj->ij", [(0, 30), (30, 40)])
    _hip.einsum_contract_acc(empty, [0, 0], 0, 2.0, -0.5, 0)
    _hip.einsum_contract_acc(empty, [0, 0], 0, 0.5, 0.0, 0)


def test_reduce_acc_checks_its_arguments_without_a_device():
    d = _descriptor("ei,ei->", [(10**6, 35), (10**6, 35)])
    _, _, nbytes = _hip.einsum_reduce_plan(d)
    assert nbytes > 256
    lib = _hip.load_library()
    for bad in (math.nan, math.inf, -math.inf):
        for alpha, beta in ((bad, 1.0), (1.0, bad)):
            with pytest.raises(InvalidParameterError, match="finite"):
                _hip.einsum_reduce_acc(d, [FAKE, FAKE], FAKE, FAKE, nbytes, alpha, beta, 0)
            rc = lib.fe_einsum_reduce_acc(C.byref(d), _hip._ptr_array([FAKE, FAKE]), FAKE, FAKE, C.c_size_t(nbytes),
                                          alpha, beta, None)
            assert rc == _hip.FE_EINVAL and b"finite" in lib.fe_last_error()
    # the workspace checks of fe_einsum_reduce: null, short, misaligned
    with pytest.raises(InvalidParameterError, match="workspace"):
        _hip.einsum_reduce_acc(d, [FAKE, FAKE], FAKE, 0, nbytes, 1.0, 1.0, 0)
    with pytest.raises(InvalidParameterError, match="workspace"):
        _hip.einsum_reduce_acc(d, [FAKE, FAKE], FAKE, FAKE, nbytes - 256, 1.0, 1.0, 0)
    with pytest.raises(InvalidParameterError, match="aligned"):
        _hip.einsum_reduce_acc(d, [FAKE, FAKE], FAKE, FAKE + 8, nbytes, 1.0, 1.0, 0)
    rc = lib.fe_einsum_reduce_acc(C.byref(d), _hip._ptr_array([FAKE, FAKE]), FAKE, None, C.c_size_t(nbytes), 1.0, 1.0, None)
    assert rc == _hip.FE_EINVAL
    with pytest.raises(InvalidParameterError, match="null output"):
        _hip.einsum_reduce_acc(d, [FAKE, FAKE], 0, FAKE, nbytes, 1.0, 1.0, 0)
    # more than 4096 output entries: the parent's FE_EUNSUPPORTED
    big = _descriptor("ei,ej->ij", [(1000, 100), (1000, 100)])
    with pytest.raises(NotImplementedError, match="output entries"):
        _hip.einsum_reduce_acc(big, [FAKE, FAKE], FAKE, FAKE, 1 << 30, 1.0, 1.0, 0)
    # an empty output: FE_OK without a HIP call, no workspace
    empty = _descriptor("ei,ej->ij", [(1000, 0), (1000, 16)])
    assert _hip.einsum_reduce_plan(empty)[2] == 0
    _hip.einsum_reduce_acc(empty, [0, 0], 0, 0, 0, 2.0, -0.5, 0)


def test_a_last_step_on_the_generic_kernel_is_refused_before_any_array_exists():
    chain = f.einsum("ij,jk,kl->il", f.array("A", (33, 17)), f.array("B", (17, 20)), f.array("C", (20, 9)))
    check_accumulating_steps(plan_steps(chain))                 # the optimal schedule ends in a two-operand step
    three = f.einsum("ij,jk,kl->il", f.array("A", (33, 17)), f.array("B", (17, 20)), f.array("C", (20, 9)))
    nary = ContractionSchedule(("ij,jk,kl->il",), ("_fe_out",), ((EinsumOperand(0), EinsumOperand(1), EinsumOperand(2)),))
    steps = plan_steps(three, nary)                             # an n-ary step is split: its last part has two inputs
    assert [len(st.inputs) for st in steps] == [2, 2]
    check_accumulating_steps(steps)
    # a caller's schedule that ends in a pure reduction of an intermediate
    e = f.einsum("ik,kj->i", f.array("A", (33, 17)), f.array("B", (17, 20)))
    sched = ContractionSchedule(("ik,kj->ij", "ij->i"), ("t", "_fe_out"),
                                ((EinsumOperand(0), EinsumOperand(1)), (IntermediateResult("t"),)))
    steps = plan_steps(e, sched)
    assert steps[-1].result is None and len(steps[-1].inputs) == 1
    with pytest.raises(NotImplementedError, match=r"'ij->i'.*generic"):
        check_accumulating_steps(steps)
    # the reduction plan: a "generic" last step
    from feinsum_amd.contraction import Step
    ok = ((Step("ei,ej->ij", (("op", 0), ("op", 1)), "t"), "reduce"), (Step("ij,ij->", (("tmp", "t"), ("op", 2)), None), "contract"))
    check_accumulating_plan(ok)
    check_accumulating_plan(plan_reduction(f.einsum("ei,ei->", f.array("A", ("E", 5)), f.array("B", ("E", 5))), {"E": 10}))
    bad = (ok[0], (ok[1][0], "generic"))
    with pytest.raises(NotImplementedError, match=r"'ij,ij->'.*generic"):
        check_accumulating_plan(bad)
