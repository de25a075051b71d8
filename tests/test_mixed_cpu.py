"""Einsums that mix float32 and float64 operands, without a GPU: the descriptor's dtype flags, the dtypes of a
schedule's steps, the kernel "auto" picks, and the library's refusals of bad dtype fields (before any device work)."""

import numpy as np
import pytest

import feinsum_amd as f
from feinsum_amd import _hip
from feinsum_amd.contraction import plan_step_dtypes, plan_steps
from feinsum_amd.contraction_schedule import ContractionSchedule, EinsumOperand, IntermediateResult
from feinsum_amd.diagnostics import InvalidParameterError
from feinsum_amd.measure import launch_kind

F32, F64 = np.dtype("float32"), np.dtype("float64")


class _Strided:
    """Stands in for a tensor: einsum_desc reads only the strides."""

    def __init__(self, st):
        self._st = st

    def stride(self):
        return self._st


def _gemm_desc(float64, dtypes):
    extent = {"i": 5, "k": 7, "j": 3}
    return _hip.einsum_desc(["ik", "kj"], "ij", "k", extent, [_Strided((7, 1)), _Strided((3, 1))], float64, dtypes)


def test_flag_values_match_the_header():
    assert [_hip.FE_DTYPE_OPERAND_F32(p) for p in range(3)] == [0x100, 0x200, 0x400]
    assert _hip.FE_DTYPE_OPERAND_F32_MASK == 0xff00
    assert (_hip.FE_DTYPE_F64, _hip.FE_DTYPE_F32) == (0, 1)


@pytest.mark.parametrize("dtypes, code", [
    ((F32, F64), 0x100),
    ((F64, F32), 0x200),
    ((F32, F32), 0x300),     # float64 compute over two float32 operands (an intermediate's consumer, say)
    ((F64, F64), 0),
])
def test_descriptor_flags(dtypes, code):
    assert _gemm_desc(True, dtypes).dtype == code


def test_uniform_descriptors_keep_their_codes():
    assert _gemm_desc(True, None).dtype == 0
    assert _gemm_desc(False, None).dtype == 1
    # all-float32 compute never carries flags, whatever the operand list says
    assert _gemm_desc(False, (F32, F32)).dtype == 1
    assert _hip.einsum_dtype_code(True, [F64, F32, F64, F32]) == 0x200 | 0x800


def test_step_dtypes_of_a_mixed_chain():
    A = f.array("A", (64, 32), "float32")
    B = f.array("B", (32, 16), "float32")
    C = f.array("C", (16, 8), "float64")
    expr = f.einsum("ij,jk,kl->il", A, B, C)
    # (A B) first: a float32 intermediate, then float64 with C
    sched = ContractionSchedule(("ij,jk->ik", "ik,kl->il"), ("t0", "_fe_out"),
                                ((EinsumOperand(0), EinsumOperand(1)), (IntermediateResult("t0"), EinsumOperand(2))))
    steps = plan_steps(expr, sched)
    assert plan_step_dtypes(expr, steps) == (F32, F64)
    # (B C) first: float64 from the start
    sched = ContractionSchedule(("jk,kl->jl", "ij,jl->il"), ("t0", "_fe_out"),
                                ((EinsumOperand(1), EinsumOperand(2)), (EinsumOperand(0), IntermediateResult("t0"))))
    assert plan_step_dtypes(expr, plan_steps(expr, sched)) == (F64, F64)
    # one n-ary step, split left to right: A B (float32), then C
    sched = ContractionSchedule(("ij,jk,kl->il",), ("_fe_out",),
                                ((EinsumOperand(0), EinsumOperand(1), EinsumOperand(2)),))
    assert plan_step_dtypes(expr, plan_steps(expr, sched)) == (F32, F64)
    # the optimal schedule: the last step is the output's dtype
    assert plan_step_dtypes(expr, plan_steps(expr))[-1] == F64


def test_step_dtypes_uniform_and_refused():
    expr = f.einsum("ij,jk,kl->il", *(f.array(n, (8, 8), "float32") for n in "ABC"))
    assert set(plan_step_dtypes(expr, plan_steps(expr))) == {F32}
    cplx = f.einsum("ik,kj->ij", f.array("A", (8, 8), "complex128"), f.array("B", (8, 8)))
    with pytest.raises(NotImplementedError):
        plan_step_dtypes(cplx, plan_steps(cplx))


def test_launch_kind_of_mixed_einsums():
    big = f.einsum("ik,kj->ij", f.array("A", (4096, 4096), "float32"), f.array("B", (4096, 4096), "float64"))
    erj = f.einsum("erj,rij->ei", f.array("u", ("E", 3, 35), "float32"), f.array("D", (3, 35, 35)))
    for expr in (big, erj):
        assert launch_kind(expr, "auto", {"E": 10**6}) == "generic"     # "auto" keeps mixed einsums generic
        assert launch_kind(expr, None, {"E": 10**6}) == "generic"
        assert launch_kind(expr, "generic", {"E": 10**6}) == "generic"
        assert launch_kind(expr, "contraction", {"E": 10**6}) == "contraction"
    # a mixed DG einsum is no family: "auto" sends it to the generic kernel, "contraction" to its schedule
    grad = f.einsum("es,sij,ej->ei", f.array("J", ("E", 3), "float32"), f.array("D", (3, 35, 35)),
                    f.array("u", ("E", 35)))
    assert launch_kind(grad, "auto", {"E": 1000}) == "generic"
    assert launch_kind(grad, "contraction", {"E": 1000}) == "contraction"


@pytest.mark.parametrize("code", [
    1 | 0x100,        # flags with the float32 compute type
    0x10000 | 0x100,  # a bit above the operand flags
    1 << 30,          # any other unknown bit
    0x400,            # the flag of an operand the einsum does not have (2 operands)
])
@pytest.mark.parametrize("entry", ["generic", "contract"])
def test_bad_dtype_fields_are_einval(code, entry):
    d = _gemm_desc(True, None)
    d.dtype = code
    fn = _hip.einsum_generic if entry == "generic" else _hip.einsum_contract
    # bogus non-null pointers: the refusal must come before anything touches them or the device
    with pytest.raises(InvalidParameterError):
        fn(d, [0x1000, 0x2000], 0x3000, 0)


def test_unknown_compute_code_stays_unsupported():
    d = _gemm_desc(True, None)
    d.dtype = 2
    with pytest.raises(NotImplementedError):
        _hip.einsum_generic(d, [0x1000, 0x2000], 0x3000, 0)


def test_groups_ignore_the_flags():
    assert _hip.einsum_contract_groups(_gemm_desc(True, (F32, F64))) == \
        _hip.einsum_contract_groups(_gemm_desc(True, None)) == (("m", "n"), ("k",))


def test_validation_dtype():
    from feinsum_amd.measure import validation_dtype

    def chain(*dts):
        return f.einsum("ij,jk,kl->il", *(f.array(n, (8, 8), dt) for n, dt in zip("ABC", dts)))

    gemm = f.einsum("ik,kj->ij", f.array("A", (8, 8), "float32"), f.array("B", (8, 8)))
    assert validation_dtype(gemm) == F64                      # two operands: widened, compared at 1e-10
    assert validation_dtype(chain("float64", "float32", "float64")) == F64
    assert validation_dtype(chain("float32", "float32", "float64")) == F32   # a step may meet float32 only
    assert validation_dtype(chain("float32", "float32", "float32")) == F32
    assert validation_dtype(chain("float64", "float64", "float64")) == F64
