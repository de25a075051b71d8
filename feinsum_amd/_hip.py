"""
ctypes binding of ``libfeinsum_hip.so`` (C ABI: ``include/feinsum_hip.h``).

This is the only place where the Python host code touches native code.  It
replaces the reference's PyOpenCL enqueue inside the loopy executor
(reference: ``src/feinsum/measure.py:163-165,243-251,267``).  There is no CPU
fallback: if the library is missing or fails to load, every entry point raises
:class:`~feinsum_amd.diagnostics.HipLibraryError`.
"""

from __future__ import annotations

import ctypes as C
import os
from pathlib import Path
from typing import Optional, Sequence, Tuple

import numpy as np

from feinsum_amd.diagnostics import HipLibraryError, InvalidParameterError

FE_OK, FE_EINVAL, FE_EUNSUPPORTED, FE_EHIP = 0, -1, -2, -3
VARIANT_AUTO, VARIANT_GENERIC, VARIANT_MFMA, VARIANT_TILED, VARIANT_MFMA_SPLIT = 0, 1, 2, 3, 4
# "mfma_split": div of tetrahedra p = 1..4 only -- the MFMA kernel walking both halves of the element range at once
# (two write windows for its one output: include/feinsum_hip.h, FE_VARIANT_MFMA_SPLIT)
VARIANTS = {"auto": VARIANT_AUTO, "generic": VARIANT_GENERIC, "mfma": VARIANT_MFMA, "tiled": VARIANT_TILED,
            "mfma_split": VARIANT_MFMA_SPLIT}

FAMILY_F32 = 0x100    # FE_FAMILY_F32
FAMILY_ACC = 0x200    # FE_FAMILY_ACC
FAMILY_FIELDS_F32 = 0x400    # FE_FAMILY_FIELDS_F32: float32 fields in float64 div / face-mass


class ArgPack(C.Structure):
    """``struct fe_argpack`` of include/feinsum_hip.h."""

    _fields_ = [
        ("J", C.c_void_p), ("D", C.c_void_p), ("u", C.c_void_p), ("v_div", C.c_void_p),
        ("out", C.c_void_p), ("out2", C.c_void_p),
        ("v", C.POINTER(C.c_void_p)), ("outs", C.POINTER(C.c_void_p)),
        ("E", C.c_int64),
        ("Np", C.c_int32), ("nf", C.c_int32), ("Nfp", C.c_int32), ("b", C.c_int32),
        ("layout_flags", C.c_int32), ("variant", C.c_int32),
        ("j3", C.POINTER(C.c_void_p)),
        ("ndim", C.c_int32),
        ("prepared", C.c_void_p),
        ("alpha", C.c_double), ("beta", C.c_double),
    ]


FE_MAX_EINSUM_OPERANDS = 8
FE_MAX_EINSUM_INDICES = 8
FE_DTYPE_F64 = 0
FE_DTYPE_F32 = 1
FE_DTYPE_OPERAND_F32_MASK = ((1 << FE_MAX_EINSUM_OPERANDS) - 1) << 8
FE_REDUCE_VALU, FE_REDUCE_MFMA = 0, 1   # fe_einsum_reduce_plan paths


def FE_DTYPE_OPERAND_F32(p: int) -> int:   # noqa: N802  (the header's macro)
    """Flag of an einsum descriptor's dtype: operand *p* is stored as float32 (with ``FE_DTYPE_F64`` only)."""
    return 1 << (8 + p)


class EinsumDesc(C.Structure):
    """``struct fe_einsum_desc`` of include/feinsum_hip.h."""

    _fields_ = [
        ("n_operands", C.c_int32), ("n_out", C.c_int32), ("n_sum", C.c_int32), ("dtype", C.c_int32),
        ("out_extent", C.c_int64 * FE_MAX_EINSUM_INDICES),
        ("sum_extent", C.c_int64 * FE_MAX_EINSUM_INDICES),
        ("op_out_stride", (C.c_int64 * FE_MAX_EINSUM_INDICES) * FE_MAX_EINSUM_OPERANDS),
        ("op_sum_stride", (C.c_int64 * FE_MAX_EINSUM_INDICES) * FE_MAX_EINSUM_OPERANDS),
    ]


# The C types of include/feinsum_hip.h.  Every pointer to data travels as an address (device pointers are plain integers;
# host out-parameters go through ``byref``), every table of pointers as ``void**``.
_int, _i32, _i64, _size, _f64, _str = C.c_int, C.c_int32, C.c_int64, C.c_size_t, C.c_double, C.c_char_p
_p, _pp = C.c_void_p, C.POINTER(C.c_void_p)

#: ``name: (restype, argtypes)`` of every function declared in include/feinsum_hip.h, in its order (tests/test_abi.py
#: parses the header and compares)
SIGNATURES = {
    "fe_version": (_int, []),
    "fe_last_error": (_str, []),
    "fe_device_count": (_int, []),
    "fe_device_info": (_int, [_int, _str, _size, _p, _p]),
    "fe_grad3d_f64": (_int, [_p, _p, _p, _p, _i64, _i32, _i32, _p]),
    "fe_grad3d_f64_ex": (_int, [_p, _p, _p, _p, _i64, _i32, _i32, _i32, _p]),
    "fe_div3d_f64_ex": (_int, [_p, _p, _p, _p, _i64, _i32, _i32, _i32, _p]),
    "fe_divcomp3d_f64": (_int, [_p, _p, _p, _p, _i64, _i32, _i32, _i32, _p]),
    "fe_divcomp_f64": (_int, [_p, _p, _p, _p, _i64, _i32, _i32, _i32, _i32, _p]),
    "fe_div3d_f64": (_int, [_p, _p, _p, _p, _i64, _i32, _i32, _p]),
    "fe_grad3d_batched_f64": (_int, [_p, _p, _pp, _pp, _i64, _i32, _i32, _i32, _i32, _p]),
    "fe_div3d_batched_f64": (_int, [_p, _p, _pp, _pp, _i64, _i32, _i32, _i32, _i32, _p]),
    "fe_grad_f64": (_int, [_p, _p, _pp, _pp, _i64, _i32, _i32, _i32, _i32, _i32, _p]),
    "fe_div_f64": (_int, [_p, _p, _pp, _pp, _i64, _i32, _i32, _i32, _i32, _i32, _p]),
    "fe_gradplanes3d_f64": (_int, [_pp, _p, _pp, _pp, _i64, _i32, _i32, _i32, _i32, _p]),
    "fe_matapply_f64": (_int, [_p, _p, _pp, _pp, _i64, _i32, _i32, _i32, _i32, _p]),
    "fe_graddiv3d_f64": (_int, [_p, _p, _p, _p, _p, _p, _i64, _i32, _i32, _p]),
    "fe_waveop3d_f64": (_int, [_p, _p, _p, _p, _p, _p, _p, _p, _pp, _pp, _i64, _i32, _i32, _i32, _i32, _i32, _i32, _p]),
    "fe_facemass_f64": (_int, [_p, _p, _pp, _pp, _i64, _i32, _i32, _i32, _i32, _i32, _i32, _p]),
    "fe_facemass_acc_f64": (_int, [_p, _p, _pp, _pp, _i64, _i32, _i32, _i32, _i32, _i32, _f64, _f64, _p]),
    "fe_grad3d_acc_f64": (_int, [_p, _p, _p, _p, _i64, _i32, _i32, _f64, _f64, _p]),
    "fe_div3d_acc_f64": (_int, [_p, _p, _p, _p, _i64, _i32, _i32, _f64, _f64, _p]),
    "fe_axpby": (_int, [_p, _p, _i64, _f64, _f64, _i32, _p]),
    "fe_prepare_operator": (_int, [_i32, _p, _i32, _i32, _i32, _i32, _p, _p]),
    "fe_release_prepared": (_int, [_p]),
    "fe_grad3d_prepared_f64": (_int, [_p, _p, _p, _pp, _pp, _i64, _i32, _i32, _i32, _i32, _p]),
    "fe_div3d_prepared_f64": (_int, [_p, _p, _p, _pp, _pp, _i64, _i32, _i32, _i32, _i32, _p]),
    "fe_facemass_prepared_f64": (_int, [_p, _p, _p, _pp, _pp, _i64, _i32, _i32, _i32, _i32, _i32, _i32, _p]),
    "fe_graddiv3d_prepared_f64": (_int, [_p, _p, _p, _p, _p, _p, _p, _i64, _i32, _i32, _p]),
    "fe_waveop3d_prepared_f64": (_int, [_p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _pp, _pp, _i64, _i32, _i32, _i32, _i32, _i32,
                                     _i32, _p]),
    "fe_kernel_resources": (_int, [_str, _size]),
    "fe_split_alloc": (_int, [_pp, _size, _i32]),
    "fe_split_free": (_int, [_p]),
    "fe_split_info": (_int, [_p, _str, _size]),
    "fe_split_stats": (_int, [_str, _size]),
    "fe_split_reserve": (_int, [_size]),
    "fe_split_trim": (_int, []),
    "fe_flops_per_element": (_i64, [_i32, _i32, _i32, _i32, _i32]),
    "fe_launch": (_int, [_i32, C.POINTER(ArgPack), _p]),
    "fe_grad3d_mixed_f64": (_int, [_p, _p, _pp, _pp, _i64, _i32, _i32, _i32, _p]),
    "fe_div3d_mixed_f64": (_int, [_p, _p, _pp, _pp, _i64, _i32, _i32, _i32, _p]),
    "fe_facemass_mixed_f64": (_int, [_p, _p, _pp, _pp, _i64, _i32, _i32, _i32, _i32, _i32, _p]),
    "fe_grad3d_mixed_state_f64": (_int, [_p, _p, _pp, _pp, _i64, _i32, _i32, _i32, _p]),
    "fe_div3d_mixed_state_f64": (_int, [_p, _p, _pp, _pp, _i64, _i32, _i32, _i32, _p]),
    "fe_facemass_mixed_state_f64": (_int, [_p, _p, _pp, _pp, _i64, _i32, _i32, _i32, _i32, _i32, _p]),
    "fe_grad3d_strided_f64": (_int, [_p, _i64, _p, _pp, _pp, _i64, _i64, _i32, _i32, _i32, _p]),
    "fe_div3d_strided_f64": (_int, [_p, _i64, _p, _pp, _i64, _pp, _i64, _i32, _i32, _i32, _p]),
    "fe_facemass_strided_f64": (_int, [_p, _i64, _p, _pp, _i64, _pp, _i64, _i32, _i32, _i32, _i32, _i32, _p]),
    "fe_launch_f32": (_int, [_i32, C.POINTER(ArgPack), _p]),
    "fe_set_tail_rounds": (_int, [_i32]),
    "fe_set_tail_min_rounds": (_int, [_i32]),
    "fe_stream_retired": (_int, [_p]),
    "fe_tail_check": (_int, [_i32, C.POINTER(_i64), C.POINTER(_i32), C.POINTER(_i32), C.POINTER(_i32)]),
    "fe_capture_id": (_int, [_p, C.POINTER(C.c_uint64)]),
    "fe_graph_retired": (_int, [C.c_uint64]),
    "fe_tail_stats": (_int, [C.POINTER(_i64), _i32]),
    "fe_tail_plant": (_int, [_p, C.c_uint32]),
    "fe_set_temporal_loads_mib": (_int, [_i32]),
    "fe_set_write_through_mib": (_int, [_i32]),
    "fe_last_launch_info": (_int, [C.POINTER(_i64), _i32]),
    "fe_set_div_interleave": (_i64, [_i64]),
    "fe_set_div_quarter_tail": (_int, [_i32]),
    "fe_set_grad_quarter_tail": (_int, [_i32]),
    "fe_set_grad_staggered_start": (_int, [_i32]),
    "fe_set_phase_priority_p5": (_int, [_i32]),
    "fe_set_cu_limit": (_int, [_i32]),
    "fe_time_launches": (_int, [_i32, C.POINTER(ArgPack), _i32, _p, C.POINTER(C.c_float)]),
    "fe_einsum_generic": (_int, [C.POINTER(EinsumDesc), _pp, _p, _p]),
    "fe_einsum_contract": (_int, [C.POINTER(EinsumDesc), _pp, _p, _p]),
    "fe_einsum_contract_acc": (_int, [C.POINTER(EinsumDesc), _pp, _p, _f64, _f64, _p]),
    "fe_einsum_contract_groups": (_int, [C.POINTER(EinsumDesc), C.POINTER(_i32), C.POINTER(_i32)]),
    "fe_einsum_reduce_plan": (_int, [C.POINTER(EinsumDesc), C.POINTER(_i32), C.POINTER(_i64), C.POINTER(_size)]),
    "fe_einsum_reduce": (_int, [C.POINTER(EinsumDesc), _pp, _p, _p, _size, _p]),
    "fe_einsum_reduce_acc": (_int, [C.POINTER(EinsumDesc), _pp, _p, _p, _size, _f64, _f64, _p]),
    "fe_geomadj_f64": (_int, [_p, _p, _p, _p, _i64, _i32, _i32, _i32, _i32, _i64, _i64, _i64, _p]),
    "fe_facemass_adj_f64": (_int, [_p, _p, _pp, _pp, _pp, _p, _i64, _i32, _i32, _i32, _i32, _i32, _p]),
    "fe_opgrad_plan": (_int, [_i64, _i32, C.POINTER(_i64), C.POINTER(_size)]),
    "fe_opgrad_f64": (_int, [_p, _pp, _pp, _p, _i64, _i32, _i32, _i32, _i32, _i64, _i64, _i64, _i64, _i64, _i64, _p, _size,
                          _p]),
    "fe_facemass_opgrad_f64": (_int, [_p, _pp, _pp, _p, _i64, _i32, _i32, _i32, _i32, _i32, _p, _size, _p]),
    "fe_weightedop_f64": (_int, [_p, _p, _p, _pp, _pp, _i64, _i32, _i32, _i32, _i32, _i32, _p]),
    "fe_weightedop_supported": (_int, [_i32, _i32, _i32]),
    "fe_weightgrad_f64": (_int, [_p, _p, _pp, _pp, _p, _i64, _i32, _i32, _i32, _i32, _i32, _p]),
    "fe_weightgrad_supported": (_int, [_i32, _i32, _i32]),
    "fe_elemop_f64": (_int, [_p, _p, _pp, _pp, _i64, _i32, _i32, _i32, _i32, _p]),
    "fe_elemop_supported": (_int, [_i32, _i32]),
}
EXPORTED_SYMBOLS = tuple(SIGNATURES)


def library_path() -> Path:
    """``$FEINSUM_HIP_LIB`` if set, else the in-tree ``feinsum_amd/libfeinsum_hip.so``."""
    env = os.environ.get("FEINSUM_HIP_LIB")
    return Path(env) if env else Path(__file__).resolve().parent / "libfeinsum_hip.so"


_lib: Optional[C.CDLL] = None


def load_library() -> C.CDLL:
    """Load (once) and type the shared library; never falls back to anything."""
    global _lib
    if _lib is not None:
        return _lib
    path = library_path()
    if not path.exists():
        raise HipLibraryError(
            f"{path} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'`"
            " (hipcc --offload-arch=gfx950) or point FEINSUM_HIP_LIB at it")
    # torch's wheel carries its own HIP runtime (torch/lib/libamdhip64.so, soname libamdhip64.so.7) and asks for it by FILE name:
    # loaded after this library -- which resolves libamdhip64.so.7 to /opt/rocm/lib -- it becomes a SECOND runtime in the process,
    # and launches here then fail with "no ROCm-capable device is detected" while torch owns the device.  Loaded first, its soname
    # satisfies this library too: one runtime.  (A process without torch -- the C ABI's other callers -- has only one anyway.)
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    try:
        lib = C.CDLL(str(path))
    except OSError as exc:
        raise HipLibraryError(f"cannot load {path}: {exc}") from exc

    for name, (restype, argtypes) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, argtypes
    _lib = lib
    return lib


def check(rc: int) -> None:
    """Map a C return code to the Python exception the reference's callers expect."""
    if rc == FE_OK:
        return
    msg = (load_library().fe_last_error() or b"").decode("utf-8", "replace")
    if rc == FE_EINVAL:
        raise InvalidParameterError(msg)
    if rc == FE_EUNSUPPORTED:
        raise NotImplementedError(msg)
    raise HipLibraryError(f"HIP error ({rc}): {msg}")


def variant_code(variant) -> int:
    if variant is None:
        return VARIANT_AUTO
    if isinstance(variant, str):
        try:
            return VARIANTS[variant]
        except KeyError:
            raise InvalidParameterError(f"unknown kernel variant '{variant}'") from None
    return int(variant)


def device_info(dev: int = 0):
    """(name, peak fp64 GFLOP/s, peak GB/s) of HIP device *dev*."""
    lib = load_library()
    name = C.create_string_buffer(256)
    pf, pb = C.c_double(), C.c_double()
    check(lib.fe_device_info(dev, name, 256, C.byref(pf), C.byref(pb)))
    return name.value.decode(), pf.value, pb.value


def _ptr_array(ptrs: Sequence[int]):
    arr = (C.c_void_p * len(ptrs))(*ptrs)
    return arr


OP_TRANSPOSED = 1   # FE_OP_TRANSPOSED: operator stored [3][Np(j)][Np(i)]
OP_J_ES = 2         # FE_OP_J_ES: div component, J stored [E][3]


def grad3d(J: int, D: int, u: int, out: int, E: int, Np: int, variant=None, stream: int = 0,
           op_flags: int = 0) -> None:
    check(load_library().fe_grad3d_f64_ex(J, D, u, out, E, Np, op_flags, variant_code(variant), stream))


def div3d(J: int, D: int, u: int, out: int, E: int, Np: int, variant=None, stream: int = 0,
          op_flags: int = 0) -> None:
    check(load_library().fe_div3d_f64_ex(J, D, u, out, E, Np, op_flags, variant_code(variant), stream))


def divcomp3d(J: int, D: int, u: int, out: int, E: int, Np: int, variant=None, stream: int = 0,
              op_flags: int = 0) -> None:
    check(load_library().fe_divcomp3d_f64(J, D, u, out, E, Np, op_flags, variant_code(variant), stream))


def grad3d_batched(J: int, D: int, u: Sequence[int], out: Sequence[int], E: int, Np: int,
                   variant=None, stream: int = 0, op_flags: int = 0) -> None:
    """``len(u)`` fields through one grad launch, sharing J and D."""
    if len(u) != len(out):
        raise InvalidParameterError("grad: need as many outputs as fields")
    check(load_library().fe_grad3d_batched_f64(J, D, _ptr_array(u), _ptr_array(out), E, Np, len(u),
                                               op_flags, variant_code(variant), stream))


def div3d_batched(J: int, D: int, u: Sequence[int], out: Sequence[int], E: int, Np: int,
                  variant=None, stream: int = 0, op_flags: int = 0) -> None:
    """``len(u)`` fields through one div launch, sharing J and D."""
    if len(u) != len(out):
        raise InvalidParameterError("div: need as many outputs as fields")
    check(load_library().fe_div3d_batched_f64(J, D, _ptr_array(u), _ptr_array(out), E, Np, len(u),
                                              op_flags, variant_code(variant), stream))


def gradplanes3d(J3: Sequence[int], D: int, u: Sequence[int], out: Sequence[Optional[int]], E: int,
                 Np: int, variant=None, stream: int = 0, op_flags: int = 0) -> None:
    """Rows of a batched 're,rij,ej->ei' sharing u and D: ``out[3k + x]`` from ``J3[x]`` and ``u[k]``
    (``None`` = plane not wanted)."""
    if len(J3) != 3 or len(out) != 3 * len(u):
        raise InvalidParameterError("grad planes: need 3 J arrays and 3 output slots per field")
    check(load_library().fe_gradplanes3d_f64(_ptr_array(J3), D, _ptr_array(u), _ptr_array(out), E, Np,
                                             len(u), op_flags, variant_code(variant), stream))


def matapply(J: Optional[int], D: int, u: Sequence[int], out: Sequence[int], E: int, Np: int,
             variant=None, stream: int = 0, op_flags: int = 0) -> None:
    """``out_k[e,i] = J[e] sum_j D[i,j] u_k[e,j]`` for ``len(u)`` fields (``J = None``: no factor)."""
    if len(u) != len(out):
        raise InvalidParameterError("matapply: need as many outputs as fields")
    check(load_library().fe_matapply_f64(J, D, _ptr_array(u), _ptr_array(out), E, Np, len(u), op_flags,
                                         variant_code(variant), stream))


def graddiv3d(J: int, D: int, u_grad: int, v_div: int, grad_out: int, div_out: int, E: int,
              Np: int, variant=None, stream: int = 0) -> None:
    check(load_library().fe_graddiv3d_f64(J, D, u_grad, v_div, grad_out, div_out, E, Np,
                                          variant_code(variant), stream))


def waveop3d(J: int, D: int, u_grad: int, grad_out: int, v_div: int, div_out: int, Jface: int, R: int,
             f: Sequence[int], lift: Sequence[int], E: int, Np: int, nf: int, Nfp: int,
             fm_layout_flags: int = 0, variant=None, stream: int = 0) -> None:
    """div(v), grad(u) and the lift of ``len(f)`` face fields in one persistent launch."""
    if len(f) != len(lift):
        raise InvalidParameterError("waveop: need as many lift outputs as face fields")
    check(load_library().fe_waveop3d_f64(J, D, u_grad, grad_out, v_div, div_out, Jface, R,
                                         _ptr_array(f), _ptr_array(lift), E, Np, nf, Nfp, len(f),
                                         fm_layout_flags, variant_code(variant), stream))


def facemass(J: int, R: int, v: Sequence[int], out: Sequence[int], E: int, Np: int, nf: int,
             Nfp: int, layout_flags: int = 0, variant=None, stream: int = 0) -> None:
    """``out_k[e,i] = sum_fj J[e,f] R[f,i,j] v_k[f,e,j]`` for ``len(v)`` fields (fe_facemass_f64).  On the matrix cores for
    tetrahedra and triangles p = 1..5 and any number of fields: one field runs the single-field kernel, with the bits it has as
    a member of a larger call."""
    if len(v) != len(out):
        raise InvalidParameterError("face-mass: need as many outputs as fields")
    check(load_library().fe_facemass_f64(J, R, _ptr_array(v), _ptr_array(out), E, Np, nf, Nfp,
                                         len(v), layout_flags, variant_code(variant), stream))


def facemass_acc(J: int, R: int, v: Sequence[int], out: Sequence[int], E: int, Np: int, nf: int, Nfp: int,
                 alpha: float, beta: float, layout_flags: int = 0, stream: int = 0) -> None:
    """``out_k <- alpha * facemass_k + beta * out_k`` (fe_facemass_acc_f64).  NotImplementedError: the shape has no fused
    kernel (tetrahedra p = 1..4, two or more fields)."""
    if len(v) != len(out):
        raise InvalidParameterError("face-mass: need as many outputs as fields")
    check(load_library().fe_facemass_acc_f64(J, R, _ptr_array(v), _ptr_array(out), E, Np, nf, Nfp, len(v), layout_flags,
                                             float(alpha), float(beta), stream))


def grad3d_acc(J: int, D: int, u: int, out: int, E: int, Np: int, alpha: float, beta: float, op_flags: int = 0,
               stream: int = 0) -> None:
    """``out <- alpha * grad(u) + beta * out`` inside the matrix-core kernel (fe_grad3d_acc_f64).  NotImplementedError: the
    order has no accumulating kernel (tetrahedra p = 1..4)."""
    check(load_library().fe_grad3d_acc_f64(J, D, u, out, E, Np, op_flags, float(alpha), float(beta), stream))


def grad3d_strided(J: int, ldJ: int, D: int, u: Sequence[int], out: Sequence[int], ldOut: int, E: int, Np: int,
                   op_flags: int = 0, stream: int = 0) -> None:
    """grad on an element slice of larger arrays (fe_grad3d_strided_f64): ``E`` elements, the rows of J ``ldJ`` and the
    output planes ``ldOut * Np`` doubles apart.  Every pointer addresses element 0 of the slice."""
    if len(u) != len(out):
        raise InvalidParameterError("grad: need as many outputs as fields")
    check(load_library().fe_grad3d_strided_f64(J, ldJ, D, _ptr_array(u), _ptr_array(out), ldOut, E, Np, len(u), op_flags, stream))


def div3d_strided(J: int, ldJ: int, D: int, u: Sequence[int], ldIn: int, out: Sequence[int], E: int, Np: int,
                  op_flags: int = 0, stream: int = 0) -> None:
    """div on an element slice (fe_div3d_strided_f64): the planes of every field ``ldIn * Np`` doubles apart."""
    if len(u) != len(out):
        raise InvalidParameterError("div: need as many outputs as fields")
    check(load_library().fe_div3d_strided_f64(J, ldJ, D, _ptr_array(u), ldIn, _ptr_array(out), E, Np, len(u), op_flags, stream))


def facemass_strided(J: int, ldJ: int, R: int, v: Sequence[int], ldIn: int, out: Sequence[int], E: int, Np: int, nf: int,
                     Nfp: int, layout_flags: int = 0, stream: int = 0) -> None:
    """face-mass on an element slice (fe_facemass_strided_f64): the face slabs of every field ``ldIn * Nfp`` doubles apart,
    the rows of a J stored ``fe`` ``ldJ``.  NotImplementedError: one field, or a shape without a matrix-core kernel."""
    if len(v) != len(out):
        raise InvalidParameterError("face-mass: need as many outputs as fields")
    check(load_library().fe_facemass_strided_f64(J, ldJ, R, _ptr_array(v), ldIn, _ptr_array(out), E, Np, nf, Nfp, len(v),
                                                 layout_flags, stream))


def grad3d_mixed_state(J: int, D: int, u: Sequence[int], out: Sequence[int], E: int, Np: int, op_flags: int = 0,
                       stream: int = 0) -> None:
    """grad of float32 fields into float32 results, float64 J, operator and arithmetic (fe_grad3d_mixed_state_f64)."""
    if len(u) != len(out):
        raise InvalidParameterError("grad: need as many outputs as fields")
    check(load_library().fe_grad3d_mixed_state_f64(J, D, _ptr_array(u), _ptr_array(out), E, Np, len(u), op_flags, stream))


def div3d_mixed_state(J: int, D: int, u: Sequence[int], out: Sequence[int], E: int, Np: int, op_flags: int = 0,
                      stream: int = 0) -> None:
    """div of float32 fields into float32 results (fe_div3d_mixed_state_f64)."""
    if len(u) != len(out):
        raise InvalidParameterError("div: need as many outputs as fields")
    check(load_library().fe_div3d_mixed_state_f64(J, D, _ptr_array(u), _ptr_array(out), E, Np, len(u), op_flags, stream))


def facemass_mixed_state(J: int, R: int, v: Sequence[int], out: Sequence[int], E: int, Np: int, nf: int, Nfp: int,
                         layout_flags: int = 0, stream: int = 0) -> None:
    """face-mass of float32 fields into float32 results (fe_facemass_mixed_state_f64)."""
    if len(v) != len(out):
        raise InvalidParameterError("face-mass: need as many outputs as fields")
    check(load_library().fe_facemass_mixed_state_f64(J, R, _ptr_array(v), _ptr_array(out), E, Np, nf, Nfp, len(v),
                                                     layout_flags, stream))


def div3d_acc(J: int, D: int, u: int, out: int, E: int, Np: int, alpha: float, beta: float, op_flags: int = 0,
              stream: int = 0) -> None:
    """``out <- alpha * div(u) + beta * out`` inside the matrix-core kernel (fe_div3d_acc_f64); as :func:`grad3d_acc`."""
    check(load_library().fe_div3d_acc_f64(J, D, u, out, E, Np, op_flags, float(alpha), float(beta), stream))


def elemop(J: Optional[int], A: int, u: Sequence[int], out: Sequence[int], E: int, Ni: int, Nj: int, op_flags: int = 0,
           stream: int = 0) -> None:
    """The element-local operator of any shape on the matrix cores (fe_elemop_f64): ``out_k[e, i] = [J[e]] sum_j A[i, j]
    u_k[e, j]``, A ``(Ni, Nj)`` or stored ``(Nj, Ni)`` with ``OP_TRANSPOSED``.  NotImplementedError: (Ni, Nj) outside
    :func:`elemop_supported`."""
    if len(u) != len(out):
        raise InvalidParameterError("elemop: need as many outputs as fields")
    check(load_library().fe_elemop_f64(J, A, _ptr_array(u), _ptr_array(out), E, Ni, Nj, len(u), op_flags, stream))


def elemop_supported(Ni: int, Nj: int) -> bool:
    """The size rule of fe_elemop_f64, asked of the library (host only: no device needed)."""
    return bool(load_library().fe_elemop_supported(int(Ni), int(Nj)))


WO_P_T = 1   # FE_WO_P_T: P stored [Nq][Ni]
WO_A_T = 2   # FE_WO_A_T: A stored [Nj][Nq]


def weightedop(P: int, W: int, A: int, u: Sequence[int], out: Sequence[int], E: int, Ni: int, Nq: int, Nj: int,
               op_flags: int = 0, stream: int = 0) -> None:
    """The weighted element operator in one matrix-core kernel (fe_weightedop_f64): ``out_k[e, i] = sum_q P[i, q] W[e, q]
    sum_j A[q, j] u_k[e, j]``, P ``(Ni, Nq)`` or stored ``(Nq, Ni)`` with ``WO_P_T``, A ``(Nq, Nj)`` or stored ``(Nj, Nq)``
    with ``WO_A_T``.  NotImplementedError: (Ni, Nq, Nj) outside :func:`weightedop_supported`."""
    if len(u) != len(out):
        raise InvalidParameterError("weightedop: need as many outputs as fields")
    check(load_library().fe_weightedop_f64(P, W, A, _ptr_array(u), _ptr_array(out), E, Ni, Nq, Nj, len(u), op_flags, stream))


def weightedop_supported(Ni: int, Nq: int, Nj: int) -> bool:
    """The size rule of fe_weightedop_f64, asked of the library (host only: no device needed)."""
    return bool(load_library().fe_weightedop_supported(int(Ni), int(Nq), int(Nj)))


def weightgrad(P: int, A: int, u: Sequence[int], g: Sequence[int], dW: int, E: int, Ni: int, Nq: int, Nj: int,
               op_flags: int = 0, stream: int = 0) -> None:
    """The gradient of the weighted element operator with respect to its weight (fe_weightgrad_f64): ``dW[e, q] = sum_k
    (sum_i P[i, q] g_k[e, i]) (sum_j A[q, j] u_k[e, j])`` over at most 8 field pairs, P and A stored as for
    :func:`weightedop`.  NotImplementedError: (Ni, Nq, Nj) outside :func:`weightgrad_supported`."""
    if len(u) != len(g):
        raise InvalidParameterError("weightgrad: need as many output gradients as fields")
    check(load_library().fe_weightgrad_f64(P, A, _ptr_array(u), _ptr_array(g), dW, E, Ni, Nq, Nj, len(u), op_flags, stream))


def weightgrad_supported(Ni: int, Nq: int, Nj: int) -> bool:
    """The size rule of fe_weightgrad_f64, asked of the library (host only: no device needed)."""
    return bool(load_library().fe_weightgrad_supported(int(Ni), int(Nq), int(Nj)))


def axpby(out: int, x: int, n: int, alpha: float, beta: float, float64: bool = True, stream: int = 0) -> None:
    """``out[i] <- alpha * x[i] + beta * out[i]`` over *n* contiguous entries (fe_axpby); ``beta == 0`` does not read *out*."""
    check(load_library().fe_axpby(out, x, int(n), float(alpha), float(beta), FE_DTYPE_F64 if float64 else FE_DTYPE_F32,
                                  stream))


def geomadj(D: int, a: int, b: int, out: int, E: int, X: int, R: int, Np: int, strides: Sequence[int],
            op_flags: int = 0, stream: int = 0) -> None:
    """``out[x sx + r sr + e se] = sum_i (sum_j K[r, i, j] a[e, j]) b[x, e, i]`` (fe_geomadj_f64; *strides* = (sx, sr, se))."""
    sx, sr, se = (int(v) for v in strides)
    check(load_library().fe_geomadj_f64(D, a, b, out, E, X, R, Np, op_flags, sx, sr, se, stream))


def facemass_adj(J: Optional[int], R: int, g: Sequence[int], v: Optional[Sequence[int]], dv: Optional[Sequence[int]],
                 dJ: Optional[int], E: int, Np: int, nf: int, Nfp: int, layout_flags: int = 0, stream: int = 0) -> None:
    """The face-mass adjoint (fe_facemass_adj_f64): *dv* (None: skipped) and *dJ* summed over the fields (*v* None:
    skipped)."""
    if dv is not None and len(dv) != len(g) or v is not None and len(v) != len(g):
        raise InvalidParameterError("face-mass adjoint: need as many v / dv arrays as output gradients")
    check(load_library().fe_facemass_adj_f64(J, R, _ptr_array(g), _ptr_array(v) if v is not None else None,
                                             _ptr_array(dv) if dv is not None else None, dJ, E, Np, nf, Nfp,
                                             len(g), layout_flags, stream))


PREPARED_OPERATOR_BYTES = 96 * 1024   # FE_PREPARED_OPERATOR_BYTES


def opgrad_plan(E: int, n_out_entries: int) -> Tuple[int, int]:
    """``(slices, workspace bytes)`` of an operator-gradient launch (``fe_opgrad_plan``, host only)."""
    slices, nbytes = C.c_int64(0), C.c_size_t(0)
    check(load_library().fe_opgrad_plan(E, n_out_entries, C.byref(slices), C.byref(nbytes)))
    return int(slices.value), int(nbytes.value)


def opgrad(J: Optional[int], a: Sequence[int], b: Sequence[int], out: int, E: int, X: int, R: int, Np: int,
           jstrides: Sequence[int], strides: Sequence[int], workspace: Optional[int], workspace_bytes: int,
           stream: int = 0) -> None:
    """``out[r sr + p sp + q sq] = sum_k sum_e (sum_x J[x jx + r jr + e je] b_k[x][e][p]) a_k[e][q]`` (fe_opgrad_f64;
    *jstrides* = (jx, jr, je), *strides* = (sr, sp, sq))."""
    check(load_library().fe_opgrad_f64(J, _ptr_array(a), _ptr_array(b), out, E, len(a), X, R, Np, *jstrides, *strides,
                                       workspace, workspace_bytes, stream))


def facemass_opgrad(J: Optional[int], g: Sequence[int], v: Sequence[int], dR: int, E: int, Np: int, nf: int, Nfp: int,
                    workspace: Optional[int], workspace_bytes: int, layout_flags: int = 0, stream: int = 0) -> None:
    """``dR[f, i, j] = sum_k sum_e g_k[e][i] J[e, f] v_k[f][e][j]`` in R's layout (fe_facemass_opgrad_f64)."""
    check(load_library().fe_facemass_opgrad_f64(J, _ptr_array(g), _ptr_array(v), dR, E, Np, nf, Nfp, len(g), layout_flags,
                                                workspace, workspace_bytes, stream))


def prepare_operator(family: int, op: int, Np: int, nf: int, Nfp: int, flags: int, prepared: int,
                     stream: int = 0) -> None:
    """Write operator *op* in the kernels' fragment layout into the device buffer *prepared*
    (PREPARED_OPERATOR_BYTES bytes).  NotImplementedError: this shape has no prepared form."""
    check(load_library().fe_prepare_operator(family, op, Np, nf, Nfp, flags, prepared, stream))


def release_prepared(prepared: int) -> None:
    """Drop the library's record of a prepared-operator buffer (before the buffer is freed)."""
    check(load_library().fe_release_prepared(prepared))


def split_alloc(nbytes: int) -> int:
    """Device pointer of a new array of the split allocator on the CURRENT device (fe_split_alloc)."""
    ptr = C.c_void_p()
    check(load_library().fe_split_alloc(C.byref(ptr), nbytes, 0))
    return int(ptr.value)


def split_free(ptr: int) -> None:
    check(load_library().fe_split_free(ptr))


def _json_call(fn, *args) -> dict:
    import json

    buf = C.create_string_buffer(1 << 14)
    n = fn(*args, buf, len(buf))
    if n < 0:
        check(n)
    return json.loads(buf.value.decode())


def split_info(ptr: int) -> dict:
    """What the split allocator did for one array: bytes, mapped bytes, class of every piece, milliseconds."""
    return _json_call(load_library().fe_split_info, ptr)


def split_stats() -> dict:
    """The current device's pool of the split allocator."""
    return _json_call(load_library().fe_split_stats)


def split_reserve(nbytes: int) -> None:
    check(load_library().fe_split_reserve(C.c_size_t(int(nbytes))))


def split_trim() -> None:
    check(load_library().fe_split_trim())


def kernel_resources() -> str:
    """Registers / LDS / resident blocks per CU of the kernels configured so far in this process."""
    buf = C.create_string_buffer(1 << 16)
    n = load_library().fe_kernel_resources(buf, len(buf))
    if n < 0:
        check(n)
    return buf.value.decode()


def flops_per_element(family: int, Np: int, nf: int = 0, Nfp: int = 0, b: int = 1) -> int:
    return int(load_library().fe_flops_per_element(family, Np, nf, Nfp, b))


def time_launches(family: int, pack: ArgPack, n_launches: int, stream: int = 0) -> float:
    """Milliseconds for *n_launches* back-to-back launches (HIP events on *stream*)."""
    ms = C.c_float()
    check(load_library().fe_time_launches(family, C.byref(pack), n_launches, stream, C.byref(ms)))
    return float(ms.value)


def einsum_generic(desc: EinsumDesc, operands: Sequence[int], out: int, stream: int = 0) -> None:
    check(load_library().fe_einsum_generic(C.byref(desc), _ptr_array(operands), out, stream))


def einsum_dtype_code(float64: bool, operand_dtypes: Optional[Sequence] = None) -> int:
    """The ``dtype`` field of an einsum descriptor: ``FE_DTYPE_F64`` / ``FE_DTYPE_F32``, and with float64 compute one
    ``FE_DTYPE_OPERAND_F32(p)`` flag per float32 operand p of *operand_dtypes* (numpy dtypes; ``None``: no flags)."""
    code = FE_DTYPE_F64 if float64 else FE_DTYPE_F32
    if float64 and operand_dtypes is not None:
        for p, dt in enumerate(operand_dtypes):
            if np.dtype(dt) == np.dtype("float32"):
                code |= FE_DTYPE_OPERAND_F32(p)
    return code


def einsum_desc(in_idxs: Sequence[str], out_idxs: Sequence[str], sum_idxs: Sequence[str], extent, tensors: Sequence,
                float64: bool, operand_dtypes: Optional[Sequence] = None) -> EinsumDesc:
    """The descriptor of ``fe_einsum_generic`` / ``fe_einsum_contract`` for operands *tensors* (torch tensors, any strides)
    whose axes carry the indices *in_idxs* (one string per operand); the output is C-contiguous in *out_idxs* order.
    A repeated index adds its strides.  *operand_dtypes* (with *float64*): the float32 operands of a mixed einsum, which
    the kernels widen to float64 as they load them (:func:`einsum_dtype_code`)."""
    if len(in_idxs) > FE_MAX_EINSUM_OPERANDS or len(out_idxs) > FE_MAX_EINSUM_INDICES \
            or len(sum_idxs) > FE_MAX_EINSUM_INDICES:
        raise NotImplementedError("einsum has more operands / indices than the generic kernel supports")
    out_idxs, sum_idxs = list(out_idxs), list(sum_idxs)
    d = EinsumDesc()
    d.n_operands, d.n_out, d.n_sum = len(in_idxs), len(out_idxs), len(sum_idxs)
    d.dtype = einsum_dtype_code(float64, operand_dtypes)
    for k, idx in enumerate(out_idxs):
        d.out_extent[k] = extent[idx]
    for k, idx in enumerate(sum_idxs):
        d.sum_extent[k] = extent[idx]
    for p, (t, idxs) in enumerate(zip(tensors, in_idxs)):
        strides = t.stride()
        for axis, idx in enumerate(idxs):
            if idx in out_idxs:
                d.op_out_stride[p][out_idxs.index(idx)] += strides[axis]
            else:
                d.op_sum_stride[p][sum_idxs.index(idx)] += strides[axis]
    return d


def time_with_events(launch, n: int, stream_ptr: int) -> float:
    """Seconds for *n* calls of ``launch(stream_ptr)``, by HIP events recorded on that stream."""
    import torch

    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    stream = torch.cuda.ExternalStream(stream_ptr) if stream_ptr else torch.cuda.current_stream()
    t0.record(stream)
    for _ in range(n):
        launch(stream_ptr)
    t1.record(stream)
    t1.synchronize()
    return t0.elapsed_time(t1) * 1e-3


CONTRACT_GROUP_NAMES = {-1: "dropped", 0: "batch", 1: "m", 2: "n", 3: "k"}   # FE_CONTRACT_*


def einsum_contract_groups(desc: EinsumDesc):
    """``(output groups, summed groups)``: the index groups ``fe_einsum_contract`` forms for *desc* (host only), by name
    (``CONTRACT_GROUP_NAMES``)."""
    og, sg = (C.c_int32 * FE_MAX_EINSUM_INDICES)(), (C.c_int32 * FE_MAX_EINSUM_INDICES)()
    check(load_library().fe_einsum_contract_groups(C.byref(desc), og, sg))
    return (tuple(CONTRACT_GROUP_NAMES[og[k]] for k in range(desc.n_out)),
            tuple(CONTRACT_GROUP_NAMES[sg[k]] for k in range(desc.n_sum)))


def einsum_contract(desc: EinsumDesc, operands: Sequence[int], out: int, stream: int = 0) -> None:
    """Two-operand einsum on the matrix cores (``fe_einsum_contract``); same descriptor as :func:`einsum_generic`."""
    check(load_library().fe_einsum_contract(C.byref(desc), _ptr_array(operands), out, stream))


def einsum_contract_acc(desc: EinsumDesc, operands: Sequence[int], out: int, alpha: float, beta: float,
                        stream: int = 0) -> None:
    """``out <- alpha * E + beta * out`` inside the contraction kernel (``fe_einsum_contract_acc``), *E* what
    :func:`einsum_contract` stores; ``beta == 0`` does not read *out*."""
    check(load_library().fe_einsum_contract_acc(C.byref(desc), _ptr_array(operands), out, float(alpha), float(beta),
                                                stream))


REDUCE_PATH_NAMES = {FE_REDUCE_VALU: "valu", FE_REDUCE_MFMA: "mfma"}


def einsum_reduce_plan(desc: EinsumDesc) -> Tuple[str, int, int]:
    """``(path, slices, workspace bytes)`` of the split reduction of *desc* (``fe_einsum_reduce_plan``, host only):
    path ``"valu"`` or ``"mfma"``."""
    path, slices, nbytes = C.c_int32(), C.c_int64(), C.c_size_t()
    check(load_library().fe_einsum_reduce_plan(C.byref(desc), C.byref(path), C.byref(slices), C.byref(nbytes)))
    return REDUCE_PATH_NAMES[path.value], int(slices.value), int(nbytes.value)


def einsum_reduce(desc: EinsumDesc, operands: Sequence[int], out: int, workspace: int, workspace_bytes: int,
                  stream: int = 0) -> None:
    """Split reduction (``fe_einsum_reduce``): same descriptor as :func:`einsum_generic`, plus a 256-byte aligned device
    workspace of at least the bytes :func:`einsum_reduce_plan` reports."""
    check(load_library().fe_einsum_reduce(C.byref(desc), _ptr_array(operands), out, workspace,
                                          C.c_size_t(int(workspace_bytes)), stream))


def einsum_reduce_acc(desc: EinsumDesc, operands: Sequence[int], out: int, workspace: int, workspace_bytes: int,
                      alpha: float, beta: float, stream: int = 0) -> None:
    """``out <- alpha * E + beta * out`` in the combine launch of the split reduction (``fe_einsum_reduce_acc``), *E* what
    :func:`einsum_reduce` stores; same workspace; ``beta == 0`` does not read *out*."""
    check(load_library().fe_einsum_reduce_acc(C.byref(desc), _ptr_array(operands), out, workspace,
                                              C.c_size_t(int(workspace_bytes)), float(alpha), float(beta), stream))


def set_tail_rounds(rounds: int) -> int:
    """Number of dynamic rounds at the end of the persistent walks (fe_set_tail_rounds; negative: static walk); returns the
    previous value.  A tuning knob -- results do not depend on it."""
    return int(load_library().fe_set_tail_rounds(int(rounds)))


def set_tail_min_rounds(rounds: int) -> int:
    """Launches of fewer than *rounds* full rounds walk statically (fe_set_tail_min_rounds; default 4); returns the previous
    setting.  A tuning knob -- results do not depend on it."""
    return int(load_library().fe_set_tail_min_rounds(int(rounds)))


def set_cu_limit(cus: int) -> int:
    """Size the persistent grids as if the device had *cus* compute units (fe_set_cu_limit; 0 = the device's own count);
    returns the previous limit.  Results do not depend on it."""
    return int(load_library().fe_set_cu_limit(int(cus)))


def stream_retired(stream: int) -> bool:
    """Tell the library that *stream* was destroyed, so that its ticket-counter group can serve another stream."""
    rc = int(load_library().fe_stream_retired(stream))
    if rc < 0:
        check(rc)
    return rc == 1


def tail_check(repair: bool = False) -> dict:
    """Wait for the device and verify that every ticket counter is zero (fe_tail_check): ``dirty_words`` must be 0."""
    dirty, groups, streams, captured = C.c_int64(), C.c_int32(), C.c_int32(), C.c_int32()
    check(load_library().fe_tail_check(int(bool(repair)), C.byref(dirty), C.byref(groups), C.byref(streams),
                                       C.byref(captured)))
    return {"dirty_words": int(dirty.value), "groups": int(groups.value), "streams": int(streams.value),
            "captured": int(captured.value)}


_TAIL_STATS = ("groups", "streams", "captured", "spare", "exhausted", "static_fallbacks", "grow_failures", "verified_after_error",
               "repaired_after_error", "live_captures", "max_groups", "hip_errors")


def tail_stats() -> dict:
    """Counters of the ticket-counter pool of the current device (fe_tail_stats): ``exhausted`` / ``static_fallbacks`` say how
    many launches that wanted tickets walked statically instead."""
    buf = (C.c_int64 * len(_TAIL_STATS))()
    n = int(load_library().fe_tail_stats(buf, len(_TAIL_STATS)))
    if n < 0:
        check(n)
    return {k: int(buf[i]) for i, k in enumerate(_TAIL_STATS[:n])}


def capture_id(stream: int) -> int:
    """Id of the stream capture in progress on *stream* (fe_capture_id; 0: not capturing)."""
    cid = C.c_uint64()
    check(load_library().fe_capture_id(stream, C.byref(cid)))
    return int(cid.value)


def graph_retired(cid: int) -> int:
    """The graph captured under *cid* and its executables are gone: its launches' counter groups may serve others
    (fe_graph_retired); returns how many groups came back."""
    rc = int(load_library().fe_graph_retired(int(cid)))
    if rc < 0:
        check(rc)
    return rc


def tail_plant(stream: int, value: int) -> None:
    """Test hook (fe_tail_plant): leave a stale ticket in the counter group of *stream*."""
    check(load_library().fe_tail_plant(stream, int(value)))


_LAST_LAUNCH = ("valid", "dynamic_walk", "temporal_loads", "write_through_stores", "blocks", "waves_per_block", "kind", "bodies", "tiles",
                "static_tiles")


def last_launch_info() -> dict:
    """What the launcher decided for the MFMA launch this thread enqueued last (fe_last_launch_info): the walk, the cache hints
    of loads and stores, the grid.  ``{}`` before the first such launch."""
    buf = (C.c_int64 * len(_LAST_LAUNCH))()
    n = int(load_library().fe_last_launch_info(buf, len(_LAST_LAUNCH)))
    if n < 0:
        check(n)
    d = {k: int(buf[i]) for i, k in enumerate(_LAST_LAUNCH[:n])}
    if not d.get("valid"):
        return {}
    d["interleaved"] = bool(d["kind"] & 4)
    d["quarter_tail"] = bool(d["kind"] & 8)
    d["staggered_start"] = bool(d["kind"] & 16)
    d["mixed_fields"] = bool(d["kind"] & 32)             # fe_grad3d_mixed_f64 / fe_div3d_mixed_f64 / fe_facemass_mixed_f64
    d["plain_field_loads"] = bool(d["kind"] & 64)        # ... with the fields through registers instead of LDS-DMA
    d["element_slice"] = bool(d["kind"] & 128)           # fe_grad3d_strided_f64 / fe_div3d_strided_f64 / fe_facemass_strided_f64
    d["float32_results"] = bool(d["kind"] & 256)         # fe_grad3d_mixed_state_f64 / fe_div3d_... / fe_facemass_mixed_state_f64
    d["dword_stores"] = bool(d["kind"] & 512)            # ... with one float per lane instead of 16-byte stores
    d["element_operator"] = bool(d["kind"] & 1024)       # fe_elemop_f64
    d["weighted_element_operator"] = bool(d["kind"] & 2048)   # fe_weightedop_f64
    d["weighted_weight_adjoint"] = bool(d["kind"] & 4096)     # fe_weightgrad_f64
    d["kind"] = "B build interleaved" if d["kind"] & 4 else "default"
    return d


def set_phase_priority_p5(on: bool) -> bool:
    """Phase priorities in the eight-wave p = 5 kernels (fe_set_phase_priority_p5); returns the previous setting."""
    return bool(load_library().fe_set_phase_priority_p5(1 if on else 0))


def set_div_quarter_tail(on: bool) -> bool:
    """The ragged last round of short interleaved div launches as quarter tiles (fe_set_div_quarter_tail); returns the previous
    setting."""
    return bool(load_library().fe_set_div_quarter_tail(1 if on else 0))


def set_grad_quarter_tail(on: bool) -> bool:
    """The ragged last round of short grad launches (one field, static walk) as quarter tiles (fe_set_grad_quarter_tail); returns
    the previous setting."""
    return bool(load_library().fe_set_grad_quarter_tail(int(on)))


def set_grad_staggered_start(on: bool) -> bool:
    """Short grad launches (one field, static walk, 2.5 to 4.5 rounds) start every second CU of an XCD half a tile period late
    (fe_set_grad_staggered_start); returns the previous setting."""
    return bool(load_library().fe_set_grad_staggered_start(1 if on else 0))


def set_div_interleave(tiles: int) -> int:
    """Short div launches of at most *tiles* tiles run on the interleaved kernel (fe_set_div_interleave; 0 = never); returns the
    previous setting."""
    return int(load_library().fe_set_div_interleave(int(tiles)))


def set_write_through_mib(mib: int) -> int:
    """grad launches that write at most *mib* MiB store write-through instead of non-temporally (fe_set_write_through_mib;
    0 = never); returns the previous setting.  A tuning knob."""
    return int(load_library().fe_set_write_through_mib(int(mib)))


def set_temporal_loads_mib(mib: int) -> int:
    """Launches whose inputs are at most *mib* MiB fetch their streamed operand with plain (cacheable) loads instead of
    non-temporal ones (fe_set_temporal_loads_mib; 0 = never); returns the previous setting.  A tuning knob."""
    return int(load_library().fe_set_temporal_loads_mib(int(mib)))
