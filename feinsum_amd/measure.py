"""
Evaluate, validate and time a :class:`BatchedEinsum` on an MI355X.

API mirror of the reference's ``feinsum.measure`` (reference:
``src/feinsum/measure.py``): :func:`timeit` (``:197-275``),
:func:`validate_batched_einsum_transform` (``:111-194``),
:func:`measure_giga_op_rate` (``:357-385``), :func:`get_roofline_flop_rate`
(``:388-418``), :func:`stringify_comparison_vs_roofline` (``:484-525``), the
input generator (``:63-108``) and the three protocol constants (``:35-37``).

What is different underneath: the reference lowers the einsum through loopy to
OpenCL and enqueues it with PyOpenCL; here :func:`evaluate` picks a
hand-written gfx950 kernel (``feinsum_amd.family``) and launches it through the
C ABI of ``libfeinsum_hip.so`` on a HIP stream.  PyTorch-ROCm is used only to
own device memory and streams.

Argument conventions kept from the reference:

``cq``         anything that names a device/stream: ``None`` (device 0), an int
               ordinal, a ``torch.device``, or a :class:`DeviceQueue`.
``transform``  the reference passes a loopy transformation here; loopy does not
               exist in this build, so a callable (or ``None``) is ignored and
               selects the default kernel variant, while a ``str`` / ``dict``
               (``"mfma"``, ``"generic"``, ``{"variant": "generic"}``) selects
               a variant explicitly (``"contraction"``: the einsum as strided batched
               contractions on the matrix cores, ``feinsum_amd.contraction``; ``"reduction"``: a long summation
               space summed into a small output as a split reduction over the whole chip,
               ``feinsum_amd.reduction``; ``"adjoint"``: the adjoint kernels of the DG families, for the einsums
               ``family.match_adjoint_family`` recognises only; ``"operator_adjoint"``: the
               operator-gradient kernels, for the einsums ``family.match_operator_adjoint`` recognises only;
               ``"mixed_family"``: grad, div and face-mass with float32 fields in float64 geometry factors and
               operators, for the einsums ``family.match_mixed_family`` recognises only, DESIGN.md §3j;
               ``"mixed_state"``: the same einsums with float32 RESULTS -- float64 arithmetic, one rounding to nearest
               where a result is stored, outputs allocated and expected as float32; ``"element_operator"``: the
               element-local operator ``ij,ej->ei`` / ``e,ij,ej->ei`` of any shape within ``family.ELEMENT_OPERATOR_RULE`` --
               rectangular, or square at any size -- on the matrix cores, for the einsums ``family.match_element_operator``
               recognises only); in a dict, ``"prepared": True`` lets a
               bound launch (``timeit``) use a prepared copy of its operator
               matrices; ``"placement"`` (or ``$FEINSUM_PLACEMENT``): ``timeit``
               allocates one array per operand as the reference does; with the
               default ``"split"`` the outputs come from the split allocator
               (``feinsum_amd.placement.zeros``; ``evaluate`` allocates the outputs it
               is not handed the same way), ``"separate"`` takes every array
               from torch; ``timeit_details(...).placement`` reports which was used;
               ``"accumulate"`` (``"kernel"`` / ``"axpby"`` / ``"epilogue"``): which way an accumulating
               ``evaluate(..., alpha=, beta=)`` adds onto its outputs, instead of what :func:`accumulate_route` picks.
``schedule``   followed by the ``"contraction"`` transform (default: the optimal one) and by the
               ``"reduction"`` transform where the einsum does not stream in one launch; the
               other kernels implement the optimal schedule and ignore it.

Inputs are drawn from ``numpy.random.default_rng(0)`` in **sorted argument-name
order** (the reference draws in hash order, which is not reproducible).
"""

from __future__ import annotations

import logging
from ctypes import byref as C_byref
from dataclasses import dataclass, field
from time import time
from types import MappingProxyType
from typing import Any, Dict, Mapping, Optional, Sequence, Tuple

import numpy as np

from feinsum_amd import _hip
from feinsum_amd.contraction import ContractionLaunch, auto_picks_contraction
from feinsum_amd.reduction import ReductionLaunch, auto_picks_reduction, check_reduction
from feinsum_amd.contraction_schedule import ContractionSchedule, count_ops
from feinsum_amd.diagnostics import (HipLibraryError, InvalidParameterError,
                                     NoDevicePeaksInfoError, TransformValidationError)
from feinsum_amd.einsum import INT_CLASSES, BatchedEinsum, SizeParam
from feinsum_amd.adjoint import AdjointLaunch
from feinsum_amd.family import (FAMILY_DIV, FAMILY_DIVCOMP, FAMILY_FACEMASS, FAMILY_GRAD,
                                FAMILY_GRADPLANES, OP_J_ES, KernelPlan,
                                ELEMENT_OPERATOR_RULE, MIXED_FAMILY_RULE, WEIGHTED_ELEMENT_OPERATOR_RULE,
                                element_operator_groups, match_adjoint_family, match_element_operator, match_family,
                                match_mixed_family, match_operator_adjoint, match_weighted_element_operator,
                                weighted_element_operator_groups)

logger = logging.getLogger(__name__)

N_WARMUP_ROUNDS = 5
N_MIN_TIMING_ROUNDS = 10
N_MIN_SIM_SECS = 2
LAUNCHES_PER_BATCH = 5


# --------------------------------------------------------------------------
# device / stream handle (stands in for pyopencl.CommandQueue)
# --------------------------------------------------------------------------

@dataclass(frozen=True)
class DeviceInfo:
    name: str


class DeviceQueue:
    """A HIP device + stream; duck-types the bits of ``cl.CommandQueue`` the
    reference uses (``cq.device.name``, ``cq.finish()``).

    *stream* need not be the calling thread's current stream.  Every array the library allocates for a launch on this
    queue -- outputs the caller does not hand in, prepared-operator buffers, intermediates, workspaces, the zero-filled
    arrays of :func:`generate_out_arrays` -- is allocated and filled under this queue's stream and belongs to it, as a
    tensor allocated inside ``torch.cuda.stream(stream)`` does: dropped, its memory goes to the next owner in this
    stream's order.  Arrays the caller allocates itself (inputs, ``out_dict``) stay the caller's to order against
    this stream."""

    def __init__(self, device: Any = 0, stream: Any = None) -> None:
        import torch

        if not torch.cuda.is_available():
            raise HipLibraryError("no HIP device visible to this process")
        self.torch_device = torch.device("cuda", device) if isinstance(device, INT_CLASSES) \
            else torch.device(device)
        if self.torch_device.index is None:
            self.torch_device = torch.device("cuda", torch.cuda.current_device())
        self._stream = stream

    @property
    def ordinal(self) -> int:
        return int(self.torch_device.index)

    @property
    def stream(self):
        import torch

        return self._stream if self._stream is not None else torch.cuda.current_stream(self.torch_device)

    @property
    def stream_ptr(self) -> int:
        return int(self.stream.cuda_stream)

    @property
    def device(self) -> DeviceInfo:
        name, _, _ = _hip.device_info(self.ordinal)
        return DeviceInfo(name)

    def finish(self) -> None:
        self.stream.synchronize()


def _on_stream_of(q: DeviceQueue):
    """Context in which allocations and fills belong to *q*'s stream: nothing at all where that stream is the current
    one (or a capture is in progress: its allocations are the capturing stream's), else ``torch.cuda.stream``."""
    import contextlib

    import torch

    if q._stream is None or q._stream == torch.cuda.current_stream(q.torch_device) or torch.cuda.is_current_stream_capturing():
        return contextlib.nullcontext()
    return torch.cuda.stream(q._stream)


def _as_queue(cq: Any) -> DeviceQueue:
    if isinstance(cq, DeviceQueue):
        return cq
    if cq is None:
        return DeviceQueue(0)
    return DeviceQueue(cq)


def _variant_from_transform(transform: Any):
    if transform is None or callable(transform):
        return None
    if isinstance(transform, Mapping):
        return transform.get("variant")
    return transform


def _prepared_from_transform(transform: Any, default: bool) -> bool:
    """``{"prepared": False}`` in a transform dict turns prepared operators off for a bound launch."""
    if isinstance(transform, Mapping) and "prepared" in transform:
        return bool(transform["prepared"])
    return default


# --------------------------------------------------------------------------
# arrays
# --------------------------------------------------------------------------

def get_real_dtype(dtype: np.dtype) -> np.dtype:
    return np.empty(0, dtype=dtype).real.dtype


def _concrete_shape(shape: Sequence[Any], long_dim_length: int) -> Tuple[int, ...]:
    return tuple(int(d) if isinstance(d, INT_CLASSES) else int(long_dim_length) for d in shape)


def _random_array(rng: np.random.Generator, dtype: np.dtype, shape: Tuple[int, ...]) -> np.ndarray:
    # reference: measure.py:63-77
    if dtype.kind == "c":
        real = get_real_dtype(dtype)
        return (rng.random(size=shape, dtype=real) + dtype.type(1j) * rng.random(size=shape, dtype=real))
    if dtype.kind == "i":
        return rng.integers(low=-100, high=100, size=shape, dtype=dtype)
    return rng.random(size=shape, dtype=dtype)


def generate_host_input_arrays(einsum: BatchedEinsum, long_dim_length: int,
                               np_seed: int = 0) -> Dict[str, np.ndarray]:
    """Host inputs: one ``default_rng(np_seed)``, arrays drawn in sorted-name order."""
    rng = np.random.default_rng(np_seed)
    return {name: _random_array(rng, einsum.arg_to_dtype[name],
                                _concrete_shape(einsum.arg_to_shape[name], long_dim_length))
            for name in sorted(einsum.arg_to_dtype)}


def generate_input_arrays(cq: Any, einsum: BatchedEinsum, long_dim_length: int,
                          np_seed: int = 0) -> Mapping[str, Any]:
    """Device inputs (reference: measure.py:80-108)."""
    import torch

    q = _as_queue(cq)
    host = generate_host_input_arrays(einsum, long_dim_length, np_seed)
    return MappingProxyType({name: torch.from_numpy(arr).to(q.torch_device)
                             for name, arr in host.items()})


def result_dtype(einsum: BatchedEinsum, row: int = 0, transform: Any = None) -> np.dtype:
    """dtype of an output = ``np.result_type`` of its operands (codegen/loopy.py:258-260) -- except under the transform
    ``"mixed_state"``, whose results are float32 (float64 arithmetic, rounded once at the store)."""
    if _variant_from_transform(transform) == "mixed_state":
        return np.dtype("float32")
    return np.result_type(*[arg.dtype for arg in einsum.args[row]])


def generate_out_arrays(cq: Any, einsum: BatchedEinsum, long_dim_length: int, *, split: bool = False,
                        transform: Any = None) -> Mapping[str, Any]:
    """Zero-filled device outputs ``_fe_out, _fe_out_0, ...`` (reference: measure.py:44-60).  *split*: one array each
    from the split allocator (``feinsum_amd.placement.zeros``: 4 MiB pieces alternating between two classes of physical
    memory) instead of the torch allocator; arrays below 8 MiB come from torch either way.  Allocated and zero-filled
    on the queue's stream (see :class:`DeviceQueue`): a launch on that queue is ordered behind the fill.  *transform*: the
    one the arrays are for (:func:`result_dtype`)."""
    import torch

    q = _as_queue(cq)
    shape = _concrete_shape(einsum.shape, long_dim_length)
    outs = {}
    with _on_stream_of(q):
        if split and len(einsum.output_names) > 1:   # several arrays, allocated one after the other: say what is coming
            from feinsum_amd import placement

            nbytes = sum(int(np.prod(shape)) * result_dtype(einsum, k, transform).itemsize for k in range(len(einsum.output_names)))
            if nbytes >= placement.SPLIT_MIN_BYTES:
                placement.split_reserve(nbytes, q.torch_device)
        for k, name in enumerate(einsum.output_names):
            tdtype = getattr(torch, result_dtype(einsum, k, transform).name)
            if split:
                from feinsum_amd import placement

                outs[name] = placement.zeros(shape, tdtype, q.torch_device)
            else:
                outs[name] = torch.zeros(shape, dtype=tdtype, device=q.torch_device)
    return MappingProxyType(outs)


# --------------------------------------------------------------------------
# the waist: run one BatchedEinsum on device arrays
# --------------------------------------------------------------------------

#: what takes element slices (``_bind``) -- quoted by every refusal of a view
ELEMENT_SLICE_RULE = ("element slices -- base.narrow(element axis, a, n) of a C-contiguous base -- are accepted for the inputs "
                      "and outputs (not the operator array) of float64 grad 'xre,rij,ej->xei', div 'xre,rij,xej->ei' and "
                      "face-mass 'ef,fij,fej->ei' (two or more fields per launch) of tetrahedra p = 1..4, under the transform "
                      "'auto' or 'mfma', with (alpha, beta) = (1, 0)")


def element_slice_ld(shape: Sequence[int], strides: Sequence[int], axis: int) -> Optional[int]:
    """
    The leading dimension of an element slice, or ``None``: *strides* (in elements) are the C-contiguous strides of
    *shape* with the extent of *axis* replaced by some ``ld >= shape[axis]`` -- what ``base.narrow(axis, a, n)`` of a
    contiguous ``base`` has (``ld`` is then the base's extent along *axis*).  A contiguous array gives ``shape[axis]``;
    steps, negative strides, transposes and expanded axes give ``None``.  As in torch, the stride of an axis of extent 1
    says nothing; an array without elements addresses nothing and gives ``shape[axis]``.  Where no axis in front of
    *axis* has an extent above 1 the array is contiguous whatever its base was, and the result is ``shape[axis]``.
    """
    shape, strides = tuple(int(n) for n in shape), tuple(int(n) for n in strides)
    if len(shape) != len(strides) or not 0 <= axis < len(shape) or any(n < 0 for n in shape):
        return None
    if 0 in shape:
        return shape[axis]
    inner = 1                                  # elements of one entry of `axis`
    for d in range(len(shape) - 1, axis - 1, -1):
        if shape[d] != 1 and strides[d] != inner:
            return None
        if d > axis:
            inner *= shape[d]
    ld, outer = None, 1                        # outer: extents between `axis` and d
    for d in range(axis - 1, -1, -1):
        if shape[d] != 1:
            unit = inner * outer
            if ld is None:
                if strides[d] <= 0 or strides[d] % unit:
                    return None
                ld = strides[d] // unit
                if ld < shape[axis]:
                    return None
            elif strides[d] != ld * unit:
                return None
        outer *= shape[d]
    return shape[axis] if ld is None else ld


def element_slice_spans(address: int, shape: Sequence[int], ld: int, axis: int, itemsize: int) -> Tuple[Tuple[int, int], ...]:
    """The ``(address, nbytes)`` span of every contiguous piece of an element slice (:func:`element_slice_ld`): one per
    entry of the axes in front of *axis* -- nine for a sliced J ``(3, 3, E)``, three for grad's output ``(3, E, Np)`` --
    or ONE where the pieces touch (``ld == shape[axis]``, or nothing in front of *axis*)."""
    shape = tuple(int(n) for n in shape)
    inner = int(np.prod(shape[axis + 1:], dtype=np.int64))
    n_outer = int(np.prod(shape[:axis], dtype=np.int64))
    piece = shape[axis] * inner * itemsize
    if n_outer <= 1 or ld == shape[axis] or piece == 0:
        return ((int(address), n_outer * piece),)
    return tuple((int(address) + k * ld * inner * itemsize, piece) for k in range(n_outer))


def _slice_axis(t: Any) -> Optional[int]:
    """The axis along which a tensor is an element slice (0 for a contiguous one), or None."""
    if t.is_contiguous():
        return 0
    shape, strides = tuple(t.shape), tuple(t.stride())
    return next((a for a in range(len(shape)) if element_slice_ld(shape, strides, a) is not None), None)


def _check_tensor(name: str, t: Any, shape: Tuple[int, ...], dtype: np.dtype, q: DeviceQueue,
                  slice_axis: Optional[int] = None) -> bool:
    """Shape, dtype, device and layout of one operand.  Returns True where *t* is not contiguous but an element slice
    along *slice_axis* (``_bind`` then decides whether the launch takes slices); any other layout is refused."""
    import torch

    if not isinstance(t, torch.Tensor):
        raise InvalidParameterError(f"argument '{name}' must be a torch.Tensor on the device")
    if t.device != q.torch_device:
        raise InvalidParameterError(f"argument '{name}' lives on {t.device}, expected {q.torch_device}")
    if tuple(t.shape) != tuple(shape):
        raise InvalidParameterError(f"argument '{name}' has shape {tuple(t.shape)}, expected {shape}")
    if t.dtype != getattr(torch, dtype.name):
        raise InvalidParameterError(f"argument '{name}' has dtype {t.dtype}, expected {dtype}")
    if not t.is_contiguous():
        if slice_axis is not None and element_slice_ld(tuple(t.shape), tuple(t.stride()), slice_axis) is not None:
            return True
        raise InvalidParameterError(f"argument '{name}' must be C-contiguous ({ELEMENT_SLICE_RULE}; this view is not such"
                                    " a slice of this operand)")
    return False


def _long_length(einsum: BatchedEinsum, arg_dict: Mapping[str, Any]) -> Dict[str, int]:
    """Values of the size parameters, read off the arrays."""
    values: Dict[str, int] = {}
    for name, shape in einsum.arg_to_shape.items():
        for axis, d in enumerate(shape):
            if isinstance(d, SizeParam):
                got = int(arg_dict[name].shape[axis])
                if values.setdefault(d.name, got) != got:
                    raise InvalidParameterError(f"inconsistent values for size parameter '{d.name}'")
    return values


def _family_groups(plan: KernelPlan, einsum: BatchedEinsum) -> list:
    """The rows of each launch of a family plan, as ``range`` objects: consecutive rows that share J and the operator
    become one multi-field launch; div components go row by row."""
    role = plan.roles
    op_role = "D" if "D" in role else "R"
    key = lambda row: (row[role["J"]].name if "J" in role else None, row[role[op_role]].name)   # noqa: E731
    starts = [k for k, row in enumerate(einsum.args)
              if k == 0 or plan.family == FAMILY_DIVCOMP or key(row) != key(einsum.args[k - 1])]
    return [range(k, k2) for k, k2 in zip(starts, starts[1:] + [len(einsum.args)])]


class _FamilyLaunch:
    """A family plan bound to concrete device arrays: launch / time."""

    def __init__(self, plan: KernelPlan, einsum: BatchedEinsum, arg_dict: Mapping[str, Any],
                 outs: Sequence[Any], variant: Any, scale: Optional[Tuple[float, float]] = None) -> None:
        self.plan, self.variant = plan, _hip.variant_code(variant)
        # (alpha, beta) of a launch that accumulates inside its kernel -- face-mass, grad and div of tetrahedra
        # (FE_FAMILY_ACC: grad and div take one launch per field) -- else None
        self.scale = scale
        role = plan.roles
        rows = einsum.args
        long_role = "J" if "J" in role else "u"       # 'ij,ej->ei' has no geometry factor
        long_axis = einsum.in_idx_sets[role[long_role]].index(plan.long_index)
        self.E = int(arg_dict[rows[0][role[long_role]].name].shape[long_axis])
        self._keep = (arg_dict, outs)
        self._prepared: Dict[Any, Any] = {}   # (operator pointer, flags) -> prepared device buffer
        p = plan.params
        self.f32 = bool(p.get("f32"))         # all-float32 einsum: FE_FAMILY_F32, whatever the variant
        self.fields_f32 = bool(p.get("fields_f32"))   # float32 fields only (match_mixed_family): FE_FAMILY_FIELDS_F32
        self.groups = []   # list of ArgPack (one per launch)
        self.group_family = plan.family
        if not (plan.family == FAMILY_DIVCOMP and not self.f32 and self._bind_planes(einsum, arg_dict, outs)):
            op_role, in_role = ("D", "u") if "D" in role else ("R", "v")
            for group in _family_groups(plan, einsum):
                first = rows[group[0]]
                vptrs = [arg_dict[rows[m][role[in_role]].name].data_ptr() for m in group]
                optrs = [outs[m].data_ptr() for m in group]
                pack = _hip.ArgPack()
                pack.J = arg_dict[first[role["J"]].name].data_ptr() if "J" in role else None
                pack.D = arg_dict[first[role[op_role]].name].data_ptr()
                pack.u, pack.out = vptrs[0], optrs[0]
                va, oa = _hip._ptr_array(vptrs), _hip._ptr_array(optrs)
                self._keep += (va, oa)
                pack.v, pack.outs = va, oa
                pack.E, pack.Np = self.E, p["Np"]
                pack.nf, pack.Nfp, pack.ndim = p.get("nf", 0), p.get("Nfp", 0), p.get("ndim", 3)
                pack.b, pack.layout_flags, pack.variant = len(group), plan.layout_flags, self.variant
                self.groups.append(pack)
        #: what fe_launch is told to run: the family of the packs and how their arrays are read and written
        self.family_code = (self.group_family | (_hip.FAMILY_F32 if self.f32 else 0)
                            | (_hip.FAMILY_FIELDS_F32 if self.fields_f32 else 0)
                            | (_hip.FAMILY_ACC if scale is not None else 0))
        for pack in self.groups:
            pack.alpha, pack.beta = scale if scale is not None else (1.0, 0.0)

    def __del__(self) -> None:
        # the library keeps a record per prepared buffer (address -> shape, source operator): drop it before the buffer
        # is freed, or an unrelated later allocation at the same address would be taken for a prepared operator
        for buf in getattr(self, "_prepared", {}).values():
            try:
                _hip.release_prepared(buf.data_ptr())
            except Exception:   # noqa: BLE001  (interpreter shutdown)
                pass

    def prepare_operators(self, stream_ptr: int = 0) -> int:
        """Write the operator of every launch group that has a prepared form (grad / div / face-mass of
        tetrahedra p = 1..4, ``fe_prepare_operator``) into a device buffer owned by this bound launch;
        the launches then fetch their MFMA fragments from it instead of rebuilding them from the
        plain array every time.  The buffers are SNAPSHOTS: call this again after changing an
        operator array in place.  Returns the number of prepared groups.  New buffers are taken on the
        current stream: call it with the stream of *stream_ptr* current (``_bind`` does)."""
        import torch

        if self.f32 or self.fields_f32 or self.variant not in (_hip.VARIANT_AUTO, _hip.VARIANT_MFMA, _hip.VARIANT_MFMA_SPLIT) or self.group_family == FAMILY_GRADPLANES \
                or self.plan.family not in (FAMILY_GRAD, FAMILY_DIV, FAMILY_FACEMASS):
            return 0
        done = 0
        for pack in self.groups:
            if self.plan.family != FAMILY_FACEMASS and pack.ndim != 3:
                continue
            key = (pack.D, pack.layout_flags)
            buf = self._prepared.get(key)
            fresh = buf is None
            if fresh:    # on the stream that writes and reads it (the caller's current one: _bind switches to the queue's)
                device = self._keep[1][0].device
                buf = torch.empty(_hip.PREPARED_OPERATOR_BYTES, dtype=torch.uint8, device=device)
            flags = pack.layout_flags & ~1 if self.plan.family == FAMILY_FACEMASS else pack.layout_flags   # (not FM_J_FE)
            try:
                _hip.prepare_operator(self.plan.family, pack.D, pack.Np, pack.nf, pack.Nfp, flags, buf.data_ptr(),
                                      stream_ptr)
            except NotImplementedError:
                continue
            self._prepared[key] = buf
            pack.prepared = buf.data_ptr()
            done += 1
        return done

    def _bind_planes(self, einsum: BatchedEinsum, arg_dict: Mapping[str, Any], outs: Sequence[Any]) -> bool:
        """Rows of 're,rij,ej->ei' that share u and D (e.g. the curl-type batch of
        ``tuning/impls/re_rji_ej_to_ei_3d_cross_product_v0.py:220-231``) go through the grad-type
        planes launch, which forms D u once per field.  False: keep one launch per row.

        The rule: J stored ``re`` (not ``er``), tetrahedra, ONE operator name, at most three geometry-factor names,
        every field with the same number of planes, that number at least two, and no (field, factor) pair twice.
        Plane x of every field is the x-th factor name in sorted order, whatever the order of the rows; a field
        without that plane gets no output there."""
        role, rows = self.plan.roles, einsum.args
        if self.plan.layout_flags & OP_J_ES or self.plan.params.get("ndim", 3) != 3:
            return False
        if len({row[role["D"]].name for row in rows}) != 1:
            return False
        jnames = sorted({row[role["J"]].name for row in rows})
        fields: dict = {}
        for m, row in enumerate(rows):
            fields.setdefault(row[role["u"]].name, {})[row[role["J"]].name] = m
        n_planes = {len(planes) for planes in fields.values()}
        if (len(jnames) > 3 or len(n_planes) != 1 or next(iter(n_planes)) < 2
                or sum(len(planes) for planes in fields.values()) != len(rows)):
            return False
        jptrs = [arg_dict[jnames[min(x, len(jnames) - 1)]].data_ptr() for x in range(3)]
        uptrs = [arg_dict[name].data_ptr() for name in fields]
        optrs = [outs[planes[jn]].data_ptr() if jn in planes else None
                 for planes in fields.values() for jn in (jnames + [None] * 3)[:3]]
        pack = _hip.ArgPack()
        ja, ua, oa = _hip._ptr_array(jptrs), _hip._ptr_array(uptrs), _hip._ptr_array(optrs)
        self._keep += (ja, ua, oa)
        pack.j3, pack.v, pack.outs = ja, ua, oa
        pack.D = arg_dict[rows[0][role["D"]].name].data_ptr()
        pack.E, pack.Np, pack.b = self.E, self.plan.params["Np"], len(uptrs)
        pack.layout_flags, pack.variant = self.plan.layout_flags, self.variant
        self.groups.append(pack)
        self.group_family = FAMILY_GRADPLANES
        return True

    def launch(self, stream_ptr: int) -> None:
        lib = _hip.load_library()
        for pack in self.groups:
            _hip.check(lib.fe_launch(self.family_code, C_byref(pack), stream_ptr))

    def time_batch(self, n: int, stream_ptr: int) -> float:
        """Seconds for *n* launches of the whole batched einsum (HIP events)."""
        if len(self.groups) == 1 and self.scale is None:
            return _hip.time_launches(self.family_code, self.groups[0], n, stream_ptr) * 1e-3
        import torch

        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        stream = torch.cuda.ExternalStream(stream_ptr) if stream_ptr else torch.cuda.current_stream()
        t0.record(stream)
        for _ in range(n):
            self.launch(stream_ptr)
        t1.record(stream)
        t1.synchronize()
        return t0.elapsed_time(t1) * 1e-3


class _GenericLaunch:
    """Any other einsum: one generic-kernel launch per output row (float64 / float32 operands in any mix: the row's
    ``np.result_type`` is the compute and output type)."""

    def __init__(self, einsum: BatchedEinsum, arg_dict: Mapping[str, Any], outs: Sequence[Any]) -> None:
        dtypes = {np.dtype(dt) for dt in einsum.arg_to_dtype.values()}
        if not dtypes <= {np.dtype("float64"), np.dtype("float32")}:
            raise NotImplementedError(
                "the generic einsum kernel is compiled for float64 and float32 operands (mixed: float64 compute);"
                f" got {sorted(str(d) for d in dtypes)}")
        sizes = _long_length(einsum, arg_dict)
        extent = {idx: (sizes[d.name] if isinstance(d, SizeParam) else int(d))
                  for idx, d in einsum.index_to_dim_length.items()}
        if einsum.n > _hip.FE_MAX_EINSUM_OPERANDS or len(einsum.out_idx_set) > _hip.FE_MAX_EINSUM_INDICES \
                or len(einsum.sum_indices) > _hip.FE_MAX_EINSUM_INDICES:
            raise NotImplementedError("einsum has more operands / indices than the generic kernel supports")
        self._keep = (arg_dict, outs)
        self.launches = []
        for row, out in zip(einsum.args, outs):
            tensors = [arg_dict[a.name] for a in row]
            row_dtypes = [np.dtype(a.dtype) for a in row]   # mixed: float64 compute, float32 operands flagged
            d = _hip.einsum_desc(einsum.in_idx_sets, einsum.out_idx_set, einsum.sum_indices, extent, tensors,
                                 np.result_type(*row_dtypes) == np.dtype("float64"), row_dtypes)
            self.launches.append((d, [t.data_ptr() for t in tensors], out.data_ptr()))

    def launch(self, stream_ptr: int) -> None:
        for d, ops, out in self.launches:
            _hip.einsum_generic(d, ops, out, stream_ptr)

    def time_batch(self, n: int, stream_ptr: int) -> float:
        return _hip.time_with_events(self.launch, n, stream_ptr)


def _generic_kernel_is_the_einsum_one(plan: KernelPlan) -> bool:
    """float64 grad / div / div components of triangles have the matrix-core and the tiled kernels but no plain
    one-thread-per-entry kernel of their own: ``"generic"`` runs them on the generic einsum kernel."""
    return (plan.family in (FAMILY_GRAD, FAMILY_DIV, FAMILY_DIVCOMP) and plan.params.get("ndim") == 2
            and not plan.params.get("f32"))


def _overlap(a: Sequence[Tuple[int, int]], b: Sequence[Tuple[int, int]]) -> bool:
    """Do two lists of (address, nbytes) ranges share a byte?  (A range of no bytes shares none.)"""
    return any(pa < pb + nb and pb < pa + na for pa, na in a for pb, nb in b if na and nb)


def _span(t: Any) -> Tuple[int, int]:
    """(address, nbytes) of a contiguous tensor."""
    return int(t.data_ptr()), int(t.numel()) * int(t.element_size())


def _spans(t: Any) -> Tuple[Tuple[int, int], ...]:
    """The byte ranges of a tensor ``_bind`` accepts: one for a contiguous tensor, one per contiguous piece of an element
    slice (:func:`element_slice_spans`) -- so that two disjoint element ranges of one array do not overlap."""
    axis = _slice_axis(t)
    if axis is None:
        raise InvalidParameterError("a tensor that is neither C-contiguous nor an element slice has no byte ranges here")
    if axis == 0:                   # contiguous
        return (_span(t),)
    ld = element_slice_ld(tuple(t.shape), tuple(t.stride()), axis)
    return element_slice_spans(int(t.data_ptr()), tuple(t.shape), ld, axis, int(t.element_size()))


def _refuse_aliased_outputs(einsum: BatchedEinsum, arg_dict: Mapping[str, Any], given: Mapping[str, Any]) -> None:
    """The aliasing rule of :func:`evaluate`: no output handed in may share a byte with an input or with another
    output (the kernels read their operands while other threads already store results)."""
    names = list(given)
    for k, name in enumerate(names):
        for other in sorted(einsum.all_args):
            if _overlap(_spans(given[name]), _spans(arg_dict[other])):
                raise InvalidParameterError(
                    f"output '{name}' shares memory with input '{other}': an evaluation may not write what it reads"
                    " (hand in an output of its own)")
        for other in names[:k]:
            if _overlap(_spans(given[name]), _spans(given[other])):
                raise InvalidParameterError(
                    f"output '{name}' shares memory with output '{other}': every output needs memory of its own")


def launch_kind(einsum: BatchedEinsum, transform: Any, sizes: Mapping[str, int]) -> str:
    """
    Which kernels run *einsum* under *transform* (size parameters *sizes*): ``"reduction"`` (the transform of that
    name -- ``NotImplementedError`` above ``reduction.REDUCE_MAX_OUT`` output entries -- or ``"auto"`` outside the DG
    families where ``reduction.auto_picks_reduction`` finds a long summation space summed into a small output),
    ``"contraction"`` (the transform of that name, or ``"auto"`` on a two-operand einsum outside the DG families where
    ``contraction.auto_picks_contraction`` says the contraction kernel wins), ``"family"`` (a DG family kernel) or
    ``"generic"`` (also the ``"generic"`` transform on float64 grad / div / div components of triangles, which have no
    plain kernel of their own).  The reduction rule is checked before the contraction rule.  ``"adjoint"`` (that transform only: an
    einsum that ``family.match_adjoint_family`` recognises, else ``NotImplementedError``) runs the adjoint kernels, and
    ``"operator_adjoint"`` (that transform only: ``family.match_operator_adjoint``, else ``NotImplementedError``) the
    operator-gradient kernels.  ``"mixed_family"`` (that transform only: ``family.match_mixed_family``, else
    ``NotImplementedError`` naming the rule) runs the DG kernels for float32 fields, and ``"mixed_state"`` (that transform
    only, the same einsums, the same error) their forms with float32 results.  ``"element_operator"`` (that transform only:
    ``family.match_element_operator``, else ``NotImplementedError`` naming ``family.ELEMENT_OPERATOR_RULE``) runs the
    element-local operator of any shape on the matrix cores, and ``"weighted_element_operator"`` (that transform only:
    ``family.match_weighted_element_operator``, else ``NotImplementedError`` naming
    ``family.WEIGHTED_ELEMENT_OPERATOR_RULE``) the sandwich ``iq,eq,qj,ej->ei`` in one matrix-core kernel.
    """
    variant = _variant_from_transform(transform)
    if variant == "weighted_element_operator":
        if match_weighted_element_operator(einsum) is None:
            raise NotImplementedError(
                f"transform 'weighted_element_operator': einsum '{einsum.get_subscripts()}' x {einsum.b} is not "
                f"{WEIGHTED_ELEMENT_OPERATOR_RULE} (feinsum_amd.family.match_weighted_element_operator, "
                "WEIGHTED_ELEMENT_OPERATOR_RULE)")
        return "weighted_element_operator"
    if variant == "element_operator":
        if match_element_operator(einsum) is None:
            raise NotImplementedError(
                f"transform 'element_operator': einsum '{einsum.get_subscripts()}' x {einsum.b} is not {ELEMENT_OPERATOR_RULE}"
                " (feinsum_amd.family.match_element_operator, ELEMENT_OPERATOR_RULE)")
        return "element_operator"
    if variant in ("mixed_family", "mixed_state"):
        if match_mixed_family(einsum) is None:
            raise NotImplementedError(
                f"transform '{variant}': einsum '{einsum.get_subscripts()}' x {einsum.b} is not {MIXED_FAMILY_RULE}"
                " (feinsum_amd.family.match_mixed_family)")
        return variant
    if variant == "adjoint":
        if match_adjoint_family(einsum) is None:
            raise NotImplementedError(
                f"einsum '{einsum.get_subscripts()}' is not one of the adjoint kernels' shapes"
                " (feinsum_amd.family.match_adjoint_family)")
        return "adjoint"
    if variant == "operator_adjoint":
        if match_operator_adjoint(einsum) is None:
            raise NotImplementedError(
                f"transform 'operator_adjoint': einsum '{einsum.get_subscripts()}' is not an operator gradient of a DG"
                " family at a compiled size (feinsum_amd.family.match_operator_adjoint)")
        return "operator_adjoint"
    if variant == "contraction":
        return "contraction"
    if variant == "reduction":
        check_reduction(einsum, sizes)
        return "reduction"
    plan = match_family(einsum)
    if plan is not None and not (variant in ("generic", 1) and _generic_kernel_is_the_einsum_one(plan)):
        return "family"
    if variant not in (None, "auto", "generic", 0, 1):
        raise NotImplementedError(
            f"einsum '{einsum.get_subscripts()}' is outside the DG kernel families;"
            " only the generic, contraction and reduction kernels are available for it")
    if variant in (None, "auto", 0) and auto_picks_reduction(einsum, sizes):
        return "reduction"
    if variant in (None, "auto", 0) and auto_picks_contraction(einsum, sizes):
        return "contraction"
    return "generic"


def accepts_element_slices(einsum: BatchedEinsum, transform: Any = None, alpha: float = 1.0, beta: float = 0.0) -> bool:
    """Does a launch of *einsum* under *transform* take element slices (``ELEMENT_SLICE_RULE``)?  From the einsum alone:
    no arrays, no device.  The launch kind ``"family"``, a float64 GRAD / DIV / FACEMASS plan of tetrahedra p = 1..4 --
    face-mass with every launch group of two or more fields --, the variant auto or ``"mfma"``, no accumulation."""
    if (float(alpha), float(beta)) != (1.0, 0.0) or (isinstance(transform, Mapping) and "accumulate" in transform):
        return False
    variant = _variant_from_transform(transform)
    if variant not in (None, "auto", "mfma", 0, 2):
        return False
    plan = match_family(einsum)      # (under these variants launch_kind is "family" exactly where a plan exists)
    if plan is None:
        return False
    p = plan.params
    if plan.family not in (FAMILY_GRAD, FAMILY_DIV, FAMILY_FACEMASS) or p.get("f32") or p.get("fields_f32"):
        return False
    if plan.family == FAMILY_FACEMASS:
        return (p.get("nf") == 4 and (p.get("Np"), p.get("Nfp")) in _ACC_FACEMASS_SHAPES
                and min(len(g) for g in _family_groups(plan, einsum)) >= 2)
    return p.get("ndim", 3) == 3 and p.get("Np") in _ACC_EPILOGUE_NP


def _element_axes(einsum: BatchedEinsum) -> Tuple[Dict[str, int], Optional[int]]:
    """Where the element axis is: per argument that may be an element slice, and in the outputs.  Empty / None outside the
    DG families; the operator array has none."""
    plan = match_family(einsum)
    if plan is None:
        return {}, None
    axes: Dict[str, int] = {}
    for row in einsum.args:
        for pos, arg in enumerate(row):
            if plan.long_index in einsum.in_idx_sets[pos]:
                axes[arg.name] = einsum.in_idx_sets[pos].index(plan.long_index)
    out_axis = einsum.out_idx_set.index(plan.long_index) if plan.long_index in einsum.out_idx_set else None
    return axes, out_axis


def _strided_runs(plan: KernelPlan, einsum: BatchedEinsum, arg_dict: Mapping[str, Any], outs: Sequence[Any]) -> list:
    """The launches of a family plan on element slices: ``[(first row of the group, (ldIn, ldOut), rows)]``.  A launch has one
    ldIn and one ldOut, so the fields of a group of ``_family_groups`` are gathered by their pair of leading dimensions, in order
    of first appearance (fields A, B, A, B of two bases become the launches {A, A} and {B, B}; every field's result is the same
    in any grouping).  An entry of *outs* may be None: an output that is yet to be allocated, contiguous.  Face-mass needs two
    fields per launch: a field that is alone with its leading dimensions is refused (``InvalidParameterError``)."""
    role, rows = plan.roles, einsum.args
    in_role = "u" if "D" in role else "v"
    in_axis = einsum.in_idx_sets[role[in_role]].index(plan.long_index)
    out_axis = einsum.out_idx_set.index(plan.long_index)
    ld_of = lambda t, axis: element_slice_ld(tuple(t.shape), tuple(t.stride()), axis)   # noqa: E731
    runs = []
    for group in _family_groups(plan, einsum):
        by_ld: Dict[Tuple[int, int], list] = {}
        for m in group:
            field = arg_dict[rows[m][role[in_role]].name]
            n = int(field.shape[in_axis])
            by_ld.setdefault((ld_of(field, in_axis), n if outs[m] is None else ld_of(outs[m], out_axis)), []).append(m)
        for lds, members in by_ld.items():
            if plan.family == FAMILY_FACEMASS and len(members) < 2 and int(arg_dict[rows[members[0]][role[in_role]].name].shape[in_axis]) > 0:
                raise InvalidParameterError(
                    f"face-mass on element slices: field '{rows[members[0]][role[in_role]].name}' is alone in its launch group with its "
                    f"leading dimensions (ldIn, ldOut) = {lds}, and one field has no matrix-core kernel: slice the fields and outputs of a "
                    f"group out of bases of equal length, at least two of each length, or hand in C-contiguous arrays ({ELEMENT_SLICE_RULE})")
            runs.append((group[0], lds, members))
    return runs


class _MixedStateLaunch:
    """grad, div or face-mass of tetrahedra p = 1..4 with float32 fields AND float32 results in float64 geometry, operator and
    arithmetic (transform ``"mixed_state"``): the named entry points ``fe_grad3d_mixed_state_f64`` /
    ``fe_div3d_mixed_state_f64`` / ``fe_facemass_mixed_state_f64``, one call per group of ``_family_groups``.  No prepared
    operators."""

    fields_f32 = True     # (operator.py: float32 fields, a launch of its own)

    def __init__(self, plan: KernelPlan, einsum: BatchedEinsum, arg_dict: Mapping[str, Any], outs: Sequence[Any]) -> None:
        self.plan = plan
        self._keep = (arg_dict, outs)
        role, rows, p = plan.roles, einsum.args, plan.params
        op_role, in_role = ("D", "u") if "D" in role else ("R", "v")
        self.entry_point = {FAMILY_GRAD: "fe_grad3d_mixed_state_f64", FAMILY_DIV: "fe_div3d_mixed_state_f64",
                            FAMILY_FACEMASS: "fe_facemass_mixed_state_f64"}[plan.family]
        j_axis = einsum.in_idx_sets[role["J"]].index(plan.long_index)
        self.E = int(arg_dict[rows[0][role["J"]].name].shape[j_axis])
        self.calls = []      # (function, arguments in front of the stream)
        for group in _family_groups(plan, einsum):
            first = rows[group[0]]
            J, A = arg_dict[first[role["J"]].name].data_ptr(), arg_dict[first[role[op_role]].name].data_ptr()
            vptrs = [arg_dict[rows[m][role[in_role]].name].data_ptr() for m in group]
            optrs = [outs[m].data_ptr() for m in group]
            if plan.family == FAMILY_GRAD:
                self.calls.append((_hip.grad3d_mixed_state, (J, A, vptrs, optrs, self.E, p["Np"], plan.layout_flags)))
            elif plan.family == FAMILY_DIV:
                self.calls.append((_hip.div3d_mixed_state, (J, A, vptrs, optrs, self.E, p["Np"], plan.layout_flags)))
            else:
                self.calls.append((_hip.facemass_mixed_state, (J, A, vptrs, optrs, self.E, p["Np"], p["nf"], p["Nfp"],
                                                               plan.layout_flags)))

    def launch(self, stream_ptr: int) -> None:
        for fn, args in self.calls:
            fn(*args, stream=stream_ptr)

    def time_batch(self, n: int, stream_ptr: int) -> float:
        return _hip.time_with_events(self.launch, n, stream_ptr)


class _ElementOperatorLaunch:
    """The element-local operator of any shape (transform ``"element_operator"``): the named entry point ``fe_elemop_f64``,
    one call per group of ``family.element_operator_groups``.  No prepared operators; a launch of its own in a bound
    operator (``operator._merge`` fuses ``_FamilyLaunch`` stages only)."""

    entry_point = "fe_elemop_f64"

    def __init__(self, plan: Any, einsum: BatchedEinsum, arg_dict: Mapping[str, Any], outs: Sequence[Any]) -> None:
        self.plan = plan
        self._keep = (arg_dict, outs)
        role, rows, p = plan.roles, einsum.args, plan.params
        u_axis = einsum.in_idx_sets[role["u"]].index(plan.long_index)
        self.E = int(arg_dict[rows[0][role["u"]].name].shape[u_axis])
        self.calls = []      # (arguments of _hip.elemop in front of the stream)
        self.rows = []       # the rows of every call
        for group in element_operator_groups(plan, einsum):
            first = rows[group[0]]
            J = arg_dict[first[role["J"]].name].data_ptr() if "J" in role else None
            A = arg_dict[first[role["A"]].name].data_ptr()
            uptrs = [arg_dict[rows[m][role["u"]].name].data_ptr() for m in group]
            optrs = [outs[m].data_ptr() for m in group]
            self.rows.append(tuple(group))
            self.calls.append((J, A, uptrs, optrs, self.E, p["Ni"], p["Nj"], plan.layout_flags))

    def launch(self, stream_ptr: int) -> None:
        for args in self.calls:
            _hip.elemop(*args, stream=stream_ptr)

    def time_batch(self, n: int, stream_ptr: int) -> float:
        return _hip.time_with_events(self.launch, n, stream_ptr)


class _WeightedElementOperatorLaunch:
    """The weighted element operator ``iq,eq,qj,ej->ei`` (transform ``"weighted_element_operator"``): the named entry point
    ``fe_weightedop_f64``, one call per group of ``family.weighted_element_operator_groups``.  No prepared operators; a
    launch of its own in a bound operator (``operator._merge`` fuses ``_FamilyLaunch`` stages only)."""

    entry_point = "fe_weightedop_f64"

    def __init__(self, plan: Any, einsum: BatchedEinsum, arg_dict: Mapping[str, Any], outs: Sequence[Any]) -> None:
        self.plan = plan
        self._keep = (arg_dict, outs)
        role, rows, p = plan.roles, einsum.args, plan.params
        u_axis = einsum.in_idx_sets[role["u"]].index(plan.long_index)
        self.E = int(arg_dict[rows[0][role["u"]].name].shape[u_axis])
        self.calls = []      # (arguments of _hip.weightedop in front of the stream)
        self.rows = []       # the rows of every call
        for group in weighted_element_operator_groups(plan, einsum):
            first = rows[group[0]]
            P, W, A = (arg_dict[first[role[r]].name].data_ptr() for r in ("P", "W", "A"))
            uptrs = [arg_dict[rows[m][role["u"]].name].data_ptr() for m in group]
            optrs = [outs[m].data_ptr() for m in group]
            self.rows.append(tuple(group))
            self.calls.append((P, W, A, uptrs, optrs, self.E, p["Ni"], p["Nq"], p["Nj"], plan.layout_flags))

    def launch(self, stream_ptr: int) -> None:
        for args in self.calls:
            _hip.weightedop(*args, stream=stream_ptr)

    def time_batch(self, n: int, stream_ptr: int) -> float:
        return _hip.time_with_events(self.launch, n, stream_ptr)


class _WeightGradLaunch:
    """The weight gradient of the weighted element operator, ``iq,qj,ej,ei->eq`` with its rows summed
    (``family.match_weighted_operator_weight_adjoint``): the named entry point ``fe_weightgrad_f64``, one call per at most 8
    rows, call c into ``outs[c]`` -- whoever binds it adds them in that order.  Reached from the backward pass of
    ``evaluate_differentiable(element_gradients="kernel")`` only."""

    entry_point = "fe_weightgrad_f64"

    def __init__(self, plan: Any, einsum: BatchedEinsum, arg_dict: Mapping[str, Any], outs: Sequence[Any]) -> None:
        from feinsum_amd.family import WEIGHTED_WEIGHT_ADJOINT_MAX_FIELDS as per_call

        self.plan = plan
        self._keep = (arg_dict, outs)
        role, rows, p = plan.roles, einsum.args, plan.params
        self.E = int(arg_dict[rows[0][role["u"]].name].shape[0])
        self.rows = [tuple(range(k, min(k + per_call, len(rows)))) for k in range(0, len(rows), per_call)]
        if len(outs) != len(self.rows):
            raise InvalidParameterError(f"the weight gradient of {len(rows)} rows takes {len(self.rows)} calls: one output each")
        P, A = (arg_dict[rows[0][role[r]].name].data_ptr() for r in ("P", "A"))
        self.calls = []      # (arguments of _hip.weightgrad in front of the stream)
        for group, out in zip(self.rows, outs):
            uptrs = [arg_dict[rows[m][role["u"]].name].data_ptr() for m in group]
            gptrs = [arg_dict[rows[m][role["g"]].name].data_ptr() for m in group]
            self.calls.append((P, A, uptrs, gptrs, out.data_ptr(), self.E, p["Ni"], p["Nq"], p["Nj"], plan.layout_flags))
        self.accumulate = None
        self.reads = tuple(sp for name in sorted(einsum.all_args) for sp in _spans(arg_dict[name]))
        self.writes = tuple(_span(t) for t in outs)

    def launch(self, stream_ptr: int) -> None:
        for args in self.calls:
            _hip.weightgrad(*args, stream=stream_ptr)

    def time_batch(self, n: int, stream_ptr: int) -> float:
        return _hip.time_with_events(self.launch, n, stream_ptr)


class _StridedFamilyLaunch:
    """float64 grad, div or face-mass of tetrahedra p = 1..4 with element slices among its arrays: the named entry points
    ``fe_grad3d_strided_f64`` / ``fe_div3d_strided_f64`` / ``fe_facemass_strided_f64``, one launch per group of
    ``_family_groups`` and pair of leading dimensions in it (``_strided_runs``).  No prepared operators."""

    def __init__(self, plan: KernelPlan, einsum: BatchedEinsum, arg_dict: Mapping[str, Any], outs: Sequence[Any]) -> None:
        self.plan = plan
        self._keep = (arg_dict, outs)
        role, rows, p = plan.roles, einsum.args, plan.params
        op_role, in_role = ("D", "u") if "D" in role else ("R", "v")
        self.entry_point = {FAMILY_GRAD: "fe_grad3d_strided_f64", FAMILY_DIV: "fe_div3d_strided_f64",
                            FAMILY_FACEMASS: "fe_facemass_strided_f64"}[plan.family]
        j_axis = einsum.in_idx_sets[role["J"]].index(plan.long_index)
        self.E = int(arg_dict[rows[0][role["J"]].name].shape[j_axis])
        self.calls = []      # (function, arguments in front of the stream)
        self.rows = []       # the rows of every call
        for first, (ld_in, ld_out), members in _strided_runs(plan, einsum, arg_dict, outs):
            J, A = arg_dict[rows[first][role["J"]].name], arg_dict[rows[first][role[op_role]].name]
            ldJ = element_slice_ld(tuple(J.shape), tuple(J.stride()), j_axis)
            vptrs = [arg_dict[rows[m][role[in_role]].name].data_ptr() for m in members]
            optrs = [outs[m].data_ptr() for m in members]
            self.rows.append(tuple(members))
            if plan.family == FAMILY_GRAD:
                self.calls.append((_hip.grad3d_strided, (J.data_ptr(), ldJ, A.data_ptr(), vptrs, optrs, ld_out, self.E,
                                                         p["Np"], plan.layout_flags)))
            elif plan.family == FAMILY_DIV:
                self.calls.append((_hip.div3d_strided, (J.data_ptr(), ldJ, A.data_ptr(), vptrs, ld_in, optrs, self.E,
                                                        p["Np"], plan.layout_flags)))
            else:
                self.calls.append((_hip.facemass_strided, (J.data_ptr(), ldJ, A.data_ptr(), vptrs, ld_in, optrs, self.E,
                                                           p["Np"], p["nf"], p["Nfp"], plan.layout_flags)))

    def launch(self, stream_ptr: int) -> None:
        for fn, args in self.calls:
            fn(*args, stream=stream_ptr)

    def time_batch(self, n: int, stream_ptr: int) -> float:
        return _hip.time_with_events(self.launch, n, stream_ptr)


ACCUMULATE_ROUTES = ("kernel", "axpby", "epilogue")
#: (Np, Nfp) of the tetrahedral orders p = 1..4: the shapes fe_facemass_acc_f64 is compiled for
_ACC_FACEMASS_SHAPES = frozenset({(4, 3), (10, 6), (20, 10), (35, 15)})
#: Np of the same orders: the shapes fe_grad3d_acc_f64 and fe_div3d_acc_f64 are compiled for
_ACC_EPILOGUE_NP = frozenset(np_ for np_, _ in _ACC_FACEMASS_SHAPES)


def _check_scale(alpha: Any, beta: Any) -> Tuple[float, float]:
    try:
        alpha, beta = float(alpha), float(beta)
    except (TypeError, ValueError):
        raise InvalidParameterError(f"alpha and beta must be numbers (got {alpha!r}, {beta!r})") from None
    if not (np.isfinite(alpha) and np.isfinite(beta)):
        raise InvalidParameterError(f"alpha and beta must be finite (got {alpha}, {beta})")
    return alpha, beta


def accumulate_route(einsum: BatchedEinsum, transform: Any = None) -> str:
    """
    Which way an accumulating evaluation of *einsum* (``evaluate(..., alpha=, beta=)`` other than (1, 0)) takes under
    *transform*, from the einsum alone (no device): ``"kernel"`` -- the accumulating face-mass kernel
    (``fe_facemass_acc_f64``): float64 face-mass of tetrahedra p = 1..4, every launch group of two or more fields, the
    variant ``"auto"`` or ``"mfma"`` -- or ``"axpby"``: the einsum's ordinary launch into a temporary, then ``fe_axpby``.
    ``transform={"accumulate": "axpby"}`` forces the second; ``{"accumulate": "kernel"}`` insists on the first
    (``NotImplementedError`` where it does not exist).

    A third route is opt-in and never chosen by default: ``{"accumulate": "epilogue"}`` returns ``"epilogue"`` -- the
    accumulating grad / div kernels (``fe_grad3d_acc_f64`` / ``fe_div3d_acc_f64``, one launch per field), which read the old
    output where they store the new one -- for float64 grad and div of tetrahedra p = 1..4, either operator layout, the
    variant ``"auto"`` or ``"mfma"``; ``NotImplementedError`` for everything else (face-mass accumulates through
    ``"kernel"``).

    The contraction and the split reduction accumulate inside their kernels on request, never by default:
    ``{"variant": "contraction", "accumulate": "kernel"}`` returns ``"kernel"`` for an einsum of two or more float32 /
    float64 operands (``fe_einsum_contract_acc``: the store epilogue of the step that writes the output), and
    ``{"variant": "reduction", "accumulate": "kernel"}`` for float32 / float64 operands (``fe_einsum_reduce_acc``: the
    launch that sums the partials).  Without a forced route both variants stay ``"axpby"``, and ``"epilogue"`` stays
    ``NotImplementedError`` for them.  One check is left to bind time, because it needs the schedule and the sizes, which
    this function does not see: the step that writes the output must run on the contraction or the split-reduction
    kernel; a last step on the generic kernel (a caller's schedule whose last step has one input, a ``"generic"`` last
    step of ``reduction.plan_reduction``) is ``NotImplementedError`` naming the step, before anything is allocated or
    launched.
    """
    forced = transform.get("accumulate") if isinstance(transform, Mapping) else None
    if forced is not None and forced not in ACCUMULATE_ROUTES:
        raise InvalidParameterError(f"accumulate must be one of {ACCUMULATE_ROUTES}, got {forced!r}")
    variant = _variant_from_transform(transform)
    plan = match_family(einsum) if variant in (None, "auto", "mfma", 0, 2) else None
    fused = (plan is not None and plan.family == FAMILY_FACEMASS and not plan.params.get("f32")
             and plan.params.get("nf") == 4 and (plan.params.get("Np"), plan.params.get("Nfp")) in _ACC_FACEMASS_SHAPES
             and min(len(g) for g in _family_groups(plan, einsum)) >= 2)
    if forced == "epilogue":
        if (plan is not None and plan.family in (FAMILY_GRAD, FAMILY_DIV) and not plan.params.get("f32")
                and plan.params.get("ndim", 3) == 3 and plan.params.get("Np") in _ACC_EPILOGUE_NP):
            return "epilogue"
        hint = ('; face-mass accumulates inside its kernel through {"accumulate": "kernel"}'
                if plan is not None and plan.family == FAMILY_FACEMASS else "")
        raise NotImplementedError(
            f"einsum '{einsum.get_subscripts()}' x {einsum.b} has no accumulating epilogue under this transform (float64"
            f" grad or div of tetrahedra p = 1..4, variant auto or mfma){hint}")
    if forced == "kernel" and variant in ("contraction", "reduction"):
        real = all(np.dtype(d) in (np.dtype("float64"), np.dtype("float32")) for d in einsum.arg_to_dtype.values())
        if real and (variant == "reduction" or einsum.n >= 2):
            return "kernel"
        raise NotImplementedError(
            f"einsum '{einsum.get_subscripts()}' x {einsum.b} has no accumulating kernel under the transform '{variant}'"
            " (float32 / float64 operands" + ("" if variant == "reduction" else ", two or more of them") + ")")
    if forced == "kernel" and not fused:
        raise NotImplementedError(
            f"einsum '{einsum.get_subscripts()}' x {einsum.b} has no accumulating kernel under this transform (float64"
            " face-mass of tetrahedra p = 1..4, two or more fields per launch, variant auto or mfma)")
    return "kernel" if fused and forced != "axpby" else "axpby"


class _AxpbyLaunch:
    """The fallback route of an accumulating evaluation: *inner* evaluates into *temps* (one per output, allocated at bind
    time on the queue's stream, so that the bound launch can be captured and replayed), then ``fe_axpby`` combines each
    with its output on the same stream."""

    def __init__(self, inner: Any, temps: Sequence[Any], outs: Sequence[Any], alpha: float, beta: float) -> None:
        import torch

        self.inner, self.temps, self.scale = inner, tuple(temps), (alpha, beta)
        self._keep = tuple(outs)
        self.passes = [(o.data_ptr(), t.data_ptr(), int(o.numel()), o.dtype == torch.float64) for o, t in zip(outs, temps)]

    def launch(self, stream_ptr: int) -> None:
        self.inner.launch(stream_ptr)
        for out, tmp, n, f64 in self.passes:
            _hip.axpby(out, tmp, n, self.scale[0], self.scale[1], f64, stream_ptr)

    def time_batch(self, n: int, stream_ptr: int) -> float:
        return _hip.time_with_events(self.launch, n, stream_ptr)


def _bind(einsum: BatchedEinsum, cq: Any, arg_dict: Mapping[str, Any],
          out_dict: Optional[Mapping[str, Any]], transform: Any, prepare: bool = False,
          schedule: Optional[ContractionSchedule] = None, alpha: float = 1.0, beta: float = 0.0):
    import torch

    q = _as_queue(cq)
    missing = sorted(set(einsum.all_args) - set(arg_dict))
    if missing:
        raise InvalidParameterError(f"missing input arrays: {missing}")
    sizes = _long_length(einsum, arg_dict)
    in_axes, out_axis = _element_axes(einsum)
    sliced = []      # arguments that are element slices and not contiguous
    for name, shape in einsum.arg_to_shape.items():
        concrete = tuple(sizes[d.name] if isinstance(d, SizeParam) else int(d) for d in shape)
        if _check_tensor(name, arg_dict[name], concrete, einsum.arg_to_dtype[name], q, in_axes.get(name)):
            sliced.append(name)
    out_shape = tuple(sizes[d.name] if isinstance(d, SizeParam) else int(d) for d in einsum.shape)
    given = {name: out_dict[name] for name in einsum.output_names if out_dict is not None and name in out_dict}
    for k, name in enumerate(einsum.output_names):
        if name in given:
            if _check_tensor(name, given[name], out_shape, result_dtype(einsum, k, transform), q, out_axis):
                sliced.append(name)
    _refuse_aliased_outputs(einsum, arg_dict, given)     # before anything is allocated, prepared or launched
    alpha, beta = _check_scale(alpha, beta)
    if _variant_from_transform(transform) in ("element_operator", "weighted_element_operator"):
        launch_kind(einsum, transform, sizes)            # (likewise: the size rule refuses before anything is allocated)
    if sliced:                                           # (likewise: which launches take slices, and how their fields group)
        if not accepts_element_slices(einsum, transform, alpha, beta):
            raise InvalidParameterError(f"argument '{sliced[0]}' must be C-contiguous for this launch: {ELEMENT_SLICE_RULE}")
        _strided_runs(match_family(einsum), einsum, arg_dict, [given.get(name) for name in einsum.output_names])
    route = None if (alpha, beta) == (1.0, 0.0) else accumulate_route(einsum, transform)
    if beta != 0.0 and len(given) != len(einsum.output_names):
        raise InvalidParameterError(
            f"beta = {beta} adds onto the outputs: every one of them must be handed in through out_dict (missing: "
            f"{sorted(set(einsum.output_names) - set(given))})")
    outs = []
    allocated: dict = {}      # outputs this call allocated itself: name -> "split" | "torch" | "torch (<why>)"
    owned = []                # ... and the arrays: they belong to the queue's stream (DeviceQueue)
    with _on_stream_of(q):
        for k, name in enumerate(einsum.output_names):
            dt = result_dtype(einsum, k, transform)
            if name in given:
                outs.append(given[name])
            else:
                tensor, how = _allocate_output(out_shape, getattr(torch, dt.name), q.torch_device, transform)
                outs.append(tensor)
                owned.append(tensor)
                allocated[name] = how
        final_outs = outs
        if route == "axpby":    # the launch writes temporaries of the queue's stream; fe_axpby combines them with the outputs
            outs = [torch.empty_like(t) for t in final_outs]
            owned.extend(outs)
    kind = launch_kind(einsum, transform, sizes)
    if kind == "contraction":
        bound = ContractionLaunch(einsum, arg_dict, outs, sizes, schedule, stream=q.stream,
                                  scale=(alpha, beta) if route == "kernel" else None)
    elif kind == "reduction":
        bound = ReductionLaunch(einsum, arg_dict, outs, sizes, schedule, stream=q.stream,
                                scale=(alpha, beta) if route == "kernel" else None)
    elif kind == "adjoint":
        bound = AdjointLaunch(match_adjoint_family(einsum), einsum, arg_dict, outs)
    elif kind == "operator_adjoint":
        with torch.cuda.device(q.torch_device):
            bound = AdjointLaunch(match_operator_adjoint(einsum), einsum, arg_dict, outs, stream=q.stream)
    elif kind == "mixed_family":     # (accumulation: the "axpby" route -- accumulate_route knows no other for it)
        bound = _FamilyLaunch(match_mixed_family(einsum), einsum, arg_dict, outs, None)
    elif kind == "mixed_state":      # (float32 outputs: result_dtype; accumulation by "axpby" with float32 temporaries)
        bound = _MixedStateLaunch(match_mixed_family(einsum), einsum, arg_dict, outs)
    elif kind == "element_operator":  # (accumulation: the "axpby" route only)
        bound = _ElementOperatorLaunch(match_element_operator(einsum), einsum, arg_dict, outs)
    elif kind == "weighted_element_operator":  # (likewise)
        bound = _WeightedElementOperatorLaunch(match_weighted_element_operator(einsum), einsum, arg_dict, outs)
    elif kind == "family" and sliced:
        bound = _StridedFamilyLaunch(match_family(einsum), einsum, arg_dict, outs)
    elif kind == "family":
        bound = _FamilyLaunch(match_family(einsum), einsum, arg_dict, outs, _variant_from_transform(transform),
                              scale=(alpha, beta) if route in ("kernel", "epilogue") else None)
        if route not in ("kernel", "epilogue") and _prepared_from_transform(transform, prepare):
            with torch.cuda.device(q.torch_device), _on_stream_of(q):
                bound.prepare_operators(q.stream_ptr)
    else:
        bound = _GenericLaunch(einsum, arg_dict, outs)
    if route == "axpby":
        bound, temps, outs = _AxpbyLaunch(bound, outs, final_outs, alpha, beta), outs, final_outs
    #: None (the outputs are overwritten), or which way the launch adds onto them: "kernel" | "axpby" | "epilogue" (accumulate_route)
    bound.accumulate = route
    # byte ranges the launch reads and writes (operator.py checks them before reordering launches)
    bound.reads = (tuple(sp for name in sorted(einsum.all_args) for sp in _spans(arg_dict[name]))
                   + (tuple(sp for t in outs for sp in _spans(t)) if beta != 0.0 else ()))
    bound.writes = tuple(sp for t in outs for sp in _spans(t)) + (tuple(_span(t) for t in temps) if route == "axpby" else ())
    bound.output_allocations = MappingProxyType(allocated)
    bound.owned_arrays, bound.owned_stream_ptr = tuple(owned), q.stream_ptr   # (operator.py: launches on another stream mark them)
    return q, bound, outs


def _allocate_output(shape: Tuple[int, ...], dtype: Any, device: Any, transform: Any):
    """
    An output array the caller did not supply (the reference allocates them through its PyOpenCL pool,
    ``src/feinsum/measure.py:44-60,236-246``).  Arrays of 8 MiB and more come from the split allocator
    (``placement.empty``: on MI355X a launch writing into its arrays runs 5-12 % faster than into ordinary allocations,
    DESIGN.md section 3d) unless ``transform={"placement": "separate"}`` / ``$FEINSUM_PLACEMENT=separate`` asks for plain
    ones; whatever the allocator cannot serve (no VMM support, address-space cap, out of memory in its pool) is a plain
    ``torch.empty``.  Returns ``(tensor, how)``.
    """
    import torch

    from feinsum_amd import placement

    nbytes = int(np.prod(shape, dtype=np.int64)) * torch.empty((), dtype=dtype).element_size() if shape else 0
    if torch.device(device).type != "cuda" or nbytes < placement.SPLIT_MIN_BYTES:
        return torch.empty(shape, dtype=dtype, device=device), "torch"
    if _placement_mode(transform) != "split":
        return torch.empty(shape, dtype=dtype, device=device), "torch (placement: separate)"
    if torch.cuda.is_current_stream_capturing():
        # the allocator creates handles, probes with kernels of its own and may synchronise the device: none of that may
        # happen inside a stream capture -- torch's allocator knows how to allocate for a graph
        return torch.empty(shape, dtype=dtype, device=device), "torch (stream capture in progress)"
    try:
        t = placement.empty(shape, dtype, device)
        # (the allocator refuses an array that would be of one class of physical memory: placement.empty then allocates ordinarily)
        return t, "split" if placement.is_split(t) else "torch (the split allocator found no second class of physical memory)"
    except (RuntimeError, HipLibraryError) as exc:
        logger.warning("split allocator not available (%s); the output is an ordinary allocation", str(exc)[:160])
        return torch.empty(shape, dtype=dtype, device=device), f"torch (split allocator failed: {str(exc)[:120]})"


def evaluate(einsum: BatchedEinsum, cq: Any, arg_dict: Mapping[str, Any], *,
             out_dict: Optional[Mapping[str, Any]] = None, transform: Any = None,
             wait: bool = False, schedule: Optional[ContractionSchedule] = None,
             alpha: float = 1.0, beta: float = 0.0) -> Mapping[str, Any]:
    """
    Enqueue *einsum* on the queue's stream and return ``{"_fe_out": tensor, ...}``
    (the replacement for ``t_unit.executor(cq, ...)(cq, **arg_dict)``,
    reference measure.py:163-165).  Asynchronous unless *wait*; outputs are
    fully overwritten.  *schedule*: see the module docstring.

    Accumulating: with *alpha*, *beta* (Python floats, finite) other than (1, 0) every output row k becomes
    ``out_k <- alpha * E_k + beta * out_k``, ``E_k`` being what the call computes otherwise (``C <- alpha A B + beta C`` of
    BLAS; a time stepper's ``k <- a k + dt rhs``).  ``beta != 0`` needs every output in *out_dict*
    (``InvalidParameterError``, like the aliasing rule below and in the same place); ``beta == 0`` does not read the
    outputs: NaN or infinity sitting in them does not reach the result.  Float32 outputs get alpha and beta cast to
    float32.  Rounding: ``E_k`` is bitwise what the non-accumulating launch of the same kernel produces; the combine,
    ``fma(alpha, E_k, beta * out_k)``, adds at most two roundings per entry; with alpha and beta signed powers of two both
    products are exact and the result is bitwise ``fl(alpha E_k + beta out_k)``.  It works under every transform, one of
    two ways (:func:`accumulate_route`; the bound launch says which in ``bound.accumulate``): the accumulating face-mass
    kernel, which reads the old output where it stores the new one, or the ordinary launch into a temporary (allocated at
    bind time on the queue's stream) followed by ``fe_axpby`` on the same stream.  ``transform={"accumulate": "epilogue"}``
    opts grad and div of tetrahedra p = 1..4 into kernels that accumulate the same way as the face-mass one, and
    ``{"variant": "contraction" | "reduction", "accumulate": "kernel"}`` the contraction and the split reduction (no temporary;
    the step that writes the output must run on one of these two kernels, else ``NotImplementedError`` at bind).  (1, 0), the
    default, is the code path without any of this.  DESIGN.md section 3m.

    Aliasing: an output handed in through *out_dict* may not share a byte with any input, nor with another output
    (``InvalidParameterError``, raised before anything is allocated, prepared or launched, under every transform): the
    kernels read their operands while other threads already store results, so an in-place step needs a second
    array.  Arrays of no bytes overlap nothing, views that merely touch are fine, and inputs may overlap inputs.

    Stream order: the outputs this call allocates (those not in *out_dict*) and everything else it allocates belong to
    the queue's stream (:class:`DeviceQueue`), which need not be the current stream: they may be dropped at once, and
    whoever gets their memory next -- on any stream -- is ordered behind this launch without a host synchronisation.
    To READ them on another stream, order that stream behind the queue's and, as with any torch tensor,
    ``placement.record_stream(out, that_stream)`` before dropping them.  The arrays the caller allocates (*arg_dict*,
    *out_dict*) are the caller's to order against the queue's stream.
    """
    import torch

    q, bound, outs = _bind(einsum, cq, arg_dict, out_dict, transform, schedule=schedule, alpha=alpha, beta=beta)
    with torch.cuda.device(q.torch_device):
        bound.launch(q.stream_ptr)
    if wait:
        q.finish()
    return MappingProxyType(dict(zip(einsum.output_names, outs)))


# --------------------------------------------------------------------------
# validation and timing
# --------------------------------------------------------------------------

def _tolerances(dtype: np.dtype) -> Tuple[float, float]:
    real = get_real_dtype(np.dtype(dtype))
    if real == np.float32:
        return 1e-6, 1e-6
    if real == np.float64:
        return 1e-10, 1e-10
    raise NotImplementedError(real)


def validation_dtype(einsum: BatchedEinsum, row: int = 0) -> np.dtype:
    """The dtype whose tolerances validate output *row*: its ``result_dtype``, except that a float64 output of three or
    more operands of which two or more are float32 is validated as float32.  There a schedule step can meet float32
    operands only, and such a step rounds to float32 -- in ``np.einsum(optimize="optimal")``, the reference's own
    yardstick, and in a float32 intermediate of the "contraction" transform alike."""
    dt = result_dtype(einsum, row)
    n_f32 = sum(np.dtype(a.dtype) == np.dtype("float32") for a in einsum.args[row])
    if dt == np.dtype("float64") and len(einsum.args[row]) >= 3 and n_f32 >= 2:
        return np.dtype("float32")
    return dt


def validate_batched_einsum_transform(einsum: BatchedEinsum, cq: Any, transform: Any,
                                      schedule: Optional[ContractionSchedule] = None) -> None:
    """
    Run the selected kernel at ``long_dim_length = 100`` and compare every output
    with ``np.einsum(subscripts, *inputs, optimize="optimal")``; atol = rtol =
    1e-10 (float64) / 1e-6 (float32; :func:`validation_dtype` picks which).  Raises
    :class:`~feinsum_amd.diagnostics.TransformValidationError` on mismatch.
    (reference: measure.py:111-194)
    """
    long_dim_length = 100
    q = _as_queue(cq)
    host = generate_host_input_arrays(einsum, long_dim_length)
    import torch

    arg_dict = {name: torch.from_numpy(arr).to(q.torch_device) for name, arr in host.items()}
    ref_outs = {name: np.einsum(einsum.get_subscripts(), *[host[arg.name] for arg in row],
                                optimize="optimal")
                for name, row in zip(einsum.output_names, einsum.args)}
    outs = evaluate(einsum, q, arg_dict, transform=transform, wait=True, schedule=schedule)
    state = _variant_from_transform(transform) == "mixed_state"     # float32 results: the reference rounded likewise
    if state:
        ref_outs = {name: ref.astype(np.float32) for name, ref in ref_outs.items()}
    if set(ref_outs) != set(outs):
        raise RuntimeError("Output names mismatch")
    rows = dict(zip(einsum.output_names, range(len(einsum.args))))
    for name in sorted(ref_outs):
        got = outs[name].cpu().numpy()
        ref = ref_outs[name]
        if got.dtype != ref.dtype:
            raise RuntimeError(f"dtype mismatch for output '{name}'")
        atol, rtol = _tolerances(np.dtype("float32") if state else validation_dtype(einsum, rows[name]))
        try:
            np.testing.assert_allclose(got, ref, atol=atol, rtol=rtol)
        except AssertionError as exc:
            raise TransformValidationError(f"{exc}") from exc
    logger.info("Statistically verified the soundness of the transformation")


PLACEMENT_MODES = ("split", "separate")


def _placement_mode(transform: Any) -> str:
    """
    Where ``timeit`` puts the arrays it allocates: ``transform={"placement": ...}``, else ``$FEINSUM_PLACEMENT``, else
    ``"split"``.

    ``"split"``     one allocation per array, as the reference does (``src/feinsum/measure.py:44-60,80-108``); the
                    OUTPUTS come from the split allocator (``feinsum_amd.placement.zeros``), whose arrays alternate
                    between two classes of physical memory every 4 MiB -- no arena, no scan, memory = the footprint.
                    ``evaluate`` allocates the outputs it is not handed the same way, and a caller gets such arrays
                    with ``placement.empty``.
    ``"separate"``  every array from the torch allocator: the reference's protocol to the letter, and what a caller
                    who allocates with ``torch.empty`` gets.
    The :class:`TimingResult` says which one was used (``record_facts`` stores it with the fact).
    """
    import os

    mode = transform.get("placement") if isinstance(transform, Mapping) else None
    mode = mode or os.environ.get("FEINSUM_PLACEMENT") or "split"
    if mode == "auto":          # round 2's default name
        mode = "split"
    if mode not in PLACEMENT_MODES:
        raise InvalidParameterError(f"placement must be one of {PLACEMENT_MODES}, got {mode!r}")
    return mode


@dataclass(frozen=True)
class TimingResult:
    """What :func:`timeit_details` measured (seconds are per launch)."""

    seconds_device: float     # HIP-event time per launch (what timeit returns)
    seconds_wall: float       # host wall-clock per launch, reference protocol
    rounds: int
    #: how the timed arrays were placed: {"mode": "split", "outputs": the allocator's report per output} (one allocation
    #: per array, outputs from the split allocator) or {"mode": "separate"} (every array from torch); a placement that
    #: could not be had says so under "fallback"
    placement: Mapping[str, Any] = field(default_factory=lambda: MappingProxyType({"mode": "separate"}))


def timeit_details(einsum: BatchedEinsum, *, transform: Any = None, cq: Any = None,
                   long_dim_length: int = 100000,
                   schedule: Optional[ContractionSchedule] = None,
                   min_rounds: int = N_MIN_TIMING_ROUNDS,
                   min_secs: float = N_MIN_SIM_SECS, validate: bool = True) -> TimingResult:
    """The reference's timing protocol (measure.py:248-275) with both clocks reported."""
    import torch

    q = _as_queue(cq)
    if validate:
        validate_batched_einsum_transform(einsum, q, transform, schedule)
    arg_dict = generate_input_arrays(q, einsum, long_dim_length)
    mode = _placement_mode(transform)
    report: Mapping[str, Any] = {"mode": "separate"}
    if mode == "split":
        from feinsum_amd import placement

        try:
            with torch.cuda.device(q.torch_device):
                out_dict = generate_out_arrays(q, einsum, long_dim_length, split=True, transform=transform)
            infos = {n: placement.split_info(t) for n, t in out_dict.items()}
            report = {"mode": "split", "outputs": {n: ({"pieces_by_class": i["pieces_by_class"], "first_pieces": i["first_pieces"]} if i
                                                      else "torch allocation (below 8 MiB, or no second class of physical memory found)") for n, i in infos.items()},
                      "alloc_ms": round(sum(i.get("alloc_ms", 0.0) for i in infos.values()), 3)}
        except (RuntimeError, HipLibraryError) as exc:     # the allocator could not serve: the reference's protocol, and say so
            logger.warning("split allocator not available (%s); timing torch allocations", str(exc)[:160])
            out_dict = generate_out_arrays(q, einsum, long_dim_length, transform=transform)
            report = {"mode": "separate", "fallback": f"split allocator failed: {str(exc)[:160]}"}
    else:
        out_dict = generate_out_arrays(q, einsum, long_dim_length, transform=transform)
    # `transform={"prepared": True}`: the operator matrices are written once in fragment layout (see
    # _FamilyLaunch.prepare_operators) instead of being rebuilt by every launch
    prepare = _prepared_from_transform(transform, False)
    _, bound, _ = _bind(einsum, q, arg_dict, out_dict, transform, prepare=prepare, schedule=schedule)
    with torch.cuda.device(q.torch_device):
        for _ in range(N_WARMUP_ROUNDS):
            bound.launch(q.stream_ptr)
        q.finish()
        dev_time = wall_time = 0.0
        rounds = 0
        while rounds < min_rounds or wall_time < min_secs:
            t0 = time()
            dev_time += bound.time_batch(LAUNCHES_PER_BATCH, q.stream_ptr)   # fences like evt.wait()
            wall_time += time() - t0
            rounds += LAUNCHES_PER_BATCH
    return TimingResult(dev_time / rounds, wall_time / rounds, rounds, MappingProxyType(dict(report)))


def timeit(einsum: BatchedEinsum, *, transform: Any = None, cq: Any = None,
           long_dim_length: int = 100000,
           schedule: Optional[ContractionSchedule] = None) -> float:
    """
    Mean seconds per launch of *einsum* on the device of *cq*: validation at
    E = 100, 5 warm-up launches, then batches of 5 launches until at least 10
    launches and 2 s have elapsed (reference: measure.py:197-275).  Device time
    is taken with HIP events around each batch.
    """
    return timeit_details(einsum, transform=transform, cq=cq, long_dim_length=long_dim_length,
                          schedule=schedule).seconds_device


# --------------------------------------------------------------------------
# op counts, footprint, roofline
# --------------------------------------------------------------------------

def _get_giga_ops_from_einsum(expr: BatchedEinsum, long_dim_length: int) -> Mapping[np.dtype, float]:
    """GOps of the optimal schedule by result dtype (reference: measure.py:278-331).

    Complex arithmetic is weighted as in the reference (add = 2, mul = 6 real ops).
    """
    dt = np.result_type(*[np.dtype(d) for d in expr.arg_to_dtype.values()])
    ops = count_ops(expr, long_dim_length=long_dim_length)
    if dt.kind == "c":
        # count_ops returns adds + muls; split them to apply the weights
        from feinsum_amd.contraction_schedule import (_dim_lengths, _step_ops,
                                                      get_opt_einsum_contraction_schedule)
        dims = _dim_lengths(expr, long_dim_length)
        total = 0
        for subs in get_opt_einsum_contraction_schedule(expr).subscripts:
            lhs, rhs = subs.replace(" ", "").split("->")
            sets = [frozenset(s) for s in lhs.split(",")]
            pts = 1
            for idx in frozenset().union(*sets):
                pts *= dims[idx]
            both = _step_ops(sets, frozenset(rhs), dims)
            mults = (len(sets) - 1) * pts
            total += 6 * mults + 2 * (both - mults)
        ops = total * expr.b
        dt = get_real_dtype(dt)
    return MappingProxyType({np.dtype(dt): ops * 1e-9})


def _get_footprint_gbytes(expr: BatchedEinsum, long_dim_length: int) -> float:
    """Every distinct input once + every output once (reference: measure.py:334-354)."""
    nbytes = 0
    for name, shape in expr.arg_to_shape.items():
        nbytes += int(np.prod(_concrete_shape(shape, long_dim_length), dtype=np.int64)) \
            * np.dtype(expr.arg_to_dtype[name]).itemsize
    out_entries = int(np.prod(_concrete_shape(expr.shape, long_dim_length), dtype=np.int64))
    for k in range(expr.b):
        nbytes += out_entries * result_dtype(expr, k).itemsize
    return nbytes * 1e-9


def measure_giga_op_rate(expr: BatchedEinsum, *, transform: Any = None, cq: Any = None,
                         long_dim_length: int = 100000,
                         schedule: Optional[ContractionSchedule] = None) -> Mapping[np.dtype, float]:
    """GOps/s by result dtype (reference: measure.py:357-385)."""
    runtime = timeit(expr, transform=transform, cq=cq, long_dim_length=long_dim_length,
                     schedule=schedule)
    return MappingProxyType({dt: gops / runtime
                             for dt, gops in _get_giga_ops_from_einsum(expr, long_dim_length).items()})


def get_roofline_flop_rate(expr: BatchedEinsum, dev_name: str,
                           long_dim_length: int = 100_000) -> Mapping[np.dtype, float]:
    """
    ``t_roof = max(GOps / peak_GOps[dtype], GB / peak_BW)``; returns GOps / t_roof
    per dtype (reference: measure.py:388-418).  Unknown device ->
    :class:`NoDevicePeaksInfoError`.
    """
    from feinsum_amd.device_info import DEV_TO_PEAK_BW, DEV_TO_PEAK_GFLOPS, normalize_device_name

    dev_name = normalize_device_name(dev_name)
    gops = _get_giga_ops_from_einsum(expr, long_dim_length)
    ngbs = _get_footprint_gbytes(expr, long_dim_length)
    try:
        t_flops = max(g / DEV_TO_PEAK_GFLOPS[dev_name][dt.name] for dt, g in gops.items())
        t_bw = ngbs / DEV_TO_PEAK_BW[dev_name]
    except KeyError as exc:
        raise NoDevicePeaksInfoError(dev_name) from exc
    t_roof = max(t_flops, t_bw)
    return MappingProxyType({dt: g / t_roof for dt, g in gops.items()})


def _strify_measured_vs_roofline(measured: Mapping[np.dtype, Any],
                                 roofline: Mapping[np.dtype, Any]) -> str:
    from tabulate import tabulate

    assert set(measured) == set(roofline)
    fmt = lambda v: f"{v:.1f}" if isinstance(v, float) else str(v)  # noqa: E731
    table = [["Dtype", "Measured GOps/s", "Roofline GOps/s"]]
    for dt in sorted(measured, key=lambda d: d.itemsize):
        table.append([dt.name, fmt(measured[dt]), fmt(roofline[dt])])
    return tabulate(table, tablefmt="fancy_grid")


def stringify_comparison_vs_roofline(expr: BatchedEinsum, *,
                                     schedule: Optional[ContractionSchedule] = None,
                                     transform: Any = None, cq: Any = None,
                                     long_dim_length: int = 100000,
                                     ignore_unknown_device: bool = True) -> str:
    """The reference's fancy_grid table "Dtype / Measured GOps/s / Roofline GOps/s"
    (reference: measure.py:484-525); roofline at the SAME long_dim_length."""
    q = _as_queue(cq)
    measured = measure_giga_op_rate(expr, transform=transform, schedule=schedule, cq=q,
                                    long_dim_length=long_dim_length)
    try:
        roofline: Mapping[np.dtype, Any] = get_roofline_flop_rate(expr, q.device.name, long_dim_length)
    except NoDevicePeaksInfoError:
        if not ignore_unknown_device:
            raise
        roofline = dict.fromkeys(measured, "N/A")
    return _strify_measured_vs_roofline(measured, roofline)
