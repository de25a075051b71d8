"""
The ``"reduction"`` transform: einsums that sum a long summation space into a small output -- inner products and
norms (``ei,ei->``), per-mode sums (``ej,ej->j``), Gram matrices (``ei,ej->ij``), weighted energies
(``e,ij,ei,ej->``) -- evaluated as split reductions (``fe_einsum_reduce``, ``csrc/fe_reduce.h``).

The generic kernel walks the whole summation space of an output entry with one lane group, and the contraction
kernel one 64 x 64 tile with one block, so such an einsum used to run on one wave or one block of the chip.  A split
reduction cuts the summation space into S slices, writes one partial output per slice into a workspace and sums the
partials of every output entry in a fixed order: bitwise reproducible, whatever the stream, the graph or the timing.
Two paths (``_hip.einsum_reduce_plan``): the contraction kernel split along k (two operands the contraction kernel
takes, few tiles) and a VALU kernel over the flattened summation space (everything else).

``"auto"`` (outside the DG families) takes this transform for an einsum whose launch meets :func:`split_path`: shape
only, never the device or a knob.  An einsum of three or more operands is one split launch while its trivial loop
nest only streams its operands (:data:`REDUCE_STREAM_FACTOR`); otherwise it follows its contraction schedule, the
caller's or the optimal one, and every step that sums a long space into a small output is a split launch.
"""

from __future__ import annotations

from typing import Any, Dict, List, Mapping, Optional, Sequence, Tuple

import numpy as np

from feinsum_amd import _hip
from feinsum_amd.contraction import (AUTO_MIN_K, AUTO_MIN_M, AUTO_MIN_MN, AUTO_MIN_N, Step, _contract_acc_call, _desc,
                                     _extents, _split, contraction_sizes, intermediate_shapes, plan_step_dtypes,
                                     plan_steps)
from feinsum_amd.contraction_schedule import ContractionSchedule
from feinsum_amd.einsum import BatchedEinsum

#: at most this many output entries per row (``fe_einsum_reduce``'s limit; ``"reduction"`` above it is
#: ``NotImplementedError``)
REDUCE_MAX_OUT = 4096
#: ``"auto"`` splits a launch whose summation space has at least this many points (K for the matrix-core path)
REDUCE_MIN_SUM = 65536
#: the matrix-core path: fewer than this many (batch x m tile x n tile) work units of 64 x 64
REDUCE_MAX_TILES = 256
#: an einsum of three or more operands is ONE split launch when its summation points are at most this many times
#: the elements of its largest operand (``e,ei,ei->``); otherwise it follows its schedule (``e,ij,ei,ej->``)
REDUCE_STREAM_FACTOR = 4

_TILE = 64
_REAL = (np.dtype("float64"), np.dtype("float32"))


def reduction_sizes(subscripts: str, extent: Mapping[str, int]) -> Tuple[int, int]:
    """``(output entries, summation points)`` of one launch *subscripts*."""
    ins, out = _split(subscripts)
    sums = [c for c in dict.fromkeys("".join(ins)) if c not in out]
    prod = lambda idxs: int(np.prod([extent[i] for i in idxs], dtype=np.int64))   # noqa: E731
    return prod(out), prod(sums)


def _mfma_fits(subscripts: str, extent: Mapping[str, int]) -> Tuple[bool, int]:
    """Whether the contraction kernel takes the two-operand launch (the ``AUTO_MIN_*`` sizes) with fewer than
    REDUCE_MAX_TILES tiles, and its K."""
    b, M, N, K = contraction_sizes(subscripts, extent)
    tiles = b * -(-M // _TILE) * -(-N // _TILE)
    fits = M >= AUTO_MIN_M and N >= AUTO_MIN_N and K >= AUTO_MIN_K and M * N >= AUTO_MIN_MN and tiles < REDUCE_MAX_TILES
    return fits, K


def reduce_path(subscripts: str, extent: Mapping[str, int], dtypes: Sequence[Any]) -> str:
    """The path ``fe_einsum_reduce`` takes for the launch (``_hip.einsum_reduce_plan`` on its descriptor agrees):
    ``"mfma"`` for two operands the contraction kernel takes with few tiles (float32 operands of a float64 einsum
    included), ``"valu"`` otherwise.  *dtypes*: unused, the path depends on the shape alone."""
    ins, _ = _split(subscripts)
    return "mfma" if len(ins) == 2 and _mfma_fits(subscripts, extent)[0] else "valu"


def split_path(subscripts: str, extent: Mapping[str, int], dtypes: Sequence[Any]) -> Optional[str]:
    """The ``"auto"`` rule for one launch of at most REDUCE_MAX_OUT output entries: ``"mfma"`` when
    ``auto_picks_contraction`` would take its two operands, its grid has fewer than REDUCE_MAX_TILES tiles and
    K >= REDUCE_MIN_SUM; ``"valu"`` when it has at least REDUCE_MIN_SUM summation points; ``None`` otherwise."""
    ins, _ = _split(subscripts)
    if not all(np.dtype(d) in _REAL for d in dtypes):
        return None
    n_out, n_sum = reduction_sizes(subscripts, extent)
    if n_out > REDUCE_MAX_OUT:
        return None
    if len(ins) == 2 and len({np.dtype(d) for d in dtypes}) == 1:
        fits, K = _mfma_fits(subscripts, extent)
        if fits and K >= REDUCE_MIN_SUM:
            return "mfma"
    if n_sum >= REDUCE_MIN_SUM:
        return reduce_path(subscripts, extent, dtypes)   # (the path the launch takes; mixed Gram: the matrix cores)
    return None


def _fits_kernels(einsum: BatchedEinsum) -> bool:
    return (einsum.n <= _hip.FE_MAX_EINSUM_OPERANDS and len(einsum.out_idx_set) <= _hip.FE_MAX_EINSUM_INDICES
            and len(einsum.sum_indices) <= _hip.FE_MAX_EINSUM_INDICES)


def auto_picks_reduction(einsum: BatchedEinsum, sizes: Mapping[str, int]) -> bool:
    """Whether ``"auto"`` runs *einsum* (outside the DG families) as a split reduction: every row meets
    :func:`split_path` (the rows share their shapes; their dtypes may differ).  An einsum of three or more operands
    that does not stream in one launch (:func:`streams_in_one_launch`) is judged by the launches it would be: when a
    step of its optimal schedule meets :func:`split_path` (``e,ij,ei,ej->`` at E = 10^6: ``ej,ei->ji`` with K = E)."""
    if not _fits_kernels(einsum) or any(np.dtype(d) not in _REAL for d in einsum.arg_to_dtype.values()):
        return False
    extent = _extents(einsum, sizes)
    if reduction_sizes(einsum.get_subscripts(), extent)[0] > REDUCE_MAX_OUT:
        return False
    if einsum.n > 2 and not streams_in_one_launch(einsum, sizes):
        try:
            return any(how == "reduce" for _, how in plan_reduction(einsum, sizes))
        except NotImplementedError:   # (rows that would need intermediates of different dtypes)
            return False
    subs = einsum.get_subscripts()
    return all(split_path(subs, extent, [a.dtype for a in row]) is not None for row in einsum.args)


def check_reduction(einsum: BatchedEinsum, sizes: Mapping[str, int]) -> None:
    """``NotImplementedError`` unless the ``"reduction"`` transform can run *einsum*: real operands, at most
    REDUCE_MAX_OUT output entries per row, the kernels' operand and index limits."""
    bad = sorted({str(np.dtype(d)) for d in einsum.arg_to_dtype.values()} - {str(d) for d in _REAL})
    if bad:
        raise NotImplementedError(f"the split reduction is compiled for float64 / float32 operands; got {bad}")
    if not _fits_kernels(einsum):
        raise NotImplementedError("einsum has more operands / indices than the split reduction supports")
    n_out, _ = reduction_sizes(einsum.get_subscripts(), _extents(einsum, sizes))
    if n_out > REDUCE_MAX_OUT:
        raise NotImplementedError(
            f"einsum '{einsum.get_subscripts()}' has {n_out} output entries per row; the split reduction writes at most"
            f" {REDUCE_MAX_OUT} (use \"generic\" or \"contraction\")")


def streams_in_one_launch(einsum: BatchedEinsum, sizes: Mapping[str, int]) -> bool:
    """Whether the trivial loop nest of *einsum* only streams its operands: summation points at most
    REDUCE_STREAM_FACTOR x the elements of its largest operand."""
    extent = _extents(einsum, sizes)
    _, n_sum = reduction_sizes(einsum.get_subscripts(), extent)
    largest = max(int(np.prod([extent[c] for c in idxs], dtype=np.int64)) for idxs in einsum.in_idx_sets)
    return n_sum <= REDUCE_STREAM_FACTOR * largest


def plan_reduction(einsum: BatchedEinsum, sizes: Mapping[str, int],
                   schedule: Optional[ContractionSchedule] = None) -> Tuple[Tuple[Step, str], ...]:
    """
    The launches of the ``"reduction"`` transform: ``(step, how)`` pairs, *how* one of ``"reduce"`` (a split launch),
    ``"contract"`` or ``"generic"``.  One or two operands, or a trivial nest that only streams
    (:func:`streams_in_one_launch`): one split launch of the whole einsum.  Otherwise the steps of the schedule
    (``plan_steps``: the caller's or the optimal one); a step meeting :func:`split_path` is a split launch, any other
    step takes the kernel ``"auto"`` would give that einsum (the contraction kernel where ``auto_picks_contraction`` says
    so, the generic kernel otherwise -- a pointwise step such as ``e,ei->ei`` is a stream, not a 64 x 64 tile per
    element).
    """
    if einsum.n <= 2 or streams_in_one_launch(einsum, sizes):
        whole = Step(einsum.get_subscripts(), tuple(("op", i) for i in range(einsum.n)), None)
        return ((whole, "reduce"),)
    extent = _extents(einsum, sizes)
    steps = plan_steps(einsum, schedule)
    plan = []
    tmp: Dict[str, np.dtype] = {}
    for st, dt in zip(steps, plan_step_dtypes(einsum, steps)):
        ins, _ = _split(st.subscripts)
        dtypes = [np.dtype(einsum.args[0][x].dtype) if kind == "op" else tmp[x] for kind, x in st.inputs]
        if st.result is not None:
            tmp[st.result] = dt
        if split_path(st.subscripts, extent, dtypes) is not None:
            how = "reduce"
        elif len(ins) == 2 and len(set(dtypes)) == 1 and _auto_contract(st.subscripts, extent):
            how = "contract"
        else:
            how = "generic"
        plan.append((st, how))
    return tuple(plan)


def check_accumulating_plan(plan: Sequence[Tuple[Step, str]]) -> None:
    """``NotImplementedError`` unless the step of *plan* (:func:`plan_reduction`) that writes the einsum's output can
    accumulate inside its kernel (``{"accumulate": "kernel"}``): a ``"reduce"`` step (``fe_einsum_reduce_acc``) or a
    ``"contract"`` step (``fe_einsum_contract_acc``).  A ``"generic"`` last step has no accumulating form."""
    for st, how in plan:
        if st.result is None and how == "generic":
            raise NotImplementedError(
                f"the step '{st.subscripts}' that writes the output runs on the generic kernel, which has no accumulating"
                ' form: {"accumulate": "kernel"} needs a split-reduction or contraction last step (use'
                ' {"accumulate": "axpby"} or another schedule)')


def _auto_contract(subscripts: str, extent: Mapping[str, int]) -> bool:
    _, M, N, K = contraction_sizes(subscripts, extent)
    return M >= AUTO_MIN_M and N >= AUTO_MIN_N and K >= AUTO_MIN_K and M * N >= AUTO_MIN_MN


class ReductionLaunch:
    """An einsum bound to device arrays for the ``"reduction"`` transform: its launches, in order.

    The intermediates and the one workspace every split launch shares (the launches run one after the other on one
    stream) are allocated on *stream*, as ``ContractionLaunch`` allocates its intermediates; a launch on another stream
    marks them with ``record_stream``.

    *scale* = ``(alpha, beta)``: the launch accumulates, ``out <- alpha E + beta out``, inside the step that writes each
    row's output -- ``fe_einsum_reduce_acc`` for a ``"reduce"`` step (its combine launch), ``fe_einsum_contract_acc`` for a
    ``"contract"`` step; the earlier steps, the intermediates and the workspace are those of the overwriting launch.
    ``NotImplementedError`` (:func:`check_accumulating_plan`) before anything is allocated for a ``"generic"`` last
    step."""

    entry_point = "fe_einsum_reduce"

    def __init__(self, einsum: BatchedEinsum, arg_dict: Mapping[str, Any], outs: Sequence[Any],
                 sizes: Mapping[str, int], schedule: Optional[ContractionSchedule] = None, stream: Any = None,
                 scale: Optional[Tuple[float, float]] = None) -> None:
        import contextlib

        import torch

        check_reduction(einsum, sizes)
        extent = _extents(einsum, sizes)
        self.plan = plan_reduction(einsum, sizes, schedule)
        self.scale = scale
        if scale is not None:
            check_accumulating_plan(self.plan)
            self.entry_point = "fe_einsum_reduce_acc"
        steps = [st for st, _ in self.plan]
        # (one launch of the whole einsum: no intermediates, and each row computes in its own np.result_type)
        step_dtypes: Tuple[np.dtype, ...] = plan_step_dtypes(einsum, steps) if len(steps) > 1 else ()
        tmp_dtype = {st.result: dt for st, dt in zip(steps, step_dtypes) if st.result is not None}
        device = outs[0].device
        self._stream_ptr = int(stream.cuda_stream) if stream is not None else None
        with torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext():
            self.intermediates: Dict[str, Any] = {
                name: torch.empty(shape, dtype=getattr(torch, tmp_dtype[name].name), device=device)
                for name, shape in intermediate_shapes(steps, extent).items()}
        pending = []
        ws_bytes = 0
        for row, out in zip(einsum.args, outs):
            for st, how in self.plan:
                tensors = [arg_dict[row[x].name] if kind == "op" else self.intermediates[x] for kind, x in st.inputs]
                dtypes = [np.dtype(row[x].dtype) if kind == "op" else tmp_dtype[x] for kind, x in st.inputs]
                target = out if st.result is None else self.intermediates[st.result]
                d = _desc(st.subscripts, tensors, extent, dtypes)
                if how == "reduce":
                    ws_bytes = max(ws_bytes, _hip.einsum_reduce_plan(d)[2])
                acc = scale is not None and st.result is None
                pending.append((how, acc, d, [t.data_ptr() for t in tensors], target.data_ptr()))
        with torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext():
            self.workspace = torch.empty(ws_bytes, dtype=torch.uint8, device=device) if ws_bytes else None
        ws = self.workspace.data_ptr() if self.workspace is not None else 0
        self._keep = (arg_dict, outs)
        self.launches = []
        for how, acc, d, ops, out_ptr in pending:
            if how == "reduce":
                self.launches.append((_reduce_call(ws, ws_bytes, scale if acc else None), d, ops, out_ptr))
            elif acc:   # (check_accumulating_plan: a "contract" step)
                self.launches.append((_contract_acc_call(*scale), d, ops, out_ptr))
            else:
                self.launches.append((_hip.einsum_contract if how == "contract" else _hip.einsum_generic,
                                      d, ops, out_ptr))

    def _buffers(self) -> List[Any]:
        return list(self.intermediates.values()) + ([self.workspace] if self.workspace is not None else [])

    def launch(self, stream_ptr: int) -> None:
        bufs = self._buffers()
        if bufs and stream_ptr != self._stream_ptr:
            import torch

            if not torch.cuda.is_current_stream_capturing():   # (a captured graph keeps its pool's blocks itself)
                s = torch.cuda.ExternalStream(stream_ptr) if stream_ptr else torch.cuda.current_stream()
                for t in bufs:
                    t.record_stream(s)
        for fn, d, ops, out in self.launches:
            fn(d, ops, out, stream_ptr)

    def time_batch(self, n: int, stream_ptr: int) -> float:
        return _hip.time_with_events(self.launch, n, stream_ptr)


def _reduce_call(ws: int, ws_bytes: int, scale: Optional[Tuple[float, float]] = None):
    def call(desc: "_hip.EinsumDesc", operands: Sequence[int], out: int, stream: int) -> None:
        if scale is None:
            _hip.einsum_reduce(desc, operands, out, ws, ws_bytes, stream)
        else:
            _hip.einsum_reduce_acc(desc, operands, out, ws, ws_bytes, scale[0], scale[1], stream)
    call.entry_point = "fe_einsum_reduce" if scale is None else "fe_einsum_reduce_acc"
    return call


__all__ = ["REDUCE_MAX_OUT", "REDUCE_MIN_SUM", "REDUCE_MAX_TILES", "REDUCE_STREAM_FACTOR", "reduction_sizes",
           "reduce_path", "split_path", "auto_picks_reduction", "check_reduction", "streams_in_one_launch",
           "plan_reduction", "check_accumulating_plan", "ReductionLaunch"]
