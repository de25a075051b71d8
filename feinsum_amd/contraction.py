"""
The ``"contraction"`` transform: einsums evaluated as strided batched tensor contractions on the
matrix cores (``fe_einsum_contract``, ``csrc/fe_contract.h``).

The reference's tuned transforms for this class (``tuning/impls/ttgt.py``, ``cogent.py``,
``cogent_w_register_prftch*.py``) accept two-operand einsums; here a two-operand einsum is one
``fe_einsum_contract`` launch per row, and an einsum of three or more operands follows a
:class:`~feinsum_amd.contraction_schedule.ContractionSchedule`: every two-operand step is a
contraction launch, a one-operand step (a pure reduction) a generic-kernel launch, and the
intermediates are device arrays allocated when the launch is bound.

Index groups of a two-operand step ``A, B -> C`` (:func:`classify_indices` by subscripts;
``fe_einsum_contract`` applies the same rule to the strides of its descriptor, ``_hip.einsum_contract_groups``):

``batch``  output index carried by both operands, or by neither (a stride-0 broadcast)
``m``      output index carried by A only
``n``      output index carried by B only
``k``      summed index (carried by one operand only: stride 0 in the other)

An operand "carries" an index when its stride along it is nonzero; a repeated index adds its strides.
"""

from __future__ import annotations

from dataclasses import dataclass
from typing import Any, Dict, List, Mapping, Optional, Sequence, Tuple

import numpy as np

from feinsum_amd import _hip
from feinsum_amd.contraction_schedule import (ContractionSchedule, EinsumOperand,
                                              get_opt_einsum_contraction_schedule,
                                              get_trivial_contraction_schedule)
from feinsum_amd.diagnostics import InvalidParameterError
from feinsum_amd.einsum import BatchedEinsum, SizeParam

#: ``"auto"`` runs a two-operand einsum outside the DG families on the contraction kernel when its m, n and k
#: spaces (products of the extents of each group, :func:`contraction_sizes`) are all at least this large and M x N fills
#: at least an eighth of a 64 x 64 tile.  Measured crossover (profiles/contraction/bench_contraction.jsonl,
#: float64): 'ik,kj->ij' with the other two sizes large -- M = 8 ties (0.97x), M = 16 wins 1.6x; N = 4 ties (1.03x),
#: N = 8 wins 2.3x; K = 4 already wins 1.6x, K = 8 4.3x; 'bij,bjk->bik' with 10^5 batches -- 16 x 8 x 8 (M N = 128)
#: loses 3.3x, 32 x 16 x 16 (512) wins 1.3x, 16 x 64 x 32 (1024) 3.6x.
AUTO_MIN_M = 16
AUTO_MIN_N = 8
AUTO_MIN_K = 8
AUTO_MIN_MN = 512


@dataclass(frozen=True)
class IndexGroups:
    batch: Tuple[str, ...]
    m: Tuple[str, ...]
    n: Tuple[str, ...]
    k: Tuple[str, ...]


def _split(subscripts: str) -> Tuple[List[str], str]:
    lhs, rhs = subscripts.replace(" ", "").split("->")
    return lhs.split(","), rhs


def classify_indices(subscripts: str) -> IndexGroups:
    """
    Batch / m / n / k groups of the two-operand einsum *subscripts* (output indices in output order, summed indices
    in order of first appearance), as the subscripts name them.  What the kernel forms from an actual descriptor
    (strides of 0, extents of 1) is ``_hip.einsum_contract_groups``.
    """
    ins, out = _split(subscripts)
    if len(ins) != 2:
        raise ValueError(f"'{subscripts}': a contraction has two operands")
    batch, m, n = [], [], []
    for idx in out:
        a, b = idx in ins[0], idx in ins[1]
        (batch if a == b else m if a else n).append(idx)
    k = [idx for idx in dict.fromkeys(ins[0] + ins[1]) if idx not in out]
    return IndexGroups(tuple(batch), tuple(m), tuple(n), tuple(k))


def contraction_sizes(subscripts: str, extent: Mapping[str, int]) -> Tuple[int, int, int, int]:
    """``(batch count, M, N, K)`` of a two-operand step: the products of the extents of each group."""
    g = classify_indices(subscripts)
    prod = lambda idxs: int(np.prod([extent[i] for i in idxs], dtype=np.int64))   # noqa: E731
    return prod(g.batch), prod(g.m), prod(g.n), prod(g.k)


def _extents(einsum: BatchedEinsum, sizes: Mapping[str, int]) -> Dict[str, int]:
    return {idx: (int(sizes[d.name]) if isinstance(d, SizeParam) else int(d))
            for idx, d in einsum.index_to_dim_length.items()}


def _uniform_real_dtype(einsum: BatchedEinsum) -> Optional[np.dtype]:
    dtypes = {np.dtype(dt) for dt in einsum.arg_to_dtype.values()}
    if len(dtypes) == 1 and next(iter(dtypes)) in (np.dtype("float64"), np.dtype("float32")):
        return next(iter(dtypes))
    return None


def auto_picks_contraction(einsum: BatchedEinsum, sizes: Mapping[str, int]) -> bool:
    """Whether ``"auto"`` runs *einsum* (outside the DG families) on the contraction kernel: two operands of one
    real dtype, M >= AUTO_MIN_M, N >= AUTO_MIN_N, K >= AUTO_MIN_K and M N >= AUTO_MIN_MN.  Matrix-vector products, reductions,
    pointwise products and everything with one or three and more operands keep the generic kernel."""
    if einsum.n != 2 or _uniform_real_dtype(einsum) is None:
        return False
    if len(einsum.out_idx_set) > _hip.FE_MAX_EINSUM_INDICES or len(einsum.sum_indices) > _hip.FE_MAX_EINSUM_INDICES:
        return False
    _, M, N, K = contraction_sizes(einsum.get_subscripts(), _extents(einsum, sizes))
    return M >= AUTO_MIN_M and N >= AUTO_MIN_N and K >= AUTO_MIN_K and M * N >= AUTO_MIN_MN


# --------------------------------------------------------------------------
# the steps of a schedule
# --------------------------------------------------------------------------

@dataclass(frozen=True)
class Step:
    """One launch: ``subscripts`` over ``inputs`` (``("op", i)``: operand i of the einsum, ``("tmp", name)``: the result
    of an earlier step) into ``result`` (``None``: the einsum's output)."""

    subscripts: str
    inputs: Tuple[Tuple[str, Any], ...]
    result: Optional[str]


def plan_steps(einsum: BatchedEinsum, schedule: Optional[ContractionSchedule] = None) -> Tuple[Step, ...]:
    """
    The launches of the ``"contraction"`` transform.  *schedule* defaults to the whole einsum for one or two
    operands and to ``get_opt_einsum_contraction_schedule`` otherwise.  A schedule step of three or more operands
    is split left to right into two-operand steps, each keeping the indices still needed.  The last step writes
    the output, and its output subscripts must be the einsum's own.
    """
    if schedule is None:
        schedule = get_trivial_contraction_schedule(einsum) if einsum.n <= 2 \
            else get_opt_einsum_contraction_schedule(einsum)
    out_str = "".join(einsum.out_idx_set)
    steps: List[Step] = []
    for istep, (subs, args, name) in enumerate(zip(schedule.subscripts, schedule.arguments,
                                                   schedule.result_names)):
        ins, rhs = _split(subs)
        if len(ins) != len(args):
            raise InvalidParameterError(f"schedule step '{subs}' has {len(args)} arguments")
        last = istep == schedule.nsteps - 1
        if last and rhs != out_str:
            raise InvalidParameterError(f"the last schedule step writes '{rhs}', the einsum's output is '{out_str}'")
        srcs = [("op", a.ioperand) if isinstance(a, EinsumOperand) else ("tmp", a.name) for a in args]
        result = None if last else name
        terms = list(zip(ins, srcs))
        part = 0
        while len(terms) > 2:   # an n-ary step: contract the first two, keep what the rest or the output needs
            (sa, xa), (sb, xb) = terms[0], terms[1]
            need = set(rhs).union(*[s for s, _ in terms[2:]])
            keep = "".join(c for c in dict.fromkeys(sa + sb) if c in need)
            tmp = f"{name}_part{part}"
            part += 1
            steps.append(Step(f"{sa},{sb}->{keep}", (xa, xb), tmp))
            terms = [(keep, ("tmp", tmp))] + terms[2:]
        steps.append(Step(",".join(s for s, _ in terms) + "->" + rhs, tuple(x for _, x in terms), result))
    return tuple(steps)


def intermediate_shapes(steps: Sequence[Step], extent: Mapping[str, int]) -> Dict[str, Tuple[int, ...]]:
    """Shape of every intermediate the steps produce, by name."""
    return {st.result: tuple(int(extent[c]) for c in _split(st.subscripts)[1])
            for st in steps if st.result is not None}


def check_accumulating_steps(steps: Sequence[Step]) -> None:
    """``NotImplementedError`` unless the step of *steps* (``plan_steps``) that writes the einsum's output can accumulate
    inside its kernel (``{"accumulate": "kernel"}``): a two-operand step, which runs on the contraction kernel
    (``fe_einsum_contract_acc``).  A one-input last step -- a caller's schedule that ends in a pure reduction -- runs on
    the generic kernel, which has no accumulating form."""
    for st in steps:
        if st.result is None and len(st.inputs) != 2:
            raise NotImplementedError(
                f"the step '{st.subscripts}' that writes the output has {len(st.inputs)} input(s) and runs on the generic"
                ' kernel, which has no accumulating form: {"accumulate": "kernel"} needs a two-operand last step'
                ' (use {"accumulate": "axpby"} or another schedule)')


_REAL = (np.dtype("float64"), np.dtype("float32"))


def plan_step_dtypes(einsum: BatchedEinsum, steps: Sequence[Step]) -> Tuple[np.dtype, ...]:
    """
    The result dtype of every step of *steps* (``plan_steps``): ``np.result_type`` of the step's own operands, as the
    reference types each intermediate (codegen/loopy.py:258-260) -- a step over float32 operands stays float32, one
    that meets a float64 operand is float64.  The intermediates are allocated in these dtypes.  The rows of the einsum
    share the intermediates, so they must agree: rows whose operands differ in dtype where a step meets them are
    ``NotImplementedError``, as is any operand that is not float32 or float64.
    """
    bad = sorted({str(np.dtype(d)) for d in einsum.arg_to_dtype.values()} - {str(d) for d in _REAL})
    if bad:
        raise NotImplementedError(f"the contraction kernel is compiled for float64 / float32 operands; got {bad}")
    result: Optional[Tuple[np.dtype, ...]] = None
    for row in einsum.args:
        tmp: Dict[str, np.dtype] = {}
        dts = []
        for st in steps:
            dt = np.result_type(*[np.dtype(row[x].dtype) if kind == "op" else tmp[x] for kind, x in st.inputs])
            if st.result is not None:
                tmp[st.result] = dt
            dts.append(dt)
        if result is not None and tuple(dts) != result:
            raise NotImplementedError("the rows of this einsum would need intermediates of different dtypes")
        result = tuple(dts)
    return result or ()


def _desc(subscripts: str, tensors: Sequence[Any], extent: Mapping[str, int],
          operand_dtypes: Sequence[np.dtype]) -> "_hip.EinsumDesc":
    """Descriptor of one step: ``np.result_type`` of its operands is the compute type; float32 operands of a float64 step
    are flagged (mixed: the kernels widen them as they load them)."""
    ins, rhs = _split(subscripts)
    sums = [c for c in dict.fromkeys("".join(ins)) if c not in rhs]
    return _hip.einsum_desc(ins, rhs, sums, extent, tensors,
                            np.result_type(*operand_dtypes) == np.dtype("float64"), operand_dtypes)


class ContractionLaunch:
    """An einsum bound to device arrays for the ``"contraction"`` transform: its launches, in order.

    The intermediates are allocated on *stream* (the queue's stream: the launches run there), so that the caching
    allocator hands their blocks to later allocations only in that stream's order; a launch on another stream marks
    them as used by it (``record_stream``) so that they outlive its work too.

    *scale* = ``(alpha, beta)``: the launch accumulates, ``out <- alpha E + beta out``, inside the kernel of the step that
    writes each row's output (``fe_einsum_contract_acc``); the earlier steps and the intermediates are those of the
    overwriting launch.  ``NotImplementedError`` (:func:`check_accumulating_steps`) before anything is allocated when
    that step is not a two-operand one."""

    entry_point = "fe_einsum_contract"

    def __init__(self, einsum: BatchedEinsum, arg_dict: Mapping[str, Any], outs: Sequence[Any],
                 sizes: Mapping[str, int], schedule: Optional[ContractionSchedule] = None, stream: Any = None,
                 scale: Optional[Tuple[float, float]] = None) -> None:
        import contextlib

        import torch

        extent = _extents(einsum, sizes)
        self.steps = plan_steps(einsum, schedule)
        self.scale = scale
        if scale is not None:
            check_accumulating_steps(self.steps)
            self.entry_point = "fe_einsum_contract_acc"
        self.step_dtypes = plan_step_dtypes(einsum, self.steps)
        tmp_dtype = {st.result: dt for st, dt in zip(self.steps, self.step_dtypes) if st.result is not None}
        device = outs[0].device
        # intermediates: one set, reused by every row (the rows run one after the other on one stream), each in the
        # dtype of its own step (plan_step_dtypes)
        self._stream_ptr = int(stream.cuda_stream) if stream is not None else None
        with torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext():
            self.intermediates = {name: torch.empty(shape, dtype=getattr(torch, tmp_dtype[name].name), device=device)
                                  for name, shape in intermediate_shapes(self.steps, extent).items()}
        self._keep = (arg_dict, outs)
        self.launches = []
        for row, out in zip(einsum.args, outs):
            for st in self.steps:
                tensors = [arg_dict[row[x].name] if kind == "op" else self.intermediates[x] for kind, x in st.inputs]
                dtypes = [np.dtype(row[x].dtype) if kind == "op" else tmp_dtype[x] for kind, x in st.inputs]
                target = out if st.result is None else self.intermediates[st.result]
                d = _desc(st.subscripts, tensors, extent, dtypes)
                fn = _hip.einsum_contract if len(tensors) == 2 else _hip.einsum_generic
                if scale is not None and st.result is None:
                    fn = _contract_acc_call(*scale)
                self.launches.append((fn, d, [t.data_ptr() for t in tensors], target.data_ptr()))

    def launch(self, stream_ptr: int) -> None:
        if self.intermediates and stream_ptr != self._stream_ptr:
            import torch

            if not torch.cuda.is_current_stream_capturing():   # (a captured graph keeps its pool's blocks itself)
                s = torch.cuda.ExternalStream(stream_ptr) if stream_ptr else torch.cuda.current_stream()
                for t in self.intermediates.values():
                    t.record_stream(s)
        for fn, d, ops, out in self.launches:
            fn(d, ops, out, stream_ptr)

    def time_batch(self, n: int, stream_ptr: int) -> float:
        return _hip.time_with_events(self.launch, n, stream_ptr)


def _contract_acc_call(alpha: float, beta: float):
    def call(desc: "_hip.EinsumDesc", operands: Sequence[int], out: int, stream: int) -> None:
        _hip.einsum_contract_acc(desc, operands, out, alpha, beta, stream)
    call.entry_point = "fe_einsum_contract_acc"
    return call
