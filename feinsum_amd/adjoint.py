"""
Host side of the adjoint kernels (``feinsum_amd/csrc/fe_adjoint.h``): an einsum that
:func:`feinsum_amd.family.match_adjoint_family` recognises, bound to device arrays.

Reached in two ways only: ``evaluate(..., transform="adjoint")`` and the backward pass of
:func:`feinsum_amd.autograd.evaluate_differentiable`.  ``"auto"`` never picks these kernels.
"""

from __future__ import annotations

from typing import Any, Mapping, Sequence

from feinsum_amd import _hip
from feinsum_amd.einsum import BatchedEinsum
from feinsum_amd.family import (ADJ_FACEMASS_J, ADJ_FACEMASS_V, ADJ_GEOM, ADJ_OPERATOR_D, ADJ_OPERATOR_R, OP_TRANSPOSED,
                                AdjointPlan)


def _contiguous_strides(shape: Sequence[int]) -> Sequence[int]:
    strides, acc = [], 1
    for d in reversed(shape):
        strides.append(acc)
        acc *= int(d)
    return tuple(reversed(strides))


class AdjointLaunch:
    """An adjoint plan bound to device arrays: one launch per row (geometric-factor adjoint, face-mass J-adjoint) or per
    run of rows sharing J and R (face-mass v-adjoint).  ``sum_rows``: the face-mass J-adjoint of rows that all share R
    writes the SUM of its rows into ``outs[0]`` in one launch (the fields summed in row order inside the kernel).

    The operator gradients (``ADJ_OPERATOR_D`` / ``ADJ_OPERATOR_R``, ``family.match_operator_adjoint``) are one launch
    per row, or with ``sum_rows`` one launch for all rows (they share J) into ``outs[0]``.  Their workspace is allocated
    on *stream* (the queue's), as ``ReductionLaunch`` allocates its own; a launch on another stream marks it with
    ``record_stream``."""

    def __init__(self, plan: AdjointPlan, einsum: BatchedEinsum, arg_dict: Mapping[str, Any], outs: Sequence[Any],
                 sum_rows: bool = False, stream: Any = None) -> None:
        self.plan = plan
        self._keep = (arg_dict, outs)
        self.calls = []
        self.workspace, self._stream_ptr = None, None
        role, rows, p = plan.roles, einsum.args, plan.params
        ptr = lambda row, r: int(arg_dict[row[role[r]].name].data_ptr())   # noqa: E731
        if plan.kind in (ADJ_OPERATOR_D, ADJ_OPERATOR_R):
            self._bind_operator_gradient(einsum, arg_dict, outs, sum_rows, stream, ptr)
            return
        if plan.kind == ADJ_GEOM:
            E = int(arg_dict[rows[0][role["a"]].name].shape[0])
            shape = [int(outs[0].shape[k]) for k in range(outs[0].dim())]
            strides = dict(zip(einsum.out_idx_set, _contiguous_strides(shape)))
            st = tuple(strides.get(plan.letters[t], 0) if t in plan.letters else 0 for t in ("x", "r", "e"))
            opT = OP_TRANSPOSED if plan.layout_flags & OP_TRANSPOSED else 0
            for row, out in zip(rows, outs):
                self.calls.append((_hip.geomadj, (ptr(row, "D"), ptr(row, "a"), ptr(row, "b"), int(out.data_ptr()), E,
                                                  p["X"], p["R"], p["Np"], st), {"op_flags": opT}))
            return
        E = int(arg_dict[rows[0][role["g"]].name].shape[0])
        fm = (p["Np"], p["nf"], p["Nfp"])
        if plan.kind == ADJ_FACEMASS_V:
            k = 0
            while k < len(rows):   # consecutive rows sharing J and R: one launch
                k2 = k + 1
                while k2 < len(rows) and all(rows[k2][role[r]].name == rows[k][role[r]].name for r in ("J", "R")):
                    k2 += 1
                self.calls.append((_hip.facemass_adj, (ptr(rows[k], "J"), ptr(rows[k], "R"),
                                                       [ptr(rows[m], "g") for m in range(k, k2)], None,
                                                       [int(outs[m].data_ptr()) for m in range(k, k2)], None, E, *fm),
                                   {"layout_flags": plan.layout_flags}))
                k = k2
            return
        assert plan.kind == ADJ_FACEMASS_J
        groups = [list(range(len(rows)))] if sum_rows else [[m] for m in range(len(rows))]
        if sum_rows and len({row[role["R"]].name for row in rows}) != 1:
            raise ValueError("sum_rows needs one R shared by every row")
        for m in groups:
            self.calls.append((_hip.facemass_adj, (None, ptr(rows[m[0]], "R"), [ptr(rows[q], "g") for q in m],
                                                   [ptr(rows[q], "v") for q in m], None, int(outs[m[0]].data_ptr()),
                                                   E, *fm),
                               {"layout_flags": plan.layout_flags}))

    def _bind_operator_gradient(self, einsum, arg_dict, outs, sum_rows, stream, ptr) -> None:
        import contextlib

        import torch

        plan, rows, p = self.plan, einsum.args, self.plan.params
        volume = plan.kind == ADJ_OPERATOR_D
        first = arg_dict[rows[0][plan.roles["a" if volume else "g"]].name]
        E = int(first.shape[0])
        entries = p["R"] * p["Np"] * p["Np"] if volume else p["nf"] * p["Np"] * p["Nfp"]
        _, ws_bytes = _hip.opgrad_plan(E, entries)
        self._stream_ptr = int(stream.cuda_stream) if stream is not None else None
        with torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext():
            self.workspace = torch.empty(ws_bytes, dtype=torch.uint8, device=first.device) if ws_bytes else None
        ws = int(self.workspace.data_ptr()) if self.workspace is not None else None
        groups = [list(range(len(rows)))] if sum_rows else [[m] for m in range(len(rows))]
        for m in groups:
            out = int(outs[m[0]].data_ptr())
            if volume:
                jst = tuple(ce * E + c for ce, c in p["jstrides"])
                self.calls.append((_hip.opgrad, (ptr(rows[m[0]], "J"), [ptr(rows[q], "a") for q in m],
                                                 [ptr(rows[q], "b") for q in m], out, E, p["X"], p["R"], p["Np"], jst,
                                                 p["strides"], ws, ws_bytes), {}))
            else:
                self.calls.append((_hip.facemass_opgrad, (ptr(rows[m[0]], "J"), [ptr(rows[q], "g") for q in m],
                                                          [ptr(rows[q], "v") for q in m], out, E, p["Np"], p["nf"],
                                                          p["Nfp"], ws, ws_bytes), {"layout_flags": plan.layout_flags}))

    def launch(self, stream_ptr: int) -> None:
        if self.workspace is not None and stream_ptr != self._stream_ptr:
            import torch

            if not torch.cuda.is_current_stream_capturing():   # (a captured graph keeps its pool's blocks itself)
                s = torch.cuda.ExternalStream(stream_ptr) if stream_ptr else torch.cuda.current_stream()
                self.workspace.record_stream(s)
        for fn, args, kw in self.calls:
            fn(*args, stream=stream_ptr, **kw)

    def time_batch(self, n: int, stream_ptr: int) -> float:
        return _hip.time_with_events(self.launch, n, stream_ptr)


def adjoint_bytes_per_element(plan: AdjointPlan, b: int = 1, with_dv: bool = True, with_dJ: bool = True) -> int:
    """Bytes an adjoint launch must move per element (the roofline's numerator; operators not counted)."""
    p = plan.params
    if plan.kind == ADJ_GEOM:
        return 8 * (p["Np"] + p["X"] * p["Np"] + p["X"] * p["R"])
    if plan.kind == ADJ_OPERATOR_D:
        return 8 * (b * (p["Np"] + p["X"] * p["Np"]) + p["X"] * p["R"])
    if plan.kind == ADJ_OPERATOR_R:
        return 8 * (b * (p["Np"] + p["nf"] * p["Nfp"]) + p["nf"])
    nf, Np, Nfp = p["nf"], p["Np"], p["Nfp"]
    n = b * Np                                          # g_k
    n += (nf if with_dv else 0) + (b * nf * Nfp if with_dv else 0)   # J, dv_k
    n += (b * nf * Nfp + nf if with_dJ else 0)          # v_k, dJ
    return 8 * n
