"""
Differentiate einsum evaluations through ``torch.autograd``.

Every einsum is linear in each operand, so the vector-Jacobian product with respect to an input array A is a sum of
einsums: for every occurrence of A (every row, every operand position), the row's other operands times the gradient
of that row's output, summed to A's subscripts.  :func:`adjoint_einsums` builds those terms with the existing
builders; :func:`evaluate_differentiable` evaluates the forward with :func:`~feinsum_amd.measure.evaluate` and the
terms in its backward pass -- on the DG family kernels where a term is a family einsum (grad's u-adjoint is div with
the transposed operator, ...), on the adjoint kernels where :func:`~feinsum_amd.family.match_adjoint_family`
recognises it (the geometric-factor and face-mass adjoints), and with ``"auto"`` otherwise.
"""

from __future__ import annotations

from collections import Counter
from dataclasses import dataclass
from types import MappingProxyType
from typing import Any, List, Mapping, NamedTuple, Optional, Sequence, Tuple

import numpy as np

from feinsum_amd.contraction_schedule import ContractionSchedule
from feinsum_amd.einsum import BatchedEinsum, SizeParam
from feinsum_amd.family import (ADJ_FACEMASS_J, WEIGHTED_WEIGHT_ADJOINT_MAX_FIELDS, element_operator_groups, match_adjoint_family,
                                match_element_operator, match_family, match_operator_adjoint, match_weighted_element_operator,
                                match_weighted_operator_weight_adjoint, weighted_element_operator_groups)
from feinsum_amd.make_einsum import array

#: prefix of the output-gradient operands of the adjoint einsums; no user array may start with it
GRAD_PREFIX = "_fe_grad"

#: launches of the backward passes of this process, by route: "family", "geomadj", "facemass_v", "facemass_j", "auto",
#: and with ``operator_gradients="kernel"`` also "opgrad_d", "opgrad_r"; with ``element_gradients="kernel"`` also "weighted_u",
#: "weighted_w", "elemop_u" (these three count calls of the C entry points)
launch_counts: Counter = Counter()


def output_grad_name(out_name: str) -> str:
    """Name of the operand that carries the gradient of output *out_name* (``_fe_out`` -> ``_fe_grad_fe_out``)."""
    return GRAD_PREFIX + out_name


class AdjointTerm(NamedTuple):
    """One adjoint einsum of :func:`adjoint_terms`: each row is one occurrence of ``wrt``; ``wrt_subscripts`` are
    ``wrt``'s subscripts at that operand position.  ``einsum.out_idx_set`` is ``wrt_subscripts`` without the indices
    that no other operand and not the output carry: the term's value is broadcast along those."""

    einsum: BatchedEinsum
    wrt_subscripts: Tuple[str, ...]
    forward_rows: Tuple[int, ...]


def adjoint_terms(einsum: BatchedEinsum, wrt: str) -> List[AdjointTerm]:
    """The adjoint einsums of *einsum* with respect to input array *wrt*, one :class:`AdjointTerm` per operand position
    at which *wrt* occurs (its rows: the forward rows with *wrt* there).  The outputs of all rows of all terms, each
    broadcast to *wrt*'s shape (:func:`expand_to_operand`), sum to the vector-Jacobian product."""
    if wrt not in einsum.all_args:
        raise ValueError(f"'{wrt}' is not an input array of '{einsum.get_subscripts()}'")
    clash = sorted(name for name in einsum.all_args if name.startswith(GRAD_PREFIX))
    if clash:
        raise ValueError(f"array names starting with '{GRAD_PREFIX}' are reserved for output gradients: {clash}")
    positions: dict = {}
    for k, row in enumerate(einsum.args):
        for p, arg in enumerate(row):
            if arg.name == wrt:
                positions.setdefault(p, []).append(k)
    terms = []
    for p, rows in sorted(positions.items()):
        w_idx = einsum.in_idx_sets[p]
        if len(set(w_idx)) != len(w_idx):
            raise NotImplementedError(
                f"operand '{wrt}' repeats an index in its subscripts '{''.join(w_idx)}' (a diagonal): its gradient "
                "is not an einsum of the other operands")
        others = [q for q in range(einsum.n) if q != p]
        in_sets = tuple(einsum.in_idx_sets[q] for q in others) + (einsum.out_idx_set,)
        present = {i for s in in_sets for i in s}
        out_idx = tuple(i for i in w_idx if i in present)
        args = []
        for k in rows:
            dt = np.result_type(*[a.dtype for a in einsum.args[k]])
            args.append(tuple(einsum.args[k][q] for q in others)
                        + (array(output_grad_name(einsum.output_names[k]), einsum.shape, dt),))
        terms.append(AdjointTerm(BatchedEinsum(out_idx, in_sets, tuple(args)), w_idx, tuple(rows)))
    return terms


def adjoint_einsums(einsum: BatchedEinsum, wrt: str) -> List[BatchedEinsum]:
    """The einsums whose outputs sum to the vector-Jacobian product of *einsum* for input array *wrt*: one output row per
    occurrence of *wrt*; the gradient of output ``name`` is the operand ``output_grad_name(name)`` (0-d for a scalar
    output); indices of *wrt* that no other operand carries are left out of a term's output (broadcast, see
    :func:`adjoint_terms`).  ``NotImplementedError`` for an operand with a repeated index (``ii->i``)."""
    return [t.einsum for t in adjoint_terms(einsum, wrt)]


def expand_to_operand(value: Any, term_out: Sequence[str], wrt_subscripts: Sequence[str], shape: Sequence[int]) -> Any:
    """Broadcast a term's output (numpy or torch; axes *term_out*) to the operand's axes *wrt_subscripts* / *shape*."""
    view = tuple(int(shape[k]) if i in term_out else 1 for k, i in enumerate(wrt_subscripts))
    value = value.reshape(view)
    if hasattr(value, "expand"):      # torch (a size tuple: a 0-d operand expands to ())
        return value.expand(tuple(int(d) for d in shape))
    return np.broadcast_to(value, tuple(int(d) for d in shape))


# --------------------------------------------------------------------------
# torch.autograd
# --------------------------------------------------------------------------

@dataclass(frozen=True)
class _Spec:
    einsum: BatchedEinsum
    names: Tuple[str, ...]
    queue: Any
    transform: Any
    schedule: Optional[ContractionSchedule]
    operator_gradients: str = "auto"
    element_gradients: str = "auto"


def _concrete(shape, sizes) -> Tuple[int, ...]:
    return tuple(sizes[d.name] if isinstance(d, SizeParam) else int(d) for d in shape)


def _sum_rows(term: BatchedEinsum, outs: Mapping[str, Any]) -> Any:
    total = None
    for name in term.output_names:
        total = outs[name] if total is None else total.add_(outs[name])
    return total


def _run_element_term(term: BatchedEinsum, args: Mapping[str, Any], q: Any, shape: Tuple[int, ...], dtypes: Sequence[Any]) -> Any:
    """``element_gradients="kernel"``: the term on the matrix-core kernels of the element operators where a matcher accepts
    it (sum of its rows), else ``None``."""
    import torch

    from feinsum_amd import measure

    w_plan = match_weighted_operator_weight_adjoint(term)
    if w_plan is not None:
        # the weight gradient: one call sums at most 8 rows; the results of further calls are added in row order
        n_calls = -(-term.b // WEIGHTED_WEIGHT_ADJOINT_MAX_FIELDS)
        outs = [torch.empty(shape, dtype=dtypes[0], device=q.torch_device) for _ in range(n_calls)]
        with torch.cuda.device(q.torch_device):
            measure._WeightGradLaunch(w_plan, term, args, outs).launch(q.stream_ptr)
        launch_counts[w_plan.kind] += n_calls
        total = outs[0]
        for more in outs[1:]:
            total.add_(more)
        return total
    for match, groups, transform, route in (
            (match_weighted_element_operator, weighted_element_operator_groups, "weighted_element_operator", "weighted_u"),
            (match_element_operator, element_operator_groups, "element_operator", "elemop_u")):
        plan = match(term)
        if plan is not None:
            outs = {name: torch.empty(shape, dtype=dt, device=q.torch_device) for name, dt in zip(term.output_names, dtypes)}
            measure.evaluate(term, q, args, out_dict=outs, transform=transform)
            launch_counts[route] += len(groups(plan, term))
            return _sum_rows(term, outs)
    return None


def _run_term(term: BatchedEinsum, args: Mapping[str, Any], q: Any, operator_gradients: str = "auto",
              element_gradients: str = "auto") -> Any:
    """Sum of the rows of an adjoint einsum, on q's stream, in ordinary torch allocations."""
    import torch

    from feinsum_amd import measure
    from feinsum_amd.adjoint import AdjointLaunch

    sizes = measure._long_length(term, args)
    shape = _concrete(term.shape, sizes)
    dtypes = [getattr(torch, measure.result_dtype(term, k).name) for k in range(term.b)]
    if element_gradients == "kernel":
        total = _run_element_term(term, args, q, shape, dtypes)
        if total is not None:
            return total
    op_plan = match_operator_adjoint(term) if operator_gradients == "kernel" else None
    if op_plan is not None:
        # the operator gradient on the matrix cores: one launch, the rows (they share J) summed in the kernel in row order
        out = torch.empty(shape, dtype=dtypes[0], device=q.torch_device)
        with torch.cuda.device(q.torch_device):
            AdjointLaunch(op_plan, term, args, [out], sum_rows=True, stream=q.stream).launch(q.stream_ptr)
        launch_counts[op_plan.kind] += 1
        return out
    plan = match_adjoint_family(term)
    if plan is not None and plan.kind == ADJ_FACEMASS_J and len({row[plan.roles["R"]].name for row in term.args}) == 1:
        # every field into one dJ, summed inside the kernel in row order
        out = torch.empty(shape, dtype=dtypes[0], device=q.torch_device)
        with torch.cuda.device(q.torch_device):
            AdjointLaunch(plan, term, args, [out], sum_rows=True).launch(q.stream_ptr)
        launch_counts[plan.kind] += 1
        return out
    outs = {name: torch.empty(shape, dtype=dt, device=q.torch_device) for name, dt in zip(term.output_names, dtypes)}
    if plan is not None:
        measure.evaluate(term, q, args, out_dict=outs, transform="adjoint")
        launch_counts[plan.kind] += 1
    else:
        measure.evaluate(term, q, args, out_dict=outs)
        launch_counts["family" if match_family(term) is not None else "auto"] += 1
    return _sum_rows(term, outs)


def _batched_field_gradients(ctx, spec: _Spec, args: Mapping[str, Any], have: set) -> Mapping[str, Any]:
    """``element_gradients="kernel"`` and a forward that is a weighted element operator: the u-adjoints of the rows of one
    forward call (``family.weighted_element_operator_groups``: they share P, W and A) as ONE batched einsum in one
    ``evaluate`` call, so that a tile's W is read once for all fields, as in the forward.  Of every such group the rows
    whose field needs a gradient and whose output gradient is present -- where each of those fields occurs in exactly one
    forward row; anything else is left to the per-term route.  Returns {field name: gradient}."""
    import torch

    from feinsum_amd import measure

    einsum, q = spec.einsum, spec.queue
    plan = match_weighted_element_operator(einsum)
    if plan is None:
        return {}
    u_pos = plan.roles["u"]
    occurrences = Counter(arg.name for row in einsum.args for arg in row)
    needs = {name for pos, name in enumerate(spec.names) if ctx.needs_input_grad[pos + 1]}
    done = {}
    for group in weighted_element_operator_groups(plan, einsum):
        fields = [einsum.args[k][u_pos].name for k in group
                  if einsum.output_names[k] in have and einsum.args[k][u_pos].name in needs]
        if not fields or any(occurrences[name] != 1 for name in fields):
            continue
        terms = [adjoint_terms(einsum, name)[0].einsum for name in fields]    # one term of one row each, all of one shape
        batched = terms[0].copy(args=tuple(t.args[0] for t in terms))
        adj_plan = match_weighted_element_operator(batched)
        if adj_plan is None:                                                  # (the size rule is not symmetric under Ni <-> Nj)
            continue
        shape = _concrete(batched.shape, measure._long_length(batched, args))
        outs = {name: torch.empty(shape, dtype=torch.float64, device=q.torch_device) for name in batched.output_names}
        measure.evaluate(batched, q, args, out_dict=outs, transform="weighted_element_operator")
        launch_counts["weighted_u"] += len(weighted_element_operator_groups(adj_plan, batched))
        done.update(zip(fields, (outs[name] for name in batched.output_names)))
    return done


def _backward(ctx, spec: _Spec, grads) -> List[Any]:
    einsum, q = spec.einsum, spec.queue
    saved = ctx.saved_tensors
    args = dict(zip(spec.names, saved))
    have = set()
    for name, g in zip(einsum.output_names, grads):
        if g is not None:                        # an output without a gradient contributes nothing
            args[output_grad_name(name)] = g.contiguous()
            have.add(name)
    batched = _batched_field_gradients(ctx, spec, args, have) if spec.element_gradients == "kernel" else {}
    result = []
    for pos, name in enumerate(spec.names):
        if not ctx.needs_input_grad[pos + 1]:
            result.append(None)
            continue
        if name in batched:
            result.append(batched[name])
            continue
        target = saved[pos]
        total = None
        for term in adjoint_terms(einsum, name):
            rows = tuple(row for row, k in zip(term.einsum.args, term.forward_rows) if einsum.output_names[k] in have)
            if not rows:
                continue
            sub = term.einsum.copy(args=rows)
            value = expand_to_operand(_run_term(sub, args, q, spec.operator_gradients, spec.element_gradients), sub.out_idx_set, term.wrt_subscripts, target.shape)
            total = value.contiguous() if total is None else total.add_(value)
        if total is not None and total.dtype != target.dtype:
            total = total.to(target.dtype)       # float32 operand of a float64 einsum: computed in float64, rounded once
        result.append(total)
    return result


def _function():
    import torch
    from torch.autograd.function import once_differentiable

    class _EinsumFunction(torch.autograd.Function):
        @staticmethod
        def forward(ctx, spec: _Spec, *tensors):
            from feinsum_amd import measure

            ctx.set_materialize_grads(False)
            q = spec.queue
            cur = torch.cuda.current_stream(q.torch_device)
            own = q.stream != cur
            if own:
                q.stream.wait_stream(cur)
            outs = measure.evaluate(spec.einsum, q, dict(zip(spec.names, tensors)), transform=spec.transform,
                                    schedule=spec.schedule)
            if own:      # the outputs belong to the queue's stream (measure.DeviceQueue); torch goes on with them on its own
                from feinsum_amd import placement

                cur.wait_stream(q.stream)
                for t in outs.values():
                    placement.record_stream(t, cur)
            ctx.spec = spec
            ctx.save_for_backward(*tensors)
            return tuple(outs[name] for name in spec.einsum.output_names)

        @staticmethod
        @once_differentiable
        def backward(ctx, *grads):
            spec = ctx.spec
            q = spec.queue
            cur = torch.cuda.current_stream(q.torch_device)
            if q.stream == cur:
                return (None, *_backward(ctx, spec, grads))
            # a queue of its own stream: everything below (launches, allocations, sums) runs on it, after the work that
            # produced the output gradients, and torch's current stream waits for it before it uses the gradients
            q.stream.wait_stream(cur)
            with torch.cuda.stream(q.stream):
                result = _backward(ctx, spec, grads)
            cur.wait_stream(q.stream)
            for t in result:
                if t is not None:
                    t.record_stream(cur)
            return (None, *result)

    return _EinsumFunction


_FN = None


def evaluate_differentiable(einsum: BatchedEinsum, cq: Any, arg_dict: Mapping[str, Any], *, transform: Any = None,
                            schedule: Optional[ContractionSchedule] = None,
                            operator_gradients: str = "auto", element_gradients: str = "auto") -> Mapping[str, Any]:
    """:func:`~feinsum_amd.measure.evaluate` as a ``torch.autograd.Function``: returns ``{name: tensor}``, bitwise the
    outputs of ``evaluate`` with the same *transform*, carrying a ``grad_fn`` when an input requires grad.  The backward
    pass computes the gradients ``ctx.needs_input_grad`` asks for, on the stream it runs on (with a ``DeviceQueue`` of
    its own stream: ordered against torch's current stream by events both ways), into ordinary torch allocations.
    Double backward is not supported (``once_differentiable``).

    *operator_gradients*: ``"auto"`` runs the gradients with respect to the operator matrices (D, R) as ``"auto"`` runs
    their adjoint einsums; ``"kernel"`` sends every such term that :func:`~feinsum_amd.family.match_operator_adjoint`
    accepts to the operator-gradient kernels (``launch_counts["opgrad_d"]`` / ``["opgrad_r"]``; one launch for all rows
    of a batched term) and leaves every other term on its route.  Anything else: ``InvalidParameterError``.

    *element_gradients*: ``"auto"`` changes nothing (``transform="element_operator"`` and ``"weighted_element_operator"`` are
    refused).  ``"kernel"`` allows those two transforms in the forward and, whatever the forward transform, sends every adjoint
    term that :func:`~feinsum_amd.family.match_weighted_element_operator` or
    :func:`~feinsum_amd.family.match_element_operator` accepts (the u-adjoints) to those kernels, and every term that
    :func:`~feinsum_amd.family.match_weighted_operator_weight_adjoint` accepts (the gradient of the weight W) to
    ``fe_weightgrad_f64``; ``launch_counts["weighted_u"]`` / ``["elemop_u"]`` / ``["weighted_w"]`` count the calls.  The fields
    of one forward call of a weighted element operator are differentiated in one batched call (W is read once per tile).
    Every other term -- the gradients of P, A and J among them -- keeps its route.  Anything else: ``InvalidParameterError``."""
    global _FN
    from feinsum_amd.diagnostics import InvalidParameterError
    from feinsum_amd.measure import _as_queue

    if operator_gradients not in ("auto", "kernel"):
        raise InvalidParameterError(f"operator_gradients must be 'auto' or 'kernel' (got {operator_gradients!r})")
    if isinstance(transform, (str, Mapping)) and (transform if isinstance(transform, str) else transform.get("variant")) == "mixed_state":
        raise NotImplementedError("evaluate_differentiable: transform 'mixed_state' rounds its float64 results to float32 and has no "
                                  "backward pass; differentiate under 'mixed_family' or 'auto'")
    if element_gradients not in ("auto", "kernel"):
        raise InvalidParameterError(f"element_gradients must be 'auto' or 'kernel' (got {element_gradients!r})")
    if element_gradients == "auto" and isinstance(transform, (str, Mapping)) and (transform if isinstance(transform, str) else transform.get("variant")) == "element_operator":
        raise NotImplementedError("evaluate_differentiable: transform 'element_operator' has no backward pass yet (its u-adjoint is the "
                                  "same kernel with the transposed operator); differentiate under 'auto'")
    if element_gradients == "auto" and isinstance(transform, (str, Mapping)) and (transform if isinstance(transform, str) else transform.get("variant")) == "weighted_element_operator":
        raise NotImplementedError("evaluate_differentiable: transform 'weighted_element_operator' has no backward pass yet (its "
                                  "u-adjoint is the same kernel with P and A exchanged and transposed); differentiate under 'auto'")
    if _FN is None:
        _FN = _function()
    q = _as_queue(cq)
    names = tuple(sorted(einsum.all_args))
    missing = [n for n in names if n not in arg_dict]
    if missing:
        raise InvalidParameterError(f"missing input arrays: {missing}")
    # (element slices, measure.ELEMENT_SLICE_RULE: the adjoint kernels take whole arrays only -- refused up front, before the
    #  forward pass could accept them)
    strided = [n for n in names if hasattr(arg_dict[n], "is_contiguous") and not arg_dict[n].is_contiguous()]
    if strided:
        raise InvalidParameterError(f"evaluate_differentiable: argument '{strided[0]}' must be C-contiguous (the adjoint kernels "
                                    "do not take element slices; differentiate .contiguous() copies)")
    outs = _FN.apply(_Spec(einsum, names, q, transform, schedule, operator_gradients, element_gradients), *[arg_dict[n] for n in names])
    return MappingProxyType(dict(zip(einsum.output_names, outs)))
