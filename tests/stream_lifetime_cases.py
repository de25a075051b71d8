"""Helpers of tests/test_gpu_stream_lifetime.py (a plain module, not a conftest): the PATHS through the public API whose
arrays the library allocates itself, each with exact data (``m * 2**s``) and the int64 einsum of oracle/einsum_ref.py
as the expected value, and the helper that holds a stream busy.

Data and references come from what the fuzz tools provide (tools/fuzz_dg.py ``DGCase`` / ``host_data``,
tools/fuzz_einsum.py ``Case`` / ``exact_data``, tools/fuzz_autograd.py ``AGCase`` / ``host_data`` /
``host_references``); every reference array is ``einsum_ref.int_reference`` / ``exact_reference`` of the whole array
on the host -- never a run of the code under test."""

from __future__ import annotations

import math
import sys
import time
from dataclasses import replace
from pathlib import Path as _FsPath
from typing import Any, Callable, Dict, List, Optional, Sequence

import numpy as np

sys.path.insert(0, str(_FsPath(__file__).resolve().parents[1] / "tools"))
import fuzz_autograd as AGF  # noqa: E402
import fuzz_dg as D  # noqa: E402
import fuzz_einsum as FE  # noqa: E402

import feinsum_amd as f  # noqa: E402
from feinsum_amd import autograd as AG  # noqa: E402
from feinsum_amd.family import match_adjoint_family  # noqa: E402
from oracle import einsum_ref as ref_  # noqa: E402

SENTINEL = -7.25          # (exact in float32 and float64; no exact-data result of these cases is -7.25 everywhere)
MIN_HOLD_S = 0.05
E_SPLIT_GRAD = 12_000     # grad p=4: 3 x 12 000 x 35 x 8 B = 10.08 MB >= 8 MiB: the output is the split allocator's
E_SPLIT_FM = 30_011       # face-mass: 30 011 x 35 x 8 B = 8.4 MB per output, ragged
E_SMALL = 1003            # 62 tiles and 11 elements behind them: torch's allocator
E_MID = 4099


class LibraryPath:
    """One way through the public API that makes the library allocate: ``run(q, i)`` evaluates data set *i* (0 or 1)
    asynchronously on queue *q* and returns the library-allocated result tensors, ``refs(i)`` the oracle's arrays in the
    same order (device tensors).  ``expr`` / ``args(i)`` / ``transform``: the single ``evaluate`` behind ``run`` where
    there is one (scenarios (d) and (e))."""

    def __init__(self, name: str, run: Callable[[Any, int], List[Any]], refs: Callable[[int], List[Any]], *,
                 expr: Any = None, args: Optional[Callable[[int], Dict[str, Any]]] = None, transform: Any = None,
                 E: int = 0, prepared: bool = False, droppable: bool = True) -> None:
        self.name, self.run, self.refs = name, run, refs
        self.expr, self.args, self.transform, self.E = expr, args, transform, E
        self.prepared, self.droppable = prepared, droppable


#: every path by name, in the order of the issue's list (static: the module collects without a GPU)
PATH_NAMES = ("grad_split", "grad_separate", "grad_ragged", "facemass4", "grad_f32", "div_mixed",
              "prepared_grad", "prepared_div", "prepared_facemass", "pipeline", "generic", "contraction3",
              "reduction", "adjoint", "differentiable")
PREPARED = ("prepared_grad", "prepared_div", "prepared_facemass")
#: paths that are one ``evaluate(expr, q, args)``: scenario (e) hands them ``generate_out_arrays`` outputs
SINGLE = tuple(n for n in PATH_NAMES if n not in ("pipeline", "differentiable"))

_DG = {
    "grad_split": (D.DGCase("grad", 35, 15, 1, "rij", "float64", E_SPLIT_GRAD, "large", 101), None),
    "grad_separate": (D.DGCase("grad", 35, 15, 1, "rij", "float64", E_SPLIT_GRAD, "large", 101), {"placement": "separate"}),
    "grad_ragged": (D.DGCase("grad", 35, 15, 1, "rij", "float64", E_SMALL, "ragged", 103), None),
    "facemass4": (D.DGCase("fm", 35, 15, 4, "rij", "float64", E_SPLIT_FM, "large", 105), None),
    "grad_f32": (D.DGCase("grad", 35, 15, 1, "rij", "float32", E_MID, "ragged", 107), None),
    "div_mixed": (D.DGCase("div", 35, 15, 1, "rij", "mixed", E_MID, "ragged", 109), None),
    "prepared_grad": (D.DGCase("grad", 35, 15, 1, "rij", "float64", E_MID, "ragged", 111), {"prepared": True}),
    "prepared_div": (D.DGCase("div", 35, 15, 1, "rij", "float64", E_MID, "ragged", 113), {"prepared": True}),
    "prepared_facemass": (D.DGCase("fm", 35, 15, 4, "rij", "float64", E_MID, "ragged", 115), {"prepared": True}),
    "pipeline": (D.DGCase("pipeline", 35, 15, 4, "rij", "float64", E_MID, "ragged", 117, "normal", True), None),
}
_EINSUM = {
    "generic": (FE.Case("ei,ei->e", (("E", 7), ("E", 7)), ("float64", "float64"), E_MID, seed=121), "generic"),
    "contraction3": (FE.Case("ei,ij,jk->ek", (("E", 16), (16, 17), (17, 8)), ("float64",) * 3, E_MID, seed=123), "contraction"),
    "reduction": (FE.Case("ei,ej->ij", (("E", 33), ("E", 17)), ("float64", "float64"), 5003, seed=125), "reduction"),
}
_AG_CASE = D.DGCase("grad", 35, 15, 1, "rij", "float64", E_SMALL, "ragged", 127)

_cache: Dict[Any, Any] = {}


def _dev(torch, arrays: Dict[str, np.ndarray]) -> Dict[str, Any]:
    return {k: torch.from_numpy(np.ascontiguousarray(a)).cuda() for k, a in arrays.items()}


def dg_data(torch, case: D.DGCase, i: int):
    """``(device arrays by key, [[reference per output] per stage])`` of data set *i* of a DG case: the references
    are the int64 einsums of the mantissas of the whole arrays."""
    case = replace(case, seed=case.seed + 1000 * i)
    key = ("dg", case)
    if key not in _cache:
        arrays, mants, scales, sig = D.host_data(case)
        out_dt = np.dtype("float32") if case.dtype == "float32" else np.dtype("float64")
        refs = []
        for expr, keys in case.stages():
            per = []
            for row in expr.args:
                ks = [keys[a.name] for a in row]
                host = ref_.int_reference(expr.get_subscripts(), [mants[k] for k in ks], sum(scales[k] for k in ks), out_dt, sig)
                per.append(torch.from_numpy(host).cuda())
            refs.append(per)
        _cache[key] = (_dev(torch, arrays), refs)
    return _cache[key]


def _dg_path(torch, name: str) -> LibraryPath:
    case, transform = _DG[name]
    stages = case.stages()

    def staged(i):
        dev, _ = dg_data(torch, case, i)
        return [(expr, {nm: dev[k] for nm, k in keys.items()}) for expr, keys in stages]

    def refs(i):
        return [r for per in dg_data(torch, case, i)[1] for r in per]

    if case.kind == "pipeline":
        def run(q, i):
            outs = f.evaluate_operator(staged(i), q, fuse=case.fuse)
            return [od[n] for (expr, _), od in zip(stages, outs) for n in expr.output_names]

        return LibraryPath(name, run, refs, E=case.E)
    expr = stages[0][0]

    def run(q, i):
        outs = f.evaluate(expr, q, staged(i)[0][1], transform=transform)
        return [outs[n] for n in expr.output_names]

    return LibraryPath(name, run, refs, expr=expr, args=lambda i: staged(i)[0][1], transform=transform, E=case.E,
                       prepared=name in PREPARED)


def _einsum_path(torch, name: str) -> LibraryPath:
    case0, transform = _EINSUM[name]
    expr = case0.expr()

    def data(i):
        case = replace(case0, seed=case0.seed + 1000 * i)
        key = ("einsum", case)
        if key not in _cache:
            arrays, ref, _ = FE.exact_data(case)
            _cache[key] = ({f"A{k}": torch.from_numpy(np.array(a, order="C")).cuda() for k, a in enumerate(arrays)},
                           [torch.from_numpy(np.ascontiguousarray(ref)).cuda()])
        return _cache[key]

    def run(q, i):
        return [f.evaluate(expr, q, data(i)[0], transform=transform)["_fe_out"]]

    return LibraryPath(name, run, lambda i: data(i)[1], expr=expr, args=lambda i: data(i)[0], transform=transform, E=case0.E)


def _ag_data(torch, i: int):
    case = AGF.AGCase(replace(_AG_CASE, seed=_AG_CASE.seed + 1000 * i), None, "auto")
    key = ("ag", case)
    if key not in _cache:
        arrays, mants, scales = AGF.host_data(case)
        fwd, grads = AGF.host_references(case, mants, scales)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()   # noqa: E731
        _cache[key] = (case, _dev(torch, arrays), {n: up(a) for n, a in fwd.items()}, {n: up(a) for n, a in grads.items()})
    return _cache[key]


def _adjoint_path(torch) -> LibraryPath:
    """grad's geometric-factor adjoint (dJ) under ``transform="adjoint"``: the one adjoint term of J, its expected
    value the oracle's exact gradient of J."""
    expr = _ag_data(torch, 0)[0].expr()
    term = AG.adjoint_terms(expr, "J")[0].einsum
    assert match_adjoint_family(term) is not None and tuple(term.shape) == tuple(expr.arg_to_shape["J"])

    def args(i):
        dev = _ag_data(torch, i)[1]
        return {n: dev[n] for n in term.all_args}

    def run(q, i):
        return [f.evaluate(term, q, args(i), transform="adjoint")["_fe_out"]]

    return LibraryPath("adjoint", run, lambda i: [_ag_data(torch, i)[3]["J"]], expr=term, args=args, transform="adjoint",
                       E=_AG_CASE.E)


def _differentiable_path(torch) -> LibraryPath:
    """``evaluate_differentiable`` forward and backward, every input requiring grad: the outputs, then the gradients in
    sorted-name order."""
    expr = _ag_data(torch, 0)[0].expr()
    names = sorted(expr.all_args)

    def run(q, i):
        _, dev, _, _ = _ag_data(torch, i)
        leaves = {n: dev[n].detach().requires_grad_(True) for n in names}
        outs = f.evaluate_differentiable(expr, q, leaves)
        torch.autograd.backward([outs[n] for n in expr.output_names],
                                [dev[AG.output_grad_name(n)] for n in expr.output_names])
        return [outs[n].detach() for n in expr.output_names] + [leaves[n].grad for n in names]

    def refs(i):
        _, _, fwd, grads = _ag_data(torch, i)
        return [fwd[n] for n in expr.output_names] + [grads[n] for n in names]

    return LibraryPath("differentiable", run, refs, E=_AG_CASE.E, droppable=False)


def get_path(torch, name: str) -> LibraryPath:
    if ("path", name) not in _cache:
        _cache[("path", name)] = (_dg_path(torch, name) if name in _DG else _einsum_path(torch, name) if name in _EINSUM
                                  else _adjoint_path(torch) if name == "adjoint" else _differentiable_path(torch))
    return _cache[("path", name)]


def clear() -> None:
    _cache.clear()
    _filler.clear()


def mismatches(got: Sequence[Any], refs: Sequence[Any]) -> List[str]:
    """One line per result that is not bitwise the oracle's (``einsum_ref.differing_entries``)."""
    bad = []
    if len(got) != len(refs):
        return [f"{len(got)} results, {len(refs)} references"]
    for k, (g, r) in enumerate(zip(got, refs)):
        n = ref_.differing_entries(g, r)
        if n:
            zeros = int((g == 0).sum()) if tuple(g.shape) == tuple(r.shape) else -1
            bad.append(f"result {k}: {n} of {r.numel()} entries differ from the int64 einsum ({zeros} entries are zero)")
    return bad


# --------------------------------------------------------------------------
# holding a stream busy
# --------------------------------------------------------------------------

_filler: Dict[str, Any] = {}


def _sleep_cycles_per_second(torch) -> float:
    """``torch.cuda._sleep`` counts device clock ticks: measured once, with events, on a stream of its own."""
    if "rate" not in _filler:
        s = torch.cuda.Stream()
        n = 20_000_000
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(s):
            torch.cuda._sleep(1000)
            t0.record(s)
            torch.cuda._sleep(n)
            t1.record(s)
        t1.synchronize()
        _filler["rate"] = n / max(t0.elapsed_time(t1) * 1e-3, 1e-6)
    return _filler["rate"]


def _grad_filler(torch):
    """Without ``torch.cuda._sleep``: the library's own grad at E = 10^6 into caller-allocated outputs, and its time."""
    if "grad" not in _filler:
        import dg
        from feinsum_amd import measure

        expr, E = dg.grad(), 1_000_000
        dev = measure.generate_input_arrays(0, expr, E)
        outs = measure.generate_out_arrays(0, expr, E)
        _, bound, _ = measure._bind(expr, 0, dev, outs, None)
        torch.cuda.synchronize()
        s = torch.cuda.Stream()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        bound.launch(int(s.cuda_stream))
        t0.record(s)
        bound.launch(int(s.cuda_stream))
        t1.record(s)
        t1.synchronize()
        _filler["grad"] = (bound, max(t0.elapsed_time(t1) * 1e-3, 1e-5))
    return _filler["grad"]


def hold(torch, stream, seconds: float):
    """Enqueue about *seconds* of filler work on *stream*; returns an event recorded behind it."""
    if hasattr(torch.cuda, "_sleep"):
        cycles = int(seconds * _sleep_cycles_per_second(torch))
        with torch.cuda.stream(stream):
            torch.cuda._sleep(cycles)
    else:
        bound, each = _grad_filler(torch)
        with torch.cuda.device(0):
            for _ in range(int(math.ceil(seconds / each))):
                bound.launch(int(stream.cuda_stream))
    ev = torch.cuda.Event()
    ev.record(stream)
    return ev


def still_busy(ev, what: str) -> None:
    """The precondition of every scenario: the filler is unfinished where the hazard would occur.  Fails otherwise."""
    assert not ev.query(), f"precondition not established: the filler finished before {what} -- the scenario proves nothing"


def run_held(torch, body: Callable[[Optional[float]], Any]):
    """Run *body* twice serially (``body(None)``: no filler; first use of allocators, maps and kernels, then a timed
    run), then ``body(seconds)`` with ``seconds`` = ten times the timed run's host time, at least 50 ms.  Returns
    ``(body's result, seconds)``."""
    for _ in range(2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        body(None)
        torch.cuda.synchronize()
        serial = time.perf_counter() - t0
    seconds = max(10.0 * serial, MIN_HOLD_S)
    if hasattr(torch.cuda, "_sleep"):
        _sleep_cycles_per_second(torch)
    else:
        _grad_filler(torch)
    torch.cuda.synchronize()
    return body(seconds), seconds
