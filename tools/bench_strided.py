#!/usr/bin/env python3
"""What a launch on element slices costs: p = 4 grad, div and face-mass x 4 at n = 1e5 and 1e6,
three variants per case, written to profiles/strided/bench_strided.jsonl:

  A  the contiguous launch of n elements by the PARENT commit's library, in a process of its own that imports the parent's
     tree (``--parent-tree``: a checkout of the parent commit with its library built); once as the launcher decides and
     once forced to the static walk (fe_set_tail_rounds(-1));
  B  the strided launch: every operand with an element axis sliced out of a base of 2 n elements at an odd offset;
  C  what callers did before: copies of the sliced operands into dense arrays, the contiguous launch, copy_ of the result
     into the output slice (the dense temporaries are allocated once: the best case of that route).

Outputs come from the split allocator, as in ``timeit``.  The variants alternate: every round starts the A process, then
times B and C in this one.  A line holds the per-launch microseconds of every batch and their median.  Not symmetric: A's
batches are the C loop ``fe_time_launches``, B's and C's a Python loop between two events (B builds two ctypes pointer tables
per launch); ``--decompose`` times both sides through the same Python loop.

``--decompose`` (this tree only, written to profiles/strided/decomposition.jsonl): where B - A arises.  Per case, on ONE set
of dense arrays: the contiguous launch as the launcher decides; forced to the static walk (``fe_set_tail_rounds(-1)``); static
with the optional forms the strided kernels lack switched off (``fe_set_grad_quarter_tail(0)``,
``fe_set_grad_staggered_start(0)``, ``fe_set_div_quarter_tail(0)``, ``fe_set_div_interleave(0)``,
``fe_set_write_through_mib(0)``); the same forms off under the launcher's walk; and the strided entry point on the same arrays
(every ld = n), as the launcher decides and static.

    python tools/bench_strided.py --parent-tree ../parent [--rounds 3] [--sizes 100000 1000000]
    python tools/bench_strided.py --decompose
"""
from __future__ import annotations

import argparse
import json
import statistics
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
NP, NF, NFP = 35, 4, 15
BATCH, BATCHES = 40, 5


def einsums(f):
    J, D = f.array("J", (3, 3, "E")), f.array("D", (3, NP, NP))
    return {
        "grad": f.einsum("xre,rij,ej->xei", J, D, f.array("u", ("E", NP))),
        "div": f.einsum("xre,rij,xej->ei", J, D, f.array("u", (3, "E", NP))),
        "facemass_x4": f.batched_einsum("fe,fij,fej->ei", [[f.array("Jf", (NF, "E")), f.array("R", (NF, NP, NFP)),
                                                            f.array(f"v{k}", (NF, "E", NFP))] for k in range(4)]),
    }


def element_axis(f, shape):
    return next((k for k, d in enumerate(shape) if isinstance(d, f.SizeParam)), None)


def time_runs(torch, launch_batch, n):
    """[microseconds per launch] of BATCHES batches, after one untimed batch; a batch is BATCH launches at n = 1e6 and
    proportionally more at smaller sizes, so that every batch times several milliseconds of device work."""
    batch = max(BATCH, BATCH * 1_000_000 // n)
    launch_batch(batch)             # warm-up: one whole batch, so that the spread of the timed ones is run-to-run noise
    torch.cuda.synchronize()
    return [round(launch_batch(batch) / batch * 1e6, 3) for _ in range(BATCHES)]


def out_arrays(torch, f, expr, n, q, shape_of=None):
    """Outputs in the placement ``timeit`` uses: the split allocator (plain allocations where it cannot serve)."""
    from feinsum_amd import placement

    shape = [n if isinstance(d, f.SizeParam) else int(d) for d in expr.shape]
    shape = shape_of(shape) if shape_of else shape
    outs = {}
    for name in expr.output_names:
        try:
            outs[name] = placement.zeros(tuple(shape), torch.float64, q.torch_device)
        except Exception:   # noqa: BLE001
            outs[name] = torch.zeros(shape, dtype=torch.float64, device=q.torch_device)
    return outs


def contiguous_variant(sizes):
    """Variant A: runs in the tree on sys.path[0] (the parent's)."""
    import torch

    import feinsum_amd as f
    from feinsum_amd import _hip
    from feinsum_amd.measure import _bind, generate_input_arrays

    q = f.DeviceQueue(0)
    for name, expr in einsums(f).items():
        for n in sizes:
            args = generate_input_arrays(q, expr, n)
            outs = out_arrays(torch, f, expr, n, q)
            _, bound, _ = _bind(expr, q, args, outs, None)
            for walk, rounds in (("launcher's choice", None), ("static", -1)):
                prev = _hip.set_tail_rounds(rounds) if rounds is not None else None
                runs = time_runs(torch, lambda k: bound.time_batch(k, q.stream_ptr), n)
                bound.launch(q.stream_ptr)
                torch.cuda.synchronize()
                info = _hip.last_launch_info()
                if prev is not None:
                    _hip.set_tail_rounds(prev)
                print(json.dumps({"case": name, "n": n, "variant": "A", "walk": walk, "dynamic_walk": bool(info.get("dynamic_walk")),
                                  "runs_us": runs}), flush=True)
            del args, outs, bound
            torch.cuda.empty_cache()


def sliced_variants(sizes):
    """Variants B and C, in this tree."""
    import torch

    import feinsum_amd as f
    from feinsum_amd import _hip
    from feinsum_amd.measure import _bind, generate_input_arrays

    q = f.DeviceQueue(0)
    lines = []
    for name, expr in einsums(f).items():
        for n in sizes:
            a = 1 + 2 * (n // 3 // 2)            # an odd offset inside a base of 2 n elements
            dense = dict(generate_input_arrays(q, expr, n))
            views = {}
            for k, t in dense.items():
                axis = element_axis(f, expr.arg_to_shape[k])
                if axis is None:
                    views[k] = t
                    continue
                base = torch.zeros([2 * n if d == axis else s for d, s in enumerate(t.shape)], dtype=t.dtype, device=t.device)
                views[k] = base.narrow(axis, a, n)
                views[k].copy_(t)
            oaxis = element_axis(f, expr.shape)
            obases = out_arrays(torch, f, expr, n, q, lambda shape: [2 * n if d == oaxis else s for d, s in enumerate(shape)])
            oviews = {o: t.narrow(oaxis, a, n) for o, t in obases.items()}
            dense_out = out_arrays(torch, f, expr, n, q)
            _, strided, _ = _bind(expr, q, views, oviews, None)
            _, contiguous, _ = _bind(expr, q, dense, dense_out, None)
            copied = [k for k, v in views.items() if not v.is_contiguous()]

            def old_route(stream_ptr):
                for k in copied:
                    dense[k].copy_(views[k])
                contiguous.launch(stream_ptr)
                for o in oviews:
                    oviews[o].copy_(dense_out[o])

            runs_b = time_runs(torch, lambda k: strided.time_batch(k, q.stream_ptr), n)
            strided.launch(q.stream_ptr)
            torch.cuda.synchronize()
            info = _hip.last_launch_info()
            runs_c = time_runs(torch, lambda k: _hip.time_with_events(old_route, k, q.stream_ptr), n)
            same = all(torch.equal(oviews[o].contiguous().view(torch.int64), dense_out[o].view(torch.int64)) for o in oviews)
            lines.append({"case": name, "n": n, "variant": "B", "walk": "launcher's choice", "dynamic_walk": bool(info.get("dynamic_walk")),
                          "element_slice": bool(info.get("element_slice")),
                          "offset": a, "ld": 2 * n, "runs_us": runs_b})
            lines.append({"case": name, "n": n, "variant": "C", "copied_operands": copied, "bitwise_equal_to_B": same, "runs_us": runs_c})
            del dense, views, obases, oviews, dense_out, strided, contiguous
            torch.cuda.empty_cache()
    return lines


def decompose(sizes, rounds):
    """See the module docstring; returns the lines."""
    import torch

    import feinsum_amd as f
    from feinsum_amd import _hip
    from feinsum_amd.measure import _bind, generate_input_arrays

    q = f.DeviceQueue(0)
    knobs = [(_hip.set_grad_quarter_tail, False), (_hip.set_grad_staggered_start, False), (_hip.set_div_quarter_tail, False),
             (_hip.set_div_interleave, 0), (_hip.set_write_through_mib, 0)]
    merged: dict = {}
    for _ in range(rounds):
        for name, expr in einsums(f).items():
            for n in sizes:
                dense = dict(generate_input_arrays(q, expr, n))
                outs = out_arrays(torch, f, expr, n, q)
                _, bound, _ = _bind(expr, q, dense, outs, None)
                plan = f.match_family(expr)
                J, A = (dense[a.name].data_ptr() for a in expr.args[0][:2])
                fields = [dense[row[2].name].data_ptr() for row in expr.args]
                optrs = [outs[o].data_ptr() for o in expr.output_names]
                if name == "grad":
                    strided = lambda s: _hip.grad3d_strided(J, n, A, fields, optrs, n, n, NP, plan.layout_flags, stream=s)   # noqa: E731
                elif name == "div":
                    strided = lambda s: _hip.div3d_strided(J, n, A, fields, n, optrs, n, NP, plan.layout_flags, stream=s)   # noqa: E731
                else:
                    strided = lambda s: _hip.facemass_strided(J, n, A, fields, n, optrs, n, NP, NF, NFP, plan.layout_flags, stream=s)   # noqa: E731
                dense_loop = lambda k: _hip.time_with_events(bound.launch, k, q.stream_ptr)   # noqa: E731
                strided_loop = lambda k: _hip.time_with_events(strided, k, q.stream_ptr)   # noqa: E731

                def note(what, loop):
                    loop(1)
                    info = _hip.last_launch_info()
                    key = (name, n, what)
                    merged.setdefault(key, {"case": name, "n": n, "what": what, "dynamic_walk": bool(info.get("dynamic_walk")),
                                            "runs_us": []})["runs_us"] += time_runs(torch, loop, n)

                note("A, launcher's walk", dense_loop)
                note("B with ld = n, launcher's walk", strided_loop)
                olds = [fn(v) for fn, v in knobs]
                note("A, launcher's walk, optional forms off", dense_loop)
                prev = _hip.set_tail_rounds(-1)
                note("A, static walk, optional forms off", dense_loop)
                for (fn, _v), old in zip(knobs, olds):
                    fn(old)
                note("A, static walk", dense_loop)
                note("B with ld = n, static walk", strided_loop)
                _hip.set_tail_rounds(prev)
                del dense, outs, bound
                torch.cuda.empty_cache()
    return list(merged.values())


def write_lines(lines, path, rounds):
    path.parent.mkdir(parents=True, exist_ok=True)
    with path.open("w") as fh:
        for ln in lines:
            ln["median_us"] = round(statistics.median(ln["runs_us"]), 3)
            ln["spread_us"] = round(max(ln["runs_us"]) - min(ln["runs_us"]), 3)
            ln["rounds"] = rounds
            fh.write(json.dumps(ln) + "\n")
            print(json.dumps({k: v for k, v in ln.items() if k != "runs_us"}))


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--parent-tree", type=Path, help="checkout of the parent commit with its library built (variant A)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--sizes", type=int, nargs="+", default=[100_000, 1_000_000])
    ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "strided" / "bench_strided.jsonl")
    ap.add_argument("--decompose", action="store_true", help="where B - A arises (see the module docstring)")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ns = ap.parse_args()
    if ns.decompose:
        sys.path.insert(0, str(ROOT))
        out = ns.out if ns.out.name != "bench_strided.jsonl" else ns.out.with_name("decomposition.jsonl")
        write_lines(decompose(ns.sizes, ns.rounds), out, ns.rounds)
        return 0
    if ns.child:       # variant A: the tree to import is the first entry of sys.path (set by the parent process)
        contiguous_variant(ns.sizes)
        return 0
    sys.path.insert(0, str(ROOT))
    merged: dict = {}
    for r in range(ns.rounds):
        lines = []
        if ns.parent_tree is not None:
            child = subprocess.run([sys.executable, "-c",
                                    "import sys; sys.path.insert(0, sys.argv[1]); sys.argv = sys.argv[2:]; "
                                    "import runpy; runpy.run_path(sys.argv[0], run_name='__main__')",
                                    str(ns.parent_tree.resolve()), str(Path(__file__).resolve()), "--child", "--sizes",
                                    *map(str, ns.sizes)], capture_output=True, text=True, timeout=600)
            if child.returncode != 0:
                print(child.stderr[-2000:], file=sys.stderr)
                return 1
            lines += [json.loads(ln) for ln in child.stdout.splitlines() if ln.startswith("{")]
        lines += sliced_variants(ns.sizes)
        for ln in lines:
            key = (ln["case"], ln["n"], ln["variant"], ln.get("walk"))
            if key in merged:
                merged[key]["runs_us"] += ln["runs_us"]
            else:
                merged[key] = ln
    write_lines(list(merged.values()), ns.out, ns.rounds)
    return 0


if __name__ == "__main__":
    sys.exit(main())
