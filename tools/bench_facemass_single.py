#!/usr/bin/env python3
"""What the single-field face-mass kernel gives: 'ef,fij,fej->ei' of ONE field for tetrahedra p = 1..4,
triangles p = 4 and tetrahedra p = 5 at E = 1e5 and 1e6, three variants per case, written to
profiles/facemass_single/bench_facemass_single.jsonl:

  A  the PARENT commit's library under "auto" (the tiled VALU kernel; below ten rows the one-thread-per-entry kernel): what a
     caller got before, in a process of its own that imports the parent's tree (``--parent-tree``: a checkout of the parent
     commit with its library built);
  B  this tree under "auto";
  C  this tree's launch of TWO fields with the field duplicated -- the workaround that reached the matrix cores before --
     per launch (it writes two outputs).

A, B and C run through the same code (the ``--child`` mode of this file: ``_bind`` and the bound launch's ``time_batch``), in
turn: every round starts the A process, then the process of B and C.  Each timed series of BATCHES batches follows one untimed
batch.  A line holds the per-launch microseconds of every batch of every round, their median and slowest - fastest, the
fraction of the HBM roofline (``get_roofline_flop_rate`` of the ONE-field einsum, also for C) at the median, and what
``fe_last_launch_info`` says about the walk and the loads.

    python tools/bench_facemass_single.py --parent-tree ../parent [--rounds 3] [--sizes 100000 1000000]
"""
from __future__ import annotations

import argparse
import json
import statistics
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
#: (name, Np, nf, Nfp)
CASES = (("tet p1", 4, 4, 3), ("tet p2", 10, 4, 6), ("tet p3", 20, 4, 10), ("tet p4", 35, 4, 15), ("tri p4", 15, 3, 5),
         ("tet p5", 56, 4, 21))
BATCH, BATCHES = 40, 5
DEVICE = "AMD Instinct MI355X"


def lift(f, Np, nf, Nfp, fields):
    """'ef,fij,fej->ei' x len(fields)."""
    return f.batched_einsum("ef,fij,fej->ei", [[f.array("J", ("E", nf)), f.array("R", (nf, Np, Nfp)), f.array(v, (nf, "E", Nfp))]
                                               for v in fields])


def time_runs(torch, launch_batch, n):
    """[microseconds per launch] of BATCHES batches, after one untimed batch (tools/bench_strided.py)."""
    batch = max(BATCH, BATCH * 1_000_000 // n)
    launch_batch(batch)
    torch.cuda.synchronize()
    return [round(launch_batch(batch) / batch * 1e6, 3) for _ in range(BATCHES)]


def child(sizes, variants):
    """Runs in the tree on sys.path[0]."""
    import numpy as np
    import torch

    import feinsum_amd as f
    from feinsum_amd import _hip
    from feinsum_amd.measure import _bind, generate_input_arrays

    q = f.DeviceQueue(0)
    for name, Np, nf, Nfp in CASES:
        one = lift(f, Np, nf, Nfp, ["v0"])
        for n in sizes:
            args = dict(generate_input_arrays(q, one, n))
            gops = f.count_ops(one, long_dim_length=n) * 1e-9
            roof = f.get_roofline_flop_rate(one, DEVICE, n)[np.dtype("float64")]
            for variant in variants:
                expr = lift(f, Np, nf, Nfp, ["v0", "v1"]) if variant == "C" else one
                args["v1"] = args["v0"]          # the duplicated field: the same array under a second name
                outs = {o: torch.zeros((n, Np), dtype=torch.float64, device=q.torch_device) for o in expr.output_names}
                _, bound, _ = _bind(expr, q, args, outs, "auto")
                runs = time_runs(torch, lambda k: bound.time_batch(k, q.stream_ptr), n)
                bound.launch(q.stream_ptr)
                torch.cuda.synchronize()
                info = _hip.last_launch_info()
                print(json.dumps({"case": name, "Np": Np, "nf": nf, "Nfp": Nfp, "n": n, "variant": variant,
                                  "matrix_cores": bool(info.get("valid")), "walk": "dynamic" if info.get("dynamic_walk") else "static",
                                  "loads": "temporal" if info.get("temporal_loads") else "non-temporal",
                                  "roofline_gflops": round(roof, 1), "gops": gops, "runs_us": runs}), flush=True)
                del outs, bound
            del args
            torch.cuda.empty_cache()


def run_child(tree: Path, sizes, variants):
    res = subprocess.run([sys.executable, "-c",
                          "import sys; sys.path.insert(0, sys.argv[1]); sys.argv = sys.argv[2:]; "
                          "import runpy; runpy.run_path(sys.argv[0], run_name='__main__')",
                          str(tree.resolve()), str(Path(__file__).resolve()), "--child", "".join(variants), "--sizes",
                          *map(str, sizes)], capture_output=True, text=True, timeout=900)
    if res.returncode != 0:
        print(res.stderr[-2000:], file=sys.stderr)
        raise SystemExit(1)
    return [json.loads(ln) for ln in res.stdout.splitlines() if ln.startswith("{")]


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--parent-tree", type=Path, help="checkout of the parent commit with its library built (variant A)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--sizes", type=int, nargs="+", default=[100_000, 1_000_000])
    ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "facemass_single" / "bench_facemass_single.jsonl")
    ap.add_argument("--child", metavar="VARIANTS", help=argparse.SUPPRESS)
    ns = ap.parse_args()
    if ns.child:       # the tree to import is the first entry of sys.path (set by the parent process)
        child(ns.sizes, list(ns.child))
        return 0
    merged: dict = {}
    for _ in range(ns.rounds):
        lines = run_child(ns.parent_tree, ns.sizes, ["A"]) if ns.parent_tree is not None else []
        lines += run_child(ROOT, ns.sizes, ["B", "C"])
        for ln in lines:
            key = (ln["case"], ln["n"], ln["variant"])
            if key in merged:
                merged[key]["runs_us"] += ln["runs_us"]
            else:
                merged[key] = ln
    ns.out.parent.mkdir(parents=True, exist_ok=True)
    with ns.out.open("w") as fh:
        for ln in merged.values():
            ln["median_us"] = round(statistics.median(ln["runs_us"]), 3)
            ln["fastest_us"], ln["slowest_us"] = min(ln["runs_us"]), max(ln["runs_us"])
            ln["spread_us"] = round(ln["slowest_us"] - ln["fastest_us"], 3)
            ln["roofline_fraction"] = round(ln.pop("gops") / (ln["median_us"] * 1e-6) / ln["roofline_gflops"], 4)
            ln["rounds"] = ns.rounds
            fh.write(json.dumps(ln) + "\n")
            print(json.dumps({k: v for k, v in ln.items() if k != "runs_us"}))
    # the rule of DESIGN.md section 3p: "auto" may pick the new kernel only where B's median is below A's fastest run
    for (case, n, variant), b in merged.items():
        a = merged.get((case, n, "A"))
        if variant == "B" and a is not None:
            print(f"{case} n={n}: B median {b['median_us']} us, A fastest {a['fastest_us']} us -> "
                  f"{'B below A' if b['median_us'] < a['fastest_us'] else 'B NOT below A'}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
