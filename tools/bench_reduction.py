"""Split reductions (the "reduction" transform) against the kernels that ran these einsums before -- the generic
kernel and the contraction kernel, at E = 10^5 only, where they are slow but bounded -- and against torch.einsum.  One
JSON line per (einsum, E, form).
    python tools/bench_reduction.py [--reps N] [--quick]

Seconds per launch by HIP events over --reps back-to-back launches after a warm-up launch, float64, Np = 35.
"roofline" is the fraction of 8 TB/s the algorithmic bytes (every input once, the output once) would need.
--quick: E = 10^5 only and fewer repetitions (for a profiler run).
"""
import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import feinsum_amd as f  # noqa: E402
from feinsum_amd import _hip  # noqa: E402
from feinsum_amd.measure import _bind, launch_kind  # noqa: E402

NP = 35
BW = 8e12
TABLE = [
    ("ei,ei->", [("E", NP), ("E", NP)], "generic"),
    ("ej,ej->j", [("E", NP), ("E", NP)], "generic"),
    ("ei,ej->ij", [("E", NP), ("E", NP)], "contraction"),
    ("e,ei,ei->", [("E",), ("E", NP), ("E", NP)], "generic"),
    ("e,ij,ei,ej->", [("E",), (NP, NP), ("E", NP), ("E", NP)], "generic"),
]


def seconds(fn, reps):
    fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) * 1e-3 / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--quick", action="store_true")
    args = ap.parse_args()
    Es = [10**5] if args.quick else [10**5, 10**6]
    gen = torch.Generator(device="cuda").manual_seed(0)
    for subs, shapes, before in TABLE:
        for E in Es:
            expr = f.einsum(subs, *[f.array(n, s) for n, s in zip("ABCD", shapes)])
            dev = {n: torch.rand(tuple(E if d == "E" else d for d in s), dtype=torch.float64, device="cuda",
                                 generator=gen) for n, s in zip("ABCD", shapes)}
            nbytes = sum(t.numel() * 8 for t in dev.values()) + 8 * int(np.prod(
                [NP if c in "ij" else 1 for c in subs.split("->")[1]]))
            forms = [("reduction", "reduction", args.reps)]
            if E == 10**5:   # the kernels of before: one wave / one block walks everything
                forms.append((before, before, 3 if args.quick else 5))
            for form, transform, reps in forms:
                _, bound, _ = _bind(expr, 0, dev, None, transform)
                t = seconds(lambda: bound.launch(0), reps)
                line = {"einsum": subs, "E": E, "form": form, "us": round(t * 1e6, 2),
                        "roofline": round(nbytes / t / BW, 4), "auto": launch_kind(expr, "auto", {"E": E})}
                if form == "reduction":
                    line["launches"] = len(bound.launches)
                print(json.dumps(line), flush=True)
            ops = [dev[n] for n in "ABCD"[:len(shapes)]]
            t = seconds(lambda: torch.einsum(subs, *ops), args.reps)
            print(json.dumps({"einsum": subs, "E": E, "form": "torch.einsum", "us": round(t * 1e6, 2),
                              "roofline": round(nbytes / t / BW, 4)}), flush=True)
    res = _hip.kernel_resources()
    print(json.dumps({"kernel_resources": [ln for ln in res.splitlines() if "reduce" in ln or "split-K" in ln]}))


if __name__ == "__main__":
    main()
