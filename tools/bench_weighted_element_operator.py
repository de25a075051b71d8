#!/usr/bin/env python3
"""What the weighted-element-operator kernel gives: 'iq,eq,qj,ej->ei' x b at the sandwiches of the
tetrahedral orders, four forms per case, in ONE process, alternating, timed with HIP events:

  a  the route "auto" takes (unchanged by the kernel's arrival: the generic one-thread-per-entry kernel);
  b  ``transform="contraction"``: a pairwise schedule with E x Nq temporaries;
  c  the three-pass route a caller can chain by hand: ``"element_operator"`` (Nj -> Nq), an in-place ``torch.mul`` per field,
     ``"element_operator"`` (Nq -> Ni), the E x Nq temporaries allocated once;
  d  ``transform="weighted_element_operator"``: fe_weightedop_f64.

Every form is bound once (``measure._bind``), warmed up, then timed in windows of at least ``--window`` seconds (batches of
launches between two events), ``--rounds`` windows per form, the forms taking turns.  A line of
profiles/weighted_element_operator/bench.jsonl holds the per-launch microseconds of every batch, their median and slowest -
fastest, GB/s from the 8 (b (Ni + Nj) + Nq) E bytes the operation needs, and the fraction of the bound max(bytes / 8 TB/s,
matrix-core cycles at the sustained clock) with the name of the bound that applies.  The ratio lines (a / d, b / d, c / d)
carry the spread of both sides.

The tool is one process and stops at the first error.  Run it under a time limit, e.g.

    timeout -k 10 1100 python tools/bench_weighted_element_operator.py && echo done
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

SHAPES = ((35, 56, 35), (20, 35, 20), (10, 20, 10), (4, 10, 4), (20, 56, 35), (35, 56, 20), (35, 35, 35))
SIZES = (100_000, 200_000, 1_000_000)
PEAK_BYTES_PER_S = 8.0e12          # HBM3E of the MI355X (feinsum_amd.device_info)
MFMA_CYCLES = 64                   # v_mfma_f64_16x16x4_f64
SIMDS = 256 * 4
SUSTAINED_HZ = 2.1e9               # the clock the chip holds under this load
SUBS = "iq,eq,qj,ej->ei"


def needed_bytes(Ni, Nq, Nj, E, b):
    return 8 * (b * (Ni + Nj) + Nq) * E


def bound_seconds(Ni, Nq, Nj, E, b):
    """(seconds, name) of the bound that applies: the needed bytes at the HBM peak, or the MFMAs of both products of
    ceil(E / 16) tiles per field spread over every SIMD at the sustained clock."""
    t_bw = needed_bytes(Ni, Nq, Nj, E, b) / PEAK_BYTES_PER_S
    mfmas = (-(-Nq // 16) * -(-Nj // 4) + -(-Ni // 16) * -(-Nq // 4)) * -(-E // 16) * b
    t_mfma = mfmas / SIMDS * MFMA_CYCLES / SUSTAINED_HZ
    return (t_bw, "bandwidth") if t_bw >= t_mfma else (t_mfma, "matrix cores")


def window(torch, launch, batch, seconds):
    """[microseconds per launch] of the batches of one window of at least *seconds*."""
    runs, spent = [], 0.0
    while spent < seconds:
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(batch):
            launch()
        t1.record()
        t1.synchronize()
        ms = t0.elapsed_time(t1)
        runs.append(round(ms * 1e3 / batch, 3))
        spent += ms * 1e-3
    return runs


def three_pass(f, torch, q, arrays, outs, shape, E, b):
    """The hand-chained route: two bound "element_operator" launches around b in-place multiplies; returns the launch."""
    from feinsum_amd.measure import _bind

    Ni, Nq, Nj = shape
    s = q.stream_ptr
    up = f.batched_einsum("ij,ej->ei", [[f.array("A", (Nq, Nj)), f.array(f"u{k}", ("E", Nj))] for k in range(b)])
    down = f.batched_einsum("ij,ej->ei", [[f.array("P", (Ni, Nq)), f.array(f"t{k}", ("E", Nq))] for k in range(b)])
    temps = [torch.empty(E, Nq, dtype=torch.float64, device="cuda") for _ in range(b)]
    first = _bind(up, q, {"A": arrays["A"], **{f"u{k}": arrays[f"u{k}"] for k in range(b)}},
                  dict(zip(up.output_names, temps)), "element_operator")[1]
    second = _bind(down, q, {"P": arrays["P"], **{f"t{k}": temps[k] for k in range(b)}},
                   dict(zip(down.output_names, outs.values())), "element_operator")[1]
    W = arrays["W"]

    def launch():
        first.launch(s)
        for t in temps:
            torch.mul(t, W, out=t)
        second.launch(s)
    return launch


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--shapes", type=lambda s: tuple(int(x) for x in s.split("x")), nargs="+", default=list(SHAPES), metavar="NIxNQxNJ")
    ap.add_argument("--sizes", type=int, nargs="+", default=list(SIZES))
    ap.add_argument("--fields", type=int, nargs="+", default=[1, 4])
    ap.add_argument("--window", type=float, default=1.0, help="seconds per timed window (at least 1 for a figure that is quoted)")
    ap.add_argument("--rounds", type=int, default=2, help="windows per form; the forms take turns")
    ap.add_argument("--forms", default="abcd")
    ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "weighted_element_operator" / "bench.jsonl")
    ns = ap.parse_args()

    import torch

    import feinsum_amd as f
    from feinsum_amd.measure import _bind, launch_kind

    q = f.DeviceQueue(0)
    s = q.stream_ptr
    g = torch.Generator(device="cuda").manual_seed(0)
    rnd = lambda *shape: torch.rand(*shape, generator=g, device="cuda", dtype=torch.float64) * 2 - 1   # noqa: E731
    ns.out.parent.mkdir(parents=True, exist_ok=True)
    with ns.out.open("w") as fh:
        for shape in ns.shapes:
            Ni, Nq, Nj = shape
            for E in ns.sizes:
                for b in ns.fields:
                    expr = f.batched_einsum(SUBS, [[f.array("P", (Ni, Nq)), f.array("W", ("E", Nq)), f.array("A", (Nq, Nj)),
                                                    f.array(f"u{k}", ("E", Nj))] for k in range(b)])
                    arrays = {"P": rnd(Ni, Nq), "W": rnd(E, Nq), "A": rnd(Nq, Nj), **{f"u{k}": rnd(E, Nj) for k in range(b)}}
                    outs = {nm: torch.empty(E, Ni, dtype=torch.float64, device="cuda") for nm in expr.output_names}
                    forms = {}
                    for key, transform in (("a", "auto"), ("b", "contraction"), ("d", "weighted_element_operator")):
                        if key in ns.forms:
                            bound = _bind(expr, q, arrays, outs, transform)[1]
                            forms[key] = (lambda bd=bound: bd.launch(s), launch_kind(expr, transform, {"E": E}))
                    if "c" in ns.forms:
                        forms["c"] = (three_pass(f, torch, q, arrays, outs, shape, E, b), "element_operator, torch.mul, element_operator")
                    forms = {k: forms[k] for k in sorted(forms)}
                    runs = {k: [] for k in forms}
                    batch = {}
                    for k, (launch, _) in forms.items():            # warm-up, and the batch size of about 50 ms
                        for _ in range(3):
                            launch()
                        torch.cuda.synchronize()
                        us = window(torch, launch, 5, 1e-9)[0]
                        batch[k] = max(5, min(400, int(50_000 / max(us, 1.0))))
                    for _ in range(ns.rounds):
                        for k, (launch, _) in forms.items():
                            runs[k] += window(torch, launch, batch[k], ns.window)
                    t_bound, which = bound_seconds(Ni, Nq, Nj, E, b)
                    nbytes = needed_bytes(Ni, Nq, Nj, E, b)
                    lines = {}
                    for k, (_, route) in forms.items():
                        med = statistics.median(runs[k])
                        lines[k] = {"Ni": Ni, "Nq": Nq, "Nj": Nj, "E": E, "b": b, "form": k, "route": route,
                                    "median_us": round(med, 3), "fastest_us": min(runs[k]), "slowest_us": max(runs[k]),
                                    "spread_us": round(max(runs[k]) - min(runs[k]), 3),
                                    "GBps": round(nbytes / med * 1e-3, 1), "bound": which, "bound_us": round(t_bound * 1e6, 3),
                                    "fraction_of_bound": round(t_bound * 1e6 / med, 4), "batches": len(runs[k]), "runs_us": runs[k]}
                        fh.write(json.dumps(lines[k]) + "\n")
                    fh.flush()
                    d = lines.get("d")
                    brief = " ".join(f"{k} {ln['median_us']:9.1f} us (+-{ln['spread_us'] / 2:.1f})" for k, ln in lines.items())
                    ratios = ""
                    if d:
                        for k in ("a", "b", "c"):
                            if k in lines:
                                ratio = {"Ni": Ni, "Nq": Nq, "Nj": Nj, "E": E, "b": b, "ratio": f"{k}/d",
                                         "median": round(lines[k]["median_us"] / d["median_us"], 3),
                                         "low": round(lines[k]["fastest_us"] / d["slowest_us"], 3),
                                         "high": round(lines[k]["slowest_us"] / d["fastest_us"], 3)}
                                fh.write(json.dumps(ratio) + "\n")
                                ratios += f"  {k}/d {ratio['median']} [{ratio['low']}, {ratio['high']}]"
                        ratios += f"  d: {d['GBps']} GB/s, {d['fraction_of_bound']} of the {which} bound"
                    print(f"({Ni},{Nq},{Nj}) E={E} b={b}: {brief}{ratios}", flush=True)
                    del forms, arrays, outs
                    torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
