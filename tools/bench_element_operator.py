#!/usr/bin/env python3
"""What the element-operator kernel gives: 'ij,ej->ei' and 'e,ij,ej->ei' x b at rectangular and
untabulated square sizes, three forms per case, in ONE process, alternating, timed with HIP events:

  a  the route "auto" takes (unchanged by the kernel's arrival: the contraction kernel for 'ij,ej->ei', the generic kernel for
     'e,ij,ej->ei', the MATAPPLY family or the tiled kernel for square sizes);
  b  ``torch.einsum`` on the same arrays, an outside witness (one call per field);
  c  ``transform="element_operator"``: fe_elemop_f64.

Every form is bound once (``measure._bind``; torch: a closure), warmed up, then timed in windows of at least ``--window``
seconds (batches of launches between two events), ``--rounds`` windows per form, the forms taking turns.  A line of
profiles/element_operator/bench.jsonl holds the per-launch microseconds of every batch, their median and slowest - fastest,
GB/s from 8 (Ni + Nj [+ 1]) E b bytes, and the fraction of the bound max(bytes / 8 TB/s, matrix-core cycles at the sustained
clock) with the name of the bound that applies.  The ratio lines (a / c, b / c) carry the spread of both sides.

The tool is one process and stops at the first error.  Run it under a time limit, e.g.

    timeout -k 10 1100 python tools/bench_element_operator.py && echo done
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

SHAPES = ((56, 35), (35, 56), (60, 35), (20, 35), (35, 20), (64, 64), (13, 13))
SIZES = (100_000, 200_000, 1_000_000)
PEAK_BYTES_PER_S = 8.0e12          # HBM3E of the MI355X (feinsum_amd.device_info)
MFMA_CYCLES = 64                   # v_mfma_f64_16x16x4_f64
SIMDS = 256 * 4
SUSTAINED_HZ = 2.1e9               # the clock the chip holds under this load


def expression(f, Ni, Nj, b, with_j):
    row = lambda k: ([f.array("J", ("E",))] if with_j else []) + [f.array("A", (Ni, Nj)), f.array(f"u{k}", ("E", Nj))]   # noqa: E731
    return f.batched_einsum("e,ij,ej->ei" if with_j else "ij,ej->ei", [row(k) for k in range(b)])


def bound_seconds(Ni, Nj, E, b, with_j):
    """(seconds, name) of the bound that applies: the bytes at the HBM peak, or the MFMAs of ceil(E / 16) tiles per field
    spread over every SIMD at the sustained clock."""
    t_bw = 8 * (Ni + Nj + (1 if with_j else 0)) * E * b / PEAK_BYTES_PER_S
    mfmas = -(-Ni // 16) * -(-Nj // 4) * -(-E // 16) * b
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


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--shapes", type=lambda s: tuple(int(x) for x in s.split("x")), nargs="+", default=list(SHAPES), metavar="NIxNJ")
    ap.add_argument("--sizes", type=int, nargs="+", default=list(SIZES))
    ap.add_argument("--fields", type=int, nargs="+", default=[1, 4])
    ap.add_argument("--window", type=float, default=1.0, help="seconds per timed window (at least 1 for a figure that is quoted)")
    ap.add_argument("--rounds", type=int, default=2, help="windows per form; the forms take turns")
    ap.add_argument("--forms", default="abc")
    ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "element_operator" / "bench.jsonl")
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
        for Ni, Nj in ns.shapes:
            for E in ns.sizes:
                for b in ns.fields:
                    for with_j in (False, True):
                        expr = expression(f, Ni, Nj, b, with_j)
                        arrays = {"A": rnd(Ni, Nj), **{f"u{k}": rnd(E, Nj) for k in range(b)}}
                        if with_j:
                            arrays["J"] = rnd(E)
                        outs = {nm: torch.empty(E, Ni, dtype=torch.float64, device="cuda") for nm in expr.output_names}
                        forms = {}
                        if "a" in ns.forms:
                            bound_a = _bind(expr, q, arrays, outs, "auto")[1]
                            forms["a"] = (lambda bd=bound_a: bd.launch(s), launch_kind(expr, "auto", {"E": E}))
                        if "b" in ns.forms:
                            subs = "e,ij,ej->ei" if with_j else "ij,ej->ei"
                            ops = [([arrays["J"]] if with_j else []) + [arrays["A"], arrays[f"u{k}"]] for k in range(b)]

                            def witness(ops=ops, subs=subs):      # (results go where torch puts them: what its caller gets)
                                for o in ops:
                                    torch.einsum(subs, *o)
                            forms["b"] = (witness, "torch.einsum")
                        if "c" in ns.forms:
                            bound_c = _bind(expr, q, arrays, outs, "element_operator")[1]
                            forms["c"] = (lambda bd=bound_c: bd.launch(s), "element_operator")
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
                        t_bound, which = bound_seconds(Ni, Nj, E, b, with_j)
                        nbytes = 8 * (Ni + Nj + (1 if with_j else 0)) * E * b
                        lines = {}
                        for k, (_, route) in forms.items():
                            med = statistics.median(runs[k])
                            lines[k] = {"Ni": Ni, "Nj": Nj, "E": E, "b": b, "J": with_j, "form": k, "route": route,
                                        "median_us": round(med, 3), "fastest_us": min(runs[k]), "slowest_us": max(runs[k]),
                                        "spread_us": round(max(runs[k]) - min(runs[k]), 3),
                                        "GBps": round(nbytes / med * 1e-3, 1), "bound": which, "bound_us": round(t_bound * 1e6, 3),
                                        "fraction_of_bound": round(t_bound * 1e6 / med, 4), "batches": len(runs[k]), "runs_us": runs[k]}
                            fh.write(json.dumps(lines[k]) + "\n")
                        fh.flush()
                        c = lines.get("c")
                        brief = " ".join(f"{k} {ln['median_us']:9.1f} us (+-{ln['spread_us'] / 2:.1f})" for k, ln in lines.items())
                        ratios = ""
                        if c:
                            for k in ("a", "b"):
                                if k in lines:
                                    ratio = {"Ni": Ni, "Nj": Nj, "E": E, "b": b, "J": with_j, "ratio": f"{k}/c",
                                             "median": round(lines[k]["median_us"] / c["median_us"], 3),
                                             "low": round(lines[k]["fastest_us"] / c["slowest_us"], 3),
                                             "high": round(lines[k]["slowest_us"] / c["fastest_us"], 3)}
                                    fh.write(json.dumps(ratio) + "\n")
                                    ratios += f"  {k}/c {ratio['median']} [{ratio['low']}, {ratio['high']}]"
                            ratios += f"  c: {c['GBps']} GB/s, {c['fraction_of_bound']} of the {which} bound"
                        print(f"({Ni},{Nj}) E={E} b={b} J={int(with_j)}: {brief}{ratios}", flush=True)
                        del forms, arrays, outs
                        torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
