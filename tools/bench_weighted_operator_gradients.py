#!/usr/bin/env python3
"""What differentiating the weighted element operator on the matrix cores gives: the weight gradient
'iq,qj,ej,ei->eq' summed over b rows, three forms per case, and the whole backward pass (dW and every du_k), two forms, in ONE
process, alternating, timed with HIP events:

  a  the route "auto" takes for the adjoint einsum (the generic one-thread-per-entry kernel, one output per row, the rows added);
  c  what a caller can chain by hand from kernels older than fe_weightgrad_f64: two ``"element_operator"`` launches (A u_k and
     P^T g_k for every field), ``torch.mul`` into dW and ``addcmul_`` for the further fields, the 2 b temporaries of E x Nq
     allocated once;
  d  fe_weightgrad_f64 (``measure._WeightGradLaunch``);
  auto / kernel  ``torch.autograd.grad`` of one ``evaluate_differentiable`` graph for W and every u_k, with
     ``element_gradients="auto"`` (forward ``"auto"``) against ``"kernel"`` (forward ``"weighted_element_operator"``).

Method as tools/bench_weighted_element_operator.py: every form is bound once, warmed up, then timed in windows of at least
``--window`` seconds (batches of launches between two events), ``--rounds`` windows per form, the forms taking turns.  A line of
profiles/weighted_operator_gradients/bench.jsonl holds the per-launch microseconds of every batch, their median and slowest -
fastest; for a, c and d also GB/s from the 8 (b (Ni + Nj) + Nq) E bytes the operation needs and the fraction of the bound
max(bytes / 8 TB/s, matrix-core cycles at the sustained clock), section 3r's formula with this kernel's MFMA count.

The tool is one process and stops at the first error.  Run it under a time limit, e.g.

    timeout -k 10 1100 python tools/bench_weighted_operator_gradients.py && echo done
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))

from bench_weighted_element_operator import MFMA_CYCLES, PEAK_BYTES_PER_S, SIMDS, SUSTAINED_HZ, needed_bytes, window  # noqa: E402

SHAPES = ((35, 56, 35), (20, 35, 20), (10, 20, 10), (4, 10, 4), (20, 56, 35))
SIZES = (100_000, 200_000, 1_000_000)
FWD = "iq,eq,qj,ej->ei"


def bound_seconds(Ni, Nq, Nj, E, b):
    """(seconds, name) of the bound that applies: the needed bytes at the HBM peak, or the MFMAs of both chains of ceil(E / 16)
    tiles per field spread over every SIMD at the sustained clock."""
    t_bw = needed_bytes(Ni, Nq, Nj, E, b) / PEAK_BYTES_PER_S
    mfmas = -(-Nq // 16) * (-(-Nj // 4) + -(-Ni // 4)) * -(-E // 16) * b
    t_mfma = mfmas / SIMDS * MFMA_CYCLES / SUSTAINED_HZ
    return (t_bw, "bandwidth") if t_bw >= t_mfma else (t_mfma, "matrix cores")


def two_pass(f, torch, q, P, A, us, gs, dW, shape, E):
    """Form c: returns the launch."""
    from feinsum_amd.measure import _bind

    Ni, Nq, Nj = shape
    b, s = len(us), q.stream_ptr
    up = f.batched_einsum("ij,ej->ei", [[f.array("A", (Nq, Nj)), f.array(f"u{k}", ("E", Nj))] for k in range(b)])
    gup = f.batched_einsum("ji,ej->ei", [[f.array("P", (Ni, Nq)), f.array(f"g{k}", ("E", Ni))] for k in range(b)])
    ts = [torch.empty(E, Nq, dtype=torch.float64, device="cuda") for _ in range(b)]
    ss = [torch.empty(E, Nq, dtype=torch.float64, device="cuda") for _ in range(b)]
    first = _bind(up, q, {"A": A, **{f"u{k}": u for k, u in enumerate(us)}}, dict(zip(up.output_names, ts)), "element_operator")[1]
    second = _bind(gup, q, {"P": P, **{f"g{k}": g for k, g in enumerate(gs)}}, dict(zip(gup.output_names, ss)), "element_operator")[1]

    def launch():
        first.launch(s)
        second.launch(s)
        torch.mul(ts[0], ss[0], out=dW)
        for t, sk in zip(ts[1:], ss[1:]):
            dW.addcmul_(t, sk)
    return launch


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--shapes", type=lambda s: tuple(int(x) for x in s.split("x")), nargs="+", default=list(SHAPES), metavar="NIxNQxNJ")
    ap.add_argument("--sizes", type=int, nargs="+", default=list(SIZES))
    ap.add_argument("--fields", type=int, nargs="+", default=[1, 4])
    ap.add_argument("--window", type=float, default=1.0, help="seconds per timed window (at least 1 for a figure that is quoted)")
    ap.add_argument("--rounds", type=int, default=2, help="windows per form; the forms take turns")
    ap.add_argument("--forms", nargs="+", default=["a", "c", "d", "auto", "kernel"])
    ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "weighted_operator_gradients" / "bench.jsonl")
    ns = ap.parse_args()

    import torch

    import feinsum_amd as f
    from feinsum_amd.autograd import adjoint_terms, output_grad_name
    from feinsum_amd.family import match_weighted_operator_weight_adjoint
    from feinsum_amd.measure import _bind, _WeightGradLaunch

    q = f.DeviceQueue(0)
    s = q.stream_ptr
    gen = torch.Generator(device="cuda").manual_seed(0)
    rnd = lambda *shape: torch.rand(*shape, generator=gen, device="cuda", dtype=torch.float64) * 2 - 1   # noqa: E731
    ns.out.parent.mkdir(parents=True, exist_ok=True)
    with ns.out.open("w") as fh:
        for shape in ns.shapes:
            Ni, Nq, Nj = shape
            for E in ns.sizes:
                for b in ns.fields:
                    expr = f.batched_einsum(FWD, [[f.array("P", (Ni, Nq)), f.array("W", ("E", Nq)), f.array("A", (Nq, Nj)),
                                                   f.array(f"u{k}", ("E", Nj))] for k in range(b)])
                    P, W, A = rnd(Ni, Nq), rnd(E, Nq), rnd(Nq, Nj)
                    us, gs = [rnd(E, Nj) for _ in range(b)], [rnd(E, Ni) for _ in range(b)]
                    (term,) = adjoint_terms(expr, "W")
                    term = term.einsum
                    args = {"P": P, "A": A, **{f"u{k}": u for k, u in enumerate(us)},
                            **{output_grad_name(nm): g for nm, g in zip(expr.output_names, gs)}}
                    dW = torch.empty(E, Nq, dtype=torch.float64, device="cuda")
                    forms = {}
                    if "a" in ns.forms:
                        rows = [torch.empty(E, Nq, dtype=torch.float64, device="cuda") for _ in range(b)]
                        bound = _bind(term, q, args, dict(zip(term.output_names, rows)), "auto")[1]

                        def auto_rows(bd=bound, rows=rows):
                            bd.launch(s)
                            for r in rows[1:]:
                                rows[0].add_(r)
                        forms["a"] = (auto_rows, "auto: generic, rows added")
                    if "c" in ns.forms:
                        forms["c"] = (two_pass(f, torch, q, P, A, us, gs, dW, shape, E), "element_operator x 2, torch.mul / addcmul_")
                    if "d" in ns.forms:
                        wg = _WeightGradLaunch(match_weighted_operator_weight_adjoint(term), term, args, [dW])
                        forms["d"] = (lambda wg=wg: wg.launch(s), "fe_weightgrad_f64")
                    for key, transform in (("auto", "auto"), ("kernel", "weighted_element_operator")):
                        if key in ns.forms:
                            leaves = [W.clone().requires_grad_(True)] + [u.clone().requires_grad_(True) for u in us]
                            outs = f.evaluate_differentiable(expr, q, {"P": P, "A": A, "W": leaves[0],
                                                                       **{f"u{k}": t for k, t in enumerate(leaves[1:])}},
                                                             transform=transform, element_gradients=key)
                            heads = [outs[nm] for nm in expr.output_names]
                            forms[key] = (lambda heads=heads, leaves=leaves: torch.autograd.grad(heads, leaves, gs, retain_graph=True),
                                          f"backward pass (dW, du x {b}), element_gradients={key}")
                    runs = {k: [] for k in forms}
                    batch = {}
                    for k, (launch, _) in forms.items():            # warm-up, and the batch size of about 50 ms
                        launch()
                        torch.cuda.synchronize()
                        us_per = window(torch, launch, 2, 1e-9)[0]
                        batch[k] = max(1 if us_per > 50_000 else 5, min(400, int(50_000 / max(us_per, 1.0))))
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
                                    "spread_us": round(max(runs[k]) - min(runs[k]), 3), "batches": len(runs[k]), "runs_us": runs[k]}
                        if k in ("a", "c", "d"):
                            lines[k].update({"GBps": round(nbytes / med * 1e-3, 1), "bound": which, "bound_us": round(t_bound * 1e6, 3),
                                             "fraction_of_bound": round(t_bound * 1e6 / med, 4)})
                        fh.write(json.dumps(lines[k]) + "\n")
                    brief = " ".join(f"{k} {ln['median_us']:9.1f} us (+-{ln['spread_us'] / 2:.1f})" for k, ln in lines.items())
                    ratios = ""
                    for num, den in (("a", "d"), ("c", "d"), ("auto", "kernel")):
                        if num in lines and den in lines:
                            ratio = {"Ni": Ni, "Nq": Nq, "Nj": Nj, "E": E, "b": b, "ratio": f"{num}/{den}",
                                     "median": round(lines[num]["median_us"] / lines[den]["median_us"], 3),
                                     "low": round(lines[num]["fastest_us"] / lines[den]["slowest_us"], 3),
                                     "high": round(lines[num]["slowest_us"] / lines[den]["fastest_us"], 3)}
                            fh.write(json.dumps(ratio) + "\n")
                            ratios += f"  {num}/{den} {ratio['median']} [{ratio['low']}, {ratio['high']}]"
                    if "d" in lines:
                        ratios += f"  d: {lines['d']['GBps']} GB/s, {lines['d']['fraction_of_bound']} of the {which} bound"
                    fh.flush()
                    print(f"({Ni},{Nq},{Nj}) E={E} b={b}: {brief}{ratios}", flush=True)
                    del forms, args
                    torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
