"""Accumulating face-mass (``out <- alpha E + beta out``) at p = 4, b = 4: what a caller did before
against the two routes of ``evaluate(..., alpha=1, beta=1)`` -- and accumulating grad and div at p = 4 (one field): the add
pass, the ``"axpby"`` route (their default) and the opt-in ``"epilogue"`` route.  One JSON line per (workload, E, form),
appended to profiles/accumulate/bench_accumulate.jsonl.
    python tools/bench_accumulate.py [--min-secs S] [--sizes E ...] [--dg-sizes E ...] [--families NAME ...] [--out FILE]

Forms, all in one process on the same arrays:
  "evaluate+4adds"  the lift into four arrays of its own, then four ``torch.add(rhs, lift, out=rhs)`` (the parent commit's way)
  "axpby"           the fallback route: the lift into four temporaries, then four ``fe_axpby``
  "kernel"          the accumulating face-mass kernel (``fe_facemass_acc_f64``)
  "plain"           the lift alone, overwriting (what the add passes are paid on top of)
grad / div: "plain", "evaluate+add" (one ``torch.add(out=)`` per output array), "axpby" and "epilogue" (the accumulating
kernels, ``fe_grad3d_acc_f64`` / ``fe_div3d_acc_f64``); ``speedup_vs_axpby`` is the ratio tests/test_gpu_accumulate_epilogue.py
takes its floor from.
Seconds per evaluation by HIP events over windows of at least --min-secs after a warm-up; ``doubles_per_element`` is the
traffic counted from the code, ``gbps`` that count over the measured time.
"""
import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

import torch  # noqa: E402

import bench  # noqa: E402
import feinsum_amd as f  # noqa: E402
from feinsum_amd import measure  # noqa: E402

NP, NF, NFP, B = 35, 4, 15, 4
LIFT_DOUBLES = NF + B * NF * NFP + B * NP                 # J, four face fields, four outputs: 384
DOUBLES = {"plain": LIFT_DOUBLES, "evaluate+4adds": LIFT_DOUBLES + B * 3 * NP, "axpby": LIFT_DOUBLES + B * 3 * NP,
           "kernel": LIFT_DOUBLES + B * NP}


def seconds(launch, min_secs):
    for _ in range(5):
        launch()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    total, n, batch = 0.0, 0, 4
    while total < min_secs:
        t0.record()
        for _ in range(batch):
            launch()
        t1.record()
        t1.synchronize()
        total += t0.elapsed_time(t1) * 1e-3
        n += batch
        batch = min(2 * batch, 1024)
    return total / n


def run(E, min_secs):
    expr = f.batched_einsum("ef,fij,fej->ei", [[f.array("J", ("E", NF)), f.array("R", (NF, NP, NFP)),
                                                f.array(f"v{k}", (NF, "E", NFP))] for k in range(B)])
    gen = torch.Generator(device="cuda").manual_seed(1)
    dev = {"J": torch.rand((E, NF), dtype=torch.float64, device="cuda", generator=gen),
           "R": torch.rand((NF, NP, NFP), dtype=torch.float64, device="cuda", generator=gen)}
    for k in range(B):
        dev[f"v{k}"] = torch.rand((NF, E, NFP), dtype=torch.float64, device="cuda", generator=gen)
    rhs = {n: torch.zeros((E, NP), dtype=torch.float64, device="cuda") for n in expr.output_names}
    lift = {n: torch.empty_like(t) for n, t in rhs.items()}
    q, plain, _ = measure._bind(expr, 0, dev, lift, None)
    _, axpby, _ = measure._bind(expr, 0, dev, rhs, {"accumulate": "axpby"}, alpha=1.0, beta=1.0)
    _, kernel, _ = measure._bind(expr, 0, dev, rhs, {"accumulate": "kernel"}, alpha=1.0, beta=1.0)
    s = q.stream_ptr

    def before():
        plain.launch(s)
        for n in expr.output_names:
            torch.add(rhs[n], lift[n], out=rhs[n])

    forms = (("plain", lambda: plain.launch(s)), ("evaluate+4adds", before), ("axpby", lambda: axpby.launch(s)),
             ("kernel", lambda: kernel.launch(s)))
    sha = bench.kernel_source_sha()
    rows = []
    for form, launch in forms:
        for t in rhs.values():
            t.zero_()
        sec = seconds(launch, min_secs)
        rows.append({"workload": "face_mass p4 x4, out <- E + out", "E": E, "form": form, "seconds": sec,
                     "doubles_per_element": DOUBLES[form], "gbps": DOUBLES[form] * 8 * E / sec * 1e-9, "kernel_source_sha": sha})
    base = {r["form"]: r["seconds"] for r in rows}
    for r in rows:
        r["speedup_vs_evaluate+4adds"] = base["evaluate+4adds"] / r["seconds"]
    return rows


# doubles per element, counted from the operand shapes: J, the operator's share (none), u, out; an add or axpby pass moves 3 out
DG_OUT = {"grad": 3 * NP, "div": NP}
DG_PLAIN = {"grad": 9 + NP + 3 * NP, "div": 9 + 3 * NP + NP}


def run_dg(family, E, min_secs):
    if family == "grad":
        expr = f.einsum("xre,rij,ej->xei", f.array("J", (3, 3, "E")), f.array("D", (3, NP, NP)), f.array("u", ("E", NP)))
        ushape, oshape = (E, NP), (3, E, NP)
    else:
        expr = f.einsum("xre,rij,xej->ei", f.array("J", (3, 3, "E")), f.array("D", (3, NP, NP)), f.array("u", (3, "E", NP)))
        ushape, oshape = (3, E, NP), (E, NP)
    gen = torch.Generator(device="cuda").manual_seed(1)
    dev = {"J": torch.rand((3, 3, E), dtype=torch.float64, device="cuda", generator=gen),
           "D": torch.rand((3, NP, NP), dtype=torch.float64, device="cuda", generator=gen),
           "u": torch.rand(ushape, dtype=torch.float64, device="cuda", generator=gen)}
    name = expr.output_names[0]
    rhs = torch.zeros(oshape, dtype=torch.float64, device="cuda")
    tmp = torch.empty_like(rhs)
    q, plain, _ = measure._bind(expr, 0, dev, {name: tmp}, None)
    _, axpby, _ = measure._bind(expr, 0, dev, {name: rhs}, {"accumulate": "axpby"}, alpha=1.0, beta=1.0)
    _, epilogue, _ = measure._bind(expr, 0, dev, {name: rhs}, {"accumulate": "epilogue"}, alpha=1.0, beta=1.0)
    assert (axpby.accumulate, epilogue.accumulate) == ("axpby", "epilogue")
    s = q.stream_ptr

    def before():
        plain.launch(s)
        torch.add(rhs, tmp, out=rhs)

    forms = (("plain", lambda: plain.launch(s)), ("evaluate+add", before), ("axpby", lambda: axpby.launch(s)),
             ("epilogue", lambda: epilogue.launch(s)))
    doubles = {"plain": DG_PLAIN[family], "evaluate+add": DG_PLAIN[family] + 3 * DG_OUT[family],
               "axpby": DG_PLAIN[family] + 3 * DG_OUT[family], "epilogue": DG_PLAIN[family] + DG_OUT[family]}
    sha = bench.kernel_source_sha()
    rows = []
    for form, launch in forms:
        rhs.zero_()
        sec = seconds(launch, min_secs)
        rows.append({"workload": f"{family} p4, out <- E + out", "E": E, "form": form, "seconds": sec,
                     "doubles_per_element": doubles[form], "gbps": doubles[form] * 8 * E / sec * 1e-9, "kernel_source_sha": sha})
    base = {r["form"]: r["seconds"] for r in rows}
    for r in rows:
        r["speedup_vs_evaluate+add"] = base["evaluate+add"] / r["seconds"]
        r["speedup_vs_axpby"] = base["axpby"] / r["seconds"]
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--min-secs", type=float, default=1.0)
    ap.add_argument("--sizes", type=int, nargs="+", default=[100_000, 1_000_000])
    ap.add_argument("--dg-sizes", type=int, nargs="+", default=[100_000, 200_000, 1_000_000])
    ap.add_argument("--families", nargs="+", default=["face_mass", "grad", "div"], choices=["face_mass", "grad", "div"])
    ap.add_argument("--out", default=str(ROOT / "profiles" / "accumulate" / "bench_accumulate.jsonl"))
    args = ap.parse_args()
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    with open(args.out, "a") as fh:
        jobs = [(lambda E=E: run(E, args.min_secs)) for E in args.sizes if "face_mass" in args.families]
        jobs += [(lambda fam=fam, E=E: run_dg(fam, E, args.min_secs)) for fam in ("grad", "div") if fam in args.families
                 for E in args.dg_sizes]
        for job in jobs:
            for row in job():
                line = json.dumps(row)
                print(line, flush=True)
                fh.write(line + "\n")


if __name__ == "__main__":
    main()
