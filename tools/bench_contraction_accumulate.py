"""Accumulation inside the contraction and split-reduction kernels (``out <- alpha E + beta out``):
the plain overwriting launch, the ``"axpby"`` route -- what the same accumulating call runs without the transform, the
baseline -- and the kernel route (``{"accumulate": "kernel"}``), all with (alpha, beta) = (1, 1).  One JSON line per
(shape, form), appended to profiles/contraction_accumulate/bench.jsonl.
    python tools/bench_contraction_accumulate.py [--min-secs S] [--rounds R] [--only NAME ...] [--out FILE]

One process, the same arrays for every form.  Seconds per launch by HIP events; the forms alternate (plain, axpby, kernel,
plain, ...) for --rounds rounds of windows of at least --min-secs each, so that a drift of the device's clocks meets
every form alike; the figure of a form is the mean over its windows and ``spread`` their (max - min) / mean.  ``bytes`` is
the traffic counted from the shapes: every operand and the output once for the plain launch, the output twice for the
kernel route (read and written), and for the ``"axpby"`` route the plain launch into the temporary plus a pass that reads
the temporary and the output and writes the output.  ``temporary_bytes`` is what the ``"axpby"`` route allocates at bind.
"""
import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
import feinsum_amd as f  # noqa: E402
from feinsum_amd import measure  # noqa: E402


def shapes():
    """(name, subscripts, extents, dtype, variant)"""
    out = []
    for n in (1024, 4096):
        out.append((f"gemm_{n}", "ik,kj->ij", {"i": n, "j": n, "k": n}, "float64", "contraction"))
    out.append(("gemm_4096_f32", "ik,kj->ij", {"i": 4096, "j": 4096, "k": 4096}, "float32", "contraction"))
    out.append(("ttgt_abcd_ea", "abcd,ea->ebcd", {"a": 48, "b": 48, "c": 48, "d": 48, "e": 64}, "float64", "contraction"))
    for E in (10**5, 10**6):
        out.append((f"erj_rij_{E}", "erj,rij->ei", {"e": E, "r": 3, "j": 35, "i": 35}, "float64", "contraction"))
    out.append(("batched_32x16x16", "bij,bjk->bik", {"b": 10**5, "i": 32, "j": 16, "k": 16}, "float64", "contraction"))
    out.append(("gram_ei_ej", "ei,ej->ij", {"e": 10**6, "i": 35, "j": 35}, "float64", "reduction"))
    out.append(("dot_ei_ei", "ei,ei->", {"e": 10**6, "i": 35}, "float64", "reduction"))
    return out


def window(launch, min_secs):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    total, n, batch = 0.0, 0, 2
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


def run(name, subs, extent, dtype, variant, min_secs, rounds):
    ins, rhs = subs.split("->")
    ins = ins.split(",")
    expr = f.einsum(subs, *[f.array("ABCD"[p], tuple(extent[c] for c in idx), dtype) for p, idx in enumerate(ins)])
    tdt = getattr(torch, dtype)
    gen = torch.Generator(device="cuda").manual_seed(1)
    dev = {"ABCD"[p]: torch.rand(tuple(extent[c] for c in idx), dtype=tdt, device="cuda", generator=gen) - 0.5
           for p, idx in enumerate(ins)}
    oshape = tuple(extent[c] for c in rhs)
    out = torch.zeros(oshape, dtype=tdt, device="cuda")
    tmp = torch.empty_like(out)
    oname = expr.output_names[0]
    q, plain, _ = measure._bind(expr, 0, dev, {oname: tmp}, variant)
    # alpha = 1, beta = 1 on zero-mean data: the output walks randomly and stays finite over the run
    _, axpby, _ = measure._bind(expr, 0, dev, {oname: out}, {"variant": variant, "accumulate": "axpby"}, alpha=1.0, beta=1.0)
    _, kernel, _ = measure._bind(expr, 0, dev, {oname: out}, {"variant": variant, "accumulate": "kernel"}, alpha=1.0, beta=1.0)
    assert (plain.accumulate, axpby.accumulate, kernel.accumulate) == (None, "axpby", "kernel")
    s = q.stream_ptr
    forms = (("plain", lambda: plain.launch(s)), ("axpby", lambda: axpby.launch(s)), ("kernel", lambda: kernel.launch(s)))
    for _, launch in forms:
        for _ in range(3):
            launch()
    torch.cuda.synchronize()
    times = {form: [] for form, _ in forms}
    for _ in range(rounds):
        for form, launch in forms:
            times[form].append(window(launch, min_secs))
    esize = np.dtype(dtype).itemsize
    in_bytes = sum(int(np.prod([extent[c] for c in idx], dtype=np.int64)) for idx in ins) * esize
    out_bytes = int(np.prod(oshape, dtype=np.int64)) * esize
    nbytes = {"plain": in_bytes + out_bytes, "axpby": in_bytes + 4 * out_bytes, "kernel": in_bytes + 2 * out_bytes}
    sha = bench.kernel_source_sha()
    mean = {form: float(np.mean(ts)) for form, ts in times.items()}
    rows = []
    for form, ts in times.items():
        rows.append({"shape": name, "subscripts": subs, "extents": extent, "dtype": dtype, "variant": variant, "form": form,
                     "seconds": mean[form], "windows": ts, "spread": (max(ts) - min(ts)) / mean[form],
                     "bytes": nbytes[form], "gbps": nbytes[form] / mean[form] * 1e-9,
                     "temporary_bytes": out_bytes if form == "axpby" else 0,
                     "entry_point": getattr(kernel if form == "kernel" else plain, "entry_point", None),
                     "speedup_vs_axpby": mean["axpby"] / mean[form], "kernel_source_sha": sha})
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--min-secs", type=float, default=1.0)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--only", nargs="+", default=None)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "contraction_accumulate" / "bench.jsonl"))
    args = ap.parse_args()
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    with open(args.out, "a") as fh:
        for name, subs, extent, dtype, variant in shapes():
            if args.only and name not in args.only:
                continue
            for row in run(name, subs, extent, dtype, variant, args.min_secs, args.rounds):
                line = json.dumps(row)
                print(line, flush=True)
                fh.write(line + "\n")
            fh.flush()
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
