"""Einsums mixing float32 and float64 operands: the mixed launch against the all-float64 kernel on operands converted
beforehand, and against converting the float32 operand on every launch (cast + all-float64).  One JSON line per
(shape, form).
    python tools/bench_mixed.py [--min-secs S] [--quick]

Forms: "mixed" (float32 operands widened as they are loaded), "f64" (the same kernel on pre-converted operands: the
arithmetic-only bound), "cast+f64" (``Tensor.copy_`` of the float32 operand into a float64 buffer, then the f64 launch:
what a caller does without this path).  Seconds per launch by HIP events over windows of at least --min-secs after a
warm-up; TFLOP/s = 2 x (multiply-adds) / s; GB/s counts every input once in its own dtype plus the output.
--quick: one short window per form, smaller shapes (for a profiler run).
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
from feinsum_amd import measure  # noqa: E402


def case(name, subs, shapes, f32, transform):
    return {"name": name, "subs": subs, "shapes": shapes, "f32": f32, "transform": transform}


def cases(quick):
    n = 2048 if quick else 4096
    E1, E2 = (100_000, 200_000) if quick else (100_000, 1_000_000)
    B = 16 if quick else 64
    out = [case(f"gemm_{n}_Af32", "ik,kj->ij", {"A": (n, n), "B": (n, n)}, "A", "contraction"),
           case(f"gemm_{n}_Bf32", "ik,kj->ij", {"A": (n, n), "B": (n, n)}, "B", "contraction"),
           case(f"erj_rij_ei_{E1:.0e}", "erj,rij->ei", {"u": (E1, 3, 35), "D": (3, 35, 35)}, "u", "contraction"),
           case(f"erj_rij_ei_{E2:.0e}", "erj,rij->ei", {"u": (E2, 3, 35), "D": (3, 35, 35)}, "u", "contraction"),
           case(f"bij_bjk_{B}x512", "bij,bjk->bik", {"A": (B, 512, 512), "B": (B, 512, 512)}, "A", "contraction"),
           case("generic_ej_ej_ej", "ej,ej->ej", {"A": (E2, 64), "B": (E2, 64)}, "A", "generic"),
           case(f"generic_ij_j_i_{n}", "ij,j->i", {"A": (n, n), "x": (n,)}, "A", "generic")]
    return out


def seconds(launch, min_secs):
    for _ in range(3):
        launch()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    total, n, batch = 0.0, 0, 1
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


def run(c, min_secs):
    names = list(c["shapes"])
    ins, out_idx = c["subs"].split("->")
    ext = {}
    for nm, s in zip(names, ins.split(",")):
        ext.update(zip(s, c["shapes"][nm]))
    gen = torch.Generator(device="cuda").manual_seed(1)
    dev64 = {k: torch.rand(s, dtype=torch.float64, device="cuda", generator=gen) for k, s in c["shapes"].items()}
    dev_mixed = dict(dev64, **{c["f32"]: dev64[c["f32"]].to(torch.float32)})
    dev64[c["f32"]] = dev_mixed[c["f32"]].to(torch.float64)   # the same values in both forms
    out = torch.empty(tuple(ext[i] for i in out_idx), dtype=torch.float64, device="cuda")
    mixed = f.einsum(c["subs"], *[f.array(k, s, "float32" if k == c["f32"] else "float64")
                                  for k, s in c["shapes"].items()])
    uniform = f.einsum(c["subs"], *[f.array(k, s) for k, s in c["shapes"].items()])
    _, bm, _ = measure._bind(mixed, 0, dev_mixed, {"_fe_out": out}, c["transform"])
    _, bu, _ = measure._bind(uniform, 0, dev64, {"_fe_out": out}, c["transform"])
    stream = torch.cuda.current_stream().cuda_stream
    cast_dst, cast_src = dev64[c["f32"]], dev_mixed[c["f32"]]

    def cast_then_f64():
        cast_dst.copy_(cast_src)
        bu.launch(stream)

    bm.launch(stream)
    torch.cuda.synchronize()
    ref = out.clone()
    bu.launch(stream)
    torch.cuda.synchronize()
    max_rel = float(((out - ref).abs() / ref.abs().clamp_min(1e-300)).max())
    flops = 2.0 * float(np.prod([ext[i] for i in dict.fromkeys("".join(ins.split(",")))], dtype=np.float64))
    nbytes = sum(t.numel() * t.element_size() for t in dev_mixed.values()) + out.numel() * 8
    rows = []
    for form, launch in (("mixed", lambda: bm.launch(stream)), ("f64", lambda: bu.launch(stream)),
                         ("cast+f64", cast_then_f64)):
        s = seconds(launch, min_secs)
        rows.append({"shape": c["name"], "subs": c["subs"], "f32_operand": c["f32"], "transform": c["transform"],
                     "form": form, "seconds": s, "tflops": flops / s * 1e-12, "gbps_mixed_bytes": nbytes / s * 1e-9,
                     "max_rel_vs_f64": max_rel})
    base = {r["form"]: r["seconds"] for r in rows}
    for r in rows:
        r["speedup_vs_cast"] = base["cast+f64"] / r["seconds"]
        r["rate_vs_f64"] = base["f64"] / r["seconds"]
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--min-secs", type=float, default=1.0)
    ap.add_argument("--quick", action="store_true")
    args = ap.parse_args()
    min_secs = 0.05 if args.quick else args.min_secs
    for c in cases(args.quick):
        for row in run(c, min_secs):
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
