"""Tensor contractions through the "contraction" transform (fe_einsum_contract), the generic kernel and torch.einsum
(the yardstick) on the same tensors: one JSON line per (shape, dtype, transform).
    python tools/bench_contraction.py [--min-secs S] [--only NAME ...] [--no-sweep]

Columns: seconds per launch by HIP events (warm-up first, then windows of at least --min-secs), the FLOP count of the
shape (2 M N K per batch for a two-operand einsum; the schedule's steps for the chain), TFLOP/s and the fraction of the
matrix peak (78.6 / 157.3 TFLOP/s), the bytes of every input once plus the output and the fraction of the 8.0 TB/s
bandwidth roofline, the worst relative deviation from torch.einsum, and what "auto" picks.  The sweep at the end
(shape names "sweep_*") is what the "auto" thresholds of feinsum_amd/contraction.py are read from.
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
from feinsum_amd import _hip, measure  # noqa: E402
from feinsum_amd.contraction import contraction_sizes, plan_steps  # noqa: E402
from feinsum_amd.device_info import DEV_TO_PEAK_BW, DEV_TO_PEAK_GFLOPS, MI355X  # noqa: E402


def gemm(subs, ext, dtype="float64"):
    ins, _ = subs.split("->")
    return f.einsum(subs, *[f.array(n, tuple(ext[c] for c in s), dtype) for n, s in zip("ABC", ins.split(","))])


def shapes():
    sq = lambda n, m, k: {"i": n, "j": m, "k": k}   # noqa: E731
    out = []
    for name, (M, N, K) in (("gemm_1024", (1024, 1024, 1024)), ("gemm_4096", (4096, 4096, 4096)),
                            ("gemm_8192x8192x1024", (8192, 8192, 1024))):
        out.append((name, gemm("ik,kj->ij", sq(M, N, K)), 1, "float64"))
    for subs in ("ki,kj->ij", "ik,jk->ij", "ki,jk->ji"):
        out.append((f"gemm_4096_{subs.replace(',', '_').replace('->', '_')}", gemm(subs, sq(4096, 4096, 4096)), 1, "float64"))
    out.append(("gemm_4096_f32", gemm("ik,kj->ij", sq(4096, 4096, 4096), "float32"), 1, "float32"))
    out.append(("batched_64x512", gemm("bij,bjk->bik", {"b": 64, "i": 512, "j": 512, "k": 512}), 1, "float64"))
    out.append(("ttgt_abcd_ea", gemm("abcd,ea->ebcd", {"a": 48, "b": 48, "c": 48, "d": 48, "e": 64}), 1, "float64"))
    erj = f.einsum("erj,rij->ei", f.array("u", ("E", 3, 35)), f.array("D", (3, 35, 35)))
    out.append(("erj_rij_ei_1e5", erj, 100_000, "float64"))
    out.append(("erj_rij_ei_1e6", erj, 1_000_000, "float64"))
    out.append(("chain_2048", gemm("ij,jk,kl->il", {"i": 2048, "j": 2048, "k": 2048, "l": 2048}), 1, "float64"))
    return out


def sweep():
    out = []
    for N in (4, 8, 12, 16, 24, 32, 64):
        out.append((f"sweep_N{N}", gemm("ik,kj->ij", {"i": 65536, "j": N, "k": 128}), 1, "float64"))
    for K in (4, 8, 12, 16, 24, 32, 64):
        out.append((f"sweep_K{K}", gemm("ik,kj->ij", {"i": 65536, "j": 128, "k": K}), 1, "float64"))
    for M in (8, 16, 32, 64, 128):
        out.append((f"sweep_M{M}", gemm("ik,kj->ij", {"i": M, "j": 8192, "k": 128}), 1, "float64"))
    # batch-heavy: one tile per batch, little of it filled
    for b, i, j, k in ((1_000_000, 16, 8, 8), (100_000, 16, 8, 8), (100_000, 32, 16, 16), (100_000, 16, 64, 32),
                       (20_000, 64, 64, 64)):
        out.append((f"sweep_batch_b{b}_{i}x{j}x{k}", gemm("bij,bjk->bik", {"b": b, "i": i, "j": j, "k": k}), 1, "float64"))
    return out


def time_launch(fn, min_secs):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    n = 1
    while True:
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(n):
            fn()
        t1.record()
        t1.synchronize()
        secs = t0.elapsed_time(t1) * 1e-3
        if secs >= min_secs:
            return secs / n
        n = max(n + 1, int(n * min_secs / max(secs, 1e-6) * 1.2))


def flop_count(expr, sizes):
    ext = {i: (sizes[d.name] if isinstance(d, f.SizeParam) else int(d)) for i, d in expr.index_to_dim_length.items()}
    total = 0
    for st in plan_steps(expr):
        b, M, N, K = contraction_sizes(st.subscripts, ext)
        total += 2 * b * M * N * K
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--min-secs", type=float, default=1.0)
    ap.add_argument("--only", nargs="*")
    ap.add_argument("--no-sweep", action="store_true")
    args = ap.parse_args()
    sha = bench.kernel_source_sha()
    q = f.DeviceQueue(0)
    cases = shapes() + ([] if args.no_sweep else sweep())
    for name, expr, E, dtype in cases:
        if args.only and name not in args.only:
            continue
        arg_dict = dict(measure.generate_input_arrays(q, expr, E))
        sizes = measure._long_length(expr, arg_dict)
        subs = expr.get_subscripts()
        tensors = [arg_dict[a.name] for a in expr.args[0]]
        flops = flop_count(expr, sizes)
        nbytes = sum(t.numel() * t.element_size() for t in tensors)
        ref = torch.einsum(subs, *tensors)
        nbytes += ref.numel() * ref.element_size()
        peak = DEV_TO_PEAK_GFLOPS[MI355X][dtype] * 1e9
        bw = DEV_TO_PEAK_BW[MI355X] * 1e9
        auto = measure.launch_kind(expr, "auto", sizes)
        b_M_N_K = contraction_sizes(subs, {i: (sizes[d.name] if isinstance(d, f.SizeParam) else int(d))
                                           for i, d in expr.index_to_dim_length.items()}) if expr.n == 2 else None
        secs_by = {}
        for transform in ("contraction", "generic", "torch.einsum"):
            line = {"shape": name, "subscripts": subs, "E": E, "dtype": dtype, "transform": transform,
                    "batch_M_N_K": b_M_N_K, "flop": flops, "bytes": nbytes, "auto": auto, "kernel_source_sha": sha}
            if transform == "generic" and expr.n > 2:
                line["skipped"] = "the generic kernel walks the trivial schedule: 2048^4 products"
                print(json.dumps(line), flush=True)
                continue
            if transform == "torch.einsum":
                fn = lambda: torch.einsum(subs, *tensors)   # noqa: E731
                got = ref
            else:
                out = torch.empty_like(ref)
                try:
                    _, bound, _ = measure._bind(expr, q, arg_dict, {"_fe_out": out}, transform)
                    bound.launch(q.stream_ptr)
                except NotImplementedError as exc:   # e.g. "generic" on a float32 DG-family shape: no such kernel
                    line["skipped"] = str(exc)[:160]
                    print(json.dumps(line), flush=True)
                    continue
                fn = lambda: bound.launch(q.stream_ptr)   # noqa: E731
                fn()
                torch.cuda.synchronize()
                got = out
            denom = float(ref.abs().max()) or 1.0
            line["max_rel_err_vs_torch"] = float((got.double() - ref.double()).abs().max()) / denom
            secs = time_launch(fn, args.min_secs if not name.startswith("sweep") else min(args.min_secs, 0.3))
            secs_by[transform] = secs
            line.update({"seconds": secs, "tflops": flops / secs * 1e-12, "frac_matrix_peak": flops / secs / peak,
                         "frac_bw_roofline": nbytes / secs / bw})
            if "contraction" in secs_by and transform != "contraction":
                line["contraction_speedup"] = secs / secs_by["contraction"]
            print(json.dumps(line), flush=True)
            del fn
        del arg_dict, tensors, ref
        torch.cuda.empty_cache()
    for ln in _hip.kernel_resources().splitlines():
        if "contract" in ln:
            print(json.dumps({"kernel_resources": ln.strip()}))


if __name__ == "__main__":
    main()
