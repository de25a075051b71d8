"""Float32 fields in float64 grad, div and face-mass x 4 at p = 4 (transform "mixed_family", csrc/fe_mixed.h) against what
the same caller can do without it.  One JSON line per (family, E, form).
    python tools/bench_mixed_dg.py [--min-secs S] [--sizes 100000,200000,1000000] [--out FILE]

Forms:
  "mixed_family"  the float32-field kernels;
  "auto"          transform "auto" on the same mixed einsum (the one-thread-per-entry generic kernel);
  "cast+f64"      a float32 -> float64 conversion pass of every field on the same stream (``Tensor.copy_`` into a float64
                  buffer: ``Tensor.double()`` without the allocation), then the float64 einsum under "auto";
  "f64"           the float64 einsum alone, on fields widened beforehand.
At the sizes from 2 10^5 on, "mixed_family" is also timed at E + 1 ("mixed_family, odd E"): an odd number of elements puts
the float32 planes of div and the face slabs of face-mass on 4-byte boundaries, and the fields then come through registers
instead of LDS-DMA (grad's one field array stays aligned, so its odd-E row is the LDS-DMA form with a remainder).
Seconds per launch by HIP events over windows of at least --min-secs after a warm-up, one process.  "bytes_per_element" counts
every streamed operand once in its own dtype plus the outputs; "roofline_fraction" is that traffic over 8 TB/s.
"""
import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

import torch  # noqa: E402

import feinsum_amd as f  # noqa: E402
from feinsum_amd import _hip, measure  # noqa: E402

NP, NFP, NF, B_FM = 35, 15, 4, 4
HBM_BYTES_PER_S = 8e12


def einsum_of(family, field_dtype):
    if family == "facemass":
        return f.batched_einsum("ef,fij,fej->ei", [[f.array("J", ("E", NF)), f.array("R", (NF, NP, NFP)),
                                                     f.array(f"v{k}", (NF, "E", NFP), field_dtype)] for k in range(B_FM)])
    fshape, subs = ((("E", NP), "xre,rij,ej->xei") if family == "grad" else ((3, "E", NP), "xre,rij,xej->ei"))
    return f.einsum(subs, f.array("J", (3, 3, "E")), f.array("R", (3, NP, NP)), f.array("u", fshape, field_dtype))


def bytes_per_element(family, field_bytes):
    """(J, fields, outputs) bytes per element."""
    if family == "grad":
        return 72, NP * field_bytes, 3 * NP * 8
    if family == "div":
        return 72, 3 * NP * field_bytes, NP * 8
    return NF * 8, B_FM * NF * NFP * field_bytes, B_FM * NP * 8


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


def bound_forms(family, E, gen=None):
    """The four forms of one (family, E) as ``{form: launch()}`` on the current stream, with what keeps their arrays alive."""
    gen = gen or torch.Generator(device="cuda").manual_seed(1)
    mixed, uniform = einsum_of(family, "float32"), einsum_of(family, "float64")
    shape = lambda a: tuple(E if isinstance(d, f.SizeParam) else int(d) for d in a.shape)   # noqa: E731
    dev32, dev64 = {}, {}
    for row in mixed.args:
        for a in row:
            if a.name not in dev32:
                t = torch.rand(shape(a), dtype=torch.float64, device="cuda", generator=gen) - 0.5
                dev32[a.name] = t.to(torch.float32) if a.dtype == "float32" else t
                dev64[a.name] = dev32[a.name].to(torch.float64) if a.dtype == "float32" else t
    fields = [n for n in dev32 if dev32[n].dtype == torch.float32]
    outs = dict(measure.generate_out_arrays(0, uniform, E))
    stream = torch.cuda.current_stream().cuda_stream
    _, bm, _ = measure._bind(mixed, 0, dev32, outs, "mixed_family")
    _, ba, _ = measure._bind(mixed, 0, dev32, outs, "auto")
    _, bu, _ = measure._bind(uniform, 0, dev64, outs, "auto")

    def cast_then_f64():
        for n in fields:
            dev64[n].copy_(dev32[n])
        bu.launch(stream)

    forms = {"mixed_family": lambda: bm.launch(stream), "auto": lambda: ba.launch(stream), "cast+f64": cast_then_f64,
             "f64": lambda: bu.launch(stream)}
    return forms, (dev32, dev64, outs, bm, ba, bu)


def rows_of(family, E, min_secs, only=None, label=None):
    forms, keep = bound_forms(family, E)
    outs = keep[2]
    forms["mixed_family"]()
    torch.cuda.synchronize()
    info = _hip.last_launch_info()
    ref = {n: t.clone() for n, t in outs.items()}
    forms["f64"]()
    torch.cuda.synchronize()
    max_rel = max(float(((outs[n] - ref[n]).abs().max() / ref[n].abs().max())) for n in outs)
    rows = []
    for form, launch in forms.items():
        if only and form not in only:
            continue
        s = seconds(launch, min_secs)
        j, fld, out = bytes_per_element(family, 4 if form in ("mixed_family", "auto") else 8)
        per = j + fld + out + (bytes_per_element(family, 4)[1] + fld if form == "cast+f64" else 0)   # the pass reads 4, writes 8
        rows.append({"family": family, "Np": NP, "b": B_FM if family == "facemass" else 1, "E": E, "form": label or form,
                     "seconds": s, "bytes_per_element": per, "gbps": per * E / s * 1e-9,
                     "roofline_fraction": per * E / s / HBM_BYTES_PER_S, "max_rel_vs_f64": max_rel,
                     "plain_field_loads": bool(info.get("plain_field_loads")) if form == "mixed_family" else None})
    del keep
    torch.cuda.empty_cache()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--min-secs", type=float, default=1.0)
    ap.add_argument("--sizes", default="100000,200000,1000000")
    ap.add_argument("--families", default="grad,div,facemass")
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    args = ap.parse_args()
    sink = open(args.out, "a") if args.out else None
    for family in args.families.split(","):
        for E in (int(s) for s in args.sizes.split(",")):
            rows = rows_of(family, E, args.min_secs)
            base = {r["form"]: r["seconds"] for r in rows}
            if E >= 200_000:
                rows += rows_of(family, E + 1, args.min_secs, only=("mixed_family",), label="mixed_family, odd E")
            for r in rows:
                r["auto_over_this"] = base["auto"] / r["seconds"]
                r["cast_over_this"] = base["cast+f64"] / r["seconds"]
                r["f64_over_this"] = base["f64"] / r["seconds"]
                line = json.dumps(r)
                print(line, flush=True)
                if sink:
                    sink.write(line + "\n")
                    sink.flush()
    if sink:
        sink.close()


if __name__ == "__main__":
    main()
