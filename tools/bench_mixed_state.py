"""Float32 results from the float32-field grad, div and face-mass x 4 kernels at p = 4 (transform "mixed_state", csrc/fe_mixed.h
with OUT = float) against what a float32 solver does without them, DESIGN.md section 3j:

  (a) "mixed_state"         float32 fields in, float32 results out, float64 J / operator / arithmetic;
  (b) "mixed_family+copy"   "mixed_family" (float64 results), then Tensor.copy_ of every output into a float32 array -- the
                            route a float32 solver takes without (a), and the reference of the ratio;
  (c) "mixed_family"        alone (the caller keeps float64 results);
  (d) "f64"                 the all-float64 kernel under "auto".

    python tools/bench_mixed_state.py [--sizes 100000,200000,1000000] [--min-secs 1.0] [--out file.jsonl]

Seconds per launch by HIP events, in ALTERNATING windows of at least --min-secs each (three rounds over the forms, the best
window of each), one process.  "bytes_per_element" counts every streamed operand once in its own dtype plus the outputs (and
the pass of (b): 8 read, 4 written per output entry).  At E >= 2 10^5, (a) is also timed at E + 1: an odd E puts grad's planes 1
and 2 on 4-byte boundaries, which takes the 4-byte store form.
"""
import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))

import torch  # noqa: E402

from bench_mixed_dg import B_FM, HBM_BYTES_PER_S, NF, NFP, NP, bytes_per_element, einsum_of  # noqa: E402
from feinsum_amd import _hip, measure  # noqa: E402
import feinsum_amd as f  # noqa: E402

FORMS = ("mixed_state", "mixed_family+copy", "mixed_family", "f64")


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
    outs64 = dict(measure.generate_out_arrays(0, uniform, E))
    outs32 = dict(measure.generate_out_arrays(0, mixed, E, transform="mixed_state"))
    down = {n: torch.zeros_like(t) for n, t in outs32.items()}          # where (b) puts its float32 copies
    stream = torch.cuda.current_stream().cuda_stream
    _, bs, _ = measure._bind(mixed, 0, dev32, outs32, "mixed_state")
    _, bm, _ = measure._bind(mixed, 0, dev32, outs64, "mixed_family")
    _, bu, _ = measure._bind(uniform, 0, dev64, outs64, "auto")

    def family_then_copy():
        bm.launch(stream)
        for n, t in outs64.items():
            down[n].copy_(t)

    forms = {"mixed_state": lambda: bs.launch(stream), "mixed_family+copy": family_then_copy,
             "mixed_family": lambda: bm.launch(stream), "f64": lambda: bu.launch(stream)}
    return forms, {"dev32": dev32, "dev64": dev64, "outs64": outs64, "outs32": outs32, "down": down, "bound": (bs, bm, bu)}


def window(launch, min_seconds):
    """Seconds per launch over one window of at least *min_seconds* (HIP events)."""
    reps = 4
    while True:
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(reps):
            launch()
        t1.record()
        t1.synchronize()
        total = t0.elapsed_time(t1) * 1e-3
        if total >= min_seconds:
            return total / reps
        reps *= 4


def alternating(forms, names, min_seconds, rounds=3):
    """The best window of every form, the forms taking turns."""
    for n in names:
        forms[n]()
    torch.cuda.synchronize()
    best = {n: float("inf") for n in names}
    for _ in range(rounds):
        for n in names:
            best[n] = min(best[n], window(forms[n], min_seconds))
    return best


def traffic(family, form):
    j, fld, out64 = bytes_per_element(family, 8 if form == "f64" else 4)
    if form == "mixed_state":
        return j + fld + out64 // 2
    if form == "mixed_family+copy":
        return j + fld + out64 + out64 + out64 // 2
    return j + fld + out64


def rows_of(family, E, min_secs, only=FORMS, label=None):
    forms, keep = bound_forms(family, E)
    forms["mixed_state"]()
    torch.cuda.synchronize()
    info = _hip.last_launch_info()
    forms["mixed_family+copy"]()
    torch.cuda.synchronize()
    same_bits = all(torch.equal(keep["outs32"][n], keep["down"][n]) for n in keep["outs32"])
    best = alternating(forms, only, min_secs)
    rows = []
    for form in only:
        per = traffic(family, form)
        rows.append({"family": family, "Np": NP, "Nfp": NFP, "nf": NF, "b": B_FM if family == "facemass" else 1, "E": E,
                     "form": label or form, "seconds": best[form], "bytes_per_element": per, "gbps": per * E / best[form] * 1e-9,
                     "roofline_fraction": per * E / best[form] / HBM_BYTES_PER_S, "bitwise_the_downcast": same_bits,
                     "dword_stores": bool(info.get("dword_stores")) if form == "mixed_state" else None,
                     "plain_field_loads": bool(info.get("plain_field_loads")) if form == "mixed_state" else None})
    del keep, forms
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
                rows += rows_of(family, E + 1, args.min_secs, only=("mixed_state",), label="mixed_state, odd E")
            for r in rows:
                r["copy_route_over_this"] = base["mixed_family+copy"] / r["seconds"]
                line = json.dumps(r)
                print(line, flush=True)
                if sink:
                    sink.write(line + "\n")
                    sink.flush()
    if sink:
        sink.close()


if __name__ == "__main__":
    main()
