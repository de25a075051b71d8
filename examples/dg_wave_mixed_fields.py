"""A DG wave right-hand side whose STATE is float32 while the geometry factors and the operators stay float64: div and grad
of the fields and the lift of four face fields at p = 4, through the transform ``"mixed_family"`` (float32 fields are widened
as they are read, every product and sum is float64 on the matrix cores), checked against numpy.  The route each call takes is
printed next to the one ``"auto"`` takes for the same einsum.

    python examples/dg_wave_mixed_fields.py [long_dim_length]
"""
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import feinsum_amd as f  # noqa: E402
from feinsum_amd import _hip  # noqa: E402
from feinsum_amd.measure import launch_kind  # noqa: E402

NP, NF, NFP = 35, 4, 15


def einsums():
    J, D = f.array("J", (3, 3, "Nel")), f.array("D", (3, NP, NP))
    div = f.einsum("xre,rij,xej->ei", J, D, f.array("v", (3, "Nel", NP), "float32"))
    grad = f.einsum("xre,rij,ej->xei", J, D, f.array("p", ("Nel", NP), "float32"))
    lift = f.batched_einsum("ef,fij,fej->ei", [[f.array("Jf", ("Nel", NF)), f.array("L", (NF, NP, NFP)),
                                                f.array(f"flux{k}", (NF, "Nel", NFP), "float32")] for k in range(4)])
    return {"div": div, "grad": grad, "lift": lift}


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 20_000
    rng = np.random.default_rng(0)
    for name, expr in einsums().items():
        host = {a.name: rng.uniform(-1, 1, [n if isinstance(d, f.SizeParam) else int(d) for d in a.shape]).astype(a.dtype)
                for row in expr.args for a in row}
        dev = {k: torch.from_numpy(v).cuda() for k, v in host.items()}
        outs = f.evaluate(expr, 0, dev, transform="mixed_family", wait=True)
        info = _hip.last_launch_info()
        worst = 0.0
        for out_name, row in zip(expr.output_names, expr.args):
            ref = np.einsum(expr.get_subscripts(), *[host[a.name].astype(np.float64) for a in row], optimize="optimal")
            got = outs[out_name].cpu().numpy()
            assert got.dtype == np.float64
            worst = max(worst, float(np.abs(got - ref).max() / np.abs(ref).max()))
        assert worst < 1e-13, (name, worst)
        form = "4-byte register loads" if info["plain_field_loads"] else "16-byte LDS-DMA"
        print(f"{name:5s} {expr.get_subscripts()} x {expr.b}: transform 'mixed_family' -> {launch_kind(expr, 'mixed_family', {'Nel': n})}"
              f" (float32 fields by {form}; {info['blocks']} blocks, {info['tiles']} tiles), 'auto' -> "
              f"{launch_kind(expr, 'auto', {'Nel': n})}; max error / max |ref| = {worst:.2e}")


if __name__ == "__main__":
    main()
