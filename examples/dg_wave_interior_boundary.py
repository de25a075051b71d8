"""Two element ranges of the same arrays on two streams: the elements that touch a partition boundary first -- their
results feed the halo exchange -- and the interior while that exchange would run.  grad, div and the lift of four face
fields at p = 4 are evaluated on ``[0, split)`` and ``[split, Nel)`` of the SAME input and output arrays, handed to the
library as ``narrow`` views (element slices: no copies in, no copies out), and the outputs are compared bitwise with the
launches on the whole arrays.

Why the split is a multiple of 80 elements: the kernels work in wave tiles of 16 M elements (M = 1 ... 5 by family and order,
80 the largest) and a tile's bits do not depend on where it lies, but the elements behind a launch's LAST full tile are summed
entry by entry in another order.  With the split on a tile boundary both ranges cut the element axis into the tiles and the
remainder the whole launch has, so every entry is computed by the same code in the same order; any other split moves some
elements between "tile" and "remainder" and agrees to rounding only.

    python examples/dg_wave_interior_boundary.py [Nel] [split]
"""
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

import torch  # noqa: E402

import feinsum_amd as f  # noqa: E402
from feinsum_amd import _hip  # noqa: E402

NP, NF, NFP = 35, 4, 15
TILE = 80


def einsums():
    J, D = f.array("J", (3, 3, "Nel")), f.array("D", (3, NP, NP))
    grad = f.einsum("xre,rij,ej->xei", J, D, f.array("p", ("Nel", NP)))
    div = f.einsum("xre,rij,xej->ei", J, D, f.array("v", (3, "Nel", NP)))
    lift = f.batched_einsum("fe,fij,fej->ei", [[f.array("Jf", (NF, "Nel")), f.array("L", (NF, NP, NFP)),
                                                f.array(f"flux{k}", (NF, "Nel", NFP))] for k in range(4)])
    return {"grad": grad, "div": div, "lift": lift}


def element_axis(expr, name=None):
    """The element axis of an argument (or of the outputs), or None."""
    shape = expr.shape if name is None else expr.arg_to_shape[name]
    return next((k for k, d in enumerate(shape) if isinstance(d, f.SizeParam)), None)


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 20_003
    split = int(sys.argv[2]) if len(sys.argv) > 2 else 4 * TILE
    assert 0 < split < n and split % TILE == 0, "the boundary range ends on a tile boundary (see the module docstring)"
    gen = torch.Generator(device="cpu").manual_seed(0)
    boundary, interior = (f.DeviceQueue(0, stream=torch.cuda.Stream()) for _ in range(2))
    for name, expr in einsums().items():
        arrays = {a.name: torch.rand([n if isinstance(d, f.SizeParam) else int(d) for d in a.shape], generator=gen,
                                     dtype=torch.float64).cuda() for row in expr.args for a in row}
        whole = f.evaluate(expr, 0, arrays, wait=True)
        out_axis = element_axis(expr)
        outs = {o: torch.full_like(t, float("nan")) for o, t in whole.items()}
        torch.cuda.synchronize()
        slices = 0
        for q, (a, m) in ((boundary, (0, split)), (interior, (split, n - split))):
            part = {k: (t if element_axis(expr, k) is None else t.narrow(element_axis(expr, k), a, m)) for k, t in arrays.items()}
            f.evaluate(expr, q, part, out_dict={o: t.narrow(out_axis, a, m) for o, t in outs.items()})
            slices += _hip.last_launch_info().get("element_slice", False)
        boundary.finish()
        interior.finish()
        same = all(torch.equal(outs[o].view(torch.int64), whole[o].view(torch.int64)) for o in whole)
        assert same, name
        print(f"{name:5s} {expr.get_subscripts()} x {expr.b}: elements [0, {split}) and [{split}, {n}) on two streams, "
              f"{slices} of 2 launches on element slices, outputs bitwise those of the whole-array launch")


if __name__ == "__main__":
    main()
