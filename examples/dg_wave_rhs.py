"""The right-hand side of the 3-D DG wave equation, p = 4, as volume term plus lift -- the sum done by the library:

    rhs_u  = div(v)    + lift(F_u)
    rhs_vx = grad_x(u) + lift(F_vx)      (x = 0, 1, 2)

``div`` and ``grad`` write their outputs; the face-mass launch then ADDS the four lifts onto them
(``evaluate(..., alpha=1, beta=1)``) instead of writing four arrays that the caller adds in four more
passes.  The outputs of one batched launch may not overlap, so the three grad planes are three views of the one
``[3][E][Np]`` array (views that merely touch are fine), handed in as three ``out_dict`` entries.  Checked against numpy.

    python examples/dg_wave_rhs.py [E]
"""
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import feinsum_amd as f  # noqa: E402

NP, NF, NFP = 35, 4, 15


def main(E: int = 1000) -> None:
    rng = np.random.default_rng(0)
    host = {"J": rng.standard_normal((3, 3, E)), "D": rng.standard_normal((3, NP, NP)), "u": rng.standard_normal((E, NP)),
            "v": rng.standard_normal((3, E, NP)), "Jf": rng.standard_normal((E, NF)), "R": rng.standard_normal((NF, NP, NFP))}
    host.update({f"F{k}": rng.standard_normal((NF, E, NFP)) for k in range(4)})      # face fluxes of u, vx, vy, vz
    dev = {k: torch.from_numpy(v).cuda() for k, v in host.items()}

    grad = f.einsum("xre,rij,ej->xei", f.array("J", (3, 3, "E")), f.array("D", (3, NP, NP)), f.array("u", ("E", NP)))
    div = f.einsum("xre,rij,xej->ei", f.array("J", (3, 3, "E")), f.array("D", (3, NP, NP)), f.array("v", (3, "E", NP)))
    lift = f.batched_einsum("ef,fij,fej->ei", [[f.array("Jf", ("E", NF)), f.array("R", (NF, NP, NFP)),
                                                f.array(f"F{k}", (NF, "E", NFP))] for k in range(4)])

    rhs_u = f.evaluate(div, 0, dev)["_fe_out"]                     # div(v)
    rhs_v = f.evaluate(grad, 0, dev)["_fe_out"]                    # grad(u): [3][E][Np]
    outs = dict(zip(lift.output_names, [rhs_u, rhs_v[0], rhs_v[1], rhs_v[2]]))
    f.evaluate(lift, 0, dev, out_dict=outs, alpha=1.0, beta=1.0, wait=True)      # ... + lift(F), added in the kernel

    lifts = [np.einsum("ef,fij,fej->ei", host["Jf"], host["R"], host[f"F{k}"]) for k in range(4)]
    want_u = np.einsum("xre,rij,xej->ei", host["J"], host["D"], host["v"]) + lifts[0]
    want_v = np.einsum("xre,rij,ej->xei", host["J"], host["D"], host["u"]) + np.stack(lifts[1:])
    err = max(float(np.abs(rhs_u.cpu().numpy() - want_u).max() / np.abs(want_u).max()),
              float(np.abs(rhs_v.cpu().numpy() - want_v).max() / np.abs(want_v).max()))
    print(f"E = {E}: rhs_u and rhs_v (div / grad + lift, accumulated in the face-mass kernel), max rel err vs numpy {err:.2e}")
    assert err < 1e-12, err


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 1000)
