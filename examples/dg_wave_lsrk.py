"""One low-storage Runge-Kutta stage of the 3-D DG wave operator at p = 4, written with accumulating evaluations
(``evaluate(..., alpha=, beta=)``):

    k_p <- a k_p + dt (div(v) + lift(F_p))           k_v <- a k_v + dt (grad(p) + lift(F_v))

Three evaluations add onto the stage arrays: div and grad with ``(alpha, beta) = (dt, a)`` -- they carry the ``a k`` part --
and then the lift of all four face fields with ``(dt, 1)``.  Under ``transform={"accumulate": "epilogue"}`` grad and div accumulate inside
their matrix-core kernels, as the lift always does.  Checked against numpy, and the route of every launch is printed.

    python examples/dg_wave_lsrk.py [long_dim_length]
"""
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

import feinsum_amd as f  # noqa: E402
from feinsum_amd.measure import _bind  # noqa: E402

NP, NF, NFP = 35, 4, 15
EPILOGUE = {"accumulate": "epilogue"}


def einsums():
    J, D = f.array("J", (3, 3, "E")), f.array("D", (3, NP, NP))
    div = f.einsum("xre,rij,xej->ei", J, D, f.array("v", (3, "E", NP)))
    grad = f.einsum("xre,rij,ej->xei", J, D, f.array("p", ("E", NP)))
    lift = f.batched_einsum("ef,fij,fej->ei", [[f.array("Jf", ("E", NF)), f.array("R", (NF, NP, NFP)), f.array(n, (NF, "E", NFP))]
                                               for n in ("Fp", "Fv0", "Fv1", "Fv2")])
    return div, grad, lift


def main():
    E = int(sys.argv[1]) if len(sys.argv) > 1 else 1003
    a, dt = -0.4178904745, 1.25e-3                    # a stage coefficient of Carpenter & Kennedy's LSRK4(5), a time step
    rng = np.random.default_rng(0)
    shapes = {"J": (3, 3, E), "D": (3, NP, NP), "v": (3, E, NP), "p": (E, NP), "Jf": (E, NF), "R": (NF, NP, NFP),
              "Fp": (NF, E, NFP), "Fv0": (NF, E, NFP), "Fv1": (NF, E, NFP), "Fv2": (NF, E, NFP)}
    host = {n: rng.standard_normal(s) for n, s in shapes.items()}
    k_p0, k_v0 = rng.standard_normal((E, NP)), rng.standard_normal((3, E, NP))
    dev = {n: torch.from_numpy(x).cuda() for n, x in host.items()}
    k_p, k_v = (torch.from_numpy(x).cuda() for x in (k_p0, k_v0))
    div, grad, lift = einsums()

    def step(name, expr, outs, alpha, beta, transform=None):
        q, bound, _ = _bind(expr, 0, dev, dict(zip(expr.output_names, outs)), transform, alpha=alpha, beta=beta)
        bound.launch(q.stream_ptr)
        print(f"{name:28s} alpha = {alpha:<10g} beta = {beta:<14g} route: {bound.accumulate}")

    step("k_p <- a k_p + dt div(v)", div, [k_p], dt, a, EPILOGUE)
    step("k_v <- a k_v + dt grad(p)", grad, [k_v], dt, a, EPILOGUE)
    step("k   += dt lift(F)", lift, [k_p, k_v[0], k_v[1], k_v[2]], dt, 1.0)
    torch.cuda.synchronize()

    h = host
    lift_np = lambda F: np.einsum("ef,fij,fej->ei", h["Jf"], h["R"], F)   # noqa: E731
    want_p = a * k_p0 + dt * (np.einsum("xre,rij,xej->ei", h["J"], h["D"], h["v"]) + lift_np(h["Fp"]))
    want_v = a * k_v0 + dt * (np.einsum("xre,rij,ej->xei", h["J"], h["D"], h["p"])
                              + np.stack([lift_np(h[f"Fv{x}"]) for x in range(3)]))
    worst = 0.0
    for got, want in ((k_p, want_p), (k_v, want_v)):
        worst = max(worst, float(np.abs(got.cpu().numpy() - want).max() / np.abs(want).max()))
    assert worst < 1e-12, worst
    print(f"one LSRK stage at E = {E}: max error against numpy {worst:.2e} (relative to the largest entry)")


if __name__ == "__main__":
    main()
