"""Estimating the coefficient c^2 of the wave operator from data: one misfit 1/2 ||M(c^2) u - d||^2 over four fields, M the
c^2-weighted mass term of tetrahedra at p = 4 (``qi,eq,qj,ej->ei``, examples/dg_wave_variable_speed.py), and its gradient with
respect to the weight W[e, q] = w_q c^2(x_q) detJ[e] and to the fields -- forward and backward on the matrix cores:
``evaluate_differentiable(..., transform="weighted_element_operator", element_gradients="kernel")``.
The gradient is checked against a central finite difference of the misfit along a random direction.

    python examples/dg_wave_speed_inversion.py [long_dim_length]
"""
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

import feinsum_amd as f  # noqa: E402
from feinsum_amd import autograd  # noqa: E402


def lattice(p):
    """The (p + 1)(p + 2)(p + 3) / 6 equispaced nodes of the reference tetrahedron."""
    return np.array([(a / p, b / p, c / p) for a in range(p + 1) for b in range(p + 1 - a) for c in range(p + 1 - a - b)])


def vandermonde(p, nodes):
    """Monomials x^a y^b z^c, a + b + c <= p, at *nodes*."""
    x, y, z = nodes.T
    return np.stack([x**a * y**b * z**c for a in range(p + 1) for b in range(p + 1 - a) for c in range(p + 1 - a - b)], axis=1)


def main():
    import torch

    n = int(sys.argv[1]) if len(sys.argv) > 1 else 100_000
    p, b = 4, 4
    grid = lattice(5) * 0.9 + 0.025                      # 56 points inside the reference tetrahedron (weights: equal)
    interp = vandermonde(p, grid) @ np.linalg.inv(vandermonde(p, lattice(p)))     # (56, 35): nodal values -> values at the points
    Nq, Np = interp.shape
    rng = np.random.default_rng(0)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")   # noqa: E731
    S = dev(interp)
    W_true, W_guess = dev(0.5 + rng.random((n, Nq))), dev(0.5 + rng.random((n, Nq)))
    fields = [dev(rng.random((n, Np)) * 2 - 1) for _ in range(b)]

    A, Wa = f.array("A", (Nq, Np)), f.array("W", ("E", Nq))
    expr = f.batched_einsum("qi,eq,qj,ej->ei", [[A, Wa, A, f.array(f"u{k}", ("E", Np))] for k in range(b)])

    def mass(W, us):
        outs = f.evaluate_differentiable(expr, 0, {"A": S, "W": W, **{f"u{k}": u for k, u in enumerate(us)}},
                                         transform="weighted_element_operator", element_gradients="kernel")
        return [outs[name] for name in expr.output_names]

    data = [d.detach() for d in mass(W_true, fields)]

    def misfit(W, us):
        return sum(0.5 * ((m - d) ** 2).sum() for m, d in zip(mass(W, us), data))

    W = W_guess.clone().requires_grad_(True)
    us = [u.clone().requires_grad_(True) for u in fields]
    autograd.launch_counts.clear()
    value = misfit(W, us)
    value.backward()
    torch.cuda.synchronize()
    start = float(value.detach())
    print(f"misfit {start:.6e} over {b} fields, E = {n}; backward pass: {dict(autograd.launch_counts)}")
    assert autograd.launch_counts == {"weighted_w": 1, "weighted_u": 1}, autograd.launch_counts

    # directional finite differences: (J(x + h v) - J(x - h v)) / 2 h against <grad J, v>
    with torch.no_grad():
        vW = dev(rng.random((n, Nq)) * 2 - 1)
        vu = [dev(rng.random((n, Np)) * 2 - 1) for _ in range(b)]
        slope = float((W.grad * vW).sum() + sum((u.grad * v).sum() for u, v in zip(us, vu)))
        for h in (1e-3, 1e-4, 1e-5):
            up = misfit(W_guess + h * vW, [u + h * v for u, v in zip(fields, vu)])
            down = misfit(W_guess - h * vW, [u - h * v for u, v in zip(fields, vu)])
            fd = float(up - down) / (2 * h)
            print(f"h = {h:.0e}: finite difference {fd:.10e}, <gradient, direction> {slope:.10e}, relative difference {abs(fd - slope) / abs(slope):.2e}")
        assert abs(fd - slope) <= 1e-6 * abs(slope)

    # one step of steepest descent on W with the exact line search of a quadratic (M is linear in W: M(g) u is the
    # directional derivative of the residual) lowers the misfit
    with torch.no_grad():
        step = float((W.grad ** 2).sum()) / float(sum((m ** 2).sum() for m in mass(W.grad, fields)))
        lower = float(misfit(W_guess - step * W.grad, fields))
    print(f"after one descent step on W: misfit {lower:.6e}")
    assert lower < start


if __name__ == "__main__":
    main()
