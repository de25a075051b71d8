"""The c^2-weighted mass term of the wave operator on tetrahedra at p = 4, four fields under one coefficient: interpolate the
35 nodal values of every element to 56 quadrature points, multiply by W[e, q] = w_q c^2(x_q) detJ[e], project back with the
transposed interpolation -- ``qi,eq,qj,ej->ei``, the same array in both operator positions -- in ONE matrix-core launch under
``transform="weighted_element_operator"``, checked against ``numpy.einsum``.

    python examples/dg_wave_variable_speed.py [long_dim_length]
"""
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

import feinsum_amd as f  # noqa: E402
from feinsum_amd.measure import launch_kind  # noqa: E402


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
    origin, det = rng.random((n, 3)), 0.5 + rng.random(n)                         # where an element lies, its Jacobian determinant
    xq = origin[:, None, :] + 0.1 * grid[None, :, :]
    c2 = 1.0 + 0.5 * np.sin(2 * np.pi * xq[..., 0]) * np.cos(2 * np.pi * xq[..., 1]) + 0.25 * xq[..., 2]   # c^2 at the points
    W = (1.0 / 6.0 / Nq) * c2 * det[:, None]
    fields = [rng.random((n, Np)) * 2 - 1 for _ in range(b)]

    A, Wa = f.array("A", (Nq, Np)), f.array("W", ("E", Nq))
    expr = f.batched_einsum("qi,eq,qj,ej->ei", [[A, Wa, A, f.array(f"u{k}", ("E", Np))] for k in range(b)])
    print(f"'{expr.get_subscripts()}' x {b}, (Ni, Nq, Nj) = ({Np}, {Nq}, {Np}): auto -> {launch_kind(expr, 'auto', {'E': n})}, "
          f"weighted_element_operator -> {launch_kind(expr, 'weighted_element_operator', {'E': n})}")
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")   # noqa: E731
    arrays = {"A": dev(interp), "W": dev(W), **{f"u{k}": dev(u) for k, u in enumerate(fields)}}
    got = f.evaluate(expr, 0, arrays, transform="weighted_element_operator", wait=True)
    worst = 0.0
    for k, name in enumerate(expr.output_names):
        ref = np.einsum("qi,eq,qj,ej->ei", interp, W, interp, fields[k], optimize=True)
        worst = max(worst, np.abs(got[name].cpu().numpy() - ref).max() / np.abs(ref).max())
    print(f"c^2-weighted mass term of {b} fields: max rel err vs numpy.einsum {worst:.2e}  (E = {n})")
    assert worst < 1e-12
    # the weighted mass matrix is symmetric positive definite: u . M u > 0 for every field
    energy = [float((arrays[f"u{k}"] * got[name]).sum()) for k, name in enumerate(expr.output_names)]
    print("u . M u per field:", " ".join(f"{x:.6e}" for x in energy))
    assert min(energy) > 0
    t = f.timeit(expr, transform="weighted_element_operator", cq=0, long_dim_length=n)
    print(f"one launch for {b} fields: {t * 1e6:.1f} us")


if __name__ == "__main__":
    main()
