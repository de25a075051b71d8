"""Restrict a p = 4 nodal field on tetrahedra to p = 3 and prolong it back (what p-multigrid and p-adaptivity do between
orders): two rectangular element-local operators, ``ij,ej->ei`` with (Ni, Nj) = (20, 35) and (35, 20), on the matrix cores
under ``transform="element_operator"``, checked against numpy.

    python examples/dg_project_orders.py [long_dim_length]
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


def transfer(p_from, p_to):
    """Nodal values of order *p_from* -> the interpolant's values at the nodes of order *p_to*."""
    return vandermonde(p_from, lattice(p_to)) @ np.linalg.inv(vandermonde(p_from, lattice(p_from)))


def operator(name, Ni, Nj):
    return f.einsum("ij,ej->ei", f.array(name, (Ni, Nj)), f.array("u", ("E", Nj)))


def main():
    import torch

    n = int(sys.argv[1]) if len(sys.argv) > 1 else 100_000
    restrict_op, prolong_op = transfer(4, 3), transfer(3, 4)          # (20, 35) and (35, 20)
    assert np.allclose(restrict_op @ prolong_op, np.eye(20), atol=1e-9)  # a p = 3 field survives the round trip
    rng = np.random.default_rng(0)
    u4 = rng.random((n, 35)) * 2 - 1
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")   # noqa: E731
    down, up = operator("R", 20, 35), operator("P", 35, 20)
    for expr in (down, up):
        print(f"'{expr.get_subscripts()}' {expr.arg_to_shape[expr.args[0][0].name]}: auto -> {launch_kind(expr, 'auto', {'E': n})}, "
              f"element_operator -> {launch_kind(expr, 'element_operator', {'E': n})}")
    u3 = f.evaluate(down, 0, {"R": dev(restrict_op), "u": dev(u4)}, transform="element_operator")[down.output_names[0]]
    back = f.evaluate(up, 0, {"P": dev(prolong_op), "u": u3}, transform="element_operator", wait=True)[up.output_names[0]]
    ref3 = u4 @ restrict_op.T
    ref4 = ref3 @ prolong_op.T
    err3 = np.abs(u3.cpu().numpy() - ref3).max() / np.abs(ref3).max()
    err4 = np.abs(back.cpu().numpy() - ref4).max() / np.abs(ref4).max()
    print(f"restriction p4 -> p3: max rel err vs numpy {err3:.2e};  prolongation back: {err4:.2e}  (E = {n})")
    assert err3 < 1e-12 and err4 < 1e-12
    again = f.evaluate(down, 0, {"R": dev(restrict_op), "u": back}, transform="element_operator", wait=True)[down.output_names[0]]
    drift = float((again - u3).abs().max() / u3.abs().max())
    print(f"restrict(prolong(u3)) - u3: {drift:.2e} (the round trip keeps a p = 3 field)")
    assert drift < 1e-9
    for expr in (down, up):
        t = f.timeit(expr, transform="element_operator", cq=0, long_dim_length=n)
        print(f"'{expr.get_subscripts()}' {expr.arg_to_shape[expr.args[0][0].name]}: {t * 1e6:.1f} us per launch")


if __name__ == "__main__":
    main()
