"""The gradient of a least-squares misfit through a DG operator, as an inverse problem needs it: the weak gradient of a
p = 4 field (grad 'xre,rij,ej->xei') plus the lift of its face fluxes (face-mass 'ef,fij,fej->ei' x 3), against data,

    loss = 1/2 sum |grad(J, u) - d_grad|^2 + 1/2 sum_k |lift_k(Jf, v_k) - d_k|^2,

differentiated with respect to the field u, the volume geometric factors J and the face Jacobians Jf by
``evaluate_differentiable`` and ``torch.autograd`` (the J- and face-adjoints run on the adjoint kernels),
then checked against a central finite difference along a random direction.

    python examples/dg_wave_adjoint.py [E] [--operators]

``--operators`` also differentiates with respect to the operator matrices D and L, on the operator-gradient kernels
(``operator_gradients="kernel"``).
"""
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import feinsum_amd as f  # noqa: E402

NP, NF, NFP = 35, 4, 15


def main(E: int = 100_000, operators: bool = False) -> None:
    grad = f.einsum("xre,rij,ej->xei", f.array("J", (3, 3, "E")), f.array("D", (3, NP, NP)), f.array("u", ("E", NP)))
    lift = f.batched_einsum("ef,fij,fej->ei", [[f.array("Jf", ("E", NF)), f.array("L", (NF, NP, NFP)),
                                                f.array(f"v{k}", (NF, "E", NFP))] for k in range(3)])
    rng = np.random.default_rng(0)
    host = {"J": rng.standard_normal((3, 3, E)), "D": rng.standard_normal((3, NP, NP)) / NP,
            "u": rng.standard_normal((E, NP)), "Jf": rng.random((E, NF)) + 0.5,
            "L": rng.standard_normal((NF, NP, NFP)) / NFP}
    host.update({f"v{k}": rng.standard_normal((NF, E, NFP)) for k in range(3)})
    data_grad = torch.from_numpy(rng.standard_normal((3, E, NP))).cuda()
    data_lift = [torch.from_numpy(rng.standard_normal((E, NP))).cuda() for _ in range(3)]
    dev = {k: torch.from_numpy(v).cuda() for k, v in host.items()}
    wrt = ("u", "J", "Jf") + (("D", "L") if operators else ())
    og = "kernel" if operators else "auto"
    for k in wrt:
        dev[k].requires_grad_(True)

    def loss(arrays):
        g = f.evaluate_differentiable(grad, 0, {k: arrays[k] for k in ("J", "D", "u")}, operator_gradients=og)["_fe_out"]
        outs = f.evaluate_differentiable(lift, 0, {k: arrays[k] for k in lift.all_args}, operator_gradients=og)
        val = 0.5 * ((g - data_grad) ** 2).sum()
        for name, d in zip(lift.output_names, data_lift):
            val = val + 0.5 * ((outs[name] - d) ** 2).sum()
        return val

    value = loss(dev)
    value.backward()
    direction = {k: torch.from_numpy(rng.standard_normal(host[k].shape)).cuda() for k in wrt}
    slope = sum(float((dev[k].grad * direction[k]).sum()) for k in wrt)
    h = 1e-3   # the loss is a quartic along the direction: the central difference is off by O(h^2)
    with torch.no_grad():
        plus = {k: (t + h * direction[k] if k in wrt else t) for k, t in dev.items()}
        minus = {k: (t - h * direction[k] if k in wrt else t) for k, t in dev.items()}
        fd = (float(loss(plus)) - float(loss(minus))) / (2 * h)
    rel = abs(fd - slope) / abs(fd)
    print(f"E = {E}: loss {float(value.detach()):.6e}, <grad, dir> = {slope:.10e}, finite difference {fd:.10e}, rel diff {rel:.1e}")
    assert rel < 1e-5, rel


if __name__ == "__main__":
    argv = [a for a in sys.argv[1:] if a != "--operators"]
    main(int(argv[0]) if argv else 100_000, operators="--operators" in sys.argv[1:])
