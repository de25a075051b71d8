"""The discrete energy of a p = 4 field, sum_e J_e u_e^T M u_e ('e,ij,ei,ej->'), as a time-stepping code monitors it:
"auto" runs it as a split reduction over the whole chip (the Gram step 'ej,ei->ji' on the matrix cores, split along
the element axis).

    python examples/dg_wave_energy.py [E]
"""
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import feinsum_amd as f  # noqa: E402
from feinsum_amd.measure import launch_kind  # noqa: E402

NP = 35   # tetrahedra, p = 4


def main(E: int = 1_000_000) -> None:
    expr = f.einsum("e,ij,ei,ej->", f.array("J", ("E",)), f.array("M", (NP, NP)), f.array("u", ("E", NP)),
                    f.array("v", ("E", NP)))
    rng = np.random.default_rng(0)
    A = rng.random((NP, NP))
    host = {"J": rng.random(E) + 0.5, "M": A @ A.T + NP * np.eye(NP), "u": rng.random((E, NP))}
    host["v"] = host["u"]
    dev = {k: torch.from_numpy(v).cuda() for k, v in host.items()}
    energy = f.evaluate(expr, 0, dev, transform="auto", wait=True)["_fe_out"]
    print(f"E = {E}: kernels {launch_kind(expr, 'auto', {'E': E})!r}, energy = {float(energy):.12e}")


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000)
