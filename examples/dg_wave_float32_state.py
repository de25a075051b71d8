"""A few low-storage Runge-Kutta stages of the DG wave system  dp/dt = -div v,  dv/dt = -grad p  at p = 4 with a float32 STATE
(p, v and the residuals) and float64 geometry factors J and operator D, twice:

  * transform ``"mixed_state"``: the kernels read the float32 fields, compute in float64 and store float32 results;
  * transform ``"mixed_family"`` (float64 results) followed by the downcast pass a float32 solver needs without it.

The launches of each route are printed, and the two states are checked to have the same bits.

    python examples/dg_wave_float32_state.py [long_dim_length] [steps]
"""
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

import torch  # noqa: E402

import feinsum_amd as f  # noqa: E402
from feinsum_amd import _hip  # noqa: E402

NP = 35
# the five stages of Carpenter & Kennedy's 2N-storage RK4
RK_A = (0.0, -567301805773.0 / 1357537059087.0, -2404267990393.0 / 2016746695238.0, -3550918686646.0 / 2091501179385.0,
        -1275806237668.0 / 842570457699.0)
RK_B = (1432997174477.0 / 9575080441755.0, 5161836677717.0 / 13612068292357.0, 1720146321549.0 / 2090206949498.0,
        3134564353537.0 / 4481467310338.0, 2277821191437.0 / 14882151754819.0)


def einsums():
    J, D = f.array("J", (3, 3, "Nel")), f.array("D", (3, NP, NP))
    return (f.einsum("xre,rij,xej->ei", J, D, f.array("v", (3, "Nel", NP), "float32")),
            f.einsum("xre,rij,ej->xei", J, D, f.array("p", ("Nel", NP), "float32")))


def run(route, n, steps, J, D, p0, v0, dt):
    """*steps* RK steps; returns (p, v, launches of one stage)."""
    div, grad = einsums()
    p, v = p0.clone(), v0.clone()
    kp, kv = torch.zeros_like(p), torch.zeros_like(v)
    launches = []
    for step in range(steps):
        for a, b in zip(RK_A, RK_B):
            if route == "mixed_state":
                dp = f.evaluate(div, 0, {"J": J, "D": D, "v": v}, transform="mixed_state")["_fe_out"]
                info_d = _hip.last_launch_info()
                dv = f.evaluate(grad, 0, {"J": J, "D": D, "p": p}, transform="mixed_state")["_fe_out"]
                info_g = _hip.last_launch_info()
                if not launches:
                    for name, info in (("div", info_d), ("grad", info_g)):
                        launches.append(f"{name}: fe_{name}3d_mixed_state_f64 (float32 results by "
                                        f"{'4-byte' if info['dword_stores'] else '16-byte'} stores)")
            else:
                dp64 = f.evaluate(div, 0, {"J": J, "D": D, "v": v}, transform="mixed_family")["_fe_out"]
                dv64 = f.evaluate(grad, 0, {"J": J, "D": D, "p": p}, transform="mixed_family")["_fe_out"]
                dp, dv = dp64.to(torch.float32), dv64.to(torch.float32)          # the pass "mixed_state" saves
                if not launches:
                    launches += ["div: fe_div3d_mixed_f64 (float64 results)", "downcast pass of div's output",
                                 "grad: fe_grad3d_mixed_f64 (float64 results)", "downcast pass of grad's three planes"]
            kp.mul_(a).add_(dp, alpha=-dt)
            kv.mul_(a).add_(dv, alpha=-dt)
            p.add_(kp, alpha=b)
            v.add_(kv, alpha=b)
    torch.cuda.synchronize()
    return p, v, launches


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 20_001
    steps = int(sys.argv[2]) if len(sys.argv) > 2 else 2
    gen = torch.Generator(device="cuda").manual_seed(0)
    J = torch.rand((3, 3, n), dtype=torch.float64, device="cuda", generator=gen) - 0.5
    D = torch.rand((3, NP, NP), dtype=torch.float64, device="cuda", generator=gen) - 0.5
    p0 = (torch.rand((n, NP), dtype=torch.float64, device="cuda", generator=gen) - 0.5).to(torch.float32)
    v0 = (torch.rand((3, n, NP), dtype=torch.float64, device="cuda", generator=gen) - 0.5).to(torch.float32)
    results = {}
    for route in ("mixed_state", "mixed_family"):
        p, v, launches = run(route, n, steps, J, D, p0, v0, dt=1e-3)
        results[route] = (p, v)
        print(f"{route}: per stage {len(launches)} launches")
        for line in launches:
            print("   ", line)
    same = all(torch.equal(a, b) for a, b in zip(results["mixed_state"], results["mixed_family"]))
    print(f"{steps} steps of {len(RK_A)} stages at {n} elements: the two states have {'the same bits' if same else 'DIFFERENT bits'}")
    assert same and all(t.dtype == torch.float32 for t in results["mixed_state"])


if __name__ == "__main__":
    main()
