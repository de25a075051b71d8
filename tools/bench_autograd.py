"""The adjoint kernels against the routes these einsums had before -- "auto" (the generic kernel) and
"contraction" (the optimal schedule as strided contractions) -- in the same process, the operator-gradient kernels
(transform "operator_adjoint") against "auto", and the forward + backward time of evaluate_differentiable under both
settings of operator_gradients.  One JSON line per (case, E, route).
    python tools/bench_autograd.py [--E 100000 1000000] [--reps N]

Seconds per launch by HIP events over --reps back-to-back launches after a warm-up launch, float64, tetrahedra p = 4.
"roofline" is the fraction of 8 TB/s that the algorithmic bytes per element (geometric-factor adjoint
1192 B, face-mass adjoint 1304 B with dJ, 792 B without) would need.
"""
import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import autograd_cases as C  # noqa: E402
import feinsum_amd as f  # noqa: E402
from feinsum_amd import _hip  # noqa: E402
from feinsum_amd.autograd import adjoint_einsums, evaluate_differentiable, output_grad_name  # noqa: E402
from feinsum_amd.measure import _bind  # noqa: E402

BW = 8e12
NP, NF, NFP = 35, 4, 15


def seconds(fn, reps):
    fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) * 1e-3 / reps


def device_inputs(einsum, E, seed=0):
    rng = np.random.default_rng(seed)
    out = {}
    for name in sorted(einsum.all_args):
        shape = C.concrete(einsum.arg_to_shape[name], E)
        out[name] = torch.from_numpy(rng.standard_normal(shape)).cuda()
    return out


def bound_seconds(einsum, args, transform, reps):
    q, bound, _ = _bind(einsum, 0, args, None, transform)
    s = q.stream_ptr
    return seconds(lambda: bound.launch(s), reps)


def emit(**kw):
    print(json.dumps(kw), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--E", type=int, nargs="+", default=[100000, 1000000])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--old-reps", type=int, default=3, help="repetitions of the existing (slow) routes")
    a = ap.parse_args()
    (gj,) = adjoint_einsums(C.grad(3, NP), "J")
    fm = C.face_mass(NP, NF, NFP, 1)
    (fv,) = adjoint_einsums(fm, "v0")
    (fj,) = adjoint_einsums(fm, "J")
    for E in a.E:
        # geometric-factor adjoint 'rij,ej,xei->xre' (grad's J-gradient)
        args = device_inputs(gj, E)
        per = {}
        for route in ("adjoint", "auto", "contraction"):
            sec = bound_seconds(gj, args, route, a.reps if route == "adjoint" else a.old_reps)
            per[route] = sec
            emit(case="geomadj", einsum=gj.get_subscripts(), E=E, route=route, seconds=sec,
                 roofline=1192 * E / BW / sec)
        emit(case="geomadj", E=E, speedup_vs_best_existing=min(per["auto"], per["contraction"]) / per["adjoint"])
        del args
        # face-mass adjoint without dJ: 'ef,fij,ei->fej'
        args = device_inputs(fv, E, 1)
        per = {}
        for route in ("adjoint", "auto", "contraction"):
            sec = bound_seconds(fv, args, route, a.reps if route == "adjoint" else a.old_reps)
            per[route] = sec
            emit(case="facemass_adj_v", einsum=fv.get_subscripts(), E=E, route=route, seconds=sec,
                 roofline=792 * E / BW / sec)
        emit(case="facemass_adj_v", E=E, speedup_vs_best_existing=min(per["auto"], per["contraction"]) / per["adjoint"])
        # face-mass adjoint with dJ, one launch; the existing routes need the v- and the J-einsum
        argsj = dict(device_inputs(fj, E, 2), **{output_grad_name("_fe_out"): args[output_grad_name("_fe_out")]})
        J, R, g, v = args["J"], args["R"], args[output_grad_name("_fe_out")], argsj["v0"]
        dv, dJ = torch.empty_like(v), torch.empty_like(J)
        s = torch.cuda.current_stream().cuda_stream
        fused = seconds(lambda: _hip.facemass_adj(J.data_ptr(), R.data_ptr(), [g.data_ptr()], [v.data_ptr()],
                                                  [dv.data_ptr()], dJ.data_ptr(), E, NP, NF, NFP, stream=s), a.reps)
        emit(case="facemass_adj_dJ", E=E, route="adjoint (one launch)", seconds=fused, roofline=1304 * E / BW / fused)
        best = min(per["auto"], per["contraction"])
        bestj = min(bound_seconds(fj, argsj, r, a.old_reps) for r in ("auto", "contraction"))
        emit(case="facemass_adj_dJ", E=E, route="best existing (v-einsum + J-einsum)", seconds=best + bestj,
             roofline=1304 * E / BW / (best + bestj))
        emit(case="facemass_adj_dJ", E=E, speedup_vs_best_existing=(best + bestj) / fused)
        del args, argsj, dv, dJ
        # operator gradients: dD 'xre,ej,xei->rij' and dR 'ef,fej,ei->fij' (b = 4, a launch per row under both transforms)
        for case, fwd_e, wrt, nbytes in (("opgrad_d", C.grad(3, NP), "D", 1192),
                                         ("opgrad_r_b4", C.face_mass(NP, NF, NFP, 4), "R", 8 * (4 * (NP + NF * NFP) + NF))):
            (term,) = adjoint_einsums(fwd_e, wrt)
            args = device_inputs(term, E, 4)
            per = {}
            for route in ("operator_adjoint", "auto"):
                per[route] = bound_seconds(term, args, route, a.reps if route == "operator_adjoint" else a.old_reps)
                emit(case=case, einsum=term.get_subscripts(), E=E, route=route, seconds=per[route],
                     roofline=nbytes * E / BW / per[route])
            emit(case=case, E=E, speedup_vs_auto=per["auto"] / per["operator_adjoint"])
            del args
        # forward + backward of evaluate_differentiable
        for name, ein, og in [(n, e, og) for n, e in (("grad", C.grad(3, NP)), ("facemass_b4", C.face_mass(NP, NF, NFP, 4)))
                              for og in ("auto", "kernel")]:
            dev = device_inputs(ein, E, 3)
            for t in dev.values():
                t.requires_grad_(True)
            gbar = [torch.ones(C.concrete(ein.shape, E), dtype=torch.float64, device="cuda") for _ in ein.output_names]

            def step():
                for t in dev.values():
                    t.grad = None
                outs = evaluate_differentiable(ein, 0, dev, operator_gradients=og)
                torch.autograd.backward([outs[n] for n in ein.output_names], gbar)

            fwd = seconds(lambda: evaluate_differentiable(ein, 0, {n: t.detach() for n, t in dev.items()}), a.reps)
            both = seconds(step, max(3, a.reps // 4))
            emit(case=f"{name} forward + backward (all inputs)", operator_gradients=og, E=E, forward_seconds=fwd,
                 forward_backward_seconds=both)
            del dev
        torch.cuda.empty_cache()
    emit(device=f.DeviceQueue(0).device.name)


if __name__ == "__main__":
    main()
