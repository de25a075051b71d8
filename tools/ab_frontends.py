#!/usr/bin/env python
"""Two builds of the library on the same calls, bit for bit:

    python tools/ab_frontends.py <parent.so> <child.so>            # compare; exit status 1 on any difference
    python tools/ab_frontends.py --enqueue <lib.so>                # the host cost of a launch, per form

The calls are those of tests/test_gpu_field_groups.py (orders p = 4 and p = 1; plain, prepared, accumulating, slice and
float32-field forms; one wave tile plus three elements and one tile minus one; every field count that falls into groups
differently) and, at p = 4, E = 100 000 and 1 000 004 with b = 1 and b = 4.  Each library runs in a fresh process of its own
(FEINSUM_HIP_LIB) and prints per call the SHA-256 of its outputs (seeded inputs) and the dict of last_launch_info(), and at the
end the sorted lines of kernel_resources().  The two must agree on every line.  A record, not a test: the digests go stale with
the next change of a kernel.

--enqueue: grad p = 4, one field, E = one wave tile -- a launch that measures the host path: microseconds per launch over
2 000 launches through fe_time_launches (plain, accumulating, float32 fields) or a loop of calls of the entry point (slice,
which fe_launch does not route), under a host clock that ends in a synchronise; 25 batches, the fastest (and the median)."""
from __future__ import annotations

import ctypes
import hashlib
import importlib.util
import os
import statistics
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
BIG = (100_000, 1_000_004)


for _p in (ROOT, ROOT / "tests"):     # the package, and tests/dg.py for the cases
    if str(_p) not in sys.path:
        sys.path.insert(0, str(_p))


def _cases_module():
    spec = importlib.util.spec_from_file_location("field_group_cases", ROOT / "tests" / "test_gpu_field_groups.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def worker():
    import torch

    from feinsum_amd import _hip
    from feinsum_amd.family import FAMILY_DIV, FAMILY_FACEMASS, FAMILY_GRAD

    g = _cases_module()
    names = {FAMILY_GRAD: "grad", FAMILY_DIV: "div", FAMILY_FACEMASS: "face-mass"}
    calls = []
    for family in names:
        for form in g.FORMS:
            for order in g.ORDERS:
                tile = g._tile(family, order)
                fields = (1, 2, 4, 5, 9) if family == FAMILY_FACEMASS else (1, 8, 9)
                calls += [(family, form, order, E, b) for E in (tile + 3, tile - 1) for b in fields]
            calls += [(family, form, "p4", E, b) for E in BIG for b in (1, 4)]
    for family, form, order, E, b in calls:
        Np, Nfp = g.ORDERS[order][:2]
        rc, outs, _ = g._run(family, form, Np, Nfp, E, b, seed=1000 * (E % 100_000) + b, reference=False)
        digest = hashlib.sha256()
        for o in outs:
            digest.update(o.contiguous().cpu().numpy())
        info = _hip.last_launch_info() if rc == 0 else {}
        print(f"{names[family]} {form} {order} E={E} b={b} rc={rc} sha256={digest.hexdigest()} launch={info}", flush=True)
        del outs
        torch.cuda.empty_cache()
    print("== kernel_resources")
    print("\n".join(sorted(_hip.kernel_resources().splitlines())), flush=True)


def enqueue():
    import torch

    from feinsum_amd import _hip
    from feinsum_amd.family import FAMILY_GRAD

    lib = _hip.load_library()
    stream = torch.cuda.current_stream().cuda_stream
    E, Np, n = 16, 35, 2000
    gen = torch.Generator(device="cuda").manual_seed(1)
    J, D = torch.rand(3, 3, E, dtype=torch.float64, device="cuda", generator=gen), torch.rand(3, Np, Np, dtype=torch.float64, device="cuda", generator=gen)
    u = torch.rand(E, Np, dtype=torch.float64, device="cuda", generator=gen)
    u32, out = u.float(), torch.zeros(3, E, Np, dtype=torch.float64, device="cuda")
    for form, family, field in (("plain", FAMILY_GRAD, u), ("accumulating", FAMILY_GRAD | _hip.FAMILY_ACC, u),
                                ("slice", None, u), ("float32 fields", FAMILY_GRAD | _hip.FAMILY_FIELDS_F32, u32)):
        vt, ot = _hip._ptr_array([field.data_ptr()]), _hip._ptr_array([out.data_ptr()])
        pack = _hip.ArgPack()
        pack.J, pack.D, pack.u, pack.out, pack.v, pack.outs = J.data_ptr(), D.data_ptr(), field.data_ptr(), out.data_ptr(), vt, ot
        pack.E, pack.Np, pack.b, pack.ndim, pack.alpha, pack.beta = E, Np, 1, 3, 0.5, 0.0
        ms = ctypes.c_float()

        def batch():
            if family is None:
                for _ in range(n):
                    rc = lib.fe_grad3d_strided_f64(J.data_ptr(), E, D.data_ptr(), vt, ot, E, E, Np, 1, 0, stream)
                    if rc:
                        _hip.check(rc)
            else:
                _hip.check(lib.fe_time_launches(family, ctypes.byref(pack), n, stream, ctypes.byref(ms)))

        batch()
        torch.cuda.synchronize()
        times = []
        for _ in range(25):
            t0 = time.perf_counter()
            batch()
            torch.cuda.synchronize()
            times.append((time.perf_counter() - t0) / n * 1e6)
        # the fastest batch is the figure: a cost on the host path raises every batch, the state of the box only some
        print(f"enqueue grad p4 b=1 E={E} {form}: {min(times):.3f} us per launch, the fastest of {len(times)} batches"
              f" (median {statistics.median(times):.3f}; batches {' '.join(f'{t:.3f}' for t in times)})", flush=True)


def main():
    if sys.argv[1:2] == ["--worker"]:
        return worker()
    if sys.argv[1:2] == ["--enqueue"]:
        os.environ["FEINSUM_HIP_LIB"] = str(Path(sys.argv[2]).resolve())
        return enqueue()
    outputs = []
    for lib in sys.argv[1:3]:   # a fresh process per library; this one never opens the device
        env = dict(os.environ, FEINSUM_HIP_LIB=str(Path(lib).resolve()), FEINSUM_STRICT_RESIDENCY="1")
        res = subprocess.run([sys.executable, __file__, "--worker"], env=env, capture_output=True, text=True, timeout=900)
        if res.returncode != 0:
            print(res.stdout[-2000:], res.stderr[-4000:])
            return 2
        outputs.append(res.stdout.splitlines())
    parent, child = outputs
    differing = [(a, b) for a, b in zip(parent, child) if a != b]
    print(f"== parent library ({sys.argv[1]})")
    print("\n".join(parent))
    print(f"== child library ({sys.argv[2]}): {len(child)} lines, {len(differing) + abs(len(parent) - len(child))} differ from the parent's")
    for a, b in differing:
        print("parent:", a)
        print("child: ", b)
    return 1 if differing or len(parent) != len(child) else 0


if __name__ == "__main__":
    sys.exit(main())
