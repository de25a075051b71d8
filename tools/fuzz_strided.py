#!/usr/bin/env python3
"""Element slices of larger arrays: the cases and checks behind tests/test_gpu_strided.py.

Every sliced operand is ``base.narrow(element axis, a, n)`` of a base of its OWN length, so that ldJ, ldIn, ldOut and n are
four different numbers: a kernel that takes the wrong one reads NaN or misses the sentinel.  Input bases hold NaN outside
the slice, output bases a sentinel bit pattern everywhere; afterwards the inputs are bitwise what they were and the outputs
bitwise the sentinel outside the slice.  Inside the slice there are two references: ``evaluate`` on ``.contiguous()`` copies
of the same slices under the same transform (bitwise), and, on integer-valued data up to 4099 elements, the int64 einsum on
the host (exact).

    python tools/fuzz_strided.py            # every family, order and size once, on cuda:0
"""
from __future__ import annotations

import itertools
import sys
from dataclasses import dataclass
from pathlib import Path
from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

import feinsum_amd as f   # noqa: E402
from feinsum_amd import _hip   # noqa: E402

ORDERS = {1: (4, 3), 2: (10, 6), 3: (20, 10), 4: (35, 15)}          # p -> (Np, Nfp)
#: 16-element sub-tiles of a wave tile, per order p = 1..4 (GradGeom / DivGeom / FmGeom)
SUBTILES = {"grad": (5, 3, 2, 1), "div": (5, 3, 1, 1), "fm": (4, 2, 1, 1)}
FIELDS = {"grad": (1, 3), "div": (1, 3), "fm": (2, 4, 9)}
LAYOUTS = {"grad": ("rij", "rji"), "div": ("rij", "rji"),
           "fm": tuple(f"{j},{r}" for j in ("ef", "fe") for r in ("ifj", "fij", "jfi", "fji"))}
LARGE_P4 = (20_004, 100_007, 170_003)      # several rounds, the quarter-tail rule, the dynamic-walk threshold
HOST_REF_MAX = 4099
PLACEMENTS = ("odd", "even", "zero")       # a and ld both odd (planes only 8-byte aligned) / both even / a = 0 with ld > n
IN_NAN = 0x7FF8_0000_DEAD_BEEF             # outside the slices of the inputs
SENTINEL = 0x7FF8_0000_0000_0BAD           # everywhere in the outputs before the launch
#: (case label, fe_last_launch_info) of every matrix-core launch on slices that run_case saw
LAUNCHES: List[Tuple[str, dict]] = []


def sizes(family: str, p: int) -> Tuple[int, ...]:
    m = SUBTILES[family][p - 1]
    small = sorted({1, 15, 16, 17, 16 * m, 16 * m + 1, 4099})
    return tuple(small) + (LARGE_P4 if p == 4 else ())


@dataclass(frozen=True)
class Case:
    family: str        # "grad" | "div" | "fm"
    p: int
    n: int
    b: int
    layout: str
    placement: str
    only: Optional[str] = None     # slice this role alone ("J", "in", "out"); None: every operand

    @property
    def label(self) -> str:
        return f"{self.family} p={self.p} n={self.n} b={self.b} {self.layout} {self.placement}" + (f" only:{self.only}" if self.only else "")


def cases_of(family: str, p: int) -> List[Case]:
    """Every size x placement, with (b, layout) cycling so that every pair occurs."""
    combos = list(itertools.product(FIELDS[family], LAYOUTS[family]))
    out, i = [], 0
    for n in sizes(family, p):
        for placement in PLACEMENTS:
            for _ in range(2 if n <= HOST_REF_MAX else 1):
                b, layout = combos[i % len(combos)]
                out.append(Case(family, p, n, b, layout, placement))
                i += 1
    return out


def roles_of(case: Case) -> Dict[str, Tuple[str, Tuple[int, ...], Optional[int]]]:
    """role -> (index letters, shape with n elements, element axis or None)."""
    Np, Nfp = ORDERS[case.p]
    n = case.n
    if case.family == "fm":
        jl, rl = case.layout.split(",")
        ext = {"e": n, "f": 4, "i": Np, "j": Nfp}
        return {"J": (jl, tuple(ext[c] for c in jl), jl.index("e")), "op": (rl, tuple(ext[c] for c in rl), None),
                "in": ("fej", (4, n, Nfp), 1), "out": ("ei", (n, Np), 0)}
    ext = {"x": 3, "r": 3, "e": n, "i": Np, "j": Np}
    if case.family == "grad":
        return {"J": ("xre", (3, 3, n), 2), "op": (case.layout, (3, Np, Np), None), "in": ("ej", (n, Np), 0),
                "out": ("xei", (3, n, Np), 1)}
    return {"J": ("xre", (3, 3, n), 2), "op": (case.layout, (3, Np, Np), None), "in": ("xej", (3, n, Np), 1),
            "out": ("ei", (n, Np), 0)}


def subscripts(case: Case) -> str:
    r = roles_of(case)
    return f"{r['J'][0]},{r['op'][0]},{r['in'][0]}->{r['out'][0]}"


def expression(case: Case):
    r = roles_of(case)
    sym = lambda shape, axis: tuple("E" if d == axis else s for d, s in enumerate(shape))   # noqa: E731
    J = f.array("J", sym(r["J"][1], r["J"][2]))
    A = f.array("A", r["op"][1])
    rows = [[J, A, f.array(f"v{k}", sym(r["in"][1], r["in"][2]))] for k in range(case.b)]
    return f.batched_einsum(subscripts(case), rows)


def geometry(case: Case, role: str) -> Tuple[int, int]:
    """(a, ld) of a role's slice: offsets and base lengths differ from role to role and from n."""
    k = {"J": 0, "in": 1, "out": 2}[role]
    if case.only is not None and role != case.only:
        return 0, case.n
    if case.placement == "zero":
        return 0, case.n + 5 + 2 * k
    parity = 1 if case.placement == "odd" else 0
    a = 2 * (k + 1) + parity
    ld = case.n + a + 4 + 2 * k
    return a, ld + ((ld & 1) != parity)


class Operand:
    """One array of a launch: a base (NaN / sentinel outside the slice), the view handed to the library, the values."""

    def __init__(self, torch, shape, axis: Optional[int], a: int, ld: int, values, fill: int, dev) -> None:
        self.axis, self.a = axis, a
        base_shape = tuple(ld if d == axis else s for d, s in enumerate(shape))
        self.base = torch.full(base_shape, fill, dtype=torch.int64, device=dev).view(torch.float64)
        self.view = self.base if axis is None else self.base.narrow(axis, a, shape[axis])
        if values is not None:
            self.view.copy_(values)
        self.before = self.base.view(torch.int64).clone() if values is not None else None

    def unchanged(self, torch) -> bool:
        return bool(torch.equal(self.base.view(torch.int64), self.before))

    def outside_is(self, torch, fill: int) -> bool:
        mask = torch.ones(self.base.shape, dtype=torch.bool, device=self.base.device)
        if self.axis is not None:
            mask.narrow(self.axis, self.a, self.view.shape[self.axis]).fill_(False)
        else:
            mask.fill_(False)
        return bool((self.base.view(torch.int64)[mask] == fill).all())


def make_values(torch, case: Case, kind: str, seed: int, dev) -> Dict[str, Any]:
    """``"int"``: small integers (every product and sum exact in float64); ``"real"``: normal deviates."""
    gen = torch.Generator(device="cpu").manual_seed(seed)
    r = roles_of(case)

    def one(shape):
        if kind == "int":
            return torch.randint(-3, 4, shape, generator=gen, dtype=torch.int64).to(torch.float64).to(dev)
        return torch.randn(shape, generator=gen, dtype=torch.float64).to(dev)

    vals = {"J": one(r["J"][1]), "A": one(r["op"][1])}
    for k in range(case.b):
        vals[f"v{k}"] = one(r["in"][1])
    return vals


def host_reference(case: Case, vals: Dict[str, Any]) -> List[np.ndarray]:
    """The int64 einsum on the host (integer-valued data)."""
    to_int = lambda t: t.cpu().numpy().astype(np.int64)   # noqa: E731
    J, A = to_int(vals["J"]), to_int(vals["A"])
    return [np.einsum(subscripts(case), J, A, to_int(vals[f"v{k}"]), optimize=True) for k in range(case.b)]


def bind_sliced(torch, case: Case, vals: Dict[str, Any], dev):
    """The operands of one launch: ({name: Operand} of the inputs, [Operand] of the outputs)."""
    r = roles_of(case)
    aJ, ldJ = geometry(case, "J")
    ai, ldi = geometry(case, "in")
    ao, ldo = geometry(case, "out")
    ins = {"J": Operand(torch, r["J"][1], r["J"][2], aJ, ldJ, vals["J"], IN_NAN, dev),
           "A": Operand(torch, r["op"][1], None, 0, 0, vals["A"], IN_NAN, dev)}
    for k in range(case.b):
        ins[f"v{k}"] = Operand(torch, r["in"][1], r["in"][2], ai, ldi, vals[f"v{k}"], IN_NAN, dev)
    outs = [Operand(torch, r["out"][1], r["out"][2], ao, ldo, None, SENTINEL, dev) for _ in range(case.b)]
    return ins, outs


def run_case(torch, case: Case, dev="cuda:0", transform: Any = "auto", seed: int = 0) -> List[str]:
    """Run one case on both data kinds; returns the list of failures (empty: all checks hold)."""
    expr = expression(case)
    bad: List[str] = []
    for kind in ("int", "real"):
        vals = make_values(torch, case, kind, seed + (kind == "real"), dev)
        ins, outs = bind_sliced(torch, case, vals, dev)
        args = {name: op.view for name, op in ins.items()}
        out_dict = {name: o.view for name, o in zip(expr.output_names, outs)}
        f.evaluate(expr, 0, args, out_dict=out_dict, transform=transform, wait=True)
        info = _hip.last_launch_info()
        tel = 16 * SUBTILES[case.family][case.p - 1]
        if info.get("element_slice"):
            LAUNCHES.append((case.label, dict(info)))
        sliced = any(not t.is_contiguous() for t in list(args.values()) + list(out_dict.values()))
        if case.n >= tel and sliced and not (info.get("valid") and info.get("tiles", 0) > 0 and info.get("element_slice")):
            bad.append(f"{case.label} [{kind}]: no matrix-core launch on an element slice reported: {info}")
        # (the reference writes into plain torch arrays: outputs that evaluate allocates itself come from the split allocator from
        #  8 MiB up, whose search for a second class of memory has one time budget per process -- not this test's to spend)
        ref = {name: torch.empty_like(o.view, memory_format=torch.contiguous_format) for name, o in zip(expr.output_names, outs)}
        f.evaluate(expr, 0, {k: v.contiguous() for k, v in args.items()}, out_dict=ref, transform=transform, wait=True)
        for k, (name, o) in enumerate(zip(expr.output_names, outs)):
            if not torch.equal(o.view.contiguous().view(torch.int64), ref[name].view(torch.int64)):
                diff = int((o.view.contiguous().view(torch.int64) != ref[name].view(torch.int64)).sum())
                bad.append(f"{case.label} [{kind}]: output {k} differs from the contiguous launch in {diff} entries")
            if not o.outside_is(torch, SENTINEL):
                bad.append(f"{case.label} [{kind}]: output {k}: the base changed outside the slice")
        for name, op in ins.items():
            if not op.unchanged(torch):
                bad.append(f"{case.label} [{kind}]: input {name} changed")
        if kind == "int" and case.n <= HOST_REF_MAX:
            for k, (want, o) in enumerate(zip(host_reference(case, vals), outs)):
                got = o.view.cpu().numpy()
                if not (np.isfinite(got).all() and np.array_equal(got.astype(np.int64), want) and np.array_equal(got, want.astype(np.float64))):
                    bad.append(f"{case.label}: output {k} is not the exact int64 einsum")
    return bad


def main(argv: Sequence[str]) -> int:
    import torch

    failures: List[str] = []
    count = 0
    for family in ("grad", "div", "fm"):
        for p in (1, 2, 3, 4):
            for case in cases_of(family, p):
                failures += run_case(torch, case)
                count += 1
    for line in failures:
        print("FAIL", line)
    print(f"{count} cases, {len(failures)} failures")
    return 1 if failures else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
