"""Seeded sweep of the DG family kernels (grad, div, face-mass, mass / operator apply, div components, the cross
product, triangles, the fused operator) through every transform that accepts them, against the references of
oracle/einsum_ref.py (test infrastructure, like tests/).

    python tools/fuzz_dg.py [n_cases] [seed]
    python tools/fuzz_dg.py --placement [seed]
    python tools/fuzz_dg.py --repro '<REPRO line of either kind>'

Passes:

``run_exact``      exact data (``m * 2**s``, bits and scales per array NAME, so that arrays shared by rows and stages
                   keep every row within budget; near-overflow and subnormal scales too): bitwise equal to the int64
                   einsum of the mantissas, or, at E > 4099, to torch's float64 einsum, itself checked against the int64
                   einsum on first / middle / last / random slices.
``run_bounded``    signed uniform data: ``|got - ref| <= gamma(n, u) * absref`` entrywise (u = 2^-24 for float32).
``run_nonfinite``  exact data with one NaN / +Inf / -Inf planted in a field, a geometry factor or an operator entry: the
                   dependency set of that entry (and nothing else) is NaN / non-finite, every other entry bitwise exact.
``run_poison``     the same launch on all-NaN inputs of another size first: the clean launch after it stays exact.
``run_large``      whole-array exact checks at E = 98 304 ... 1 000 007 (8e6 on request) with the walk, tail, load and
                   store knobs and the output allocation varied; float32 at E = 70 004 and 1 000 004.
``run_placement``  a fixed case list with every operand 0 or 8 bytes (float64), 0, 4, 8 or 12 bytes (float32) past a
                   256-byte boundary (:func:`embed`): one array shifted at a time, all of them, a random mix, against
                   the aligned launch.  Inputs sit between NaN bands, so a value read from behind an input shows as
                   a NaN (``leak:``); every input buffer must come back bitwise unchanged.  Exact data: bitwise the
                   int64 einsum.  Signed data: the bound, and every all-float64 result bitwise that of the aligned
                   launch (no float64 route looks at more than ``& 7`` of a pointer, so the same kernel runs the same
                   arithmetic; float32 and mixed cases may move between the matrix-core and the tiled kernel and
                   get the bound alone).  A launch accepted aligned must be accepted at every placement.

Outputs land in NaN-filled buffers between sentinel guard bands (tools/fuzz_einsum.py).  Runs are counted per family,
order, dtype, transform, E class, walk and fused / prepared (:data:`MINIMUMS`).
"""

from __future__ import annotations

import json
import math
import random
import sys
from collections import Counter
from dataclasses import asdict, dataclass
from pathlib import Path
from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
for _p in (ROOT, ROOT / "tools"):
    if str(_p) not in sys.path:
        sys.path.insert(0, str(_p))

import feinsum_amd as f  # noqa: E402
from feinsum_amd import _hip  # noqa: E402
from feinsum_amd.measure import launch_kind  # noqa: E402
from fuzz_einsum import GUARD, SENTINEL, Stats, _guarded, _guards_intact, missing_buckets  # noqa: E402,F401
from oracle import einsum_ref as ref_  # noqa: E402

ORDERS3 = [(4, 3), (10, 6), (20, 10), (35, 15), (56, 21), (7, 4), (13, 5)]   # (Np, Nfp); 7 and 13: tiled kernels only
ORDERS2 = [(3, 2), (6, 3), (10, 4), (15, 5), (21, 6)]
KINDS = ("grad", "div", "bgrad", "bdiv", "divcomp", "cross", "fm", "fm_ifj", "fm_jfi", "fm_fji", "mass", "apply",
         "grad2", "div2", "lift2")
TRANSFORMS = ("auto", "mfma", "tiled", "generic", "mfma_split", "prepared")
E_CLASSES = {
    "one": [1],
    "sub-tile": [2, 3, 5, 7, 15],
    "tiles": [16, 32, 64, 128, 256, 1024, 4096],
    "ragged": [17, 33, 63, 65, 127, 129, 1003, 4099],
    "static-rounds": [20_004, 33_333, 49_152, 65_537],
    "quarter-tail": [98_304, 100_000, 100_007],
    "dynamic": [170_003, 262_144],
}
#: E at most this: the int64 reference of the whole array on the host, else torch's float64 einsum on the device
HOST_REF_MAX_E = 4099

#: minimum runs per bucket of the fixed-seed exact sweep (tests/test_dg_exact_cpu.py, tests/test_gpu_dg_exact.py)
MINIMUMS = {**{f"family:{k}": 3 for k in KINDS}, "family:pipeline": 4,
            **{f"order:3d-{n}": 8 for n, _ in ORDERS3}, **{f"order:2d-{n}": 3 for n, _ in ORDERS2},
            "dtype:float64": 60, "dtype:float32": 30, "dtype:mixed": 10,
            **{f"transform:{t}": 20 for t in TRANSFORMS},
            **{f"E:{c}": 4 for c in E_CLASSES},
            "range:overflow": 6, "range:subnormal": 6, "fused:yes": 2, "fused:no": 2}


@dataclass(frozen=True)
class DGCase:
    kind: str          # one of KINDS, or "pipeline" (div + grad + lift through evaluate_operator)
    Np: int
    Nfp: int
    b: int
    op: str            # "rij" / "rji" (mass / apply: "ij" / "ji")
    dtype: str         # "float64", "float32" or "mixed" (fields float32, the rest float64)
    E: int
    eclass: str
    seed: int
    scale: str = "normal"     # "normal", "overflow", "subnormal"
    fuse: bool = True

    def repro(self) -> str:
        return json.dumps(asdict(self), separators=(",", ":"))

    @staticmethod
    def from_repro(text: str) -> "DGCase":
        return DGCase(**json.loads(text))

    # ---- the einsums: list of stages, each (expr, {array name: data key}); keys are shared where arrays are
    def stages(self) -> List[Tuple[Any, Dict[str, str]]]:
        Np, Nfp, b, op = self.Np, self.Nfp, self.b, self.op
        fdt = "float32" if self.dtype in ("float32", "mixed") else "float64"
        gdt = "float32" if self.dtype == "float32" else "float64"
        A = lambda name, shape, field=False: f.array(name, shape, fdt if field else gdt)   # noqa: E731
        k = self.kind
        if k == "pipeline":
            div = f.einsum("xre,rij,xej->ei", A("J", (3, 3, "E")), A("R", (3, Np, Np)), A("u", (3, "E", Np), True))
            grad = f.einsum("xre,rij,ej->xei", A("J", (3, 3, "E")), A("R", (3, Np, Np)), A("u", ("E", Np), True))
            lift = f.batched_einsum("ef,fij,fej->ei", [[A("J", ("E", 4)), A("R", (4, Np, Nfp)),
                                                         A(f"v{i}", (4, "E", Nfp), True)] for i in range(b)])
            return [(div, {"J": "J", "R": "R", "u": "u_div"}), (grad, {"J": "J", "R": "R", "u": "u_grad"}),
                    (lift, {"J": "LJ", "R": "LR", **{f"v{i}": f"v{i}" for i in range(b)}})]
        if k in ("grad", "div", "bgrad", "bdiv", "grad2", "div2"):
            nd = 2 if k.endswith("2") else 3
            nb = 1 if k in ("grad", "div") else b
            subs = f"xre,{op},ej->xei" if "grad" in k else f"xre,{op},xej->ei"
            ushape = ("E", Np) if "grad" in k else (nd, "E", Np)
            expr = f.batched_einsum(subs, [[A("J", (nd, nd, "E")), A("R", (nd, Np, Np)), A(f"u{i}", ushape, True)]
                                           for i in range(nb)])
        elif k == "divcomp":
            expr = f.batched_einsum("se,sij,ej->ei", [[A("J" + c, (3, "E")), A("R", (3, Np, Np)),
                                                       A("u" + c, ("E", Np), True)] for c in "xyz"])
        elif k == "cross":
            fields = {"ux": ("Jy", "Jz"), "uy": ("Jx", "Jz"), "uz": ("Jx", "Jy"), "vx": ("Jy", "Jz")}
            expr = f.batched_einsum(f"re,{op},ej->ei", [[A(J, (3, "E")), A("D", (3, Np, Np)), A(u, ("E", Np), True)]
                                                        for u, js in fields.items() for J in js])
        elif k.startswith("fm") or k == "lift2":
            nf = 3 if k == "lift2" else 4
            layout = "fm" if k == "lift2" else k
            rows = []
            for i in range(b):
                v = A(f"v{i}", (nf, "E", Nfp), True)
                rows.append({"fm": [A("J", ("E", nf)), A("R", (nf, Np, Nfp)), v],
                             "fm_fji": [A("J", ("E", nf)), A("R", (nf, Nfp, Np)), v],
                             "fm_ifj": [A("L", (Np, nf, Nfp)), A("J", (nf, "E")), v],
                             "fm_jfi": [A("L", (Nfp, nf, Np)), A("J", (nf, "E")), v]}[layout])
            subs = {"fm": "ef,fij,fej->ei", "fm_fji": "ef,fji,fej->ei", "fm_ifj": "ifj,fe,fej->ei",
                    "fm_jfi": "jfi,fe,fej->ei"}[layout]
            expr = f.batched_einsum(subs, rows)
        elif k == "mass":
            expr = f.batched_einsum(f"e,{op},ej->ei", [[A("J", ("E",)), A("D", (Np, Np)), A(f"u{i}", ("E", Np), True)]
                                                       for i in range(b)])
        else:   # apply
            expr = f.einsum(f"{op},ej->ei", A("D", (Np, Np)), A("u", ("E", Np), True))
        return [(expr, {nm: nm for nm in expr.all_args})]

    def transforms(self) -> List[Any]:
        if self.kind == "pipeline":
            return [None]
        return [{"prepared": True} if t == "prepared" else t for t in TRANSFORMS]


def tname(t: Any) -> str:
    return "prepared" if isinstance(t, dict) else "auto" if t is None else str(t)


def eclass_of(E: int) -> str:
    for c, xs in E_CLASSES.items():
        if E in xs:
            return c
    return "ragged"


# --------------------------------------------------------------------------
# cases (host only)
# --------------------------------------------------------------------------

def _case(rng: random.Random, kind: str, eclass: Optional[str] = None, dtype: Optional[str] = None,
          scale: str = "normal") -> DGCase:
    Np, Nfp = rng.choice(ORDERS2 if kind.endswith("2") else ORDERS3[:5] if kind == "pipeline" else ORDERS3)
    if dtype is None:
        dtype = "float64" if kind == "pipeline" else rng.choice(["float64"] * 5 + ["float32"] * 3 + ["mixed"] * 2)
    if eclass is None:
        eclass = rng.choice(["one", "sub-tile", "tiles", "tiles", "ragged", "ragged", "ragged", "static-rounds"])
    E = rng.choice(E_CLASSES[eclass])
    if dtype == "float32" and rng.random() < 0.5 and E > 4:   # float32: the tiled kernel at E not a multiple of 4
        E += rng.choice([1, 2, 3]) if E % 4 == 0 else 0
    if kind in ("mass", "apply"):
        op = rng.choice(["ij", "ji"])
    else:
        op = rng.choice(["rij", "rji"])
    b = rng.choice([1, 2, 3, 4, 5, 8, 9]) if kind != "pipeline" else rng.choice([1, 2, 3, 4, 5])
    return DGCase(kind, Np, Nfp, b, op, dtype, E, eclass_of(E) if E not in E_CLASSES[eclass] else eclass,
                  rng.randrange(1 << 30), scale, rng.random() < 0.5)


def gen_cases(n: int, seed: int) -> List[DGCase]:
    """*n* random cases, then fixed sets: every family once per E class of the small ones, the range cases, the fused
    operator both ways, and the launches of the quarter tails and the dynamic walk."""
    rng = random.Random(seed)
    cases = [_case(rng, rng.choice(KINDS)) for _ in range(n)]
    for kind in KINDS:
        cases.append(_case(rng, kind, rng.choice(["one", "sub-tile", "tiles", "ragged"])))
    for scale in ("overflow", "subnormal"):
        for dt in ("float64", "float32", "float64", "float32"):
            cases.append(_case(rng, rng.choice(KINDS), rng.choice(["tiles", "ragged", "sub-tile"]), dt, scale))
    for fuse in (True, False):
        for ec in ("ragged", "tiles", "quarter-tail"):
            cases.append(DGCase(**{**asdict(_case(rng, "pipeline", ec)), "fuse": fuse}))
    for kind, ec in (("grad", "quarter-tail"), ("div", "quarter-tail"), ("bgrad", "quarter-tail"),
                     ("fm", "quarter-tail"), ("grad", "dynamic"), ("div", "dynamic"), ("fm", "dynamic")):
        c = _case(rng, kind, ec, "float64")
        cases.append(DGCase(**{**asdict(c), "Np": 35, "Nfp": 15, "b": min(c.b, 3)}))
    return cases


def buckets_of(case: DGCase, transform: Any) -> List[str]:
    nd = "2d" if case.kind.endswith("2") else "3d"
    b = [f"family:{case.kind}", f"order:{nd}-{case.Np}", f"dtype:{case.dtype}", f"transform:{tname(transform)}",
         f"E:{case.eclass}", f"range:{case.scale}"]
    if case.kind == "pipeline":
        b.append("fused:" + ("yes" if case.fuse else "no"))
    return b


def accepted_on_host(case: DGCase, transform: Any) -> bool:
    """Whether the host plan takes the case under *transform* (the device may still refuse a variant: counted then)."""
    try:
        for expr, _ in case.stages():
            launch_kind(expr, transform, {"E": case.E})
    except NotImplementedError:
        return False
    return True


def coverage(cases: Sequence[DGCase]) -> Counter:
    cnt: Counter = Counter()
    for c in cases:
        for t in c.transforms():
            if accepted_on_host(c, t):
                cnt.update(buckets_of(c, t))
    return cnt


# --------------------------------------------------------------------------
# exact data
# --------------------------------------------------------------------------

def _terms(expr) -> int:
    ins, out = expr.get_subscripts().replace(" ", "").split("->")
    ext = {i: (2 if isinstance(d, f.SizeParam) else int(d)) for i, d in expr.index_to_dim_length.items()}
    return ref_.summed_points(f"{ins}->{out}", ext)


def plan_data(case: DGCase, rng: np.random.Generator):
    """``(bits, scales, dtypes, significand)`` per data key."""
    stages = case.stages()
    dtypes = {}
    rows = []
    for expr, keys in stages:
        for row in expr.args:
            rows.append(([keys[a.name] for a in row], _terms(expr)))
            for a in row:
                dtypes[keys[a.name]] = np.dtype(a.dtype)
    sig = 24 if case.dtype == "float32" else 53
    if case.scale == "subnormal":
        sig -= 4     # every sum below the smallest normal: subnormal results
    f32 = [k for k, d in dtypes.items() if d == np.dtype("float32")]
    bits = ref_.shared_exact_bits(rows, f32, sig, rng)
    scales: Dict[str, int] = {}
    out_dt = np.dtype("float32") if case.dtype == "float32" else np.dtype("float64")
    for expr, keys in stages:
        positions = [[keys[row[p].name] for row in expr.args] for p in range(len(expr.args[0]))]
        for k, s in ref_.range_scales(positions, bits, sig, out_dt, case.scale, rng).items():
            scales.setdefault(k, s)
    return bits, scales, dtypes, sig


def _shape(expr, name: str, E: int) -> Tuple[int, ...]:
    return tuple(E if isinstance(d, f.SizeParam) else int(d) for d in expr.arg_to_shape[name])


def host_data(case: DGCase, extra: int = 0):
    """``(arrays by key, mantissas by key, scales, significand)`` of exact data for the case."""
    rng = np.random.default_rng(case.seed + 7919 * extra)
    bits, scales, dtypes, sig = plan_data(case, rng)
    shapes = {}
    for expr, keys in case.stages():
        for nm, k in keys.items():
            shapes[k] = _shape(expr, nm, case.E)
    arrays, mants = {}, {}
    for k in sorted(shapes):
        m, x = ref_.exact_operands([shapes[k]], [dtypes[k]], [bits[k]], [scales[k]], rng)
        mants[k], arrays[k] = m[0], x[0]
    return arrays, mants, scales, sig


def _e_axis(expr, name: Optional[str]) -> Optional[int]:
    shape = expr.shape if name is None else expr.arg_to_shape[name]
    for ax, d in enumerate(shape):
        if isinstance(d, f.SizeParam):
            return ax
    return None


def references(torch, case: DGCase, arrays, mants, scales, sig, dev, st: Optional[Stats] = None, e_axis=None):
    """``[{output name: reference (device tensor)}]`` per stage (*e_axis*: ``(expr, array name or None) -> element axis``
    where the element axis is not a size parameter; default :func:`_e_axis`).  E <= HOST_REF_MAX_E: the int64 reference of the whole
    array, and torch's float64 einsum must agree with it everywhere; else torch's float64 einsum of the whole array,
    checked against the int64 reference on first / middle / last / random slices."""
    refs = []
    rng = np.random.default_rng(case.seed + 1)
    E = case.E
    e_axis = e_axis or _e_axis
    for expr, keys in case.stages():
        subs = expr.get_subscripts()
        out_dt = np.dtype("float32") if case.dtype == "float32" else np.dtype("float64")
        oax = e_axis(expr, None)
        per = {}
        for out_name, row in zip(expr.output_names, expr.args):
            ks = [keys[a.name] for a in row]
            total = sum(scales[k] for k in ks)
            eaxes = [e_axis(expr, a.name) for a in row]
            if E <= HOST_REF_MAX_E:
                host = ref_.int_reference(subs, [mants[k] for k in ks], total, out_dt, sig)
                r = torch.from_numpy(host).cuda()
                if case.scale == "normal":   # (the device einsum is only used, and only checked, in the normal range)
                    tr = ref_.torch_exact_reference(torch, subs, [dev[k] for k in ks], eaxes, oax, out_dt)
                    if ref_.differing_entries(tr, r) and st is not None:
                        st.fail(f"reference: torch float64 einsum != int64 einsum  REPRO {case.repro()}")
            else:
                r = ref_.torch_exact_reference(torch, subs, [dev[k] for k in ks], eaxes, oax, out_dt)
                starts = [0, E // 2 - 16, E - 37] + [int(x) for x in rng.integers(0, E - 37, size=3)]
                for e0 in starts:
                    w = min(37, E - e0)
                    sl = [_take(mants, k, ax, e0, w) for k, ax in zip(ks, eaxes)]
                    want = ref_.int_reference(subs, sl, total, out_dt, sig)
                    got = r.narrow(oax, e0, w).cpu().numpy()
                    if not ref_.bitwise_equal(got, want) and st is not None:
                        st.fail(f"reference: torch float64 einsum != int64 einsum on [{e0}, {e0 + w})  REPRO {case.repro()}")
            per[out_name] = r
        refs.append(per)
    return refs


# --------------------------------------------------------------------------
# launching
# --------------------------------------------------------------------------

def _out_buffers(torch, case: DGCase):
    bufs, out_dicts = [], []
    for expr, _ in case.stages():
        shape = tuple(case.E if isinstance(d, f.SizeParam) else int(d) for d in expr.shape)
        dt = torch.float32 if case.dtype == "float32" else torch.float64
        d = {}
        for name in expr.output_names:
            buf, out, n = _guarded(torch, shape, dt)
            bufs.append((buf, n))
            d[name] = out
        out_dicts.append(d)
    return bufs, out_dicts


def launch(torch, case: DGCase, dev, transform, out_dicts):
    """Run the case (one stage: ``evaluate``; the pipeline: ``evaluate_operator``); ``last_launch_info`` after it."""
    stages = case.stages()
    if case.kind == "pipeline":
        args = [(expr, {nm: dev[k] for nm, k in keys.items()}) for expr, keys in stages]
        f.evaluate_operator(args, 0, out_dicts=out_dicts, fuse=case.fuse, wait=True)
    else:
        expr, keys = stages[0]
        f.evaluate(expr, 0, {nm: dev[k] for nm, k in keys.items()}, out_dict=out_dicts[0], transform=transform, wait=True)
    return _hip.last_launch_info()


def _walk_buckets(case: DGCase, info: dict) -> List[str]:
    if not info or case.dtype != "float64" or case.E < 20_000:
        return []   # (the record belongs to the last f64 matrix-core launch: small and float32 launches do not set it)
    b = ["walk:" + ("dynamic" if info.get("dynamic_walk") else "static")]
    b += [k for k in ("quarter_tail", "staggered_start") if info.get(k)]
    return b


def _compare(st: Stats, label: str, refs, out_dicts, bufs, case: DGCase) -> bool:
    if not all(_guards_intact(buf, n) for buf, n in bufs):
        st.fail(f"{label}: wrote outside its output  REPRO {case.repro()}")
        return False
    ok = True
    for per, outs in zip(refs, out_dicts):
        for name, r in per.items():
            got = outs[name]
            st.exact_runs += 1
            bad = ref_.differing_entries(got, r)   # (-0.0 == 0.0: the sign of an exact zero sum is not specified)
            if not bad:
                st.exact_equal += 1
            else:
                ok = False
                st.fail(f"{label}: output {name}: {bad} entries differ from the exact result  REPRO {case.repro()}")
    return ok


def _exact_case(torch, case: DGCase, st: Stats, poison: bool = False) -> None:
    arrays, mants, scales, sig = host_data(case)
    if sig == 53 and case.scale == "normal":
        # float64 compute: some entry must need more than float32's 24 bits (a float32 step in the kernel then fails)
        for extra in range(1, 4):
            probe = _host_probe(case, mants, scales, sig)
            if probe is None or ref_.needs_more_than_f32(probe):
                break
            arrays, mants, scales, sig = host_data(case, extra)
        probe = _host_probe(case, mants, scales, sig)
        if probe is not None and probe.any() and not ref_.needs_more_than_f32(probe):
            st.without_wide_entry += 1
    dev = {k: torch.from_numpy(np.ascontiguousarray(a)).cuda() for k, a in arrays.items()}
    refs = references(torch, case, arrays, mants, scales, sig, dev, st)
    for t in case.transforms():
        label = f"exact {tname(t)}{' poisoned' if poison else ''}: {case.kind} Np={case.Np} b={case.b} {case.op}" \
                f" {case.dtype} E={case.E} {case.scale}"
        if poison:   # the same launch on all-NaN inputs of another size first
            E2 = case.E + 37 if case.E < 4000 else max(1, case.E // 3)
            pc = DGCase(**{**asdict(case), "E": E2})
            pdev = {}
            for expr, keys in pc.stages():
                for nm, k in keys.items():
                    pdev[k] = torch.full(_shape(expr, nm, E2), float("nan"), dtype=dev[k].dtype, device="cuda")
            pb, pod = _out_buffers(torch, pc)
            try:
                launch(torch, pc, pdev, t, pod)
            except NotImplementedError:
                continue
            del pb, pod, pdev
        bufs, out_dicts = _out_buffers(torch, case)
        try:
            info = launch(torch, case, dev, t, out_dicts)
        except NotImplementedError:
            st.cov["not-accepted:" + tname(t)] += 1
            continue
        st.cov.update(buckets_of(case, t) + _walk_buckets(case, info))
        if poison:
            st.cov["poisoned"] += 1
        _compare(st, label, refs, out_dicts, bufs, case)


def _host_probe(case: DGCase, mants, scales, sig) -> Optional[np.ndarray]:
    """The exact result of the first row on up to 64 elements (enough to see whether some entry needs > 24 bits)."""
    expr, keys = case.stages()[0]
    row = expr.args[0]
    ks = [keys[a.name] for a in row]
    w = min(case.E, 64)
    if w == 0:
        return None
    sl = [np.take(mants[k], range(w), axis=ax) if ax is not None else mants[k]
          for k, ax in zip(ks, [_e_axis(expr, a.name) for a in row])]
    return ref_.int_reference(expr.get_subscripts(), sl, sum(scales[k] for k in ks), np.float64, sig)


def run_exact(n: int, seed: int) -> Stats:
    import torch

    st = Stats(f"dg exact seed={seed}")
    for case in gen_cases(n, seed):
        _exact_case(torch, case, st)
    return st


def run_poison(n: int, seed: int) -> Stats:
    """Every transform of *n* small cases with a launch on all-NaN inputs of another size in front."""
    import torch

    st = Stats(f"dg poison seed={seed}")
    rng = random.Random(seed + 3)
    for _ in range(n):
        _exact_case(torch, _case(rng, rng.choice(KINDS + ("pipeline",)), rng.choice(["tiles", "ragged", "sub-tile"])),
                    st, poison=True)
    return st


# --------------------------------------------------------------------------
# signed uniform data
# --------------------------------------------------------------------------

def run_bounded(n: int, seed: int) -> Stats:
    import torch

    st = Stats(f"dg bounded seed={seed}")
    rng = random.Random(seed + 5)
    for _ in range(n):
        case = _case(rng, rng.choice(KINDS + ("pipeline",)), rng.choice(["one", "sub-tile", "tiles", "ragged"]))
        if case.E > 1100:
            case = DGCase(**{**asdict(case), "E": rng.choice([63, 64, 65, 127, 128, 129, 1003])})
        nrng = np.random.default_rng(case.seed)
        dev, host = {}, {}
        for expr, keys in case.stages():
            for nm, k in keys.items():
                if k not in host:
                    host[k] = (nrng.random(_shape(expr, nm, case.E)) * 2 - 1).astype(expr.arg_to_dtype[nm])
                    dev[k] = torch.from_numpy(host[k]).cuda()
        u = ref_.U32 if case.dtype == "float32" else ref_.U64
        for t in case.transforms():
            bufs, out_dicts = _out_buffers(torch, case)
            try:
                launch(torch, case, dev, t, out_dicts)
            except NotImplementedError:
                st.cov["not-accepted:" + tname(t)] += 1
                continue
            bk = buckets_of(case, t)
            st.cov.update(bk)
            label = f"bounded {tname(t)}: {case.kind} Np={case.Np} b={case.b} {case.op} {case.dtype} E={case.E}"
            if not all(_guards_intact(buf, m) for buf, m in bufs):
                st.fail(f"{label}: wrote outside its output  REPRO {case.repro()}")
                continue
            for (expr, keys), outs in zip(case.stages(), out_dicts):
                nb = ref_.bound_terms(expr.get_subscripts(), _extent(expr, case.E), 3)
                for name, row in zip(expr.output_names, expr.args):
                    r, ar = ref_.bounded_reference(expr.get_subscripts(), [host[keys[a.name]] for a in row])
                    ratio = ref_.bound_ratio(outs[name].cpu().numpy(), r, ar, nb, u)
                    for b_ in bk:
                        st.worst[b_] = max(st.worst.get(b_, 0.0), ratio)
                    if ratio > 1:
                        st.fail(f"{label}: output {name}: |got - ref| = {ratio:.3g} x the bound  REPRO {case.repro()}")
    return st


def _extent(expr, E: int) -> Dict[str, int]:
    return {i: (E if isinstance(d, f.SizeParam) else int(d)) for i, d in expr.index_to_dim_length.items()}


# --------------------------------------------------------------------------
# non-finite values
# --------------------------------------------------------------------------

def plant_sites(case: DGCase, rng: random.Random) -> List[Tuple[str, str, Tuple[int, ...]]]:
    """``(role, key, index)``: a field, a geometry factor and an operator entry, at the first element, the last of a
    tile, the last one, and one inside the last quarter tiles / dynamically walked rounds."""
    E = case.E
    elems = sorted({0, min(E - 1, 15), min(E - 1, 63), E - 1, max(0, E - 1 - rng.randrange(max(E // 40, 1)))})
    stage = rng.randrange(len(case.stages()))
    expr, keys = case.stages()[stage]
    row = expr.args[rng.randrange(len(expr.args))]
    sites = []
    for a in row:
        shape = _shape(expr, a.name, E)
        ax = _e_axis(expr, a.name)
        role = "operator" if ax is None else ("field" if a is row[-1] else "geometry")
        if ax is None:
            choices = [tuple(0 for _ in shape), tuple(s - 1 for s in shape),
                       tuple(rng.randrange(s) for s in shape[:-1]) + (0,),          # a column-0 entry
                       tuple(rng.randrange(s) for s in shape)]
            sites.append((role, keys[a.name], rng.choice(choices)))
        else:
            for e in elems if role == "field" else rng.sample(elems, min(2, len(elems))):
                idx = [rng.randrange(s) for s in shape]
                idx[ax] = e
                sites.append((role, keys[a.name], tuple(idx)))
    return sites


#: orders whose f64 matrix-core grad / div kernels pad the k (column) dimension of the operator fragments
PADDED_ORDERS = (4, 10, 20, 35, 56)


def padding_sites(Np: int, op: str) -> List[Tuple[int, int, int]]:
    """Operator entries (indices of the STORED array) that padding reads can reach: the kernels stage the operator
    contiguously, so a read past the end of a row (grad's padding column j = Np, div's ``asmall`` build with j >= Np)
    lands on the first entries of the next row ("rij": ``R[r, i, 0..2]`` for i >= 1) or of the next plane (``R[r, 0,
    0..2]`` for r >= 1; "rji", stored [r][j][i]: ``R[r, 0..2, i]`` for r >= 1).  A select keeps them out; a multiply
    by the zero-or-one mask would carry a NaN or Inf there into a neighbouring row, outside its dependency set."""
    rows = sorted({1, 2, Np // 2, Np - 1} - {0}) if Np > 1 else []
    cols = range(min(3, Np))
    if op == "rij":
        sites = [(r, i, c) for r in range(3) for i in rows for c in cols] + [(r, 0, c) for r in (1, 2) for c in cols]
    else:
        sites = [(r, c, i) for r in (1, 2) for c in cols for i in sorted({0, 1, Np // 2, Np - 1})]
        sites += [(0, c, i) for c in cols for i in (1, Np - 1)]
    return sorted(set(sites))


def padding_cases(seed: int) -> List[DGCase]:
    """grad and div, both operator layouts, every padded order, float64, at E = 16 (one tile) and 1003 (ragged)."""
    rng = random.Random(seed + 13)
    return [DGCase(kind, Np, 0, 1, op, "float64", E, eclass_of(E), rng.randrange(1 << 30))
            for kind in ("grad", "div") for Np in PADDED_ORDERS for op in ("rij", "rji") for E in (16, 1003)]


def _plant_runs(torch, st: Stats, case: DGCase, dev, refs, role: str, key: str, idx, value: float,
                transforms: Sequence[Any]) -> None:
    """Plant *value* at ``dev[key][idx]``, run *transforms*, check the dependency rule
    (``einsum_ref.nonfinite_violations``), put the entry back."""
    old = dev[key][idx].clone()
    dev[key][idx] = value
    deps = _dependency(torch, case, key, idx)
    for t in transforms:
        bufs, out_dicts = _out_buffers(torch, case)
        try:
            launch(torch, case, dev, t, out_dicts)
        except NotImplementedError:
            continue
        st.cov.update([f"planted:{role}", f"value:{value}", f"transform:{tname(t)}", f"family:{case.kind}",
                       f"E:{case.eclass}", f"dtype:{case.dtype}"])
        label = f"nonfinite {tname(t)}: {case.kind} Np={case.Np} b={case.b} {case.op} {case.dtype} E={case.E}" \
                f" {value} in {key}{list(idx)}"
        if not all(_guards_intact(buf, m) for buf, m in bufs):
            st.fail(f"{label}: wrote outside its output  REPRO {case.repro()}")
            continue
        st.exact_runs += 1
        bad = 0
        for per, outs, dep in zip(refs, out_dicts, deps):
            for name, r in per.items():
                bad += ref_.nonfinite_violations(outs[name], r, dep[name], value)
        if bad:
            st.fail(f"{label}: {bad} entries break the dependency rule  REPRO {case.repro()}")
        else:
            st.exact_equal += 1
    dev[key][idx] = old


def _prepare(torch, case: DGCase, st: Stats):
    arrays, mants, scales, sig = host_data(case)
    dev = {k: torch.from_numpy(np.ascontiguousarray(a)).cuda() for k, a in arrays.items()}
    return dev, references(torch, case, arrays, mants, scales, sig, dev, st)


def run_nonfinite(n: int, seed: int) -> Stats:
    """*n* random cases with a field, a geometry factor and an operator entry planted at random, the quarter-tail
    cases, then every :func:`padding_sites` entry of every :func:`padding_cases` case under "mfma" and "auto"."""
    import torch

    st = Stats(f"dg nonfinite seed={seed}")
    rng = random.Random(seed + 7)
    cases = [_case(rng, rng.choice(KINDS + ("pipeline",)), rng.choice(["one", "tiles", "ragged", "ragged"]))
             for _ in range(n)]
    cases += [_case(rng, k, ec, "float64") for k in ("grad", "div", "fm", "pipeline") for ec in ("quarter-tail",)]
    cases += [_case(rng, "grad", "tiles", "float64") for _ in range(2)]
    for case in cases:
        dev, refs = _prepare(torch, case, st)
        for role, key, idx in plant_sites(case, rng):
            _plant_runs(torch, st, case, dev, refs, role, key, idx, rng.choice([math.nan, math.inf, -math.inf]),
                        case.transforms())
    for case in padding_cases(seed):
        dev, refs = _prepare(torch, case, st)
        for k, idx in enumerate(padding_sites(case.Np, case.op)):
            _plant_runs(torch, st, case, dev, refs, "padding-read", "R", idx, (math.nan, math.inf, -math.inf)[k % 3],
                        ("mfma", "auto"))
    return st


def _dependency(torch, case: DGCase, key: str, idx) -> List[Dict[str, Any]]:
    """Per stage, ``{output: bool tensor}`` of the entries that depend on entry *idx* of array *key*
    (oracle.einsum_ref.dependency_set, on the device: a one-hot array, all-ones for the rest)."""
    out = []
    for expr, keys in case.stages():
        per = {}
        for name, row in zip(expr.output_names, expr.args):
            ops, hit = [], False
            for a in row:
                t = torch.ones(_shape(expr, a.name, case.E), dtype=torch.float64, device="cuda")
                if keys[a.name] == key:
                    t.zero_()
                    t[idx] = 1.0
                    hit = True
                ops.append(t)
            shape = tuple(case.E if isinstance(d, f.SizeParam) else int(d) for d in expr.shape)
            per[name] = (torch.einsum(expr.get_subscripts(), *ops) != 0) if hit else \
                torch.zeros(shape, dtype=torch.bool, device="cuda")
        out.append(per)
    return out


# --------------------------------------------------------------------------
# whole-array checks of large launches
# --------------------------------------------------------------------------

LARGE_E = (98_304, 100_000, 100_007, 131_077, 163_856, 1_000_007)
QUARTER_E = (98_304, 100_000, 100_007)
LARGE_LAUNCHES = ("grad", "grad_t", "div", "fm", "fm_ifj", "fm_jfi", "fm_fji", "bgrad", "bdiv", "pipeline")
KNOBS = ("tail_rounds", "quarter_tail", "staggered_start", "temporal_loads", "write_through", "prepared", "alloc")


def large_cases(seed: int, sizes: Sequence[int] = LARGE_E, f32: bool = True) -> List[Tuple[DGCase, Dict[str, Any]]]:
    """Each launch at each size with a random setting of every knob, float64, p = 4; float32 grad / div / face-mass at
    E = 70 004 and 1 000 004."""
    rng = random.Random(seed + 11)
    out = []
    for E in sizes:
        for launch_ in LARGE_LAUNCHES:
            kind = {"grad_t": "grad", "bgrad": "bgrad", "bdiv": "bdiv"}.get(launch_, launch_)
            op = "rji" if launch_ == "grad_t" else "rij"
            b = 3 if launch_ in ("bgrad", "bdiv") else 4 if launch_.startswith("fm") else 2
            case = DGCase(kind, 35, 15, b, op, "float64", E, "large", rng.randrange(1 << 30), "normal", rng.random() < 0.7)
            knobs = {"tail_rounds": rng.choice([None, -1]), "quarter_tail": rng.choice([True, False]),
                     "staggered_start": rng.choice([True, False]), "temporal_loads": rng.choice([None, 0, 248]),
                     "write_through": rng.choice([None, 0, 64, 4096]), "prepared": rng.random() < 0.4,
                     "alloc": rng.choice(["split", "torch"])}
            out.append((case, knobs))
    for E in QUARTER_E if tuple(sizes) == LARGE_E else ():   # quarter tails on (static walk, plain operators)
        for launch_ in ("grad", "grad_t", "div"):
            case = DGCase("grad" if launch_ == "grad_t" else launch_, 35, 15, 1, "rji" if launch_ == "grad_t" else "rij",
                          "float64", E, "large", rng.randrange(1 << 30))
            out.append((case, {"tail_rounds": -1, "quarter_tail": True, "staggered_start": False,
                               "temporal_loads": rng.choice([None, 0, 248]), "prepared": False,
                               "alloc": rng.choice(["split", "torch"])}))
    for E in (70_004, 1_000_004) if f32 else ():
        for kind in ("grad", "div", "fm"):
            out.append((DGCase(kind, 35, 15, 4 if kind == "fm" else 1, "rij", "float32", E, "large",
                               rng.randrange(1 << 30)), {"alloc": "torch"}))
    return out


def device_data(torch, case: DGCase):
    """Exact data made on the device (large E): ``(tensors by key, scales, significand)``; mantissas are recovered from
    the values for the slice checks (``x * 2**-s`` is exact)."""
    rng = np.random.default_rng(case.seed)
    bits, scales, dtypes, sig = plan_data(case, rng)
    gen = torch.Generator(device="cuda").manual_seed(case.seed)
    dev = {}
    for expr, keys in case.stages():
        for nm, k in keys.items():
            if k in dev:
                continue
            top = (1 << bits[k]) - 1
            m = torch.randint(-top, top + 1, _shape(expr, nm, case.E), dtype=torch.int64, device="cuda", generator=gen)
            # (a Python float power of two: torch.ldexp scales by a device pow(2, s), which need not be exact)
            x = m.to(torch.float64) * math.ldexp(1.0, scales[k])
            assert torch.equal(x * math.ldexp(1.0, -scales[k]), m.to(torch.float64)), "operand not exact"
            dev[k] = x.to(getattr(torch, dtypes[k].name))
            del m, x
    return dev, scales, sig


def _device_refs(torch, case: DGCase, dev, scales, sig, st: Stats):
    """references() for device-made data: torch's float64 einsum, checked against the int64 einsum on slices."""
    mants = _SliceMants(torch, dev, scales)
    return references(torch, case, None, mants, scales, sig, dev, st)


class _SliceMants:
    """Mantissas by key, made from the device values of one slice at a time (``x * 2**-s`` is exact)."""

    def __init__(self, torch, dev, scales):
        self._torch, self._dev, self._scales = torch, dev, scales

    def slice(self, k, ax, e0, w):
        t = self._dev[k] if ax is None else self._dev[k].narrow(ax, e0, w)
        return np.ldexp(t.to(self._torch.float64).cpu().numpy(), -self._scales[k]).astype(np.int64)


def _take(mants, k, ax, e0, w):
    if isinstance(mants, _SliceMants):
        return mants.slice(k, ax, e0, w)
    return np.take(mants[k], range(e0, e0 + w), axis=ax) if ax is not None else mants[k]


def run_large(seed: int, sizes: Sequence[int] = LARGE_E, only: Optional[Sequence[str]] = None, f32: bool = True) -> Stats:
    """Whole-array exact checks of :func:`large_cases`; every knob is restored afterwards."""
    import torch

    st = Stats(f"dg large seed={seed}")
    saved = (_hip.set_tail_rounds(0), _hip.set_grad_quarter_tail(True), _hip.set_div_quarter_tail(True),
             _hip.set_grad_staggered_start(True), _hip.set_temporal_loads_mib(0), _hip.set_write_through_mib(0))
    restore = lambda: (_hip.set_tail_rounds(saved[0]), _hip.set_grad_quarter_tail(saved[1]),  # noqa: E731
                       _hip.set_div_quarter_tail(saved[2]), _hip.set_grad_staggered_start(saved[3]),
                       _hip.set_temporal_loads_mib(saved[4]), _hip.set_write_through_mib(saved[5]))
    restore()
    try:
        for case, knobs in large_cases(seed, sizes, f32):
            if only is not None and case.kind not in only:
                continue
            dev, scales, sig = device_data(torch, case)
            refs = _device_refs(torch, case, dev, scales, sig, st)
            restore()
            if knobs.get("tail_rounds") is not None:
                _hip.set_tail_rounds(knobs["tail_rounds"])
            if "quarter_tail" in knobs:
                _hip.set_grad_quarter_tail(knobs["quarter_tail"])
                _hip.set_div_quarter_tail(knobs["quarter_tail"])
            if "staggered_start" in knobs:
                _hip.set_grad_staggered_start(knobs["staggered_start"])
            if knobs.get("temporal_loads") is not None:
                _hip.set_temporal_loads_mib(knobs["temporal_loads"])
            if knobs.get("write_through") is not None:
                _hip.set_write_through_mib(knobs["write_through"])
            transform = {"prepared": True} if knobs.get("prepared") else None
            label = f"large {case.kind} {case.op} {case.dtype} E={case.E} b={case.b} fuse={case.fuse} {knobs}"
            if knobs.get("alloc") == "split":   # outputs from the library's own allocation (placement.empty)
                stages = [(expr, {nm: dev[k] for nm, k in keys.items()}) for expr, keys in case.stages()]
                if case.kind == "pipeline":
                    outs = f.evaluate_operator(stages, 0, transform=transform, fuse=case.fuse, wait=True)
                else:
                    outs = [f.evaluate(stages[0][0], 0, stages[0][1], transform=transform, wait=True)]
                info, bufs = _hip.last_launch_info(), []
            else:
                bufs, outs = _out_buffers(torch, case)
                if case.kind == "pipeline":
                    stages = [(expr, {nm: dev[k] for nm, k in keys.items()}) for expr, keys in case.stages()]
                    f.evaluate_operator(stages, 0, out_dicts=outs, transform=transform, fuse=case.fuse, wait=True)
                    info = _hip.last_launch_info()
                else:
                    info = launch(torch, case, dev, transform, outs)
            restore()
            st.cov.update([f"large:{case.kind}", f"dtype:{case.dtype}", f"alloc:{knobs.get('alloc')}",
                           *(["prepared"] if transform else []), *_walk_buckets(case, info)])
            _compare(st, label, refs, outs, bufs, case)
            del dev, refs, outs, bufs
    finally:
        restore()
    return st


# --------------------------------------------------------------------------
# operands at every accepted address offset
# --------------------------------------------------------------------------

#: elements of NaN (inputs) or SENTINEL (outputs) on either side of an embedded array; 4 and 8 x BAND bytes are
#: multiples of 256
BAND = 1024
assert BAND >= GUARD and BAND * 4 % 256 == 0
#: the bands of an input: NaNs with this payload (integer view), so that "unchanged" is a bitwise statement
IN_NAN = {8: 0x7FF8_0000_DEAD_BEEF, 4: 0x7FC0_BEEF}
#: the payload of an output before the launch: a NaN no arithmetic makes, so an entry that was never written can be
#: told from a NaN that was computed from an over-read
OUT_NAN = {8: 0x7FF8_0000_0000_0BAD, 4: 0x7FC0_0BAD}
K_MAX_FIELDS = 8   # fe_common.h kMaxFields: fields per launch group
PLACEMENTS = ("aligned", "only:geometry", "only:operator", "only:field", "only:last-field", "only:output",
              "only:last-output", "all", "mixed")
FULL_TRANSFORMS = ("auto", "mfma")   # every placement; the other transforms run "aligned" and "all"
#: orders with float32 matrix-core kernels (fe_launch_f32), and the kinds that reach them
F32_MFMA_ORDERS = ((4, 3), (10, 6), (20, 10), (35, 15))
F32_MFMA_KINDS = ("grad", "div", "bgrad", "bdiv", "fm", "fm_ifj", "fm_jfi", "fm_fji")


class Embedded:
    """An array ``shift`` elements past a 256-byte boundary inside a larger buffer (:func:`embed`)."""

    def __init__(self, torch, buf, lead: int, shape, role: str, shift: int) -> None:
        self._torch, self.buf, self.lead, self.role, self.shift = torch, buf, lead, role, shift
        self.n = int(np.prod(shape, dtype=np.int64)) if len(shape) else 1
        self.view = buf[lead:lead + self.n].view(tuple(shape))
        self.esize = buf.element_size()

    def ints(self):
        """The whole buffer, bands and payload, as integers."""
        return self.buf.view(self._torch.int64 if self.esize == 8 else self._torch.int32)

    def bands(self):
        return self.buf[:self.lead], self.buf[self.lead + self.n:]

    def guards_intact(self) -> bool:
        """(outputs) both bands still hold SENTINEL."""
        lo, hi = self.bands()
        return bool((lo == SENTINEL).all()) and bool((hi == SENTINEL).all())

    def snapshot(self, checksum: bool = False):
        """A copy of :meth:`ints`, or with *checksum* its integer sum and xor."""
        return _checksum(self.ints()) if checksum else self.ints().clone()

    def unchanged(self, snap) -> bool:
        if isinstance(snap, tuple):
            return _checksum(self.ints()) == snap
        return bool(self._torch.equal(self.ints(), snap))

    def first_change(self, snap) -> Optional[int]:
        """Index, relative to the array's first element, of the first changed entry (negative: the band in front)."""
        if isinstance(snap, tuple):
            return None
        where = (self.ints() != snap).nonzero()
        return int(where[0]) - self.lead if len(where) else None


def _checksum(ints) -> Tuple[int, int]:
    """``(sum mod 2^64, xor)`` of an integer tensor."""
    import torch

    x = ints.reshape(-1)
    total = int(x.sum(dtype=torch.int64))
    while x.numel() > 1:
        h = x.numel() // 2
        folded = x[:h] ^ x[h:2 * h]
        if x.numel() % 2:
            folded[0] ^= x[2 * h]
        x = folded
    return total, int(x[0]) if x.numel() else 0


def embed(torch, shape, dtype, shift: int, role: str, values=None, device: str = "cuda") -> Embedded:
    """Place an array of *shape* ``shift`` elements past a 256-byte boundary of a new buffer, at least :data:`BAND`
    elements from either end.  *role* ``"in"``: the bands are NaNs of payload :data:`IN_NAN`, the array is *values*;
    ``"out"``: the bands are SENTINEL, the array NaNs of payload :data:`OUT_NAN`.  The address of the view is ``shift``
    elements mod 256 bytes, so mod 16 exactly ``shift * itemsize % 16`` (asserted)."""
    esize = 4 if dtype == torch.float32 else 8
    assert dtype in (torch.float32, torch.float64) and 0 <= shift < 16 // esize and role in ("in", "out")
    n = int(np.prod(shape, dtype=np.int64)) if len(shape) else 1
    buf = torch.empty(n + 2 * BAND + 256 // esize + 4, dtype=dtype, device=device)
    base = buf.data_ptr()
    assert base % esize == 0
    lead = BAND + (-base % 256) // esize + shift
    emb = Embedded(torch, buf, lead, shape, role, shift)
    ints = emb.ints()
    if role == "in":
        ints.fill_(IN_NAN[esize])
        emb.view.copy_(values)
    else:
        buf.fill_(SENTINEL)
        ints[lead:lead + n] = OUT_NAN[esize]
    ptr = emb.view.data_ptr()
    assert ptr % 256 == shift * esize and ptr % 16 == shift * esize % 16, (ptr, shift, esize)
    assert emb.view.is_contiguous() and tuple(emb.view.shape) == tuple(shape)
    assert lead >= BAND and buf.numel() - lead - n >= BAND
    return emb


@dataclass(frozen=True)
class PlacedRun:
    """One launch of the placement pass: the case, its data ("exact" / "signed"), the transform's name, the
    placement's name and its non-zero shifts (elements) by slot: a data key, or ``out:<stage>:<output name>``."""

    case: DGCase
    data: str
    transform: str
    placement: str
    shifts: Tuple[Tuple[str, int], ...] = ()
    knobs: Tuple[Tuple[str, Any], ...] = ()

    def repro(self) -> str:
        return json.dumps({"case": asdict(self.case), "data": self.data, "transform": self.transform,
                           "placement": self.placement, "shifts": dict(self.shifts), "knobs": dict(self.knobs)},
                          separators=(",", ":"))

    @staticmethod
    def from_repro(text: str) -> "PlacedRun":
        d = json.loads(text)
        return PlacedRun(DGCase(**d["case"]), d["data"], d["transform"], d["placement"],
                         tuple(sorted(d["shifts"].items())), tuple(sorted(d["knobs"].items())))


def slots_of(case: DGCase):
    """``(inputs, outputs)``: ``[(data key, role, numpy dtype, shape)]`` in the order of first use, role "geometry",
    "operator" or "field" as in :func:`plant_sites`; ``[(slot, stage, output name, numpy dtype, shape)]``."""
    ins: Dict[str, Tuple[str, str, Any, Tuple[int, ...]]] = {}
    outs = []
    out_dt = np.dtype("float32") if case.dtype == "float32" else np.dtype("float64")
    for s, (expr, keys) in enumerate(case.stages()):
        for row in expr.args:
            for a in row:
                role = "operator" if _e_axis(expr, a.name) is None else "field" if a is row[-1] else "geometry"
                ins.setdefault(keys[a.name], (keys[a.name], role, np.dtype(a.dtype), _shape(expr, a.name, case.E)))
        shape = tuple(case.E if isinstance(d, f.SizeParam) else int(d) for d in expr.shape)
        outs += [(f"out:{s}:{name}", s, name, out_dt, shape) for name in expr.output_names]
    return list(ins.values()), outs


def placements_of(case: DGCase, full: bool) -> List[Tuple[str, Tuple[Tuple[str, int], ...]]]:
    """``(placement name, non-zero shifts)`` of the case (deterministic in ``case.seed``): "aligned" first; with *full*
    every ``only:<role>`` (each geometry and operator array, the first and the last field and output, and one of each
    in the second launch group of more than K_MAX_FIELDS fields), "all" and "mixed"; else "aligned" and "all".  A
    float64 array shifts by one element (8 bytes); float32 arrays take 1, 2 and 3 elements in turn ("only:"), or at
    random ("all", "mixed")."""
    rng = random.Random(case.seed + 31)
    ins, outs = slots_of(case)
    dts = {**{k: dt for k, _, dt, _ in ins}, **{slot: dt for slot, _, _, dt, _ in outs}}
    turn = [case.seed % 3]

    def nz(slot: str, random_: bool = False) -> int:
        if dts[slot].itemsize == 8:
            return 1
        if random_:
            return rng.choice([1, 2, 3])
        turn[0] += 1
        return 1 + turn[0] % 3

    everything = list(dts)
    out = [("aligned", ())]
    if full:
        fields = [k for k, role, _, _ in ins if role == "field"]
        oslots = [slot for slot, *_ in outs]
        only = [("only:geometry", k) for k, role, _, _ in ins if role == "geometry"]
        only += [("only:operator", k) for k, role, _, _ in ins if role == "operator"]
        only += [("only:field", fields[0])] + ([("only:last-field", fields[-1])] if len(fields) > 1 else [])
        only += [("only:field", fields[K_MAX_FIELDS])] if len(fields) > K_MAX_FIELDS else []
        only += [("only:output", oslots[0])] + ([("only:last-output", oslots[-1])] if len(oslots) > 1 else [])
        only += [("only:output", oslots[K_MAX_FIELDS])] if len(oslots) > K_MAX_FIELDS and case.kind != "pipeline" else []
        out += [(name, ((slot, nz(slot)),)) for name, slot in only]
    out.append(("all", tuple(sorted((slot, nz(slot, True)) for slot in everything))))
    if full and len(everything) > 1:
        while True:
            pick = [slot for slot in everything if rng.random() < 0.5]
            if 0 < len(pick) < len(everything):
                break
        out.append(("mixed", tuple(sorted((slot, nz(slot, True)) for slot in pick))))
    return out


def _c(kind, order, b, op, dtype, E, seed, scale="normal", fuse=True) -> DGCase:
    return DGCase(kind, order[0], order[1], b, op, dtype, E, eclass_of(E), seed, scale, fuse)


def placement_cases(seed: int) -> Dict[str, List[DGCase]]:
    """The fixed list, by part.  "small": every kind, every matrix-core order, a tiled-only and a triangle order, E in
    {1, 5, 16, 17, 64, 65, 1003, 4099} (the large E with the low orders: the host references stay cheap); float32 at
    E in {16, 64, 1024, 4096}, where only the pointer can keep a launch off the matrix cores, and at 17 and 1003;
    mixed; the fused operator both ways.  These run on exact and on signed data.  "range": an overflow and a
    subnormal case per dtype.  "rounds": p = 4 at E = 20 004 (several rounds of the walk).  "large": quarter tails on
    a static walk (grad, div at 100 007) and the dynamic walk (grad at 170 003)."""
    rng = random.Random(seed + 29)
    o1, o2, o3, o4, o5, t7, t13 = ORDERS3
    small = []
    ops = ["rij", "rji"]

    def add(kind, order, E, b=1, dtype="float64", fuse=True):
        op = ops[len(small) % 2]
        small.append(_c(kind, order, b, op[1:] if kind in ("mass", "apply") else op, dtype, E, rng.randrange(1 << 30),
                        "normal", fuse))

    for order, E in ((o1, 4099), (o2, 1003), (o3, 65), (o4, 17), (o5, 16), (t7, 64), (o4, 1), (o4, 5)):
        add("grad", order, E)
    for order, E in ((o1, 1003), (o2, 4099), (o3, 17), (o4, 65), (o5, 5), (t13, 16)):
        add("div", order, E)
    for order, E, b in ((o1, 65, 9), (o2, 17, 2), (o3, 1003, 1), (o4, 64, 3), (o5, 16, 2)):
        add("fm", order, E, b)
    add("bgrad", o3, 64, 9)
    add("bdiv", o2, 65, 9)
    add("divcomp", o4, 17)
    add("cross", o3, 65)
    add("fm_ifj", o2, 16, 2)
    add("fm_jfi", o4, 5, 2)
    add("fm_fji", o3, 1003, 3)
    add("mass", o4, 64, 2)
    add("apply", o5, 17)
    add("grad2", ORDERS2[2], 65)
    add("div2", ORDERS2[3], 17)
    add("lift2", ORDERS2[1], 64, 2)
    add("pipeline", o3, 65, 2, fuse=True)
    add("pipeline", o2, 1003, 3, fuse=False)
    for order, E in ((o4, 16), (o3, 64), (o2, 1024), (o1, 4096), (o4, 17)):
        add("grad", order, E, dtype="float32")
    for order, E in ((o4, 64), (o3, 16), (o2, 4096), (o1, 1024), (o3, 1003)):
        add("div", order, E, dtype="float32")
    for order, E, b in ((o4, 1024, 2), (o3, 4096, 1), (o2, 16, 3), (o1, 64, 9)):
        add("fm", order, E, b, dtype="float32")
    add("bgrad", o3, 64, 9, dtype="float32")
    add("grad", o3, 64, dtype="mixed")
    add("fm", o2, 65, 2, dtype="mixed")
    S = lambda: rng.randrange(1 << 30)   # noqa: E731
    range_ = [_c("grad", o3, 1, "rij", "float64", 17, S(), "overflow"), _c("div", o2, 1, "rji", "float64", 65, S(), "subnormal"),
              _c("grad", o2, 1, "rij", "float32", 64, S(), "overflow"), _c("fm", o3, 2, "rij", "float32", 16, S(), "subnormal")]
    rounds = [_c("grad", o4, 1, "rij", "float64", 20_004, S()), _c("div", o4, 1, "rij", "float64", 20_004, S()),
              _c("fm", o4, 2, "rij", "float64", 20_004, S()), _c("grad", o3, 1, "rij", "float32", 20_004, S())]
    large = [_c("grad", o4, 1, "rij", "float64", 100_007, S()), _c("div", o4, 1, "rij", "float64", 100_007, S()),
             _c("grad", o4, 1, "rij", "float64", 170_003, S())]
    return {"small": small, "range": range_, "rounds": rounds, "large": large}


#: knobs of the three large cases (as :func:`large_cases`): quarter tails on a static walk; the defaults (dynamic walk)
LARGE_KNOBS = {100_007: (("quarter_tail", True), ("staggered_start", False), ("tail_rounds", -1)), 170_003: ()}


def placement_runs(seed: int, part: str) -> List[List[PlacedRun]]:
    """The runs of *part* ("exact", "signed" or "large"), one list per case, grouped by transform with "aligned" in
    front of each group."""
    cases = placement_cases(seed)
    data = "signed" if part == "signed" else "exact"
    todo = cases["large"] if part == "large" else cases["small"] + (cases["range"] + cases["rounds"] if part == "exact" else [])
    out = []
    for case in todo:
        runs = []
        for t in ["auto"] if part == "large" else [tname(t) for t in case.transforms()]:
            full = t in FULL_TRANSFORMS and part != "large"
            runs += [PlacedRun(case, data, t, name, shifts, LARGE_KNOBS[case.E] if part == "large" else ())
                     for name, shifts in placements_of(case, full)]
        out.append(runs)
    return out


def placement_buckets(run: PlacedRun) -> List[str]:
    case, t = run.case, run.transform
    ins, outs = slots_of(case)
    dts = {**{k: dt for k, _, dt, _ in ins}, **{slot: dt for slot, _, _, dt, _ in outs}}
    roles = {k: role for k, role, _, _ in ins}
    b = buckets_of(case, t) + ["place:" + run.placement]
    sizes = sorted({(dts[slot].itemsize, s * dts[slot].itemsize) for slot, s in run.shifts})
    b += [f"shift:f{8 * w}:{nbytes}" for w, nbytes in sizes]
    mfma = t in FULL_TRANSFORMS
    if mfma and run.placement.startswith("only:"):
        b.append(f"role:{case.kind}:{run.placement[5:]}")
    fam = "fm" if case.kind.startswith("fm") else case.kind[1:] if case.kind in ("bgrad", "bdiv") else case.kind
    if case.dtype == "float32" and fam in ("grad", "div", "fm"):
        b += [f"shift:f32:{nbytes}:{fam}" for w, nbytes in sizes if w == 4]
    if (mfma and case.dtype == "float32" and case.kind in F32_MFMA_KINDS and (case.Np, case.Nfp) in F32_MFMA_ORDERS
            and case.E % 4 == 0 and case.E >= 16 and run.shifts):
        b.append("path:f32-pointer-fallback")
    if (mfma and case.dtype == "float64" and case.kind in ("grad", "bgrad") and case.Np in PADDED_ORDERS and case.E >= 16
            and any(roles.get(slot) == "field" for slot, _ in run.shifts)):
        b.append("path:lds-dma-8")
    return b


def placement_coverage(seed: int, part: str) -> Counter:
    """Host-only counterpart of the pass's coverage (:func:`accepted_on_host` per case and transform)."""
    cnt: Counter = Counter()
    for runs in placement_runs(seed, part):
        ok: Dict[str, bool] = {}
        for run in runs:
            if run.transform not in ok:
                ok[run.transform] = accepted_on_host(run.case, _transform_of(run))
            if ok[run.transform]:
                cnt.update(placement_buckets(run))
    return cnt


def _transform_of(run: PlacedRun) -> Any:
    if run.case.kind == "pipeline":
        return None
    return {"prepared": True} if run.transform == "prepared" else run.transform


def _pair_minimums() -> Dict[str, int]:
    """Every (kind, role) pair once under "auto" or "mfma"."""
    m = {}
    for kind in KINDS + ("pipeline",):
        roles = ["operator", "field", "output"]
        roles += ["geometry"] if kind != "apply" else []
        roles += ["last-field", "last-output"] if kind not in ("grad", "div", "apply", "grad2", "div2") else []
        m.update({f"role:{kind}:{r}": 1 for r in roles})
    return m


#: minimum runs per bucket of the fixed-seed placement pass, by part (tests/test_dg_placement_cpu.py,
#: tests/test_gpu_dg_placement.py): every (kind, role) pair under "auto" or "mfma", every float32 shift per family
PLACEMENT_MINIMUMS = {
    "exact": {**_pair_minimums(),
              **{f"shift:f32:{n}:{fam}": 1 for n in (4, 8, 12) for fam in ("grad", "div", "fm")},
              "place:aligned": 200, "place:only:geometry": 80, "place:only:operator": 80, "place:only:field": 80,
              "place:only:last-field": 30, "place:only:output": 80, "place:only:last-output": 30, "place:all": 200,
              "place:mixed": 80, "shift:f64:8": 400, "shift:f32:4": 60, "shift:f32:8": 60, "shift:f32:12": 60,
              "path:f32-pointer-fallback": 100, "path:lds-dma-8": 30,
              **{f"family:{k}": 10 for k in KINDS}, "family:pipeline": 20,
              **{f"order:3d-{n}": 10 for n, _ in ORDERS3}, "order:2d-6": 10, "order:2d-10": 10, "order:2d-15": 10,
              "dtype:float64": 400, "dtype:float32": 200, "dtype:mixed": 20,
              "transform:auto": 300, "transform:mfma": 150, "transform:tiled": 50, "transform:generic": 50,
              "transform:prepared": 20, "E:one": 10, "E:sub-tile": 20, "E:tiles": 200, "E:ragged": 200,
              "E:static-rounds": 40, "range:overflow": 20, "range:subnormal": 20, "fused:yes": 10, "fused:no": 10},
    "signed": {"place:aligned": 150, "place:all": 150, "place:mixed": 60, "place:only:field": 60,
               "place:only:geometry": 60, "place:only:operator": 60, "place:only:output": 60,
               "shift:f64:8": 300, "shift:f32:4": 50, "shift:f32:8": 50, "shift:f32:12": 50,
               "path:f32-pointer-fallback": 80, "path:lds-dma-8": 20, "dtype:float64": 300, "dtype:float32": 150,
               "dtype:mixed": 20, "transform:mfma": 100, "transform:tiled": 40, "transform:generic": 40},
    "large": {"place:aligned": 3, "place:all": 3, "shift:f64:8": 3, "family:grad": 4, "family:div": 2,
              "E:quarter-tail": 4, "E:dynamic": 2},
}


class _Knobs:
    """Set the walk and tail knobs of a large case; every knob is restored on exit (as :func:`run_large`)."""

    def __init__(self, knobs: Dict[str, Any]) -> None:
        self.knobs = knobs

    def __enter__(self):
        k = self.knobs
        self.saved = (_hip.set_tail_rounds(0), _hip.set_grad_quarter_tail(True), _hip.set_div_quarter_tail(True),
                      _hip.set_grad_staggered_start(True))
        self._restore()
        if k.get("tail_rounds") is not None:
            _hip.set_tail_rounds(k["tail_rounds"])
        if "quarter_tail" in k:
            _hip.set_grad_quarter_tail(k["quarter_tail"])
            _hip.set_div_quarter_tail(k["quarter_tail"])
        if "staggered_start" in k:
            _hip.set_grad_staggered_start(k["staggered_start"])

    def _restore(self) -> None:
        _hip.set_tail_rounds(self.saved[0])
        _hip.set_grad_quarter_tail(self.saved[1])
        _hip.set_div_quarter_tail(self.saved[2])
        _hip.set_grad_staggered_start(self.saved[3])

    def __exit__(self, *exc) -> None:
        self._restore()


def check_inputs(st: Stats, label: str, run, ins: Dict[str, Tuple[Embedded, Any]]) -> bool:
    """Every input buffer, bands and payload, is bitwise its snapshot."""
    ok = True
    for key, (emb, snap) in ins.items():
        if not emb.unchanged(snap):
            ok = False
            at = emb.first_change(snap)
            st.fail(f"{label}: input {key} changed by the launch" + (f" (first at element {at})" if at is not None else "")
                    + f"  REPRO {run.repro()}")
    return ok


def nan_entries(got, ref) -> Tuple[int, int]:
    """``(unwritten, leaked)``: entries of *got* that still hold :data:`OUT_NAN`, and other NaN entries where *ref*
    has none: only a value read from an input's NaN band can make those."""
    import torch

    esize = got.element_size()
    nan = torch.isnan(got)
    if ref is not None:
        nan = nan & ~torch.isnan(ref)
    unwritten = nan & (got.contiguous().view(torch.int64 if esize == 8 else torch.int32) == OUT_NAN[esize])
    return int(unwritten.sum()), int(nan.sum()) - int(unwritten.sum())


def check_outputs(st: Stats, label: str, run, outs: List[Dict[str, Embedded]], refs=None, aligned=None) -> bool:
    """Guard bands; NaNs from behind an input (``leak:`` bucket: the line says *over-read*) and unwritten entries; with
    *refs* every output bitwise the exact reference (:func:`_compare`); with *aligned* (integer copies of the outputs
    of the aligned launch) every output bitwise that launch's."""
    ok = True
    for per in outs:
        for name, emb in per.items():
            if not emb.guards_intact():
                ok = False
                st.fail(f"{label}: output {name}: wrote outside its output  REPRO {run.repro()}")
    for s, per in enumerate(outs):
        for name, emb in per.items():
            unwritten, leaked = nan_entries(emb.view, refs[s][name] if refs is not None else None)
            if leaked:
                ok = False
                st.cov["leak:nan-entries"] += leaked
                st.fail(f"{label}: output {name}: over-read: {leaked} NaN entries from behind an input  REPRO {run.repro()}")
            if unwritten:
                ok = False
                st.cov["unwritten:entries"] += unwritten
                st.fail(f"{label}: output {name}: {unwritten} entries never written  REPRO {run.repro()}")
    if refs is not None:
        ok = _compare(st, label, refs, [{n: e.view for n, e in per.items()} for per in outs], [], run) and ok
    if aligned is not None:
        for per, base in zip(outs, aligned):
            for name, emb in per.items():
                st.exact_runs += 1
                mine = emb.view.contiguous().view(base[name].dtype)
                bad = int((mine != base[name]).sum())
                if bad:
                    ok = False
                    st.fail(f"{label}: output {name}: {bad} entries differ bitwise from the aligned launch  REPRO {run.repro()}")
                else:
                    st.exact_equal += 1
    return ok


def _int_copy(torch, emb: Embedded):
    return emb.view.contiguous().view(torch.int64 if emb.esize == 8 else torch.int32).clone()


def _placed_case(torch, st: Stats, runs: Sequence[PlacedRun], checksum: bool = False) -> None:
    """All runs of one case: its data and references once, every input embedded once per shift (the launches must
    leave them unchanged, which every run checks), fresh outputs per run."""
    case, data = runs[0].case, runs[0].data
    refs = bounds = None
    if data == "exact":
        if case.E > 50_000:
            dev, scales, sig = device_data(torch, case)
            refs = _device_refs(torch, case, dev, scales, sig, st)
        else:
            arrays, mants, scales, sig = host_data(case)
            dev = {k: torch.from_numpy(np.ascontiguousarray(a)).cuda() for k, a in arrays.items()}
            refs = references(torch, case, arrays, mants, scales, sig, dev, st)
    else:
        nrng = np.random.default_rng(case.seed)
        host, dev = {}, {}
        for expr, keys in case.stages():
            for nm, k in keys.items():
                if k not in host:
                    host[k] = (nrng.random(_shape(expr, nm, case.E)) * 2 - 1).astype(expr.arg_to_dtype[nm])
                    dev[k] = torch.from_numpy(host[k]).cuda()
        bounds = []
        for expr, keys in case.stages():
            nb = ref_.bound_terms(expr.get_subscripts(), _extent(expr, case.E), 3)
            bounds.append({name: ref_.bounded_reference(expr.get_subscripts(), [host[keys[a.name]] for a in row]) + (nb,)
                           for name, row in zip(expr.output_names, expr.args)})
    u = ref_.U32 if case.dtype == "float32" else ref_.U64
    ins_slots, out_slots = slots_of(case)
    cache: Dict[Tuple[str, int], Tuple[Embedded, Any]] = {}
    aligned: Dict[str, Any] = {}     # transform -> integer copies of the aligned launch's outputs (None: not accepted)
    for run in runs:
        t = run.transform
        if run.placement != "aligned" and aligned.get(t) is None:
            continue     # the aligned launch of this (case, transform) is not accepted
        shifts = dict(run.shifts)
        ins = {}
        for key, _, dt, shape in ins_slots:
            at = (key, shifts.get(key, 0))
            if at not in cache:
                emb = embed(torch, shape, getattr(torch, dt.name), at[1], "in", dev[key])
                cache[at] = (emb, emb.snapshot(checksum))
            ins[key] = cache[at]
        outs: List[Dict[str, Embedded]] = [{} for _ in case.stages()]
        for slot, s, name, dt, shape in out_slots:
            outs[s][name] = embed(torch, shape, getattr(torch, dt.name), shifts.get(slot, 0), "out")
        label = f"placement {run.placement} {data} {t}: {case.kind} Np={case.Np} b={case.b} {case.op} {case.dtype}" \
                f" E={case.E} {case.scale}"
        try:
            with _Knobs(dict(run.knobs)):
                info = launch(torch, case, {k: e.view for k, (e, _) in ins.items()}, _transform_of(run),
                              [{n: e.view for n, e in per.items()} for per in outs])
        except NotImplementedError as exc:
            if run.placement == "aligned":
                st.cov["not-accepted:" + t] += 1
                aligned[t] = None
            else:
                st.fail(f"{label}: refused ({exc}), but the aligned launch is accepted  REPRO {run.repro()}")
            continue
        except f.InvalidParameterError as exc:
            st.fail(f"{label}: refused ({exc})  REPRO {run.repro()}")
            continue
        st.cov.update(placement_buckets(run) + _walk_buckets(case, info))
        check_inputs(st, label, run, ins)
        f64_family = case.dtype == "float64"
        base = aligned.get(t) if (data == "signed" and f64_family and run.placement != "aligned") else None
        check_outputs(st, label, run, outs, refs, base)
        if run.placement == "aligned":
            aligned[t] = [{n: _int_copy(torch, e) for n, e in per.items()} for per in outs]
        if bounds is not None:
            bk = placement_buckets(run)
            for per, bnd, base_ in zip(outs, bounds, aligned[t]):
                for name, emb in per.items():
                    if run.placement != "aligned" and torch.equal(_int_copy(torch, emb), base_[name]):
                        continue     # bitwise the aligned launch, which was held to the bound
                    r, ar, nb = bnd[name]
                    ratio = ref_.bound_ratio(emb.view.cpu().numpy(), r, ar, nb, u)
                    for b_ in bk:
                        st.worst[b_] = max(st.worst.get(b_, 0.0), ratio)
                    if ratio > 1:
                        st.fail(f"{label}: output {name}: |got - ref| = {ratio:.3g} x the bound  REPRO {run.repro()}")


def run_placement(seed: int, part: str = "all") -> Stats:
    """Every case of :func:`placement_cases` with its operands at every accepted address offset (DESIGN.md section
    3, "Alignment"): *part* "exact", "signed", "large" or "all"."""
    import torch

    st = Stats(f"dg placement {part} seed={seed}")
    st.cov["leak:nan-entries"] += 0
    for p in ("exact", "signed", "large") if part == "all" else (part,):
        for runs in placement_runs(seed, p):
            _placed_case(torch, st, runs, checksum=p == "large")
    return st


def repro_placement(text: str) -> Stats:
    """Replay one ``REPRO`` line of the placement pass (the aligned launch of its case and transform first)."""
    import torch

    run = PlacedRun.from_repro(text)
    st = Stats("repro")
    st.cov["leak:nan-entries"] += 0
    first = [PlacedRun(run.case, run.data, run.transform, "aligned", (), run.knobs)] if run.placement != "aligned" else []
    _placed_case(torch, st, first + [run], checksum=run.case.E > 50_000)
    return st


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--placement":
        st = run_placement(int(sys.argv[2]) if len(sys.argv) > 2 else 0)
        print(st.report())
        sys.exit(1 if st.failures else 0)
    if len(sys.argv) > 2 and sys.argv[1] == "--repro" and "placement" in json.loads(sys.argv[2]):
        st = repro_placement(sys.argv[2])
        print(st.report())
        sys.exit(1 if st.failures else 0)
    if len(sys.argv) > 2 and sys.argv[1] == "--repro":
        import torch

        st = Stats("repro")
        _exact_case(torch, DGCase.from_repro(sys.argv[2]), st)
        print(st.report())
        sys.exit(1 if st.failures else 0)
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 120
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else 0
    results = [run_exact(n, seed), run_bounded(n // 3, seed), run_nonfinite(n // 6, seed), run_poison(n // 8, seed),
               run_large(seed)]
    for s in results:
        print(s.report())
    sys.exit(1 if sum(s.failures for s in results) else 0)
