"""Seeded sweep of the DG family kernels (grad, div, face-mass, mass / operator apply, div components, the cross
product, triangles, the fused operator) through every transform that accepts them, against the references of
oracle/einsum_ref.py (test infrastructure, like tests/).

    python tools/fuzz_dg.py [n_cases] [seed]
    python tools/fuzz_dg.py --placement [seed]
    python tools/fuzz_dg.py --accumulate [seed]
    python tools/fuzz_dg.py --repro '<REPRO line of any kind>'

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

``run_accumulate`` accumulating evaluation, ``out <- alpha E + beta out``, on the routes "kernel",
                   "epilogue" and "axpby", the route predicted on the host (``measure.accumulate_route``) and asserted on
                   the device; a route refused on the host must be refused with every output bitwise unchanged.  Four
                   parts.  ``run_accumulate_exact``: exact operands, old outputs on the grid of the sum, nine factor
                   pairs; the contract ``fma(alpha, E, fl(beta old))`` fixes every bit: the whole array for powers of
                   two (:func:`combine_pow2`), a correctly rounded integer reference (:func:`combine_entry`) for general
                   factors, float32 rounded once, near overflow and in the subnormal range too.
                   ``run_accumulate_bounded``: signed data within ``gamma(K + 2, u) (|alpha| absref + |beta| |old|)``,
                   float64 bitwise the "axpby" route, powers of two bitwise torch's two passes.
                   ``run_accumulate_nonfinite``: a NaN / Inf in a field, a geometry factor, an operator entry or an old
                   output; poisoned old outputs under beta = 0; alpha = 0 with a non-finite E gives NaN.
                   ``run_accumulate_placement``: the placements of ``run_placement`` with the outputs holding old
                   values between sentinel bands.

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
            if k.startswith("fm:"):   # "fm:<J layout>:<R layout>": the eight layouts of the accumulating pass
                _, jl, rl = k.split(":")
                rshape = {"fij": (nf, Np, Nfp), "ifj": (Np, nf, Nfp), "fji": (nf, Nfp, Np), "jfi": (Nfp, nf, Np)}[rl]
                rows = [[A("J", ("E", nf) if jl == "ef" else (nf, "E")), A("R", rshape), A(f"v{i}", (nf, "E", Nfp), True)]
                        for i in range(b)]
                expr = f.batched_einsum(f"{jl},{rl},fej->ei", rows)
                return [(expr, {nm: nm for nm in expr.all_args})]
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


def plan_data(case: DGCase, rng: np.random.Generator, headroom: int = 0):
    """``(bits, scales, dtypes, significand)`` per data key (*headroom*: bits of the significand left unused, for the
    accumulating pass, which scales the sum and adds an old output to it)."""
    stages = case.stages()
    dtypes = {}
    rows = []
    for expr, keys in stages:
        for row in expr.args:
            rows.append(([keys[a.name] for a in row], _terms(expr)))
            for a in row:
                dtypes[keys[a.name]] = np.dtype(a.dtype)
    sig = (24 if case.dtype == "float32" else 53) - headroom
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


def host_data(case: DGCase, extra: int = 0, headroom: int = 0):
    """``(arrays by key, mantissas by key, scales, significand)`` of exact data for the case."""
    rng = np.random.default_rng(case.seed + 7919 * extra)
    bits, scales, dtypes, sig = plan_data(case, rng, headroom)
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


def device_data(torch, case: DGCase, headroom: int = 0):
    """Exact data made on the device (large E): ``(tensors by key, scales, significand)``; mantissas are recovered from
    the values for the slice checks (``x * 2**-s`` is exact)."""
    rng = np.random.default_rng(case.seed)
    bits, scales, dtypes, sig = plan_data(case, rng, headroom)
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
    acc: Tuple[Any, ...] = ()      # an accumulating run: (alpha, beta, forced route, old shift) of its AccCase

    def repro(self) -> str:
        d = {"case": asdict(self.case), "data": self.data, "transform": self.transform,
             "placement": self.placement, "shifts": dict(self.shifts), "knobs": dict(self.knobs)}
        if self.acc:
            d["accumulate"] = list(self.acc)
        return json.dumps(d, separators=(",", ":"))

    @staticmethod
    def from_repro(text: str) -> "PlacedRun":
        d = json.loads(text)
        return PlacedRun(DGCase(**d["case"]), d["data"], d["transform"], d["placement"],
                         tuple(sorted(d["shifts"].items())), tuple(sorted(d["knobs"].items())),
                         tuple(d.get("accumulate", ())))


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


# --------------------------------------------------------------------------
# accumulating evaluation: out <- alpha E + beta out
# --------------------------------------------------------------------------

#: the six pairs of tests/test_gpu_accumulate.py (AB), two general pairs (the second with |alpha| < 1 < |beta|) and a pair
#: of large powers of two
ACC_AB = ((1.0, 1.0), (-1.0, 1.0), (2.0, -0.5), (0.5, 0.0), (0.0, 1.0), (0.0, 0.0))
ACC_GENERAL = ((0.3, -1.7), (-0.7, 2.3))
ACC_BIG = ((-2.0 ** -3, 2.0 ** 5),)
ACC_PAIRS = ACC_AB + ACC_GENERAL + ACC_BIG
ACC_ROUTES = (None, "axpby", "kernel", "epilogue")
#: bits of the significand the operands of an accumulating case leave unused, and the bits of an old output's mantissa
#: below that budget: with |sum| <= 2^(sig - 8), |old mantissa| < 2^(sig - 16), old outputs 0 or 3 binary places above
#: the grid of the sum and factors 2^-3 ... 2^5, alpha sum + beta old is below 2^(sig - 3) grid units of the finest of
#: the three grids (:func:`acc_budget_ok`): exact for every power-of-two pair
ACC_HEADROOM = 8
ACC_OLD_BITS_BELOW = 8
ACC_OLD_SHIFTS = (0, 3)
#: general pairs: the correctly rounded reference covers the whole array up to this E; above it the first and the last
#: ACC_EDGE elements (a wave tile is at most 80 elements) and a seeded sample of ACC_SAMPLE entries
ACC_WHOLE_E = 129
ACC_EDGE = 80
ACC_SAMPLE = 4096
ACC_FM_KINDS = tuple(f"fm:{jl}:{rl}" for jl in ("ef", "fe") for rl in ("fij", "ifj", "fji", "jfi"))
ACC_KINDS = KINDS + ACC_FM_KINDS
TET_ORDERS = ORDERS3[:4]                    # p = 1..4: the orders of the three accumulating kernels
TEL_SIZES = ("tel-1", "tel", "tel+1", "2tel+3")
ACC_SMALL_E = (1, 5, 16, 17, 33, 64, 65, 129, 1003, 4099)
FORMAT = {np.dtype("float64"): (53, -1074, 1023), np.dtype("float32"): (24, -149, 127)}   # significand, quantum, emax


def is_pow2(x: float) -> bool:
    """Zero or a signed power of two."""
    return x == 0.0 or math.frexp(abs(x))[0] == 0.5


@dataclass(frozen=True)
class AccCase:
    """An accumulating case: the DG case, the factors as the caller passes them, the forced route (``None``: what
    ``measure.accumulate_route`` picks), the forward transform's name and how many binary places the grid of the old
    outputs lies above the grid of the sum.  ``case.E == -1``: a size named by ``case.eclass`` ("tel+1", ...,
    "second-tile") that :func:`acc_resolve` reads from the launcher."""

    case: DGCase
    alpha: float
    beta: float
    route: Optional[str] = None
    transform: str = "auto"
    old_shift: int = 0

    def repro(self) -> str:
        return json.dumps({"accumulate": {"alpha": self.alpha, "beta": self.beta, "route": self.route,
                                          "transform": self.transform, "old_shift": self.old_shift},
                           "case": asdict(self.case)}, separators=(",", ":"))

    @staticmethod
    def from_repro(text: str) -> "AccCase":
        d = json.loads(text)
        a = d["accumulate"]
        return AccCase(DGCase(**d["case"]), float(a["alpha"]), float(a["beta"]), a["route"], a["transform"],
                       int(a["old_shift"]))

    def out_dtype(self) -> np.dtype:
        return np.dtype("float32") if self.case.dtype == "float32" else np.dtype("float64")

    def factors(self) -> Tuple[float, float]:
        """``(alpha, beta)`` as the launch applies them: cast to float32 for float32 outputs."""
        if self.case.dtype == "float32":
            return float(np.float32(self.alpha)), float(np.float32(self.beta))
        return self.alpha, self.beta

    def pow2(self) -> bool:
        return is_pow2(self.alpha) and is_pow2(self.beta)

    def family(self) -> Optional[str]:
        """"fm", "grad" or "div" for the kinds the accumulating kernels serve."""
        k = self.case.kind
        return "fm" if k.startswith("fm") else k if k in ("grad", "div") else None


def acc_transform(ac: AccCase) -> Any:
    """The ``transform`` argument of the case: the forward transform and the forced route in one mapping."""
    t: Dict[str, Any] = {}
    if ac.transform == "prepared":
        t["prepared"] = True
    elif ac.transform != "auto":
        t["variant"] = ac.transform
    if ac.route is not None:
        t["accumulate"] = ac.route
    return t or None


def predicted_route(ac: AccCase) -> Optional[str]:
    """The route the host predicts (``measure.accumulate_route``), or ``None`` where the host refuses the case."""
    from feinsum_amd.measure import accumulate_route

    expr, _ = ac.case.stages()[0]
    try:
        launch_kind(expr, acc_transform(ac), {"E": max(ac.case.E, 1)})
        return accumulate_route(expr, acc_transform(ac))
    except NotImplementedError:
        return None


# ---- the combine reference: fl(alpha E + fl(beta old)), E exact

def _decompose(x: float) -> Tuple[int, int]:
    """``(m, e)`` with ``x == m * 2**e``, Python integers."""
    m, e = math.frexp(x)
    return int(m * (1 << 53)), e - 53


def fl_int(R: int, g: int, dtype) -> float:
    """``R * 2**g`` rounded to nearest, ties to even, into *dtype* (subnormals and overflow included): Python integers."""
    sig, quantum, emax = FORMAT[np.dtype(dtype)]
    if R == 0:
        return 0.0
    a = abs(R)
    qe = max(a.bit_length() - 1 + g - (sig - 1), quantum)
    drop = qe - g
    if drop > 0:
        q, rem = a >> drop, a & ((1 << drop) - 1)
        half = 1 << (drop - 1)
        if rem > half or (rem == half and q & 1):
            q += 1
    else:
        q, qe = a, g
    if q.bit_length() + qe - 1 > emax:
        return math.copysign(math.inf, R)
    return math.copysign(math.ldexp(float(q), qe), R)      # q <= 2**sig: exact


def combine_entry(ms: int, t: int, alpha: float, beta: float, old: float, dtype) -> float:
    """One entry of the contract: ``E = ms * 2**t`` exactly, ``p = fl(beta * old)`` (not read when beta is 0), then the
    single rounding of ``alpha * E + p``.  *alpha*, *beta* as the launch applies them (:meth:`AccCase.factors`)."""
    p = 0.0
    if beta != 0.0:
        mb, eb = _decompose(beta)
        mo, eo = _decompose(old)
        p = fl_int(mb * mo, eb + eo, dtype)
    ma, ea = _decompose(alpha)
    mp, ep = _decompose(p)
    if not mp:
        return fl_int(ma * ms, t + ea, dtype)
    g = min(t + ea, ep)
    return fl_int((ma * ms << (t + ea - g)) + (mp << (ep - g)), g, dtype)


def _bit_length(a: np.ndarray) -> np.ndarray:
    x, n = a.copy(), np.zeros(a.shape, dtype=np.int64)
    for s in (32, 16, 8, 4, 2, 1):
        big = (x >> s) != 0
        n += big * s
        x = np.where(big, x >> s, x)
    return n + (x != 0)


def round_to_format(R: np.ndarray, g: int, dtype) -> np.ndarray:
    """:func:`fl_int` on an int64 array with ``|R| < 2**60`` (no overflow of the format: asserted)."""
    sig, quantum, _ = FORMAT[np.dtype(dtype)]
    R = np.asarray(R, dtype=np.int64)
    a = np.abs(R)
    assert not a.size or int(a.max()) < (1 << 60)
    qe = np.maximum(_bit_length(a) - 1 + g - (sig - 1), quantum)
    drop = np.minimum(np.maximum(qe - g, 0), 61)
    q = a >> drop
    rem = a - (q << drop)
    half = np.where(drop > 0, np.int64(1) << np.maximum(drop - 1, 0), 0)
    q = q + ((drop > 0) & ((rem > half) | ((rem == half) & ((q & 1) == 1))))
    val = np.ldexp(q.astype(np.float64), (g + drop).astype(np.int64))
    out = (np.sign(R) * val).astype(np.dtype(dtype))
    assert np.isfinite(out).all(), "the reference overflows its format"
    return out


def combine_pow2(ms: np.ndarray, t: int, alpha: float, beta: float, mo: np.ndarray, go: int, dtype) -> np.ndarray:
    """The contract on whole arrays for factors that are zero or signed powers of two: ``E = ms * 2**t``,
    ``old = mo * 2**go``.  ``beta * old`` rounds where it falls below the quantum of the format, and so does the sum."""
    assert is_pow2(alpha) and is_pow2(beta)
    _, quantum, _ = FORMAT[np.dtype(dtype)]
    ms, mo = np.asarray(ms, dtype=np.int64), np.asarray(mo, dtype=np.int64)
    A, a = (0, 0) if alpha == 0 else (int(math.copysign(1, alpha)), math.frexp(abs(alpha))[1] - 1)
    B, b = (0, 0) if beta == 0 else (int(math.copysign(1, beta)), math.frexp(abs(beta))[1] - 1)
    p = round_to_format(B * mo, go + b, dtype).astype(np.float64)
    gp = max(quantum, go + b)
    g = min(t + a, gp) if A and B else (t + a) if A else gp
    P = np.ldexp(p, -g)
    assert (P == np.rint(P)).all()
    return round_to_format(A * ms * (1 << (t + a - g) if A else 0) + P.astype(np.int64), g, dtype)


def acc_old_bits(sig: int) -> int:
    """Mantissa bits of an old output, *sig* being the operands' budget (``plan_data`` with ACC_HEADROOM)."""
    return max(sig - ACC_OLD_BITS_BELOW, 1)


def acc_budget_ok(sig: int, out_sig: int) -> bool:
    """Whether ``alpha sum + beta old`` is exact for every power-of-two pair of :data:`ACC_PAIRS` and every old shift:
    in units of the finest grid involved the absolute value stays within ``2**out_sig`` (Python integers)."""
    ob = acc_old_bits(sig)
    for alpha, beta in ACC_PAIRS:
        if not (is_pow2(alpha) and is_pow2(beta)):
            continue
        a = math.frexp(abs(alpha))[1] - 1 if alpha else None
        b = math.frexp(abs(beta))[1] - 1 if beta else None
        for sh in ACC_OLD_SHIFTS:
            grids = [x for x in (a, None if b is None else b + sh) if x is not None]
            if not grids:
                continue
            g = min(grids)
            worst = ((1 << sig) << (a - g) if a is not None else 0) + ((1 << ob) << (b + sh - g) if b is not None else 0)
            if worst > (1 << out_sig):
                return False
    return True


def acc_old(ac_case: DGCase, sig: int, t: int, shift: int, out_dt) -> List[Tuple[np.ndarray, np.ndarray]]:
    """``[(mantissas, values)]`` per output: old outputs ``m * 2**(t + shift)`` on (a multiple of) the grid of the sum,
    the same for every pair of a case."""
    expr, _ = ac_case.stages()[0]
    shape = tuple(ac_case.E if isinstance(d, f.SizeParam) else int(d) for d in expr.shape)
    rng = np.random.default_rng(ac_case.seed + 104_729 + shift)
    top = (1 << acc_old_bits(sig)) - 1
    out = []
    for _ in expr.output_names:
        m = rng.integers(-top, top + 1, size=shape, dtype=np.int64)
        x = np.ldexp(m.astype(np.float64), t + shift).astype(out_dt)
        assert np.array_equal(np.ldexp(x.astype(np.float64), -(t + shift)), m.astype(np.float64)), "old output not exact"
        out.append((m, x))
    return out


# ---- the case list (host only)

def _sym(kind, order, b, op, eclass, seed) -> DGCase:
    return DGCase(kind, order[0], order[1], b, op, "float64", -1, eclass, seed)


def acc_cases(seed: int) -> List[AccCase]:
    """The fixed list of the exact part, cases of one DG case next to each other (they share data and references).
    Face-mass under "kernel" and the default route: all eight layouts at p = 1..4, b in 2, 3, 4, 5, 8.  grad and div
    under "epilogue": both operator layouts at p = 1..4.  Per kernel and order the sizes around the wave tile, one size
    of several rounds and, at p = 4, one at which a wave walks a second tile.  Every kind of KINDS under "axpby" with every
    forward transform, float64, float32 and mixed, and under the default route; face-mass with b = 1 ... 9 there.  Routes
    forced where they do not exist (refused on the host).  The range cases.  The nine factor pairs rotate."""
    rng = random.Random(seed + 41)
    S = lambda: rng.randrange(1 << 30)   # noqa: E731
    out: List[AccCase] = []
    turn = [0]

    def add(case: DGCase, route, transform="auto", n=3):
        for _ in range(n):
            alpha, beta = ACC_PAIRS[turn[0] % len(ACC_PAIRS)]
            turn[0] += 1
            out.append(AccCase(case, alpha, beta, route, transform, ACC_OLD_SHIFTS[turn[0] % 2]))

    bs = (2, 3, 4, 5, 8)
    for pi, order in enumerate(TET_ORDERS):
        for li, kind in enumerate(ACC_FM_KINDS):
            E = ACC_SMALL_E[(3 * pi + li) % (len(ACC_SMALL_E) - (1 if pi == 3 else 0))]
            case = _c(kind, order, bs[(pi + li) % 5], "rij", "float64", E, S())
            add(case, "kernel" if li % 2 else None, "mfma" if li % 4 == 3 else "auto", 4)
        for fi, fam in enumerate(("grad", "div")):
            for oi, op in enumerate(("rij", "rji")):
                E = ACC_SMALL_E[(2 * pi + 5 * fi + 3 * oi + 1) % len(ACC_SMALL_E)]
                add(_c(fam, order, 1, op, "float64", E, S()), "epilogue", "mfma" if (pi + oi) % 2 else "auto", 4)
        for k, sym in enumerate(TEL_SIZES):
            add(_sym(ACC_FM_KINDS[(2 * pi + k) % 8], order, bs[(pi + k) % 5], "rij", sym, S()), "kernel", n=2)
            add(_sym("grad", order, 1, ("rij", "rji")[k % 2], sym, S()), "epilogue", n=2)
            add(_sym("div", order, 1, ("rji", "rij")[k % 2], sym, S()), "epilogue", n=2)
    o1, o2, o3, o4, o5, t7, t13 = ORDERS3
    for kind, route in (("fm", "kernel"), ("grad", "epilogue"), ("div", "epilogue")):
        add(_c(kind, o4, 2, "rij", "float64", 20_004, S()), route, n=2)
        add(_sym(kind, o4, 2, "rij", "second-tile", S()), route, n=2)
    # every kind under "axpby" with every forward transform and under the default route
    dts = ("float64", "float32", "mixed")
    b7 = (1, 2, 3, 4, 5, 8, 9)
    for ki, kind in enumerate(KINDS):
        orders = ORDERS2 if kind.endswith("2") else ORDERS3
        for di in range(2):
            order = orders[(ki + 3 * di) % len(orders)]
            op = ("rij", "rji")[(ki + di) % 2]
            E = (17, 65, 64, 1003, 16, 5, 129)[(ki + 4 * di) % 7]
            case = _c(kind, order, b7[(ki + 3 * di) % 7], op[1:] if kind in ("mass", "apply") else op, dts[(ki + di) % 3], E, S())
            for t in TRANSFORMS:
                add(case, "axpby", t, 1)
            add(case, None, "auto", 1)
    for b in b7:       # face-mass of tetrahedra, float64, every field count: a single field takes "axpby" by default
        add(_c("fm", TET_ORDERS[b % 4], b, "rij", "float64", (65, 17, 129)[b % 3], S()), None, "auto", 2)
    for dt in dts:
        add(_c("fm", o3, 4, "rij", dt, 64, S()), None, "auto", 1)
        add(_c("fm", o2, 3, "rij", dt, 65, S()), "axpby", "mfma", 1)
    # routes forced where they do not exist: refused on the host, outputs untouched on the device
    for case, route, t in ((_c("grad", o3, 1, "rij", "float64", 65, S()), "kernel", "auto"),
                           (_c("fm", o3, 3, "rij", "float64", 65, S()), "epilogue", "auto"),
                           (_c("fm", o4, 1, "rij", "float64", 17, S()), "kernel", "auto"),
                           (_c("fm", o2, 9, "rij", "float64", 17, S()), "kernel", "mfma"),
                           (_c("grad", o5, 1, "rij", "float64", 64, S()), "epilogue", "auto"),
                           (_c("div2", ORDERS2[2], 1, "rij", "float64", 65, S()), "epilogue", "auto"),
                           (_c("fm", o3, 4, "rij", "float32", 64, S()), "kernel", "auto"),
                           (_c("div", o3, 1, "rij", "mixed", 64, S()), "epilogue", "auto"),
                           (_c("fm", o4, 4, "rij", "float64", 65, S()), "kernel", "tiled"),
                           (_c("grad", o2, 1, "rji", "float64", 65, S()), "epilogue", "generic")):
        add(case, route, t, 1)
    # the range cases
    for scale in ("overflow", "subnormal"):
        add(_c("fm:fe:jfi", o3, 3, "rij", "float64", 65, S(), scale), "kernel", n=4)
        add(_c("grad", o2, 1, "rji", "float64", 129, S(), scale), "epilogue", n=4)
        add(_c("div", o4, 1, "rij", "float64", 17, S(), scale), "epilogue", n=4)
        add(_c("cross", o3, 1, "rij", "float64", 33, S(), scale), "axpby", n=3)
        add(_c("grad", o3, 1, "rij", "float32", 64, S(), scale), "axpby", n=3)
        add(_c("fm", o2, 2, "rij", "float32", 17, S(), scale), None, n=3)
    return out


def acc_buckets(ac: AccCase) -> List[str]:
    case = ac.case
    route = predicted_route(ac)
    nd = "2d" if case.kind.endswith("2") else "3d"
    if route is None:
        return [f"refused:{ac.route}", f"refused-family:{case.kind}"]
    b = [f"family:{case.kind}", f"route:{route}", f"route:{route}:{nd}-{case.Np}", f"forced:{ac.route}",
         f"pair:{ac.alpha:g},{ac.beta:g}:{route}", f"dtype:{case.dtype}", f"range:{case.scale}", f"E:{case.eclass}",
         f"transform:{ac.transform}:{route}", "factors:" + ("pow2" if ac.pow2() else "general"), f"old-shift:{ac.old_shift}"]
    fam = ac.family()
    if fam == "fm" and case.dtype == "float64":
        b.append(f"fm-fields:{case.b}")
    if route == "kernel":
        layout = case.kind[3:] if case.kind.startswith("fm:") else {"fm": "ef:fij", "fm_fji": "ef:fji", "fm_ifj": "fe:ifj",
                                                                    "fm_jfi": "fe:jfi"}[case.kind]
        b.append(f"fm-layout:{layout}:p{TET_ORDERS.index((case.Np, case.Nfp)) + 1}")
    if route == "epilogue":
        b.append(f"op:{fam}:{case.op}:p{TET_ORDERS.index((case.Np, case.Nfp)) + 1}")
    if route in ("kernel", "epilogue") and case.eclass in TEL_SIZES + ("second-tile",):
        b.append(f"size:{fam}:p{TET_ORDERS.index((case.Np, case.Nfp)) + 1}:{case.eclass}")
    return b


def acc_coverage(cases: Sequence[AccCase]) -> Counter:
    cnt: Counter = Counter()
    for ac in cases:
        cnt.update(acc_buckets(ac))
    return cnt


def _pairs_by_route() -> Dict[str, int]:
    return {f"pair:{a:g},{b:g}:{r}": 1 for a, b in ACC_PAIRS for r in ("axpby", "kernel", "epilogue")}


#: minimum runs per bucket of the exact part of the accumulating pass (tests/test_dg_accumulate_cpu.py on the case list,
#: tests/test_gpu_dg_accumulate.py on what ran)
ACC_MINIMUMS = {
    **{f"family:{k}": 2 for k in KINDS}, **{f"family:{k}": 3 for k in ACC_FM_KINDS},
    "route:axpby": 150, "route:kernel": 120, "route:epilogue": 120,
    **{f"route:axpby:3d-{n}": 4 for n, _ in ORDERS3}, **{f"route:axpby:2d-{n}": 1 for n in (6, 10, 15)},
    **{f"route:{r}:3d-{n}": 20 for r in ("kernel", "epilogue") for n, _ in TET_ORDERS},
    **{f"fm-layout:{k[3:]}:p{p}": 2 for k in ACC_FM_KINDS for p in (1, 2, 3, 4)},
    **{f"op:{fam}:{op}:p{p}": 4 for fam in ("grad", "div") for op in ("rij", "rji") for p in (1, 2, 3, 4)},
    **{f"size:{fam}:p{p}:{s}": 2 for fam in ("fm", "grad", "div") for p in (1, 2, 3, 4) for s in TEL_SIZES},
    **{f"size:{fam}:p4:second-tile": 2 for fam in ("fm", "grad", "div")},
    **_pairs_by_route(), "forced:None": 30, "forced:axpby": 150, "forced:kernel": 60, "forced:epilogue": 120,
    "dtype:float64": 300, "dtype:float32": 50, "dtype:mixed": 40,
    **{f"transform:{t}:axpby": 10 for t in TRANSFORMS}, "transform:mfma:kernel": 8, "transform:mfma:epilogue": 8,
    **{f"fm-fields:{b}": 2 for b in (1, 2, 3, 4, 5, 8, 9)},
    "range:overflow": 15, "range:subnormal": 15, "factors:pow2": 300, "factors:general": 100,
    "old-shift:0": 150, "old-shift:3": 150, "E:one": 4, "E:sub-tile": 10, "E:tiles": 40, "E:ragged": 100, "E:static-rounds": 6,
    "refused:kernel": 4, "refused:epilogue": 5,
}


ACC_SHARES = ("kernel", "epilogue", "axpby", "rounds")


def acc_share(cases: Sequence[AccCase], share: str) -> List[AccCase]:
    """The cases of one share of the exact part (the GPU tests run one share each): "rounds" -- E = 20 004 and the
    second-tile sizes -- else by the predicted route, the refused cases with "axpby"."""
    def of(ac: AccCase) -> str:
        if ac.case.E > HOST_REF_MAX_E or ac.case.eclass == "second-tile":
            return "rounds"
        route = predicted_route(ac)
        return route if route in ("kernel", "epilogue") else "axpby"
    return [ac for ac in cases if of(ac) == share]


def acc_share_minimums(cases: Sequence[AccCase], share: str) -> Dict[str, int]:
    """What the share must deliver of :data:`ACC_MINIMUMS` when every other share delivers what the host predicts."""
    total, mine = acc_coverage(cases), acc_coverage(acc_share(cases, share))
    need = {k: v - (total[k] - mine[k]) for k, v in ACC_MINIMUMS.items()}
    return {k: v for k, v in need.items() if v > 0}


# ---- on the device

_ACC_GEOMETRY: Dict[Tuple[str, int], Tuple[int, int]] = {}


def acc_geometry(torch, fam: str, order: Tuple[int, int]) -> Tuple[int, int]:
    """``(TEL, E2)`` of an accumulating kernel at one order, from what the launcher reports (as ``geometry()`` of
    tests/test_gpu_accumulate.py): the wave tile TEL = E / tiles at an E that every wave tile divides, and E2 = waves x
    TEL + TEL + 5, at which some wave of the full grid walks a second tile."""
    if (fam, order[0]) not in _ACC_GEOMETRY:
        kind, route = ("fm", "kernel") if fam == "fm" else (fam, "epilogue")
        E = 4800     # 2^6 3 5^2: a multiple of the wave tiles (16, 32, 48, 80 elements)
        ac = AccCase(_c(kind, order, 2, "rij", "float64", E, 1), 1.0, 1.0, route)
        expr, _ = ac.case.stages()[0]
        dev = {nm: torch.zeros(_shape(expr, nm, E), dtype=torch.float64, device="cuda") for nm in expr.all_args}
        outs = {n: torch.zeros(tuple(E if isinstance(d, f.SizeParam) else int(d) for d in expr.shape), dtype=torch.float64,
                               device="cuda") for n in expr.output_names}
        assert acc_launch(ac, dev, outs) == route
        tel = E // _hip.last_launch_info()["tiles"]
        assert tel % 16 == 0 and E % tel == 0, (fam, order, tel)
        waves = 2 * torch.cuda.get_device_properties(0).multi_processor_count * 4   # two blocks of four waves per CU
        E2 = waves * tel + tel + 5
        assert E2 <= 2 * 10 ** 5
        _ACC_GEOMETRY[fam, order[0]] = (tel, E2)
    return _ACC_GEOMETRY[fam, order[0]]


def acc_resolve(torch, ac: AccCase) -> AccCase:
    """The case with its named size replaced by the element count (the class keeps the name)."""
    if ac.case.E >= 0:
        return ac
    tel, E2 = acc_geometry(torch, ac.family(), (ac.case.Np, ac.case.Nfp))
    E = {"tel-1": tel - 1, "tel": tel, "tel+1": tel + 1, "2tel+3": 2 * tel + 3, "second-tile": E2}[ac.case.eclass]
    return AccCase(DGCase(**{**asdict(ac.case), "E": E}), ac.alpha, ac.beta, ac.route, ac.transform, ac.old_shift)


def acc_launch(ac: AccCase, dev, outs) -> Optional[str]:
    """Bind (``measure._bind``, as tests/test_gpu_accumulate.py does) and launch onto *outs*, which hold the old
    values; returns ``bound.accumulate``."""
    from feinsum_amd.measure import _bind

    expr, keys = ac.case.stages()[0]
    q, bound, _ = _bind(expr, 0, {nm: dev[k] for nm, k in keys.items()}, outs, acc_transform(ac), alpha=ac.alpha, beta=ac.beta)
    bound.launch(q.stream_ptr)
    q.finish()
    return bound.accumulate


def _plain_accepted(torch, case: DGCase, dev, tr: str, cache: Dict[str, bool]) -> bool:
    """Whether the non-accumulating launch of the case under the forward transform is accepted on the device."""
    if tr not in cache:
        _, out_dicts = _out_buffers(torch, case)
        try:
            launch(torch, case, dev, {"prepared": True} if tr == "prepared" else tr, out_dicts)
            cache[tr] = True
        except NotImplementedError:
            cache[tr] = False
    return cache[tr]


def acc_run(torch, st: Stats, ac: AccCase, dev, olds, label: str, plain_ok: Dict[str, bool], guarded: bool = True):
    """One accumulating launch onto copies of *olds* (device tensors by output name) between guard bands.  Returns the
    outputs by name, or ``None`` where the launch was refused -- as the host predicted, with every output buffer bitwise
    unchanged (counted), or because the plain launch of the same forward transform is refused too (counted); any other
    refusal, a route other than the predicted one and a write outside an output are failures."""
    expr, _ = ac.case.stages()[0]
    want_route = predicted_route(ac)
    bufs, outs = [], {}
    for name in expr.output_names:
        buf, out, n = _guarded(torch, tuple(olds[name].shape), olds[name].dtype)
        out.copy_(olds[name])
        bufs.append((buf, n))
        outs[name] = out
    before = [buf.clone() for buf, _ in bufs]
    try:
        route = acc_launch(ac, dev, outs)
    except NotImplementedError as exc:
        torch.cuda.synchronize()
        same = all(torch.equal(buf.view(torch.int8), b.view(torch.int8)) for (buf, _), b in zip(bufs, before))
        if not same:
            st.fail(f"{label}: refused ({exc}) after writing to an output  REPRO {ac.repro()}")
        elif want_route is None:
            st.cov.update(acc_buckets(ac))
        elif not _plain_accepted(torch, ac.case, dev, ac.transform, plain_ok):
            st.cov["not-accepted:" + ac.transform] += 1
        else:
            st.cov["refused:unpredicted"] += 1
            st.fail(f"{label}: refused ({exc}), but the host predicts the route {want_route!r}  REPRO {ac.repro()}")
        return None
    if want_route is None or route != want_route:
        st.fail(f"{label}: took the route {route!r}, the host predicts {want_route!r}  REPRO {ac.repro()}")
        return None
    if not all(_guards_intact(buf, n) for buf, n in bufs):
        st.fail(f"{label}: wrote outside its output  REPRO {ac.repro()}")
        return None
    return outs


def _acc_label(part: str, ac: AccCase) -> str:
    c = ac.case
    return f"accumulate {part} {ac.route}/{ac.transform} ({ac.alpha:g}, {ac.beta:g}): {c.kind} Np={c.Np} b={c.b} {c.op}" \
           f" {c.dtype} E={c.E} {c.scale}"


def _sample_index(case: DGCase, expr, shape: Tuple[int, ...]) -> np.ndarray:
    """Flat indices of the entries a general pair is checked on: everything up to ACC_WHOLE_E elements, else the
    first and the last ACC_EDGE elements and ACC_SAMPLE seeded entries."""
    n = int(np.prod(shape, dtype=np.int64))
    if case.E <= ACC_WHOLE_E:
        return np.arange(n, dtype=np.int64)
    ax = _e_axis(expr, None)
    e = np.arange(n, dtype=np.int64).reshape(shape)
    edge = np.concatenate([np.take(e, range(ACC_EDGE), axis=ax).reshape(-1),
                           np.take(e, range(case.E - ACC_EDGE, case.E), axis=ax).reshape(-1)])
    rnd = np.random.default_rng(case.seed + 17).integers(0, n, size=ACC_SAMPLE)
    return np.unique(np.concatenate([edge, rnd]))


def acc_general_reference(ac: AccCase, ms: np.ndarray, t: int, old: np.ndarray) -> np.ndarray:
    """:func:`combine_entry` on flat arrays of mantissas of the sum and of old values."""
    alpha, beta = ac.factors()
    dt = ac.out_dtype()
    return np.array([combine_entry(int(m), t, alpha, beta, float(o), dt) for m, o in zip(ms, old)], dtype=dt)


def _acc_data(torch, case: DGCase, st: Stats):
    """Exact data with ACC_HEADROOM: ``(dev, refs of the plain einsum by output, integer sums by output or None, t, sig)``."""
    if case.E > 50_000:
        dev, scales, sig = device_data(torch, case, ACC_HEADROOM)
        refs = _device_refs(torch, case, dev, scales, sig, st)[0]
        mants = None
    else:
        arrays, mants, scales, sig = host_data(case, headroom=ACC_HEADROOM)
        dev = {k: torch.from_numpy(np.ascontiguousarray(a)).cuda() for k, a in arrays.items()}
        refs = references(torch, case, arrays, mants, scales, sig, dev, st)[0]
    expr, keys = case.stages()[0]
    t = sum(scales[keys[a.name]] for a in expr.args[0])
    sums = None
    if mants is not None and case.E <= HOST_REF_MAX_E:
        sums = {name: np.asarray(np.einsum(expr.get_subscripts(), *[mants[keys[a.name]] for a in row], optimize=True),
                                 dtype=np.int64) for name, row in zip(expr.output_names, expr.args)}
    return dev, refs, sums, t, sig


def acc_check_exact(torch, st: Stats, ac: AccCase, label: str, outs, refs, sums, t: int, olds_host) -> None:
    """Power-of-two pairs: the whole array, bitwise.  General pairs: the correctly rounded reference on
    :func:`_sample_index`, bitwise."""
    expr, _ = ac.case.stages()[0]
    alpha, beta = ac.factors()
    dt = ac.out_dtype()
    for k, name in enumerate(expr.output_names):
        mo, old = olds_host[k]
        got = outs[name]
        st.exact_runs += 1
        if ac.pow2():
            if sums is not None:
                want = torch.from_numpy(combine_pow2(sums[name], t, alpha, beta, mo, t + ac.old_shift, dt)).cuda()
            else:   # (large E, normal range: every term exact in float64 by the bit budget)
                assert ac.case.scale == "normal"
                want = (alpha * refs[name].double() + beta * torch.from_numpy(old).cuda().double()).to(got.dtype)
            bad = ref_.differing_entries(got, want)
        else:
            idx = _sample_index(ac.case, expr, tuple(got.shape))
            tidx = torch.from_numpy(idx).cuda()
            if sums is not None:
                ms = sums[name].reshape(-1)[idx]
            else:
                ms = np.ldexp(refs[name].reshape(-1)[tidx].double().cpu().numpy(), -t).astype(np.int64)
            want = acc_general_reference(ac, ms, t, old.reshape(-1)[idx])
            bad = ref_.differing_entries(got.reshape(-1)[tidx].cpu().numpy(), want)
            st.cov["checked:sampled" if ac.case.E > ACC_WHOLE_E else "checked:whole"] += 1
        if bad:
            st.fail(f"{label}: output {name}: {bad} entries differ from fl(alpha E + fl(beta old))  REPRO {ac.repro()}")
        else:
            st.exact_equal += 1


def _groups(cases: Sequence[AccCase]) -> List[List[AccCase]]:
    out: List[List[AccCase]] = []
    for ac in cases:
        if out and out[-1][0].case == ac.case:
            out[-1].append(ac)
        else:
            out.append([ac])
    return out


def _acc_exact_group(torch, st: Stats, group: Sequence[AccCase]) -> None:
    group = [acc_resolve(torch, ac) for ac in group]
    case = group[0].case
    dev, refs, sums, t, sig = _acc_data(torch, case, st)
    dt = group[0].out_dtype()
    olds_host = {sh: acc_old(case, sig, t, sh, dt) for sh in sorted({ac.old_shift for ac in group})}
    expr, _ = case.stages()[0]
    plain_ok: Dict[str, bool] = {}
    for ac in group:
        label = _acc_label("exact", ac)
        olds = {name: torch.from_numpy(olds_host[ac.old_shift][k][1]).cuda() for k, name in enumerate(expr.output_names)}
        outs = acc_run(torch, st, ac, dev, olds, label, plain_ok)
        if outs is None:
            continue
        st.cov.update(acc_buckets(ac))
        acc_check_exact(torch, st, ac, label, outs, refs, sums, t, olds_host[ac.old_shift])


def run_accumulate_exact(seed: int, cases: Optional[Sequence[AccCase]] = None) -> Stats:
    """The exact part of the accumulating pass: :func:`acc_cases`, every output bit fixed by the contract."""
    import torch

    st = Stats(f"dg accumulate exact seed={seed}")
    st.cov["refused:unpredicted"] += 0
    for group in _groups(acc_cases(seed) if cases is None else cases):
        _acc_exact_group(torch, st, group)
    return st


# ---- signed data

def acc_bounded_cases(seed: int) -> List[AccCase]:
    """The accepted cases of :func:`acc_cases` in the normal range, E at most 1100 (named sizes included), every other
    pair of each case."""
    keep = [ac for ac in acc_cases(seed) if ac.case.scale == "normal" and ac.case.E <= 1100
            and ac.case.eclass != "second-tile" and predicted_route(ac) is not None]
    return keep[::2]


def run_accumulate_bounded(seed: int, cases: Optional[Sequence[AccCase]] = None) -> Stats:
    """Signed uniform operands and normal old outputs: within ``gamma(K + 2, u) (|alpha| absref + |beta| |old|)`` of the
    long-double value, K the family's bound terms (the bound tests/test_gpu_accumulate_epilogue.py derives); every float64
    result bitwise the "axpby" route of the same case; for power-of-two pairs bitwise torch's ``alpha plain + beta old``."""
    import torch

    st = Stats(f"dg accumulate bounded seed={seed}")
    st.cov["refused:unpredicted"] += 0
    for group in _groups(acc_bounded_cases(seed) if cases is None else cases):
        group = [acc_resolve(torch, ac) for ac in group]
        case = group[0].case
        expr, keys = case.stages()[0]
        nrng = np.random.default_rng(case.seed)
        host = {k: (nrng.random(_shape(expr, nm, case.E)) * 2 - 1).astype(expr.arg_to_dtype[nm]) for nm, k in sorted(keys.items())}
        dev = {k: torch.from_numpy(v).cuda() for k, v in host.items()}
        dt = group[0].out_dtype()
        shape = tuple(case.E if isinstance(d, f.SizeParam) else int(d) for d in expr.shape)
        old_host = {name: nrng.standard_normal(shape).astype(dt) for name in expr.output_names}
        olds = {name: torch.from_numpy(v).cuda() for name, v in old_host.items()}
        nb = ref_.bound_terms(expr.get_subscripts(), _extent(expr, case.E), 3)
        bounds = {name: ref_.bounded_reference(expr.get_subscripts(), [host[keys[a.name]] for a in row])
                  for name, row in zip(expr.output_names, expr.args)}
        u = ref_.U32 if case.dtype == "float32" else ref_.U64
        plain_ok: Dict[str, bool] = {}
        plains: Dict[str, Any] = {}
        for ac in group:
            label = _acc_label("bounded", ac)
            outs = acc_run(torch, st, ac, dev, olds, label, plain_ok)
            if outs is None:
                continue
            bk = acc_buckets(ac)
            st.cov.update(bk)
            alpha, beta = ac.factors()
            for name in expr.output_names:
                r, ar = bounds[name]
                o = old_host[name].astype(np.longdouble)
                want = np.longdouble(alpha) * r + np.longdouble(beta) * o
                absw = abs(np.longdouble(alpha)) * ar + abs(np.longdouble(beta)) * np.abs(o)
                ratio = ref_.bound_ratio(outs[name].cpu().numpy(), want, absw, nb + 2, u)
                for b_ in bk:
                    st.worst[b_] = max(st.worst.get(b_, 0.0), ratio)
                if ratio > 1:
                    st.fail(f"{label}: output {name}: |got - ref| = {ratio:.3g} x the bound  REPRO {ac.repro()}")
            route = predicted_route(ac)
            if case.dtype == "float64" and route != "axpby":
                other = AccCase(case, ac.alpha, ac.beta, "axpby", ac.transform, ac.old_shift)
                fb = acc_run(torch, st, other, dev, olds, label + " (axpby)", plain_ok)
                if fb is not None:
                    st.exact_runs += 1
                    bad = sum(int((outs[n].view(torch.int64) != fb[n].view(torch.int64)).sum()) for n in expr.output_names)
                    if bad:
                        st.fail(f"{label}: {bad} entries differ bitwise from the \"axpby\" route  REPRO {ac.repro()}")
                    else:
                        st.exact_equal += 1
                        st.cov["equal:axpby-route"] += 1
            if ac.pow2() and _plain_accepted(torch, case, dev, ac.transform, plain_ok):
                if ac.transform not in plains:
                    _, pod = _out_buffers(torch, case)
                    launch(torch, case, dev, {"prepared": True} if ac.transform == "prepared" else ac.transform, pod)
                    plains[ac.transform] = pod[0]
                st.exact_runs += 1
                bad = 0
                for n in expr.output_names:
                    two_pass = alpha * plains[ac.transform][n] + beta * olds[n] if beta != 0 else alpha * plains[ac.transform][n]
                    bad += ref_.differing_entries(outs[n], two_pass)
                if bad:
                    st.fail(f"{label}: {bad} entries differ from torch's alpha plain + beta old  REPRO {ac.repro()}")
                else:
                    st.exact_equal += 1
                    st.cov["equal:torch-two-pass"] += 1
    return st


# ---- non-finite values

ACC_PLANT_ROLES = ("field", "geometry", "operator", "old")
ACC_PLANT_VALUES = (math.nan, math.inf, -math.inf)


def acc_plants(seed: int) -> List[Tuple[AccCase, str, float]]:
    """``(case, role, value)``: every role x value with beta = 0 and with beta != 0, and with alpha = 0, on the three
    accumulating kernels (the sizes behind a tile, below one and of several tiles) and on the "axpby" route."""
    rng = random.Random(seed + 43)
    S = lambda: rng.randrange(1 << 30)   # noqa: E731
    o1, o2, o3, o4 = TET_ORDERS
    bases = [(_c("fm:fe:ifj", o4, 4, "rij", "float64", 163, S()), "kernel"), (_c("grad", o3, 1, "rij", "float64", 99, S()), "epilogue"),
             (_c("div", o4, 1, "rji", "float64", 163, S()), "epilogue"), (_c("fm", o2, 5, "rij", "float64", 7, S()), "kernel"),
             (_c("grad", o1, 1, "rji", "float64", 35, S()), "epilogue"), (_c("div", o2, 1, "rij", "float64", 7, S()), "epilogue"),
             (_c("grad", o4, 1, "rij", "float64", 163, S()), "axpby"), (_c("fm", o3, 2, "rij", "float32", 65, S()), "axpby"),
             (_c("divcomp", o3, 1, "rij", "float64", 33, S()), None)]
    reads, blind = ((1.0, 1.0), (0.0, 1.0), (2.0, -0.5), (0.3, -1.7)), ((0.5, 0.0), (0.0, 0.0))
    out = []
    k = 0
    for case, route in bases:
        for role in ACC_PLANT_ROLES:
            for value in ACC_PLANT_VALUES:
                for alpha, beta in (reads[k % 4], blind[k % 2]):
                    out.append((AccCase(case, alpha, beta, route), role, value))
                k += 1
    return out


def acc_plant_buckets(ac: AccCase, role: str, value: float) -> List[str]:
    return [f"planted:{role}:{value}:" + ("beta=0" if ac.beta == 0 else "beta!=0"), f"planted-route:{predicted_route(ac)}",
            f"planted:{role}:alpha=0" if ac.alpha == 0 else f"planted:{role}:alpha!=0"]


ACC_PLANT_MINIMUMS = {**{f"planted:{r}:{v}:{b}": 2 for r in ACC_PLANT_ROLES for v in ACC_PLANT_VALUES for b in ("beta=0", "beta!=0")},
                      **{f"planted:{r}:alpha=0": 4 for r in ACC_PLANT_ROLES},
                      "planted-route:kernel": 40, "planted-route:epilogue": 80, "planted-route:axpby": 60}


def _plant_site(case: DGCase, role: str, rng: random.Random):
    """``(key, index)`` of a planted input entry of the first row; for "old" the output name and an index."""
    expr, keys = case.stages()[0]
    row = expr.args[rng.randrange(len(expr.args))]
    elems = sorted({0, min(case.E - 1, 15), case.E // 2, case.E - 1})
    if role == "old":
        shape = [case.E if isinstance(d, f.SizeParam) else int(d) for d in expr.shape]
        idx = [rng.randrange(s) for s in shape]
        idx[_e_axis(expr, None)] = rng.choice(elems)
        return expr.output_names[expr.args.index(row)], tuple(idx)
    for a in row:
        ax = _e_axis(expr, a.name)
        r = "operator" if ax is None else ("field" if a is row[-1] else "geometry")
        if r == role:
            idx = [rng.randrange(s) for s in _shape(expr, a.name, case.E)]
            if ax is not None:
                idx[ax] = rng.choice(elems)
            return keys[a.name], tuple(idx)
    return None


def acc_check_plant(ac: AccCase, role: str, value: float, got, clean, dep) -> int:
    """Violations of the rule of a planted value: exactly *dep* is non-finite -- NaN for a planted NaN, and NaN for any
    value planted in an input when alpha is 0 (``0 * Inf`` is NaN: all three routes multiply) -- and every other entry
    is bitwise the clean accumulating launch."""
    return ref_.nonfinite_violations(got, clean, dep, math.nan if ac.alpha == 0 and role != "old" else value)


def run_accumulate_nonfinite(seed: int, plants: Optional[Sequence[Tuple[AccCase, str, float]]] = None) -> Stats:
    """One NaN / +Inf / -Inf in a field, a geometry factor, an operator entry or an old output of an accumulating launch.
    beta != 0: exactly the dependency set of the einsum is non-finite (a plant in an old output: that single entry), the
    rest bitwise the clean accumulating launch.  beta = 0: the old outputs are all NaN / +-Inf poison and do not show.
    alpha = 0: a non-finite E_k still gives NaN, on every route (the contract)."""
    import torch

    st = Stats(f"dg accumulate nonfinite seed={seed}")
    st.cov["refused:unpredicted"] += 0
    rng = random.Random(seed + 47)
    todo = acc_plants(seed) if plants is None else plants
    data: Dict[DGCase, Any] = {}
    for ac, role, value in todo:
        case = ac.case
        expr, keys = case.stages()[0]
        if case not in data:
            data.clear()
            dev, _, _, t, sig = _acc_data(torch, case, st)
            olds = {name: torch.from_numpy(x).cuda() for name, (_, x) in zip(expr.output_names, acc_old(case, sig, t, 0, ac.out_dtype()))}
            data[case] = (dev, olds, {})
        dev, olds, plain_ok = data[case]
        label = _acc_label(f"nonfinite {value} in {role}", ac)
        clean = acc_run(torch, st, ac, dev, olds, label + " (clean)", plain_ok)
        site = _plant_site(case, role, rng)
        if clean is None or site is None:
            continue
        key, idx = site
        start = {n: o.clone() for n, o in olds.items()}
        if ac.beta == 0:      # not read: poison everywhere
            for o in start.values():
                o.fill_(math.nan)
                o.view(-1)[1::2] = math.inf
                o.view(-1)[2::4] = -math.inf
        if role == "old":
            start[key][idx] = value
            deps = {n: torch.zeros_like(o, dtype=torch.bool) for n, o in olds.items()}
            if ac.beta != 0:
                deps[key][idx] = True
            got = acc_run(torch, st, ac, dev, start, label, plain_ok)
        else:
            keep = dev[key][idx].clone()
            dev[key][idx] = value
            deps = _dependency(torch, case, key, idx)[0]
            got = acc_run(torch, st, ac, dev, start, label, plain_ok)
            dev[key][idx] = keep
        if got is None:
            continue
        st.cov.update(acc_plant_buckets(ac, role, value))
        st.exact_runs += 1
        bad = sum(acc_check_plant(ac, role, value, got[n], clean[n], deps[n]) for n in expr.output_names)
        if bad:
            st.fail(f"{label}: {bad} entries break the dependency rule at {key}{list(idx)}  REPRO {ac.repro()}")
        else:
            st.exact_equal += 1
    return st


# ---- placement

ACC_PLACE_E = 163     # 2 x 80 + 3: full tiles and a remainder at every order


def acc_placement_runs(seed: int, part: str) -> List[List[PlacedRun]]:
    """Accumulating runs of the placement pass, one list per (case, factors), "aligned" in front.  The full set of
    PLACEMENTS under "kernel" (face-mass) and "epilogue" (grad, div) at every order p = 1..4, E = 163 (full tiles and a
    remainder) and, at two orders each, E = 17 (below one tile); "aligned" and "all" under "axpby".  *part* "exact":
    power-of-two pairs with beta != 0, bitwise the reference; "signed": a general pair, bitwise the aligned launch."""
    rng = random.Random(seed + 53)
    S = lambda: rng.randrange(1 << 30)   # noqa: E731
    data = "signed" if part == "signed" else "exact"
    pow2 = [p for p in ACC_PAIRS if is_pow2(p[0]) and is_pow2(p[1]) and p[1] != 0 and p[0] != 0] + [(0.5, 0.0)]
    out = []
    k = 0

    def add(case, route, transform, full):
        nonlocal k
        alpha, beta = ACC_GENERAL[k % 2] if part == "signed" else pow2[k % len(pow2)]
        k += 1
        acc = (alpha, beta, route, k % 2 * 3)
        out.append([PlacedRun(case, data, transform, name, shifts, (), acc) for name, shifts in placements_of(case, full)])

    for pi, order in enumerate(TET_ORDERS):
        for E in (ACC_PLACE_E, 17) if pi % 2 else (ACC_PLACE_E,):
            add(_c(ACC_FM_KINDS[(3 * pi + E) % 8], order, (3, 2, 4, 5)[pi], "rij", "float64", E, S()), "kernel", "auto", True)
            add(_c("grad", order, 1, ("rij", "rji")[pi % 2], "float64", E, S()), "epilogue", "mfma" if pi == 2 else "auto", True)
            add(_c("div", order, 1, ("rji", "rij")[pi % 2], "float64", E, S()), "epilogue", "auto", True)
    o1, o2, o3, o4, o5, t7, t13 = ORDERS3
    for case, t in ((_c("grad", o4, 1, "rij", "float64", 65, S()), "auto"), (_c("fm", o3, 9, "rij", "float64", 65, S()), "auto"),
                    (_c("fm", o2, 2, "rij", "float32", 64, S()), "auto"), (_c("divcomp", o3, 1, "rij", "float64", 17, S()), "tiled"),
                    (_c("mass", o5, 2, "ij", "float64", 65, S()), "auto"), (_c("grad", o3, 1, "rij", "mixed", 64, S()), "auto"),
                    (_c("div", o2, 1, "rij", "float32", 1003, S()), "auto")):
        add(case, "axpby", t, False)
    return out


def acc_placement_buckets(run: PlacedRun) -> List[str]:
    route = run.acc[2]
    ac = _acc_of(run)
    b = ["place:" + run.placement, f"accplace-route:{predicted_route(ac)}", f"dtype:{run.case.dtype}"]
    fam = ac.family()
    if route in ("kernel", "epilogue") and run.placement in ("only:field", "only:output") and run.case.E >= ACC_PLACE_E:
        b.append(f"accplace:{fam}:p{TET_ORDERS.index((run.case.Np, run.case.Nfp)) + 1}:{run.placement}")
    return b


def _acc_of(run: PlacedRun) -> AccCase:
    alpha, beta, route, old_shift = run.acc
    return AccCase(run.case, float(alpha), float(beta), route, run.transform, int(old_shift))


def acc_placement_coverage(seed: int, part: str) -> Counter:
    cnt: Counter = Counter()
    for runs in acc_placement_runs(seed, part):
        for run in runs:
            cnt.update(acc_placement_buckets(run))
    return cnt


#: minimum runs per bucket of the accumulating placement runs, either part: ``only:field`` (the output aligned) and
#: ``only:output`` (the fields aligned) for face-mass, grad and div at every order, by name
ACC_PLACEMENT_MINIMUMS = {
    **{f"accplace:{fam}:p{p}:{pl}": 1 for fam in ("fm", "grad", "div") for p in (1, 2, 3, 4) for pl in ("only:field", "only:output")},
    **{"place:" + p: 18 for p in PLACEMENTS if "last" not in p}, "place:only:last-field": 6, "place:only:last-output": 6,
    "place:aligned": 25, "place:all": 25, "accplace-route:kernel": 50, "accplace-route:epilogue": 80, "accplace-route:axpby": 14,
}


def _acc_placed_case(torch, st: Stats, runs: Sequence[PlacedRun]) -> None:
    """All runs of one accumulating case: inputs embedded between NaN bands once per shift, outputs between sentinel
    bands holding the old values; exact data bitwise the reference, signed float64 data bitwise the aligned launch."""
    ac = _acc_of(runs[0])
    case, data = ac.case, runs[0].data
    expr, keys = case.stages()[0]
    dt = ac.out_dtype()
    refs = None
    if data == "exact":
        assert ac.pow2() and case.E <= HOST_REF_MAX_E
        dev, _, sums, t, sig = _acc_data(torch, case, st)
        old_host = acc_old(case, sig, t, ac.old_shift, dt)
        alpha, beta = ac.factors()
        refs = [{name: torch.from_numpy(combine_pow2(sums[name], t, alpha, beta, old_host[k][0], t + ac.old_shift, dt)).cuda()
                 for k, name in enumerate(expr.output_names)}]
        olds = {name: torch.from_numpy(old_host[k][1]).cuda() for k, name in enumerate(expr.output_names)}
    else:
        nrng = np.random.default_rng(case.seed)
        dev = {k: torch.from_numpy((nrng.random(_shape(expr, nm, case.E)) * 2 - 1).astype(expr.arg_to_dtype[nm])).cuda()
               for nm, k in sorted(keys.items())}
        shape = tuple(case.E if isinstance(d, f.SizeParam) else int(d) for d in expr.shape)
        olds = {name: torch.from_numpy(nrng.standard_normal(shape).astype(dt)).cuda() for name in expr.output_names}
    ins_slots, out_slots = slots_of(case)
    cache: Dict[Tuple[str, int], Tuple[Embedded, Any]] = {}
    aligned = None
    want_route = predicted_route(ac)
    for run in runs:
        shifts = dict(run.shifts)
        ins = {}
        for key, _, idt, shape in ins_slots:
            at = (key, shifts.get(key, 0))
            if at not in cache:
                emb = embed(torch, shape, getattr(torch, idt.name), at[1], "in", dev[key])
                cache[at] = (emb, emb.snapshot())
            ins[key] = cache[at]
        outs: Dict[str, Embedded] = {}
        for slot, _, name, odt, shape in out_slots:
            outs[name] = embed(torch, shape, getattr(torch, odt.name), shifts.get(slot, 0), "out")
            outs[name].view.copy_(olds[name])
        label = f"placement {run.placement} {data} " + _acc_label("", ac)
        try:
            route = acc_launch(ac, {k: e.view for k, (e, _) in ins.items()}, {n: e.view for n, e in outs.items()})
        except (NotImplementedError, f.InvalidParameterError) as exc:
            st.cov["refused:unpredicted"] += 1
            st.fail(f"{label}: refused ({exc})  REPRO {run.repro()}")
            continue
        if route != want_route:
            st.fail(f"{label}: took the route {route!r}, the host predicts {want_route!r}  REPRO {run.repro()}")
            continue
        st.cov.update(acc_placement_buckets(run))
        check_inputs(st, label, run, ins)
        base = aligned if (data == "signed" and case.dtype == "float64" and run.placement != "aligned") else None
        check_outputs(st, label, run, [outs], refs, base)
        if run.placement == "aligned":
            aligned = [{n: _int_copy(torch, e) for n, e in outs.items()}]


def run_accumulate_placement(seed: int, part: str = "all") -> Stats:
    """The accumulating runs of the placement pass: *part* "exact", "signed" or "all"."""
    import torch

    st = Stats(f"dg accumulate placement {part} seed={seed}")
    st.cov["leak:nan-entries"] += 0
    st.cov["refused:unpredicted"] += 0
    for p in ("exact", "signed") if part == "all" else (part,):
        for runs in acc_placement_runs(seed, p):
            _acc_placed_case(torch, st, runs)
    return st


def run_accumulate(seed: int) -> List[Stats]:
    return [run_accumulate_exact(seed), run_accumulate_bounded(seed), run_accumulate_nonfinite(seed),
            run_accumulate_placement(seed)]


def repro_accumulate(text: str) -> Stats:
    """Replay one ``REPRO`` line of the accumulating pass on exact and on signed data (a placement line: its aligned
    launch first)."""
    import torch

    d = json.loads(text)
    if "placement" in d:
        run = PlacedRun.from_repro(text)
        st = Stats("repro")
        st.cov["leak:nan-entries"] += 0
        first = [PlacedRun(run.case, run.data, run.transform, "aligned", (), run.knobs, run.acc)] if run.placement != "aligned" else []
        _acc_placed_case(torch, st, first + [run])
        return st
    ac = AccCase.from_repro(text)
    st = run_accumulate_exact(0, [ac])
    if ac.case.scale == "normal" and predicted_route(ac) is not None:
        st2 = run_accumulate_bounded(0, [ac])
        st.failures += st2.failures
        st.exact_runs += st2.exact_runs
        st.exact_equal += st2.exact_equal
        st.cov.update(st2.cov)
    return st


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--placement":
        st = run_placement(int(sys.argv[2]) if len(sys.argv) > 2 else 0)
        print(st.report())
        sys.exit(1 if st.failures else 0)
    if len(sys.argv) > 1 and sys.argv[1] == "--accumulate":
        results = run_accumulate(int(sys.argv[2]) if len(sys.argv) > 2 else 0)
        for s in results:
            print(s.report())
        sys.exit(1 if sum(s.failures for s in results) else 0)
    if len(sys.argv) > 2 and sys.argv[1] == "--repro" and "accumulate" in json.loads(sys.argv[2]):
        st = repro_accumulate(sys.argv[2])
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
