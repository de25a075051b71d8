"""Seeded sweep of random explicit-mode einsums outside the DG families through every transform that accepts them
("generic", "contraction", "reduction", "auto"), against the references of oracle/einsum_ref.py (test
infrastructure, like tests/).

    python tools/fuzz_einsum.py [n_cases] [seed]

Three passes:

``run_exact``        exact data (``m * 2**s``): every result bitwise equal to the int64 einsum of the mantissas.
``run_bounded``      signed uniform data: ``|got - ref| <= gamma(n, u) * absref`` entrywise (longdouble reference).
``run_descriptors``  ``_hip.einsum_generic`` / ``einsum_contract`` / ``einsum_reduce`` on torch views (permuted, step
                     slices, one-element offsets, ``expand``, float32 views), exact data.

Every output lands in a NaN-filled buffer between sentinel guard bands.  Each failure prints one line with a
reproducer (``python tools/fuzz_einsum.py --repro '<case>'``).  Every run records the path it took (``launch_kind``,
``einsum_reduce_plan``), so :func:`coverage` can assert a minimum number of cases per bucket (:data:`MINIMUMS`).
"""

from __future__ import annotations

import json
import random
import sys
from collections import Counter
from dataclasses import asdict, dataclass
from pathlib import Path
from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

import feinsum_amd as f  # noqa: E402
from feinsum_amd import _hip  # noqa: E402
from feinsum_amd.contraction import _desc, _extents, _split, intermediate_shapes, plan_steps  # noqa: E402
from feinsum_amd.contraction_schedule import get_trivial_contraction_schedule  # noqa: E402
from feinsum_amd.measure import launch_kind, result_dtype  # noqa: E402
from feinsum_amd.reduction import (REDUCE_MAX_OUT, REDUCE_MIN_SUM, REDUCE_STREAM_FACTOR,  # noqa: E402
                                   plan_reduction)
from oracle import einsum_ref as ref_  # noqa: E402

TRANSFORMS = ("generic", "contraction", "reduction", "auto")
#: extents at the kernels' edges (vector widths, waves, 64 x 64 tiles)
EDGES = (1, 2, 3, 4, 5, 7, 8, 15, 16, 17, 31, 33, 63, 64, 65, 127, 129)
BIG_E = (1000, 4099, 100_003, 300_007, 1_000_003)
LETTERS = "ijklm"   # with "e", the element index (size parameter "E")
GUARD = 1024
SENTINEL = -7.25

#: minimum runs per coverage bucket of the fixed-seed sweeps (tests/test_gpu_einsum_fuzz.py, test_einsum_fuzz_cpu.py)
MINIMUMS = {
    "path:generic": 40, "path:contraction": 20, "path:reduction-mfma": 4,
    "path:reduction-valu-Esummed": 20, "path:reduction-valu-Ekept": 10,
    "dtype:float32": 20, "dtype:mixed": 20, "dtype:float64": 20,
    "ops:1": 10, "ops:2": 20, "ops:3+": 20,
    "E:summed": 20, "E:kept": 20,
}
DESC_MINIMUMS = {
    "layout:contiguous": 10, "layout:permuted": 10, "layout:strided": 10, "layout:offset": 10, "layout:stride0": 10,
    "entry:generic": 20, "entry:contract": 10, "entry:reduce-valu": 10, "entry:reduce-mfma": 2,
    "dtype:float32": 5, "dtype:mixed": 5, "dtype:float64": 5,
}


@dataclass(frozen=True)
class Case:
    """One einsum: subscripts over operands ``shapes`` (``"E"`` the element axis), ``dtypes``, the element count, and
    whether 3+ operand einsums also run with the explicit left-to-right schedule."""

    subs: str
    shapes: Tuple[Tuple[Any, ...], ...]
    dtypes: Tuple[str, ...]
    E: int
    schedule: bool = False
    seed: int = 0
    tag: str = "random"

    def expr(self):
        return f.einsum(self.subs, *[f.array(f"A{k}", s, dt) for k, (s, dt) in enumerate(zip(self.shapes, self.dtypes))])

    def concrete_shapes(self) -> List[Tuple[int, ...]]:
        return [tuple(self.E if d == "E" else int(d) for d in s) for s in self.shapes]

    def extent(self) -> Dict[str, int]:
        ins, _ = self.subs.split("->")
        ext: Dict[str, int] = {}
        for idxs, shape in zip(ins.split(","), self.concrete_shapes()):
            for c, n in zip(idxs, shape):
                ext[c] = n
        return ext

    def repro(self) -> str:
        return json.dumps({**asdict(self), "shapes": [list(s) for s in self.shapes]}, separators=(",", ":"))

    @staticmethod
    def from_repro(text: str) -> "Case":
        d = json.loads(text)
        return Case(**{**d, "shapes": tuple(tuple(s) for s in d["shapes"]), "dtypes": tuple(d["dtypes"])})


def _points(subs: str, ext: Dict[str, int]) -> Tuple[int, int]:
    ins, out = subs.split("->")
    n_out = int(np.prod([ext[c] for c in out], dtype=np.int64)) if out else 1
    return n_out, ref_.summed_points(subs, ext)


def _dtype_mix(rng: random.Random, n_ops: int) -> Tuple[str, ...]:
    mode = rng.choice(["float64", "float32", "mixed"] if n_ops > 1 else ["float64", "float32"])
    if mode != "mixed":
        return (mode,) * n_ops
    dts = [rng.choice(["float32", "float64"]) for _ in range(n_ops)]
    a, b = rng.sample(range(n_ops), 2)   # at least one of each
    dts[a], dts[b] = "float32", "float64"
    return tuple(dts)


# templates: the shapes the new kernels were written for, with random extents
TEMPLATES = ("ei,ei->", "ej,ej->j", "ei,ej->ij", "e,ei,ei->", "e,ij,ei,ej->", "xei,xei->x", "ei->i", "ij,ej->ei",
             "eij,ej->ei", "bei,bej->bij", "ik,kj->ij", "ei,ej,e->", "eii->e", "ei,ei->e")


def _random_subs(rng: random.Random) -> str:
    if rng.random() < 0.3:
        return rng.choice(TEMPLATES)
    n_ops = rng.choice([1, 2, 2, 3, 3, 4])
    pool = ["e"] + rng.sample(LETTERS, rng.randint(1, 5))
    ops = []
    for _ in range(n_ops):
        k = rng.choice([0, 1, 1, 2, 2, 2, 3, 3]) if n_ops > 1 else rng.choice([1, 2, 3])
        axes = [rng.choice(pool) for _ in range(k)]
        if k >= 2 and rng.random() < 0.15:   # a repeated (diagonal) index
            j = rng.choice([c for c in axes if c != "e"] or [pool[1]])
            axes[rng.randrange(k)] = j
            axes[rng.randrange(k)] = j
        while axes.count("e") > 1:           # (never an E x E operand)
            axes.remove("e")
        ops.append("".join(axes))
    if not any("e" in o for o in ops):
        ops[rng.randrange(n_ops)] += "e"
    used = list(dict.fromkeys("".join(ops)))
    out = [c for c in rng.sample(used, len(used)) if rng.random() < 0.45]
    keep_e = rng.random() < 0.5
    out = [c for c in out if c != "e"] + (["e"] if keep_e else [])
    rng.shuffle(out)
    return ",".join(ops) + "->" + "".join(out)


def _fit(rng: random.Random, subs: str, ext: Dict[str, int], max_points: int, max_sum: int, max_elems: int) -> None:
    """Shrink extents until the case is cheap enough for the CPU reference: out entries x summed points, summed
    points per entry and operand sizes under their caps."""
    ins = subs.split("->")[0].split(",")
    for _ in range(64):
        n_out, n_sum = _points(subs, ext)
        biggest = max((int(np.prod([ext[c] for c in o], dtype=np.int64)) for o in ins), default=1)
        if n_out * max(n_sum, 1) <= max_points and n_sum <= max_sum and biggest <= max_elems:
            return
        big = max(ext, key=lambda c: ext[c])
        ext[big] = rng.choice([x for x in EDGES if x < ext[big]] or [1])
    raise AssertionError(f"could not fit {subs} {ext}")


def gen_cases(n: int, seed: int, *, max_points: int = 4_000_000, max_sum: int = 1 << 40,
              max_elems: int = 16_000_000, edges: bool = True) -> List[Case]:
    """*n* random cases (deterministic in *seed*, host only), and with *edges* the cases at the ``"auto"`` thresholds
    (:func:`threshold_cases`, up to 3 x 10^8 points).  *max_points* caps out entries x summed points of the random
    cases, *max_sum* the summed points per entry."""
    rng = random.Random(seed)
    cases: List[Case] = []
    while len(cases) < n:
        subs = _random_subs(rng)
        ins, out = subs.split("->")
        ops = ins.split(",")
        letters = dict.fromkeys(ins)
        ext = {c: rng.choice(EDGES) for c in letters if c != "e"}
        r = rng.random()
        ext["e"] = 0 if r < 0.03 else rng.choice(BIG_E) if r < 0.25 else rng.choice(EDGES)
        if rng.random() < 0.02 and len(ext) > 1:
            ext[rng.choice([c for c in ext if c != "e"])] = 0
        dts = _dtype_mix(rng, len(ops))
        while True:   # operands, and the intermediates of either schedule, under max_elems
            _fit(rng, subs, ext, max_points, max_sum, max_elems)
            shapes = tuple(tuple("E" if c == "e" else ext[c] for c in o) for o in ops)
            case = Case(subs, shapes, dts, ext["e"], schedule=len(ops) >= 3 and rng.random() < 0.6,
                        seed=rng.randrange(1 << 30))
            big = _largest_intermediate(case)
            if big <= max_elems:
                break
            c = max((c for c in ext if c != "e" or ext["e"] > 1), key=lambda c: ext[c])
            ext[c] = max(1, ext[c] // 2)
        cases.append(case)
    return cases + (threshold_cases(seed) if edges else [])


def _largest_intermediate(case: Case) -> int:
    if len(case.shapes) < 3:
        return 0
    expr = case.expr()
    ext = case.extent()
    sizes = [int(np.prod(s, dtype=np.int64)) for sched in (None, get_trivial_contraction_schedule(expr))
             for s in intermediate_shapes(plan_steps(expr, sched), ext).values()]
    return max(sizes, default=0)


def threshold_cases(seed: int, max_points: int = 300_000_000, max_sum: int = 1 << 62) -> List[Case]:
    """Cases on both sides of the ``"auto"`` rules of reduction.py: summed points 65535 / 65536 / 65537
    (REDUCE_MIN_SUM), output entries 4096 / 4097 (REDUCE_MAX_OUT), both sides of REDUCE_STREAM_FACTOR, the largest
    grids of the matrix-core path, and E up to 10^6 for the slices.  (REDUCE_MAX_TILES does not bind: a two-operand
    launch of at most REDUCE_MAX_OUT entries has at most 8 tiles of 64 x 64 -- see test_einsum_fuzz_cpu.)"""
    rng = random.Random(seed + 1)
    m = REDUCE_MIN_SUM
    sf = REDUCE_STREAM_FACTOR
    spec = [("e,e->", [("E",), ("E",)], E) for E in (m - 1, m, m + 1)]
    spec += [("ei,ei->", [("E", 4), ("E", 4)], E) for E in (m // 4 - 1, m // 4, m // 4 + 1)]
    spec += [("ej,ej->j", [("E", 7), ("E", 7)], E) for E in (m - 1, m + 1)]
    spec += [("e,j->j", [("E",), (J,)], m + 1) for J in (REDUCE_MAX_OUT, REDUCE_MAX_OUT + 1)]
    spec += [("e,jk->jk", [("E",), (64, 64)], m), ("e,jk->jk", [("E",), (17, 241)], m)]   # 4096, 4097 entries
    spec += [("ei,ej,e->", [("E", sf), ("E", sf + 1), ("E",)], 16_001),                    # streams: 4 x largest
             ("ei,ej,e->", [("E", sf + 1), ("E", sf + 1), ("E",)], 16_001)]                # 5 x: the schedule
    spec += [("ei,ej->ij", [("E", 64), ("E", 64)], m + 1), ("ei,ej->ij", [("E", 65), ("E", 63)], m - 1),
             ("bei,bej->bij", [(8, "E", 16), (8, "E", 32)], m + 3), ("ie,je->ij", [(16, "E"), (33, "E")], 100_003)]
    # the split-K path at K below the "auto" threshold (explicit "reduction"), ragged tiles and k slices
    spec += [("ei,ej->ij", [("E", 33), ("E", 17)], 5003), ("ik,kj->ij", [(16, 7001), (7001, 32)], 1),
             ("bei,bej->bij", [(3, "E", 17), (3, "E", 31)], 2049), ("ei,je->ij", [("E", 65), (9, "E")], 4097),
             ("eik,ejk->ij", [("E", 16, 3), ("E", 40, 3)], 3001)]
    spec += [("ei,ei->", [("E", 3), ("E", 3)], 1_000_003), ("ej,ej->j", [("E", 7), ("E", 7)], 300_007),
             ("e,ei,ei->", [("E",), ("E", 2), ("E", 2)], 1_000_003), ("ei->i", [("E", 5)], 999_999)]
    cases = []
    for subs, shapes, E in spec:
        ext = {c: (E if d == "E" else d) for o, s in zip(subs.split("->")[0].split(","), shapes) for c, d in zip(o, s)}
        n_out, n_sum = _points(subs, ext)
        if n_out * max(n_sum, 1) > max_points or n_sum > max_sum:
            continue
        dts = _dtype_mix(rng, len(shapes))
        cases.append(Case(subs, tuple(tuple(s) for s in shapes), dts, E, schedule=len(shapes) >= 3,
                          seed=rng.randrange(1 << 30), tag="threshold"))
    return cases


# --------------------------------------------------------------------------
# coverage (host only)
# --------------------------------------------------------------------------

class _Strided:   # C-contiguous strides of a shape, without an allocation (descriptors for the host-only plan query)
    def __init__(self, shape):
        self._st = tuple(int(np.prod(shape[k + 1:], dtype=np.int64)) for k in range(len(shape)))

    def stride(self):
        return self._st


def runs_of(case: Case) -> List[Tuple[str, Any]]:
    """``(transform, schedule)`` pairs the case runs under: every transform, and for 3+ operands with
    ``case.schedule`` the explicit left-to-right schedule under "contraction" and "reduction" too."""
    runs: List[Tuple[str, Any]] = [(t, None) for t in TRANSFORMS]
    if case.schedule:
        sched = get_trivial_contraction_schedule(case.expr())
        runs += [("contraction", sched), ("reduction", sched)]
    return runs


def paths_of(case: Case, transform: str, schedule: Any) -> Optional[List[str]]:
    """The launches *transform* makes for the case, host only: ``"generic"``, ``"contraction"``,
    ``"reduction-mfma"``, ``"reduction-valu-Esummed"`` / ``"-Ekept"`` (per split launch, E summed or kept in its
    output) or ``"family"``; ``None`` when the transform does not take the case (``NotImplementedError``)."""
    expr = case.expr()
    sizes = {"E": case.E}
    try:
        kind = launch_kind(expr, transform, sizes)
    except NotImplementedError:
        return None
    ext = _extents(expr, sizes)
    if kind in ("generic", "family"):
        return [kind]
    if kind == "contraction":
        return ["contraction" if len(st.inputs) == 2 else "generic" for st in plan_steps(expr, schedule)]
    out = []
    plan = plan_reduction(expr, sizes, schedule)
    for st, how in plan:
        if how != "reduce":
            out.append("contraction" if how == "contract" else "generic")
            continue
        ins, rhs = _split(st.subscripts)
        ts = [_Strided([ext[c] for c in idx]) for idx in ins]
        # (the path depends on the shape alone: an intermediate's dtype does not matter here)
        dts = [np.dtype(case.dtypes[x]) if kind_ == "op" else np.dtype("float64") for kind_, x in st.inputs]
        try:
            path = _hip.einsum_reduce_plan(_desc(st.subscripts, ts, ext, dts))[0]
        except NotImplementedError:
            return None
        out.append("reduction-mfma" if path == "mfma" else
                   "reduction-valu-" + ("Ekept" if "e" in rhs else "Esummed"))
    return out


def buckets_of(case: Case, paths: Sequence[str]) -> List[str]:
    n = len(case.shapes)
    dset = set(case.dtypes)
    out_idx = case.subs.split("->")[1]
    b = [f"path:{p}" for p in dict.fromkeys(paths)]
    b.append("dtype:" + ("mixed" if len(dset) > 1 else case.dtypes[0]))
    b.append("ops:" + (str(n) if n < 3 else "3+"))
    b.append("E:" + ("kept" if "e" in out_idx else "summed"))
    return b


def coverage(cases: Sequence[Case]) -> Counter:
    """Runs per bucket over the cases and every transform that accepts them (host only)."""
    cnt: Counter = Counter()
    for case in cases:
        for transform, sched in runs_of(case):
            paths = paths_of(case, transform, sched)
            if paths is None:
                cnt["not-accepted:" + transform] += 1
                continue
            cnt.update(buckets_of(case, paths))
    return cnt


def missing_buckets(cnt: Counter, minimums: Dict[str, int]) -> Dict[str, Tuple[int, int]]:
    return {k: (cnt.get(k, 0), v) for k, v in minimums.items() if cnt.get(k, 0) < v}


# --------------------------------------------------------------------------
# data
# --------------------------------------------------------------------------

def exact_data(case: Case, extra: int = 0):
    """``(arrays, reference, significand)`` of exact data for the case (*extra* perturbs the seed)."""
    rng = np.random.default_rng(case.seed + 7919 * extra)
    n = len(case.shapes)
    sig = ref_.compute_significand(case.dtypes, ref_.f32_step_possible(case.dtypes, n))
    n_terms = ref_.summed_points(case.subs, case.extent())
    bits = ref_.exact_bits(n, case.dtypes, n_terms, sig, rng)
    assert ref_.bits_fit(bits, n_terms, sig), (bits, n_terms, sig)
    scales = [int(s) for s in rng.integers(-8, 9, size=n)]
    mants, arrays = ref_.exact_operands(case.concrete_shapes(), case.dtypes, bits, scales, rng)
    out_dt = np.result_type(*[np.dtype(d) for d in case.dtypes])
    return arrays, ref_.exact_reference(case.subs, mants, scales, out_dt, sig), sig


def bounded_data(case: Case):
    rng = np.random.default_rng(case.seed)
    return [(rng.random(s) * 2 - 1).astype(np.dtype(dt)) for s, dt in zip(case.concrete_shapes(), case.dtypes)]


def _guarded(torch, shape, dtype):
    n = int(np.prod(shape, dtype=np.int64)) if shape else 1
    buf = torch.full((n + 2 * GUARD,), float("nan"), dtype=dtype, device="cuda")
    buf[:GUARD] = SENTINEL
    buf[GUARD + n:] = SENTINEL
    return buf, buf[GUARD:GUARD + n].view(shape), n


def _guards_intact(buf, n) -> bool:
    return bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[GUARD + n:] == SENTINEL).all())


# --------------------------------------------------------------------------
# the passes (GPU)
# --------------------------------------------------------------------------

class Stats:
    def __init__(self, name: str) -> None:
        self.name = name
        self.cov: Counter = Counter()
        self.worst: Dict[str, float] = {}
        self.exact_runs = self.exact_equal = self.failures = self.without_wide_entry = 0

    def fail(self, line: str) -> None:
        self.failures += 1
        print("FAIL " + line, flush=True)

    def report(self) -> str:
        lines = [f"[{self.name}] failures {self.failures}"]
        if self.exact_runs:
            lines.append(f"[{self.name}] exact-data runs {self.exact_runs}, bitwise equal {self.exact_equal}"
                         f" (float64 cases without an entry needing > 24 bits: {self.without_wide_entry})")
        for k in sorted(self.cov):
            w = f"  worst |got-ref|/bound {self.worst[k]:.3e}" if k in self.worst else ""
            lines.append(f"[{self.name}] {k:32s} {self.cov[k]:6d}{w}")
        return "\n".join(lines)


def _run_case(torch, case: Case, mode: str, st: Stats) -> None:
    expr = case.expr()
    if mode == "exact":
        arrays, ref, sig = exact_data(case)
        for extra in range(1, 4):   # float64 compute: some entry must need more than float32's 24 bits
            if sig != 53 or ref.size == 0 or not ref.any() or ref_.needs_more_than_f32(ref):
                break
            arrays, ref, sig = exact_data(case, extra)
        if sig == 53 and ref.size and ref.any() and not ref_.needs_more_than_f32(ref):
            st.without_wide_entry += 1
    else:
        arrays = bounded_data(case)
        ref, absref = ref_.bounded_reference(case.subs, arrays)
        n_ops = len(arrays)
        n = ref_.bound_terms(case.subs, case.extent(), n_ops, n_ops - 1 if n_ops >= 3 else 0)
        u = ref_.unit_roundoff(case.dtypes, n_ops)
    dev = {f"A{k}": torch.from_numpy(np.array(a, order="C")).cuda() for k, a in enumerate(arrays)}
    out_shape = tuple(case.E if isinstance(d, f.SizeParam) else int(d) for d in expr.shape)
    out_dt = getattr(torch, result_dtype(expr).name)
    for transform, sched in runs_of(case):
        label = f"{mode} {transform}{' +schedule' if sched is not None else ''}: {case.subs} E={case.E} dtypes={case.dtypes}"
        paths = paths_of(case, transform, sched)
        buf, out, n_out = _guarded(torch, out_shape, out_dt)
        try:
            f.evaluate(expr, 0, dev, out_dict={"_fe_out": out}, transform=transform, schedule=sched, wait=True)
        except NotImplementedError:
            st.cov["not-accepted:" + transform] += 1
            if paths is not None:
                st.fail(f"{label}: NotImplementedError, but the host plan accepts it  REPRO {case.repro()}")
            continue
        if paths is None:
            st.fail(f"{label}: ran, but the host plan rejects it  REPRO {case.repro()}")
            continue
        buckets = buckets_of(case, paths)
        st.cov.update(buckets)
        if not _guards_intact(buf, n_out):
            st.fail(f"{label}: wrote outside its output  REPRO {case.repro()}")
            continue
        got = out.cpu().numpy()
        if mode == "exact":
            st.exact_runs += 1
            if ref_.bitwise_equal(got, ref):
                st.exact_equal += 1
            else:
                bad = int((got != ref).sum()) if got.shape == ref.shape else -1
                st.fail(f"{label}: {bad} entries differ from the exact result  REPRO {case.repro()}")
        else:
            ratio = ref_.bound_ratio(got, ref, absref, n, u)
            for b in buckets:
                st.worst[b] = max(st.worst.get(b, 0.0), ratio)
            if ratio > 1:
                st.fail(f"{label}: |got - ref| = {ratio:.3g} x the bound (n={n}, u=2^{int(np.log2(u))})"
                        f"  REPRO {case.repro()}")
        del buf, out


def run_transforms(n: int, seed: int, mode: str = "exact", **gen_kw) -> Stats:
    """The cross-transform sweep: *n* random cases plus the threshold cases, *mode* ``"exact"`` or ``"bounded"``."""
    import torch

    st = Stats(f"{mode} seed={seed}")
    cases = gen_cases(n, seed, **gen_kw)
    for case in cases:
        _run_case(torch, case, mode, st)
    return st


def run_exact(n: int, seed: int) -> Stats:
    return run_transforms(n, seed, "exact")


def run_bounded(n: int, seed: int) -> Stats:
    """Summed points per entry at most 10^4 (where the bound is tight enough to mean something)."""
    return run_transforms(n, seed, "bounded", max_points=1_000_000, max_sum=10_000, max_elems=2_000_000, edges=False)


# --------------------------------------------------------------------------
# descriptor-level pass
# --------------------------------------------------------------------------

LAYOUTS = ("contiguous", "permuted", "strided", "offset", "stride0")


@dataclass(frozen=True)
class DescCase:
    case: Case
    layouts: Tuple[str, ...]


def gen_desc_cases(n: int, seed: int) -> List[DescCase]:
    rng = random.Random(seed)
    out = []
    for case in gen_cases(n, seed, max_points=1_000_000, max_elems=1_000_000, edges=False):
        layouts = []
        for s in case.shapes:
            opts = [lay for lay in LAYOUTS if len(s) >= (2 if lay == "permuted" else 1) or lay in ("contiguous", "offset")]
            layouts.append(rng.choice(opts))
        out.append(DescCase(case, tuple(layouts)))
    # the contraction and the split-K path see every layout too
    for k, lay in enumerate(LAYOUTS):
        for subs, shapes in (("ik,kj->ij", ((70, 40), (40, 90))), ("ei,ej->ij", (("E", 33), ("E", 17)))):
            out.append(DescCase(Case(subs, shapes, _dtype_mix(rng, 2), 70_001, seed=rng.randrange(1 << 30),
                                     tag="desc"), (lay, rng.choice(LAYOUTS))))
    return out


def make_view(torch, arr: np.ndarray, layout: str, rng: np.random.Generator):
    """A device view of *arr*'s shape in *layout* whose values are those of *arr* (stride0: the first entry along one
    axis, expanded)."""
    t = torch.from_numpy(np.array(arr, order="C"))
    shape = tuple(arr.shape)
    if layout == "permuted" and len(shape) >= 2:
        perm = list(rng.permutation(len(shape)))
        while perm == sorted(perm):
            perm = list(rng.permutation(len(shape)))
        inv = list(np.argsort(perm))
        return t.permute(*perm).contiguous().cuda().permute(*inv)
    if layout == "strided" and len(shape) >= 1:
        ax = int(rng.integers(len(shape)))
        step = int(rng.choice([2, 3]))
        big = list(shape)
        big[ax] = shape[ax] * step
        base = torch.full(big, float("nan"), dtype=t.dtype)
        idx = [slice(None)] * len(shape)
        idx[ax] = slice(None, None, step)
        base[tuple(idx)] = t
        return base.cuda()[tuple(idx)]
    if layout == "offset":
        flat = torch.empty(t.numel() + 1, dtype=t.dtype, device="cuda")
        flat[1:] = t.reshape(-1).cuda()
        return flat[1:].view(shape)
    if layout == "stride0" and len(shape) >= 1 and t.numel():
        ax = int(rng.integers(len(shape)))
        one = t.narrow(ax, 0, 1).contiguous().cuda()
        return one.expand(*shape)
    return t.cuda()


def run_descriptors(n: int, seed: int) -> Stats:
    """Random einsums straight through the C ABI entry points with operands as torch views; exact data, reference
    from ``view.cpu().numpy()``."""
    import torch

    st = Stats(f"descriptors seed={seed}")
    for dc in gen_desc_cases(n, seed):
        case = dc.case
        ins, rhs = case.subs.split("->")
        ins_l = ins.split(",")
        ext = case.extent()
        arrays, _, _ = exact_data(case)
        rng = np.random.default_rng(case.seed)
        views = [make_view(torch, a, lay, rng) for a, lay in zip(arrays, dc.layouts)]
        host = [v.cpu().numpy() for v in views]
        n_ops = len(views)
        dts = [np.dtype(d) for d in case.dtypes]
        out_dt = np.result_type(*dts)
        # the views hold exact data (a stride-0 view repeats entries, within the same bit budget): every partial sum
        # of the float64 einsum of their values is exact, so it is the exact result
        wide = [a.astype(np.float64) for a in host]
        ref = np.asarray(np.einsum(case.subs, *wide, optimize=False)).astype(out_dt)
        d = _desc(case.subs, views, ext, dts)
        out_shape = tuple(ext[c] for c in rhs)
        entries = [("generic", _hip.einsum_generic)]
        if n_ops == 2:
            entries.append(("contract", _hip.einsum_contract))
        try:
            rplan = _hip.einsum_reduce_plan(d)
            entries.append(("reduce-" + rplan[0], None))
        except NotImplementedError:
            rplan = None
        label_base = f"descriptors {case.subs} E={case.E} dtypes={case.dtypes} layouts={dc.layouts}"
        for name, fn in entries:
            buf, out, n_out = _guarded(torch, out_shape, getattr(torch, out_dt.name))
            ptrs = [v.data_ptr() for v in views]
            try:
                if fn is None:
                    ws = torch.empty(max(rplan[2], 1), dtype=torch.uint8, device="cuda")
                    _hip.einsum_reduce(d, ptrs, out.data_ptr(), ws.data_ptr(), rplan[2], 0)
                else:
                    fn(d, ptrs, out.data_ptr(), 0)
                torch.cuda.synchronize()
            except NotImplementedError:
                st.cov["not-accepted:" + name] += 1
                continue
            st.cov["entry:" + name] += 1
            st.cov.update("layout:" + lay for lay in dict.fromkeys(dc.layouts))
            st.cov["dtype:" + ("mixed" if len(set(case.dtypes)) > 1 else case.dtypes[0])] += 1
            label = f"{label_base} entry={name}"
            if not _guards_intact(buf, n_out):
                st.fail(f"{label}: wrote outside its output  REPRO {json.dumps(list(dc.layouts))} {case.repro()}")
                continue
            got = out.cpu().numpy()
            st.exact_runs += 1
            if ref_.bitwise_equal(got, ref):
                st.exact_equal += 1
            else:
                bad = int((got != ref).sum()) if got.shape == ref.shape else -1
                st.fail(f"{label}: {bad} entries differ from the exact result  REPRO {json.dumps(list(dc.layouts))}"
                        f" {case.repro()}")
        del views
    return st


def desc_coverage(dcases: Sequence[DescCase]) -> Counter:
    """Host-only counterpart of the descriptor pass's coverage: entry points and layouts per case."""
    cnt: Counter = Counter()
    for dc in dcases:
        case = dc.case
        ext = case.extent()
        ins = case.subs.split("->")[0].split(",")
        ts = [_Strided([ext[c] for c in idx]) for idx in ins]
        d = _desc(case.subs, ts, ext, [np.dtype(x) for x in case.dtypes])
        names = ["generic"] + (["contract"] if len(ins) == 2 else [])
        try:
            names.append("reduce-" + _hip.einsum_reduce_plan(d)[0])
        except NotImplementedError:
            pass
        for nm in names:
            cnt["entry:" + nm] += 1
            cnt.update("layout:" + lay for lay in dict.fromkeys(dc.layouts))
            cnt["dtype:" + ("mixed" if len(set(case.dtypes)) > 1 else case.dtypes[0])] += 1
    return cnt


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--repro":
        import torch

        st = Stats("repro")
        c = Case.from_repro(sys.argv[2])
        for mode in ("exact", "bounded"):
            _run_case(torch, c, mode, st)
        print(st.report())
        sys.exit(1 if st.failures else 0)
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 200
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else 0
    results = [run_exact(n, seed), run_bounded(n, seed), run_descriptors(n // 2, seed)]
    for s in results:
        print(s.report())
    sys.exit(1 if sum(s.failures for s in results) else 0)
