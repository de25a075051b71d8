"""Seeded sweep of how a user's ``BatchedEinsum`` is BOUND to the DG family launches (``family.match_family`` ->
``measure._bind`` -> ``_FamilyLaunch`` / ``_bind_planes`` -> ``operator.bind_operator``): which operand is the geometry
factor, which the operator and which the field; which rows share a launch; which pointer goes into which slot.

    python tools/fuzz_bind.py [n_cases] [seed]
    python tools/fuzz_bind.py --repro '<one line printed by a failure>'

A case (:class:`BindCase`) is drawn along three axes:

spelling    every forward template of ``family._TEMPLATES`` and the triangle shapes, with the operands in every order,
            random letters for every index (the element index too), random array names, and in a share of the cases a
            concrete integer for the element axis instead of a size parameter;
near misses the same einsums with one thing changed (an axis order, a non-square operator, x != r, 1 or 4 dimensions, a
            repeated index): NOT a family launch, still exact under ``None`` / ``"auto"`` / ``"generic"``;
rows        batched einsums whose rows draw the geometry factor, the operator and the field from small pools, in random
            order, with duplicates, up to ``2 * FE_MAX_FIELDS + 3`` rows, the tables that hit every condition of
            ``_bind_planes`` from both sides, and two names bound to the same device tensor or to equal copies.

The data is exact (``m * 2**s``, bits per array from ``oracle.einsum_ref.shared_exact_bits``): every output of every row
must equal the int64 einsum of the mantissas of the row's OWN subscripts and arrays, bitwise (``fuzz_dg.references``).
The tool also predicts the launch shape from the documented rules (:func:`predict_entry_points`) and compares it with
``bind_operator(..., fuse=False).entry_points``, and it predicts which forced transforms the kernels do not take
(:func:`accepted_on_host`): a refusal anywhere else is a failure.
"""

from __future__ import annotations

import json
import random
import string
import sys
from collections import Counter
from dataclasses import asdict, dataclass
from functools import lru_cache
from itertools import permutations
from pathlib import Path
from typing import Any, Dict, List, Optional, Sequence, Tuple

ROOT = Path(__file__).resolve().parents[1]
for _p in (ROOT, ROOT / "tools"):
    if str(_p) not in sys.path:
        sys.path.insert(0, str(_p))

import feinsum_amd as f  # noqa: E402
from feinsum_amd.measure import launch_kind  # noqa: E402
from fuzz_dg import (E_CLASSES, ORDERS2, ORDERS3, Stats, _compare, _out_buffers, host_data, missing_buckets,  # noqa: E402,F401
                     references, tname)

FE_MAX_FIELDS = 8     # include/feinsum_hip.h
TRANSFORMS = ("auto", "mfma", "tiled", "generic", "prepared")
NEAR_TRANSFORMS = (None, "auto", "generic")

#: the forward templates, written out by hand: (subscripts, family, role of each operand).  tests/test_bind_fuzz_cpu.py
#: checks that the subscripts are exactly those of ``family._TEMPLATES``.
TEMPLATES: Tuple[Tuple[str, str, Tuple[str, ...]], ...] = (
    ("xre,rij,ej->xei", "grad", ("J", "D", "u")), ("xre,rji,ej->xei", "grad", ("J", "D", "u")),
    ("xre,rij,xej->ei", "div", ("J", "D", "u")), ("xre,rji,xej->ei", "div", ("J", "D", "u")),
    ("re,rij,ej->ei", "divcomp", ("J", "D", "u")), ("re,rji,ej->ei", "divcomp", ("J", "D", "u")),
    ("er,rij,ej->ei", "divcomp", ("J", "D", "u")), ("er,rji,ej->ei", "divcomp", ("J", "D", "u")),
    ("e,ij,ej->ei", "matapply", ("J", "D", "u")), ("e,ji,ej->ei", "matapply", ("J", "D", "u")),
    ("ij,ej->ei", "matapply", ("D", "u")), ("ji,ej->ei", "matapply", ("D", "u")),
    ("ef,fij,fej->ei", "facemass", ("J", "R", "v")), ("ef,ifj,fej->ei", "facemass", ("J", "R", "v")),
    ("ef,fji,fej->ei", "facemass", ("J", "R", "v")), ("ef,jfi,fej->ei", "facemass", ("J", "R", "v")),
    ("fe,fij,fej->ei", "facemass", ("J", "R", "v")), ("fe,ifj,fej->ei", "facemass", ("J", "R", "v")),
    ("fe,fji,fej->ei", "facemass", ("J", "R", "v")), ("fe,jfi,fej->ei", "facemass", ("J", "R", "v")),
)
FAMILY_OF = {subs: fam for subs, fam, _ in TEMPLATES}
#: (subscripts, dimension): the templates on tetrahedra, and grad / div / div component / lift on triangles
SHAPES: Tuple[Tuple[str, int], ...] = tuple((subs, 3) for subs, _, _ in TEMPLATES) + (
    ("xre,rij,ej->xei", 2), ("xre,rij,xej->ei", 2), ("re,rij,ej->ei", 2), ("ef,fij,fej->ei", 2))
#: batched einsums of the row-structure cases
ROW_SUBS = ("xre,rij,ej->xei", "xre,rji,ej->xei", "xre,rij,xej->ei", "re,rij,ej->ei", "re,rji,ej->ei", "ef,fij,fej->ei",
            "fe,ifj,fej->ei", "ef,fji,fej->ei", "fe,jfi,fej->ei", "e,ij,ej->ei", "e,ji,ej->ei")
#: near misses: kind -> [(subscripts, what differs from the template)]; "dims" names a change of an extent instead
NEAR: Dict[str, Tuple[Tuple[str, str], ...]] = {
    "out-perm": (("xre,rij,ej->xie", ""), ("re,rij,ej->ie", ""), ("ef,fij,fej->ie", "")),
    "operand-perm": (("rxe,rij,ej->xei", ""), ("exr,rij,ej->xei", ""), ("re,rij,je->ei", ""), ("ij,je->ei", "")),
    "non-square": (("xre,rij,ej->xei", "j+1"), ("e,ij,ej->ei", "j+1"), ("re,rij,ej->ei", "j+1")),
    "x!=r": (("xre,rij,ej->xei", "r-1"), ("xre,rij,xej->ei", "r-1")),
    "ndim": (("xre,rij,ej->xei", "nd1"), ("xre,rij,xej->ei", "nd4"), ("re,rij,ej->ei", "nd4"), ("re,rij,ej->ei", "nd1")),
    "repeated": (("e,ii,ei->ei", ""), ("re,rii,ei->ei", ""), ("xre,rjj,ej->xej", "")),
}
ROW_TABLES = ("random", "nonadjacent", "duplicate", "big")
#: 're,rij,ej->ei' tables: each condition of ``_bind_planes`` from both sides (:func:`planes_conditions`)
PLANE_TABLES = ("planes-2j", "planes-3j", "planes-4j", "planes-unequal", "planes-one", "planes-dup", "planes-2op",
                "planes-er", "planes-tri", "planes-reversed", "planes-big", "planes-big2")
PLANE_CONDITIONS = ("re-layout", "tets", "one-operator", "jnames<=3", "equal-count", "count>=2", "no-duplicate")

#: minimum cases per bucket (per-transform buckets: runs) of the fixed-seed sweep
MINIMUMS = {**{f"template:{subs}@{nd}d": 3 for subs, nd in SHAPES},
            **{f"order:3-{k}": 2 for k in range(6)}, **{f"order:2-{k}": 2 for k in range(2)},
            "renamed": 20, "concrete-E": 10, "near": 20, **{f"near:{k}": 2 for k in NEAR},
            "rows:non-adjacent-sharing": 10, "rows:duplicate": 10, "rows:>16": 10,
            "alias:same-tensor": 10, "alias:equal-copies": 10,
            **{f"planes:{c}:{side}": 1 for c in PLANE_CONDITIONS for side in ("yes", "no")},
            "planes:launch": 4, "planes:sort-reverses-rows": 1, "planes:fields>8": 1, "planes:fields>16": 1,
            **{f"transform:{t}": 20 for t in TRANSFORMS},
            **{f"E:{c}": 4 for c in ("one", "sub-tile", "tiles", "ragged", "static-rounds")},
            "dtype:float64": 30, "dtype:float32": 20}


@dataclass(frozen=True)
class BindCase:
    mode: str            # "spell", "near" or "rows"
    subs: str            # the template (or near-miss) subscripts in canonical letters and operand order
    nd: int              # 3: tetrahedra (nf = 4), 2: triangles (nf = 3); near misses "ndim": 1 or 4
    Np: int
    Nfp: int
    dtype: str           # "float64" or "float32" (every operand)
    E: int
    eclass: str
    seed: int            # data, letters, names and the rows are drawn from it
    order: int = 0       # which permutation of the operands (index into itertools.permutations)
    renamed: bool = False
    concrete: bool = False     # the element axis is the integer E instead of a size parameter
    table: str = ""      # rows: one of ROW_TABLES / PLANE_TABLES
    alias: str = "none"  # "same": two names, one device tensor; "copies": two names, equal-valued distinct tensors
    near: str = ""       # near misses: kind, and what differs
    tweak: str = ""
    scale: str = "normal"

    def repro(self) -> str:
        return json.dumps(asdict(self), separators=(",", ":"))

    @staticmethod
    def from_repro(text: str) -> "BindCase":
        return BindCase(**json.loads(text))

    def stages(self):
        b = build(self)
        return [(b.expr, b.keys)]

    def transforms(self) -> List[Any]:
        if self.mode == "near":
            return list(NEAR_TRANSFORMS)
        return [{"prepared": True} if t == "prepared" else t for t in TRANSFORMS]


@dataclass(frozen=True)
class Built:
    expr: Any
    keys: Any                    # {array name: data key}; two aliased names share a key
    rows: Tuple[Tuple[Optional[str], str, str], ...]   # (J, operator, field) NAMES per row (J None: 'ij,ej->ei')
    pair: Optional[Tuple[str, str]]                    # the two aliased names
    e_letter: str
    sizes: Any                   # {size parameter: E} (empty: concrete element axis)

    def e_axis(self, expr, name: Optional[str]) -> Optional[int]:
        if name is None:
            idxs = expr.out_idx_set
        else:
            pos = next(p for row in expr.args for p, a in enumerate(row) if a.name == name)
            idxs = expr.in_idx_sets[pos]
        return idxs.index(self.e_letter) if self.e_letter in idxs else None


def _split(subs: str):
    lhs, rhs = subs.split("->")
    return [tuple(s) for s in lhs.split(",")], tuple(rhs)


def _extents(case: BindCase) -> Dict[str, int]:
    nd, tw = case.nd, case.tweak
    if tw.startswith("nd"):
        nd = int(tw[2:])
    ext = {"e": case.E, "x": nd, "r": nd, "i": case.Np, "j": case.Nfp if "f" in case.subs else case.Np,
           "f": 4 if nd == 3 else 3}
    if tw == "j+1":
        ext["j"] += 1
    if tw == "r-1":
        ext["r"] -= 1
    return ext


def _names(rng: random.Random, n: int, taken: Sequence[str]) -> List[str]:
    out: List[str] = []
    while len(out) < n:
        nm = rng.choice(string.ascii_uppercase) + "".join(rng.choice(string.ascii_lowercase + string.digits + "_")
                                                          for _ in range(rng.randint(1, 4)))
        if nm not in out and nm not in taken:
            out.append(nm)
    return out


def _plane_rows(table: str, rng: random.Random) -> List[Tuple[str, str, str]]:
    """(J label, operator label, field label) rows of a 're,rij,ej->ei' table."""
    two = lambda nu: [(f"J{x}", "D0", f"u{k}") for k in range(nu) for x in range(2)]   # noqa: E731
    if table in ("planes-2j", "planes-er", "planes-tri"):
        rows = two(rng.randint(2, 4))
    elif table == "planes-3j":       # every field takes two of the three factors (the cross product), or all three
        full = rng.random() < 0.5
        rows = [(f"J{x}", "D0", f"u{k}") for k in range(rng.randint(2, 4))
                for x in (range(3) if full else sorted(rng.sample(range(3), 2)))]
        if len({r[0] for r in rows}) < 3:
            rows += [(f"J{x}", "D0", "u9") for x in (0, 2)] + [("J1", "D0", "u8"), ("J2", "D0", "u8")]
    elif table == "planes-4j":
        rows = [(f"J{x}", "D0", f"u{k}") for k in range(rng.randint(2, 3)) for x in (2 * (k % 2), 2 * (k % 2) + 1)]
    elif table == "planes-unequal":
        rows = two(2) + [("J2", "D0", "u0")]
    elif table == "planes-one":
        rows = [(f"J{k % 3}", "D0", f"u{k}") for k in range(rng.randint(2, 5))]
    elif table == "planes-dup":
        rows = two(rng.randint(2, 3))
        rows.append(rows[rng.randrange(len(rows))])
    elif table == "planes-2op":
        rows = two(rng.randint(2, 3))
        k = rng.randrange(len(rows))
        rows[k] = (rows[k][0], "D1", rows[k][2])
    elif table == "planes-reversed":  # not shuffled: build() names the factors so that sorting them reverses this order
        return [(f"J{x}", "D0", f"u{k}") for k in range(rng.randint(2, 3)) for x in range(3)]
    elif table == "planes-big":
        rows = two(rng.randint(FE_MAX_FIELDS + 1, FE_MAX_FIELDS + 2))              # 9 or 10 fields: one split
    elif table == "planes-big2":
        rows = two(2 * FE_MAX_FIELDS + 1)                                            # 17 fields: two splits
    else:
        raise ValueError(table)
    rng.shuffle(rows)
    return rows


def _label_rows(case: BindCase, rng: random.Random, n_ops: int) -> List[Tuple[str, ...]]:
    if case.mode != "rows":
        return [("J0", "D0", "u0")[3 - n_ops:]]
    t = case.table
    if t.startswith("planes"):
        return _plane_rows(t, rng)
    top = 2 * FE_MAX_FIELDS + 3
    if t == "big":           # one group of more than 2 * FE_MAX_FIELDS rows (the field pool may be smaller)
        b = rng.randint(2 * FE_MAX_FIELDS + 1, top)
        nu = rng.choice([b, b, b // 2])
        return [("J0", "D0", f"u{rng.randrange(nu) if nu < b else k}") for k in range(b)]
    if t == "nonadjacent":   # two (J, operator) pairs in turns: the rows that share are never neighbours
        b = rng.randint(3, 12)
        pairs = rng.choice([[("J0", "D0"), ("J1", "D0")], [("J0", "D0"), ("J0", "D1")], [("J1", "D1"), ("J0", "D0")]])
        nu = rng.randint(2, b)
        rows = [pairs[k % 2] + (f"u{rng.randrange(nu)}",) for k in range(b)]
        rows[1] = rows[1][:2] + ("u0",)
        rows[0] = rows[0][:2] + ("u1",)
        return rows
    b = rng.randint(2, top)
    nj, nd_, nu = rng.randint(1, 4), rng.randint(1, 2), rng.randint(1, b)
    rows = [(f"J{rng.randrange(nj)}", f"D{rng.randrange(nd_)}", f"u{rng.randrange(nu)}") for _ in range(b)]
    if t == "duplicate":
        for _ in range(rng.randint(1, 3)):
            if len(rows) < top:
                rows.insert(rng.randrange(len(rows) + 1), rows[rng.randrange(len(rows))])
        if len(set(rows)) == len(rows):
            rows[-1] = rows[0]
    return rows


@lru_cache(maxsize=64)
def build(case: BindCase) -> Built:
    """The einsum of the case as the user would spell it, the data key of every array, and the role names per row."""
    rng = random.Random(case.seed)
    t_in, t_out = _split(case.subs)
    n = len(t_in)
    letters = sorted({c for s in t_in for c in s})
    ren = dict(zip(letters, rng.sample(string.ascii_lowercase, len(letters)))) if case.renamed else {c: c for c in letters}
    size = rng.choice(["E", "N", "Nel", "K_"]) if case.renamed else "E"
    ext = _extents(case)
    perm = list(permutations(range(n)))[case.order]      # operand p of the einsum is operand perm[p] of the template
    labels = _label_rows(case, rng, n)
    used = list(dict.fromkeys(lb for row in labels for lb in row))
    names = dict(zip(used, _names(rng, len(used), (size,))))
    if case.table == "planes-reversed":                  # sorted(names of the factors) is the reverse of the row order
        js = [lb for lb in used if lb.startswith("J")]
        for lb, nm in zip(js, sorted((names[lb] for lb in js), reverse=True)):
            names[lb] = nm
    shape = lambda idxs: tuple((case.E if case.concrete else size) if c == "e" else ext[c] for c in idxs)   # noqa: E731
    rows = [[f.array(names[row[perm[p]]], shape(t_in[perm[p]]), case.dtype) for p in range(n)] for row in labels]
    subs = ",".join("".join(ren[c] for c in t_in[perm[p]]) for p in range(n)) + "->" + "".join(ren[c] for c in t_out)
    expr = f.batched_einsum(subs, rows)
    keys = {names[lb]: lb for lb in used}
    pair = None
    if case.alias != "none":     # two geometry factors (J / J') if the rows have two, else two fields
        for prefix in ("J", "u"):
            cand = [lb for lb in used if lb.startswith(prefix)]
            if len(cand) >= 2:
                a, b = rng.sample(cand, 2)
                keys[names[b]] = a
                pair = (names[a], names[b])
                break
    role_rows = tuple((names[row[0]] if n == 3 else None, names[row[-2]], names[row[-1]]) for row in labels)
    return Built(expr, keys, role_rows, pair, ren["e"], {} if case.concrete else {size: case.E})


# --------------------------------------------------------------------------
# what the binding layer is documented to do, written down independently of it
# --------------------------------------------------------------------------

def planes_conditions(subs: str, nd: int, rows: Sequence[Tuple[Optional[str], str, str]]) -> Dict[str, bool]:
    """The conditions under which rows of 're,rij,ej->ei' become ONE planes launch (``_bind_planes``): J stored ``re``,
    tetrahedra, one operator, at most three geometry factors, every field with the same number of planes, that number
    at least two, and no (field, factor) pair twice."""
    per: Dict[str, List[str]] = {}
    for j, _, u in rows:
        per.setdefault(u, []).append(j)
    counts = {len(set(js)) for js in per.values()}
    return {"re-layout": subs.startswith("re,"), "tets": nd == 3,
            "one-operator": len({d for _, d, _ in rows}) == 1,
            "jnames<=3": len({j for j, _, _ in rows}) <= 3,
            "equal-count": len(counts) == 1, "count>=2": min(counts) >= 2,
            "no-duplicate": len({(j, u) for j, _, u in rows}) == len(rows)}


def groups_of(subs: str, nd: int, dtype: str, rows: Sequence[Tuple[Optional[str], str, str]]) -> Tuple[str, List[int]]:
    """``(entry point, rows per launch)`` of a family einsum whose rows read the arrays *rows* (``(J, operator, field)``
    NAMES): consecutive rows with the same geometry-factor and operator names share a launch; div components go row
    by row, or -- float64, :func:`planes_conditions` -- all together through the planes launch."""
    fam = FAMILY_OF[subs]
    if fam == "divcomp":
        if dtype == "float64" and all(planes_conditions(subs, nd, rows).values()):
            return "fe_gradplanes", [len(rows)]
        return "fe_divcomp", [1] * len(rows)
    groups: List[int] = []
    for k, (j, d, _) in enumerate(rows):
        if k and (j, d) == tuple(rows[k - 1][:2]):
            groups[-1] += 1
        else:
            groups.append(1)
    return f"fe_{fam}", groups


def launch_groups(case: BindCase) -> List[int]:
    return groups_of(case.subs, case.nd, case.dtype, build(case).rows)[1]


def predict_entry_points(case: BindCase) -> Tuple[str, ...]:
    """``bind_operator([...], fuse=False).entry_points`` under the default transform, from :func:`groups_of`."""
    if case.mode == "near":
        return ("fe_einsum_generic",) * len(build(case).rows)
    entry, groups = groups_of(case.subs, case.nd, case.dtype, build(case).rows)
    return (entry,) * len(groups)


MFMA_ORDERS = {("grad", 3): (4, 10, 20, 35, 56), ("div", 3): (4, 10, 20, 35, 56), ("divcomp", 3): (4, 10, 20, 35, 56),
               ("grad", 2): (3, 6, 10, 15, 21), ("div", 2): (3, 6, 10, 15, 21), ("divcomp", 2): (3, 6, 10, 15, 21),
               ("matapply", 3): (3, 4, 6, 10, 15, 20, 35, 56)}
FM_MFMA = {(4, 56, 21), (4, 35, 15), (4, 20, 10), (4, 10, 6), (4, 4, 3), (3, 21, 6), (3, 15, 5), (3, 10, 4), (3, 6, 3),
           (3, 3, 2)}


def accepted_on_host(case: BindCase, transform: Any) -> bool:
    """Whether the kernels take the case under *transform* (include/feinsum_hip.h): ``None`` / ``"auto"`` /
    ``"generic"`` / ``"tiled"`` / prepared always; all-float32 einsums ignore the variant; a forced ``"mfma"`` needs a
    compiled order, and for face-mass at least two rows in every launch."""
    t = tname(transform)
    if case.mode == "near":
        return t in ("auto", "generic")
    if t != "mfma" or case.dtype == "float32":
        return True
    fam = FAMILY_OF[case.subs]
    if fam == "facemass":
        return (4 if case.nd == 3 else 3, case.Np, case.Nfp) in FM_MFMA and min(launch_groups(case)) >= 2
    return case.Np in MFMA_ORDERS[(fam, 3 if fam == "matapply" else case.nd)]


# --------------------------------------------------------------------------
# cases and coverage (host only)
# --------------------------------------------------------------------------

_ECYCLE = ("tiles", "ragged", "sub-tile", "ragged", "one", "tiles", "ragged", "sub-tile", "tiles", "ragged", "one")


def _mk(rng: random.Random, mode: str, subs: str, nd: int, k: int, **kw) -> BindCase:
    Np, Nfp = rng.choice(ORDERS2 if nd == 2 else ORDERS3[:5] if mode != "spell" or rng.random() < 0.85 else ORDERS3)
    eclass = kw.pop("eclass", None) or _ECYCLE[k % len(_ECYCLE)]
    E = rng.choice(E_CLASSES[eclass]) if eclass != "static-rounds" else 20_004
    if kw.get("table") in ("big", "planes-big", "planes-big2") and E > 300:
        E, eclass = rng.choice([(17, "ragged"), (129, "ragged"), (64, "tiles"), (256, "tiles")])
    dtype = kw.pop("dtype", None) or ("float32" if k % 3 == 1 else "float64")
    n_ops = len(subs.split("->")[0].split(","))
    order = kw.pop("order", None)
    if order is None:
        order = rng.randrange(6 if n_ops == 3 else 2)
    return BindCase(mode, subs, nd, Np, Nfp, dtype, E, eclass, rng.randrange(1 << 30), order, **kw)


def gen_bind_cases(n: int, seed: int) -> List[BindCase]:
    """Fixed sets (every shape three times with the operand orders in turn; every near miss in both dtypes; every row
    table; every planes table) and *n* random row-structure cases."""
    rng = random.Random(seed)
    cases: List[BindCase] = []
    for s, (subs, nd) in enumerate(SHAPES):
        n_perm = 6 if subs.count(",") == 2 else 2
        for k in range(3):
            cases.append(_mk(rng, "spell", subs, nd, s + k, order=(s + k) % n_perm, renamed=k != 0,
                             concrete=k == 2 and s % 2 == 0))
    for s in range(4):   # one size of the static rounds
        subs, nd = SHAPES[(5 * s) % len(SHAPES)]
        cases.append(_mk(rng, "spell", subs, nd, s, renamed=True, eclass="static-rounds", dtype="float64"))
    k = 0
    for kind, variants in NEAR.items():
        for subs, tweak in variants:
            for dt in ("float64", "float32"):
                k += 1
                cases.append(_mk(rng, "near", subs, 3, k, near=kind, tweak=tweak, dtype=dt, order=0,
                                 renamed=k % 2 == 0, concrete=k % 5 == 0))
    aliases = ("same", "copies", "none")
    tables = [t for t in ("nonadjacent", "duplicate", "big") for _ in range(11)] + ["random"] * n
    for k, table in enumerate(tables):
        subs = ROW_SUBS[k % len(ROW_SUBS)]
        if table == "big" and FAMILY_OF[subs] == "divcomp":
            subs = "xre,rij,ej->xei"
        cases.append(_mk(rng, "rows", subs, 3, k, table=table, alias=aliases[k % 3], renamed=k % 2 == 1,
                         concrete=k % 7 == 0))
    for k, table in enumerate(PLANE_TABLES + PLANE_TABLES[:6]):
        subs = {"planes-er": "er,rij,ej->ei"}.get(table, ("re,rij,ej->ei", "re,rji,ej->ei")[k % 2])
        cases.append(_mk(rng, "rows", subs, 2 if table == "planes-tri" else 3, k, table=table, dtype="float64",
                         alias=aliases[k % 3], renamed=k % 2 == 0, concrete=k % 5 == 1))
    for k, table in enumerate(("planes-2j", "planes-3j", "planes-big")):   # float32: never a planes launch
        cases.append(_mk(rng, "rows", "re,rij,ej->ei", 3, k, table=table, dtype="float32", alias=aliases[k % 3]))
    return cases


def _non_adjacent_sharing(rows) -> bool:
    key = [r[:2] for r in rows]
    return any(key[a] == key[c] and any(key[b] != key[a] for b in range(a + 1, c))
               for a in range(len(rows)) for c in range(a + 2, len(rows)))


def case_buckets(case: BindCase) -> List[str]:
    """Buckets a case counts in once (when at least one of its transforms ran)."""
    b = [f"mode:{case.mode}", f"dtype:{case.dtype}", f"E:{case.eclass}"]
    if case.renamed:
        b.append("renamed")
    if case.concrete:
        b.append("concrete-E")
    if case.mode == "near":
        return b + ["near", f"near:{case.near}"]
    rows = build(case).rows
    b.append(f"order:{3 if rows[0][0] is not None else 2}-{case.order}")
    if case.mode == "spell":
        b.append(f"template:{case.subs}@{case.nd}d")
        return b
    if _non_adjacent_sharing(rows):
        b.append("rows:non-adjacent-sharing")
    if len(set(rows)) < len(rows):
        b.append("rows:duplicate")
    if len(rows) > 2 * FE_MAX_FIELDS:
        b.append("rows:>16")
    if build(case).pair is not None:
        b.append("alias:same-tensor" if case.alias == "same" else "alias:equal-copies")
    if FAMILY_OF[case.subs] == "divcomp" and case.dtype == "float64":
        cond = planes_conditions(case.subs, case.nd, rows)
        # a condition counts from the "no" side only where it alone refuses the table
        for c, ok in cond.items():
            if ok:
                b.append(f"planes:{c}:yes")
            elif all(v for k2, v in cond.items() if k2 != c):
                b.append(f"planes:{c}:no")
        if all(cond.values()):
            b.append("planes:launch")
            js = list(dict.fromkeys(r[0] for r in rows))
            if len(js) > 1 and sorted(js) == js[::-1]:
                b.append("planes:sort-reverses-rows")
            fields = len({r[2] for r in rows})
            b += ["planes:fields>8"] * (fields > FE_MAX_FIELDS) + ["planes:fields>16"] * (fields > 2 * FE_MAX_FIELDS)
    return b


def coverage(cases: Sequence[BindCase]) -> Tuple[Counter, int, int]:
    """``(buckets, (case, transform) pairs the host plan accepts, all pairs)``."""
    cnt: Counter = Counter()
    run = total = 0
    for c in cases:
        ts = [t for t in c.transforms() if accepted_on_host(c, t)]
        total += len(c.transforms())
        run += len(ts)
        if ts:
            cnt.update(case_buckets(c))
        cnt.update(f"transform:{tname(t)}" for t in ts if c.mode != "near")
    return cnt, run, total


# --------------------------------------------------------------------------
# the pass (GPU)
# --------------------------------------------------------------------------

def bind_arrays(torch, case: BindCase, dev: Dict[str, Any], alias: str) -> Dict[str, Any]:
    """``{array name: device tensor}``: two aliased names get ONE tensor (``"same"``) or equal-valued distinct ones."""
    b = build(case)
    args = {nm: dev[k] for nm, k in b.keys.items()}
    if b.pair is not None and alias != "same":
        args[b.pair[1]] = dev[b.keys[b.pair[1]]].clone()
    return args


def _run(torch, case: BindCase, args, transform):
    bufs, out_dicts = _out_buffers(torch, case)
    f.evaluate(build(case).expr, 0, args, out_dict=out_dicts[0], transform=transform, wait=True)
    return bufs, out_dicts


def _bind_case(torch, case: BindCase, st: Stats) -> None:
    import numpy as np

    b = build(case)
    arrays, mants, scales, sig = host_data(case)
    dev = {k: torch.from_numpy(np.ascontiguousarray(a)).cuda() for k, a in arrays.items()}
    refs = references(torch, case, arrays, mants, scales, sig, dev, st, e_axis=b.e_axis)
    args = bind_arrays(torch, case, dev, case.alias)
    what = f"{case.mode} {b.expr.get_subscripts()} b={len(b.rows)} {case.table}{case.near} Np={case.Np} {case.dtype} E={case.E}"
    # ---- which launches: never a family launch for a near miss; the predicted groups for everything else
    kind = launch_kind(b.expr, None, b.sizes)
    if (kind == "family") != (case.mode != "near"):
        st.fail(f"launch kind {kind}: {what}  REPRO {case.repro()}")
    if case.mode != "near":
        got = f.bind_operator([(b.expr, args)], 0, fuse=False).entry_points
        if tuple(got) != predict_entry_points(case):
            st.fail(f"launch shape: {len(got)} x {sorted(set(got))}, predicted {len(predict_entry_points(case))} x"
                    f" {sorted(set(predict_entry_points(case)))}: {what}  REPRO {case.repro()}")
        else:
            st.cov["launch-shape:as-predicted"] += 1
    ran = False
    for t in case.transforms():
        try:
            bufs, out_dicts = _run(torch, case, args, t)
        except NotImplementedError as exc:
            st.cov["refused:" + tname(t)] += 1
            if accepted_on_host(case, t) or tname(t) in ("auto", "generic"):
                st.fail(f"refused under {tname(t)} ({str(exc)[:80]}): {what}  REPRO {case.repro()}")
            continue
        ran = True
        if case.mode != "near":
            st.cov[f"transform:{tname(t)}"] += 1
        st.cov["pairs-run"] += 1
        _compare(st, f"bind {tname(t)}: {what}", refs, out_dicts, bufs, case)
        if b.pair is not None and tname(t) == "auto" and t is not None:
            # the other way of binding the two names: one tensor <-> equal copies; the results agree bitwise
            other = bind_arrays(torch, case, dev, "copies" if case.alias == "same" else "same")
            _, out2 = _run(torch, case, other, t)
            same = all(torch.equal(out_dicts[0][nm], out2[0][nm]) for nm in b.expr.output_names)
            st.cov["alias:both-bindings-agree"] += int(same)
            if not same:
                st.fail(f"one tensor under two names != equal copies: {what}  REPRO {case.repro()}")
    st.cov["pairs"] += len(case.transforms())
    if ran:
        st.cov.update(case_buckets(case))


def run_bindings(n: int, seed: int, cases: Optional[Sequence[BindCase]] = None) -> Stats:
    """The sweep; ``cov["pairs-run"] / cov["pairs"]`` is the share of (case, transform) pairs that ran, and
    ``cov["refused:<transform>"]`` counts the refusals."""
    import torch

    st = Stats(f"dg bindings seed={seed}")
    for case in gen_bind_cases(n, seed) if cases is None else cases:
        _bind_case(torch, case, st)
    return st


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--repro":
        s = run_bindings(0, 0, [BindCase.from_repro(sys.argv[2])])
    else:
        s = run_bindings(int(sys.argv[1]) if len(sys.argv) > 1 else 30, int(sys.argv[2]) if len(sys.argv) > 2 else 0)
    print(s.report())
    sys.exit(1 if s.failures else 0)
