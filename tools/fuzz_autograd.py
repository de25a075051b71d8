"""Seeded sweep of the backward pass of :func:`feinsum_amd.evaluate_differentiable` against the
references of oracle/einsum_ref.py (test infrastructure, like tests/): the single-stage DG einsums of tools/fuzz_dg.py
and random einsums of tools/fuzz_einsum.py, every input requiring grad.

    python tools/fuzz_autograd.py [n_cases] [seed]

Every case predicts on the host which route each adjoint term takes (:func:`plan_backward`: the logic of
``autograd._run_term``), and the device run must count exactly those launches in ``autograd.launch_counts``.

Passes:

``run_exact``      exact data (``m * 2**s``, bits and scales per array NAME, the output gradients included): every
                   gradient bitwise equal to the sum of the int64 einsums of the mantissas over all its adjoint terms and
                   rows (or, at E > 4099, to torch's float64 einsum, checked against the int64 einsum on slices); the
                   forward outputs bitwise exact too; near-overflow and subnormal scales.
``run_bounded``    signed uniform data: ``|got - ref| <= gamma(n, u) * absref`` entrywise, n = the term's summed points
                   plus the additions across terms and rows; one more float32 rounding for a float32 operand of a float64
                   einsum.
``run_nonfinite``  exact data with one NaN / +Inf / -Inf planted in a field, a geometric factor, an operator entry or an
                   output gradient: exactly the union of the dependency sets of the gradient's terms is NaN / non-finite,
                   every other entry bitwise exact.
``run_large``      grad, div and face-mass x 9 at E = 98 304 ... 1 000 003 (and float32 grad at about 10^5): every
                   gradient checked over the whole array.
``run_kernels``    the two adjoint kernels and the two operator-gradient kernels called directly, every compiled shape and
                   layout, outputs (and the operator-gradient workspace, exactly its planned bytes) in NaN-filled buffers
                   between sentinel guard bands.

A fixed share of the exact, bounded, non-finite and large passes runs with ``operator_gradients="kernel"`` (the
operator gradients dD, dR on the matrix cores: routes "opgrad_d" / "opgrad_r", predicted from ``match_operator_adjoint``
with their fall-backs to the other routes), some of it with the operator ``frozen`` (no gradient asked: no such launch).
"""

from __future__ import annotations

import json
import math
import random
import sys
from collections import Counter
from dataclasses import asdict, dataclass, replace
from pathlib import Path
from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
for _p in (ROOT, ROOT / "tools"):
    if str(_p) not in sys.path:
        sys.path.insert(0, str(_p))

import feinsum_amd as f  # noqa: E402
import fuzz_dg as D  # noqa: E402
import fuzz_einsum as FE  # noqa: E402
from feinsum_amd import autograd as AG  # noqa: E402
from feinsum_amd.family import (FACEMASS_ADJ_SHAPES, FM_J_FE, FM_R_IFJ, FM_R_T, GEOMADJ_NP,  # noqa: E402
                                OP_TRANSPOSED, match_adjoint_family, match_family, match_operator_adjoint)
from feinsum_amd.measure import launch_kind  # noqa: E402
from fuzz_einsum import Stats, _guarded, _guards_intact, missing_buckets  # noqa: E402,F401
from oracle import einsum_ref as ref_  # noqa: E402

#: the single-stage DG kinds (the fused pipeline is not differentiable)
KINDS = tuple(k for k in D.KINDS if k != "pipeline")
FWD_TRANSFORMS = ("auto", "mfma", "tiled", "generic", "prepared")
ROUTES = ("geomadj", "facemass_v", "facemass_j", "family", "auto", "opgrad_d", "opgrad_r")
OPGRAD_ROUTES = ("opgrad_d", "opgrad_r")
#: E at most this: the int64 reference of the whole array on the host, else torch's float64 einsum on the device
HOST_REF_MAX_E = D.HOST_REF_MAX_E
#: the element of a one-trip-past persistent grid of the adjoint kernels (two blocks of four waves per CU, 16 elements
#: per wave: 32 768 elements per trip on 256 CUs)
MULTI_TRIP_E = 100_003

#: minimum runs per bucket of the fixed-seed exact sweep (tests/test_autograd_fuzz_cpu.py, test_gpu_autograd_fuzz.py)
MINIMUMS = {**{f"kind:{k}": 3 for k in KINDS}, "kind:einsum": 12,
            **{f"order:3d-{n}": 3 for n, _ in D.ORDERS3}, **{f"order:2d-{n}": 2 for n, _ in D.ORDERS2},
            "dtype:float64": 40, "dtype:float32": 20, "dtype:mixed": 15,
            **{f"transform:{t}": 8 for t in FWD_TRANSFORMS},
            **{f"route:{r}": 10 for r in ROUTES}, "route:facemass_j:b>8": 3, "route:auto:Np56": 3,
            **{f"opgrad:kind:{k}": 1 for k in KINDS if k not in ("cross", "divcomp", "apply")}, "opgrad:mode": 40,
            # rows with different J (one kept row of a partial gradient does run on the kernel); no J at all
            "opgrad:fallback:kind:cross": 1, "opgrad:fallback:kind:divcomp": 1, "opgrad:fallback:kind:apply": 1, "opgrad:b>8": 4, "opgrad:frozen-operator": 4,
            "opgrad:partial": 4, "opgrad:fallback:Np56": 2, "opgrad:fallback:float32": 2, "opgrad:fallback:mixed": 2,
            "opgrad:fallback:tiled-order": 2, "opgrad:transform:tiled": 1, "opgrad:transform:prepared": 1,
            "b:>8": 8, "grads:partial": 6, "range:overflow": 3, "range:subnormal": 3,
            "E:one": 3, "E:sub-tile": 3, "E:tiles": 6, "E:ragged": 6, "E:static-rounds": 2,
            "einsum:broadcast": 3, "einsum:twice": 3, "einsum:0d": 3, "einsum:ops3+": 4}


# --------------------------------------------------------------------------
# cases (host only)
# --------------------------------------------------------------------------

@dataclass(frozen=True)
class EinCase:
    """A random einsum outside the DG families: operands named ``names`` (a repeated name: one array used twice)."""

    subs: str
    shapes: Tuple[Tuple[Any, ...], ...]
    dtypes: Tuple[str, ...]
    names: Tuple[str, ...]
    E: int
    seed: int

    def expr(self):
        return f.einsum(self.subs, *[f.array(n, s, dt) for n, s, dt in zip(self.names, self.shapes, self.dtypes)])


@dataclass(frozen=True)
class AGCase:
    """One differentiated evaluation: a DG case (``dg``) or a random einsum (``ein``), the forward transform, the rows
    whose outputs get no gradient (``drop``: ``None`` is passed for them), the exact-data range, how the operator
    gradients run (``operator_gradients``: "auto" or "kernel", the matrix-core kernels of DESIGN.md section 3l) and the
    inputs that do not require a gradient (``frozen``)."""

    dg: Optional[D.DGCase]
    ein: Optional[EinCase]
    transform: str
    drop: Tuple[int, ...] = ()
    scale: str = "normal"
    operator_gradients: str = "auto"
    frozen: Tuple[str, ...] = ()

    def expr(self):
        return self.dg.stages()[0][0] if self.dg is not None else self.ein.expr()

    @property
    def E(self) -> int:
        return self.dg.E if self.dg is not None else self.ein.E

    @property
    def seed(self) -> int:
        return self.dg.seed if self.dg is not None else self.ein.seed

    @property
    def kind(self) -> str:
        return self.dg.kind if self.dg is not None else "einsum"

    @property
    def dtype(self) -> str:
        if self.dg is not None:
            return self.dg.dtype
        return "mixed" if len(set(self.ein.dtypes)) > 1 else self.ein.dtypes[0]

    def fwd_transform(self) -> Any:
        return {"prepared": True} if self.transform == "prepared" else None if self.transform == "auto" else self.transform

    def repro(self) -> str:
        d = asdict(self)
        if self.ein is not None:
            d["ein"]["shapes"] = [list(s) for s in self.ein.shapes]
        return json.dumps(d, separators=(",", ":"))

    @staticmethod
    def from_repro(text: str) -> "AGCase":
        d = json.loads(text)
        dg = D.DGCase(**d["dg"]) if d["dg"] else None
        ein = None
        if d["ein"]:
            e = d["ein"]
            ein = EinCase(e["subs"], tuple(tuple(s) for s in e["shapes"]), tuple(e["dtypes"]), tuple(e["names"]),
                          e["E"], e["seed"])
        return AGCase(dg, ein, d["transform"], tuple(d["drop"]), d["scale"], d.get("operator_gradients", "auto"),
                      tuple(d.get("frozen", ())))


def accepted(case: AGCase) -> bool:
    try:
        launch_kind(case.expr(), case.fwd_transform(), {"E": case.E})
    except NotImplementedError:
        return False
    return True


def _with_transform(rng: random.Random, dg: Optional[D.DGCase], ein: Optional[EinCase], drop=(), scale="normal",
                    transform: Optional[str] = None) -> AGCase:
    order = [transform] if transform else []
    order += rng.sample(FWD_TRANSFORMS, len(FWD_TRANSFORMS))
    for t in order:
        c = AGCase(dg, ein, t, tuple(drop), scale)
        if accepted(c):
            return c
    raise AssertionError("no forward transform takes the case")


def _drop(rng: random.Random, b: int) -> Tuple[int, ...]:
    """Some (not all) rows of a batched case, or none."""
    if b < 2:
        return ()
    k = rng.randint(1, b - 1)
    return tuple(sorted(rng.sample(range(b), k)))


def _dg(rng: random.Random, kind: str, eclass: Optional[str] = None, dtype: Optional[str] = None,
        scale: str = "normal", **over) -> D.DGCase:
    return replace(D._case(rng, kind, eclass, dtype, scale), **over)


def _dg_case(rng: random.Random, c: D.DGCase, partial_share: float = 1 / 3, scale: str = "normal",
             transform: Optional[str] = None) -> AGCase:
    b = c.stages()[0][0].b
    drop = _drop(rng, b) if b > 1 and rng.random() < partial_share else ()
    return _with_transform(rng, c, None, drop, scale, transform)


#: random einsum templates the generator of tools/fuzz_einsum.py rarely makes: an operand used twice (names), a
#: gradient broadcast along an index only its operand carries, 0-d outputs, three or more operands
EIN_FIXED = (("ei,ei->", (("E", 5), ("E", 5)), ("U", "U")),
             ("e,ij,ei,ej->", (("E",), (4, 4), ("E", 4), ("E", 4)), ("W", "A", "X", "X")),
             ("ei,ej,e->ij", (("E", 3), ("E", 3), ("E",)), ("P", "P", "C")),
             ("ij->i", (("E", 6),), ("A",)),
             ("ei,j->", (("E", 7), (3,)), ("P", "Q")),
             ("eij,ej->ei", (("E", 4, 5), ("E", 5)), ("A", "X")),
             ("ej,ej->j", (("E", 17), ("E", 17)), ("P", "Q")),
             ("ik,kj->ij", ((16, 7), (7, 33)), ("A", "B")),
             ("bei,bej->bij", ((3, "E", 4), (3, "E", 6)), ("P", "Q")),
             ("ei,->i", (("E", 4), ()), ("A", "S")))        # a 0-d operand (its gradient expands to ())


def _ein_case(rng: random.Random, c: "FE.Case") -> Optional[EinCase]:
    ins = c.subs.split("->")[0].split(",")
    if any(len(set(o)) != len(o) for o in ins):      # a repeated index: its gradient raises NotImplementedError
        return None
    if c.E == 0 or any(0 in s for s in c.concrete_shapes()) or c.E > HOST_REF_MAX_E:
        return None
    names = [f"A{k}" for k in range(len(ins))]
    for k in range(1, len(ins)):   # an operand used twice where the shapes allow
        for q in range(k):
            if c.shapes[q] == c.shapes[k] and ins[q] != ins[k] and c.dtypes[q] == c.dtypes[k] and rng.random() < 0.5:
                names[k] = names[q]
    return EinCase(c.subs, c.shapes, c.dtypes, tuple(names), c.E, c.seed)


def einsum_cases(n: int, seed: int) -> List[AGCase]:
    rng = random.Random(seed + 17)
    out: List[AGCase] = []
    for c in FE.gen_cases(6 * n, seed + 17, max_points=400_000, max_sum=1 << 16, max_elems=400_000, edges=False):
        e = _ein_case(rng, c)
        if e is not None:
            out.append(_with_transform(rng, None, e, (), "normal", "auto"))
        if len(out) >= n:
            break
    for subs, shapes, names in EIN_FIXED:
        for dts in (("float64",) * len(shapes), ("float32",) * len(shapes), None):
            if dts is None:   # mixed: one name float32, the rest float64
                first = names[0]
                dts = tuple("float32" if nm == first else "float64" for nm in names)
                if len(set(dts)) == 1:
                    continue
            E = rng.choice([1, 16, 17, 63, 1003])
            out.append(_with_transform(rng, None, EinCase(subs, shapes, dts, names, E, rng.randrange(1 << 30)),
                                       (), "normal", "auto"))
    return out


def gen_cases(n: int, seed: int, n_einsum: Optional[int] = None) -> List[AGCase]:
    """*n* random DG cases, the fixed sets (every kind, every order, b = 9 / 17 face-mass and bgrad, tetrahedra p = 5,
    the range cases), and random einsums outside the DG families."""
    rng = random.Random(seed)
    small = ["one", "sub-tile", "tiles", "tiles", "ragged", "ragged", "ragged"]
    cases = [_dg_case(rng, _dg(rng, rng.choice(KINDS), "static-rounds" if rng.random() < 0.05 else rng.choice(small)))
             for _ in range(n)]
    for kind in KINDS:
        for dt in ("float64", "float32", "mixed"):
            cases.append(_dg_case(rng, _dg(rng, kind, rng.choice(small), dt)))
    for Np, Nfp in D.ORDERS3:   # every order, the tiled-only ones and p = 5 included
        for kind in ("grad", "div", "fm", "bdiv"):
            cases.append(_dg_case(rng, _dg(rng, kind, rng.choice(small), "float64", Np=Np, Nfp=Nfp)))
    for Np, Nfp in D.ORDERS2:
        for kind in ("grad2", "lift2"):
            cases.append(_dg_case(rng, _dg(rng, kind, rng.choice(small), rng.choice(["float64", "float32"]), Np=Np,
                                           Nfp=Nfp)))
    for b in (9, 17):   # more fields than one adjoint launch takes (FE_MAX_FIELDS = 8)
        for kind in ("fm", "fm_ifj", "fm_jfi", "fm_fji", "bgrad"):
            cases.append(_dg_case(rng, _dg(rng, kind, rng.choice(["tiles", "ragged"]), "float64", b=b, Np=35, Nfp=15),
                                  partial_share=0.0))
        cases.append(_dg_case(rng, _dg(rng, "lift2", "ragged", "float64", b=b, Np=21, Nfp=6), partial_share=0.0))
    for kind in ("grad", "div", "fm", "divcomp"):   # p = 5: the J-adjoint on "auto"
        cases.append(_dg_case(rng, _dg(rng, kind, rng.choice(["tiles", "ragged"]), "float64", Np=56, Nfp=21)))
    for scale in ("overflow", "subnormal"):
        for dt in ("float64", "float32", "float64"):
            c = _dg(rng, rng.choice(KINDS), rng.choice(["tiles", "ragged", "sub-tile"]), dt)
            cases.append(_dg_case(rng, c, scale=scale))
    cases += einsum_cases(n // 4 if n_einsum is None else n_einsum, seed)
    return cases + kernel_cases(cases, seed)


def kernel_cases(cases: Sequence[AGCase], seed: int) -> List[AGCase]:
    """The share of a case list that runs again with ``operator_gradients="kernel"``: every fifth DG case (partial
    gradients, forward transforms, float32 / mixed and p = 5 fall-backs and the range cases come with them), then fixed
    ones -- every kind, batched kinds with b = 9 (two launches adding to their own slice), partial gradients, the
    operator frozen (no opgrad launch), and the fall-backs by name."""
    rng = random.Random(seed + 59)
    dg = [c for c in cases if c.dg is not None]
    out = [with_kernel(c) for c in dg[::5]]
    small = ["sub-tile", "tiles", "ragged", "ragged"]
    for kind in KINDS:
        tri = kind.endswith("2")
        Np, Nfp = rng.choice(D.ORDERS2) if tri else rng.choice(D.ORDERS3[:4])
        out.append(with_kernel(_dg_case(rng, _dg(rng, kind, rng.choice(small), "float64", Np=Np, Nfp=Nfp), partial_share=0.0)))
    for kind in ("fm", "fm_jfi", "bgrad", "bdiv", "mass"):
        c = _dg(rng, kind, rng.choice(["tiles", "ragged"]), "float64", b=9, Np=20, Nfp=10)
        out.append(with_kernel(_dg_case(rng, c, partial_share=0.0)))
    for kind in ("fm", "fm_ifj", "bgrad", "divcomp", "cross", "lift2"):
        order = dict(Np=10, Nfp=4) if kind == "lift2" else dict(Np=10, Nfp=6)
        c = _dg(rng, kind, rng.choice(small), "float64", b=4, **order)
        out.append(with_kernel(_dg_case(rng, c, partial_share=1.0)))
    for kind in ("grad", "div", "fm", "mass"):
        c = _dg_case(rng, _dg(rng, kind, rng.choice(small), "float64", b=3, Np=20, Nfp=10), partial_share=0.5)
        out.append(with_kernel(c, frozen=tuple(operator_names(c.expr()))))
    for over in (dict(dtype="float64", Np=56, Nfp=21), dict(dtype="float32", Np=20, Nfp=10), dict(dtype="mixed", Np=10, Nfp=6),
                 dict(dtype="float64", Np=7, Nfp=4)):
        for kind in ("grad", "fm"):
            dt = over["dtype"]
            c = _dg(rng, kind, rng.choice(["tiles", "ragged"]), dt, **{k: v for k, v in over.items() if k != "dtype"})
            out.append(with_kernel(_dg_case(rng, c, partial_share=0.0)))
    for t in ("tiled", "prepared"):
        out.append(with_kernel(_dg_case(rng, _dg(rng, "grad", "ragged", "float64", Np=35, Nfp=15), partial_share=0.0, transform=t)))
    return out


# --------------------------------------------------------------------------
# routes (host only)
# --------------------------------------------------------------------------

def route_of(sub, operator_gradients: str = "auto") -> str:
    """The route ``autograd._run_term`` takes for an adjoint einsum (one count in ``launch_counts``): under
    ``operator_gradients="kernel"`` the operator-gradient kernels where ``match_operator_adjoint`` accepts the term
    (float64, a compiled size), else today's routes."""
    if operator_gradients == "kernel":
        op_plan = match_operator_adjoint(sub)
        if op_plan is not None:
            return op_plan.kind
    plan = match_adjoint_family(sub)
    if plan is not None:
        return plan.kind
    return "family" if match_family(sub) is not None else "auto"


def plan_backward(expr, drop: Sequence[int] = (), operator_gradients: str = "auto",
                  frozen: Sequence[str] = ()) -> List[Tuple[str, str, Any, Any]]:
    """``(wrt, route, adjoint einsum of the rows with a gradient, AdjointTerm)`` of every ``_run_term`` call the backward
    pass makes when every input outside *frozen* requires grad and the rows in *drop* get no output gradient."""
    out = []
    for wrt in sorted(expr.all_args):
        if wrt in frozen:
            continue
        for term in AG.adjoint_terms(expr, wrt):
            rows = tuple(row for row, k in zip(term.einsum.args, term.forward_rows) if k not in drop)
            if rows:
                sub = term.einsum.copy(args=rows)
                out.append((wrt, route_of(sub, operator_gradients), sub, term))
    return out


def predicted_launches(case: AGCase) -> Counter:
    return Counter(r for _, r, _, _ in plan_backward(case.expr(), case.drop, case.operator_gradients, case.frozen))


def operator_names(expr) -> List[str]:
    """The inputs without an element axis (D, R)."""
    return [n for n in sorted(expr.all_args) if not any(isinstance(d, f.SizeParam) for d in expr.arg_to_shape[n])]


def with_kernel(case: AGCase, **over) -> AGCase:
    """The case with its operator gradients on the matrix cores."""
    return replace(case, operator_gradients="kernel", **over)


def _eclass(case: AGCase) -> str:
    return case.dg.eclass if case.dg is not None else D.eclass_of(case.E)


def buckets_of(case: AGCase, routes: Sequence[str]) -> List[str]:
    expr = case.expr()
    b = [f"kind:{case.kind}", f"dtype:{case.dtype}", f"transform:{case.transform}", f"E:{_eclass(case)}",
         f"range:{case.scale}"]
    if case.dg is not None:
        b.append(f"order:{'2d' if case.kind.endswith('2') else '3d'}-{case.dg.Np}")
    big = expr.b > 8
    if big:
        b.append("b:>8")
    if case.drop:
        b.append("grads:partial")
    for r in dict.fromkeys(routes):
        b.append(f"route:{r}")
    if "facemass_j" in routes and big:
        b.append("route:facemass_j:b>8")
    if "auto" in routes and case.dg is not None and case.dg.Np == 56:
        b.append("route:auto:Np56")
    if case.operator_gradients == "kernel":
        b.append("opgrad:mode")
        hit = any(r in OPGRAD_ROUTES for r in routes)
        if set(operator_names(expr)) <= set(case.frozen):
            b.append("opgrad:frozen-operator")      # (no opgrad launch: _check_routes holds the run to the prediction)
        elif hit:
            b += [f"opgrad:kind:{case.kind}", f"opgrad:transform:{case.transform}"]
            b += ["opgrad:b>8"] if big else []
            b += ["opgrad:partial"] if case.drop else []
        elif case.dg is not None:
            why = case.dtype if case.dtype != "float64" else "Np56" if case.dg.Np == 56 else \
                "tiled-order" if case.dg.Np in (7, 13) else f"kind:{case.kind}"
            b.append(f"opgrad:fallback:{why}")
    if case.ein is not None:
        ins = case.ein.subs.split("->")[0].split(",")
        if len(set(case.ein.names)) < len(case.ein.names):
            b.append("einsum:twice")
        if not expr.out_idx_set:
            b.append("einsum:0d")
        if len(ins) >= 3:
            b.append("einsum:ops3+")
        if any(len(t.einsum.out_idx_set) < len(t.wrt_subscripts) for _, _, _, t in plan_backward(expr)):
            b.append("einsum:broadcast")
    return b


def coverage(cases: Sequence[AGCase]) -> Counter:
    cnt: Counter = Counter()
    for c in cases:
        cnt.update(buckets_of(c, list(predicted_launches(c).elements())))
    return cnt


# --------------------------------------------------------------------------
# exact data
# --------------------------------------------------------------------------

def _extent(expr, E: int) -> Dict[str, int]:
    return {i: (E if isinstance(d, f.SizeParam) else int(d)) for i, d in expr.index_to_dim_length.items()}


def _shape(expr, name: str, E: int) -> Tuple[int, ...]:
    return tuple(E if isinstance(d, f.SizeParam) else int(d) for d in expr.arg_to_shape[name])


def _row_sig(dtypes) -> int:
    return ref_.compute_significand(dtypes, ref_.f32_step_possible(dtypes, len(dtypes)))


def grad_names(expr, drop: Sequence[int] = ()) -> List[str]:
    return [AG.output_grad_name(n) for k, n in enumerate(expr.output_names) if k not in drop]


def budget_rows(expr, drop: Sequence[int], E: int) -> List[Tuple[List[str], int, int]]:
    """``(array names, products per entry, significand)`` of every row whose sums must be exact: the forward rows, and
    every row of every adjoint term of every input, whose count is the total number of products summed into one
    gradient entry over all the terms and rows added for that input.  Rows of a float32 einsum (or of a float32 step) use
    24 bits; so does every row of the gradient of a float32 operand (it is rounded to float32 at the end)."""
    ext = _extent(expr, E)
    subs = expr.get_subscripts()
    rows = [([a.name for a in row], ref_.summed_points(subs, ext), _row_sig([a.dtype for a in row]))
            for k, row in enumerate(expr.args)]
    per: Dict[str, List[Tuple[List[str], int, int]]] = {}
    for wrt, _, sub, _ in plan_backward(expr, drop):
        n = ref_.summed_points(sub.get_subscripts(), _extent(sub, E))
        f32_wrt = np.dtype(expr.arg_to_dtype[wrt]) == np.dtype("float32")
        for row in sub.args:
            sig = _row_sig([a.dtype for a in row])
            per.setdefault(wrt, []).append(([a.name for a in row], n, min(sig, 24) if f32_wrt else sig))
    for wrt, rs in per.items():
        total = sum(n for _, n, _ in rs)
        rows += [(names, total, sig) for names, _, sig in rs]
    return rows


def plan_data(case: AGCase, rng: np.random.Generator):
    """``(bits, scales, dtypes, S)`` per array name (inputs and output gradients).  Rows of a smaller significand enter
    :func:`oracle.einsum_ref.shared_exact_bits` with their count times ``2**(53 - significand)`` against one common
    significand S (53; 49 for the subnormal range, as tools/fuzz_dg.py).  Scales: every row of the gradient of an input
    has the same total (``C - s_w``: the output-gradient scales make every forward row total plus its gradient's scale
    equal), so the sum over terms and rows is one integer sum; the range cases put every gradient at the range's
    edge."""
    expr = case.expr()
    dtypes = {nm: np.dtype(dt) for nm, dt in expr.arg_to_dtype.items()}
    for k, nm in enumerate(expr.output_names):
        if k not in case.drop:
            dtypes[AG.output_grad_name(nm)] = np.dtype(np.result_type(*[a.dtype for a in expr.args[k]]))
    S = 49 if case.scale == "subnormal" else 53
    rows = [(names, n << (53 - sig), ) for names, n, sig in budget_rows(expr, case.drop, case.E)]
    f32 = [k for k, d in dtypes.items() if d == np.dtype("float32")]
    bits = ref_.shared_exact_bits(rows, f32, S, rng)
    gnames = grad_names(expr, case.drop)
    if case.scale == "normal":
        scales = {nm: int(rng.integers(-8, 9)) for nm in sorted(expr.all_args)}
        C = int(rng.integers(-8, 9))
        for k, nm in enumerate(expr.output_names):
            if k not in case.drop:
                scales[AG.output_grad_name(nm)] = C - sum(scales[a.name] for a in expr.args[k])
    else:
        # every input at one scale s, the output gradients at ``target - (operands - 1) s``: every gradient total is
        # the target -- near overflow, or the subnormal quantum (S four bits short: every gradient sum subnormal)
        top, quantum = ref_.RANGE[np.dtype("float32") if case.dtype == "float32" else np.dtype("float64")]
        s = int(rng.integers(0, 9))
        target = top - (24 if case.dtype == "float32" else 53) if case.scale == "overflow" else quantum
        s = s if case.scale == "overflow" else -s
        scales = {nm: s for nm in expr.all_args}
        for k, nm in enumerate(expr.output_names):
            if k not in case.drop:
                scales[AG.output_grad_name(nm)] = target - (len(expr.args[k]) - 1) * s
    return bits, scales, dtypes, S


def host_data(case: AGCase):
    """``(arrays, mantissas, scales)`` by name, inputs and output gradients."""
    rng = np.random.default_rng(case.seed)
    bits, scales, dtypes, _ = plan_data(case, rng)
    expr = case.expr()
    shapes = {nm: _shape(expr, nm, case.E) for nm in expr.all_args}
    oshape = tuple(case.E if isinstance(d, f.SizeParam) else int(d) for d in expr.shape)
    shapes.update({g: oshape for g in grad_names(expr, case.drop)})
    arrays, mants = {}, {}
    for k in sorted(shapes):
        m, x = ref_.exact_operands([shapes[k]], [dtypes[k]], [bits[k]], [scales[k]], rng)
        mants[k], arrays[k] = m[0], x[0]
    return arrays, mants, scales


def _int_einsum(subs: str, ops: Sequence[np.ndarray]) -> np.ndarray:
    return np.asarray(np.einsum(subs, *ops, optimize=True), dtype=np.int64)


def grad_reference(expr, drop, mants, scales, wrt: str, E: int, skip: Optional[Tuple[int, int]] = None,
                   extra: Optional[Tuple[int, int]] = None) -> Optional[np.ndarray]:
    """The exact gradient of *wrt*: the int64 sum, over every adjoint term and row with an output gradient, of the
    einsum of the mantissas (broadcast to *wrt*'s shape), scaled back -- ``None`` when no row has a gradient.  Asserts
    that every row has the same total scale and that the absolute sum fits the budget.  *skip* / *extra* (``(term,
    row)``) leave a row out / add it twice (the checkers' planted errors)."""
    shape = tuple(np.shape(mants[wrt]))
    total = np.zeros(shape, dtype=np.int64)
    absum = np.zeros(shape, dtype=np.int64)
    scale = None
    hit = False
    for t, (w, _, sub, term) in enumerate(x for x in plan_backward(expr, drop) if x[0] == wrt):
        s = sub.get_subscripts()
        for r, row in enumerate(sub.args):
            if skip == (t, r):
                continue
            ops = [mants[a.name] for a in row]
            sc = sum(scales[a.name] for a in row)
            assert scale is None or sc == scale, "rows of one gradient at different scales"
            scale = sc
            for _ in range(2 if extra == (t, r) else 1):
                total = total + AG.expand_to_operand(_int_einsum(s, ops), sub.out_idx_set, term.wrt_subscripts, shape)
                absum = absum + AG.expand_to_operand(_int_einsum(s, [np.abs(o) for o in ops]), sub.out_idx_set,
                                                     term.wrt_subscripts, shape)
            hit = True
    if not hit:
        return None
    sig = 24 if np.dtype(expr.arg_to_dtype[wrt]) == np.dtype("float32") else 53
    assert (absum <= (1 << sig)).all(), "exact-data budget exceeded"
    return np.ldexp(total.astype(np.float64), int(scale)).astype(np.dtype(expr.arg_to_dtype[wrt]))


def forward_reference(expr, mants, scales, name: str) -> np.ndarray:
    k = list(expr.output_names).index(name)
    row = expr.args[k]
    dts = [a.dtype for a in row]
    return ref_.int_reference(expr.get_subscripts(), [mants[a.name] for a in row], sum(scales[a.name] for a in row),
                              np.result_type(*dts), _row_sig(dts))


def host_references(case: AGCase, mants, scales) -> Tuple[Dict[str, np.ndarray], Dict[str, Optional[np.ndarray]]]:
    expr = case.expr()
    fwd = {n: forward_reference(expr, mants, scales, n) for n in expr.output_names}
    grads = {w: grad_reference(expr, case.drop, mants, scales, w, case.E) for w in sorted(expr.all_args)}
    return fwd, grads


# --------------------------------------------------------------------------
# device references (large E) and dependency sets
# --------------------------------------------------------------------------

def _einsum_chunked(torch, subs: str, ops, e_letter: Optional[str], chunk: int = 1 << 16):
    """torch's float64 einsum of exact data in chunks along the element letter: concatenated where the output carries it,
    summed where it does not (exact under the budget: every partial sum fits the significand)."""
    ins, out = subs.replace(" ", "").split("->")
    ins = ins.split(",")
    axes = [o.index(e_letter) if e_letter and e_letter in o else None for o in ins]
    wide = [t.to(torch.float64) for t in ops]
    if all(a is None for a in axes):
        return torch.einsum(subs, *wide)
    E = next(int(t.shape[a]) for t, a in zip(wide, axes) if a is not None)
    parts = []
    for e0 in range(0, max(E, 1), chunk):
        w = min(chunk, E - e0)
        parts.append(torch.einsum(subs, *[t if a is None else t.narrow(a, e0, w) for t, a in zip(wide, axes)]))
    if e_letter in out:
        return torch.cat(parts, dim=out.index(e_letter))
    total = parts[0]
    for p in parts[1:]:
        total = total + p
    return total


def _e_letter(expr) -> Optional[str]:
    for i, d in expr.index_to_dim_length.items():
        if isinstance(d, f.SizeParam):
            return i
    return None


def device_references(torch, case: AGCase, dev):
    """Forward outputs and gradients on the device: float64 einsums of exact data, summed over terms and rows in
    float64 (exact under the budget), cast to the output / operand dtype."""
    expr = case.expr()
    fwd = {}
    for name, row in zip(expr.output_names, expr.args):
        dt = getattr(torch, np.result_type(*[a.dtype for a in row]).name)
        fwd[name] = _einsum_chunked(torch, expr.get_subscripts(), [dev[a.name] for a in row], _e_letter(expr)).to(dt)
    grads: Dict[str, Any] = {}
    for wrt, _, sub, term in plan_backward(expr, case.drop):
        shape = tuple(dev[wrt].shape)
        for row in sub.args:
            v = _einsum_chunked(torch, sub.get_subscripts(), [dev[a.name] for a in row], _e_letter(sub))
            v = AG.expand_to_operand(v, sub.out_idx_set, term.wrt_subscripts, shape)
            grads[wrt] = v.contiguous() if wrt not in grads else grads[wrt] + v
    out = {w: (grads[w].to(dev[w].dtype) if w in grads else None) for w in sorted(expr.all_args)}
    return fwd, out


def dependency(torch, expr, drop, shapes: Dict[str, Tuple[int, ...]], key: str, idx, E: int, device) -> Dict[str, Any]:
    """``{output or input name: bool tensor}``: the forward outputs and the gradients that depend on entry *idx* of
    array *key* -- the union, over every row of every adjoint term (and every forward row) and over every operand
    position holding *key*, of the einsum of a one-hot array there with all-ones arrays elsewhere
    (oracle.einsum_ref.dependency_set), broadcast to the operand with ``expand_to_operand``."""
    def one(subs, row, out_shape):
        acc = None
        for p, a in enumerate(row):
            if a.name != key:
                continue
            ops = [torch.ones(shapes[b.name], dtype=torch.float64, device=device) for b in row]
            ops[p] = torch.zeros(shapes[key], dtype=torch.float64, device=device)
            ops[p][idx] = 1.0
            v = torch.einsum(subs, *ops) != 0
            acc = v if acc is None else acc | v
        return acc if acc is not None else torch.zeros(out_shape, dtype=torch.bool, device=device)

    oshape = tuple(E if isinstance(d, f.SizeParam) else int(d) for d in expr.shape)
    out = {}
    for name, row in zip(expr.output_names, expr.args):
        out[name] = one(expr.get_subscripts(), row, oshape)
    for wrt, _, sub, term in plan_backward(expr, drop):
        shape = shapes[wrt]
        sub_shape = tuple(shape[term.wrt_subscripts.index(i)] for i in sub.out_idx_set)
        for row in sub.args:
            v = AG.expand_to_operand(one(sub.get_subscripts(), row, sub_shape), sub.out_idx_set, term.wrt_subscripts,
                                     shape)
            out[wrt] = v.clone() if wrt not in out else out[wrt] | v
    return out


# --------------------------------------------------------------------------
# running (GPU)
# --------------------------------------------------------------------------

DEVICE = "cuda"


class Refused(Exception):
    """The device refused the forward transform (a variant not compiled for the shape): counted, then run on "auto"."""


def forward_backward(torch, case: AGCase, dev: Dict[str, Any]):
    """``(forward outputs, {input: gradient or None}, launch counts of the backward pass)``: every input requires grad,
    every output with a gradient in *dev* passes it to ``torch.autograd.backward``, the others pass ``None``."""
    expr = case.expr()
    leaves = {n: dev[n].detach().requires_grad_(n not in case.frozen) for n in sorted(expr.all_args)}
    before = Counter(AG.launch_counts)
    try:
        outs = f.evaluate_differentiable(expr, 0, leaves, transform=case.fwd_transform(),
                                         operator_gradients=case.operator_gradients)
    except NotImplementedError as exc:
        raise Refused(str(exc)) from exc
    keep = [k for k in range(expr.b) if k not in case.drop]
    torch.autograd.backward([outs[expr.output_names[k]] for k in keep],
                            [dev[AG.output_grad_name(expr.output_names[k])] for k in keep])
    torch.cuda.synchronize()
    delta = Counter(AG.launch_counts)
    delta.subtract(before)
    fwd = {n: t.detach() for n, t in outs.items()}
    return fwd, {n: t.grad for n, t in leaves.items()}, +delta


def run_case(torch, st: Stats, case: AGCase, dev):
    """:func:`forward_backward`; a forward transform the device refuses is counted (``not-accepted:<transform>``) and
    the case runs on "auto" instead.  Returns ``(case as run, forward outputs, gradients, launch counts)``."""
    try:
        return (case, *forward_backward(torch, case, dev))
    except Refused:
        st.cov["not-accepted:" + case.transform] += 1
        case = replace(case, transform="auto")
        return (case, *forward_backward(torch, case, dev))


def _label(what: str, case: AGCase) -> str:
    extra = f" Np={case.dg.Np} b={case.dg.b} {case.dg.op}" if case.dg is not None else f" {case.ein.subs}"
    mode = f" opgrad={case.operator_gradients} frozen={list(case.frozen)}" if case.operator_gradients != "auto" or case.frozen else ""
    return f"{what} {case.kind}{extra} {case.dtype} E={case.E} {case.transform} drop={list(case.drop)} {case.scale}{mode}"


def _compare(st: Stats, label: str, case: AGCase, fwd, grads, rfwd, rgrads, deps=None, value=None) -> bool:
    ok = True
    for name, r in list(rfwd.items()) + list(rgrads.items()):
        got = fwd[name] if name in rfwd else grads[name]
        if r is None or got is None:
            if (r is None) != (got is None):
                ok = False
                st.fail(f"{label}: {name}: gradient {'missing' if got is None else 'unexpected'}  REPRO {case.repro()}")
            continue
        st.exact_runs += 1
        if deps is None:
            bad = ref_.differing_entries(got, r)
        else:
            bad = ref_.nonfinite_violations(got, r, deps[name], value)
        if bad:
            ok = False
            st.fail(f"{label}: {name}: {bad} entries {'differ from the exact result' if deps is None else 'break the dependency rule'}"
                    f"  REPRO {case.repro()}")
        else:
            st.exact_equal += 1
    return ok


def _check_routes(st: Stats, label: str, case: AGCase, delta: Counter) -> List[str]:
    want = predicted_launches(case)
    if +want != delta:
        st.fail(f"{label}: backward launches {dict(delta)}, predicted {dict(want)}  REPRO {case.repro()}")
    return list(want.elements())


def _to_dev(torch, arrays):
    return {k: torch.from_numpy(np.array(a, order="C")).to(DEVICE) for k, a in arrays.items()}


def _slice_checks(torch, st: Stats, label: str, case: AGCase, dev, scales, rfwd, rgrads, rng) -> None:
    """The device references against the int64 ones on first / middle / last / random element slices (the forward
    outputs and every gradient whose terms all keep the element axis)."""
    expr = case.expr()
    e = _e_letter(expr)
    E = case.E
    starts = [0, E // 2 - 16, E - 37] + [int(x) for x in rng.integers(0, E - 37, size=2)]
    for e0 in starts:
        w = min(37, E - e0)
        sl = {}
        for k, t in dev.items():
            spec = expr.arg_to_shape.get(k) if k in expr.arg_to_shape else expr.shape
            ax = next((a for a, d in enumerate(spec) if isinstance(d, f.SizeParam)), None)
            v = t if ax is None else t.narrow(ax, e0, w)
            sl[k] = np.ldexp(v.to(torch.float64).cpu().numpy(), -scales[k]).astype(np.int64)
        for name in expr.output_names:
            ax = list(expr.out_idx_set).index(e)
            want = forward_reference(expr, sl, scales, name)
            if not ref_.bitwise_equal(rfwd[name].narrow(ax, e0, w).cpu().numpy(), want):
                st.fail(f"{label}: reference of {name} != int64 einsum on [{e0}, {e0 + w})  REPRO {case.repro()}")
        for wrt in sorted(expr.all_args):
            terms = [t for x, _, _, t in plan_backward(expr, case.drop) if x == wrt]
            if rgrads[wrt] is None or not terms or any(e not in t.einsum.out_idx_set for t in terms):
                continue
            ax = terms[0].wrt_subscripts.index(e)
            want = grad_reference(expr, case.drop, sl, scales, wrt, w)
            if not ref_.bitwise_equal(rgrads[wrt].narrow(ax, e0, w).cpu().numpy(), want):
                st.fail(f"{label}: reference of d{wrt} != int64 einsum on [{e0}, {e0 + w})  REPRO {case.repro()}")


def _prepare(torch, case: AGCase, st: Stats):
    arrays, mants, scales = host_data(case)
    dev = _to_dev(torch, arrays)
    if case.E <= HOST_REF_MAX_E:
        rfwd, rgrads = host_references(case, mants, scales)
        rfwd = {k: torch.from_numpy(np.array(v, order="C")).to(DEVICE) for k, v in rfwd.items()}
        rgrads = {k: (torch.from_numpy(np.array(v, order="C")).to(DEVICE) if v is not None else None)
                  for k, v in rgrads.items()}
    else:
        rfwd, rgrads = device_references(torch, case, dev)
        _slice_checks(torch, st, _label("reference", case), case, dev, scales, rfwd, rgrads,
                      np.random.default_rng(case.seed + 1))
    rgrads = {k: (None if k in case.frozen else v) for k, v in rgrads.items()}     # an input without requires_grad gets none
    return dev, rfwd, rgrads


def run_exact(n: int, seed: int, n_einsum: Optional[int] = None) -> Stats:
    import torch

    st = Stats(f"autograd exact seed={seed}")
    for case in gen_cases(n, seed, n_einsum):
        dev, rfwd, rgrads = _prepare(torch, case, st)
        case, fwd, grads, delta = run_case(torch, st, case, dev)
        label = _label("exact", case)
        routes = _check_routes(st, label, case, delta)
        st.cov.update(buckets_of(case, routes))
        _compare(st, label, case, fwd, grads, rfwd, rgrads)
        del dev, rfwd, rgrads, fwd, grads
    return st


# --------------------------------------------------------------------------
# signed uniform data
# --------------------------------------------------------------------------

def bounded_cases(n: int, seed: int) -> List[AGCase]:
    rng = random.Random(seed + 5)
    out = []
    for k in range(n):
        kind = KINDS[k % len(KINDS)]
        c = _dg(rng, kind, rng.choice(["one", "sub-tile", "tiles", "ragged"]))
        if c.E > 1100:
            c = replace(c, E=rng.choice([63, 64, 65, 127, 128, 129, 1003]))
        if c.Np == 56:
            c = replace(c, E=min(c.E, 129))
        out.append(_dg_case(rng, c))
    for c in (_dg(rng, "fm", "ragged", "float64", b=9, Np=35, Nfp=15),
              _dg(rng, "bgrad", "ragged", "float64", b=17, Np=20, Nfp=10)):
        out.append(_dg_case(rng, replace(c, E=min(c.E, 129)), partial_share=0.0))
    out += [c for c in einsum_cases(max(n // 4, 4), seed + 5) if c.E <= 1100]
    rng = random.Random(seed + 61)      # a fixed share under operator_gradients="kernel"
    kernel = [with_kernel(c) for c in out if c.dg is not None][::4]
    for kind, b in (("grad", 1), ("div", 1), ("fm", 9), ("bgrad", 9), ("divcomp", 1), ("mass", 2), ("lift2", 2)):
        order = dict(Np=15, Nfp=5) if kind == "lift2" else dict(Np=35, Nfp=15)
        c = replace(_dg(rng, kind, "ragged", "float64", b=b, **order), E=rng.choice([65, 129, 1003]))
        kernel.append(with_kernel(_dg_case(rng, c, partial_share=0.0)))
    return out + kernel


def bound_of(expr, drop, wrt: str, E: int, operator_gradients: str = "auto") -> Tuple[int, float, bool]:
    """``(n, u, rounded)`` of a gradient's bound: n = the largest ``operands - 1 + summed points (+ schedule steps)``
    of its term rows plus the additions across terms and rows; u the largest unit roundoff of its rows; *rounded*: a
    float32 operand of a float64 einsum (one more float32 rounding at the end).  A term on the operator-gradient
    kernels: the n tests/test_gpu_opgrad.py derives from ``fe_opgrad_plan`` -- the products per entry, two roundings
    of the J-weighted factor, and the combine: a lane's slices in order, six butterfly steps."""
    from feinsum_amd import _hip

    ns, us, rows = [], [], 0
    for w, route, sub, _ in plan_backward(expr, drop, operator_gradients):
        if w != wrt:
            continue
        for row in sub.args:
            dts = [a.dtype for a in row]
            k = len(row)
            if route in OPGRAD_ROUTES:
                entries = int(np.prod([int(sub.index_to_dim_length[i]) for i in sub.out_idx_set]))
                slices = _hip.opgrad_plan(E, entries)[0]
                ns.append(2 + ref_.summed_points(sub.get_subscripts(), _extent(sub, E)) + 6 + -(-slices // 64))
                us.append(ref_.U64)
                rows += 1
                continue
            ns.append(ref_.bound_terms(sub.get_subscripts(), _extent(sub, E), k, k - 1 if k >= 3 else 0))
            us.append(ref_.unit_roundoff(dts, k))
            rows += 1
    wide = np.result_type(*[a.dtype for row in expr.args for a in row]) == np.dtype("float64")
    rounded = np.dtype(expr.arg_to_dtype[wrt]) == np.dtype("float32") and wide
    return max(ns) + rows - 1, max(us), rounded


def bounded_grad(expr, drop, host, wrt: str) -> Tuple[np.ndarray, np.ndarray]:
    """``(ref, absref)`` in longdouble: the sum over the gradient's term rows."""
    shape = np.shape(host[wrt])
    ref = np.zeros(shape, dtype=np.longdouble)
    absref = np.zeros(shape, dtype=np.longdouble)
    for w, _, sub, term in plan_backward(expr, drop):
        if w != wrt:
            continue
        for row in sub.args:
            r, a = ref_.bounded_reference(sub.get_subscripts(), [host[x.name] for x in row])
            ref = ref + AG.expand_to_operand(r, sub.out_idx_set, term.wrt_subscripts, shape)
            absref = absref + AG.expand_to_operand(a, sub.out_idx_set, term.wrt_subscripts, shape)
    return ref, absref


def grad_bound_ratio(got: np.ndarray, ref, absref, n: int, u: float, rounded: bool) -> float:
    """``max |got - ref| / bound``: bound = ``gamma(n, u) absref``, or with *rounded* ``u32 |ref| + (1 + u32) gamma(n,
    u) absref``; ``inf`` on a non-finite entry or a shape mismatch."""
    if not rounded:
        return ref_.bound_ratio(got, ref, absref, n, u)
    got = np.asarray(got)
    if got.shape != ref.shape:
        return math.inf
    if got.size == 0:
        return 0.0
    g = got.astype(np.longdouble)
    if not np.isfinite(g).all():
        return math.inf
    err = np.abs(g - ref)
    bound = np.longdouble(ref_.U32) * np.abs(ref) + np.longdouble(1 + ref_.U32) * np.longdouble(ref_.gamma(n, u)) * absref
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err == 0, np.longdouble(0), err / bound)
    return float(np.max(ratio))


def bounded_data(case: AGCase) -> Dict[str, np.ndarray]:
    expr = case.expr()
    rng = np.random.default_rng(case.seed)
    host = {}
    for nm in sorted(expr.all_args):
        host[nm] = (rng.random(_shape(expr, nm, case.E)) * 2 - 1).astype(expr.arg_to_dtype[nm])
    oshape = tuple(case.E if isinstance(d, f.SizeParam) else int(d) for d in expr.shape)
    for k, nm in enumerate(expr.output_names):
        if k not in case.drop:
            dt = np.result_type(*[a.dtype for a in expr.args[k]])
            host[AG.output_grad_name(nm)] = np.asarray((rng.random(oshape) * 2 - 1)).astype(dt)
    return host


def run_bounded(n: int, seed: int) -> Stats:
    import torch

    st = Stats(f"autograd bounded seed={seed}")
    for case in bounded_cases(n, seed):
        expr = case.expr()
        host = bounded_data(case)
        case, fwd, grads, delta = run_case(torch, st, case, _to_dev(torch, host))
        label = _label("bounded", case)
        routes = _check_routes(st, label, case, delta)
        bk = buckets_of(case, routes)
        st.cov.update(bk)
        for wrt in sorted(expr.all_args):
            if grads[wrt] is None:
                if wrt not in case.frozen and any(w == wrt for w, _, _, _ in plan_backward(expr, case.drop)):
                    st.fail(f"{label}: d{wrt} missing  REPRO {case.repro()}")
                continue
            n_, u, rounded = bound_of(expr, case.drop, wrt, case.E, case.operator_gradients)
            ref, absref = bounded_grad(expr, case.drop, host, wrt)
            ratio = grad_bound_ratio(grads[wrt].cpu().numpy(), ref, absref, n_, u, rounded)
            for b_ in bk:
                st.worst[b_] = max(st.worst.get(b_, 0.0), ratio)
            if ratio > 1:
                st.fail(f"{label}: d{wrt}: |got - ref| = {ratio:.3g} x the bound (n={n_})  REPRO {case.repro()}")
    return st


# --------------------------------------------------------------------------
# non-finite values
# --------------------------------------------------------------------------

def roles_of(expr, drop) -> Dict[str, str]:
    """Role of every array: "output-grad", "operator" (no element axis), "field" (the last operand of a row) or
    "geometry" (another element-axis operand)."""
    roles = {g: "output-grad" for g in grad_names(expr, drop)}
    for row in expr.args:
        for p, a in enumerate(row):
            if not any(isinstance(d, f.SizeParam) for d in expr.arg_to_shape[a.name]):
                roles[a.name] = "operator"
            else:
                roles.setdefault(a.name, "field" if p == len(row) - 1 else "geometry")
    return roles


def plant_sites(case: AGCase, rng: random.Random, shapes: Dict[str, Tuple[int, ...]]) -> List[Tuple[str, str, Tuple]]:
    """``(role, name, index)``, one per role: elements 15, 16 and E - 1 in turn (the tile ends), and along the other
    axes the last entry (the last row before the 16-row padding of the adjoint kernels), the first or a random one."""
    expr = case.expr()
    roles = roles_of(expr, case.drop)
    E = case.E
    elems = [e for e in (15, 16, E - 1, 0) if 0 <= e < E]
    by_role: Dict[str, List[str]] = {}
    for nm, r in sorted(roles.items()):
        by_role.setdefault(r, []).append(nm)
    sites = []
    for k, (role, names) in enumerate(sorted(by_role.items())):
        nm = rng.choice(names)
        shape = shapes[nm]
        spec = expr.arg_to_shape[nm] if nm in expr.arg_to_shape else expr.shape
        idx = []
        for ax, (s, d) in enumerate(zip(shape, spec)):
            if isinstance(d, f.SizeParam):
                idx.append(elems[(k + rng.randrange(len(elems))) % len(elems)])
            else:
                idx.append(rng.choice([s - 1, s - 1, 0, rng.randrange(s)]))
        sites.append((role, nm, tuple(idx)))
    return sites


def nonfinite_cases(n: int, seed: int) -> List[AGCase]:
    """*n* random DG cases, fixed ones that reach every route (geomadj, the face-mass adjoints with b = 9, the family
    adjoints, "auto" at p = 5), and a few random einsums."""
    rng = random.Random(seed + 7)
    out = [_dg_case(rng, _dg(rng, rng.choice(KINDS), rng.choice(["one", "tiles", "ragged", "ragged"])))
           for _ in range(n)]
    fixed = [_dg(rng, "grad", "tiles", "float64", Np=35, Nfp=15), _dg(rng, "div", "ragged", "float64", Np=20, Nfp=10),
             _dg(rng, "fm", "ragged", "float64", b=9, Np=35, Nfp=15),
             _dg(rng, "fm_jfi", "tiles", "float64", b=4, Np=10, Nfp=6),
             _dg(rng, "lift2", "ragged", "float64", b=2, Np=21, Nfp=6),
             _dg(rng, "grad", "ragged", "float64", Np=56, Nfp=21), _dg(rng, "divcomp", "ragged", "float64", Np=4, Nfp=3),
             _dg(rng, "mass", "tiles", "float64", b=2, Np=35, Nfp=15)]
    out += [_dg_case(rng, c, partial_share=0.0) for c in fixed]
    out += einsum_cases(4, seed + 7)[:6]
    # under operator_gradients="kernel": the fixed cases again (plants in the output gradient and in J among them)
    out += [with_kernel(_dg_case(rng, replace(c, seed=rng.randrange(1 << 30)), partial_share=0.0)) for c in fixed]
    return out


def run_nonfinite(n: int, seed: int) -> Stats:
    import torch

    st = Stats(f"autograd nonfinite seed={seed}")
    rng = random.Random(seed + 9)
    for case in nonfinite_cases(n, seed):
        expr = case.expr()
        dev, rfwd, rgrads = _prepare(torch, case, st)
        shapes = {k: tuple(t.shape) for k, t in dev.items()}
        routes = list(predicted_launches(case).elements())
        for role, key, idx in plant_sites(case, rng, shapes):
            value = rng.choice([math.nan, math.inf, -math.inf])
            old = dev[key][idx].clone()
            dev[key][idx] = value
            deps = dependency(torch, expr, case.drop, shapes, key, idx, case.E, DEVICE)
            case, fwd, grads, delta = run_case(torch, st, case, dev)
            label = _label("nonfinite", case) + f" {value} in {key}{list(idx)}"
            _check_routes(st, label, case, delta)
            st.cov.update([f"planted:{role}", f"value:{value}", f"kind:{case.kind}", f"dtype:{case.dtype}"]
                          + [f"route:{r}" for r in dict.fromkeys(routes)]
                          + ([f"opgrad:planted:{role}"] if any(r in OPGRAD_ROUTES for r in routes) else []))
            _compare(st, label, case, fwd, grads, rfwd, rgrads, deps, value)
            dev[key][idx] = old
        del dev, rfwd, rgrads
    return st


# --------------------------------------------------------------------------
# large element counts, whole arrays
# --------------------------------------------------------------------------

LARGE_E = (98_304, 100_007, 1_000_003)


def large_cases(seed: int, sizes: Sequence[int] = LARGE_E) -> List[AGCase]:
    rng = random.Random(seed + 11)
    out = []
    for E in sizes:
        for kind, b in (("grad", 1), ("div", 1), ("fm", 9)):
            c = D.DGCase(kind, 35, 15, b, "rij", "float64", E, "large", rng.randrange(1 << 30))
            out.append(AGCase(c, None, "auto"))
    out.append(AGCase(D.DGCase("grad", 35, 15, 1, "rij", "float32", 100_003, "large", rng.randrange(1 << 30)), None,
                      "auto"))
    if tuple(sizes) == LARGE_E:      # past the slice cap of fe_opgrad_plan (64 x 1023 elements): the operator-gradient kernels
        for kind, b, op in (("grad", 1, "rij"), ("div", 1, "rij"), ("fm", 9, "rij"), ("grad", 1, "rji"), ("fm_jfi", 9, "rij"),
                            ("fm_fji", 2, "rij")):
            c = D.DGCase(kind, 35, 15, b, op, "float64", MULTI_TRIP_E, "large", rng.randrange(1 << 30))
            out.append(AGCase(c, None, "auto", operator_gradients="kernel"))
    return out


def device_data(torch, case: AGCase):
    """Exact data made on the device: ``(tensors by name, scales)`` (mantissas are recovered from the values for the
    slice checks: ``x * 2**-s`` is exact)."""
    rng = np.random.default_rng(case.seed)
    bits, scales, dtypes, _ = plan_data(case, rng)
    expr = case.expr()
    gen = torch.Generator(device=DEVICE).manual_seed(case.seed)
    shapes = {nm: _shape(expr, nm, case.E) for nm in expr.all_args}
    oshape = tuple(case.E if isinstance(d, f.SizeParam) else int(d) for d in expr.shape)
    shapes.update({g: oshape for g in grad_names(expr, case.drop)})
    dev = {}
    for k in sorted(shapes):
        top = (1 << bits[k]) - 1
        m = torch.randint(-top, top + 1, shapes[k], dtype=torch.int64, device=DEVICE, generator=gen)
        x = m.to(torch.float64) * math.ldexp(1.0, scales[k])
        dev[k] = x.to(getattr(torch, dtypes[k].name))
        del m, x
    return dev, scales


def run_large(seed: int, sizes: Sequence[int] = LARGE_E) -> Stats:
    import torch

    st = Stats(f"autograd large seed={seed}")
    for case in large_cases(seed, sizes):
        dev, scales = device_data(torch, case)
        rfwd, rgrads = device_references(torch, case, dev)
        label = _label("large", case)
        _slice_checks(torch, st, label, case, dev, scales, rfwd, rgrads, np.random.default_rng(case.seed + 1))
        fwd, grads, delta = forward_backward(torch, case, dev)
        routes = _check_routes(st, label, case, delta)
        st.cov.update([f"large:{case.kind}", f"dtype:{case.dtype}", f"E:{case.E}"]
                      + [f"route:{r}" for r in dict.fromkeys(routes)]
                      + ([f"opgrad:large:{case.kind}:E{case.E}"] if any(r in OPGRAD_ROUTES for r in routes) else [])
                      + (["route:facemass_j:b>8"] if "facemass_j" in routes and case.expr().b > 8 else []))
        _compare(st, label, case, fwd, grads, rfwd, rgrads)
        del dev, rfwd, rgrads, fwd, grads
        torch.cuda.empty_cache()
    return st


# --------------------------------------------------------------------------
# the adjoint kernels, called directly
# --------------------------------------------------------------------------

#: geomadj's output layouts: name -> (X, R) allowed, einsum output letters
GEOM_LAYOUTS = {"xre": None, "re": 1, "er": 1, "e": 1}
FM_LAYOUT_FLAGS = [(jl, rl, (FM_J_FE if jl == "fe" else 0) | {"fij": 0, "ifj": FM_R_IFJ, "fji": FM_R_T,
                                                              "jfi": FM_R_IFJ | FM_R_T}[rl])
                   for jl in ("ef", "fe") for rl in ("fij", "ifj", "fji", "jfi")]
KERNEL_E = (1, 15, 16, 17, 1003)


def geomadj_runs(seed: int) -> List[Tuple[int, int, int, int, str, int, int]]:
    """``(Np, X, R, op_flags, layout, E, seed)``: every compiled Np x (X, R) x operator layout x J layout, one E each
    from :data:`KERNEL_E`, and a multi-trip E for one combination per Np."""
    rng = random.Random(seed + 19)
    out = []
    for Np in GEOMADJ_NP:
        for lay in GEOM_LAYOUTS:
            xs = (1, 2, 3) if lay == "xre" else (1,)
            rs = (1,) if lay == "e" else (1, 2, 3)
            for X in xs:
                for R in rs:
                    for op in (0, OP_TRANSPOSED):
                        out.append((Np, X, R, op, lay, rng.choice(KERNEL_E), rng.randrange(1 << 30)))
        out.append((Np, 3, 3, rng.choice((0, OP_TRANSPOSED)), "xre", MULTI_TRIP_E, rng.randrange(1 << 30)))
    return out


def facemass_runs(seed: int) -> List[Tuple[Tuple[int, int, int], Tuple[str, str, int], int, str, int, int]]:
    """``((nf, Np, Nfp), (J layout, R layout, flags), b, outputs, E, seed)``: every compiled shape x layout x b in
    {1, 8, 9, 17} x {dv, dJ, both}, one E each from :data:`KERNEL_E`; a multi-trip E for one combination per shape."""
    rng = random.Random(seed + 23)
    out = []
    for shape in FACEMASS_ADJ_SHAPES:
        for lay in FM_LAYOUT_FLAGS:
            for b in (1, 8, 9, 17):
                for what in ("dv", "dJ", "both"):
                    out.append((shape, lay, b, what, rng.choice(KERNEL_E), rng.randrange(1 << 30)))
        out.append((shape, rng.choice(FM_LAYOUT_FLAGS), 9 if shape == (4, 35, 15) else 2, "both", MULTI_TRIP_E,
                    rng.randrange(1 << 30)))
    return out


def geomadj_reference(mD, ma, mb, op: int, layout: str) -> np.ndarray:
    K = np.swapaxes(mD, 1, 2) if op & OP_TRANSPOSED else mD
    out = _int_einsum("rij,ej,xei->xre", [K, ma, mb])
    if layout == "xre":
        return out
    if layout == "re":
        return out[0]
    if layout == "er":
        return np.ascontiguousarray(out[0].T)
    return out[0, 0]


def _r_shape(rl: str, nf: int, Np: int, Nfp: int) -> Tuple[int, int, int]:
    return {"fij": (nf, Np, Nfp), "ifj": (Np, nf, Nfp), "fji": (nf, Nfp, Np), "jfi": (Nfp, nf, Np)}[rl]


def _r_fij(mR: np.ndarray, rl: str) -> np.ndarray:
    """R in (f, i, j) order from its stored layout."""
    return {"fij": lambda a: a, "ifj": lambda a: a.transpose(1, 0, 2), "fji": lambda a: a.transpose(0, 2, 1),
            "jfi": lambda a: a.transpose(1, 2, 0)}[rl](mR)


def facemass_references(mJ, mR, mg, mv, jl: str, rl: str):
    """``(dv_k list, dJ)`` in int64: dv_k[f, e, j] = J[e, f] sum_i R[f, i, j] g_k[e, i]; dJ = sum_k sum_j (sum_i R[f, i,
    j] g_k[e, i]) v_k[f, e, j] in J's layout."""
    R = _r_fij(mR, rl)
    Jef = mJ if jl == "ef" else mJ.T
    dv = [_int_einsum("ef,fij,ei->fej", [Jef, R, g]) for g in mg]
    dJ = None
    if mv is not None:
        dJ = sum(_int_einsum("fij,ei,fej->ef", [R, g, v]) for g, v in zip(mg, mv))
        dJ = dJ if jl == "ef" else np.ascontiguousarray(dJ.T)
    return dv, dJ


def _exact(rng: np.random.Generator, shapes: Dict[str, Tuple[int, ...]], rows, sig: int = 53):
    bits = ref_.shared_exact_bits(rows, [], sig, rng)
    m, x = {}, {}
    for k in sorted(shapes):
        mm, xx = ref_.exact_operands([shapes[k]], [np.float64], [bits[k]], [0], rng)
        m[k], x[k] = mm[0], xx[0]
    return m, x


KERNEL_PLACEMENTS = ("aligned", "all", "only:geometry", "only:operator", "only:field", "only:last-field", "only:output",
                     "only:last-output")


def kernel_shifts(placement: Optional[str], ins: Sequence[Tuple[str, str]], outs: Sequence[str]) -> Dict[str, int]:
    """Shift in elements (float64: 8 bytes) per array of a direct kernel call: *ins* ``(name, role)`` with role
    "geometry", "operator" or "field", *outs* the output names (tools/fuzz_dg.py: placements)."""
    assert placement is None or placement in KERNEL_PLACEMENTS, placement
    names = [n for n, _ in ins] + list(outs)
    fields = [n for n, r in ins if r == "field"]
    hit = {None: [], "aligned": [], "all": names,
           "only:geometry": [n for n, r in ins if r == "geometry"], "only:operator": [n for n, r in ins if r == "operator"],
           "only:field": fields[:1], "only:last-field": fields[-1:], "only:output": list(outs[:1]),
           "only:last-output": list(outs[-1:])}[placement]
    return {n: int(n in hit) for n in names}


class _KernelArrays:
    """The device arrays of one direct kernel call.  Without a placement: inputs from the allocator, outputs between
    guard bands.  With one: every array embedded by ``fuzz_dg.embed`` (inputs between NaN bands and snapshotted,
    outputs between sentinel bands) at its shift."""

    def __init__(self, torch, placement: Optional[str], x: Dict[str, np.ndarray], ins: Sequence[Tuple[str, str]],
                 outs: Dict[str, Tuple[int, ...]]) -> None:
        self.placement = placement
        self.out: Dict[str, Any] = {}
        if placement is None:
            self.d = _to_dev(torch, x)
            self._bufs = []
            for name, shape in outs.items():
                buf, out, nn = _guarded(torch, shape, torch.float64)
                self._bufs.append((buf, nn))
                self.out[name] = out
            return
        shifts = {"ws": 0, **kernel_shifts(placement, ins, [n for n in outs if n != "ws"])}     # (a workspace must be 256-byte aligned)
        self._ins = {}
        for name, _ in ins:
            emb = D.embed(torch, x[name].shape, torch.float64, shifts[name], "in", torch.from_numpy(x[name]), DEVICE)
            self._ins[name] = (emb, emb.snapshot())
        self.d = {name: emb.view for name, (emb, _) in self._ins.items()}
        self._outs = {name: D.embed(torch, shape, torch.float64, shifts[name], "out", device=DEVICE)
                      for name, shape in outs.items()}
        self.out = {name: emb.view for name, emb in self._outs.items()}

    def guards_intact(self) -> bool:
        if self.placement is None:
            return all(_guards_intact(buf, nn) for buf, nn in self._bufs)
        return all(emb.guards_intact() for emb in self._outs.values())

    def changed_inputs(self) -> List[str]:
        if self.placement is None:
            return []
        return [name for name, (emb, snap) in self._ins.items() if not emb.unchanged(snap)]


def _kernel_checks(st: Stats, label: str, arrays: _KernelArrays, got) -> None:
    """Guards, inputs unchanged, then every ``(name, output, int64 reference)`` of *got*: NaNs the reference does not
    have (``leak:``), bitwise equality."""
    import torch

    if not arrays.guards_intact():
        st.fail(f"{label}: wrote outside its outputs")
        return
    for name in arrays.changed_inputs():
        st.fail(f"{label}: input {name} changed by the launch")
    for name, g, w in got:
        want = torch.from_numpy(w.astype(np.float64)).to(DEVICE)
        st.exact_runs += 1
        _, leaked = D.nan_entries(g, want)
        if leaked:
            st.cov["leak:nan-entries"] += leaked
            st.fail(f"{label}: {name}: over-read: {leaked} NaN entries from behind an input")
        bad = ref_.differing_entries(g, want)
        if bad:
            st.fail(f"{label}: {name}: {bad} entries differ from the exact result")
        else:
            st.exact_equal += 1


OPGRAD_E = KERNEL_E + (65, 66)      # 65: the smallest E with two slices (fe_opgrad_plan)
OPGRAD_OUT_LAYOUTS = ("rpq", "rqp")


def opgrad_runs(seed: int) -> List[Tuple[int, int, int, str, str, int, int, int]]:
    """``(Np, X, R, J layout, output layout, fields, E, seed)`` of direct ``fe_opgrad_f64`` calls: every compiled Np x
    J layout ("xre", "re", "er", "e") x output layout, (X, R) and one or two fields in turn, E from :data:`OPGRAD_E`."""
    rng = random.Random(seed + 67)
    out = []
    k = 0
    for Np in GEOMADJ_NP:
        for lay in GEOM_LAYOUTS:
            for ol in OPGRAD_OUT_LAYOUTS:
                X = (1, 2, 3)[k % 3] if lay == "xre" else 1
                R = 1 if lay == "e" else (3, 1, 2)[(k // 2) % 3]
                out.append((Np, X, R, lay, ol, 1 + k % 2, OPGRAD_E[(k + k // 7) % len(OPGRAD_E)], rng.randrange(1 << 30)))
                k += 1
    return out


def facemass_opgrad_runs(seed: int) -> List[Tuple[Tuple[int, int, int], Tuple[str, str, int], int, int, int]]:
    """``((nf, Np, Nfp), (J layout, R layout, flags), b, E, seed)`` of direct ``fe_facemass_opgrad_f64`` calls: every
    compiled shape x the eight flag combinations, b in {1, 2, 4, 9} in turn (9: a second launch adding to its own
    slice), E from :data:`OPGRAD_E`."""
    rng = random.Random(seed + 71)
    out = []
    k = 0
    for shape in FACEMASS_ADJ_SHAPES:
        for lay in FM_LAYOUT_FLAGS:
            out.append((shape, lay, (1, 2, 4, 9)[(k + k // 8) % 4], OPGRAD_E[(k + k // 7) % len(OPGRAD_E)], rng.randrange(1 << 30)))
            k += 1
    return out


def placement_opgrad_runs(seed: int):
    """``(opgrad runs, facemass opgrad runs)`` of the placement pass: every J layout x output layout at four of the
    compiled Np, and every flag combination of face-mass at p = 1 and p = 4 of the tetrahedra."""
    og = [r for r in opgrad_runs(seed) if r[0] in (4, 10, 21, 35)]
    fm = [r for r in facemass_opgrad_runs(seed) if r[0] in ((4, 4, 3), (4, 35, 15))]
    return og, fm


_OPGRAD_J = {"xre": (lambda X, R, E: (X, R, E), lambda R, E: (R * E, E, 1)), "re": (lambda X, R, E: (R, E), lambda R, E: (0, E, 1)),
             "er": (lambda X, R, E: (E, R), lambda R, E: (0, 1, R)), "e": (lambda X, R, E: (E,), lambda R, E: (0, 0, 1))}
_FM_PERM = {"fij": (0, 1, 2), "ifj": (1, 0, 2), "fji": (0, 2, 1), "jfi": (2, 0, 1)}     # dR [f][i][j] in R's stored layout


def opgrad_reference(mJ, ma, mb, layout: str, ol: str) -> np.ndarray:
    """``out[r, p, q] = sum_k sum_e (sum_x J[x, r, e] b_k[x, e, p]) a_k[e, q]`` in int64, in the output's stored layout."""
    J = {"xre": lambda j: j, "re": lambda j: j[None], "er": lambda j: j.T[None], "e": lambda j: j[None, None]}[layout](mJ)
    out = sum(_int_einsum("xre,eq,xep->rpq", [J, a, b]) for a, b in zip(ma, mb))
    return out if ol == "rpq" else np.ascontiguousarray(out.transpose(0, 2, 1))


def facemass_opgrad_reference(mJ, mg, mv, jl: str, rl: str) -> np.ndarray:
    Jef = mJ if jl == "ef" else mJ.T
    out = sum(_int_einsum("ei,ef,fej->fij", [g, Jef, v]) for g, v in zip(mg, mv))
    return np.ascontiguousarray(out.transpose(_FM_PERM[rl]))


def _with_workspace(outs: Dict[str, Tuple[int, ...]], E: int, entries: int) -> Tuple[Dict[str, Tuple[int, ...]], int]:
    """The outputs of an operator-gradient call plus its workspace of exactly the planned bytes (``fe_opgrad_plan``):
    embedded like an output, so a write behind the planned bytes lands in a guard band; the library asks for a 256-byte
    aligned workspace, so it is never shifted."""
    from feinsum_amd import _hip

    nbytes = _hip.opgrad_plan(E, entries)[1]
    assert nbytes % 8 == 0
    return ({**outs, "ws": (nbytes // 8,)} if nbytes else dict(outs)), nbytes


def placement_kernel_runs(seed: int):
    """``(geomadj runs, facemass runs)`` of the placement pass: a subset of :func:`geomadj_runs` (every Np, output
    layout and operator layout; every (X, R) of "xre") and face-mass runs of every compiled shape and layout with b
    in {1, 2, 4} and one b = 9 (two launch groups), at the E of :data:`KERNEL_E`."""
    rng = random.Random(seed + 37)
    geom, combos, xr = [], set(), set()
    for run in geomadj_runs(seed):
        Np, X, R, op, lay, E, _ = run
        if E != MULTI_TRIP_E and ((Np, lay, op) not in combos or (lay == "xre" and (X, R) not in xr)):
            combos.add((Np, lay, op))
            xr.update({(X, R)} if lay == "xre" else ())
            geom.append(run)
    fm = []
    for shape in FACEMASS_ADJ_SHAPES:
        for k, lay in enumerate(FM_LAYOUT_FLAGS):
            b = (1, 2, 4)[(k + len(fm)) % 3]
            fm.append((shape, lay, b, ("both", "dv", "dJ")[k % 3], rng.choice(KERNEL_E), rng.randrange(1 << 30)))
        fm.append((shape, rng.choice(FM_LAYOUT_FLAGS), 9, "both", rng.choice(KERNEL_E), rng.randrange(1 << 30)))
    return geom, fm


def run_kernels(seed: int, geom_runs=None, fm_runs=None, placement: Optional[str] = None, og_runs=None,
                ogfm_runs=None) -> Stats:
    """Every :func:`geomadj_runs` / :func:`facemass_runs` combination through ``_hip.geomadj`` /
    ``_hip.facemass_adj``, and every :func:`opgrad_runs` / :func:`facemass_opgrad_runs` combination through
    ``_hip.opgrad`` / ``_hip.facemass_opgrad`` (the workspace an output of exactly the planned bytes),
    exact data (scale 1), outputs in NaN-filled buffers between guard bands.  With *placement*
    (:data:`KERNEL_PLACEMENTS`) every array sits at that placement's address offset between bands
    (:class:`_KernelArrays`), and the inputs must come back unchanged."""
    import torch

    from feinsum_amd import _hip

    st = Stats(f"adjoint kernels seed={seed}" + (f" {placement}" if placement else ""))
    if placement:
        st.cov["leak:nan-entries"] += 0
    tag = f" [{placement}]" if placement else ""
    for Np, X, R, op, lay, E, s in (geomadj_runs(seed) if geom_runs is None else geom_runs):
        rng = np.random.default_rng(s)
        m, x = _exact(rng, {"D": (R, Np, Np), "a": (E, Np), "b": (X, E, Np)}, [(["D", "a", "b"], Np * Np)])
        shape = {"xre": (X, R, E), "re": (R, E), "er": (E, R), "e": (E,)}[lay]
        strides = {"xre": (R * E, E, 1), "re": (0, E, 1), "er": (0, 1, R), "e": (0, 0, 1)}[lay]
        arrays = _KernelArrays(torch, placement, x, [("D", "operator"), ("a", "field"), ("b", "field")], {"out": shape})
        d, out = arrays.d, arrays.out["out"]
        _hip.geomadj(d["D"].data_ptr(), d["a"].data_ptr(), d["b"].data_ptr(), out.data_ptr(), E, X, R, Np, strides,
                     op_flags=op)
        torch.cuda.synchronize()
        label = f"geomadj Np={Np} X={X} R={R} op={op} {lay} E={E} seed={s}{tag}"
        st.cov.update([f"geomadj:Np{Np}", f"geomadj:{lay}", f"geomadj:op{op}", f"geomadj:X{X}R{R}",
                       f"E:{'multi-trip' if E == MULTI_TRIP_E else E}"] + ([f"place:{placement}"] if placement else []))
        _kernel_checks(st, label, arrays, [("out", out, geomadj_reference(m["D"], m["a"], m["b"], op, lay))])
    for (nf, Np, Nfp), (jl, rl, flags), b, what, E, s in (facemass_runs(seed) if fm_runs is None else fm_runs):
        rng = np.random.default_rng(s)
        shapes = {"J": (E, nf) if jl == "ef" else (nf, E), "R": _r_shape(rl, nf, Np, Nfp)}
        rows = []
        for k in range(b):
            shapes[f"g{k}"] = (E, Np)
            shapes[f"v{k}"] = (nf, E, Nfp)
            rows += [(["J", "R", f"g{k}"], Np), (["R", f"g{k}", f"v{k}"], b * Np * Nfp)]
        m, x = _exact(rng, shapes, rows)
        with_dv, with_dJ = what in ("dv", "both"), what in ("dJ", "both")
        dv_want, dJ_want = facemass_references(m["J"], m["R"], [m[f"g{k}"] for k in range(b)],
                                               [m[f"v{k}"] for k in range(b)] if with_dJ else None, jl, rl)
        ins = [("J", "geometry"), ("R", "operator")] + [(f"g{k}", "field") for k in range(b)] + \
              ([(f"v{k}", "field") for k in range(b)] if with_dJ else [])
        outs = {**({f"dv{k}": (nf, E, Nfp) for k in range(b)} if with_dv else {}), **({"dJ": shapes["J"]} if with_dJ else {})}
        arrays = _KernelArrays(torch, placement, x, ins, outs)
        d = arrays.d
        dvs = [arrays.out[f"dv{k}"] for k in range(b)] if with_dv else []
        dJ = arrays.out["dJ"] if with_dJ else None
        _hip.facemass_adj(d["J"].data_ptr(), d["R"].data_ptr(), [d[f"g{k}"].data_ptr() for k in range(b)],
                          [d[f"v{k}"].data_ptr() for k in range(b)] if with_dJ else None,
                          [t.data_ptr() for t in dvs] if with_dv else None,
                          dJ.data_ptr() if with_dJ else None, E, Np, nf, Nfp, layout_flags=flags)
        torch.cuda.synchronize()
        label = f"facemass_adj (nf, Np, Nfp)=({nf}, {Np}, {Nfp}) {jl},{rl} b={b} {what} E={E} seed={s}{tag}"
        st.cov.update([f"facemass_adj:Np{Np}", f"facemass_adj:{jl},{rl}", f"facemass_adj:b{b}",
                       f"facemass_adj:{what}", f"E:{'multi-trip' if E == MULTI_TRIP_E else E}"]
                      + ([f"place:{placement}"] if placement else []))
        _kernel_checks(st, label, arrays, ([(f"dv{k}", dvs[k], dv_want[k]) for k in range(b)] if with_dv else []) +
                       ([("dJ", dJ, dJ_want)] if with_dJ else []))
    for Np, X, R, lay, ol, nk, E, s in (opgrad_runs(seed) if og_runs is None else og_runs):
        rng = np.random.default_rng(s)
        shapes = {"J": _OPGRAD_J[lay][0](X, R, E)}
        for k in range(nk):
            shapes[f"a{k}"], shapes[f"b{k}"] = (E, Np), (X, E, Np)
        m, x = _exact(rng, shapes, [(["J", f"a{k}", f"b{k}"], E * X * nk) for k in range(nk)])
        outs, nbytes = _with_workspace({"out": (R, Np, Np)}, E, R * Np * Np)
        ins = [("J", "geometry")] + [(f"a{k}", "field") for k in range(nk)] + [(f"b{k}", "field") for k in range(nk)]
        arrays = _KernelArrays(torch, placement, x, ins, outs)
        d, out = arrays.d, arrays.out["out"]
        _hip.opgrad(d["J"].data_ptr(), [d[f"a{k}"].data_ptr() for k in range(nk)], [d[f"b{k}"].data_ptr() for k in range(nk)],
                    out.data_ptr(), E, X, R, Np, _OPGRAD_J[lay][1](R, E), (Np * Np, Np, 1) if ol == "rpq" else (Np * Np, 1, Np),
                    arrays.out["ws"].data_ptr() if nbytes else None, nbytes)
        torch.cuda.synchronize()
        label = f"opgrad Np={Np} X={X} R={R} {lay} {ol} fields={nk} E={E} seed={s}{tag}"
        st.cov.update([f"opgrad:Np{Np}", f"opgrad:{lay}", f"opgrad:{ol}", f"opgrad:{lay},{ol}", f"opgrad:E{E}"]
                      + (["opgrad:workspace"] if nbytes else []) + ([f"place:{placement}"] if placement else []))
        want = opgrad_reference(m["J"], [m[f"a{k}"] for k in range(nk)], [m[f"b{k}"] for k in range(nk)], lay, ol)
        _kernel_checks(st, label, arrays, [("out", out, want)])
    for (nf, Np, Nfp), (jl, rl, flags), b, E, s in (facemass_opgrad_runs(seed) if ogfm_runs is None else ogfm_runs):
        rng = np.random.default_rng(s)
        shapes = {"J": (E, nf) if jl == "ef" else (nf, E)}
        for k in range(b):
            shapes[f"g{k}"], shapes[f"v{k}"] = (E, Np), (nf, E, Nfp)
        m, x = _exact(rng, shapes, [(["J", f"g{k}", f"v{k}"], E * b) for k in range(b)])
        outs, nbytes = _with_workspace({"dR": _r_shape(rl, nf, Np, Nfp)}, E, nf * Np * Nfp)
        ins = [("J", "geometry")] + [(f"g{k}", "field") for k in range(b)] + [(f"v{k}", "field") for k in range(b)]
        arrays = _KernelArrays(torch, placement, x, ins, outs)
        d, dR = arrays.d, arrays.out["dR"]
        _hip.facemass_opgrad(d["J"].data_ptr(), [d[f"g{k}"].data_ptr() for k in range(b)], [d[f"v{k}"].data_ptr() for k in range(b)],
                             dR.data_ptr(), E, Np, nf, Nfp, arrays.out["ws"].data_ptr() if nbytes else None, nbytes,
                             layout_flags=flags)
        torch.cuda.synchronize()
        label = f"facemass_opgrad (nf, Np, Nfp)=({nf}, {Np}, {Nfp}) {jl},{rl} b={b} E={E} seed={s}{tag}"
        st.cov.update([f"opgrad_fm:Np{Np}", f"opgrad_fm:{jl},{rl}", f"opgrad_fm:b{b}", f"opgrad:E{E}"]
                      + (["opgrad:workspace"] if nbytes else []) + ([f"place:{placement}"] if placement else []))
        want = facemass_opgrad_reference(m["J"], [m[f"g{k}"] for k in range(b)], [m[f"v{k}"] for k in range(b)], jl, rl)
        _kernel_checks(st, label, arrays, [("dR", dR, want)])
    return st


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--repro":
        import torch

        st = Stats("repro")
        c = AGCase.from_repro(sys.argv[2])
        dev, rfwd, rgrads = _prepare(torch, c, st)
        fwd, grads, delta = forward_backward(torch, c, dev)
        _check_routes(st, "repro", c, delta)
        _compare(st, "repro", c, fwd, grads, rfwd, rgrads)
        print(st.report())
        sys.exit(1 if st.failures else 0)
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 80
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else 0
    results = [run_exact(n, seed), run_bounded(n // 2, seed), run_nonfinite(n // 4, seed), run_large(seed),
               run_kernels(seed)]
    for s in results:
        print(s.report())
    sys.exit(1 if sum(s.failures for s in results) else 0)
