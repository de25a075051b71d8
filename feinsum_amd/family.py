"""
Recognise which hand-written kernel family a :class:`BatchedEinsum` belongs to.

This is the build's replacement for the reference's canonicalisation +
transform-archive lookup (reference: ``src/feinsum/canonicalization.py:1087``
``canonicalize_einsum`` and ``src/feinsum/sql_utils.py:160-294``
``query``/``retrieve``): instead of a graph canonical form keyed into sqlite, a
short table of templates is matched up to (a) renaming of indices and (b)
order of the operands.  Axis order inside an operand and inside the output is
memory layout and must match the template exactly.

Families: grad ``xre,rij,ej->xei``; div ``xre,rij,xej->ei``;
face-mass ``ef,fij,fej->ei`` with its layout siblings (J as ``fe``, operator as
``ifj`` -- ``tuning/impls/ifj_fe_fej_to_ei.py:46-60``), and the transposed-operator
siblings of all three (``rji``: ``tuning/impls/xre_rji_xej_to_ei_v1.py``; ``fji`` /
``jfi``: ``tuning/impls/jfi_fe_fej_to_ei.py:46-56``); the div component
``re,rij,ej->ei`` of ``test/test_codegen.py:34-66`` (batched over the three components);
the element-local operator ``e,ij,ej->ei`` / ``ij,ej->ei``
(``tuning/impls/e_ij_ej_to_ei_no_prftch.py``, ``ij_ej_to_ei_no_prftch.py``).
Anything else is evaluated by the generic einsum kernel.
"""

from __future__ import annotations

from dataclasses import dataclass
from itertools import permutations
from typing import Dict, Iterator, Optional, Tuple

import numpy as np

from feinsum_amd.einsum import BatchedEinsum, SizeParam

FAMILY_GRAD, FAMILY_DIV, FAMILY_GRADDIV, FAMILY_FACEMASS, FAMILY_DIVCOMP, FAMILY_GRADPLANES = 1, 2, 3, 4, 5, 6
FAMILY_MATAPPLY = 7
FM_J_FE, FM_R_IFJ, FM_R_T = 1, 2, 4
OP_TRANSPOSED, OP_J_ES = 1, 2

# (family, layout_flags, subscripts, roles of the operands in template order)
_TEMPLATES = (
    (FAMILY_GRAD, 0, "xre,rij,ej->xei", ("J", "D", "u")),
    (FAMILY_GRAD, OP_TRANSPOSED, "xre,rji,ej->xei", ("J", "D", "u")),
    (FAMILY_DIV, 0, "xre,rij,xej->ei", ("J", "D", "u")),
    (FAMILY_DIV, OP_TRANSPOSED, "xre,rji,xej->ei", ("J", "D", "u")),     # xre_rji_xej_to_ei_v{0,1}.py
    # div components: test/test_codegen.py:34-66, re_rij_ej_to_ei.py, re_rji_ej_to_ei_*.py
    (FAMILY_DIVCOMP, 0, "re,rij,ej->ei", ("J", "D", "u")),
    (FAMILY_DIVCOMP, OP_TRANSPOSED, "re,rji,ej->ei", ("J", "D", "u")),
    (FAMILY_DIVCOMP, OP_J_ES, "er,rij,ej->ei", ("J", "D", "u")),        # examples/dg_wave_div.py
    (FAMILY_DIVCOMP, OP_J_ES | OP_TRANSPOSED, "er,rji,ej->ei", ("J", "D", "u")),
    # element-local operator with / without a per-element factor:
    # tuning/impls/e_ij_ej_to_ei_no_prftch.py:30-38, ij_ej_to_ei_no_prftch.py
    (FAMILY_MATAPPLY, 0, "e,ij,ej->ei", ("J", "D", "u")),
    (FAMILY_MATAPPLY, OP_TRANSPOSED, "e,ji,ej->ei", ("J", "D", "u")),
    (FAMILY_MATAPPLY, 0, "ij,ej->ei", ("D", "u")),
    (FAMILY_MATAPPLY, OP_TRANSPOSED, "ji,ej->ei", ("D", "u")),
) + tuple(
    (FAMILY_FACEMASS, jflag | rflag, f"{jsub},{rsub},fej->ei", ("J", "R", "v"))
    for jflag, jsub in ((0, "ef"), (FM_J_FE, "fe"))
    for rflag, rsub in ((0, "fij"), (FM_R_IFJ, "ifj"), (FM_R_T, "fji"), (FM_R_IFJ | FM_R_T, "jfi"))  # jfi_fe_fej_to_ei.py
)


@dataclass(frozen=True)
class KernelPlan:
    """How to evaluate an einsum with the HIP library.

    ``roles[k]`` maps a role (``"J"``, ``"D"``/``"R"``, ``"u"``/``"v"``) to the
    operand *position* in row k of ``einsum.args``; ``long_index`` is the einsum's
    own letter of the element axis; ``params`` holds Np / nf / Nfp.
    """

    family: int
    layout_flags: int
    roles: Dict[str, int]
    long_index: str
    params: Dict[str, int]

    @property
    def name(self) -> str:
        return {FAMILY_GRAD: "grad", FAMILY_DIV: "div", FAMILY_FACEMASS: "facemass",
                FAMILY_DIVCOMP: "divcomp", FAMILY_MATAPPLY: "matapply"}[self.family]


def _match_template(einsum: BatchedEinsum, subscripts: str) -> Optional[Tuple[Tuple[int, ...], Dict[str, str]]]:
    return next(_template_matches(einsum, subscripts), None)


def _template_matches(einsum: BatchedEinsum, subscripts: str) -> Iterator[Tuple[Tuple[int, ...], Dict[str, str]]]:
    """Every (operand order, letters) under which *einsum* is the template, in the order of ``itertools.permutations``."""
    lhs, rhs = subscripts.split("->")
    t_in = [tuple(s) for s in lhs.split(",")]
    t_out = tuple(rhs)
    if len(t_in) != einsum.n or len(t_out) != len(einsum.out_idx_set):
        return
    for perm in permutations(range(einsum.n)):
        # template operand k <-> einsum operand perm[k]
        mapping: Dict[str, str] = {}
        ok = True
        pairs = [(t_in[k], einsum.in_idx_sets[perm[k]]) for k in range(einsum.n)]
        pairs.append((t_out, einsum.out_idx_set))
        for t_idxs, e_idxs in pairs:
            if len(t_idxs) != len(e_idxs):
                ok = False
                break
            for t, e in zip(t_idxs, e_idxs):
                if mapping.setdefault(t, e) != e:
                    ok = False
                    break
            if not ok:
                break
        if ok and len(set(mapping.values())) == len(mapping) == len(einsum.all_indices):
            yield perm, mapping


def match_family(einsum: BatchedEinsum) -> Optional[KernelPlan]:
    """Return the :class:`KernelPlan` for *einsum*, or ``None`` if it is not a DG-family einsum."""
    dtypes = {np.dtype(dt) for dt in einsum.arg_to_dtype.values()}
    if dtypes not in ({np.dtype("float64")}, {np.dtype("float32")}):
        return None     # mixed or other element types: the generic einsum kernel (or none)
    is_f32 = dtypes == {np.dtype("float32")}
    for family, flags, subscripts, roles in _TEMPLATES:
        m = _match_template(einsum, subscripts)
        if m is None:
            continue
        perm, mapping = m
        dim = lambda t: einsum.index_to_dim_length[mapping[t]]  # noqa: E731
        long_dim = dim("e")
        fixed = [t for t in mapping if t != "e"]
        if any(isinstance(dim(t), SizeParam) for t in fixed):
            continue
        if family in (FAMILY_GRAD, FAMILY_DIV):
            # tetrahedra (ndim = 3) and triangles (ndim = 2)
            if int(dim("x")) not in (2, 3) or int(dim("r")) != int(dim("x")) or int(dim("i")) != int(dim("j")):
                continue
            params = {"Np": int(dim("i")), "ndim": int(dim("x"))}
        elif family == FAMILY_DIVCOMP:
            if int(dim("r")) not in (2, 3) or int(dim("i")) != int(dim("j")):
                continue
            params = {"Np": int(dim("i")), "ndim": int(dim("r"))}
        elif family == FAMILY_MATAPPLY:
            if int(dim("i")) != int(dim("j")):
                continue
            params = {"Np": int(dim("i"))}
        else:
            params = {"Np": int(dim("i")), "nf": int(dim("f")), "Nfp": int(dim("j"))}
        del long_dim
        if is_f32:
            params["f32"] = 1      # all-float32 operands: fe_launch_f32 (the LDS-tiled kernel in float)
        return KernelPlan(family, flags, {role: perm[k] for k, role in enumerate(roles)},
                          mapping["e"], params)
    return None


# --------------------------------------------------------------------------
# float32 fields in the float64 families: grad, div and face-mass of tetrahedra p = 1..4 whose fields
# are float32 while every J and every operator is float64.  Kept apart from match_family on purpose -- "auto" keeps its
# route for these einsums; only transform="mixed_family" reaches the kernels of csrc/fe_mixed.h.
# --------------------------------------------------------------------------

#: (Np, Nfp) of the tetrahedral orders p = 1..4 (nf = 4): the shapes fe_mixed.h is compiled for
MIXED_TET_SHAPES = ((4, 3), (10, 6), (20, 10), (35, 15))
MIXED_FAMILY_RULE = ("grad 'xre,rij,ej->xei', div 'xre,rij,xej->ei' (operator 'rij' or 'rji') or face-mass 'ef,fij,fej->ei' (its "
                     "eight J / R layouts) of tetrahedra p = 1..4 (Np = 4, 10, 20, 35; nf = 4, Nfp = 3, 6, 10, 15), every "
                     "field of every row float32, every J and every operator float64")


def match_mixed_family(einsum: BatchedEinsum) -> Optional[KernelPlan]:
    """The :class:`KernelPlan` (``params["fields_f32"] = 1``) of a DG einsum with float32 fields in float64 geometry
    factors and operators -- :data:`MIXED_FAMILY_RULE` -- else ``None``."""
    f32, f64 = np.dtype("float32"), np.dtype("float64")
    for family, flags, subscripts, roles in _TEMPLATES:
        if family not in (FAMILY_GRAD, FAMILY_DIV, FAMILY_FACEMASS):
            continue
        m = _match_template(einsum, subscripts)
        if m is None:
            continue
        perm, mapping = m
        dim = lambda t: einsum.index_to_dim_length[mapping[t]]  # noqa: E731
        if any(isinstance(dim(t), SizeParam) for t in mapping if t != "e"):
            continue
        role = {name: perm[k] for k, name in enumerate(roles)}
        field ="u" if "u" in role else "v"
        if not all(np.dtype(row[role[field]].dtype) == f32 and
                   all(np.dtype(row[p].dtype) == f64 for name, p in role.items() if name != field)
                   for row in einsum.args):
            continue
        if family == FAMILY_FACEMASS:
            if int(dim("f")) != 4 or (int(dim("i")), int(dim("j"))) not in MIXED_TET_SHAPES:
                continue
            params = {"Np": int(dim("i")), "nf": 4, "Nfp": int(dim("j"))}
        else:
            if (int(dim("x")), int(dim("r"))) != (3, 3) or int(dim("i")) != int(dim("j")) \
                    or int(dim("i")) not in [np_ for np_, _ in MIXED_TET_SHAPES]:
                continue
            params = {"Np": int(dim("i")), "ndim": 3}
        params["fields_f32"] = 1
        return KernelPlan(family, flags, role, mapping["e"], params)
    return None


# --------------------------------------------------------------------------
# adjoint-only shapes: the einsums that the gradients of the DG families need and that no forward
# family kernel covers.  Kept apart from match_family on purpose -- "auto" on a user-built einsum of one of these shapes
# keeps its kernel; only the autograd path and the "adjoint" transform reach these kernels.
# --------------------------------------------------------------------------

ADJ_GEOM, ADJ_FACEMASS_V, ADJ_FACEMASS_J = "geomadj", "facemass_v", "facemass_j"
GEOMADJ_NP = (3, 4, 6, 10, 15, 20, 21, 35)      # fe_geomadj_f64
FACEMASS_ADJ_SHAPES = ((4, 4, 3), (4, 10, 6), (4, 20, 10), (4, 35, 15),               # fe_facemass_adj_f64: (nf, Np, Nfp)
                       (3, 3, 2), (3, 6, 3), (3, 10, 4), (3, 15, 5), (3, 21, 6))

# geometric-factor adjoint  out[x, r, e] = sum_i (sum_j K[r, i, j] a[e, j]) b[x, e, i]  in J's layouts; the div family's
# J-adjoint ('rij,xej,ei->xre') is the grad template of the transposed operator up to operand order
_ADJ_TEMPLATES = tuple(
    (ADJ_GEOM, flag, f"{dsub},ej,{bsub}->{osub}", ("D", "a", "b"))
    for bsub, osub, dsubs in (("xei", "xre", ("rij", "rji")), ("ei", "re", ("rij", "rji")), ("ei", "er", ("rij", "rji")),
                              ("ei", "e", ("ij", "ji")))
    for flag, dsub in zip((0, OP_TRANSPOSED), dsubs)
) + tuple(
    (ADJ_FACEMASS_V, jflag | rflag, f"{jsub},{rsub},ei->fej", ("J", "R", "g"))
    for jflag, jsub in ((0, "ef"), (FM_J_FE, "fe"))
    for rflag, rsub in ((0, "fij"), (FM_R_IFJ, "ifj"), (FM_R_T, "fji"), (FM_R_IFJ | FM_R_T, "jfi"))
) + tuple(
    (ADJ_FACEMASS_J, jflag | rflag, f"{rsub},fej,ei->{jsub}", ("R", "v", "g"))
    for jflag, jsub in ((0, "ef"), (FM_J_FE, "fe"))
    for rflag, rsub in ((0, "fij"), (FM_R_IFJ, "ifj"), (FM_R_T, "fji"), (FM_R_IFJ | FM_R_T, "jfi"))
)


@dataclass(frozen=True)
class AdjointPlan:
    """How the adjoint kernels evaluate an einsum: ``kind`` (``ADJ_GEOM`` / ``ADJ_FACEMASS_V`` / ``ADJ_FACEMASS_J``),
    layout flags (``OP_TRANSPOSED``; ``FM_*``), ``roles`` (role -> operand position), the einsum's own letters of the
    template's indices (``letters``: template letter -> einsum letter) and ``params`` (Np, X, R / nf, Nfp)."""

    kind: str
    layout_flags: int
    roles: Dict[str, int]
    letters: Dict[str, str]
    params: Dict[str, int]

    @property
    def name(self) -> str:
        return self.kind


def match_adjoint_family(einsum: BatchedEinsum) -> Optional[AdjointPlan]:
    """The :class:`AdjointPlan` of an adjoint-only einsum of a DG family (float64, compiled shapes), else ``None``."""
    if {np.dtype(dt) for dt in einsum.arg_to_dtype.values()} != {np.dtype("float64")}:
        return None
    for kind, flags, subscripts, roles in _ADJ_TEMPLATES:
        m = _match_template(einsum, subscripts)
        if m is None:
            continue
        perm, mapping = m
        dim = lambda t: einsum.index_to_dim_length[mapping[t]]  # noqa: E731
        if any(isinstance(dim(t), SizeParam) for t in mapping if t != "e"):
            continue
        if kind == ADJ_GEOM:
            X = int(dim("x")) if "x" in mapping else 1
            R = int(dim("r")) if "r" in mapping else 1
            Np = int(dim("i"))
            if int(dim("j")) != Np or Np not in GEOMADJ_NP or not (1 <= X <= 3 and 1 <= R <= 3):
                continue
            params = {"Np": Np, "X": X, "R": R}
        else:
            shape = (int(dim("f")), int(dim("i")), int(dim("j")))
            if shape not in FACEMASS_ADJ_SHAPES:
                continue
            params = {"nf": shape[0], "Np": shape[1], "Nfp": shape[2]}
        return AdjointPlan(kind, flags, {role: perm[k] for k, role in enumerate(roles)}, dict(mapping), params)
    return None


# --------------------------------------------------------------------------
# operator gradients: the adjoint einsums of the DG families with respect to D / R.  A matcher of
# its own -- match_adjoint_family and "auto" do not know these shapes; only transform="operator_adjoint" and
# evaluate_differentiable(operator_gradients="kernel") reach the kernels of csrc/fe_opgrad.h.
# --------------------------------------------------------------------------

ADJ_OPERATOR_D, ADJ_OPERATOR_R = "opgrad_d", "opgrad_r"

# out[r, p, q] = sum_e (sum_x J[x, r, e] b[x, e, p]) a[e, q]: b carries the planes (grad: the output gradient, div: u).
# With X = 1 the two factors are alike, so 'rqp' is 'rpq' with a and b swapped and needs no template of its own.
_OPGRAD_TEMPLATES = tuple(
    (ADJ_OPERATOR_D, 0, sub, ("J", "a", "b"))
    for sub in ("xre,eq,xep->rpq", "xre,eq,xep->rqp", "re,eq,ep->rpq", "er,eq,ep->rpq", "e,eq,ep->pq")
) + tuple(
    (ADJ_OPERATOR_R, jflag | rflag, f"{jsub},fej,ei->{rsub}", ("J", "v", "g"))
    for jflag, jsub in ((0, "ef"), (FM_J_FE, "fe"))
    for rflag, rsub in ((0, "fij"), (FM_R_IFJ, "ifj"), (FM_R_T, "fji"), (FM_R_IFJ | FM_R_T, "jfi"))
)


def match_operator_adjoint(einsum: BatchedEinsum) -> Optional[AdjointPlan]:
    """The :class:`AdjointPlan` (kind ``ADJ_OPERATOR_D`` / ``ADJ_OPERATOR_R``) of an operator-gradient einsum of a DG
    family -- what ``adjoint_einsums(fwd, "D" / "R")`` builds, up to index renaming and operand order; float64, the
    compiled sizes of the adjoint kernels, all rows sharing J and no array used twice in a row -- else ``None``.
    ``params`` of an ``ADJ_OPERATOR_D`` plan: Np, X, R, ``jstrides`` (jx, jr, je in units of E: ``("E", k)`` / plain
    ints are resolved by :class:`~feinsum_amd.adjoint.AdjointLaunch`) and ``strides`` (sr, sp, sq) of
    ``out[r sr + p sp + q sq] = sum_e (sum_x J[x jx + r jr + e je] b[x, e, p]) a[e, q]``."""
    if {np.dtype(dt) for dt in einsum.arg_to_dtype.values()} != {np.dtype("float64")}:
        return None
    for kind, flags, subscripts, roles in _OPGRAD_TEMPLATES:
        m = _match_template(einsum, subscripts)
        if m is None:
            continue
        perm, mapping = m
        dim = lambda t: einsum.index_to_dim_length[mapping[t]]  # noqa: E731
        if any(isinstance(dim(t), SizeParam) for t in mapping if t != "e") or not isinstance(dim("e"), SizeParam):
            continue
        role = {name: perm[k] for k, name in enumerate(roles)}
        if len({row[role["J"]].name for row in einsum.args}) != 1:
            continue      # every row shares J
        if any(len({arg.name for arg in row}) != len(row) for row in einsum.args):
            continue      # an array used twice in one row: not an adjoint of a family einsum
        if kind == ADJ_OPERATOR_D:
            X = int(dim("x")) if "x" in mapping else 1
            R = int(dim("r")) if "r" in mapping else 1
            Np = int(dim("p"))
            if int(dim("q")) != Np or Np not in GEOMADJ_NP or not (1 <= X <= 3 and 1 <= R <= 3):
                continue
            lhs, rhs = subscripts.split("->")
            ext = {"x": X, "r": R, "p": Np, "q": Np}
            jst, acc = {}, (0, 1)         # J's strides as (multiples of E, plain): 'e' is the long axis
            for t in reversed(lhs.split(",")[0]):
                jst[t] = acc
                acc = (acc[1], 0) if t == "e" else (acc[0] * ext[t], acc[1] * ext[t])
            ost, n = {}, 1
            for t in reversed(rhs):
                ost[t] = n
                n *= ext[t]
            params = {"Np": Np, "X": X, "R": R,
                      "jstrides": tuple(jst.get(t, (0, 0)) for t in ("x", "r", "e")),
                      "strides": tuple(ost.get(t, 0) for t in ("r", "p", "q"))}
        else:
            shape = (int(dim("f")), int(dim("i")), int(dim("j")))
            if shape not in FACEMASS_ADJ_SHAPES:
                continue
            params = {"nf": shape[0], "Np": shape[1], "Nfp": shape[2]}
        return AdjointPlan(kind, flags, role, dict(mapping), params)
    return None


# --------------------------------------------------------------------------
# the element-local operator of any shape: 'ij,ej->ei' / 'e,ij,ej->ei' with Ni != Nj, and square
# sizes the MATAPPLY family has no matrix-core kernel for.  A matcher of its own -- match_family and "auto" are untouched;
# only transform="element_operator" reaches the kernel of csrc/fe_elemop.h.
# --------------------------------------------------------------------------

ELEMENT_OPERATOR_MAX_N = 96           # fe::kElemOpMaxN
ELEMENT_OPERATOR_MAX_FRAGMENTS = 64   # fe::kElemOpMaxFragments: the operator image, 512 bytes per fragment, stays within 32 KiB
ELEMENT_OPERATOR_RULE = ("the element-local operator 'ij,ej->ei' or 'e,ij,ej->ei' (operator 'ij' or 'ji'; up to index renaming and "
                         "operand order), every operand float64, fixed extents 1 <= Ni, Nj <= 96 with ceil(Ni / 16) * ceil(Nj / 4) "
                         "<= 64 (the operator's matrix-core image and four wave tiles fit half a CU's LDS)")

_ELEMENT_OPERATOR_TEMPLATES = (
    (0, "e,ij,ej->ei", ("J", "A", "u")),
    (OP_TRANSPOSED, "e,ji,ej->ei", ("J", "A", "u")),
    (0, "ij,ej->ei", ("A", "u")),
    (OP_TRANSPOSED, "ji,ej->ei", ("A", "u")),
)


def element_operator_supported(Ni: int, Nj: int) -> bool:
    """The size rule of ``fe_elemop_f64`` (``fe_elemop_supported`` in C says the same): a pure function of (Ni, Nj)."""
    Ni, Nj = int(Ni), int(Nj)
    return (1 <= Ni <= ELEMENT_OPERATOR_MAX_N and 1 <= Nj <= ELEMENT_OPERATOR_MAX_N
            and ((Ni + 15) // 16) * ((Nj + 3) // 4) <= ELEMENT_OPERATOR_MAX_FRAGMENTS)


@dataclass(frozen=True)
class ElementOperatorPlan:
    """How ``fe_elemop_f64`` evaluates an einsum: ``layout_flags`` (``OP_TRANSPOSED``), ``roles`` (``"J"`` -- three-operand
    forms only --, ``"A"``, ``"u"`` -> operand position), the einsum's letter of the element axis and ``params`` (Ni, Nj)."""

    layout_flags: int
    roles: Dict[str, int]
    long_index: str
    params: Dict[str, int]

    name = "element_operator"


def match_element_operator(einsum: BatchedEinsum) -> Optional[ElementOperatorPlan]:
    """The :class:`ElementOperatorPlan` of an element-local operator -- :data:`ELEMENT_OPERATOR_RULE` -- else ``None``."""
    if {np.dtype(dt) for dt in einsum.arg_to_dtype.values()} != {np.dtype("float64")}:
        return None
    for flags, subscripts, roles in _ELEMENT_OPERATOR_TEMPLATES:
        m = _match_template(einsum, subscripts)
        if m is None:
            continue
        perm, mapping = m
        dim = lambda t: einsum.index_to_dim_length[mapping[t]]  # noqa: E731
        if isinstance(dim("i"), SizeParam) or isinstance(dim("j"), SizeParam):
            continue
        if not element_operator_supported(int(dim("i")), int(dim("j"))):
            continue
        return ElementOperatorPlan(flags, {role: perm[k] for k, role in enumerate(roles)}, mapping["e"],
                                   {"Ni": int(dim("i")), "Nj": int(dim("j"))})
    return None


def element_operator_groups(plan: ElementOperatorPlan, einsum: BatchedEinsum) -> list:
    """The rows of each launch, as ``range`` objects: consecutive rows that share A (and J) -- the rule of
    ``measure._family_groups``; rows that share them without being neighbours launch separately."""
    role = plan.roles
    key = lambda row: (row[role["J"]].name if "J" in role else None, row[role["A"]].name)   # noqa: E731
    starts = [k for k, row in enumerate(einsum.args) if k == 0 or key(row) != key(einsum.args[k - 1])]
    return [range(k, k2) for k, k2 in zip(starts, starts[1:] + [len(einsum.args)])]


# --------------------------------------------------------------------------
# the weighted element operator: 'iq,eq,qj,ej->ei' -- interpolate to a quadrature grid, weigh every
# point of every element, project back -- in one launch.  A matcher of its own, like the one above: match_family and "auto"
# are untouched; only transform="weighted_element_operator" reaches the kernel of csrc/fe_weightedop.h.
# --------------------------------------------------------------------------

WO_P_T = 1   # FE_WO_P_T: P stored (Nq, Ni)
WO_A_T = 2   # FE_WO_A_T: A stored (Nj, Nq)
WEIGHTED_ELEMENT_OPERATOR_MAX_N = 48              # fe::kWtOpMaxN: Ni, Nj
WEIGHTED_ELEMENT_OPERATOR_MAX_Q = 64              # fe::kWtOpMaxQ: Nq
WEIGHTED_ELEMENT_OPERATOR_MAX_LDS = 80 * 1024     # fe::kWtOpMaxLds: two blocks per CU
WEIGHTED_ELEMENT_OPERATOR_RULE = (
    "the weighted element operator 'iq,eq,qj,ej->ei' (P 'iq' or 'qi', A 'qj' or 'jq'; up to index renaming and operand order), "
    "every operand float64, fixed extents 1 <= Ni, Nj <= 48 and 1 <= Nq <= 64 with 512 * (ceil(Nq / 16) * ceil(Nj / 4) + "
    "ceil(Ni / 16) * ceil(Nq / 4)) + 32 * even(max(16 * Nj + 2, 16 * Nq + 2, 16 * (Ni | 1))) <= 81920 (both operators' "
    "matrix-core images and four wave buffers fit half a CU's LDS)")

_WEIGHTED_ELEMENT_OPERATOR_TEMPLATES = (
    (0, "iq,eq,qj,ej->ei"),
    (WO_P_T, "qi,eq,qj,ej->ei"),
    (WO_A_T, "iq,eq,jq,ej->ei"),
    (WO_P_T | WO_A_T, "qi,eq,jq,ej->ei"),
)


def weighted_element_operator_lds_bytes(Ni: int, Nq: int, Nj: int) -> int:
    """Dynamic LDS of a block of ``fe_weightedop_f64`` (``fe::weightedop_lds_bytes``)."""
    buf = (max(16 * Nj + 2, 16 * Nq + 2, 16 * (Ni | 1)) + 1) & ~1
    return 8 * ((((Nq + 15) // 16) * ((Nj + 3) // 4) + ((Ni + 15) // 16) * ((Nq + 3) // 4)) * 64 + 4 * buf)


def weighted_element_operator_supported(Ni: int, Nq: int, Nj: int) -> bool:
    """The size rule of ``fe_weightedop_f64`` (``fe_weightedop_supported`` in C says the same): a pure function of
    (Ni, Nq, Nj)."""
    Ni, Nq, Nj = int(Ni), int(Nq), int(Nj)
    return (1 <= Ni <= WEIGHTED_ELEMENT_OPERATOR_MAX_N and 1 <= Nj <= WEIGHTED_ELEMENT_OPERATOR_MAX_N
            and 1 <= Nq <= WEIGHTED_ELEMENT_OPERATOR_MAX_Q
            and weighted_element_operator_lds_bytes(Ni, Nq, Nj) <= WEIGHTED_ELEMENT_OPERATOR_MAX_LDS)


@dataclass(frozen=True)
class WeightedElementOperatorPlan:
    """How ``fe_weightedop_f64`` evaluates an einsum: ``layout_flags`` (``WO_P_T | WO_A_T``), ``roles`` (``"P"``, ``"W"``,
    ``"A"``, ``"u"`` -> operand position), the einsum's letter of the element axis and ``params`` (Ni, Nq, Nj)."""

    layout_flags: int
    roles: Dict[str, int]
    long_index: str
    params: Dict[str, int]

    name = "weighted_element_operator"


def match_weighted_element_operator(einsum: BatchedEinsum) -> Optional[WeightedElementOperatorPlan]:
    """The :class:`WeightedElementOperatorPlan` of a weighted element operator -- :data:`WEIGHTED_ELEMENT_OPERATOR_RULE` --
    else ``None``.  P and A may be the same array (the Galerkin form ``qi,eq,qj,ej->ei``)."""
    if {np.dtype(dt) for dt in einsum.arg_to_dtype.values()} != {np.dtype("float64")}:
        return None
    for flags, subscripts in _WEIGHTED_ELEMENT_OPERATOR_TEMPLATES:
        m = _match_template(einsum, subscripts)
        if m is None:
            continue
        perm, mapping = m
        dim = lambda t: einsum.index_to_dim_length[mapping[t]]  # noqa: E731
        if any(isinstance(dim(t), SizeParam) for t in "iqj"):
            continue
        if not weighted_element_operator_supported(int(dim("i")), int(dim("q")), int(dim("j"))):
            continue
        return WeightedElementOperatorPlan(flags, {role: perm[k] for k, role in enumerate(("P", "W", "A", "u"))}, mapping["e"],
                                           {"Ni": int(dim("i")), "Nq": int(dim("q")), "Nj": int(dim("j"))})
    return None


def weighted_element_operator_groups(plan: WeightedElementOperatorPlan, einsum: BatchedEinsum) -> list:
    """The rows of each C call, as ``range`` objects: consecutive rows that share P, W and A -- the rule of
    :func:`element_operator_groups`; rows that share them without being neighbours are calls of their own.  (A call of more
    than 8 fields is split into kernel launches of at most 8 by the library.)"""
    role = plan.roles
    key = lambda row: (row[role["P"]].name, row[role["W"]].name, row[role["A"]].name)   # noqa: E731
    starts = [k for k, row in enumerate(einsum.args) if k == 0 or key(row) != key(einsum.args[k - 1])]
    return [range(k, k2) for k, k2 in zip(starts, starts[1:] + [len(einsum.args)])]


# --------------------------------------------------------------------------
# the weight gradient of the weighted element operator: 'iq,qj,ej,ei->eq', what
# adjoint_einsums(fwd, "W") builds.  A matcher of its own: match_family, match_adjoint_family, match_operator_adjoint, "auto"
# and transform="adjoint" are untouched; only evaluate_differentiable(element_gradients="kernel") reaches the kernel of
# csrc/fe_weightgrad.h.
# --------------------------------------------------------------------------

ADJ_WEIGHTED_W = "weighted_w"
WEIGHTED_WEIGHT_ADJOINT_MAX_FIELDS = 8           # fe::kMaxFields: the rows one call sums
WEIGHTED_WEIGHT_ADJOINT_RULE = (
    "the weight gradient of the weighted element operator, 'iq,qj,ej,ei->eq' (P 'iq' or 'qi', A 'qj' or 'jq'; up to index "
    "renaming and operand order), every operand float64, e a size parameter, all rows sharing P and A, fixed extents "
    "1 <= Ni, Nj <= 48 and 1 <= Nq <= 64 with 512 * ceil(Nq / 16) * (ceil(Nj / 4) + ceil(Ni / 4)) + 32 * even(max(16 * Nj + 2, "
    "16 * Ni + 2, 16 * (Nq | 1))) <= 81920 (both operators' matrix-core images and four wave buffers fit half a CU's LDS)")

_WEIGHTED_WEIGHT_ADJOINT_TEMPLATES = (
    (0, "iq,qj,ej,ei->eq"),
    (WO_P_T, "qi,qj,ej,ei->eq"),
    (WO_A_T, "iq,jq,ej,ei->eq"),
    (WO_P_T | WO_A_T, "qi,jq,ej,ei->eq"),
)


def weighted_weight_adjoint_lds_bytes(Ni: int, Nq: int, Nj: int) -> int:
    """Dynamic LDS of a block of ``fe_weightgrad_f64`` (``fe::weightgrad_lds_bytes``)."""
    buf = (max(16 * Nj + 2, 16 * Ni + 2, 16 * (Nq | 1)) + 1) & ~1
    return 8 * (((Nq + 15) // 16) * ((Nj + 3) // 4 + (Ni + 3) // 4) * 64 + 4 * buf)


def weighted_weight_adjoint_supported(Ni: int, Nq: int, Nj: int) -> bool:
    """The size rule of ``fe_weightgrad_f64`` (``fe_weightgrad_supported`` in C says the same): a pure function of
    (Ni, Nq, Nj).  Every shape of :func:`weighted_element_operator_supported` is inside."""
    Ni, Nq, Nj = int(Ni), int(Nq), int(Nj)
    return (1 <= Ni <= WEIGHTED_ELEMENT_OPERATOR_MAX_N and 1 <= Nj <= WEIGHTED_ELEMENT_OPERATOR_MAX_N
            and 1 <= Nq <= WEIGHTED_ELEMENT_OPERATOR_MAX_Q
            and weighted_weight_adjoint_lds_bytes(Ni, Nq, Nj) <= WEIGHTED_ELEMENT_OPERATOR_MAX_LDS)


def match_weighted_operator_weight_adjoint(einsum: BatchedEinsum) -> Optional[AdjointPlan]:
    """The :class:`AdjointPlan` (kind ``"weighted_w"``; ``layout_flags``: ``WO_P_T | WO_A_T``; roles ``"P"``, ``"A"``, ``"u"``,
    ``"g"``; params Ni, Nq, Nj) of :data:`WEIGHTED_WEIGHT_ADJOINT_RULE`, else ``None``.  P and A may be the same array; the u
    and g operands of a row are different arrays.  The einsum is its own mirror image -- (P, g, i) for (A, u, j), both operators
    transposed -- and both readings give the same bits (the product commutes); where both fit, the one whose g operands carry
    the names of output gradients (``autograd.output_grad_name``) is taken, else the first."""
    from feinsum_amd.autograd import GRAD_PREFIX

    if {np.dtype(dt) for dt in einsum.arg_to_dtype.values()} != {np.dtype("float64")}:
        return None
    fits = []
    for flags, subscripts in _WEIGHTED_WEIGHT_ADJOINT_TEMPLATES:
        for perm, mapping in _template_matches(einsum, subscripts):
            dim = lambda t: einsum.index_to_dim_length[mapping[t]]  # noqa: E731
            if any(isinstance(dim(t), SizeParam) for t in "iqj") or not isinstance(dim("e"), SizeParam):
                continue
            if not weighted_weight_adjoint_supported(int(dim("i")), int(dim("q")), int(dim("j"))):
                continue
            role = {name: perm[k] for k, name in enumerate(("P", "A", "u", "g"))}
            if len({(row[role["P"]].name, row[role["A"]].name) for row in einsum.args}) != 1:
                continue      # every row shares P and A
            if any(row[role["u"]].name == row[role["g"]].name for row in einsum.args):
                continue
            fits.append(AdjointPlan(ADJ_WEIGHTED_W, flags, role, dict(mapping),
                                    {"Ni": int(dim("i")), "Nq": int(dim("q")), "Nj": int(dim("j"))}))
    for plan in fits:
        if all(row[plan.roles["g"]].name.startswith(GRAD_PREFIX) for row in einsum.args):
            return plan
    return fits[0] if fits else None
