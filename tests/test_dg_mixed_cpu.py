"""Float32 fields in float64 grad, div and face-mass (transform ``"mixed_family"``) without a device:
which einsums ``family.match_mixed_family`` accepts and what it refuses, that nothing else changed its route for them, and
what ``fe_launch`` answers under ``FE_FAMILY_FIELDS_F32`` before any device work."""

import ctypes

import numpy as np
import pytest

import feinsum_amd as f
from feinsum_amd import _hip
from feinsum_amd.family import (FAMILY_DIV, FAMILY_DIVCOMP, FAMILY_FACEMASS, FAMILY_GRAD, FAMILY_GRADDIV, FAMILY_GRADPLANES,
                                FAMILY_MATAPPLY, FM_J_FE, FM_R_IFJ, FM_R_T, OP_TRANSPOSED, match_family)
from feinsum_amd.measure import accumulate_route, launch_kind

TETS = ((4, 3), (10, 6), (20, 10), (35, 15))          # (Np, Nfp) of p = 1..4
FM_LAYOUTS = [(j, r, jf | rf) for j, jf in (("ef", 0), ("fe", FM_J_FE))
              for r, rf in (("fij", 0), ("ifj", FM_R_IFJ), ("fji", FM_R_T), ("jfi", FM_R_IFJ | FM_R_T))]
F32, ACC, FIELDS_F32 = _hip.FAMILY_F32, _hip.FAMILY_ACC, _hip.FAMILY_FIELDS_F32


def _shape(sub, ext):
    return tuple(ext[c] for c in sub)


def mixed_einsum(family, Np, b=1, layout=None, nf=4, Nfp=None, ndim=3, dtypes=("float64", "float64", "float32"), order=(0, 1, 2)):
    """grad / div / face-mass x b with operand dtypes (J, operator, field); *layout*: the operator subscripts of grad / div,
    (J, R) subscripts of face-mass; *order*: the operand order within a row."""
    Nfp = dict(TETS).get(Np, 3) if Nfp is None else Nfp
    if family == "facemass":
        jsub, rsub = layout or ("ef", "fij")
        subs, out = [jsub, rsub, "fej"], "ei"
        ext = {"e": "E", "f": nf, "i": Np, "j": Nfp}
    else:
        subs, out = ["xre", layout or "rij", "ej" if family == "grad" else "xej"], "xei" if family == "grad" else "ei"
        ext = {"e": "E", "x": ndim, "r": ndim, "i": Np, "j": Np}
    names = ("J", "R", "u")
    rows = []
    for k in range(b):
        row = [f.array(names[p] + (str(k) if p == 2 else ""), _shape(subs[p], ext),
                       dtypes[p][k] if isinstance(dtypes[p], (list, tuple)) else dtypes[p]) for p in range(3)]
        rows.append([row[p] for p in order])
    return f.batched_einsum(",".join(subs[p] for p in order) + "->" + out, rows)


ACCEPTED = ([("grad", Np, op, OP_TRANSPOSED * (op == "rji")) for Np, _ in TETS for op in ("rij", "rji")]
            + [("div", Np, op, OP_TRANSPOSED * (op == "rji")) for Np, _ in TETS for op in ("rij", "rji")]
            + [("facemass", Np, (j, r), flags) for Np, _ in TETS for j, r, flags in FM_LAYOUTS])


@pytest.mark.parametrize("family,Np,layout,flags", ACCEPTED, ids=[f"{a[0]}-{a[1]}-{a[2]}" for a in ACCEPTED])
def test_the_matcher_accepts_every_listed_einsum(family, Np, layout, flags):
    from feinsum_amd.family import match_mixed_family

    code = {"grad": FAMILY_GRAD, "div": FAMILY_DIV, "facemass": FAMILY_FACEMASS}[family]
    for b in (1, 2, 9):
        for order in ((0, 1, 2), (2, 0, 1), (1, 2, 0)):
            expr = mixed_einsum(family, Np, b, layout, order=order)
            plan = match_mixed_family(expr)
            assert plan is not None, (family, Np, layout, b, order)
            assert (plan.family, plan.layout_flags, plan.params["Np"], plan.params["fields_f32"]) == (code, flags, Np, 1)
            assert [order[plan.roles[r]] for r in ("J", "D" if family != "facemass" else "R", "u" if family != "facemass" else "v")] \
                == [0, 1, 2]
            if family == "facemass":
                assert (plan.params["nf"], plan.params["Nfp"]) == (4, dict(TETS)[Np])
            assert launch_kind(expr, "mixed_family", {"E": 1000}) == "mixed_family"
            assert launch_kind(expr, {"variant": "mixed_family"}, {"E": 1000}) == "mixed_family"
            # ... and nothing else changed its mind about the einsum
            assert match_family(expr) is None
            assert launch_kind(expr, "auto", {"E": 1000}) == "generic" and launch_kind(expr, None, {"E": 1000}) == "generic"
            assert launch_kind(expr, "contraction", {"E": 1000}) == "contraction"
            assert accumulate_route(expr, "mixed_family") == "axpby"
            for forced in ("kernel", "epilogue"):
                with pytest.raises(NotImplementedError):
                    accumulate_route(expr, {"variant": "mixed_family", "accumulate": forced})


REFUSED = [
    ("a float32 J", lambda: mixed_einsum("div", 35, dtypes=("float32", "float64", "float32"))),
    ("a float32 operator", lambda: mixed_einsum("grad", 35, dtypes=("float64", "float32", "float32"))),
    ("a float32 operator, face-mass", lambda: mixed_einsum("facemass", 35, 2, dtypes=("float64", "float32", "float32"))),
    ("one float64 field in the batch", lambda: mixed_einsum("facemass", 35, 3, dtypes=("float64", "float64", ["float32", "float64", "float32"]))),
    ("one float64 field in the batch, div", lambda: mixed_einsum("div", 20, 2, dtypes=("float64", "float64", ["float64", "float32"]))),
    ("triangles", lambda: mixed_einsum("div", 10, ndim=2)),
    ("triangles, face-mass", lambda: mixed_einsum("facemass", 10, nf=3, Nfp=4)),
    ("p = 5", lambda: mixed_einsum("grad", 56)),
    ("p = 5, face-mass", lambda: mixed_einsum("facemass", 56, Nfp=21)),
    ("a face count that is no order's", lambda: mixed_einsum("facemass", 35, Nfp=10)),
    ("all float64", lambda: mixed_einsum("div", 35, dtypes=("float64",) * 3)),
    ("all float32", lambda: mixed_einsum("facemass", 35, 4, dtypes=("float32",) * 3)),
    ("div components", lambda: f.einsum("re,rij,ej->ei", f.array("J", (3, "E")), f.array("R", (3, 35, 35)),
                                        f.array("u", ("E", 35), "float32"))),
    ("the element-local operator", lambda: f.einsum("e,ij,ej->ei", f.array("J", ("E",)), f.array("R", (35, 35)),
                                                    f.array("u", ("E", 35), "float32"))),
    ("the operator alone", lambda: f.einsum("ij,ej->ei", f.array("R", (35, 35)), f.array("u", ("E", 35), "float32"))),
    ("a matrix product", lambda: f.einsum("ik,kj->ij", f.array("a", (8, "E")), f.array("b", ("E", 8), "float32"))),
]


@pytest.mark.parametrize("what,make", REFUSED, ids=[r[0] for r in REFUSED])
def test_everything_else_is_refused_by_name_of_the_rule(what, make):
    from feinsum_amd.family import match_mixed_family

    expr = make()
    assert match_mixed_family(expr) is None
    with pytest.raises(NotImplementedError, match="mixed_family.*float32.*float64"):
        launch_kind(expr, "mixed_family", {"E": 1000})


def test_a_bound_launch_carries_the_bit():
    import torch

    from feinsum_amd.family import match_mixed_family
    from feinsum_amd.measure import _FamilyLaunch

    E = 5
    for family, code in (("grad", FAMILY_GRAD), ("div", FAMILY_DIV), ("facemass", FAMILY_FACEMASS)):
        expr = mixed_einsum(family, 10, 2)
        args = {a.name: torch.zeros([E if isinstance(d, f.SizeParam) else int(d) for d in a.shape],
                                    dtype=getattr(torch, np.dtype(a.dtype).name)) for row in expr.args for a in row}
        outs = [torch.zeros((3, E, 10) if family == "grad" else (E, 10), dtype=torch.float64) for _ in range(2)]
        bound = _FamilyLaunch(match_mixed_family(expr), expr, args, outs, None)
        assert bound.family_code == code | _hip.FAMILY_FIELDS_F32 == code | 0x400
        assert [p.b for p in bound.groups] == [2]
        assert [bound.groups[0].v[k] for k in range(2)] == [args["u0"].data_ptr(), args["u1"].data_ptr()]
        assert bound.prepare_operators() == 0


# ---- fe_launch under FE_FAMILY_FIELDS_F32, no device --------------------------------------------------------------------

def _pack(E=10, Np=35, b=1, ptr=8, fields=None, outs=None, **kw):
    n = max(b, 1)
    v = _hip._ptr_array([ptr if fields is None else fields] * n)
    o = _hip._ptr_array([ptr if outs is None else outs] * n)
    pack = _hip.ArgPack()
    pack.J = pack.D = pack.u = pack.out = ptr
    pack.v, pack.outs = v, o
    pack.E, pack.Np, pack.nf, pack.Nfp, pack.b, pack.ndim = E, Np, 4, 15, b, 3
    pack.alpha, pack.beta = 1.0, 0.0
    for key, value in kw.items():
        setattr(pack, key, value)
    return pack, (v, o)


def _launch(family, pack):
    lib = _hip.load_library()
    rc = lib.fe_launch(family, ctypes.byref(pack) if pack is not None else None, None)
    return rc, lib.fe_last_error()


MIXED = tuple(fam | FIELDS_F32 for fam in (FAMILY_GRAD, FAMILY_DIV, FAMILY_FACEMASS))


def test_the_constant_and_the_entry_points_exist():
    assert _hip.FAMILY_FIELDS_F32 == 0x400
    for name in ("fe_grad3d_mixed_f64", "fe_div3d_mixed_f64", "fe_facemass_mixed_f64"):
        assert name in _hip.SIGNATURES and hasattr(_hip.load_library(), name)


def test_a_null_pack_is_invalid():
    for family in MIXED:
        rc, msg = _launch(family, None)
        assert rc == _hip.FE_EINVAL and b"null argument pack" in msg, (family, msg)


def test_misaligned_pointers_are_invalid_before_any_device_work():
    for family in MIXED:
        for fields in (9, 10, 11, 6):                       # a float32 field needs 4 bytes
            pack, _keep = _pack(fields=fields, b=2)
            rc, msg = _launch(family, pack)
            assert rc == _hip.FE_EINVAL and b"4-byte aligned" in msg, (family, fields, msg)
        for fields in (4, 12, 16):                          # ... and no more
            pack, _keep = _pack(E=0, fields=fields, b=2)
            assert _launch(family, pack)[0] == _hip.FE_OK, (family, fields)
        for key in ("J", "D"):
            pack, _keep = _pack(**{key: 12})
            rc, msg = _launch(family, pack)
            assert rc == _hip.FE_EINVAL and b"8-byte aligned" in msg, (family, key, msg)
        pack, _keep = _pack(outs=12)
        rc, msg = _launch(family, pack)
        assert rc == _hip.FE_EINVAL and b"8-byte aligned" in msg, (family, msg)
        # the single pair u / out of a pack without tables
        pack = _hip.ArgPack()
        pack.J = pack.D = pack.out = 8
        pack.u, pack.E, pack.Np, pack.nf, pack.Nfp, pack.b = 6, 10, 35, 4, 15, 1
        rc, msg = _launch(family, pack)
        assert rc == _hip.FE_EINVAL and b"4-byte aligned" in msg, (family, msg)
        pack.b = 2
        rc, msg = _launch(family, pack)
        assert rc == _hip.FE_EINVAL and b"v / outs" in msg, (family, msg)


def test_the_bit_goes_with_three_families_and_no_other_bit():
    pack, _keep = _pack(b=2)
    for family in (FAMILY_GRADDIV, FAMILY_DIVCOMP, FAMILY_GRADPLANES, FAMILY_MATAPPLY):
        rc, msg = _launch(family | FIELDS_F32, pack)
        assert rc == _hip.FE_EUNSUPPORTED and b"0x%x" % family in msg, (family, msg)
    for family in (FAMILY_GRAD, FAMILY_DIV, FAMILY_FACEMASS):
        for other in (F32, ACC, F32 | ACC):
            rc, msg = _launch(family | FIELDS_F32 | other, pack)
            assert rc == _hip.FE_EUNSUPPORTED and b"float32 fields" in msg, (family, other, msg)


def test_an_order_without_a_kernel_is_unsupported_and_no_elements_a_no_op():
    for family in MIXED:
        for Np in (56, 3, 21, 36):
            pack, _keep = _pack(Np=Np)
            rc, msg = _launch(family, pack)
            assert rc == _hip.FE_EUNSUPPORTED and b"p = 1..4" in msg, (family, Np, msg)
        pack, _keep = _pack(E=0, ptr=0, b=3)
        assert _launch(family, pack)[0] == _hip.FE_OK
        pack, _keep = _pack(E=-1)
        assert _launch(family, pack)[0] == _hip.FE_EINVAL
        pack, _keep = _pack(ptr=0, fields=8, outs=8)
        rc, msg = _launch(family, pack)
        assert rc == _hip.FE_EINVAL and b"null device pointer" in msg, (family, msg)
    pack, _keep = _pack(Nfp=10)                              # face-mass: (Np, Nfp) must be one order's
    assert _launch(FAMILY_FACEMASS | FIELDS_F32, pack)[0] == _hip.FE_EUNSUPPORTED
    pack, _keep = _pack(nf=3)
    assert _launch(FAMILY_FACEMASS | FIELDS_F32, pack)[0] == _hip.FE_EUNSUPPORTED
    for family, flags in ((FAMILY_GRAD | FIELDS_F32, 2), (FAMILY_DIV | FIELDS_F32, 4), (FAMILY_FACEMASS | FIELDS_F32, 8)):
        pack, _keep = _pack(layout_flags=flags)
        assert _launch(family, pack)[0] == _hip.FE_EINVAL
