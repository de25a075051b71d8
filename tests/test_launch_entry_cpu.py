"""``fe_launch``, the one dispatcher of bound DG launches, without a device: what it refuses, that E = 0 is a no-op, that a
pack reaches the named entry point's own argument checks -- and the one rule that groups the rows of a batched einsum into
launches (``measure._family_groups``), against the packs a bound launch holds."""

import ctypes

import pytest
import torch

import feinsum_amd as f
from feinsum_amd import _hip
from feinsum_amd.family import (FAMILY_DIV, FAMILY_DIVCOMP, FAMILY_FACEMASS, FAMILY_GRAD, FAMILY_GRADPLANES,
                                FAMILY_MATAPPLY, match_family)
from feinsum_amd.measure import _family_groups, _FamilyLaunch, accumulate_route

FAMILY_GRADDIV = 3
FAMILIES = (FAMILY_GRAD, FAMILY_DIV, FAMILY_GRADDIV, FAMILY_FACEMASS, FAMILY_DIVCOMP, FAMILY_GRADPLANES, FAMILY_MATAPPLY)
F32, ACC = _hip.FAMILY_F32, _hip.FAMILY_ACC


def _pack(E=10, Np=35, b=1, ptr=8, fields=None, **kw):
    """A pack whose device pointers all hold the (never dereferenced) address *ptr*; ``(pack, what keeps it alive)``."""
    n = 3 * max(b, 1)                       # room for the planes of FE_FAMILY_GRADPLANES
    v, outs, j3 = (_hip._ptr_array([ptr if fields is None else fields] * n) for _ in range(3))
    pack = _hip.ArgPack()
    pack.J = pack.D = pack.u = pack.v_div = pack.out = pack.out2 = ptr
    pack.v, pack.outs, pack.j3 = v, outs, j3
    pack.E, pack.Np, pack.nf, pack.Nfp, pack.b, pack.ndim = E, Np, 4, 15, b, 3
    pack.alpha, pack.beta = 1.0, 0.0
    for key, value in kw.items():
        setattr(pack, key, value)
    return pack, (v, outs, j3)


def _launch(family, pack):
    lib = _hip.load_library()
    rc = lib.fe_launch(family, ctypes.byref(pack) if pack is not None else None, None)
    return rc, lib.fe_last_error()


def _named(entry, *args):
    lib = _hip.load_library()
    rc = getattr(lib, entry)(*args)
    return rc, lib.fe_last_error()


def test_null_pack_and_unknown_family_are_invalid():
    for family in FAMILIES + (FAMILY_GRAD | F32, FAMILY_FACEMASS | ACC):
        rc, msg = _launch(family, None)
        assert rc == _hip.FE_EINVAL and b"null argument pack" in msg, (family, msg)
    pack, _keep = _pack()
    for family in (0, 8, 99, 255):
        rc, msg = _launch(family, pack)
        assert rc == _hip.FE_EINVAL and b"unknown family" in msg, (family, msg)


def test_accumulating_is_refused_where_no_kernel_accumulates():
    pack, _keep = _pack(b=2)
    for family in (FAMILY_MATAPPLY, FAMILY_DIVCOMP, FAMILY_GRADPLANES, FAMILY_GRADDIV):
        rc, msg = _launch(family | ACC, pack)
        assert rc == _hip.FE_EUNSUPPORTED and b"0x%x" % family in msg, (family, msg)
    for family in FAMILIES:                                  # float32 never accumulates, whatever the family
        rc, msg = _launch(family | ACC | F32, pack)
        assert rc == _hip.FE_EUNSUPPORTED and b"0x%x" % (family | F32) in msg, (family, msg)


def test_no_elements_is_a_no_op_for_every_family():
    pack, _keep = _pack(E=0, b=2, ptr=0)
    pack1, _keep1 = _pack(E=0, b=1, ptr=0)
    codes = FAMILIES + tuple(fam | ACC for fam in (FAMILY_GRAD, FAMILY_DIV, FAMILY_FACEMASS)) \
        + tuple(fam | F32 for fam in (FAMILY_GRAD, FAMILY_DIV, FAMILY_DIVCOMP, FAMILY_MATAPPLY, FAMILY_FACEMASS))
    for family in codes:
        assert _launch(family, pack)[0] == _hip.FE_OK, (family, _launch(family, pack))
    for family in (FAMILY_GRAD, FAMILY_DIV, FAMILY_DIVCOMP):     # the single pair u / out
        assert _launch(family, pack1)[0] == _hip.FE_OK, family


def test_a_pack_reaches_the_named_entry_points_checks():
    """Every check of test_abi.test_argument_validation_without_gpu, once through the named entry point and once through a
    pack: the same code and the same text."""
    one, two = _hip._ptr_array([8]), _hip._ptr_array([8, 8])
    nan = float("nan")
    cases = [
        # negative E, Np = 0, null pointer, unknown variant, misaligned pointer, bad operator flags
        (("fe_grad3d_f64_ex", 0, 0, 0, 0, -1, 35, 0, 0, None), FAMILY_GRAD, dict(E=-1, ptr=0)),
        (("fe_div3d_f64_ex", 0, 0, 0, 0, 10, 0, 0, 0, None), FAMILY_DIV, dict(Np=0, ptr=0)),
        (("fe_grad3d_f64_ex", 0, 0, 0, 0, 10, 35, 0, 0, None), FAMILY_GRAD, dict(ptr=0)),
        (("fe_grad3d_f64_ex", 8, 8, 8, 8, 10, 35, 0, 7, None), FAMILY_GRAD, dict(variant=7)),
        (("fe_div3d_f64_ex", 8, 8, 12, 8, 10, 35, 0, 0, None), FAMILY_DIV, dict(u=12)),
        (("fe_grad3d_f64_ex", 8, 8, 8, 8, 10, 35, 4, 0, None), FAMILY_GRAD, dict(layout_flags=4)),
        (("fe_divcomp3d_f64", 8, 8, 8, 8, 10, 35, 8, 0, None), FAMILY_DIVCOMP, dict(layout_flags=8)),
        (("fe_facemass_f64", 8, 8, one, one, 10, 35, 4, 15, 1, 8, 0, None), FAMILY_FACEMASS, dict(layout_flags=8)),
        (("fe_matapply_f64", 8, 8, two, two, 10, 35, 2, 2, 0, None), FAMILY_MATAPPLY, dict(b=2, layout_flags=2)),
        (("fe_grad_f64", 8, 8, two, two, 10, 2, 10, 2, 0, 1, None), FAMILY_GRAD, dict(b=2, ndim=2, Np=10, variant=1)),
        # ... and of the accumulating entry points: non-finite alpha or beta, negative E, no kernel for the shape
        (("fe_grad3d_acc_f64", 8, 8, 8, 8, 10, 35, 0, nan, 0.0, None), FAMILY_GRAD | ACC, dict(b=2, alpha=nan)),
        (("fe_div3d_acc_f64", 8, 8, 8, 8, 10, 35, 0, 1.0, float("inf"), None), FAMILY_DIV | ACC,
         dict(b=2, beta=float("inf"))),
        (("fe_div3d_acc_f64", 8, 8, 8, 8, -3, 35, 0, 1.0, 0.0, None), FAMILY_DIV | ACC, dict(b=2, E=-3)),
        (("fe_grad3d_acc_f64", 8, 8, 8, 8, 10, 56, 0, 1.0, 0.0, None), FAMILY_GRAD | ACC, dict(b=2, Np=56)),
        (("fe_grad3d_acc_f64", 8, 8, 0, 8, 10, 35, 0, 1.0, 0.0, None), FAMILY_GRAD | ACC, dict(b=2, fields=0)),
        (("fe_facemass_acc_f64", 8, 8, two, two, 10, 35, 4, 15, 2, 0, nan, 0.0, None), FAMILY_FACEMASS | ACC,
         dict(b=2, alpha=nan)),
        (("fe_facemass_acc_f64", 8, 8, one, one, 10, 35, 4, 15, 1, 0, 1.0, 1.0, None), FAMILY_FACEMASS | ACC,
         dict(b=1, beta=1.0)),
    ]
    for named, family, fields in cases:
        pack, _keep = _pack(**fields)
        want = _named(*named)
        assert want[0] in (_hip.FE_EINVAL, _hip.FE_EUNSUPPORTED) and want[1], named
        assert _launch(family, pack) == want, (named, _launch(family, pack))
    pack, _keep = _pack(layout_flags=4)                       # float32: the pack's own entry point
    want = _named("fe_launch_f32", FAMILY_GRAD, ctypes.byref(pack), None)
    assert want[0] == _hip.FE_EINVAL and _launch(FAMILY_GRAD | F32, pack) == want
    # alpha and beta are read with FE_FAMILY_ACC only
    pack, _keep = _pack(E=0, alpha=nan, beta=nan)
    assert _launch(FAMILY_GRAD, pack)[0] == _launch(FAMILY_GRAD | F32, pack)[0] == _hip.FE_OK
    # accumulating grad / div walk the field tables; without them the pack is refused, not dereferenced
    pack = _hip.ArgPack()
    pack.E, pack.Np, pack.b = 10, 35, 1
    rc, msg = _launch(FAMILY_GRAD | ACC, pack)
    assert rc == _hip.FE_EINVAL and b"v / outs" in msg


# ---- the grouping rule ---------------------------------------------------------------------------------------------

Np, Nfp, E = 10, 6, 5
GRAD, COMP, NOJ, LIFT = "xre,rij,ej->xei", "re,rij,ej->ei", "ij,ej->ei", "ef,fij,fej->ei"
_SHAPES = {GRAD: ((3, 3, E), (3, Np, Np), (E, Np)), COMP: ((3, E), (3, Np, Np), (E, Np)), NOJ: ((Np, Np), (E, Np)),
           LIFT: ((E, 4), (4, Np, Nfp), (4, E, Nfp))}

#: (what, subscripts, the operand names of every row, the rows of every launch)
GROUPING = [
    ("one row", GRAD, [("J", "D", "a")], [range(0, 1)]),
    ("shared J and D", GRAD, [("J", "D", "a"), ("J", "D", "b"), ("J", "D", "c")], [range(0, 3)]),
    ("shared J and R", LIFT, [("J", "R", f"v{k}") for k in range(4)], [range(0, 4)]),
    ("the same field twice", GRAD, [("J", "D", "a"), ("J", "D", "a")], [range(0, 2)]),
    ("alternating operators", GRAD, [("J", "D0", "a"), ("J", "D1", "b"), ("J", "D0", "c"), ("J", "D1", "d")],
     [range(0, 1), range(1, 2), range(2, 3), range(3, 4)]),
    ("alternating factors", GRAD, [("J0", "D", "a"), ("J1", "D", "b"), ("J0", "D", "c")],
     [range(0, 1), range(1, 2), range(2, 3)]),
    ("non-adjacent sharing", GRAD, [("J", "D", "a"), ("J", "D", "b"), ("K", "D", "c"), ("J", "D", "d")],
     [range(0, 2), range(2, 3), range(3, 4)]),
    ("a change of operator ends a group", GRAD, [("J", "D", "a"), ("J", "R", "a"), ("J", "R", "b")],
     [range(0, 1), range(1, 3)]),
    ("div components never group", COMP, [("J", "D", "a"), ("J", "D", "b"), ("J", "D", "c")],
     [range(0, 1), range(1, 2), range(2, 3)]),
    ("no J: the operator alone", NOJ, [("D", "a"), ("D", "b"), ("D2", "c"), ("D", "d")],
     [range(0, 2), range(2, 3), range(3, 4)]),
]


@pytest.mark.parametrize("what,subs,names,expected", GROUPING, ids=[g[0] for g in GROUPING])
def test_rows_that_share_j_and_the_operator_become_one_launch(what, subs, names, expected):
    expr = f.batched_einsum(subs, [[f.array(n, shape) for n, shape in zip(row, _SHAPES[subs])] for row in names])
    plan = match_family(expr)
    assert plan is not None
    assert _family_groups(plan, expr) == expected
    assert [k for group in expected for k in group] == list(range(len(names)))      # every row once, in order
    # a bound launch holds one pack per group, with the group's fields in row order (host tensors: nothing is launched)
    args = {a.name: torch.zeros([int(d) for d in a.shape], dtype=torch.float64) for row in expr.args for a in row}
    outs = [torch.zeros([E if i == plan.long_index else (3 if i == "x" else Np) for i in expr.out_idx_set],
                        dtype=torch.float64) for _ in names]
    bound = _FamilyLaunch(plan, expr, args, outs, None)
    assert bound.group_family == plan.family and bound.family_code == plan.family
    assert [p.b for p in bound.groups] == [len(group) for group in expected]
    for pack, group in zip(bound.groups, expected):
        assert [pack.v[k] for k in range(pack.b)] == [args[names[m][-1]].data_ptr() for m in group]
        assert [pack.outs[k] for k in range(pack.b)] == [outs[m].data_ptr() for m in group]
        assert pack.D == args[names[group[0]][-2]].data_ptr()
        assert pack.J == (args[names[group[0]][0]].data_ptr() if len(names[0]) == 3 else None)
        assert (pack.u, pack.out, pack.E) == (pack.v[0], pack.outs[0], E)


def test_the_family_code_says_how_the_packs_are_read():
    rows = [("J", "R", f"v{k}") for k in range(2)]
    for dtype, scale, code in (("float64", None, FAMILY_FACEMASS), ("float32", None, FAMILY_FACEMASS | F32),
                               ("float64", (0.5, -2.0), FAMILY_FACEMASS | ACC)):
        expr = f.batched_einsum(LIFT, [[f.array(n, s, dtype) for n, s in zip(row, _SHAPES[LIFT])] for row in rows])
        tdt = getattr(torch, dtype)
        args = {a.name: torch.zeros([int(d) for d in a.shape], dtype=tdt) for row in expr.args for a in row}
        outs = [torch.zeros((E, Np), dtype=tdt) for _ in rows]
        bound = _FamilyLaunch(match_family(expr), expr, args, outs, None, scale=scale)
        assert bound.family_code == code
        assert [(p.alpha, p.beta) for p in bound.groups] == [scale or (1.0, 0.0)]


def test_accumulate_route_uses_the_same_groups():
    lift = lambda rows: f.batched_einsum(LIFT, [[f.array(n, s) for n, s in zip(row, _SHAPES[LIFT])] for row in rows])   # noqa: E731
    assert accumulate_route(lift([("J", "R", "a"), ("J", "R", "b")])) == "kernel"
    assert accumulate_route(lift([("J", "R", "a"), ("K", "R", "b"), ("K", "R", "c")])) == "axpby"    # a group of one
    assert accumulate_route(lift([("J", "R", "a"), ("K", "R", "b"), ("J", "R", "c")])) == "axpby"    # non-adjacent
