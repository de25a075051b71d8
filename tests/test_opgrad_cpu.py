"""Operator gradients (dD, dR) on the matrix cores, host side: the matcher, the transform's routing, the slice plan and
the argument checks of the C entry points -- everything that needs no GPU."""

import numpy as np
import pytest

import autograd_cases as C
import feinsum_amd as f
from feinsum_amd import _hip
from feinsum_amd.autograd import adjoint_einsums, evaluate_differentiable
from feinsum_amd.diagnostics import InvalidParameterError
from feinsum_amd.family import ADJ_OPERATOR_D, ADJ_OPERATOR_R
from feinsum_amd.measure import launch_kind

CASES = [(name, e) for name, e in C.dg_cases() if "noj" not in name]     # (the operator without J has no J-adjoint either)


def _term(name, e):
    (t,) = adjoint_einsums(e, "R" if name.startswith("facemass") else "D")
    return t


def _small_ints(einsum, E, seed=0):
    rng = np.random.default_rng(seed)
    return {n: rng.integers(-3, 4, size=C.concrete(einsum.arg_to_shape[n], E)).astype(np.float64)
            for n in sorted(einsum.all_args)}


def formula(plan, term, arrays, E):
    """The plan's roles and strides put through the kernel's stride formula, in numpy, summed over the rows."""
    p = plan.params
    if plan.kind == ADJ_OPERATOR_D:
        X, R, Np = p["X"], p["R"], p["Np"]
        jx, jr, je = (ce * E + c for ce, c in p["jstrides"])
        sr, sp, sq = p["strides"]
        out = np.zeros(R * Np * Np)
        for row in term.args:
            J, a, b = (arrays[row[plan.roles[r]].name] for r in ("J", "a", "b"))
            Jf, b = J.reshape(-1), b.reshape(X, E, Np)
            pp, q = np.meshgrid(np.arange(Np), np.arange(Np), indexing="ij")
            for r in range(R):
                w = sum(Jf[x * jx + r * jr + np.arange(E) * je][:, None] * b[x] for x in range(X))      # [E][p]
                np.add.at(out, r * sr + pp * sp + q * sq, w.T @ a)
        return out
    nf, Np, Nfp = p["nf"], p["Np"], p["Nfp"]
    out = np.zeros((nf, Np, Nfp))
    for row in term.args:
        J, v, g = (arrays[row[plan.roles[r]].name] for r in ("J", "v", "g"))
        Jef = J.T if plan.layout_flags & f.family.FM_J_FE else J
        out += np.einsum("ei,ef,fej->fij", g, Jef, v)
    rl = plan.layout_flags & (f.family.FM_R_IFJ | f.family.FM_R_T)
    perm = {0: (0, 1, 2), f.family.FM_R_IFJ: (1, 0, 2), f.family.FM_R_T: (0, 2, 1),
            f.family.FM_R_IFJ | f.family.FM_R_T: (2, 0, 1)}[rl]
    return out.transpose(perm).reshape(-1)


@pytest.mark.parametrize("name,e", CASES, ids=[n for n, _ in CASES])
def test_matcher_accepts_every_family_and_layout(name, e):
    t = _term(name, e)
    plan = f.match_operator_adjoint(t)
    assert plan is not None and plan.kind == (ADJ_OPERATOR_R if name.startswith("facemass") else ADJ_OPERATOR_D)
    E = 5
    arrays = _small_ints(t, E)
    sub = t.get_subscripts().replace(" ", "")
    ref = sum(np.einsum(sub, *[arrays[a.name] for a in row]) for row in t.args)
    assert np.array_equal(formula(plan, t, arrays, E), ref.reshape(-1))
    # the routes of today do not know these terms
    assert f.match_adjoint_family(t) is None
    assert launch_kind(t, "operator_adjoint", {"E": 10}) == "operator_adjoint"
    with pytest.raises(NotImplementedError):
        launch_kind(t, "adjoint", {"E": 10})


def test_default_launch_kind_is_unchanged():
    t = _term("grad", C.grad(3, 35))
    assert launch_kind(t, None, {"E": 10 ** 6}) == "reduction"
    assert launch_kind(t, None, {"E": 10}) == launch_kind(t, "auto", {"E": 10}) != "operator_adjoint"


def test_matcher_rejects():
    u56 = _term("grad", C.grad(3, 56))
    assert f.match_operator_adjoint(u56) is None
    for Np in (7, 13):
        assert f.match_operator_adjoint(_term("grad", C.grad(2, Np))) is None
    f32 = f.einsum("xre,ej,xei->rij", f.array("J", (3, 3, "E"), "float32"), f.array("u", ("E", 35), "float32"),
                   f.array("g", (3, "E", 35), "float32"))
    mixed = f.einsum("xre,ej,xei->rij", f.array("J", (3, 3, "E"), "float32"), f.array("u", ("E", 35)),
                     f.array("g", (3, "E", 35)))
    twice = f.einsum("re,ej,ei->rij", f.array("J", (3, "E")), f.array("u", ("E", 35)), f.array("u", ("E", 35)))
    for e in (f32, mixed, twice, C.grad(3, 35)):
        assert f.match_operator_adjoint(e) is None
    # rows of a batched term must share J
    rows = [[f.array(f"J{k}", (3, 3, "E")), f.array(f"u{k}", ("E", 35)), f.array(f"g{k}", (3, "E", 35))] for k in range(2)]
    assert f.match_operator_adjoint(f.batched_einsum("xre,ej,xei->rij", rows)) is None
    with pytest.raises(NotImplementedError, match="operator_adjoint"):
        launch_kind(C.grad(3, 35), "operator_adjoint", {"E": 10})
    import feinsum
    assert feinsum.match_operator_adjoint is f.match_operator_adjoint


def test_plan():
    assert _hip.opgrad_plan(0, 3675) == (0, 0)
    last = 0
    for E in list(range(1, 700)) + [10 ** 3, 65472, 65473, 65474, 10 ** 5, 10 ** 6, 10 ** 7]:
        S, nbytes = _hip.opgrad_plan(E, 3675)
        assert last <= S <= 1024 and S == min(1024, -(-E // 64))
        assert nbytes == -(-(S * 3675 * 8) // 256) * 256
        last = S
    assert _hip.opgrad_plan(10 ** 9, 48)[0] == 1024
    assert _hip.opgrad_plan(65, 48) == (2, 768)
    with pytest.raises(InvalidParameterError):
        _hip.opgrad_plan(-1, 48)
    for name in ("fe_opgrad_plan", "fe_opgrad_f64", "fe_facemass_opgrad_f64"):
        assert name in _hip.EXPORTED_SYMBOLS


def test_argument_checks_without_a_device():
    ok = dict(E=100, X=3, R=3, Np=35, jstrides=(300, 100, 1), strides=(1225, 35, 1))
    _, need = _hip.opgrad_plan(100, 3675)

    def call(J=256, a=256, b=256, out=256, ws=256, ws_bytes=need, **kw):
        k = {**ok, **kw}
        _hip.opgrad(J, [a], [b], out, k["E"], k["X"], k["R"], k["Np"], k["jstrides"], k["strides"], ws, ws_bytes)

    with pytest.raises(InvalidParameterError, match="E must be"):
        call(E=-1)
    for kw in (dict(Np=56), dict(Np=7), dict(X=4), dict(R=0)):
        with pytest.raises(NotImplementedError, match="not compiled"):
            call(**kw)
    for kw in (dict(J=None), dict(a=None), dict(b=None), dict(out=None)):
        with pytest.raises(InvalidParameterError, match="null"):
            call(**kw)
    with pytest.raises(InvalidParameterError, match="8-byte aligned"):
        call(a=260)
    with pytest.raises(InvalidParameterError, match="dense layout"):
        call(strides=(1225, 35, 2))
    with pytest.raises(InvalidParameterError, match="null workspace"):
        call(ws=None)
    with pytest.raises(InvalidParameterError, match="the plan needs"):
        call(ws_bytes=need - 256)
    with pytest.raises(InvalidParameterError, match="256-byte aligned"):
        call(ws=264)

    _, need = _hip.opgrad_plan(100, 4 * 35 * 15)

    def fm(J=256, g=256, v=256, dR=256, ws=256, ws_bytes=need, E=100, shape=(35, 4, 15), flags=0):
        _hip.facemass_opgrad(J, [g], [v], dR, E, *shape, ws, ws_bytes, layout_flags=flags)

    with pytest.raises(InvalidParameterError, match="E must be"):
        fm(E=-1)
    with pytest.raises(NotImplementedError, match="not compiled"):
        fm(shape=(56, 4, 21))
    with pytest.raises(InvalidParameterError, match="layout flags"):
        fm(flags=8)
    for kw in (dict(J=None), dict(g=None), dict(v=None), dict(dR=None)):
        with pytest.raises(InvalidParameterError, match="null"):
            fm(**kw)
    with pytest.raises(InvalidParameterError, match="null workspace"):
        fm(ws=None)
    with pytest.raises(InvalidParameterError, match="the plan needs"):
        fm(ws_bytes=0)
    with pytest.raises(InvalidParameterError, match="256-byte aligned"):
        fm(ws=8)


def test_keyword_is_checked_before_the_device():
    with pytest.raises(InvalidParameterError, match="operator_gradients"):
        evaluate_differentiable(C.grad(3, 35), None, {}, operator_gradients="bogus")
