"""The walk over groups of fields that every form of the tetrahedral grad, div and face-mass entry points shares
(fe_orders.h, for_each_field_group): every field of a call is computed exactly once, whatever the form, the order and the
way the fields fall into launch groups.

Orders p = 4 (Np, Nfp = 35, 15) and p = 1 (4, 3); forms plain, prepared operator, accumulating (alpha = 0.5, beta = 2),
element slice (a slice of a base of 2 E elements at an odd offset) and float32 fields; E one wave tile plus three elements
and one tile minus one (the route below one tile); b = 1, 8, 9 for grad and div (FE_MAX_FIELDS = 8 fields per launch) and
b = 2, 4, 5, 9 for face-mass (groups of up to 8 at p = 4 plain and prepared: 9 -> 7 + 2; of up to 4 in the accumulating and
slice forms: 5 -> 3 + 2, 9 -> 4 + 3 + 2), with J stored [E][nf] and [nf][E] (the slice form's ldJ).  Outputs are pre-filled
with NaN (beta = 0) or seeded values; a field that a walk skips stays NaN or unscaled, one that it doubles is wrong under
beta != 0.

Reference: the float64 einsums of tests/dg.py evaluated by the numpy oracle.  Tolerance 1e-12 on max |got - ref| / max |ref|
(the bound of smoke()): every entry is a float64 sum of at most 3 * 35 * 4 products of numbers below one, so its rounding
error stays below about 420 * 2^-53 = 5e-14 of the sum of the magnitudes, which is within a small factor of max |ref|."""
import ctypes

import dg
import numpy as np
import pytest
import torch

from feinsum_amd import _hip
from feinsum_amd.family import FAMILY_DIV, FAMILY_FACEMASS, FAMILY_GRAD
from oracle import np_oracle

pytestmark = pytest.mark.gpu

NF = 4
ORDERS = {"p4": (35, 15, 1, 1, 1), "p1": (4, 3, 5, 5, 4)}     # Np, Nfp, and the sub-tiles of grad, div, face-mass (fe_orders.h)
FORMS = ["plain", "prepared", "accumulating", "slice", "float32"]
ALPHA, BETA = 0.5, 2.0
TOL = 1e-12


@pytest.fixture(scope="module", autouse=True)
def _leave_no_device_memory_behind():
    """The many small arrays of this module go back to the driver when it ends: later tests that measure or search the
    device's free memory (tests/test_placement.py) find it as they did before this module existed."""
    yield
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _rand(gen, *shape, dtype=torch.float64):
    return torch.rand(shape, dtype=dtype, device="cuda", generator=gen) - 0.5


def _sliced(gen, shape, eaxis, E, off, fill=None):
    """A view of E elements at `off` along `eaxis` of a base array with 2 E elements there."""
    base_shape = list(shape)
    base_shape[eaxis] = 2 * E
    base = _rand(gen, *base_shape) if fill is None else torch.full(base_shape, fill, dtype=torch.float64, device="cuda")
    return base, base.narrow(eaxis, off, E)


def _run(family, form, Np, Nfp, E, b, seed, reference=True, jfe=False):
    """Launch one call; returns (return code, outputs as numpy, references)."""
    lib = _hip.load_library()
    stream = torch.cuda.current_stream().cuda_stream
    gen = torch.Generator(device="cuda").manual_seed(seed)
    grad, fm = family == FAMILY_GRAD, family == FAMILY_FACEMASS
    sl, acc, f32 = form == "slice", form == "accumulating", form == "float32"
    off = 3
    in_shape = (NF, E, Nfp) if fm else (E, Np) if grad else (3, E, Np)
    out_shape = (3, E, Np) if grad else (E, Np)
    # J: [3][3][E]; for face-mass [E][nf] (contiguous in a slice too) or, with jfe, [nf][E] (FE_FM_J_FE: the slice has an ldJ)
    flags = 1 if fm and jfe else 0
    if fm and jfe:
        Jb, J = _sliced(gen, (NF, E), 1, E, off) if sl else (None, _rand(gen, NF, E))
    elif fm:
        Jb, J = _sliced(gen, (E, NF), 0, E, off) if sl else (None, _rand(gen, E, NF))
    else:
        Jb, J = _sliced(gen, (3, 3, E), 2, E, off) if sl else (None, _rand(gen, 3, 3, E))
    op = _rand(gen, NF, Np, Nfp) if fm else _rand(gen, 3, Np, Np)
    ins, outs, keep = [], [], [Jb]
    for _ in range(b):
        if sl and not grad:      # div, face-mass: the inputs carry the element axis of the base
            base, v = _sliced(gen, in_shape, 1, E, off)
            keep.append(base)
        else:
            v = _rand(gen, *in_shape, dtype=torch.float32 if f32 else torch.float64)
        ins.append(v)
        if sl and grad:          # grad: the outputs do
            base, o = _sliced(gen, out_shape, 1, E, off, fill=float("nan"))
            keep.append(base)
        elif acc:
            o = _rand(gen, *out_shape)
        else:
            o = torch.full(out_shape, float("nan"), dtype=torch.float64, device="cuda")
        outs.append(o)
    before = [o.clone() for o in outs]
    vt, ot = _hip._ptr_array([t.data_ptr() for t in ins]), _hip._ptr_array([t.data_ptr() for t in outs])
    Jp, opp, ld = J.data_ptr(), op.data_ptr(), 2 * E
    prep = buf = None
    if form == "prepared":
        buf = torch.empty(_hip.PREPARED_OPERATOR_BYTES, dtype=torch.uint8, device="cuda")
        prep = buf.data_ptr()
        _hip.prepare_operator(family, opp, Np, NF if fm else 0, Nfp if fm else 0, 0, prep, stream)
    if form in ("plain", "prepared"):
        if fm:
            rc = lib.fe_facemass_prepared_f64(Jp, opp, prep, vt, ot, E, Np, NF, Nfp, b, flags, 0, stream)
        else:
            entry = lib.fe_grad3d_prepared_f64 if grad else lib.fe_div3d_prepared_f64
            rc = entry(Jp, opp, prep, vt, ot, E, Np, b, 0, 0, stream)
    elif acc:
        if fm:
            rc = lib.fe_facemass_acc_f64(Jp, opp, vt, ot, E, Np, NF, Nfp, b, flags, ALPHA, BETA, stream)
        else:
            pack = _hip.ArgPack()
            pack.J, pack.D, pack.v, pack.outs, pack.E, pack.Np, pack.b, pack.ndim = Jp, opp, vt, ot, E, Np, b, 3
            pack.alpha, pack.beta = ALPHA, BETA
            rc = lib.fe_launch(family | _hip.FAMILY_ACC, ctypes.byref(pack), stream)
    elif sl:
        if fm:
            rc = lib.fe_facemass_strided_f64(Jp, ld, opp, vt, ld, ot, E, Np, NF, Nfp, b, flags, stream)
        elif grad:
            rc = lib.fe_grad3d_strided_f64(Jp, ld, opp, vt, ot, ld, E, Np, b, 0, stream)
        else:
            rc = lib.fe_div3d_strided_f64(Jp, ld, opp, vt, ld, ot, E, Np, b, 0, stream)
    else:
        if fm:
            rc = lib.fe_facemass_mixed_f64(Jp, opp, vt, ot, E, Np, NF, Nfp, b, flags, stream)
        else:
            rc = (lib.fe_grad3d_mixed_f64 if grad else lib.fe_div3d_mixed_f64)(Jp, opp, vt, ot, E, Np, b, 0, stream)
    torch.cuda.synchronize()
    if prep is not None:
        _hip.release_prepared(prep)
    if not reference:     # (tools/ab_frontends.py hashes the outputs of large calls instead)
        return rc, outs, None
    expr = dg.face_mass(1, Np, NF, Nfp) if fm else dg.grad(Np) if grad else dg.div(Np)
    host = [J.cpu().numpy().T if flags else J.cpu().numpy(), op.cpu().numpy()]
    refs = [np_oracle.reference_outputs(expr.get_subscripts(), [[*host, v.double().cpu().numpy()]])[0] for v in ins]
    if acc:
        refs = [ALPHA * r + BETA * o0.cpu().numpy() for r, o0 in zip(refs, before)]
    return rc, [o.cpu().numpy() for o in outs], refs


def _tile(family, order):
    Np, Nfp, mg, md, mf = ORDERS[order]
    return 16 * (mg if family == FAMILY_GRAD else md if family == FAMILY_DIV else mf)


@pytest.mark.parametrize("order", list(ORDERS))
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("family", [FAMILY_GRAD, FAMILY_DIV, FAMILY_FACEMASS], ids=["grad", "div", "face-mass"])
def test_every_field_of_every_group_is_computed_once(family, form, order):
    Np, Nfp = ORDERS[order][:2]
    tile = _tile(family, order)
    for E in (tile + 3, tile - 1):
        for b in ((2, 4, 5, 9) if family == FAMILY_FACEMASS else (1, 8, 9)):
            for jfe in ((False, True) if family == FAMILY_FACEMASS else (False,)):     # both J layouts of face-mass
                rc, outs, refs = _run(family, form, Np, Nfp, E, b, seed=1000 * E + b, jfe=jfe)
                _hip.check(rc)
                for k, (got, ref) in enumerate(zip(outs, refs)):
                    err = np_oracle.max_rel_err(got, ref) if np.isfinite(got).all() else float("inf")
                    print(f"{form} {order} family {family} E={E} b={b} jfe={jfe} field {k}: max rel err {err:.2e}")
                    assert np.isfinite(got).all(), (form, order, E, b, jfe, k)
                    assert err <= TOL, (form, order, E, b, jfe, k, err)


@pytest.mark.parametrize("order", list(ORDERS))
@pytest.mark.parametrize("form", ["accumulating", "slice"])
def test_one_face_mass_field_is_still_unsupported(form, order):
    Np, Nfp = ORDERS[order][:2]
    rc, outs, _ = _run(FAMILY_FACEMASS, form, Np, Nfp, _tile(FAMILY_FACEMASS, order) + 3, 1, seed=7)
    assert rc == _hip.FE_EUNSUPPORTED
