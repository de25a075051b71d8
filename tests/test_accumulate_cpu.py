"""Accumulating evaluation (``out <- alpha E + beta out``) without a device: the two new entry
points are declared and exported and check their arguments before they touch the HIP runtime, and the routing --
which einsums add onto their outputs inside the face-mass kernel and which through ``fe_axpby`` -- follows from the
einsum alone."""

import inspect
import math
import re
from pathlib import Path

import pytest

import autograd_cases as C
import feinsum
import feinsum_amd as f
from feinsum_amd import _hip, measure
from feinsum_amd.diagnostics import InvalidParameterError

ROOT = Path(__file__).resolve().parents[1]


def test_both_symbols_are_declared_and_exported():
    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "feinsum_hip.h").read_text(), flags=re.S)
    lib = _hip.load_library()
    for sym in ("fe_facemass_acc_f64", "fe_axpby"):
        assert re.search(rf"\bint {sym}\s*\(", header), sym
        assert sym in _hip.EXPORTED_SYMBOLS and hasattr(lib, sym)


def test_facemass_acc_checks_its_arguments_without_gpu():
    ok = dict(E=10, Np=35, nf=4, Nfp=15, alpha=1.0, beta=1.0)
    with pytest.raises(InvalidParameterError, match="E must be"):
        _hip.facemass_acc(8, 8, [8, 8], [8, 8], **{**ok, "E": -1})
    lib = _hip.load_library()
    rc = lib.fe_facemass_acc_f64(8, 8, None, None, 10, 35, 4, 15, 2, 0, 1.0, 1.0, None)     # null tables
    assert rc == _hip.FE_EINVAL and b"null pointer table" in lib.fe_last_error()
    with pytest.raises(InvalidParameterError, match="layout"):
        _hip.facemass_acc(8, 8, [8, 8], [8, 8], **ok, layout_flags=8)
    with pytest.raises(InvalidParameterError, match="8-byte aligned"):
        _hip.facemass_acc(8, 8, [8, 12], [8, 8], **ok)
    with pytest.raises(InvalidParameterError, match="8-byte aligned"):
        _hip.facemass_acc(8, 8, [8, 8], [8, 20], **ok)
    with pytest.raises(InvalidParameterError, match="8-byte aligned"):
        _hip.facemass_acc(12, 8, [8, 8], [8, 8], **ok)
    with pytest.raises(InvalidParameterError, match="null"):
        _hip.facemass_acc(0, 8, [8, 8], [8, 8], **ok)
    for bad in (math.nan, math.inf, -math.inf):
        with pytest.raises(InvalidParameterError, match="finite"):
            _hip.facemass_acc(8, 8, [8, 8], [8, 8], **{**ok, "alpha": bad})
        with pytest.raises(InvalidParameterError, match="finite"):
            _hip.facemass_acc(8, 8, [8, 8], [8, 8], **{**ok, "beta": bad})
    with pytest.raises(InvalidParameterError, match="as many outputs"):
        _hip.facemass_acc(8, 8, [8, 8], [8], **ok)
    # outside the compiled scope: one field, triangles, p = 5, a shape of no order
    for kw, v in (({}, [8]), ({"Np": 10, "nf": 3, "Nfp": 4}, [8, 8]), ({"Np": 56, "Nfp": 21}, [8, 8]), ({"Np": 36}, [8, 8])):
        with pytest.raises(NotImplementedError, match="no fused kernel"):
            _hip.facemass_acc(8, 8, v, v, **{**ok, **kw})
    _hip.facemass_acc(0, 0, [0, 0], [0, 0], **{**ok, "E": 0})      # E == 0: a valid no-op, no HIP call


def test_axpby_checks_its_arguments_without_gpu():
    with pytest.raises(InvalidParameterError, match="n must be"):
        _hip.axpby(8, 8, -1, 1.0, 1.0)
    with pytest.raises(InvalidParameterError, match="null"):
        _hip.axpby(0, 8, 4, 1.0, 1.0)
    with pytest.raises(InvalidParameterError, match="null"):
        _hip.axpby(8, 0, 4, 1.0, 1.0)
    with pytest.raises(InvalidParameterError, match="aligned"):
        _hip.axpby(12, 8, 4, 1.0, 1.0)                      # float64 needs 8 bytes, float32 four
    with pytest.raises(InvalidParameterError, match="aligned"):
        _hip.axpby(8, 10, 4, 1.0, 1.0, float64=False)
    for bad in (math.nan, math.inf):
        with pytest.raises(InvalidParameterError, match="finite"):
            _hip.axpby(8, 8, 4, bad, 1.0)
        with pytest.raises(InvalidParameterError, match="finite"):
            _hip.axpby(8, 8, 4, 1.0, bad)
    lib = _hip.load_library()
    assert lib.fe_axpby(8, 8, 4, 1.0, 1.0, 7, None) == _hip.FE_EINVAL and b"dtype" in lib.fe_last_error()
    _hip.axpby(0, 0, 0, 2.0, 1.0)                           # n == 0: a valid no-op


def test_routing_table_from_the_plan_alone():
    """``"kernel"``: float64 face-mass of tetrahedra p = 1..4 with two or more fields; everything else ``"axpby"``."""
    table = {name: measure.accumulate_route(e) for name, e in C.dg_cases()}
    kernel = sorted(n for n, r in table.items() if r == "kernel")
    want = sorted(f"facemass_{jl}_{rl}_b4_tet{p}" for jl, rl in C.FM_LAYOUTS for p in (1, 2, 3, 4))
    assert kernel == want and len(want) == 32
    assert set(table.values()) == {"kernel", "axpby"}
    for name, r in table.items():        # grad, div, div components, matapply, triangles, one field
        if name not in want:
            assert r == "axpby", name
    fm = C.face_mass(35, 4, 15, 4)
    for b in (2, 3, 5, 9):
        assert measure.accumulate_route(C.face_mass(20, 4, 10, b)) == "kernel"
    assert measure.accumulate_route(C.face_mass(56, 4, 21, 4)) == "axpby"                     # p = 5
    assert measure.accumulate_route(fm, "mfma") == "kernel" == measure.accumulate_route(fm, {"variant": "auto"})
    for forced in ("tiled", "generic", {"variant": "tiled"}, "contraction", "reduction", {"accumulate": "axpby"}):
        assert measure.accumulate_route(fm, forced) == "axpby", forced
    f32 = f.batched_einsum("ef,fij,fej->ei", [[f.array("J", ("E", 4), "float32"), f.array("R", (4, 35, 15), "float32"),
                                               f.array(f"v{k}", (4, "E", 15), "float32")] for k in range(4)])
    assert measure.accumulate_route(f32) == "axpby"
    # fields that do not share J and R go one per launch: no fused form
    apart = f.batched_einsum("ef,fij,fej->ei", [[f.array(f"J{k}", ("E", 4)), f.array("R", (4, 35, 15)),
                                                 f.array(f"v{k}", (4, "E", 15))] for k in range(2)])
    assert measure.accumulate_route(apart) == "axpby"
    for name, e in C.other_cases():
        assert measure.accumulate_route(e) == "axpby", name
    assert measure.accumulate_route(fm, {"accumulate": "kernel"}) == "kernel"
    with pytest.raises(NotImplementedError, match="no accumulating kernel"):
        measure.accumulate_route(C.grad(3, 35), {"accumulate": "kernel"})
    with pytest.raises(InvalidParameterError, match="accumulate must be"):
        measure.accumulate_route(fm, {"accumulate": "fused"})


def test_public_interface_carries_alpha_and_beta():
    for fn in (f.evaluate, feinsum.evaluate):
        params = inspect.signature(fn).parameters
        assert params["alpha"].default == 1.0 and params["beta"].default == 0.0
        assert params["alpha"].kind is inspect.Parameter.KEYWORD_ONLY
    assert f.accumulate_route is measure.accumulate_route is feinsum.accumulate_route
    for bad in ((math.nan, 0.0), (1.0, math.inf), ("x", 0.0)):
        with pytest.raises(InvalidParameterError):
            measure._check_scale(*bad)
    assert measure._check_scale(2, -0.5) == (2.0, -0.5)


def test_bind_operator_refuses_to_accumulate():
    e = C.face_mass(35, 4, 15, 4)
    with pytest.raises(NotImplementedError, match="do not accumulate"):
        f.bind_operator([(e, {})], None, alpha=2.0)
    with pytest.raises(NotImplementedError, match="do not accumulate"):
        f.evaluate_operator([(e, {})], None, beta=1.0)
    with pytest.raises(NotImplementedError, match="do not accumulate"):
        f.bind_operator([(e, {})], None, transform={"accumulate": "axpby"})
