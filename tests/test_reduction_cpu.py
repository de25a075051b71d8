"""The "reduction" transform without a GPU: the "auto" rule, the launches it plans, and the C ABI's host-only plan
query and workspace checks."""

import ctypes as C

import numpy as np
import pytest

import feinsum_amd as f
from feinsum_amd import _hip
from feinsum_amd.contraction import _desc, _extents, auto_picks_contraction
from feinsum_amd.diagnostics import InvalidParameterError
from feinsum_amd.measure import launch_kind
from feinsum_amd.reduction import (REDUCE_MAX_OUT, REDUCE_MIN_SUM, plan_reduction, reduce_path, split_path)

import dg

NP = 35
TABLE = {   # the einsums of a DG time step's norms, inner products and energies
    "ei,ei->": [("E", NP), ("E", NP)],
    "ej,ej->j": [("E", NP), ("E", NP)],
    "ei->i": [("E", NP)],
    "xei,xei->x": [(3, "E", NP), (3, "E", NP)],
    "ei,ej->ij": [("E", NP), ("E", NP)],
    "e,ei,ei->": [("E",), ("E", NP), ("E", NP)],
    "e,ij,ei,ej->": [("E",), (NP, NP), ("E", NP), ("E", NP)],
    "ej,e->j": [("E", NP), ("E",)],
}


def _expr(subs, dtype="float64"):
    return f.einsum(subs, *[f.array(n, s, dtype) for n, s in zip("ABCD", TABLE[subs])])


def _plan_desc(subs, E, dtype="float64"):
    expr = _expr(subs, dtype)
    ext = _extents(expr, {"E": E})

    class T:   # C-contiguous strides of a tensor of this shape, without allocating it
        def __init__(self, shape):
            self._st = tuple(int(np.prod(shape[k + 1:], dtype=np.int64)) for k in range(len(shape)))

        def stride(self):
            return self._st

    ts = [T([ext[c] for c in idx]) for idx in expr.in_idx_sets]
    return _desc(subs, ts, ext, [np.dtype(dtype)] * expr.n), ext


@pytest.mark.parametrize("subs", sorted(TABLE))
def test_auto_takes_the_reduction_at_a_million_elements(subs):
    expr = _expr(subs)
    assert launch_kind(expr, "auto", {"E": 10**6}) == "reduction"
    assert launch_kind(expr, None, {"E": 10**6}) == "reduction"
    assert launch_kind(expr, "reduction", {"E": 10**6}) == "reduction"
    assert launch_kind(expr, {"variant": "reduction"}, {"E": 10**6}) == "reduction"
    # explicit transforms keep their kernels
    assert launch_kind(expr, "generic", {"E": 10**6}) == "generic"
    assert launch_kind(expr, "contraction", {"E": 10**6}) == "contraction"


@pytest.mark.parametrize("subs", sorted(TABLE))
def test_small_element_counts_keep_todays_kernel(subs):
    expr = _expr(subs)
    want = "contraction" if auto_picks_contraction(expr, {"E": 1000}) else "generic"
    assert launch_kind(expr, "auto", {"E": 1000}) == want
    assert want == ("contraction" if subs == "ei,ej->ij" else "generic")


def test_shapes_pinned_elsewhere_keep_their_kernels():
    mv = f.einsum("ij,j->i", f.array("A", (4096, 4096)), f.array("x", (4096,)))
    red = f.einsum("ej->e", f.array("A", ("E", 64)))
    pw = f.einsum("ej,ej->ej", f.array("A", ("E", 64)), f.array("B", ("E", 64)))
    chain = f.einsum("ij,jk,kl->il", f.array("A", (512, 512)), f.array("B", (512, 512)), f.array("C", (512, 512)))
    mixed = f.einsum("ik,kj->ij", f.array("A", (512, 512), "float32"), f.array("B", (512, 512), "float64"))
    for expr in (mv, red, pw, chain, mixed):
        assert launch_kind(expr, "auto", {"E": 100000}) == "generic", expr.get_subscripts()
    erj = f.einsum("erj,rij->ei", f.array("u", ("E", 3, 35)), f.array("D", (3, 35, 35)))
    assert launch_kind(erj, "auto", {"E": 100000}) == "contraction"
    assert launch_kind(erj, "auto", {"E": 10**6}) == "contraction"
    fuller = f.einsum("bij,bjk->bik", f.array("A", ("E", 32, 16)), f.array("B", ("E", 16, 16)))
    assert launch_kind(fuller, "auto", {"E": 100000}) == "contraction"
    big = f.einsum("ik,kj->ij", f.array("A", (4096, 4000)), f.array("B", (4000, 4096)))
    assert launch_kind(big, "auto", {}) == "contraction"
    for fam in (dg.grad(), dg.div()):
        assert launch_kind(fam, "auto", {"E": 10**6}) == "family"


def test_explicit_reduction_refuses_large_outputs():
    expr = f.einsum("ej->e", f.array("A", ("E", 64)))
    assert launch_kind(expr, "reduction", {"E": REDUCE_MAX_OUT}) == "reduction"
    with pytest.raises(NotImplementedError, match="output entries"):
        launch_kind(expr, "reduction", {"E": REDUCE_MAX_OUT + 1})
    cplx = f.einsum("ei,ei->", f.array("A", ("E", 4), "complex128"), f.array("B", ("E", 4), "complex128"))
    with pytest.raises(NotImplementedError):
        launch_kind(cplx, "reduction", {"E": 10})


def test_three_operand_plans():
    (whole, how), = plan_reduction(_expr("e,ei,ei->"), {"E": 10**6})
    assert how == "reduce" and whole.result is None and len(whole.inputs) == 3
    plan = plan_reduction(_expr("e,ij,ei,ej->"), {"E": 10**6})
    assert [st.subscripts for st, _ in plan] == ["e,ei->ei", "ej,ei->ji", "ij,ji->"]
    assert [how for _, how in plan] == ["generic", "reduce", "generic"]
    ext = {"e": 10**6, "i": NP, "j": NP}
    assert split_path("ej,ei->ji", ext, ["float64"] * 2) == "mfma"


@pytest.mark.parametrize("subs", sorted(TABLE))
@pytest.mark.parametrize("E", [1000, 10**6])
def test_plan_query_runs_without_a_device_and_agrees(subs, E):
    if subs == "e,ij,ei,ej->":
        subs_launch = "ej,ei->ji"
        expr = f.einsum(subs_launch, f.array("A", ("E", NP)), f.array("B", ("E", NP)))
        ext = _extents(expr, {"E": E})

        class T:
            def stride(self):
                return (NP, 1)
        d = _desc(subs_launch, [T(), T()], ext, [np.dtype("float64")] * 2)
    else:
        subs_launch = subs
        d, ext = _plan_desc(subs, E)
    first = _hip.einsum_reduce_plan(d)
    path, slices, nbytes = first
    assert path == reduce_path(subs_launch, ext, ["float64"] * len(subs_launch.split("->")[0].split(",")))
    assert path == ("mfma" if subs_launch in ("ei,ej->ij", "ej,ei->ji") else "valu")
    assert slices >= 1 and nbytes % 256 == 0
    n_out = int(np.prod([ext[c] for c in subs_launch.split("->")[1]], dtype=np.int64))
    assert nbytes >= slices * n_out * 8
    for _ in range(3):
        assert _hip.einsum_reduce_plan(d) == first
    if E == 10**6:
        assert slices > 100   # the whole chip, not one wave


def test_plan_query_limits():
    d, _ = _plan_desc("ei->i", 10)
    d.out_extent[0] = REDUCE_MAX_OUT + 1
    with pytest.raises(NotImplementedError):
        _hip.einsum_reduce_plan(d)
    d.out_extent[0] = -1
    with pytest.raises(InvalidParameterError):
        _hip.einsum_reduce_plan(d)
    d, _ = _plan_desc("ei,ei->", 10**6, "float32")
    path, slices, nbytes = _hip.einsum_reduce_plan(d)
    assert path == "valu" and nbytes >= 4 * slices
    # an empty output: nothing to launch
    d, _ = _plan_desc("ej,ej->j", 10)
    d.out_extent[0] = 0
    assert _hip.einsum_reduce_plan(d) == ("valu", 0, 0)
    assert REDUCE_MIN_SUM == 65536


def test_reduce_rejects_a_missing_or_short_workspace_without_a_device():
    d, _ = _plan_desc("ei,ei->", 10**6)
    _, _, nbytes = _hip.einsum_reduce_plan(d)
    fake = 1 << 40   # never dereferenced: the checks come before any device work
    with pytest.raises(InvalidParameterError, match="workspace"):
        _hip.einsum_reduce(d, [fake, fake], fake, 0, nbytes, 0)
    with pytest.raises(InvalidParameterError, match="workspace"):
        _hip.einsum_reduce(d, [fake, fake], fake, fake, nbytes - 256, 0)
    with pytest.raises(InvalidParameterError, match="aligned"):
        _hip.einsum_reduce(d, [fake, fake], fake, fake + 8, nbytes, 0)
    lib = _hip.load_library()
    rc = lib.fe_einsum_reduce(C.byref(d), _hip._ptr_array([fake, fake]), fake, None, C.c_size_t(nbytes), None)
    assert rc == _hip.FE_EINVAL


def test_reduce_symbols_are_exported():
    lib = _hip.load_library()
    for name in ("fe_einsum_reduce_plan", "fe_einsum_reduce"):
        assert hasattr(lib, name)
        assert name in _hip.EXPORTED_SYMBOLS
    assert lib.fe_version() == 1000
