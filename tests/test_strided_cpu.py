"""Element slices of larger arrays, as far as they go without a device: the leading-dimension rule
``measure.element_slice_ld`` against views torch builds on the host, the byte ranges of such views against numpy index
arithmetic, the three ``fe_*_strided_f64`` entry points' argument checks, which launches take slices, and the new kernels'
code-object metadata (no scratch)."""
import re
import shutil
import struct
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

import feinsum_amd as f
from feinsum_amd import _hip
from feinsum_amd.family import FM_J_FE
from feinsum_amd.measure import (ELEMENT_SLICE_RULE, _overlap, _spans, accepts_element_slices, element_slice_ld,
                                 element_slice_spans)

READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"

#: (Np, Nfp) of tetrahedra p = 1..4
ORDERS = ((4, 3), (10, 6), (20, 10), (35, 15))


def _operand_shapes(E, Np, Nfp):
    """(shape, element axis) of every operand of the three families whose element axis can be sliced."""
    return [((3, 3, E), 2), ((E, Np), 0), ((3, E, Np), 1), ((E, 4), 0), ((4, E), 1), ((4, E, Nfp), 1)]


# ---- element_slice_ld ----------------------------------------------------------------------------------------------

def _ld_by_search(shape, strides, axis, limit=400):
    """The definition, tried out: the smallest ld >= shape[axis] for which a C-contiguous array of the shape with ld along
    *axis* has these strides (where the extent is above 1), or None."""
    for ld in range(shape[axis], limit):
        ref = torch.empty([ld if d == axis else n for d, n in enumerate(shape)]).stride()
        if all(n == 1 or st == r for n, st, r in zip(shape, strides, ref)):
            return ld
    return None


@pytest.mark.parametrize("Np,Nfp", ORDERS)
def test_narrow_along_the_element_axis_gives_the_base_extent(Np, Nfp):
    E = 11
    for shape, eaxis in _operand_shapes(E, Np, Nfp):
        base = torch.zeros(shape, dtype=torch.float64)
        assert element_slice_ld(base.shape, base.stride(), eaxis) == E          # a contiguous tensor: its own extent
        for a, n in ((0, E), (0, 5), (3, 5), (E - 1, 1), (0, 1), (4, 0), (0, 0), (E, 0), (1, E - 1)):
            v = base.narrow(eaxis, a, n)
            ld = element_slice_ld(v.shape, v.stride(), eaxis)
            if n == 0:
                assert ld == 0                                                  # no elements: nothing is addressed
            elif eaxis == 0 or v.is_contiguous():
                assert ld == n and v.is_contiguous()
            else:
                assert ld == E, (shape, a, n)
        for axis in range(len(shape)):                                          # narrow along every axis, judged along every axis
            if shape[axis] < 3:
                continue
            v = base.narrow(axis, 1, shape[axis] - 2)
            for judged in range(len(shape)):
                assert element_slice_ld(v.shape, v.stride(), judged) == _ld_by_search(v.shape, v.stride(), judged), (shape, axis, judged)
            assert element_slice_ld(v.shape, v.stride(), axis) == (shape[axis] if int(np.prod(shape[:axis])) > 1 else shape[axis] - 2)


def test_views_that_are_not_element_slices():
    base = torch.zeros((3, 12, 10), dtype=torch.float64)
    # a step is refused along the axis it was taken on (seen from a LATER axis, [:, ::2] is what narrowing the last axis of a
    # base twice as long gives: that is an element slice, of that other axis)
    for v, axes in ((base[:, ::2], (0, 1)), (base[:, 1:9:3], (0, 1)), (base[::2], (0,)), (base[:, :, ::2], (0, 1, 2)),
                    (base.transpose(0, 1), (0, 1, 2)), (base.transpose(1, 2), (0, 1, 2)), (base.permute(2, 0, 1), (0, 1, 2)),
                    (base[:, :1].expand(3, 12, 10), (0, 1, 2)), (base[:1].expand(3, 12, 10), (0, 1, 2)),
                    (base[:, 2:9, 1:], (0, 1, 2))):
        for axis in axes:
            assert element_slice_ld(v.shape, v.stride(), axis) is None, (tuple(v.shape), v.stride(), axis)
    assert element_slice_ld((3, 5, 10), (-120, 10, 1), 1) is None                # a negative stride
    assert element_slice_ld((3, 5, 10), (40, 10, 1), 1) is None                  # planes closer than the slice is long
    assert element_slice_ld((3, 5, 10), (125, 10, 1), 1) is None                 # not a multiple of the entry size
    assert element_slice_ld((3, 3, 5), (36, 12, 1), 2) == 12 and element_slice_ld((3, 3, 5), (36, 13, 1), 2) is None
    assert element_slice_ld((3, 5), (7, 1), 5) is None and element_slice_ld((3, 5), (7,), 1) is None
    contiguous = torch.zeros((4, 7, 6))
    assert [element_slice_ld(contiguous.shape, contiguous.stride(), a) for a in range(3)] == [4, 7, 6]
    assert element_slice_ld((1, 1, 5), (999, 77, 1), 2) == 5                     # extents of one say nothing, as in torch


# ---- the byte ranges of a view -------------------------------------------------------------------------------------

def _bytes_of(view: torch.Tensor, base: torch.Tensor) -> set:
    """Byte offsets (from the base's first byte) the view addresses, by numpy index arithmetic on its shape and strides."""
    idx = np.indices(tuple(view.shape)).reshape(view.dim(), -1)
    first = (view.data_ptr() - base.data_ptr()) + (np.asarray(view.stride())[:, None] * idx).sum(axis=0) * view.element_size()
    return {int(b) + k for b in first for k in range(view.element_size())}


def _bytes_of_spans(spans, base: torch.Tensor) -> set:
    return {a - base.data_ptr() + k for a, n in spans for k in range(n)}


@pytest.mark.parametrize("Np,Nfp", ORDERS[:2])
def test_span_pieces_cover_exactly_the_views_bytes(Np, Nfp):
    E = 9
    for shape, eaxis in _operand_shapes(E, Np, Nfp):
        base = torch.zeros(shape, dtype=torch.float64)
        for a, n in ((0, 4), (2, 5), (8, 1), (0, E), (3, 0)):
            v = base.narrow(eaxis, a, n)
            spans = _spans(v)
            assert _bytes_of_spans(spans, base) == _bytes_of(v, base), (shape, a, n)
            pieces = 1 if (v.is_contiguous() or n == 0) else int(np.prod(shape[:eaxis]))
            assert len(spans) == pieces, (shape, a, n, spans)
    J = torch.zeros((3, 3, 20), dtype=torch.float64).narrow(2, 3, 6)
    out = torch.zeros((3, 20, 35), dtype=torch.float64).narrow(1, 3, 6)
    assert len(_spans(J)) == 9 and len(_spans(out)) == 3
    assert element_slice_spans(1000, (3, 3, 6), 20, 2, 8)[:2] == ((1000, 48), (1160, 48))


def test_disjoint_ranges_of_one_base_do_not_overlap_and_shared_elements_do():
    for shape, eaxis in _operand_shapes(12, 10, 6):
        base = torch.zeros(shape, dtype=torch.float64)
        lo, hi, mid = base.narrow(eaxis, 0, 5), base.narrow(eaxis, 5, 7), base.narrow(eaxis, 4, 3)
        assert not _overlap(_spans(lo), _spans(hi)), shape              # adjacent
        assert _overlap(_spans(lo), _spans(mid)) and _overlap(_spans(mid), _spans(hi)), shape     # one element shared
        assert _overlap(_spans(lo), _spans(base)) and _overlap(_spans(lo), _spans(lo))
        assert not _overlap(_spans(base.narrow(eaxis, 3, 0)), _spans(base))      # no bytes share none
        assert not (_bytes_of(lo, base) & _bytes_of(hi, base)) and (_bytes_of(lo, base) & _bytes_of(mid, base))


# ---- the entry points, without a device ----------------------------------------------------------------------------

def _named(entry, *args):
    lib = _hip.load_library()
    rc = getattr(lib, entry)(*args)
    return rc, lib.fe_last_error()


def _grad(J=8, ldJ=20, D=8, u=8, out=8, ldOut=20, E=10, Np=35, b=1, flags=0):
    return _named("fe_grad3d_strided_f64", J, ldJ, D, _hip._ptr_array([u] * b), _hip._ptr_array([out] * b), ldOut, E, Np, b, flags, None)


def _div(J=8, ldJ=20, D=8, u=8, ldIn=20, out=8, E=10, Np=35, b=1, flags=0):
    return _named("fe_div3d_strided_f64", J, ldJ, D, _hip._ptr_array([u] * b), ldIn, _hip._ptr_array([out] * b), E, Np, b, flags, None)


def _fm(J=8, ldJ=20, R=8, v=8, ldIn=20, out=8, E=10, Np=35, nf=4, Nfp=15, b=2, flags=0):
    return _named("fe_facemass_strided_f64", J, ldJ, R, _hip._ptr_array([v] * b), ldIn, _hip._ptr_array([out] * b), E, Np, nf,
                  Nfp, b, flags, None)


def test_the_entry_points_exist_and_are_bound():
    for name in ("fe_grad3d_strided_f64", "fe_div3d_strided_f64", "fe_facemass_strided_f64"):
        assert name in _hip.SIGNATURES and hasattr(_hip.load_library(), name)


def test_a_leading_dimension_below_e_is_invalid():
    for rc, msg in (_grad(ldJ=9), _grad(ldOut=9), _grad(ldJ=-1), _div(ldJ=9), _div(ldIn=9), _div(ldIn=0), _fm(ldIn=9),
                    _fm(ldJ=9, flags=FM_J_FE)):
        assert rc == _hip.FE_EINVAL and b"leading dimension" in msg, msg
    # J stored ef is contiguous in a slice: ldJ is ignored -- and counts for J stored fe (E = 0: nothing reaches a device)
    assert _fm(ldJ=-1, E=0)[0] == _hip.FE_OK
    rc, msg = _fm(ldJ=-1, E=0, flags=FM_J_FE)
    assert rc == _hip.FE_EINVAL and b"leading dimension" in msg, msg


def test_a_misaligned_pointer_is_invalid():
    for rc, msg in (_grad(J=12), _grad(D=12), _grad(u=12), _grad(out=20), _div(J=4), _div(u=12), _div(out=12), _div(D=9),
                    _fm(J=12), _fm(R=12), _fm(v=12), _fm(out=12), _grad(u=12, b=3), _grad(out=12, E=0)):
        assert rc == _hip.FE_EINVAL and b"8-byte aligned" in msg, msg


def test_other_shapes_and_one_face_mass_field_are_unsupported():
    for rc, msg in (_grad(Np=56), _grad(Np=15), _grad(Np=0), _div(Np=56), _div(Np=6), _fm(Np=56, Nfp=21), _fm(Nfp=14),
                    _fm(Np=20, Nfp=15), _fm(nf=3, Np=10, Nfp=4), _fm(b=1), _fm(b=1, E=0), _grad(Np=56, ldJ=1)):
        assert rc == _hip.FE_EUNSUPPORTED and msg, msg


def test_no_elements_is_a_no_op():
    for rc, _msg in (_grad(E=0, ldJ=0, ldOut=0), _grad(E=0, J=0, D=0, u=0, out=0), _div(E=0, ldJ=5, ldIn=0), _div(E=0, b=3),
                     _fm(E=0, ldIn=0), _fm(E=0, b=9, J=0, R=0, v=0, out=0)):
        assert rc == _hip.FE_OK
    assert _grad(E=-1)[0] == _hip.FE_EINVAL and _grad(b=0)[0] == _hip.FE_EINVAL


# ---- which launches take slices ------------------------------------------------------------------------------------

def _expr(subs, Np=35, Nfp=15, b=1, dtype="float64", nf=4, ndim=3):
    shapes = {"xre": (ndim, ndim, "E"), "rij": (ndim, Np, Np), "rji": (ndim, Np, Np), "ej": ("E", Np), "xej": (ndim, "E", Np),
              "ef": ("E", nf), "fe": (nf, "E"), "fij": (nf, Np, Nfp), "ifj": (Np, nf, Nfp), "fej": (nf, "E", Nfp),
              "re": (ndim, "E")}
    ins = subs.split("->")[0].split(",")
    rows = [[f.array(f"a{pos}" if pos < 2 else f"a{pos}_{k}", shapes[s], dtype) for pos, s in enumerate(ins)] for k in range(b)]
    return f.batched_einsum(subs, rows)


GRAD, GRADT, DIV, DIVT = "xre,rij,ej->xei", "xre,rji,ej->xei", "xre,rij,xej->ei", "xre,rji,xej->ei"
LIFT, LIFT_FE = "ef,fij,fej->ei", "fe,ifj,fej->ei"


def test_which_launches_take_element_slices():
    for Np, Nfp in ORDERS:
        for subs in (GRAD, GRADT, DIV, DIVT):
            for b in (1, 3):
                assert accepts_element_slices(_expr(subs, Np, b=b))
                assert accepts_element_slices(_expr(subs, Np, b=b), "mfma") and accepts_element_slices(_expr(subs, Np, b=b), {"variant": "auto"})
        for subs in (LIFT, LIFT_FE):
            for b in (2, 4, 9):
                assert accepts_element_slices(_expr(subs, Np, Nfp, b=b), "mfma")
            assert not accepts_element_slices(_expr(subs, Np, Nfp, b=1))         # one field: the tiled kernel
    e = _expr(GRAD)
    for transform in ("generic", "tiled", "mixed_family", "contraction", "reduction", "adjoint", {"variant": "tiled"},
                      {"accumulate": "epilogue"}, {"variant": "mfma", "accumulate": "axpby"}):
        assert not accepts_element_slices(e, transform), transform
    for alpha, beta in ((2.0, 0.0), (1.0, 1.0), (0.5, -1.0)):
        assert not accepts_element_slices(e, None, alpha, beta) and not accepts_element_slices(_expr(LIFT, b=2), None, alpha, beta)
    assert not accepts_element_slices(_expr(GRAD, dtype="float32")) and not accepts_element_slices(_expr(LIFT, b=2, dtype="float32"))
    assert not accepts_element_slices(_expr(GRAD, Np=56)) and not accepts_element_slices(_expr(DIV, Np=56))      # p = 5
    assert not accepts_element_slices(_expr(GRAD, Np=10, ndim=2)) and not accepts_element_slices(_expr(DIV, Np=15, ndim=2))   # triangles
    assert not accepts_element_slices(_expr(LIFT, Np=56, Nfp=21, b=2)) and not accepts_element_slices(_expr(LIFT, Np=10, Nfp=4, nf=3, b=2))
    assert not accepts_element_slices(_expr("re,rij,ej->ei"))                    # div components
    assert not accepts_element_slices(f.einsum("ij,jk->ik", f.array("A", (8, 8)), f.array("B", (8, 8))))
    mixed = f.einsum(GRAD, f.array("J", (3, 3, "E")), f.array("D", (3, 35, 35)), f.array("u", ("E", 35), "float32"))
    assert not accepts_element_slices(mixed) and not accepts_element_slices(mixed, "mixed_family")
    assert "contiguous" in ELEMENT_SLICE_RULE and "narrow" in ELEMENT_SLICE_RULE


# ---- the new kernels use no scratch --------------------------------------------------------------------------------

def _gfx950_code_object(lib: Path) -> bytes:
    data = lib.read_bytes()
    start = data.find(b"__CLANG_OFFLOAD_BUNDLE__")
    assert start >= 0, "no offload bundle in the library"
    (count,) = struct.unpack_from("<Q", data, start + 24)
    off = start + 32
    for _ in range(count):
        o, size, length = struct.unpack_from("<QQQ", data, off)
        off += 24
        triple = data[off:off + length].decode()
        off += length
        if "gfx950" in triple:
            return data[start + o:start + o + size]
    raise AssertionError("no gfx950 code object in the library")


@pytest.mark.skipif(shutil.which(READELF) is None, reason="llvm-readelf of the ROCm toolchain not found")
def test_the_strided_kernels_use_no_scratch(tmp_path):
    lib = _hip.library_path()
    if not lib.exists():
        pytest.skip("library not built")
    co = tmp_path / "gfx950.co"
    co.write_bytes(_gfx950_code_object(lib))
    notes = subprocess.run([READELF, "--notes", str(co)], capture_output=True, text=True, check=True).stdout
    kernels = re.split(r"\n\s*- (?=\.agpr_count|\.args)", notes)
    scratch = {}
    for k in kernels:
        name = re.search(r"\.name:\s+(\S+)", k)
        private = re.search(r"\.private_segment_fixed_size:\s+(\d+)", k)
        if name and private and "_mfma_strided_" in name.group(1):
            scratch[name.group(1)] = int(private.group(1))
    families = {fam: [n for n in scratch if fam in n] for fam in ("grad3d_mfma_strided", "div3d_mfma_strided", "facemass_mfma_strided")}
    # p = 1..4, static and dynamic walk; face-mass x (2, 3, 4 fields) static and x (3, 4) dynamic
    assert len(families["grad3d_mfma_strided"]) == 8 and len(families["div3d_mfma_strided"]) == 8, sorted(scratch)
    assert len(families["facemass_mfma_strided"]) == 20, sorted(scratch)
    assert sum("strided_tail_kernel" in n for n in scratch) == 16
    assert all(v == 0 for v in scratch.values()), {n: v for n, v in scratch.items() if v}


# ---- how the fields of a launch group are gathered into launches ---------------------------------------------------

def test_fields_are_gathered_by_their_leading_dimensions():
    from feinsum_amd.family import match_family
    from feinsum_amd.measure import _StridedFamilyLaunch, _strided_runs

    n, Np, Nfp = 7, 10, 6

    def fields(subs, lengths):
        expr = _expr(subs, Np, Nfp, b=len(lengths))
        names = [[a.name for a in row] for row in expr.args]
        in_shape = (3, n, Np) if "xej" in subs else (4, n, Nfp) if "fej" in subs else (n, Np)
        axis = in_shape.index(n)
        args = {names[0][0]: torch.zeros((3, 3, 2 * n) if "xre" in subs else (n, 4), dtype=torch.float64).narrow(2 if "xre" in subs else 0, 0, n),
                names[0][1]: torch.zeros((3, Np, Np) if "rij" in subs else (4, Np, Nfp), dtype=torch.float64)}
        for k, ld in enumerate(lengths):
            args[names[k][2]] = torch.zeros([ld if d == axis else s for d, s in enumerate(in_shape)], dtype=torch.float64).narrow(axis, min(1, ld - n), n)
        return expr, args

    expr, args = fields(DIV, (9, 12, 9, 12, 9))
    plan = match_family(expr)
    outs = [torch.zeros((n, Np), dtype=torch.float64) for _ in range(5)]
    assert [(lds, rows) for _first, lds, rows in _strided_runs(plan, expr, args, outs)] == [((9, n), [0, 2, 4]), ((12, n), [1, 3])]
    assert _strided_runs(plan, expr, args, [None] * 5) == _strided_runs(plan, expr, args, outs)      # outputs yet to be allocated
    bound = _StridedFamilyLaunch(plan, expr, args, outs)            # (host tensors: nothing is launched)
    assert bound.rows == [(0, 2, 4), (1, 3)] and bound.entry_point == "fe_div3d_strided_f64"
    fn, call = bound.calls[1]
    assert call[3] == [args[expr.args[m][2].name].data_ptr() for m in (1, 3)] and call[4] == 12 and call[1] == 2 * n and call[6] == n
    # grad: the outputs' leading dimension counts too
    expr, args = fields(GRAD, (n, n))
    gouts = [torch.zeros((3, 2 * n, Np), dtype=torch.float64).narrow(1, 0, n), torch.zeros((3, 3 * n, Np), dtype=torch.float64).narrow(1, 2, n)]
    assert [(lds, rows) for _f, lds, rows in _strided_runs(match_family(expr), expr, args, gouts)] == [((n, 2 * n), [0]), ((n, 3 * n), [1])]
    # face-mass: two of each length are two launches; a field alone with its length is refused
    expr, args = fields(LIFT, (9, 12, 9, 12))
    assert [rows for _f, _l, rows in _strided_runs(match_family(expr), expr, args, [None] * 4)] == [[0, 2], [1, 3]]
    expr, args = fields(LIFT, (9, 9, 12))
    with pytest.raises(f.InvalidParameterError, match="alone in its launch group.*contiguous"):
        _strided_runs(match_family(expr), expr, args, [None] * 3)
