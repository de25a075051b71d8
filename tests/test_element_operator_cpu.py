"""The element-local operator of any shape (transform "element_operator"), without a device: the
matcher, the size rule in C and in Python, the argument checks of fe_elemop_f64, the routes, the code object."""

import re
import shutil
import struct
import subprocess
from itertools import permutations

import pytest
import torch

import feinsum_amd as f
from feinsum_amd import _hip
from feinsum_amd.diagnostics import InvalidParameterError
from feinsum_amd.family import (ELEMENT_OPERATOR_RULE, OP_TRANSPOSED, element_operator_groups, element_operator_supported,
                                match_element_operator, match_family)
from feinsum_amd.measure import accepts_element_slices, accumulate_route, launch_kind

READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"

#: the sizes the rule must accept at least: the DG pairs of the issue (interpolation, projection, p-multigrid, face nodes)
DG_PAIRS = ((56, 35), (35, 56), (84, 35), (35, 84), (60, 35), (35, 60), (20, 35), (35, 20), (10, 20), (20, 10))


def _expr(subs, Ni=56, Nj=35, b=1, dtype="float64", names=None, E="E"):
    """*subs* in the template's letters (e, i, j); *names*: per row, the array names of (J, A) -- rows share what they name alike."""
    ins = subs.split("->")[0].split(",")
    shape = {"e": (E,), "ij": (Ni, Nj), "ji": (Nj, Ni), "ej": (E, Nj)}
    rows = []
    for k in range(b):
        jn, an = names[k] if names else ("J", "A")
        label = {"e": jn, "ij": an, "ji": an, "ej": f"u{k}"}
        rows.append([f.array(label[s], shape[s], dtype) for s in ins])
    return f.batched_einsum(subs, rows)


def _renamed(subs, table):
    return "".join(table.get(ch, ch) for ch in subs)


# ---- the matcher ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("subs,flags,has_j", [("ij,ej->ei", 0, False), ("ji,ej->ei", OP_TRANSPOSED, False),
                                               ("e,ij,ej->ei", 0, True), ("e,ji,ej->ei", OP_TRANSPOSED, True)])
def test_every_template_under_every_operand_order_and_renamed_letters(subs, flags, has_j):
    lhs, rhs = subs.split("->")
    ins = lhs.split(",")
    shape = {"e": ("E",), "ij": (56, 35), "ji": (35, 56), "ej": ("E", 35)}
    for table in ({}, {"e": "k", "i": "a", "j": "e"}, {"i": "j", "j": "i"}):
        for order in permutations(range(len(ins))):
            arrays = [f.array(f"x{p}", shape[ins[p]]) for p in order]
            expr = f.einsum(_renamed(",".join(ins[p] for p in order) + "->" + rhs, table), *arrays)
            plan = match_element_operator(expr)
            assert plan is not None, (subs, table, order)
            assert plan.layout_flags == flags and plan.params == {"Ni": 56, "Nj": 35}
            assert plan.long_index == table.get("e", "e") and ("J" in plan.roles) == has_j
            role_of = {"e": "J", "ij": "A", "ji": "A", "ej": "u"}
            assert plan.roles == {role_of[ins[p]]: pos for pos, p in enumerate(order)}


def test_what_the_matcher_declines():
    A, u, J = f.array("A", (56, 35)), f.array("u", ("E", 35)), f.array("J", ("E",))
    assert match_element_operator(f.einsum("ij,ej->ei", A, u)) is not None
    # a size parameter on i or j
    assert match_element_operator(f.einsum("ij,ej->ei", f.array("A", ("N", 35)), u)) is None
    assert match_element_operator(f.einsum("ij,ej->ei", f.array("A", (56, "M")), f.array("u", ("E", "M")))) is None
    # J in a wrong shape: per entry, per node, two axes
    assert match_element_operator(f.einsum("ei,ij,ej->ei", f.array("J", ("E", 56)), A, u)) is None
    assert match_element_operator(f.einsum("i,ij,ej->ei", f.array("J", (56,)), A, u)) is None
    assert match_element_operator(f.einsum("j,ij,ej->ei", f.array("J", (35,)), A, u)) is None
    assert match_element_operator(f.einsum("ex,ij,ej->ei", f.array("J", ("E", 1)), A, u)) is None
    # other layouts of the field or the output, other einsums
    assert match_element_operator(f.einsum("ij,je->ei", A, f.array("u", (35, "E")))) is None
    assert match_element_operator(f.einsum("ij,ej->ie", A, u)) is None
    assert match_element_operator(f.einsum("ij,ij->i", f.array("A", (8, 8)), f.array("B", (8, 8)))) is None
    assert match_element_operator(f.einsum("xre,rij,ej->xei", f.array("J", (3, 3, "E")), f.array("D", (3, 35, 35)), u)) is None
    # float32 and mixed operands
    assert match_element_operator(_expr("ij,ej->ei", dtype="float32")) is None
    assert match_element_operator(f.einsum("ij,ej->ei", A, f.array("u", ("E", 35), "float32"))) is None
    assert match_element_operator(f.einsum("e,ij,ej->ei", f.array("J", ("E",), "float32"), A, u)) is None
    # sizes outside the rule
    assert match_element_operator(_expr("ij,ej->ei", Ni=97, Nj=4)) is None
    assert match_element_operator(_expr("ij,ej->ei", Ni=96, Nj=41)) is None
    assert match_element_operator(_expr("ij,ej->ei", Ni=96, Nj=40)) is not None
    # a fixed element count is fine, and square sizes without a MATAPPLY matrix-core kernel are included
    assert match_element_operator(_expr("e,ij,ej->ei", E=1003)) is not None
    assert match_element_operator(_expr("ij,ej->ei", Ni=13, Nj=13)).params == {"Ni": 13, "Nj": 13}
    assert match_element_operator(f.einsum("e,ij,ej->ei", J, A, u)).roles == {"J": 0, "A": 1, "u": 2}


def test_rows_that_share_the_operator_form_one_group():
    g = lambda e: [tuple(r) for r in element_operator_groups(match_element_operator(e), e)]   # noqa: E731
    assert g(_expr("ij,ej->ei", b=3)) == [(0, 1, 2)]
    assert g(_expr("e,ij,ej->ei", b=3)) == [(0, 1, 2)]
    assert g(_expr("ij,ej->ei", b=3, names=[("J", "A"), ("J", "B"), ("J", "B")])) == [(0,), (1, 2)]
    assert g(_expr("e,ij,ej->ei", b=3, names=[("J", "A"), ("K", "A"), ("K", "A")])) == [(0,), (1, 2)]
    # sharers that are not neighbours stay separate
    assert g(_expr("ij,ej->ei", b=3, names=[("J", "A"), ("J", "B"), ("J", "A")])) == [(0,), (1,), (2,)]
    assert g(_expr("e,ij,ej->ei", b=4, names=[("J", "A"), ("K", "A"), ("J", "A"), ("J", "A")])) == [(0,), (1,), (2, 3)]
    # without J only the operator counts
    assert g(_expr("ji,ej->ei", b=2, names=[("J", "A"), ("K", "A")])) == [(0, 1)]


# ---- the size rule: once in C, once in Python ----------------------------------------------------------------------

def test_the_rule_in_c_is_the_rule_in_python():
    lib = _hip.load_library()
    for Ni in range(-1, 130):
        for Nj in range(-1, 130):
            assert bool(lib.fe_elemop_supported(Ni, Nj)) == element_operator_supported(Ni, Nj) == _hip.elemop_supported(Ni, Nj), (Ni, Nj)


def test_the_required_sizes_are_accepted():
    assert all(element_operator_supported(Ni, Nj) for Ni in range(1, 65) for Nj in range(1, 65))
    assert all(element_operator_supported(Ni, Nj) for Ni, Nj in DG_PAIRS)
    assert not element_operator_supported(0, 5) and not element_operator_supported(5, 0) and not element_operator_supported(97, 1)
    assert not element_operator_supported(65, 64) and not element_operator_supported(1, 97)
    assert "96" in ELEMENT_OPERATOR_RULE and "64" in ELEMENT_OPERATOR_RULE and "float64" in ELEMENT_OPERATOR_RULE


# ---- fe_elemop_f64 without a device: every call here is refused, or has no elements --------------------------------

def _call(J=8, A=8, u=8, out=8, E=10, Ni=56, Nj=35, b=1, flags=0, tables=True):
    lib = _hip.load_library()
    ua = _hip._ptr_array([u] * max(b, 1)) if tables else None
    oa = _hip._ptr_array([out] * max(b, 1)) if tables else None
    rc = lib.fe_elemop_f64(J, A, ua, oa, E, Ni, Nj, b, flags, None)
    return rc, lib.fe_last_error()


def test_the_entry_points_exist_and_are_bound():
    for name in ("fe_elemop_f64", "fe_elemop_supported"):
        assert name in _hip.SIGNATURES and hasattr(_hip.load_library(), name)
    assert _hip.EXPORTED_SYMBOLS[-2:] == ("fe_elemop_f64", "fe_elemop_supported")


def test_argument_checks_return_their_code_and_text():
    inval, unsup = _hip.FE_EINVAL, _hip.FE_EUNSUPPORTED
    for (rc, msg), code, text in (
            (_call(tables=False), inval, b"null pointer table"),
            (_call(A=0), inval, b"null device pointer"),
            (_call(u=0), inval, b"null field pointer 0"),
            (_call(out=0), inval, b"null field pointer 0"),
            (_call(b=0), inval, b"need at least one field"),
            (_call(b=-2), inval, b"need at least one field"),
            (_call(E=-1), inval, b"E must be >= 0"),
            (_call(Ni=0), inval, b"must be positive"),
            (_call(Nj=-3), inval, b"must be positive"),
            (_call(Ni=0, E=0), inval, b"must be positive"),
            (_call(J=12), inval, b"8-byte aligned"),
            (_call(A=20), inval, b"8-byte aligned"),
            (_call(u=12), inval, b"field 0: device pointers must be 8-byte aligned"),
            (_call(out=4, b=3), inval, b"output 0: device pointers must be 8-byte aligned"),
            (_call(out=12, E=0), inval, b"8-byte aligned"),
            (_call(flags=2), inval, b"bad operator flags 2"),
            (_call(flags=-1), inval, b"bad operator flags"),
            (_call(E=1 << 33, Ni=64, Nj=8), inval, b"too large"),
            (_call(E=1 << 33, Ni=8, Nj=64), inval, b"too large"),
            (_call(Ni=97, Nj=4), unsup, b"size rule"),
            (_call(Ni=96, Nj=41), unsup, b"size rule"),
            (_call(Ni=65, Nj=64, J=None), unsup, b"(Ni, Nj) = (65, 64)"),
            (_call(Ni=4, Nj=128, flags=1), unsup, b"size rule")):
        assert rc == code and text in msg and msg.startswith(b"elemop:"), (rc, msg, text)


def test_no_elements_is_a_no_op_whatever_else():
    ok = _hip.FE_OK
    assert _call(E=0)[0] == ok and _call(E=0, J=None, A=0, u=0, out=0)[0] == ok and _call(E=0, b=11)[0] == ok
    assert _call(E=0, Ni=97, Nj=97)[0] == ok       # the size rule is the last check: no elements come before it
    assert _call(E=0, flags=1)[0] == ok


def test_the_python_wrapper_maps_the_codes():
    with pytest.raises(NotImplementedError, match="size rule"):
        _hip.elemop(None, 8, [8], [8], 10, 97, 4)
    with pytest.raises(InvalidParameterError, match="8-byte aligned"):
        _hip.elemop(12, 8, [8], [8], 10, 56, 35)
    with pytest.raises(InvalidParameterError, match="as many outputs"):
        _hip.elemop(None, 8, [8, 8], [8], 10, 56, 35)
    _hip.elemop(None, 8, [8], [8], 0, 56, 35)


# ---- routes --------------------------------------------------------------------------------------------------------

SIZES = {"E": 1000}


def test_the_transform_reaches_the_kernel_and_nothing_else_changes_route():
    rect, rect_j, square = _expr("ij,ej->ei"), _expr("e,ij,ej->ei"), _expr("ij,ej->ei", Ni=35, Nj=35)
    for e in (rect, rect_j, square, _expr("ji,ej->ei", b=3), _expr("e,ji,ej->ei", Ni=13, Nj=13)):
        assert launch_kind(e, "element_operator", SIZES) == "element_operator"
        assert launch_kind(e, {"variant": "element_operator", "placement": "separate"}, SIZES) == "element_operator"
    # what the parent commit answers for the same einsums
    for transform in (None, "auto"):
        assert launch_kind(rect, transform, SIZES) == "contraction"
        assert launch_kind(rect_j, transform, SIZES) == "generic"
        assert launch_kind(square, transform, SIZES) == "family"
    assert launch_kind(rect, "contraction", SIZES) == "contraction" and launch_kind(rect_j, "contraction", SIZES) == "contraction"
    assert launch_kind(rect, "generic", SIZES) == "generic" and launch_kind(rect_j, "generic", SIZES) == "generic"
    assert launch_kind(square, "generic", SIZES) == "family" and launch_kind(square, "mfma", SIZES) == "family"
    assert match_family(rect) is None and match_family(rect_j) is None and match_family(square) is not None


def test_the_transform_refuses_what_the_matcher_declines_and_names_the_rule():
    A, u = f.array("A", (56, 35)), f.array("u", ("E", 35))
    for e in (_expr("ij,ej->ei", Ni=97, Nj=4), _expr("ij,ej->ei", dtype="float32"),
              f.einsum("ij,ej->ei", A, f.array("u", ("E", 35), "float32")),
              f.einsum("ij,ij->i", f.array("A", (8, 8)), f.array("B", (8, 8))),
              f.einsum("xre,rij,ej->xei", f.array("J", (3, 3, "E")), f.array("D", (3, 35, 35)), u)):
        with pytest.raises(NotImplementedError) as exc:
            launch_kind(e, "element_operator", SIZES)
        assert ELEMENT_OPERATOR_RULE in str(exc.value) and "ELEMENT_OPERATOR_RULE" in str(exc.value)


def test_accumulation_goes_through_axpby_only():
    for e in (_expr("ij,ej->ei"), _expr("e,ij,ej->ei", b=2), _expr("ij,ej->ei", Ni=35, Nj=35)):
        assert accumulate_route(e, "element_operator") == "axpby"
        assert accumulate_route(e, {"variant": "element_operator", "accumulate": "axpby"}) == "axpby"
        for forced in ("kernel", "epilogue"):
            with pytest.raises(NotImplementedError):
                accumulate_route(e, {"variant": "element_operator", "accumulate": forced})


def test_slices_and_differentiation_are_refused():
    for e in (_expr("ij,ej->ei"), _expr("e,ij,ej->ei"), _expr("ij,ej->ei", Ni=35, Nj=35)):
        assert not accepts_element_slices(e, "element_operator")
        assert not accepts_element_slices(e, {"variant": "element_operator"})
    e = _expr("ij,ej->ei")
    arrays = {"A": torch.zeros(56, 35, dtype=torch.float64), "u0": torch.zeros(4, 35, dtype=torch.float64)}
    for transform in ("element_operator", {"variant": "element_operator"}):
        with pytest.raises(NotImplementedError, match="element_operator"):
            f.evaluate_differentiable(e, None, arrays, transform=transform)


# ---- the code object: resource metadata only -----------------------------------------------------------------------

def _gfx950_code_object(lib) -> bytes:
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
def test_the_kernels_use_no_scratch_and_fit_two_waves_per_simd(tmp_path):
    lib = _hip.library_path()
    if not lib.exists():
        pytest.skip("library not built")
    co = tmp_path / "gfx950.co"
    co.write_bytes(_gfx950_code_object(lib))
    notes = subprocess.run([READELF, "--notes", str(co)], capture_output=True, text=True, check=True).stdout
    found = {}
    for k in re.split(r"\n\s*- (?=\.agpr_count|\.args)", notes):
        name = re.search(r"\.name:\s+(\S+)", k)
        private = re.search(r"\.private_segment_fixed_size:\s+(\d+)", k)
        vgprs, agprs = re.search(r"\.vgpr_count:\s+(\d+)", k), re.search(r"\.agpr_count:\s+(\d+)", k)
        spills = re.search(r"\.vgpr_spill_count:\s+(\d+)", k)
        if name and private and "elemop_kernel" in name.group(1):
            found[name.group(1)] = (int(private.group(1)), int(vgprs.group(1)) if vgprs else 0, int(agprs.group(1)) if agprs else 0,
                                    int(spills.group(1)) if spills else 0)
    assert len(found) == 6, sorted(found)          # RT = 1 ... 6
    for name, (private, vgprs, agprs, spills) in found.items():
        assert private == 0 and spills == 0, (name, private, spills)
        assert vgprs <= 256, (name, vgprs, agprs)   # (.vgpr_count is the unified total: two waves per SIMD of 512 registers)
