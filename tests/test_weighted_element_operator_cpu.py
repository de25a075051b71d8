"""The weighted element operator 'iq,eq,qj,ej->ei' (transform "weighted_element_operator"), without a
device: the matcher, the size rule in C and in Python, the argument checks of fe_weightedop_f64, the routes, the grouping,
the refusals that come before anything is allocated, the code object's resource metadata."""

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
from feinsum_amd.family import (WEIGHTED_ELEMENT_OPERATOR_RULE, WO_A_T, WO_P_T, match_element_operator, match_family,
                                match_weighted_element_operator, weighted_element_operator_groups,
                                weighted_element_operator_lds_bytes, weighted_element_operator_supported)
from feinsum_amd.measure import accepts_element_slices, accumulate_route, launch_kind

READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"

#: (Ni, Nq, Nj) the rule must contain: the tetrahedral sandwiches, the order-changing ones, the square grid
MUST_HAVE = ((35, 56, 35), (20, 35, 20), (10, 20, 10), (4, 10, 4), (20, 56, 35), (35, 56, 20), (35, 35, 35))
#: (subscripts in the template's letters, layout flags)
TEMPLATES = (("iq,eq,qj,ej->ei", 0), ("qi,eq,qj,ej->ei", WO_P_T), ("iq,eq,jq,ej->ei", WO_A_T), ("qi,eq,jq,ej->ei", WO_P_T | WO_A_T))
ROLE_OF = {"iq": "P", "qi": "P", "eq": "W", "qj": "A", "jq": "A", "ej": "u"}


def _expr(subs, Ni=35, Nq=56, Nj=35, b=1, dtype="float64", names=None, E="E"):
    """*subs* in the template's letters (e, i, q, j); *names*: per row, the array names of (P, W, A) -- rows share what they
    name alike."""
    ins = subs.split("->")[0].split(",")
    shape = {"iq": (Ni, Nq), "qi": (Nq, Ni), "eq": (E, Nq), "qj": (Nq, Nj), "jq": (Nj, Nq), "ej": (E, Nj)}
    rows = []
    for k in range(b):
        pn, wn, an = names[k] if names else ("P", "W", "A")
        label = {"P": pn, "W": wn, "A": an, "u": f"u{k}"}
        rows.append([f.array(label[ROLE_OF[s]], shape[s], dtype) for s in ins])
    return f.batched_einsum(subs, rows)


def _renamed(subs, table):
    return "".join(table.get(ch, ch) for ch in subs)


# ---- the matcher ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("subs,flags", TEMPLATES)
def test_every_template_under_every_operand_order_and_renamed_letters(subs, flags):
    lhs, rhs = subs.split("->")
    ins = lhs.split(",")
    shape = {"iq": (20, 56), "qi": (56, 20), "eq": ("E", 56), "qj": (56, 35), "jq": (35, 56), "ej": ("E", 35)}
    for table in ({}, {"e": "k", "i": "a", "j": "e", "q": "z"}, {"i": "j", "j": "i"}, {"q": "e", "e": "q"}):
        for order in permutations(range(4)):
            arrays = [f.array(f"x{p}", shape[ins[p]]) for p in order]
            expr = f.einsum(_renamed(",".join(ins[p] for p in order) + "->" + rhs, table), *arrays)
            plan = match_weighted_element_operator(expr)
            assert plan is not None, (subs, table, order)
            assert plan.layout_flags == flags and plan.params == {"Ni": 20, "Nq": 56, "Nj": 35}
            assert plan.long_index == table.get("e", "e") and plan.name == "weighted_element_operator"
            assert plan.roles == {ROLE_OF[ins[p]]: pos for pos, p in enumerate(order)}


def test_the_galerkin_form_takes_one_array_in_both_operator_positions():
    A, W, u = f.array("A", (56, 35)), f.array("W", ("E", 56)), f.array("u", ("E", 35))
    plan = match_weighted_element_operator(f.einsum("qi,eq,qj,ej->ei", A, W, A, u))
    assert plan is not None and plan.layout_flags == WO_P_T and plan.params == {"Ni": 35, "Nq": 56, "Nj": 35}
    assert plan.roles == {"P": 0, "W": 1, "A": 2, "u": 3}
    # ... also where the grid is as large as the basis: which of the two is P is pinned by the output's letter, not by a shape
    S = f.array("S", (35, 35))
    plan = match_weighted_element_operator(f.einsum("qj,iq,eq,ej->ei", S, S, f.array("W", ("E", 35)), u))
    assert plan is not None and plan.layout_flags == 0 and plan.roles == {"A": 0, "P": 1, "W": 2, "u": 3}


def test_what_the_matcher_declines():
    P, W, A, u = f.array("P", (35, 56)), f.array("W", ("E", 56)), f.array("A", (56, 35)), f.array("u", ("E", 35))
    assert match_weighted_element_operator(f.einsum("iq,eq,qj,ej->ei", P, W, A, u)) is not None
    # a size parameter on i, q or j
    assert match_weighted_element_operator(f.einsum("iq,eq,qj,ej->ei", f.array("P", ("N", 56)), W, A, u)) is None
    assert match_weighted_element_operator(f.einsum("iq,eq,qj,ej->ei", f.array("P", (35, "Q")), f.array("W", ("E", "Q")),
                                                    f.array("A", ("Q", 35)), u)) is None
    assert match_weighted_element_operator(f.einsum("iq,eq,qj,ej->ei", P, W, f.array("A", (56, "M")), f.array("u", ("E", "M")))) is None
    # float32 and mixed operands
    assert match_weighted_element_operator(_expr("iq,eq,qj,ej->ei", dtype="float32")) is None
    assert match_weighted_element_operator(f.einsum("iq,eq,qj,ej->ei", P, W, A, f.array("u", ("E", 35), "float32"))) is None
    assert match_weighted_element_operator(f.einsum("iq,eq,qj,ej->ei", P, f.array("W", ("E", 56), "float32"), A, u)) is None
    # the three-operand forms, and section 3q's einsums
    assert match_weighted_element_operator(f.einsum("iq,eq,eq->ei", P, W, f.array("t", ("E", 56)))) is None
    assert match_weighted_element_operator(f.einsum("iq,qj,ej->ei", P, A, u)) is None
    assert match_weighted_element_operator(f.einsum("eq,qj,ej->eq", W, A, u)) is None
    assert match_weighted_element_operator(f.einsum("e,ij,ej->ei", f.array("J", ("E",)), f.array("B", (56, 35)), u)) is None
    assert match_weighted_element_operator(f.einsum("ij,ej->ei", f.array("B", (56, 35)), u)) is None
    # other layouts of the weight, the field or the output
    assert match_weighted_element_operator(f.einsum("iq,qe,qj,ej->ei", P, f.array("W", (56, "E")), A, u)) is None
    assert match_weighted_element_operator(f.einsum("iq,eq,qj,je->ei", P, W, A, f.array("u", (35, "E")))) is None
    assert match_weighted_element_operator(f.einsum("iq,eq,qj,ej->ie", P, W, A, u)) is None
    assert match_weighted_element_operator(f.einsum("iq,e,qj,ej->ei", P, f.array("W", ("E",)), A, u)) is None
    # sizes outside the rule
    assert match_weighted_element_operator(_expr("iq,eq,qj,ej->ei", Ni=35, Nq=84, Nj=35)) is None
    assert match_weighted_element_operator(_expr("iq,eq,qj,ej->ei", Ni=49, Nq=8, Nj=8)) is None
    assert match_weighted_element_operator(_expr("iq,eq,qj,ej->ei", Ni=8, Nq=8, Nj=49)) is None
    # a fixed element count is fine
    assert match_weighted_element_operator(_expr("iq,eq,qj,ej->ei", E=1003)) is not None
    # match_family, and the matcher of the two halves, do not see these einsums
    for subs, _ in TEMPLATES:
        assert match_family(_expr(subs)) is None and match_element_operator(_expr(subs)) is None


def test_rows_that_share_the_operators_and_the_weight_form_one_group():
    g = lambda e: [tuple(r) for r in weighted_element_operator_groups(match_weighted_element_operator(e), e)]   # noqa: E731
    s = "iq,eq,qj,ej->ei"
    assert g(_expr(s, b=4)) == [(0, 1, 2, 3)]
    assert g(_expr(s, b=11)) == [tuple(range(11))]            # (the library cuts a call into launches of at most 8 fields)
    assert g(_expr(s, b=3, names=[("P", "W", "A"), ("P", "V", "A"), ("P", "V", "A")])) == [(0,), (1, 2)]
    assert g(_expr(s, b=3, names=[("P", "W", "A"), ("P", "W", "B"), ("P", "W", "B")])) == [(0,), (1, 2)]
    assert g(_expr(s, b=3, names=[("P", "W", "A"), ("Q", "W", "A"), ("P", "W", "A")])) == [(0,), (1,), (2,)]
    # sharers that are not neighbours stay separate
    assert g(_expr("qi,eq,jq,ej->ei", b=4, names=[("P", "W", "A"), ("P", "V", "A"), ("P", "W", "A"), ("P", "W", "A")])) == [(0,), (1,), (2, 3)]


# ---- the size rule: once in C, once in Python ----------------------------------------------------------------------

def test_the_rule_in_c_is_the_rule_in_python():
    lib = _hip.load_library()
    for Ni in range(0, 66):
        for Nq in range(0, 82):
            for Nj in range(0, 66):
                assert bool(lib.fe_weightedop_supported(Ni, Nq, Nj)) == weighted_element_operator_supported(Ni, Nq, Nj), (Ni, Nq, Nj)
    assert _hip.weightedop_supported(35, 56, 35) and not _hip.weightedop_supported(35, 84, 35)
    assert not lib.fe_weightedop_supported(-1, 4, 4) and not lib.fe_weightedop_supported(4, -1, 4) and not lib.fe_weightedop_supported(4, 4, -1)


def test_the_required_sizes_are_accepted():
    assert all(weighted_element_operator_supported(*s) for s in MUST_HAVE)
    assert all(weighted_element_operator_supported(Ni, Nq, Nj) for Ni in range(1, 18) for Nq in range(1, 18) for Nj in range(1, 18))
    assert not weighted_element_operator_supported(35, 84, 35) and not weighted_element_operator_supported(35, 65, 35)
    assert not weighted_element_operator_supported(49, 4, 4) and not weighted_element_operator_supported(4, 4, 49)
    assert not weighted_element_operator_supported(0, 4, 4) and not weighted_element_operator_supported(4, 0, 4)
    # the LDS term is what cuts the corner of the box: both images at their largest and a W tile of 64 points
    assert weighted_element_operator_lds_bytes(35, 56, 35) == 18432 + 21504 + 4 * 898 * 8 == 68672
    assert weighted_element_operator_lds_bytes(48, 64, 48) == 81984 and not weighted_element_operator_supported(48, 64, 48)
    assert weighted_element_operator_supported(48, 64, 44) and weighted_element_operator_supported(48, 63, 48)
    for word in ("48", "64", "81920", "float64"):
        assert word in WEIGHTED_ELEMENT_OPERATOR_RULE


# ---- fe_weightedop_f64 without a device: every call here is refused, or has no elements ----------------------------

def _call(P=8, W=8, A=8, u=8, out=8, E=10, Ni=35, Nq=56, Nj=35, b=1, flags=0, tables=True):
    lib = _hip.load_library()
    ua = _hip._ptr_array([u] * max(b, 1)) if tables else None
    oa = _hip._ptr_array([out] * max(b, 1)) if tables else None
    rc = lib.fe_weightedop_f64(P, W, A, ua, oa, E, Ni, Nq, Nj, b, flags, None)
    return rc, lib.fe_last_error()


def test_the_entry_points_exist_and_are_bound_in_header_order():
    for name in ("fe_weightedop_f64", "fe_weightedop_supported"):
        assert name in _hip.SIGNATURES and hasattr(_hip.load_library(), name)
    names = list(_hip.SIGNATURES)
    assert names.index("fe_weightedop_supported") == names.index("fe_weightedop_f64") + 1
    assert (_hip.WO_P_T, _hip.WO_A_T) == (WO_P_T, WO_A_T) == (1, 2)


def test_argument_checks_return_their_code_and_text():
    inval, unsup = _hip.FE_EINVAL, _hip.FE_EUNSUPPORTED
    for (rc, msg), code, text in (
            (_call(tables=False), inval, b"null pointer table"),
            (_call(A=0), inval, b"null device pointer"),
            (_call(P=0), inval, b"null device pointer"),
            (_call(W=0), inval, b"null device pointer"),
            (_call(u=0), inval, b"null field pointer 0"),
            (_call(out=0), inval, b"null field pointer 0"),
            (_call(b=0), inval, b"need at least one field"),
            (_call(b=-2), inval, b"need at least one field"),
            (_call(E=-1), inval, b"E must be >= 0"),
            (_call(Ni=0), inval, b"must be positive"),
            (_call(Nq=0), inval, b"must be positive"),
            (_call(Nj=-3), inval, b"must be positive"),
            (_call(Nq=0, E=0), inval, b"must be positive"),
            (_call(P=12), inval, b"8-byte aligned"),
            (_call(W=12), inval, b"8-byte aligned"),
            (_call(A=20), inval, b"8-byte aligned"),
            (_call(u=12), inval, b"field 0: device pointers must be 8-byte aligned"),
            (_call(out=4, b=3), inval, b"output 0: device pointers must be 8-byte aligned"),
            (_call(out=12, E=0), inval, b"8-byte aligned"),
            (_call(flags=4), inval, b"bad operator flags 4"),
            (_call(flags=-1), inval, b"bad operator flags"),
            (_call(E=1 << 33, Ni=8, Nq=64, Nj=8), inval, b"too large"),
            (_call(E=1 << 34, Ni=32, Nq=8, Nj=8), inval, b"too large"),
            (_call(E=1 << 34, Ni=8, Nq=8, Nj=32), inval, b"too large"),
            # the order of fe_elemop_f64: E, the extents, b, the flags, the table, alignment, ... the size rule last
            (_call(E=-1, Ni=0, b=0, flags=4, tables=False), inval, b"E must be >= 0"),
            (_call(Ni=0, b=0, flags=4, tables=False), inval, b"must be positive"),
            (_call(b=0, flags=4, tables=False), inval, b"need at least one field"),
            (_call(flags=4, tables=False), inval, b"bad operator flags"),
            (_call(tables=False, P=12), inval, b"null pointer table"),
            (_call(P=12, A=0, Nq=84), inval, b"8-byte aligned"),
            (_call(A=0, Nq=84), inval, b"null device pointer"),
            (_call(Nq=84), unsup, b"size rule"),
            (_call(Ni=49, Nq=4, Nj=4), unsup, b"size rule"),
            (_call(Ni=48, Nq=64, Nj=48, flags=3), unsup, b"(Ni, Nq, Nj) = (48, 64, 48)"),
            (_call(Ni=4, Nq=65, Nj=4, flags=1), unsup, b"size rule")):
        assert rc == code and text in msg and msg.startswith(b"weightedop:"), (rc, msg, text)


def test_no_elements_is_a_no_op_whatever_else():
    ok = _hip.FE_OK
    assert _call(E=0)[0] == ok and _call(E=0, P=0, W=0, A=0, u=0, out=0)[0] == ok and _call(E=0, b=11)[0] == ok
    assert _call(E=0, Ni=35, Nq=84, Nj=35)[0] == ok       # the size rule is the last check: no elements come before it
    assert _call(E=0, flags=3)[0] == ok


def test_the_python_wrapper_maps_the_codes():
    with pytest.raises(NotImplementedError, match="size rule"):
        _hip.weightedop(8, 8, 8, [8], [8], 10, 35, 84, 35)
    with pytest.raises(InvalidParameterError, match="8-byte aligned"):
        _hip.weightedop(12, 8, 8, [8], [8], 10, 35, 56, 35)
    with pytest.raises(InvalidParameterError, match="as many outputs"):
        _hip.weightedop(8, 8, 8, [8, 8], [8], 10, 35, 56, 35)
    _hip.weightedop(8, 8, 8, [8], [8], 0, 35, 56, 35)


# ---- routes --------------------------------------------------------------------------------------------------------

SIZES = {"E": 1000}
NAME = "weighted_element_operator"


def _elemop_expr(subs, Ni=56, Nj=35):
    shape = {"e": ("E",), "ij": (Ni, Nj), "ji": (Nj, Ni), "ej": ("E", Nj)}
    name = {"e": "J", "ij": "A", "ji": "A", "ej": "u"}
    return f.einsum(subs, *[f.array(name[s], shape[s]) for s in subs.split("->")[0].split(",")])


def test_the_transform_reaches_the_kernel_and_nothing_else_changes_route():
    exprs = [_expr(subs, *shape, b=b) for (subs, _), shape, b in zip(TEMPLATES, MUST_HAVE, (1, 4, 9, 2))]
    A = f.array("A", (56, 35))
    exprs.append(f.einsum("qi,eq,qj,ej->ei", A, f.array("W", ("E", 56)), A, f.array("u", ("E", 35))))
    for e in exprs:
        assert launch_kind(e, NAME, SIZES) == NAME
        assert launch_kind(e, {"variant": NAME, "placement": "separate"}, SIZES) == NAME
        # what the parent commit answers for the same einsums
        assert launch_kind(e, None, SIZES) == "generic" and launch_kind(e, "auto", SIZES) == "generic"
        assert launch_kind(e, "generic", SIZES) == "generic" and launch_kind(e, "contraction", SIZES) == "contraction"
        with pytest.raises(NotImplementedError, match="ELEMENT_OPERATOR_RULE"):
            launch_kind(e, "element_operator", SIZES)
        with pytest.raises(NotImplementedError, match="outside the DG kernel families"):
            launch_kind(e, "mfma", SIZES)
    # ... and for the einsums of section 3q
    rect, rect_j, square = _elemop_expr("ij,ej->ei"), _elemop_expr("e,ij,ej->ei"), _elemop_expr("ij,ej->ei", 35, 35)
    for transform in (None, "auto"):
        assert launch_kind(rect, transform, SIZES) == "contraction"
        assert launch_kind(rect_j, transform, SIZES) == "generic"
        assert launch_kind(square, transform, SIZES) == "family"
    assert launch_kind(rect, "contraction", SIZES) == "contraction" and launch_kind(rect_j, "contraction", SIZES) == "contraction"
    assert launch_kind(rect, "generic", SIZES) == "generic" and launch_kind(rect_j, "generic", SIZES) == "generic"
    assert launch_kind(square, "generic", SIZES) == "family"
    for e in (rect, rect_j, square):
        assert launch_kind(e, "element_operator", SIZES) == "element_operator"
        with pytest.raises(NotImplementedError, match="WEIGHTED_ELEMENT_OPERATOR_RULE"):
            launch_kind(e, NAME, SIZES)


def test_the_transform_refuses_what_the_matcher_declines_and_names_the_rule():
    P, W, A, u = f.array("P", (35, 56)), f.array("W", ("E", 56)), f.array("A", (56, 35)), f.array("u", ("E", 35))
    for e in (_expr("iq,eq,qj,ej->ei", Nq=84), _expr("iq,eq,qj,ej->ei", dtype="float32"),
              f.einsum("iq,eq,qj,ej->ei", P, W, A, f.array("u", ("E", 35), "float32")),
              f.einsum("iq,qj,ej->ei", P, A, u),
              f.einsum("xre,rij,ej->xei", f.array("J", (3, 3, "E")), f.array("D", (3, 35, 35)), u)):
        with pytest.raises(NotImplementedError) as exc:
            launch_kind(e, NAME, SIZES)
        assert WEIGHTED_ELEMENT_OPERATOR_RULE in str(exc.value) and "WEIGHTED_ELEMENT_OPERATOR_RULE" in str(exc.value)


def test_accumulation_goes_through_axpby_only():
    for e in (_expr("iq,eq,qj,ej->ei"), _expr("qi,eq,jq,ej->ei", b=2), _expr("iq,eq,qj,ej->ei", 35, 35, 35)):
        assert accumulate_route(e, NAME) == "axpby"
        assert accumulate_route(e, {"variant": NAME, "accumulate": "axpby"}) == "axpby"
        for forced in ("kernel", "epilogue"):
            with pytest.raises(NotImplementedError):
                accumulate_route(e, {"variant": NAME, "accumulate": forced})


# ---- refusals that come before anything is allocated: host tensors never reach a device ------------------------------

def _host_arrays(E=4, Ni=35, Nq=56, Nj=35, dtype=torch.float64):
    return {"P": torch.zeros(Ni, Nq, dtype=dtype), "W": torch.zeros(E, Nq, dtype=dtype), "A": torch.zeros(Nq, Nj, dtype=dtype),
            "u0": torch.zeros(E, Nj, dtype=dtype)}


def test_slices_and_differentiation_are_refused():
    for e in (_expr("iq,eq,qj,ej->ei"), _expr("qi,eq,jq,ej->ei", b=4)):
        assert not accepts_element_slices(e, NAME) and not accepts_element_slices(e, {"variant": NAME})
    e = _expr("iq,eq,qj,ej->ei")
    for transform in (NAME, {"variant": NAME}):
        with pytest.raises(NotImplementedError, match=NAME):
            f.evaluate_differentiable(e, None, _host_arrays(), transform=transform)


def test_an_unsupported_size_and_other_dtypes_are_refused_at_bind(monkeypatch):
    from feinsum_amd import measure

    def never(*a, **k):
        raise AssertionError("an output was allocated before the refusal")

    class _HostQueue:                 # host tensors stand in for device arrays: a refusal at bind never touches them
        torch_device = torch.device("cpu")

    q = _HostQueue()
    monkeypatch.setattr(measure, "_allocate_output", never)
    monkeypatch.setattr(measure, "_as_queue", lambda cq: cq)
    monkeypatch.setattr(measure, "_check_tensor", lambda *a, **k: False)
    big = _expr("iq,eq,qj,ej->ei", Nq=84)
    with pytest.raises(NotImplementedError) as exc:
        measure._bind(big, q, _host_arrays(Nq=84), None, NAME)
    assert WEIGHTED_ELEMENT_OPERATOR_RULE in str(exc.value)
    f32 = _expr("iq,eq,qj,ej->ei", dtype="float32")
    with pytest.raises(NotImplementedError, match=NAME):
        measure._bind(f32, q, _host_arrays(dtype=torch.float32), None, NAME)
    for forced in ("kernel", "epilogue"):
        with pytest.raises(NotImplementedError):
            measure._bind(_expr("iq,eq,qj,ej->ei"), q, _host_arrays(), None, {"variant": NAME, "accumulate": forced}, alpha=2.0)


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
        if name and private and "weightedop_kernel" in name.group(1):
            found[name.group(1)] = (int(private.group(1)), int(vgprs.group(1)) if vgprs else 0, int(agprs.group(1)) if agprs else 0,
                                    int(spills.group(1)) if spills else 0)
    assert len(found) == 12, sorted(found)          # RQ = 1 ... 4 x RI = 1 ... 3
    for name, (private, vgprs, agprs, spills) in found.items():
        assert private == 0 and spills == 0, (name, private, spills)
        assert vgprs <= 256, (name, vgprs, agprs)   # (.vgpr_count is the unified total: two waves per SIMD of 512 registers)
