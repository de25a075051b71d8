"""Differentiating the element operators (``evaluate_differentiable(element_gradients="kernel")``),
without a device: the matcher of the weight gradient 'iq,qj,ej,ei->eq', its size rule in C and in Python, the keyword, the
argument checks of fe_weightgrad_f64, the code object's resource metadata."""

import re
import shutil
import subprocess

import pytest
import torch

import feinsum_amd as f
from feinsum_amd import _hip
from feinsum_amd.autograd import adjoint_terms, output_grad_name
from feinsum_amd.diagnostics import InvalidParameterError
from feinsum_amd.family import (WEIGHTED_WEIGHT_ADJOINT_RULE, WO_A_T, WO_P_T, match_adjoint_family, match_element_operator,
                                match_family, match_operator_adjoint, match_weighted_element_operator,
                                match_weighted_operator_weight_adjoint, weighted_element_operator_lds_bytes,
                                weighted_element_operator_supported, weighted_weight_adjoint_lds_bytes,
                                weighted_weight_adjoint_supported)
from test_weighted_element_operator_cpu import READELF, ROLE_OF, TEMPLATES, _expr, _gfx950_code_object


def _w_adjoint(subs, **kw):
    (term,) = adjoint_terms(_expr(subs, **kw), "W")
    return term.einsum


# ---- the matcher ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("subs,flags", TEMPLATES)
def test_the_weight_adjoint_of_every_forward_template_is_matched(subs, flags):
    ins = subs.split("->")[0].split(",")
    for b in (1, 4, 9):
        term = _w_adjoint(subs, Ni=20, Nq=56, Nj=35, b=b)
        assert term.b == b and "".join(term.out_idx_set) == "eq"
        plan = match_weighted_operator_weight_adjoint(term)
        assert plan is not None and plan.kind == plan.name == "weighted_w", (subs, b)
        assert plan.layout_flags == flags and plan.params == {"Ni": 20, "Nq": 56, "Nj": 35}
        # the term's operands: the forward's without W, then the output gradient
        others = [s for s in ins if ROLE_OF[s] != "W"]
        assert plan.roles == {**{ROLE_OF[s]: pos for pos, s in enumerate(others)}, "g": 3}
        assert all(row[plan.roles["g"]].name == output_grad_name(name) for row, name in zip(term.args, _expr(subs, b=b).output_names))
        assert all(row[plan.roles["u"]].name == f"u{k}" for k, row in enumerate(term.args))
        assert plan.letters["e"] == "e"


def test_renamed_letters_another_operand_order_and_one_array_in_both_operator_positions():
    P, A = f.array("P", (20, 56)), f.array("A", (56, 35))
    u, g = f.array("u", ("E", 35)), f.array(output_grad_name("_fe_out"), ("E", 20))
    plan = match_weighted_operator_weight_adjoint(f.einsum("zk,ze,ka,ae->za", g, u, P, A))
    assert plan is not None and plan.layout_flags == 0 and plan.roles == {"g": 0, "u": 1, "P": 2, "A": 3}
    assert plan.params == {"Ni": 20, "Nq": 56, "Nj": 35} and plan.letters["e"] == "z" and plan.letters["q"] == "a"
    # the Galerkin form qi,eq,qj,ej->ei: P and A are one array
    S = f.array("S", (56, 35))
    fwd = f.einsum("qi,eq,qj,ej->ei", S, f.array("W", ("E", 56)), S, f.array("u", ("E", 35)))
    (term,) = adjoint_terms(fwd, "W")
    plan = match_weighted_operator_weight_adjoint(term.einsum)
    assert plan is not None and plan.layout_flags == WO_P_T and plan.params == {"Ni": 35, "Nq": 56, "Nj": 35}
    assert plan.roles == {"P": 0, "A": 1, "u": 2, "g": 3}
    # without an output gradient's name the first reading is taken (both give the same bits)
    plain = f.einsum("iq,qj,ej,ei->eq", P, A, u, f.array("h", ("E", 20)))
    assert match_weighted_operator_weight_adjoint(plain).roles == {"P": 0, "A": 1, "u": 2, "g": 3}


def test_what_the_matcher_declines():
    P, A = f.array("P", (35, 56)), f.array("A", (56, 35))
    u, g = f.array("u", ("E", 35)), f.array("g", ("E", 35))
    s = "iq,qj,ej,ei->eq"
    assert match_weighted_operator_weight_adjoint(f.einsum(s, P, A, u, g)) is not None
    # a float32 operand
    assert match_weighted_operator_weight_adjoint(f.einsum(s, P, A, f.array("u", ("E", 35), "float32"), g)) is None
    assert match_weighted_operator_weight_adjoint(_w_adjoint("iq,eq,qj,ej->ei", dtype="float32")) is None
    # a size parameter on q, i or j; a fixed element count
    assert match_weighted_operator_weight_adjoint(f.einsum(s, f.array("P", (35, "Q")), f.array("A", ("Q", 35)), u, g)) is None
    assert match_weighted_operator_weight_adjoint(f.einsum(s, f.array("P", ("N", 56)), A, u, f.array("g", ("E", "N")))) is None
    assert match_weighted_operator_weight_adjoint(f.einsum(s, P, A, f.array("u", (1003, 35)), f.array("g", (1003, 35)))) is None
    # rows with different P, or different A
    rows = lambda names: f.batched_einsum(s, [[f.array(p, (35, 56)), f.array(a, (56, 35)), f.array(f"u{k}", ("E", 35)),   # noqa: E731
                                               f.array(f"g{k}", ("E", 35))] for k, (p, a) in enumerate(names)])
    assert match_weighted_operator_weight_adjoint(rows([("P", "A"), ("P", "A")])) is not None
    assert match_weighted_operator_weight_adjoint(rows([("P", "A"), ("Q", "A")])) is None
    assert match_weighted_operator_weight_adjoint(rows([("P", "A"), ("P", "B")])) is None
    assert match_weighted_operator_weight_adjoint(_w_adjoint("iq,eq,qj,ej->ei", b=2, names=[("P", "W", "A"), ("Q", "W", "A")])) is None
    # one array as the u and the g of a row
    assert match_weighted_operator_weight_adjoint(f.einsum(s, P, A, u, u)) is None
    # other layouts and other einsums; sizes outside the rule
    assert match_weighted_operator_weight_adjoint(f.einsum("iq,qj,ej,ei->qe", P, A, u, g)) is None
    assert match_weighted_operator_weight_adjoint(f.einsum("iq,qj,je,ei->eq", P, A, f.array("u", (35, "E")), g)) is None
    assert match_weighted_operator_weight_adjoint(f.einsum("iq,eq,qj,ej->ei", P, f.array("W", ("E", 56)), A, u)) is None
    assert match_weighted_operator_weight_adjoint(f.einsum("eq,qj,ej,ei->iq", f.array("W", ("E", 56)), A, u, g)) is None
    assert match_weighted_operator_weight_adjoint(_w_adjoint("iq,eq,qj,ej->ei", Ni=35, Nq=84, Nj=35)) is None


def test_the_other_matchers_do_not_see_these_terms():
    for subs, _ in TEMPLATES:     # (_: the forward's layout flags)
        term = _w_adjoint(subs, b=2)
        assert match_adjoint_family(term) is None and match_operator_adjoint(term) is None
        assert match_family(term) is None and match_element_operator(term) is None and match_weighted_element_operator(term) is None
        # ... and the u-adjoint is the forward kernel with P and A exchanged and transposed
        (uterm,) = adjoint_terms(_expr(subs), "u0")
        plan = match_weighted_element_operator(uterm.einsum)
        exchanged = (0 if _ & WO_A_T else WO_P_T) | (0 if _ & WO_P_T else WO_A_T)
        assert plan is not None and plan.layout_flags == exchanged and match_weighted_operator_weight_adjoint(uterm.einsum) is None


# ---- the size rule: once in C, once in Python ----------------------------------------------------------------------

def test_the_rule_in_c_is_the_rule_in_python():
    lib = _hip.load_library()
    for Ni in range(0, 66):
        for Nq in range(0, 82):
            for Nj in range(0, 66):
                assert bool(lib.fe_weightgrad_supported(Ni, Nq, Nj)) == weighted_weight_adjoint_supported(Ni, Nq, Nj), (Ni, Nq, Nj)
    assert _hip.weightgrad_supported(35, 56, 35) and not _hip.weightgrad_supported(35, 84, 35)
    assert not lib.fe_weightgrad_supported(-1, 4, 4) and not lib.fe_weightgrad_supported(4, -1, 4) and not lib.fe_weightgrad_supported(4, 4, -1)


def test_every_shape_of_the_forward_rule_is_inside():
    inside = [(ni, nq, nj) for ni in range(0, 66) for nq in range(0, 82) for nj in range(0, 66) if weighted_weight_adjoint_supported(ni, nq, nj)]
    forward = [s for s in ((ni, nq, nj) for ni in range(0, 66) for nq in range(0, 82) for nj in range(0, 66)) if weighted_element_operator_supported(*s)]
    assert set(forward) <= set(inside)
    largest = max(inside, key=lambda s: (weighted_weight_adjoint_lds_bytes(*s), s))
    assert largest == (48, 63, 48) and weighted_weight_adjoint_lds_bytes(*largest) == 81408
    assert weighted_weight_adjoint_lds_bytes(35, 56, 35) == 66048
    assert weighted_weight_adjoint_lds_bytes(48, 64, 48) == 82432 and not weighted_weight_adjoint_supported(48, 64, 48)
    assert not weighted_weight_adjoint_supported(49, 4, 4) and not weighted_weight_adjoint_supported(4, 4, 49)
    assert not weighted_weight_adjoint_supported(4, 65, 4) and not weighted_weight_adjoint_supported(0, 4, 4)
    # the forward rule is not symmetric under Ni <-> Nj: 48 of its shapes have a u-adjoint outside it, (45, 64, 33) the first
    lopsided = [s for s in forward if not weighted_element_operator_supported(s[2], s[1], s[0])]
    assert len(lopsided) == 48 and lopsided[0] == (45, 64, 33)
    assert weighted_element_operator_lds_bytes(33, 64, 45) > 81920
    for word in ("48", "64", "81920", "float64", "size parameter"):
        assert word in WEIGHTED_WEIGHT_ADJOINT_RULE


# ---- the keyword ---------------------------------------------------------------------------------------------------

def _host_arrays(E=4, Ni=35, Nq=56, Nj=35):
    z = lambda *s: torch.zeros(*s, dtype=torch.float64)   # noqa: E731
    return {"P": z(Ni, Nq), "W": z(E, Nq), "A": z(Nq, Nj), "u0": z(E, Nj)}


def test_the_keyword_takes_auto_and_kernel_only():
    e = _expr("iq,eq,qj,ej->ei")
    for bad in ("nonsense", "Kernel", None, ""):
        with pytest.raises(InvalidParameterError, match="element_gradients"):
            f.evaluate_differentiable(e, None, _host_arrays(), element_gradients=bad)
    from feinsum_amd.autograd import _Spec

    assert _Spec(e, (), None, None, None).element_gradients == "auto" and _Spec(e, (), None, None, None).operator_gradients == "auto"


def test_without_the_keyword_both_transforms_are_still_refused():
    e = _expr("iq,eq,qj,ej->ei")
    half = f.einsum("ij,ej->ei", f.array("A", (56, 35)), f.array("u", ("E", 35)))
    z = lambda *s: torch.zeros(*s, dtype=torch.float64)   # noqa: E731
    for kw in ({}, {"element_gradients": "auto"}):
        for transform in ("weighted_element_operator", {"variant": "weighted_element_operator"}):
            with pytest.raises(NotImplementedError, match="'weighted_element_operator' has no backward pass yet"):
                f.evaluate_differentiable(e, None, _host_arrays(), transform=transform, **kw)
        for transform in ("element_operator", {"variant": "element_operator"}):
            with pytest.raises(NotImplementedError, match="'element_operator' has no backward pass yet"):
                f.evaluate_differentiable(half, None, {"A": z(56, 35), "u": z(4, 35)}, transform=transform, **kw)


# ---- fe_weightgrad_f64 without a device: every call here is refused, or has no elements ----------------------------

def _call(P=8, A=8, u=8, g=8, dW=8, E=10, Ni=35, Nq=56, Nj=35, b=1, flags=0, tables=True):
    lib = _hip.load_library()
    ua = _hip._ptr_array([u] * max(b, 1)) if tables else None
    ga = _hip._ptr_array([g] * max(b, 1)) if tables else None
    rc = lib.fe_weightgrad_f64(P, A, ua, ga, dW, E, Ni, Nq, Nj, b, flags, None)
    return rc, lib.fe_last_error()


def test_the_entry_points_exist_and_are_bound_in_header_order():
    names = list(_hip.SIGNATURES)
    for name in ("fe_weightgrad_f64", "fe_weightgrad_supported"):
        assert name in _hip.SIGNATURES and hasattr(_hip.load_library(), name)
    assert names.index("fe_weightgrad_f64") == names.index("fe_weightedop_supported") + 1
    assert names.index("fe_weightgrad_supported") == names.index("fe_weightgrad_f64") + 1


def test_argument_checks_return_their_code_and_text():
    inval, unsup = _hip.FE_EINVAL, _hip.FE_EUNSUPPORTED
    for (rc, msg), code, text in (
            (_call(tables=False), inval, b"null pointer table"),
            (_call(A=0), inval, b"null device pointer"),
            (_call(P=0), inval, b"null device pointer"),
            (_call(dW=0), inval, b"null device pointer"),
            (_call(u=0), inval, b"null field pointer 0"),
            (_call(g=0), inval, b"null field pointer 0"),
            (_call(b=0), inval, b"need at least one field"),
            (_call(b=-2), inval, b"need at least one field"),
            (_call(b=9), inval, b"at most 8"),
            (_call(E=-1), inval, b"E must be >= 0"),
            (_call(Ni=0), inval, b"must be positive"),
            (_call(Nq=0), inval, b"must be positive"),
            (_call(Nj=-3), inval, b"must be positive"),
            (_call(Nq=0, E=0), inval, b"must be positive"),
            (_call(P=12), inval, b"8-byte aligned"),
            (_call(dW=12), inval, b"8-byte aligned"),
            (_call(A=20), inval, b"8-byte aligned"),
            (_call(u=12), inval, b"field 0: device pointers must be 8-byte aligned"),
            (_call(g=4, b=3), inval, b"output 0: device pointers must be 8-byte aligned"),
            (_call(g=12, E=0), inval, b"8-byte aligned"),
            (_call(flags=4), inval, b"bad operator flags 4"),
            (_call(flags=-1), inval, b"bad operator flags"),
            (_call(E=1 << 33, Ni=8, Nq=64, Nj=8), inval, b"too large"),
            (_call(E=1 << 34, Ni=32, Nq=8, Nj=8), inval, b"too large"),
            (_call(E=1 << 34, Ni=8, Nq=8, Nj=32), inval, b"too large"),
            # the order of fe_weightedop_f64: E, the extents, b, the flags, the table, alignment, ... the size rule last
            (_call(E=-1, Ni=0, b=0, flags=4, tables=False), inval, b"E must be >= 0"),
            (_call(E=-1, b=9), inval, b"E must be >= 0"),
            (_call(Ni=0, b=0, flags=4, tables=False), inval, b"must be positive"),
            (_call(Ni=0, b=9, flags=4, tables=False), inval, b"must be positive"),
            (_call(b=0, flags=4, tables=False), inval, b"need at least one field"),
            (_call(b=9, flags=4, tables=False), inval, b"at most 8"),
            (_call(b=9, E=0), inval, b"at most 8"),
            (_call(flags=4, tables=False), inval, b"bad operator flags"),
            (_call(tables=False, P=12), inval, b"null pointer table"),
            (_call(P=12, A=0, Nq=84), inval, b"8-byte aligned"),
            (_call(A=0, Nq=84), inval, b"null device pointer"),
            (_call(Nq=84), unsup, b"size rule"),
            (_call(Ni=49, Nq=4, Nj=4), unsup, b"size rule"),
            (_call(Ni=48, Nq=64, Nj=48, flags=3), unsup, b"(Ni, Nq, Nj) = (48, 64, 48)"),
            (_call(Ni=4, Nq=65, Nj=4, flags=1), unsup, b"size rule")):
        assert rc == code and text in msg and msg.startswith(b"weightgrad:"), (rc, msg, text)


def test_no_elements_is_a_no_op_whatever_else():
    ok = _hip.FE_OK
    assert _call(E=0)[0] == ok and _call(E=0, P=0, A=0, u=0, g=0, dW=0)[0] == ok and _call(E=0, b=8)[0] == ok
    assert _call(E=0, Ni=35, Nq=84, Nj=35)[0] == ok       # the size rule is the last check: no elements come before it
    assert _call(E=0, flags=3)[0] == ok


def test_the_python_wrapper_maps_the_codes():
    with pytest.raises(NotImplementedError, match="size rule"):
        _hip.weightgrad(8, 8, [8], [8], 8, 10, 35, 84, 35)
    with pytest.raises(InvalidParameterError, match="8-byte aligned"):
        _hip.weightgrad(12, 8, [8], [8], 8, 10, 35, 56, 35)
    with pytest.raises(InvalidParameterError, match="as many output gradients"):
        _hip.weightgrad(8, 8, [8, 8], [8], 8, 10, 35, 56, 35)
    _hip.weightgrad(8, 8, [8], [8], 8, 0, 35, 56, 35)


# ---- the code object: resource metadata only -----------------------------------------------------------------------

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
        vgprs, spills = re.search(r"\.vgpr_count:\s+(\d+)", k), re.search(r"\.vgpr_spill_count:\s+(\d+)", k)
        if name and private:
            found[name.group(1)] = (int(private.group(1)), int(vgprs.group(1)) if vgprs else 0, int(spills.group(1)) if spills else 0)
    mine = {n: v for n, v in found.items() if "wgrad_kernel" in n}
    assert len(mine) == 4, sorted(mine)             # RQ = 1 ... 4
    for name, (private, vgprs, spills) in mine.items():
        assert private == 0 and spills == 0, (name, private, spills)
        assert vgprs <= 256, (name, vgprs)          # (.vgpr_count is the unified total: two waves per SIMD of 512 registers)
        assert "weightedop_kernel" not in name and "elemop_kernel" not in name
    # the counts the neighbours' tests pin still hold
    assert sum("weightedop_kernel" in n for n in found) == 12 and sum("elemop_kernel" in n for n in found) == 6
