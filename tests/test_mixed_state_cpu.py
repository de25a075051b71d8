"""Float32 results from the float32-field DG kernels (transform ``"mixed_state"``) without a device: the
rule and the launch kind, what is refused, the accumulate route, the three entry points and what they answer before any device
work, and that the new kernels of the built library use no scratch."""

import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import feinsum_amd as f
from feinsum_amd import _hip
from feinsum_amd.diagnostics import InvalidParameterError
from feinsum_amd.family import MIXED_FAMILY_RULE, match_family, match_mixed_family
from feinsum_amd.measure import accepts_element_slices, accumulate_route, launch_kind, result_dtype
from test_dg_mixed_cpu import ACCEPTED, REFUSED, TETS, mixed_einsum
from test_strided_cpu import READELF, _gfx950_code_object

ENTRIES = ("fe_grad3d_mixed_state_f64", "fe_div3d_mixed_state_f64", "fe_facemass_mixed_state_f64")


@pytest.mark.parametrize("family,Np,layout,flags", ACCEPTED, ids=[f"{a[0]}-{a[1]}-{a[2]}" for a in ACCEPTED])
def test_the_rule_is_the_one_of_mixed_family(family, Np, layout, flags):
    for b in (1, 2, 9):
        expr = mixed_einsum(family, Np, b, layout)
        assert match_mixed_family(expr) is not None and match_family(expr) is None
        assert launch_kind(expr, "mixed_state", {"E": 1000}) == "mixed_state"
        assert launch_kind(expr, {"variant": "mixed_state"}, {"E": 1000}) == "mixed_state"
        # float32 results under this transform only; every other route and dtype is as it was
        assert result_dtype(expr, 0, "mixed_state") == np.float32 and result_dtype(expr, b - 1, {"variant": "mixed_state"}) == np.float32
        assert result_dtype(expr, 0) == np.float64 and result_dtype(expr, 0, "mixed_family") == np.float64
        assert launch_kind(expr, "mixed_family", {"E": 1000}) == "mixed_family"
        assert launch_kind(expr, "auto", {"E": 1000}) == "generic" and launch_kind(expr, None, {"E": 1000}) == "generic"
        assert launch_kind(expr, "contraction", {"E": 1000}) == "contraction"
        assert accumulate_route(expr, "mixed_state") == "axpby" and accumulate_route(expr, {"variant": "mixed_state"}) == "axpby"
        for forced in ("kernel", "epilogue"):
            with pytest.raises(NotImplementedError):
                accumulate_route(expr, {"variant": "mixed_state", "accumulate": forced})
        assert not accepts_element_slices(expr, "mixed_state")


@pytest.mark.parametrize("what,make", REFUSED, ids=[r[0] for r in REFUSED])
def test_everything_else_is_refused_by_name_of_the_rule(what, make):
    """Among them the cases the issue names: an all-float64 einsum, a float32 J, triangles, p = 5."""
    expr = make()
    with pytest.raises(NotImplementedError, match="mixed_state.*float32.*float64") as exc:
        launch_kind(expr, "mixed_state", {"E": 1000})
    assert MIXED_FAMILY_RULE in str(exc.value)
    with pytest.raises(NotImplementedError, match="mixed_state"):
        launch_kind(expr, {"variant": "mixed_state"}, {"E": 1000})


def _host_args(expr, E):
    return {a.name: torch.zeros([E if isinstance(d, f.SizeParam) else int(d) for d in a.shape],
                                dtype=getattr(torch, np.dtype(a.dtype).name)) for row in expr.args for a in row}


@pytest.mark.parametrize("family", ["grad", "div", "facemass"])
def test_a_float64_output_is_refused(family):
    """The check ``_bind`` makes of an ``out_dict`` entry, with the dtype it expects under this transform (no queue here: the
    whole call is in tests/test_gpu_mixed_state.py)."""
    from types import SimpleNamespace

    from feinsum_amd.measure import _check_tensor

    E, Np = 5, 10
    expr = mixed_einsum(family, Np, 2)
    shape = (3, E, Np) if family == "grad" else (E, Np)
    q = SimpleNamespace(torch_device=torch.device("cpu"))
    want = result_dtype(expr, 0, "mixed_state")
    with pytest.raises(InvalidParameterError, match="has dtype torch.float64, expected float32"):
        _check_tensor("_fe_out", torch.zeros(shape, dtype=torch.float64), shape, want, q)
    assert _check_tensor("_fe_out", torch.zeros(shape, dtype=torch.float32), shape, want, q) is False


def test_the_differentiable_entry_point_refuses_the_transform():
    expr = mixed_einsum("grad", 35)
    for transform in ("mixed_state", {"variant": "mixed_state"}):
        with pytest.raises(NotImplementedError, match="mixed_state"):
            f.evaluate_differentiable(expr, 0, _host_args(expr, 5), transform=transform)


def test_the_bound_launch_class_calls_the_named_entry_points():
    from feinsum_amd.measure import _MixedStateLaunch

    E = 5
    for family, entry in zip(("grad", "div", "facemass"), ENTRIES):
        expr = mixed_einsum(family, 10, 3)
        args = _host_args(expr, E)
        outs = [torch.zeros((3, E, 10) if family == "grad" else (E, 10), dtype=torch.float32) for _ in range(3)]
        bound = _MixedStateLaunch(match_mixed_family(expr), expr, args, outs)
        assert bound.entry_point == entry and len(bound.calls) == 1 and bound.fields_f32
        fn, call = bound.calls[0]
        assert fn.__name__ == {"grad": "grad3d_mixed_state", "div": "div3d_mixed_state", "facemass": "facemass_mixed_state"}[family]
        assert list(call[2]) == [args[f"u{k}"].data_ptr() for k in range(3)] and list(call[3]) == [o.data_ptr() for o in outs]
        assert not hasattr(bound, "prepare_operators")


# ---- the entry points, no device ------------------------------------------------------------------------------------------

def _call(entry, J=8, op=8, v=8, out=8, E=10, Np=35, nf=4, Nfp=15, b=2, flags=0):
    lib = _hip.load_library()
    va, oa = _hip._ptr_array([v] * max(b, 1)), _hip._ptr_array([out] * max(b, 1))
    if "facemass" in entry:
        rc = getattr(lib, entry)(J, op, va, oa, E, Np, nf, Nfp, b, flags, None)
    else:
        rc = getattr(lib, entry)(J, op, va, oa, E, Np, b, flags, None)
    return rc, lib.fe_last_error()


def test_the_symbols_are_in_the_header_the_library_and_the_signatures():
    from pathlib import Path

    header = (Path(__file__).resolve().parents[1] / "include" / "feinsum_hip.h").read_text()
    for name in ENTRIES:
        assert re.search(rf"\bint {name}\(", header), name
        assert name in _hip.SIGNATURES and name in _hip.EXPORTED_SYMBOLS and hasattr(_hip.load_library(), name)
    assert _hip.SIGNATURES[ENTRIES[0]] == _hip.SIGNATURES["fe_grad3d_mixed_f64"]
    assert _hip.SIGNATURES[ENTRIES[1]] == _hip.SIGNATURES["fe_div3d_mixed_f64"]
    assert _hip.SIGNATURES[ENTRIES[2]] == _hip.SIGNATURES["fe_facemass_mixed_f64"]


@pytest.mark.parametrize("entry", ENTRIES)
def test_the_scope_comes_first_then_the_alignment(entry):
    for Np in (56, 3, 21, 36):
        rc, msg = _call(entry, Np=Np, v=6, out=6, J=12)        # out of scope AND misaligned: the scope is named
        assert rc == _hip.FE_EUNSUPPORTED and b"p = 1..4" in msg, (Np, msg)
    if "facemass" in entry:
        assert _call(entry, Nfp=10)[0] == _hip.FE_EUNSUPPORTED and _call(entry, nf=3)[0] == _hip.FE_EUNSUPPORTED
    for bad in (9, 10, 11, 6):
        rc, msg = _call(entry, v=bad)
        assert rc == _hip.FE_EINVAL and b"field 0 must be 4-byte aligned" in msg, (bad, msg)
        rc, msg = _call(entry, out=bad)
        assert rc == _hip.FE_EINVAL and b"output 0 must be 4-byte aligned" in msg, (bad, msg)
    for ok in (4, 12, 16):                                     # a float32 array needs 4 bytes and no more
        assert _call(entry, v=ok, out=ok, E=0)[0] == _hip.FE_OK
    for key in ("J", "op"):
        rc, msg = _call(entry, **{key: 12})
        assert rc == _hip.FE_EINVAL and b"8-byte aligned" in msg, (key, msg)
    assert _call(entry, E=0, J=0, op=0, v=0, out=0, b=3)[0] == _hip.FE_OK          # no elements: nothing is launched
    assert _call(entry, E=-1)[0] == _hip.FE_EINVAL and _call(entry, b=0)[0] == _hip.FE_EINVAL
    assert _call(entry, flags=8)[0] == _hip.FE_EINVAL
    rc, msg = _call(entry, J=0)
    assert rc == _hip.FE_EINVAL and b"null device pointer" in msg, msg


# ---- the new kernels use no scratch ---------------------------------------------------------------------------------------

@pytest.mark.skipif(shutil.which(READELF) is None, reason="llvm-readelf of the ROCm toolchain not found")
def test_the_float32_result_kernels_use_no_scratch(tmp_path):
    lib = _hip.library_path()
    if not lib.exists():
        pytest.skip("library not built")
    co = tmp_path / "gfx950.co"
    co.write_bytes(_gfx950_code_object(lib))
    notes = subprocess.run([READELF, "--notes", str(co)], capture_output=True, text=True, check=True).stdout
    scratch, spills = {}, {}
    for k in re.split(r"\n\s*- (?=\.agpr_count|\.args)", notes):
        name = re.search(r"\.name:\s+(\S+)", k)
        private = re.search(r"\.private_segment_fixed_size:\s+(\d+)", k)
        spill = re.search(r"\.vgpr_spill_count:\s+(\d+)", k)
        # (Itanium mangling: the kernels' last template argument, OUT, is `f` for float and `d` for double)
        if name and private and re.search(r"(grad3d|div3d|facemass)_mixed_kernelI\w*Lb[01]EfEE", name.group(1)):
            scratch[name.group(1)] = int(private.group(1))
            spills[name.group(1)] = int(spill.group(1)) if spill else 0
    # p = 1..4, both forms of the field loads (the store form is a kernel argument): 24 kernels
    for fam in ("grad3d", "div3d", "facemass"):
        assert sum(fam in n for n in scratch) == 8, sorted(scratch)
    assert all(v == 0 for v in scratch.values()), {n: v for n, v in scratch.items() if v}
    assert all(v == 0 for v in spills.values()), {n: v for n, v in spills.items() if v}
