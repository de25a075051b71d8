"""The accumulating grad and div kernels (``transform={"accumulate": "epilogue"}``) without a device:
the two entry points are declared and exported and check their arguments before they touch the HIP runtime, the opt-in
route follows from the einsum alone and leaves every default where it was, and the built kernels need neither scratch
nor spills."""

import math
import re
import shutil
import struct
import subprocess
from pathlib import Path

import pytest

import autograd_cases as C
import feinsum_amd as f
from feinsum_amd import _hip, measure
from feinsum_amd.diagnostics import InvalidParameterError

ROOT = Path(__file__).resolve().parents[1]
EPILOGUE = {"accumulate": "epilogue"}
READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"
ENTRIES = [("grad", _hip.grad3d_acc, "fe_grad3d_acc_f64"), ("div", _hip.div3d_acc, "fe_div3d_acc_f64")]


def test_both_symbols_are_declared_and_exported():
    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "feinsum_hip.h").read_text(), flags=re.S)
    lib = _hip.load_library()
    for _, _, sym in ENTRIES:
        assert re.search(rf"\bint {sym}\s*\(", header), sym
        assert sym in _hip.EXPORTED_SYMBOLS and hasattr(lib, sym)
    assert measure.ACCUMULATE_ROUTES == ("kernel", "axpby", "epilogue")


@pytest.mark.parametrize("name,entry,sym", ENTRIES, ids=[e[0] for e in ENTRIES])
def test_entry_points_check_their_arguments_without_gpu(name, entry, sym):
    ok = dict(E=10, Np=35, alpha=1.0, beta=1.0)
    with pytest.raises(InvalidParameterError, match="E must be"):
        entry(8, 8, 8, 8, **{**ok, "E": -1})
    for bad in (math.nan, math.inf, -math.inf):
        with pytest.raises(InvalidParameterError, match="finite"):
            entry(8, 8, 8, 8, **{**ok, "alpha": bad})
        with pytest.raises(InvalidParameterError, match="finite"):
            entry(8, 8, 8, 8, **{**ok, "beta": bad})
    for k in range(4):                                  # J, D, u, out: four bytes past an 8-byte boundary
        ptrs = [8, 8, 8, 8]
        ptrs[k] = 12
        with pytest.raises(InvalidParameterError, match="8-byte aligned"):
            entry(*ptrs, **ok)
    for k in range(4):
        ptrs = [8, 8, 8, 8]
        ptrs[k] = 0
        with pytest.raises(InvalidParameterError, match="null"):
            entry(*ptrs, **ok)
    with pytest.raises(InvalidParameterError, match="flags"):
        entry(8, 8, 8, 8, **ok, op_flags=2)
    for np_ in (56, 36, 6):                             # p = 5, a shape of no order, a triangle
        with pytest.raises(NotImplementedError, match="no accumulating kernel"):
            entry(8, 8, 8, 8, **{**ok, "Np": np_})
    lib = _hip.load_library()
    assert getattr(lib, sym)(8, 8, 8, 8, 10, 56, 0, 1.0, 1.0, None) == _hip.FE_EUNSUPPORTED
    assert name.encode() in lib.fe_last_error()
    for np_ in (4, 10, 20, 35):
        entry(0, 0, 0, 0, **{**ok, "E": 0, "Np": np_})   # E == 0: a valid no-op, no HIP call
        entry(0, 0, 0, 0, **{**ok, "E": 0, "Np": np_}, op_flags=1)


def test_routing_table_from_the_plan_alone():
    """``"epilogue"`` where it is asked for and exists -- float64 grad / div of tetrahedra p = 1..4, either operator layout,
    variant auto or mfma -- ``NotImplementedError`` where it is asked for and does not, and never by default."""
    for make in (C.grad, C.div):
        for Np in (4, 10, 20, 35):
            for d in ("rij", "rji"):
                e = make(3, Np, d)
                assert measure.accumulate_route(e, EPILOGUE) == "epilogue"
                assert measure.accumulate_route(e, {**EPILOGUE, "variant": "mfma"}) == "epilogue"
                assert measure.accumulate_route(e, {**EPILOGUE, "variant": "auto"}) == "epilogue"
                assert measure.accumulate_route(e) == "axpby" == measure.accumulate_route(e, "mfma")     # defaults unchanged
                with pytest.raises(NotImplementedError, match="no accumulating kernel"):
                    measure.accumulate_route(e, {"accumulate": "kernel"})
                for variant in ("tiled", "generic", "contraction", "reduction"):
                    with pytest.raises(NotImplementedError, match="no accumulating epilogue"):
                        measure.accumulate_route(e, {**EPILOGUE, "variant": variant})
    f32 = "float32"
    refused = [
        ("grad_tri", C.grad(2, 10)), ("div_tri", C.div(2, 6, "rji")),                             # triangles
        ("grad_p5", C.grad(3, 56)), ("div_p5", C.div(3, 56)),                                      # p = 5
        ("grad_f32", f.einsum("xre,rij,ej->xei", f.array("J", (3, 3, "E"), f32), f.array("R", (3, 35, 35), f32),
                              f.array("u", ("E", 35), f32))),
        ("div_f32", f.einsum("xre,rij,xej->ei", f.array("J", (3, 3, "E"), f32), f.array("R", (3, 20, 20), f32),
                             f.array("u", (3, "E", 20), f32))),
        ("divcomp", C.divcomp(3, 35)), ("divcomp_es", C.divcomp(3, 20, "er", "rji")),
        ("matapply", C.matapply(35)), ("matapply_plain", C.matapply(20, "ji", False)),
    ] + list(C.other_cases())
    for name, e in refused:
        with pytest.raises(NotImplementedError, match="no accumulating epilogue"):
            measure.accumulate_route(e, EPILOGUE)
        assert measure.accumulate_route(e) == "axpby", name
    for jl, rl in C.FM_LAYOUTS:                                                                    # face-mass: its route is "kernel"
        fm = C.face_mass(35, 4, 15, 4, jl, rl)
        with pytest.raises(NotImplementedError, match='"kernel"'):
            measure.accumulate_route(fm, EPILOGUE)
        assert measure.accumulate_route(fm) == "kernel"
    # the whole table of defaults is what it was: "kernel" for the fused face-mass cases, "axpby" for everything else
    table = {name: measure.accumulate_route(e) for name, e in C.dg_cases()}
    assert set(table.values()) == {"kernel", "axpby"}
    assert all(r == "kernel" for n, r in table.items() if n.startswith("facemass_") and "_b4_tet" in n and not n.endswith("5"))
    assert all(r == "axpby" for n, r in table.items() if not n.startswith("facemass_"))
    with pytest.raises(InvalidParameterError, match="accumulate must be"):
        measure.accumulate_route(C.grad(3, 35), {"accumulate": "fused"})
    with pytest.raises(NotImplementedError, match="do not accumulate"):
        f.bind_operator([(C.grad(3, 35), {})], None, transform=EPILOGUE)


def _gfx950_notes(lib: Path, tmp_path: Path) -> str:
    """The notes of the library's gfx950 code object (as tools/kernel_regs.py reads them)."""
    data = lib.read_bytes()
    start = data.find(b"__CLANG_OFFLOAD_BUNDLE__")
    assert start >= 0
    (count,) = struct.unpack_from("<Q", data, start + 24)
    off, co = start + 32, None
    for _ in range(count):
        o, size, length = struct.unpack_from("<QQQ", data, off)
        off += 24
        triple = data[off:off + length].decode()
        off += length
        if "gfx950" in triple:
            co = data[start + o:start + o + size]
    assert co is not None
    path = tmp_path / "feinsum_gfx950.co"
    path.write_bytes(co)
    return subprocess.run([READELF, "--notes", str(path)], capture_output=True, text=True, check=True).stdout


@pytest.mark.skipif(shutil.which(READELF) is None, reason="llvm-readelf of the ROCm toolchain not found")
def test_accumulating_kernels_have_no_scratch_and_no_spills(tmp_path):
    lib = Path(_hip.library_path())
    if not lib.exists():
        pytest.skip("library not built")
    seen = {}
    for block in _gfx950_notes(lib, tmp_path).split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block)
        if not name or not re.search(r"(grad3d|div3d)_(mfma|generic)_acc_kernel", name.group(1)):
            continue
        field = lambda key: int(re.search(key + r":\s+(\d+)", block).group(1))   # noqa: E731
        seen[name.group(1)] = (field(r"\.vgpr_spill_count"), field(r"\.sgpr_spill_count"), field(r"\.private_segment_fixed_size"),
                               field(r"\.vgpr_count"))
    mfma = [n for n in seen if "_mfma_acc_kernel" in n]
    # grad and div, each at p = 1..4 (div p = 4 among them), and the two one-thread-per-entry kernels
    assert len(mfma) == 8 and len(seen) == 10, sorted(seen)
    assert any("div3d_mfma_acc_kernelILi35ELi1E" in n for n in mfma)
    for n, (vspill, sspill, scratch, vgprs) in seen.items():
        assert (vspill, sspill, scratch) == (0, 0, 0), (n, vspill, sspill, scratch)
        assert vgprs <= 256, (n, vgprs)              # two blocks of four waves per CU
