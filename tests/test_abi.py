"""The C-ABI library: it loads on a CPU-only box, exports every symbol that
include/feinsum_hip.h declares, and its argument checks work without a GPU."""

import ctypes
import re
from pathlib import Path

import pytest

from feinsum_amd import _hip
from feinsum_amd.diagnostics import HipLibraryError, InvalidParameterError

ROOT = Path(__file__).resolve().parents[1]


def _declared_symbols():
    text = (ROOT / "include" / "feinsum_hip.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(fe_[a-z0-9_]+)\s*\(", text)))


def test_library_exports_every_declared_symbol():
    lib = _hip.load_library()
    declared = _declared_symbols()
    assert len(declared) >= 14
    for sym in declared:
        assert hasattr(lib, sym), f"{sym} declared in include/feinsum_hip.h but not exported"
    assert set(declared) == set(_hip.EXPORTED_SYMBOLS)


#: the ctypes type of every C type the header spells (a spelling that is not here fails the tests below)
C_TYPES = {
    "char*": ctypes.c_char_p, "const char*": ctypes.c_char_p,
    "const double*": ctypes.c_void_p, "double*": ctypes.c_void_p, "const void*": ctypes.c_void_p, "void*": ctypes.c_void_p,
    "const double* const*": ctypes.POINTER(ctypes.c_void_p), "double* const*": ctypes.POINTER(ctypes.c_void_p),
    "const void* const*": ctypes.POINTER(ctypes.c_void_p), "void**": ctypes.POINTER(ctypes.c_void_p),
    "const fe_argpack*": ctypes.POINTER(_hip.ArgPack), "const fe_einsum_desc*": ctypes.POINTER(_hip.EinsumDesc),
    "double": ctypes.c_double, "float*": ctypes.POINTER(ctypes.c_float),
    "int": ctypes.c_int, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "size_t": ctypes.c_size_t,
    "uint32_t": ctypes.c_uint32, "uint64_t": ctypes.c_uint64,
    "int32_t*": ctypes.POINTER(ctypes.c_int32), "int64_t*": ctypes.POINTER(ctypes.c_int64),
    "size_t*": ctypes.POINTER(ctypes.c_size_t), "uint64_t*": ctypes.POINTER(ctypes.c_uint64),
}


def _header_code():
    """The header without comments; ``(code without preprocessor lines, {macro: integer value})``."""
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "feinsum_hip.h").read_text(), flags=re.S)
    macros = {m.group(1): int(m.group(2), 0) for m in re.finditer(r"^#define\s+(FE_\w+)\s+(-?(?:0x[0-9a-fA-F]+|\d+))\s*$", text, flags=re.M)}
    return re.sub(r"^\s*#.*$", "", text, flags=re.M), macros


def _split_decl(decl):
    """``"const double* const* u"`` -> ``("const double* const*", "u")``: the last word is the name."""
    m = re.fullmatch(r"(.*?)(\w+)((?:\[\w+\])*)", " ".join(decl.split()))
    assert m and m.group(1).strip(), decl
    return re.sub(r"\s*\*", "*", m.group(1).strip()), m.group(2), re.findall(r"\[(\w+)\]", m.group(3))


def _ctype(spelling):
    assert spelling in C_TYPES, f"include/feinsum_hip.h spells a C type this test has no ctypes type for: {spelling!r}"
    return C_TYPES[spelling]


def _prototypes():
    """``{name: (restype, [argtypes])}`` of every ``ret name(args);`` of the header."""
    code, _ = _header_code()
    code = re.sub(r"typedef\s+struct\s+\w+\s*\{.*?\}\s*\w+\s*;", "", code, flags=re.S)
    protos = {}
    for decl in (d.strip() for d in code.replace('extern "C" {', "").split(";")):
        if "(" not in decl:
            continue
        m = re.fullmatch(r"(.*?)\b(fe_\w+)\s*\((.*)\)", decl, flags=re.S)
        assert m, f"not of the form `ret name(args)`: {decl!r}"
        ret = re.sub(r"\s*\*", "*", " ".join(m.group(1).split()))
        args = [a.strip() for a in m.group(3).split(",")]
        args = [] if args in (["void"], [""]) else args
        assert m.group(2) not in protos
        protos[m.group(2)] = (_ctype(ret), [_ctype(_split_decl(a)[0]) for a in args])
    return protos


def _struct_fields(name):
    """``[(field, ctypes type)]`` of ``typedef struct name { ... } name;`` in declaration order."""
    code, macros = _header_code()
    body = re.search(r"typedef\s+struct\s+%s\s*\{(.*?)\}\s*%s\s*;" % (name, name), code, flags=re.S).group(1)
    fields = []
    for decl in (d.strip() for d in body.split(";")):
        if not decl:
            continue
        first, *more = [x.strip() for x in decl.split(",")]     # `int32_t Np, nf, Nfp;` declares three of one type
        spelling, fname, dims = _split_decl(first)
        for fname, dims in [(fname, dims)] + [_split_decl(spelling + " " + x)[1:] for x in more]:
            ctype = _ctype(spelling)
            for d in reversed(dims):                                  # a[X][Y] is an array of X arrays of Y
                ctype = ctype * (macros[d] if d in macros else int(d))
            fields.append((fname, ctype))
    return fields


def test_signature_table_matches_the_header():
    """restype and argtypes of every function, derived from the header's prototypes through C_TYPES, are what
    ``_hip.SIGNATURES`` gives ctypes: a wrong width or a missing argument there would be silent undefined behaviour."""
    protos = _prototypes()
    assert set(protos) == set(_declared_symbols()) == set(_hip.SIGNATURES)
    assert list(protos) == list(_hip.SIGNATURES)          # the table keeps the header's order
    for name, (restype, argtypes) in protos.items():
        assert _hip.SIGNATURES[name][0] is restype, name
        assert list(_hip.SIGNATURES[name][1]) == argtypes, name
    lib = _hip.load_library()
    for name, (restype, argtypes) in protos.items():      # ... and load_library applied it
        assert getattr(lib, name).restype is restype and list(getattr(lib, name).argtypes) == argtypes, name
    assert _hip.EXPORTED_SYMBOLS == tuple(_hip.SIGNATURES)


def test_struct_mirrors_match_the_header():
    for cname, mirror in (("fe_argpack", _hip.ArgPack), ("fe_einsum_desc", _hip.EinsumDesc)):
        assert [(n, t) for n, t in mirror._fields_] == _struct_fields(cname), cname
    _, macros = _header_code()
    assert (_hip.FAMILY_F32, _hip.FAMILY_ACC) == (macros["FE_FAMILY_F32"], macros["FE_FAMILY_ACC"])
    assert (_hip.FE_MAX_EINSUM_OPERANDS, _hip.FE_MAX_EINSUM_INDICES) == (macros["FE_MAX_EINSUM_OPERANDS"],
                                                                         macros["FE_MAX_EINSUM_INDICES"])
    # alpha and beta were appended: no earlier offset moved
    assert (_hip.ArgPack.prepared.offset, _hip.ArgPack.alpha.offset, ctypes.sizeof(_hip.ArgPack)) == (112, 120, 136)


def test_an_unmapped_c_type_fails():
    with pytest.raises(AssertionError, match="no ctypes type"):
        _ctype("long double*")


def test_version_and_flop_counters():
    lib = _hip.load_library()
    assert lib.fe_version() == 1000
    assert _hip.flops_per_element(1, 35) == 7980            # grad
    assert _hip.flops_per_element(2, 35) == 7980            # div
    assert _hip.flops_per_element(3, 35) == 15960           # fused grad + div
    assert _hip.flops_per_element(4, 35, 4, 15, 4) == 17040  # face-mass x4
    assert _hip.flops_per_element(5, 35) == 7455             # div component (x3 = 22365)
    assert _hip.flops_per_element(6, 35, b=12) == 89460      # cross-product batch: 12 planes
    assert _hip.flops_per_element(7, 35, b=4) == 9940        # e,ij,ej->ei x4
    assert _hip.flops_per_element(99, 35) == -1


def test_argument_validation_without_gpu():
    # FE_EINVAL -> InvalidParameterError, FE_EUNSUPPORTED -> NotImplementedError; none of
    # these reach the HIP runtime
    with pytest.raises(InvalidParameterError, match="E must be"):
        _hip.grad3d(0, 0, 0, 0, -1, 35)
    with pytest.raises(InvalidParameterError, match="Np must be"):
        _hip.div3d(0, 0, 0, 0, 10, 0)
    with pytest.raises(InvalidParameterError, match="null"):
        _hip.grad3d(0, 0, 0, 0, 10, 35)
    with pytest.raises(NotImplementedError, match="unknown variant"):
        _hip.grad3d(8, 8, 8, 8, 10, 35, variant=7)
    with pytest.raises(InvalidParameterError, match="8-byte aligned"):
        _hip.div3d(8, 8, 12, 8, 10, 35)
    with pytest.raises(InvalidParameterError, match="operator flags"):
        _hip.grad3d(8, 8, 8, 8, 10, 35, op_flags=4)
    with pytest.raises(InvalidParameterError, match="operator flags"):
        _hip.divcomp3d(8, 8, 8, 8, 10, 35, op_flags=8)
    with pytest.raises(InvalidParameterError, match="unknown kernel variant"):
        _hip.grad3d(8, 8, 8, 8, 10, 35, variant="fastest")
    with pytest.raises(InvalidParameterError, match="layout"):
        _hip.facemass(8, 8, [8], [8], 10, 35, 4, 15, layout_flags=8)
    with pytest.raises(InvalidParameterError, match="as many outputs"):
        _hip.facemass(8, 8, [8, 8], [8], 10, 35, 4, 15)
    # E == 0 is a valid no-op for every family (no launch, no HIP call)
    _hip.grad3d(0, 0, 0, 0, 0, 35)
    _hip.div3d(0, 0, 0, 0, 0, 35)
    _hip.facemass(0, 0, [0, 0], [0, 0], 0, 35, 4, 15)
    assert _hip.load_library().fe_last_error() is not None


def test_prepared_operator_argument_checks_without_gpu():
    with pytest.raises(InvalidParameterError, match="null"):
        _hip.prepare_operator(1, 0, 35, 0, 0, 0, 0)
    with pytest.raises(InvalidParameterError, match="aligned"):
        _hip.prepare_operator(1, 8, 35, 0, 0, 0, 24)
    with pytest.raises(NotImplementedError, match="p = 1..4"):
        _hip.prepare_operator(1, 8, 56, 0, 0, 0, 64)
    with pytest.raises(NotImplementedError, match="no prepared form"):
        _hip.prepare_operator(5, 8, 35, 0, 0, 0, 64)
    with pytest.raises(InvalidParameterError, match="flags"):
        _hip.prepare_operator(4, 8, 35, 4, 15, 1, 64)          # FE_FM_J_FE is not an operator flag
    # a buffer this process never prepared is refused before anything is launched
    lib = _hip.load_library()
    ptrs = _hip._ptr_array([8])
    rc = lib.fe_grad3d_prepared_f64(8, 8, 4096, ptrs, ptrs, 10, 35, 1, 0, 0, 0)
    assert rc == _hip.FE_EINVAL and b"fe_prepare_operator" in lib.fe_last_error()


def test_missing_library_fails_loudly(monkeypatch, tmp_path):
    monkeypatch.setenv("FEINSUM_HIP_LIB", str(tmp_path / "nope.so"))
    monkeypatch.setattr(_hip, "_lib", None)
    with pytest.raises(HipLibraryError, match="not found"):
        _hip.load_library()
    monkeypatch.undo()
    assert isinstance(_hip.load_library(), ctypes.CDLL)


def test_product_package_does_not_import_the_oracle():
    for py in (ROOT / "feinsum_amd").rglob("*.py"):
        src = py.read_text()
        assert "import oracle" not in src and "from oracle" not in src, py


def test_one_hip_runtime_whatever_the_import_order():
    """torch's wheel brings its own libamdhip64.so and asks for it by file name; this library asks for libamdhip64.so.7.  Loaded in
    the wrong order the process held TWO HIP runtimes and every launch here failed with "no ROCm-capable device is detected"
    (seen with a tool that loaded the library before anything imported torch).  load_library() imports torch first."""
    import subprocess
    import sys

    code = ("from feinsum_amd import _hip\n_hip.load_library()\nimport torch\n"
            "print(len({l.split()[-1] for l in open('/proc/self/maps') if 'libamdhip64' in l}))\n")
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=str(Path(__file__).resolve().parents[1]),
                         timeout=300)
    assert out.returncode == 0, out.stderr
    assert out.stdout.strip().splitlines()[-1] == "1", out.stdout
