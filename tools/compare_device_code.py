#!/usr/bin/env python
"""Compare the gfx950 device code of two builds of the library, function by function:

    python tools/compare_device_code.py <parent.so> <child.so>

Per function of the code object (extracted as tools/disasm_kernel.py does): the disassembly (llvm-objdump -d
--no-show-raw-insn, address comments stripped), the kernel's block of the AMDGPU metadata note and the 64-byte kernel
descriptor (<name>.kd) with kernel_code_entry_byte_offset zeroed -- it depends on where the kernel lies in the code object,
and the order of the functions may differ.  Exit status 0: the same functions in both, none different."""
import re
import struct
import subprocess
import sys
import tempfile
from pathlib import Path

LLVM = Path("/opt/rocm/lib/llvm/bin")


def code_object(lib: Path) -> bytes:
    data = lib.read_bytes()
    start = data.find(b"__CLANG_OFFLOAD_BUNDLE__")
    (count,) = struct.unpack_from("<Q", data, start + 24)
    off = start + 32
    for _ in range(count):
        o, size, length = struct.unpack_from("<QQQ", data, off)
        off += 24
        triple = data[off:off + length].decode()
        off += length
        if "gfx950" in triple:
            return data[start + o:start + o + size]
    raise SystemExit(f"{lib}: no gfx950 code object")


def run(tool: str, *args: str) -> str:
    return subprocess.run([str(LLVM / tool), *args], capture_output=True, text=True, check=True).stdout


def functions(lib: Path) -> dict:
    """mangled name -> (disassembly, metadata block, kernel descriptor)"""
    co = code_object(lib)
    with tempfile.NamedTemporaryFile(suffix=".co") as tmp:
        tmp.write(co)
        tmp.flush()
        dis = run("llvm-objdump", "-d", "--no-show-raw-insn", tmp.name)
        notes = run("llvm-readelf", "--notes", tmp.name)
        sections = run("llvm-readelf", "-S", "--wide", tmp.name)
        symbols = run("llvm-readelf", "-s", "--wide", tmp.name)
    text = {}
    for block in re.split(r"\n(?=[0-9a-f]+ <[^>]+>:)", dis):
        head, _, body = block.partition("\n")
        m = re.match(r"[0-9a-f]+ <([^>]+)>:", head)
        if m:   # (address comments: "// 000000001A2C: ..." behind every instruction)
            text[m.group(1)] = "\n".join(re.sub(r"\s*//.*$", "", ln).rstrip() for ln in body.splitlines())
    meta = {}
    for block in re.split(r"\n(?=  - \.)", notes):
        m = re.search(r"^\s+\.name:\s+(\S+)\s*$", block, re.M)
        if m and ".symbol:" in block:
            meta[m.group(1).strip("'\"")] = block.split("\namdhsa.target", 1)[0].rstrip()
    sect = []   # (address, file offset, size)
    for m in re.finditer(r"^\s*\[\s*\d+\]\s+\S+\s+\S+\s+([0-9a-f]{16})\s+([0-9a-f]+)\s+([0-9a-f]+)", sections, re.M):
        sect.append((int(m.group(1), 16), int(m.group(2), 16), int(m.group(3), 16)))
    desc = {}
    for m in re.finditer(r"^\s*\d+:\s+([0-9a-f]{16})\s+64\s+OBJECT\s+\S+\s+\S+\s+\S+\s+(\S+)\.kd\s*$", symbols, re.M):
        addr = int(m.group(1), 16)
        for a, o, size in sect:
            if a and a <= addr < a + size:
                kd = bytearray(co[o + addr - a:o + addr - a + 64])
                kd[16:24] = bytes(8)   # kernel_code_entry_byte_offset
                desc[m.group(2)] = bytes(kd)
    return {name: (body, meta.get(name), desc.get(name)) for name, body in text.items()}


def demangle(names) -> dict:
    names = list(names)
    if not names:
        return {}
    out = subprocess.run([str(LLVM / "llvm-cxxfilt")], input="\n".join(names), capture_output=True, text=True, check=True).stdout
    return dict(zip(names, out.splitlines()))


def main() -> int:
    parent, child = functions(Path(sys.argv[1])), functions(Path(sys.argv[2]))
    both = sorted(set(parent) & set(child))
    different = [n for n in both if parent[n] != child[n]]
    only_p, only_c = sorted(set(parent) - set(child)), sorted(set(child) - set(parent))
    kernels = sum(1 for n in both if parent[n][1] is not None and parent[n][2] is not None)
    print(f"functions in the gfx950 code object: parent {len(parent)}, child {len(child)}; {len(both)} carry the same name in both"
          f" ({kernels} of them kernels with a metadata block and a descriptor)")
    print(f"  identical in disassembly, metadata and kernel descriptor: {len(both) - len(different)};  different: {len(different)}")
    pretty = demangle(different + only_p + only_c)
    for title, names in (("different", different), ("only in the parent", only_p), ("only in the child", only_c)):
        print(f"{title}: {len(names)}")
        for n in names:
            what = ""
            if title == "different":
                what = "  [" + ", ".join(w for w, a, b in zip(("disassembly", "metadata", "descriptor"), parent[n], child[n]) if a != b) + "]"
            print(f"    {pretty.get(n, n)}{what}")
    return 0 if not (different or only_p or only_c) else 1


if __name__ == "__main__":
    sys.exit(main())
