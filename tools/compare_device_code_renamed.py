#!/usr/bin/env python
"""tools/compare_device_code.py for a change that appends defaulted template arguments to a kernel, which renames every
instantiation although its code is meant to stay what it was:

    python tools/compare_device_code_renamed.py <parent.so> <child.so>

Functions that carry the same mangled name in both builds are compared as compare_device_code.py compares them
(disassembly, metadata block, kernel descriptor).  A function found in the parent only is matched to the child's function
whose demangled name is the parent's once the appended arguments are removed (``RENAMES`` below: ``contract_mfma_kernel``
and ``reduce_combine_kernel`` gained ``ACC = false`` and an empty parameter pack); its own mangled name is replaced in the
disassembly and the metadata of both before they are compared.  Exit status 0: every function of the parent is in the
child, none different."""
import re
import subprocess
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent))
import compare_device_code as cdc  # noqa: E402

# demangled child name -> demangled parent name
RENAMES = [(r"(contract_mfma_kernel<[^>]*), false>", r"\1>"), (r"(reduce_combine_kernel<[^>,]*), false>", r"\1>")]


def demangle(names):
    names = list(names)
    if not names:
        return {}
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout
    return dict(zip(names, out.splitlines()))


def as_parent(pretty_child: str) -> str:
    for pat, to in RENAMES:
        pretty_child = re.sub(pat, to, pretty_child)
    return pretty_child


def main() -> int:
    parent, child = cdc.functions(Path(sys.argv[1])), cdc.functions(Path(sys.argv[2]))
    both = sorted(set(parent) & set(child))
    different = [n for n in both if parent[n] != child[n]]
    only_p, only_c = sorted(set(parent) - set(child)), sorted(set(child) - set(parent))
    pretty = demangle(only_p + only_c + different)
    by_parent_name = {as_parent(pretty[c]): c for c in only_c}
    print(f"functions in the gfx950 code object: parent {len(parent)}, child {len(child)}; {len(both)} carry the same name in both")
    print(f"  identical in disassembly, metadata and kernel descriptor: {len(both) - len(different)};  different: {len(different)}")
    for n in different:
        print(f"    DIFFERENT {pretty[n]}")
    same, changed, gone, matched = [], [], [], set()
    for n in only_p:
        c = by_parent_name.get(pretty[n])
        if c is None:
            gone.append(n)
            continue
        matched.add(c)
        (pb, pm, pd), (cb, cm, cd) = parent[n], child[c]
        agree = (pb.replace(n, "@") == cb.replace(c, "@"), (pm or "").replace(n, "@") == (cm or "").replace(c, "@"), pd == cd)
        (same if all(agree) else changed).append((n, agree))
    print(f"renamed by an appended defaulted template argument, matched by demangled name: {len(same) + len(changed)}")
    print(f"  identical in disassembly, metadata and kernel descriptor: {len(same)};  different: {len(changed)}")
    for n, _ in same:
        print(f"    same  {pretty[n]}  ({len(parent[n][0].splitlines())} instructions)")
    for n, agree in changed:
        what = ", ".join(w for w, a in zip(("disassembly", "metadata", "descriptor"), agree) if not a)
        print(f"    DIFFERENT {pretty[n]}  [{what}]")
    print(f"only in the parent, unmatched: {len(gone)}")
    for n in gone:
        print(f"    {pretty[n]}")
    new = [c for c in only_c if c not in matched]
    print(f"new in the child: {len(new)}")
    for c in new:
        print(f"    {pretty[c]}  ({len(child[c][0].splitlines())} instructions)")
    return 0 if not (different or changed or gone) else 1


if __name__ == "__main__":
    sys.exit(main())
