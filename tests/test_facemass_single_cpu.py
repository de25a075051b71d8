"""Face-mass of one field on the matrix cores, as far as it goes without a device: the new kernels are in
the built library's gfx950 code object and use no scratch, and the host-side predicates that this change must not move -- which
launches take element slices, which way an accumulating evaluation takes -- keep their values for one field."""
import re
import shutil
import subprocess

import pytest

from dg import face_mass, face_mass_ifj_fe
from feinsum_amd import _hip
from feinsum_amd.measure import accepts_element_slices, accumulate_route
from test_strided_cpu import READELF, _gfx950_code_object

#: (Np, Nfp, M, nf) of the kernels with the A fragments in registers: tetrahedra p = 1..4, triangles p = 1..5
REGISTER_KERNELS = ((4, 3, 4, 4), (10, 6, 2, 4), (20, 10, 1, 4), (35, 15, 1, 4),
                    (3, 2, 8, 3), (6, 3, 6, 3), (10, 4, 5, 3), (15, 5, 4, 3), (21, 6, 3, 3))


def _kernel_notes(tmp_path):
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
        vgprs = re.search(r"\.vgpr_count:\s+(\d+)", k)
        if name and private and vgprs:
            found[name.group(1)] = (int(private.group(1)), int(vgprs.group(1)))
    return found


@pytest.mark.skipif(shutil.which(READELF) is None, reason="llvm-readelf of the ROCm toolchain not found")
def test_the_single_field_kernels_exist_and_use_no_scratch(tmp_path):
    found = _kernel_notes(tmp_path)
    wanted = []
    for Np, Nfp, M, nf in REGISTER_KERNELS:
        wanted.append(f"_ZN2fe20facemass_mfma_kernelILi{Np}ELi{Nfp}ELi{M}ELi1ELi{nf}ELb0ELb0ELb0EEE")      # static walk
        wanted.append(f"_ZN2fe25facemass_mfma_tail_kernelILi{Np}ELi{Nfp}ELi{M}ELi1ELi{nf}EEE")            # dynamic walk
    wanted.append("_ZN2fe20facemass_mfma_kernelILi56ELi21ELi1ELi1ELi4ELb1ELb1ELb0EEE")                     # p = 5: A in LDS, eight waves
    for prefix in wanted:
        names = [n for n in found if n.startswith(prefix)]
        assert len(names) == 1, (prefix, names)
        scratch, vgprs = found[names[0]]
        assert scratch == 0 and vgprs <= 256, (names[0], scratch, vgprs)
    # nothing else of one field: no prepared, accumulating or element-slice form, no ticket kernel for p = 5
    single = [n for n in found if re.match(r"_ZN2fe\d+facemass_(mfma|w8)\w*kernelILi\d+ELi\d+ELi\d+ELi1E", n)]
    assert len(single) == len(wanted), sorted(single)


def test_one_field_still_takes_no_element_slices_and_accumulates_through_axpby():
    for Np, Nfp in ((4, 3), (10, 6), (20, 10), (35, 15)):
        for expr in (face_mass(1, Np, 4, Nfp), face_mass_ifj_fe(1, Np, 4, Nfp)):
            for transform in (None, "auto", "mfma"):
                assert not accepts_element_slices(expr, transform)
                assert accumulate_route(expr, transform) == "axpby"
            with pytest.raises(NotImplementedError):
                accumulate_route(expr, {"accumulate": "kernel"})
        assert accepts_element_slices(face_mass(2, Np, 4, Nfp), "mfma") and accumulate_route(face_mass(2, Np, 4, Nfp)) == "kernel"
    assert accumulate_route(face_mass(1, 10, 3, 4)) == "axpby" and not accepts_element_slices(face_mass(1, 56, 4, 21))
