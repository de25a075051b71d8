"""The DG family kernels, the two adjoint kernels and the two operator-gradient kernels with their operands at every accepted address offset
(tools/fuzz_dg.py ``run_placement``, tools/fuzz_autograd.py ``run_kernels(placement=...)``): each array sits 0 or 8
bytes (float64), 0, 4, 8 or 12 bytes (float32) past a 256-byte boundary, inputs between NaN bands, outputs between
sentinel bands; one array shifted at a time, all of them, and a random mix, against the aligned launch.

- a launch that is accepted aligned is accepted at every placement;
- exact data: every result bitwise the int64 einsum of the mantissas, near overflow and in the subnormal range too;
- signed data: the error bound, and float64 results bitwise those of the aligned launch;
- no NaN from behind an input (``leak:``), every input buffer bitwise unchanged, every output guard intact.

Each test prints its per-bucket report (run with ``-s`` to see it)."""

import sys
from pathlib import Path

import pytest

from test_dg_placement_cpu import SEED

sys.path.insert(0, str(Path(__file__).resolve().parents[1] / "tools"))
import fuzz_autograd as A  # noqa: E402
import fuzz_dg as D  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


@pytest.fixture(scope="module", autouse=True)
def _leave_the_device_as_found(torch_cuda):
    """Give torch's cached blocks back to the driver when the module ends (later modules start from what they did)."""
    yield
    import gc

    gc.collect()
    torch_cuda.cuda.synchronize()
    torch_cuda.cuda.empty_cache()


def _check(st, minimums):
    print("\n" + st.report(), flush=True)
    assert st.failures == 0, st.report()
    assert st.exact_runs > 0 and st.exact_equal == st.exact_runs
    assert st.cov["leak:nan-entries"] == 0
    assert not D.missing_buckets(st.cov, minimums), D.missing_buckets(st.cov, minimums)


@pytest.mark.timeout(300)
def test_exact_data_at_every_placement(torch_cuda):
    _check(D.run_placement(SEED, "exact"), D.PLACEMENT_MINIMUMS["exact"])


@pytest.mark.timeout(300)
def test_signed_data_bitwise_equal_to_the_aligned_launch(torch_cuda):
    _check(D.run_placement(SEED, "signed"), D.PLACEMENT_MINIMUMS["signed"])


@pytest.mark.timeout(300)
def test_large_tails_with_shifted_operands(torch_cuda):
    _check(D.run_placement(SEED, "large"), {**D.PLACEMENT_MINIMUMS["large"], "walk:static": 4, "quarter_tail": 4,
                                            "walk:dynamic": 2})


@pytest.mark.timeout(300)
def test_adjoint_kernels_at_every_placement(torch_cuda):
    """"aligned" and "all" on every run of the subset, each "only:" placement on every third run (in turn, so that the
    six of them together reach every run twice)."""
    geom, fm = A.placement_kernel_runs(SEED)
    og, ogfm = A.placement_opgrad_runs(SEED)      # the operator-gradient kernels, their workspace embedded like an output
    total = A.Stats("adjoint kernels, placements")
    for k, placement in enumerate(A.KERNEL_PLACEMENTS):
        every = placement in ("aligned", "all")
        st = A.run_kernels(SEED, geom if every else geom[k % 3::3], fm if every else fm[k % 3::3], placement=placement,
                           og_runs=og if every else og[k % 3::3], ogfm_runs=ogfm if every else ogfm[k % 3::3])
        total.failures += st.failures
        total.exact_runs += st.exact_runs
        total.exact_equal += st.exact_equal
        total.cov.update(st.cov)
    total.cov["leak:nan-entries"] += 0
    layouts = {f"geomadj:{lay}": 8 for lay in A.GEOM_LAYOUTS}
    layouts.update({f"facemass_adj:{jl},{rl}": 8 for jl, rl, _ in A.FM_LAYOUT_FLAGS})
    layouts.update({f"opgrad:{lay},{ol}": 8 for lay in A.GEOM_LAYOUTS for ol in A.OPGRAD_OUT_LAYOUTS})
    layouts.update({f"opgrad_fm:{jl},{rl}": 4 for jl, rl, _ in A.FM_LAYOUT_FLAGS})
    _check(total, {**{f"place:{p}": 40 + 15 for p in A.KERNEL_PLACEMENTS}, **layouts, "place:aligned": 120 + 48, "place:all": 120 + 48,
                   "facemass_adj:b1": 20, "facemass_adj:b2": 20, "facemass_adj:b4": 20, "facemass_adj:b9": 9,
                   "opgrad_fm:b1": 16, "opgrad_fm:b2": 16, "opgrad_fm:b4": 16, "opgrad_fm:b9": 16, "opgrad:workspace": 192,
                   **{f"opgrad:E{E}": 8 for E in A.OPGRAD_E}})
