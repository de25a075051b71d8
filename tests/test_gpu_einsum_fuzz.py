"""Random einsums outside the DG families through every transform that accepts them ("generic", "contraction",
"reduction", "auto", and an explicit left-to-right schedule for three or more operands), and through the C ABI entry
points on torch views, against the references of oracle/einsum_ref.py (tools/fuzz_einsum.py):

- exact data: every result bitwise equal to the int64 einsum of the mantissas (any missing, duplicated or misindexed
  term, lost sign or float32 rounding in a float64 path fails);
- signed uniform data: ``|got - ref| <= gamma(n, u) absref`` entrywise;
- NaN-filled outputs between sentinel guard bands (a missed or a stray write fails);
- a minimum number of runs on every path (generic, contraction, split-K and VALU split reductions), dtype mix,
  operand count and layout.

Each test prints its per-bucket report (run with ``-s`` to see it)."""

import sys
from pathlib import Path

import pytest

from test_einsum_fuzz_cpu import N_BOUNDED, N_DESC, N_EXACT, SEED

sys.path.insert(0, str(Path(__file__).resolve().parents[1] / "tools"))
import fuzz_einsum as F  # noqa: E402

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
    assert not F.missing_buckets(st.cov, minimums), F.missing_buckets(st.cov, minimums)


@pytest.mark.timeout(600)
def test_exact_data_every_transform(torch_cuda):
    st = F.run_exact(N_EXACT, SEED)
    assert st.exact_runs > 0 and st.exact_equal == st.exact_runs
    assert st.without_wide_entry == 0
    _check(st, F.MINIMUMS)


@pytest.mark.timeout(300)
def test_error_bound_every_transform(torch_cuda):
    st = F.run_bounded(N_BOUNDED, SEED)
    _check(st, {k: 5 for k in ("path:generic", "path:contraction", "path:reduction-valu-Esummed",
                               "path:reduction-valu-Ekept", "dtype:float32", "dtype:mixed", "dtype:float64",
                               "ops:1", "ops:2", "ops:3+")})


@pytest.mark.timeout(300)
def test_descriptors_on_views(torch_cuda):
    st = F.run_descriptors(N_DESC, SEED)
    assert st.exact_runs > 0 and st.exact_equal == st.exact_runs
    _check(st, F.DESC_MINIMUMS)
