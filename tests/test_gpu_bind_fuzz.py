"""How a ``BatchedEinsum`` is bound to the DG family launches, on the device (tools/fuzz_bind.py): every template in
every operand order, renamed, with a concrete element axis; near misses that must not become family launches; rows
that share, repeat and outnumber one launch; every condition of the planes launch from both sides; one tensor under
two names.  Every output of every row is bitwise the int64 einsum of the row's own subscripts and arrays, the launch
shape is the predicted one, and nothing is refused that the kernel table does not refuse.

The per-bucket report is printed (run with ``-s`` to see it)."""

import sys
from pathlib import Path

import pytest

from test_bind_fuzz_cpu import N_BIND, SEED

sys.path.insert(0, str(Path(__file__).resolve().parents[1] / "tools"))
import fuzz_bind as B  # noqa: E402

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


@pytest.mark.timeout(20)
def test_bindings_every_spelling_row_table_and_alias(torch_cuda):
    """Measured on an MI355X: 2.1 s for the sweep (824 (case, transform) pairs, 797 run, 27 forced-"mfma" refusals, all
    predicted), 4.1 s for this module with its fixtures; ``test_exact_data_every_family_and_transform`` took 6.0 s
    (8.1 s) in the same session.  The limit is about three times the module's time plus interpreter start-up."""
    st = B.run_bindings(N_BIND, SEED)
    print("\n" + st.report(), flush=True)
    refused = {k: v for k, v in st.cov.items() if k.startswith("refused:")}
    print(f"refusals: {refused or 'none'}; pairs run {st.cov['pairs-run']} of {st.cov['pairs']}", flush=True)
    assert st.failures == 0, st.report()
    assert st.exact_runs > 0 and st.exact_equal == st.exact_runs
    assert not B.missing_buckets(st.cov, B.MINIMUMS), B.missing_buckets(st.cov, B.MINIMUMS)
    assert st.cov["pairs-run"] >= 0.9 * st.cov["pairs"]
    assert set(refused) <= {"refused:mfma"}
    family_cases = sum(1 for c in B.gen_bind_cases(N_BIND, SEED) if c.mode != "near")
    assert st.cov["launch-shape:as-predicted"] == family_cases
    assert st.cov["alias:both-bindings-agree"] >= 20
