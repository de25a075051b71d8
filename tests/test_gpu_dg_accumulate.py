"""Accumulating evaluation, ``out <- alpha E + beta out``, swept like the other DG kernels
(tools/fuzz_dg.py ``run_accumulate``): the routes "kernel" (face-mass), "epilogue" (grad, div) and "axpby" (everything),
predicted on the host and asserted on the device.

- exact data: every output bit is fixed by the contract ``fma(alpha, E, fl(beta old))`` -- the whole array for powers of
  two, a correctly rounded integer reference for general factors, float32 rounded once, near overflow and in the subnormal
  range; a route refused on the host is refused on the device with every output buffer bitwise unchanged;
- signed data: the error bound, float64 bitwise the "axpby" route, powers of two bitwise torch's two passes;
- one NaN / Inf in a field, a geometry factor, an operator entry or an old output; ``beta = 0`` over poisoned outputs;
  ``alpha = 0`` over a non-finite ``E`` gives NaN on every route;
- every operand 0 or 8 bytes past a 256-byte boundary, the outputs holding old values between sentinel bands.

Each test prints its per-bucket report (run with ``-s`` to see it)."""

import sys
from pathlib import Path

import pytest

from test_dg_accumulate_cpu import SEED

sys.path.insert(0, str(Path(__file__).resolve().parents[1] / "tools"))
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
    assert st.cov["refused:unpredicted"] == 0 and st.cov["leak:nan-entries"] == 0
    assert not D.missing_buckets(st.cov, minimums), D.missing_buckets(st.cov, minimums)


@pytest.mark.timeout(300)
@pytest.mark.parametrize("share", D.ACC_SHARES)
def test_exact_data_fixes_every_bit(torch_cuda, share):
    cases = D.acc_cases(SEED)
    _check(D.run_accumulate_exact(SEED, D.acc_share(cases, share)), D.acc_share_minimums(cases, share))


@pytest.mark.timeout(300)
def test_signed_data_within_the_bound_and_bitwise_the_other_routes(torch_cuda):
    st = D.run_accumulate_bounded(SEED)
    assert max(st.worst.values()) <= 1
    _check(st, {"route:kernel": 40, "route:epilogue": 40, "route:axpby": 40, "equal:axpby-route": 80, "equal:torch-two-pass": 100,
                "factors:general": 30, "dtype:float32": 10, "dtype:mixed": 10})


@pytest.mark.timeout(300)
def test_non_finite_values_stay_where_they_belong(torch_cuda):
    _check(D.run_accumulate_nonfinite(SEED), D.ACC_PLANT_MINIMUMS)


@pytest.mark.timeout(300)
@pytest.mark.parametrize("part", ["exact", "signed"])
def test_old_values_and_operands_at_every_placement(torch_cuda, part):
    _check(D.run_accumulate_placement(SEED, part), D.ACC_PLACEMENT_MINIMUMS)
