"""The DG family kernels (grad, div, face-mass in four layouts, batched and component forms, the cross product, mass
and operator apply, triangles, the fused operator) through every transform that accepts them, against the references
of oracle/einsum_ref.py (tools/fuzz_dg.py):

- exact data: every result bitwise equal to the int64 einsum of the mantissas (or, at E > 4099, to torch's float64
  einsum, itself checked against the int64 einsum on slices), near overflow and in the subnormal range too;
- signed uniform data: ``|got - ref| <= gamma(n, u) absref`` entrywise (u = 2^-24 for float32);
- one NaN / +-Inf planted in a field, a geometry factor or an operator entry: exactly its dependency set is NaN /
  non-finite, every other entry bitwise exact;
- a launch on all-NaN inputs of another size in front: the clean launch stays exact;
- whole arrays of large launches (quarter tails, the staggered start, the dynamic walk, E = 1e6) with the walk, tail,
  load and store knobs, prepared operators and the output allocation varied.

Each test prints its per-bucket report (run with ``-s`` to see it)."""

import sys
from pathlib import Path

import pytest

from test_dg_exact_cpu import N_BOUNDED, N_EXACT, N_NONFINITE, N_POISON, SEED

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


def _check(st, minimums=None):
    print("\n" + st.report(), flush=True)
    assert st.failures == 0, st.report()
    if minimums:
        assert not D.missing_buckets(st.cov, minimums), D.missing_buckets(st.cov, minimums)


@pytest.mark.timeout(600)
def test_exact_data_every_family_and_transform(torch_cuda):
    st = D.run_exact(N_EXACT, SEED)
    assert st.exact_runs > 0 and st.exact_equal == st.exact_runs
    # (every generated float64 case has an entry wider than float32; the count is in the report)
    assert st.without_wide_entry <= 2
    _check(st, {**{k: v for k, v in D.MINIMUMS.items() if not k.startswith("transform:")},
                **{f"transform:{t}": 10 for t in D.TRANSFORMS}, "walk:dynamic": 1})


@pytest.mark.timeout(300)
def test_error_bound_every_family_and_transform(torch_cuda):
    st = D.run_bounded(N_BOUNDED, SEED)
    _check(st, {"dtype:float64": 20, "dtype:float32": 10, "dtype:mixed": 5, "transform:mfma": 10,
                "transform:tiled": 10, "transform:generic": 10})


@pytest.mark.timeout(300)
def test_nonfinite_values_stay_in_their_dependency_sets(torch_cuda):
    st = D.run_nonfinite(N_NONFINITE, SEED)
    assert st.exact_runs > 0 and st.exact_equal == st.exact_runs
    # every entry a padding read can reach, in grad and div of every padded order, under "mfma" and "auto"
    padding = 2 * sum(len(D.padding_sites(c.Np, c.op)) for c in D.padding_cases(SEED))
    _check(st, {"planted:field": 20, "planted:geometry": 20, "planted:operator": 10, "planted:padding-read": padding,
                "value:nan": 10, "value:inf": 10, "value:-inf": 10, "dtype:float32": 5, "E:quarter-tail": 5})


@pytest.mark.timeout(300)
def test_poisoned_launch_in_front_changes_nothing(torch_cuda):
    st = D.run_poison(N_POISON, SEED)
    assert st.exact_runs > 0 and st.exact_equal == st.exact_runs
    _check(st, {"poisoned": 40})


@pytest.mark.timeout(600)
def test_large_launches_whole_array(torch_cuda):
    st = D.run_large(SEED)
    assert st.exact_runs > 0 and st.exact_equal == st.exact_runs
    _check(st, {"walk:dynamic": 3, "walk:static": 3, "quarter_tail": 6, "staggered_start": 1, "alloc:split": 5,
                "alloc:torch": 5, "prepared": 3, "dtype:float32": 6, "large:pipeline": 4})


@pytest.mark.timeout(900)
def test_eight_million_elements_whole_array(torch_cuda):
    free, _ = torch_cuda.cuda.mem_get_info()
    if free < 80 * 2**30:
        pytest.skip("needs ~60 GB of device memory")
    st = D.run_large(SEED, sizes=(8_000_000,), only=("grad", "pipeline"), f32=False)
    assert st.exact_runs > 0 and st.exact_equal == st.exact_runs
    _check(st)
