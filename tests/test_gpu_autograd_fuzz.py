"""The backward pass of evaluate_differentiable against the references of oracle/einsum_ref.py
(tools/fuzz_autograd.py), every input requiring grad, the routes of the backward launches predicted on the host:

- exact data: every gradient bitwise equal to the int64 sum of its adjoint einsums (or, at E > 4099, to torch's float64
  einsums, checked against the int64 einsums on slices), near overflow and in the subnormal range too;
- signed uniform data: ``|got - ref| <= gamma(n, u) absref`` entrywise;
- one NaN / +-Inf planted in a field, a geometric factor, an operator entry or an output gradient: exactly the union of
  the dependency sets of each gradient's terms is NaN / non-finite, every other entry bitwise exact;
- whole arrays at E = 98 304 ... 1 000 003;
- the two adjoint kernels called directly, every compiled shape and layout, between guard bands.

Each test prints its per-bucket report (run with ``-s`` to see it)."""

import sys
from pathlib import Path

import pytest

from test_autograd_fuzz_cpu import N_BOUNDED, N_EINSUM, N_EXACT, N_NONFINITE, SEED

sys.path.insert(0, str(Path(__file__).resolve().parents[1] / "tools"))
import fuzz_autograd as A  # noqa: E402

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
        assert not A.missing_buckets(st.cov, minimums), A.missing_buckets(st.cov, minimums)


ROUTE_MINIMUMS = {f"route:{r}": 3 for r in A.ROUTES if r not in A.OPGRAD_ROUTES}
# under operator_gradients="kernel" (DESIGN.md section 3l): the operator-gradient kernels, per pass
OPGRAD_MINIMUMS = {"route:opgrad_d": 3, "route:opgrad_r": 3}


@pytest.mark.timeout(900)
def test_exact_gradients_every_kind_route_and_transform(torch_cuda):
    st = A.run_exact(N_EXACT, SEED, N_EINSUM)
    assert st.exact_runs > 0 and st.exact_equal == st.exact_runs
    # (the device refuses some forward variants, e.g. "mfma" at the tiled-only orders: run on "auto", counted)
    _check(st, {**A.MINIMUMS, **{f"transform:{t}": 4 for t in A.FWD_TRANSFORMS}})


@pytest.mark.timeout(300)
def test_gradients_within_the_error_bound(torch_cuda):
    st = A.run_bounded(N_BOUNDED, SEED)
    _check(st, {"dtype:float64": 10, "dtype:float32": 5, "dtype:mixed": 5, "b:>8": 2, "kind:einsum": 3,
                **ROUTE_MINIMUMS, **OPGRAD_MINIMUMS, "opgrad:mode": 12, "opgrad:b>8": 2,
                **{f"opgrad:kind:{k}": 1 for k in ("grad", "div", "fm", "bgrad", "mass", "lift2")}})


@pytest.mark.timeout(300)
def test_nonfinite_values_stay_in_their_gradient_dependency_sets(torch_cuda):
    st = A.run_nonfinite(N_NONFINITE, SEED)
    assert st.exact_runs > 0 and st.exact_equal == st.exact_runs
    _check(st, {"planted:field": 10, "planted:geometry": 10, "planted:operator": 10, "planted:output-grad": 10,
                "value:nan": 8, "value:inf": 8, "value:-inf": 8, **ROUTE_MINIMUMS, **OPGRAD_MINIMUMS,
                "opgrad:planted:output-grad": 5, "opgrad:planted:geometry": 5, "opgrad:planted:field": 5,
                "opgrad:planted:operator": 5})


@pytest.mark.timeout(600)
def test_large_gradients_whole_array(torch_cuda):
    st = A.run_large(SEED)
    assert st.exact_runs > 0 and st.exact_equal == st.exact_runs
    _check(st, {**ROUTE_MINIMUMS, "route:facemass_j:b>8": 3, "E:1000003": 3, "dtype:float32": 1,
                **OPGRAD_MINIMUMS,
                **{f"opgrad:large:{k}:E{A.MULTI_TRIP_E}": 1 for k in ("grad", "div", "fm", "fm_jfi", "fm_fji")},
                f"opgrad:large:grad:E{A.MULTI_TRIP_E}": 2})


@pytest.mark.timeout(600)
def test_adjoint_kernels_every_shape_and_layout(torch_cuda):
    st = A.run_kernels(SEED)
    assert st.exact_runs > 0 and st.exact_equal == st.exact_runs
    _check(st, {"E:multi-trip": 17, "facemass_adj:b17": 200, "facemass_adj:dJ": 200, "geomadj:er": 40,
                **{f"opgrad:{lay},{ol}": 8 for lay in A.GEOM_LAYOUTS for ol in A.OPGRAD_OUT_LAYOUTS},
                **{f"opgrad_fm:{jl},{rl}": 9 for jl, rl, _ in A.FM_LAYOUT_FLAGS}, **{f"opgrad_fm:b{b}": 18 for b in (1, 2, 4, 9)},
                **{f"opgrad:E{E}": 15 for E in A.OPGRAD_E}, "opgrad:workspace": 136})
