"""bench.py --dump-outputs on CPU: which elements a dump keeps, the file names and what lands in them (CPU tensors stand in
for the device outputs; tests/test_gpu_bench_line.py runs the real thing), and the bound on --steps."""

import subprocess
import sys
from pathlib import Path

import numpy as np

import bench

ROOT = Path(__file__).resolve().parents[1]


def test_the_sample_is_fixed_sorted_and_within_the_budget():
    per_element = 8 * 35 * (1 + 3 + 4)                 # pipeline: div + grad + face-mass x4
    idx = bench.dump_sample(1_000_000, per_element)
    assert len(idx) == bench.DUMP_MAX_BYTES // per_element and len(idx) * per_element <= bench.DUMP_MAX_BYTES
    assert np.all(np.diff(idx) > 0) and idx[0] >= 0 and idx[-1] < 1_000_000
    assert np.array_equal(idx, bench.dump_sample(1_000_000, per_element))
    assert bench.dump_sample(1000, per_element) is None      # fits: every element
    assert bench.dump_sample(0, per_element) is None


def _outputs_numbered_by_element(workload, E):
    """CPU stand-ins for the output arrays: entry = 1000 * (output number) + element index."""
    import torch

    import feinsum_amd as f

    exprs = bench._einsums()[workload]
    out_dicts, n = [], 0
    for expr in exprs:
        axis = [i for i, d in enumerate(expr.shape) if isinstance(d, f.SizeParam)][0]
        shape = tuple(E if isinstance(d, f.SizeParam) else int(d) for d in expr.shape)
        od = {}
        for name in expr.output_names:
            ramp = torch.arange(E, dtype=torch.float64).reshape([E if i == axis else 1 for i in range(len(shape))])
            od[name] = (ramp + 1000.0 * n).expand(shape).contiguous()
            n += 1
        out_dicts.append(od)
    return exprs, out_dicts


def test_pipeline_files_whole_and_sampled(tmp_path):
    E = 300
    exprs, out_dicts = _outputs_numbered_by_element("pipeline", E)
    names = ["div", "grad", "facemass_0", "facemass_1", "facemass_2", "facemass_3"]

    arrays, idx = bench.output_samples("pipeline", exprs, out_dicts, E)
    assert idx is None and list(arrays) == names
    rep = bench.write_dump(tmp_path / "whole", arrays, idx, E)
    assert rep["files"] == sorted(n + ".npy" for n in names) and rep["elements"] == E and rep["sample_seed"] is None
    grad = np.load(tmp_path / "whole" / "grad.npy")
    assert grad.dtype == np.float64 and grad.shape == (3, E, 35) and np.array_equal(grad[2, :, 7], 1000.0 + np.arange(E))

    budget = 100 * 8 * 35 * 8                         # room for 100 of the 300 elements
    arrays, idx = bench.output_samples("pipeline", exprs, out_dicts, E, max_bytes=budget)
    assert len(idx) == 100 and np.array_equal(idx, bench.dump_sample(E, 8 * 35 * 8, budget))
    rep = bench.write_dump(tmp_path / "sampled", arrays, idx, E)
    assert rep["bytes"] <= budget and rep["elements"] == 100 and rep["of_elements"] == E
    assert rep["sample_seed"] == bench.DUMP_SAMPLE_SEED
    for k, name in enumerate(names):
        a = np.load(tmp_path / "sampled" / f"{name}.npy")
        assert a.dtype == np.float64
        if name == "grad":
            assert a.shape == (3, 100, 35) and np.array_equal(a[1, :, 0], 1000.0 * k + idx)
        else:
            assert a.shape == (100, 35) and np.array_equal(a[:, 34], 1000.0 * k + idx)


def test_steps_below_one_are_refused():
    out = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--steps", "0"], capture_output=True, text=True,
                         timeout=120, cwd=ROOT)
    assert out.returncode == 2 and "--steps must be at least 1" in out.stderr
