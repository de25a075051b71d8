"""Accumulation inside the contraction and the split-reduction kernels on the device:
``evaluate(..., alpha=, beta=, transform={"variant": "contraction" | "reduction", "accumulate": "kernel"})`` computes
``out <- alpha E + beta out`` in the store epilogue of ``contract_mfma_kernel`` (``fe_einsum_contract_acc``) or in the
combine launch of the split reduction (``fe_einsum_reduce_acc``), without a temporary and without ``fe_axpby``.  Exact on
integer data through every row map, bitwise the ``"axpby"`` route for general factors on every accumulating instantiation,
``beta == 0`` blind to what the output held, K = 0, index groups and the persistent loop, schedules of three operands, a DG
shape, the two reduction paths, capture and replay, and refusals that leave the output alone."""

import re

import numpy as np
import pytest

import autograd_cases as C
import feinsum_amd as f
from feinsum_amd import _hip
from feinsum_amd.contraction_schedule import ContractionSchedule, EinsumOperand, IntermediateResult
from feinsum_amd.measure import _bind
from oracle import einsum_ref as ref
from test_gpu_accumulate import AB

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

KERNEL = {"variant": "contraction", "accumulate": "kernel"}
AXPBY = {"variant": "contraction", "accumulate": "axpby"}
R_KERNEL = {"variant": "reduction", "accumulate": "kernel"}
R_AXPBY = {"variant": "reduction", "accumulate": "axpby"}
GENERAL = (0.3, -1.7)
SUBSCRIPTS = ["ik,kj->ij", "ki,kj->ij", "ik,jk->ij", "ki,jk->ji"]
SIZES = [(16, 16, 4), (17, 33, 5), (65, 63, 16), (129, 64, 17)]
TOP = 4           # operands are integers in [-TOP, TOP]
ACC_NAMES = [base + " acc" for base in (
    "contract f64 (16-byte groups)", "contract f64", "contract f32 (16-byte groups)", "contract f32",
    "contract f32 x f32 -> f64 (16-byte groups)", "contract f32 x f32 -> f64",
    "contract f32 x f64 (16-byte groups)", "contract f32 x f64 (A 16-byte groups)", "contract f32 x f64 (B 16-byte groups)",
    "contract f32 x f64",
    "contract f64 x f32 (16-byte groups)", "contract f64 x f32 (A 16-byte groups)", "contract f64 x f32 (B 16-byte groups)",
    "contract f64 x f32")]


def _configured():
    """Names of the kernels configured so far in this process."""
    return {line[:line.index(" threads ")].strip() for line in _hip.kernel_resources().splitlines() if " threads " in line}


def _dev(host):
    return {n: torch.from_numpy(np.ascontiguousarray(v)).cuda() for n, v in host.items()}


def _expr(subs, extent, dtypes=None):
    ins = subs.split("->")[0].split(",")
    dtypes = dtypes or ["float64"] * len(ins)
    return f.einsum(subs, *[f.array("ABCD"[p], tuple(extent[c] for c in idx), dtypes[p]) for p, idx in enumerate(ins)])


def _out_dtype(e, row=0):
    return np.result_type(*[np.dtype(a.dtype) for a in e.args[row]])


def _old(shape, dtype):
    """Integers distinct along both of the last two axes: (7 i + 3 j) mod 31 - 15 over the flattened (rows, last axis)."""
    if len(shape) == 0:
        return np.asarray(-11.0, dtype=dtype)
    rows = int(np.prod(shape[:-1], dtype=np.int64))
    i, j = np.meshgrid(np.arange(rows), np.arange(shape[-1]), indexing="ij")
    return ((7 * i + 3 * j) % 31 - 15).reshape(shape).astype(dtype)


def _int_host(e, rng, E=1):
    return {n: rng.integers(-TOP, TOP + 1, size=C.concrete(e.arg_to_shape[n], E)).astype(e.arg_to_dtype[n])
            for n in sorted(e.all_args)}


def _signed_host(e, rng, E=1):
    return {n: rng.standard_normal(C.concrete(e.arg_to_shape[n], E)).astype(e.arg_to_dtype[n]) for n in sorted(e.all_args)}


def _launch(e, dev, olds, transform, alpha, beta, schedule=None):
    """Bind with copies of *olds* as outputs, launch once; ``(bound, [result arrays])``."""
    outs = {n: torch.from_numpy(np.array(o, copy=True)).cuda() for n, o in zip(e.output_names, olds)}
    q, bound, _ = _bind(e, 0, dev, outs, transform, schedule=schedule, alpha=alpha, beta=beta)
    bound.launch(q.stream_ptr)
    torch.cuda.synchronize()
    return bound, [outs[n].cpu().numpy() for n in e.output_names]


def _exact(e, host, olds, alpha, beta):
    """alpha E + beta old in integer arithmetic (halves are exact in either float type at these sizes)."""
    want = []
    for row, old in zip(e.args, olds):
        E = np.einsum(e.get_subscripts(), *[host[a.name].astype(np.int64) for a in row])
        want.append((alpha * E.astype(np.float64) + beta * old.astype(np.float64)).astype(old.dtype))
    return want


def _same_as_axpby(e, dev, olds, kernel, axpby, alpha=GENERAL[0], beta=GENERAL[1], schedule=None, tag=""):
    bk, got = _launch(e, dev, olds, kernel, alpha, beta, schedule)
    ba, want = _launch(e, dev, olds, axpby, alpha, beta, schedule)
    assert bk.accumulate == "kernel" and ba.accumulate == "axpby", tag
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == w.dtype and np.isfinite(w).all() and np.array_equal(g, w), (tag, k, int((g != w).sum()))
    return bk


def test_bit_budget():
    # the largest sum here: 'ei,ei->' at E = 4099, i = 35 -- products of two integers of at most TOP, doubled by alpha = 2,
    # plus half an old output: below 2^23, so float32 holds every partial sum and every result exactly, halves included
    assert 2 * (4099 * 35 * TOP * TOP) + 16 < 2 ** 23
    assert 2 * (1003 * 35 * TOP ** 3) + 16 < 2 ** 23            # 'e,ei,ei->'
    assert 2 * (129 * TOP * TOP) + 16 < 2 ** 23                 # the GEMMs (K <= 17), 'abcd,ea->ebcd' (K = 9)


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("subs", SUBSCRIPTS)
def test_exact_on_integer_data(subs, dtype):
    """Every row map (float64 and float32 differ), ragged and full tiles, more than one tile, every (alpha, beta)."""
    for M, N, K in SIZES:
        e = _expr(subs, {"i": M, "j": N, "k": K}, [dtype] * 2)
        rng = np.random.default_rng(M * 1000 + K)
        host = _int_host(e, rng)
        dev = _dev(host)
        old = _old(C.concrete(e.shape, 1), dtype)
        for alpha, beta in AB:
            bound, got = _launch(e, dev, [old], KERNEL, alpha, beta)
            assert bound.accumulate == "kernel" and bound.entry_point == "fe_einsum_contract_acc"
            want = _exact(e, host, [old], alpha, beta)[0]
            assert ref.bitwise_equal(got[0], want), (subs, dtype, M, N, K, alpha, beta, int((got[0] != want).sum()))


# (operand dtypes, K, N, the instantiation): 'ik,kj->ij' -- A walks k fastest (its groups run along K), B walks j (along N)
LADDER = [
    (("float64", "float64"), 16, 34, "contract f64 (16-byte groups) acc"),
    (("float64", "float64"), 17, 34, "contract f64 acc"),
    (("float32", "float32"), 16, 36, "contract f32 (16-byte groups) acc"),
    (("float32", "float32"), 18, 36, "contract f32 acc"),
    (("float32", "float64"), 16, 34, "contract f32 x f64 (16-byte groups) acc"),
    (("float32", "float64"), 16, 33, "contract f32 x f64 (A 16-byte groups) acc"),
    (("float32", "float64"), 18, 34, "contract f32 x f64 (B 16-byte groups) acc"),
    (("float32", "float64"), 17, 33, "contract f32 x f64 acc"),
    (("float64", "float32"), 18, 36, "contract f64 x f32 (16-byte groups) acc"),
    (("float64", "float32"), 18, 34, "contract f64 x f32 (A 16-byte groups) acc"),
    (("float64", "float32"), 17, 36, "contract f64 x f32 (B 16-byte groups) acc"),
    (("float64", "float32"), 17, 33, "contract f64 x f32 acc"),
]


@pytest.mark.parametrize("dtypes,K,N,name", LADDER, ids=[c[3][9:-4].replace(" ", "_") for c in LADDER])
def test_bitwise_the_axpby_route_on_every_instantiation(dtypes, K, N, name):
    e = _expr("ik,kj->ij", {"i": 67, "j": N, "k": K}, list(dtypes))
    rng = np.random.default_rng(K * 100 + N)
    dev = _dev(_signed_host(e, rng))
    old = rng.standard_normal((67, N)).astype(_out_dtype(e))
    _same_as_axpby(e, dev, [old], KERNEL, AXPBY, tag=name)
    assert name in _configured(), (name, sorted(_configured()))


@pytest.mark.parametrize("K,N,name", [(16, 36, ACC_NAMES[4]), (17, 36, ACC_NAMES[5])], ids=["groups", "plain"])
def test_two_float32_operands_of_a_float64_contraction(K, N, name):
    """``np.result_type`` never asks for it, the C ABI allows it: both operands stored as float32, float64 arithmetic
    and output.  Against ``fe_einsum_contract`` into a temporary, then ``fe_axpby`` -- what the ``"axpby"`` route runs."""
    M = 67
    rng = np.random.default_rng(K)
    A = torch.from_numpy(rng.standard_normal((M, K)).astype(np.float32)).cuda()
    B = torch.from_numpy(rng.standard_normal((K, N)).astype(np.float32)).cuda()
    old = torch.from_numpy(rng.standard_normal((M, N))).cuda()
    d = _hip.einsum_desc(["ik", "kj"], "ij", "k", {"i": M, "j": N, "k": K}, [A, B], True, [np.dtype("float32")] * 2)
    got, tmp, want = old.clone(), torch.empty_like(old), old.clone()
    _hip.einsum_contract_acc(d, [A.data_ptr(), B.data_ptr()], got.data_ptr(), *GENERAL, 0)
    _hip.einsum_contract(d, [A.data_ptr(), B.data_ptr()], tmp.data_ptr(), 0)
    _hip.axpby(want.data_ptr(), tmp.data_ptr(), M * N, *GENERAL, True, 0)
    torch.cuda.synchronize()
    assert torch.equal(got, want) and bool(torch.isfinite(want).all())
    np.testing.assert_allclose(tmp.cpu().numpy(), A.cpu().numpy().astype(np.float64) @ B.cpu().numpy().astype(np.float64),
                               rtol=1e-12, atol=1e-12)
    assert name in _configured()


def test_all_fourteen_accumulating_instantiations_ran():
    """(After the two tests above in this module.)"""
    missing = sorted(set(ACC_NAMES) - _configured())
    assert not missing, missing
    lines = [ln for ln in _hip.kernel_resources().splitlines() if any(ln.startswith(n + " ") for n in ACC_NAMES)]
    assert len(lines) >= 14
    for ln in lines:        # no scratch, and the two blocks per CU the persistent grid assumes
        scratch, resident, needs = re.search(r"scratch\s+(\d+) B.*blocks/CU (\d+) \(geometry needs (\d+)\)", ln).groups()
        assert int(scratch) == 0 and int(needs) == 2 and int(resident) >= 2, ln


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("M,N", [(17, 33), (64, 64)])
def test_beta_zero_ignores_what_the_output_holds(M, N, dtype):
    K, guard, sentinel = 12, 512, -777.0
    e = _expr("ik,kj->ij", {"i": M, "j": N, "k": K}, [dtype] * 2)
    host = _int_host(e, np.random.default_rng(M))
    dev = _dev(host)
    buf = torch.full((M * N + 2 * guard,), sentinel, dtype=getattr(torch, dtype), device="cuda")
    out = buf[guard:guard + M * N].view(M, N)
    flat = out.view(-1)
    flat[0::3] = float("nan")
    flat[1::3] = float("inf")
    flat[2::3] = -float("inf")
    q, bound, _ = _bind(e, 0, dev, {"_fe_out": out}, KERNEL, alpha=0.5, beta=0.0)
    assert bound.accumulate == "kernel"
    bound.launch(q.stream_ptr)
    torch.cuda.synchronize()
    want = _exact(e, host, [np.zeros((M, N), dtype)], 0.5, 0.0)[0]
    assert ref.bitwise_equal(out.cpu().numpy(), want)
    assert bool((buf[:guard] == sentinel).all()) and bool((buf[-guard:] == sentinel).all())


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_an_empty_summation_scales_the_output(dtype):
    M, N = 17, 33
    e = _expr("ik,kj->ij", {"i": M, "j": N, "k": 0}, [dtype] * 2)
    dev = {"A": torch.empty((M, 0), dtype=getattr(torch, dtype), device="cuda"),
           "B": torch.empty((0, N), dtype=getattr(torch, dtype), device="cuda")}
    old = _old((M, N), dtype)
    for alpha, beta in ((2.0, -0.5), (0.5, 0.0)):
        _, got = _launch(e, dev, [old], KERNEL, alpha, beta)
        assert ref.bitwise_equal(got[0], (beta * old).astype(dtype)), (alpha, beta)
    # an empty output: nothing to launch, nothing to fail
    e0 = _expr("ik,kj->ij", {"i": 0, "j": N, "k": 5}, [dtype] * 2)
    dev0 = {"A": torch.empty((0, 5), dtype=getattr(torch, dtype), device="cuda"),
            "B": torch.zeros((5, N), dtype=getattr(torch, dtype), device="cuda")}
    _, got = _launch(e0, dev0, [np.empty((0, N), dtype)], KERNEL, 2.0, -0.5)
    assert got[0].shape == (0, N)


GROUPS = [("abcd,ea->ebcd", {"a": 9, "b": 5, "c": 4, "d": 6, "e": 17}),
          ("bij,bjk->bik", {"b": 600, "i": 16, "j": 8, "k": 8})]     # 600 tiles on a grid of at most 512 blocks


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("subs,extent", GROUPS, ids=["index_groups", "second_tile"])
def test_index_groups_and_the_persistent_loop(subs, extent, dtype):
    e = _expr(subs, extent, [dtype] * 2)
    if subs.startswith("bij"):
        assert 600 > 2 * torch.cuda.get_device_properties(0).multi_processor_count    # some block walks a second tile
    rng = np.random.default_rng(len(subs))
    host = _int_host(e, rng)
    old = _old(C.concrete(e.shape, 1), dtype)
    _, got = _launch(e, _dev(host), [old], KERNEL, 2.0, -0.5)
    assert ref.bitwise_equal(got[0], _exact(e, host, [old], 2.0, -0.5)[0])
    signed = rng.standard_normal(old.shape).astype(dtype)
    _same_as_axpby(e, _dev(_signed_host(e, rng)), [signed], KERNEL, AXPBY, tag=subs)


def _chain_sched():
    return ContractionSchedule(("jk,kl->jl", "ij,jl->il"), ("t", "_fe_out"),
                               ((EinsumOperand(1), EinsumOperand(2)), (EinsumOperand(0), IntermediateResult("t"))))


def _entry_points(bound):
    return [getattr(fn, "entry_point", "fe_" + fn.__name__) for fn, *_ in bound.launches]


@pytest.mark.parametrize("schedule", [None, _chain_sched()], ids=["optimal", "callers"])
def test_three_operands_accumulate_in_the_last_launch_only(schedule):
    e = _expr("ij,jk,kl->il", {"i": 33, "j": 17, "k": 20, "l": 9})
    rng = np.random.default_rng(3)
    old = rng.standard_normal((33, 9))
    bound = _same_as_axpby(e, _dev(_signed_host(e, rng)), [old], KERNEL, AXPBY, schedule=schedule)
    assert _entry_points(bound) == ["fe_einsum_contract", "fe_einsum_contract_acc"]
    assert len(bound.intermediates) == 1 and bound.entry_point == "fe_einsum_contract_acc"
    host = _int_host(e, rng)
    iold = _old((33, 9), "float64")
    _, got = _launch(e, _dev(host), [iold], KERNEL, -1.0, 1.0, schedule)
    assert ref.bitwise_equal(got[0], _exact(e, host, [iold], -1.0, 1.0)[0])


def test_every_row_of_a_batched_einsum_accumulates_into_its_own_output():
    e = f.batched_einsum("ij,jk,kl->il", [[f.array(f"A{r}", (33, 17)), f.array(f"B{r}", (17, 20)), f.array(f"C{r}", (20, 9))]
                                           for r in range(2)])
    rng = np.random.default_rng(4)
    host = _int_host(e, rng)
    olds = [_old((33, 9), "float64"), -2.0 * _old((33, 9), "float64")]
    bound, got = _launch(e, _dev(host), olds, KERNEL, 2.0, -0.5)
    assert _entry_points(bound) == ["fe_einsum_contract", "fe_einsum_contract_acc"] * 2
    for g, w in zip(got, _exact(e, host, olds, 2.0, -0.5)):
        assert ref.bitwise_equal(g, w)
    signed = [rng.standard_normal((33, 9)) for _ in range(2)]
    _same_as_axpby(e, _dev(_signed_host(e, rng)), signed, KERNEL, AXPBY)


def test_a_dg_shape_through_the_schedule():
    E, (nd, Np, _, _) = 65, C.TETS[2]
    e = C.grad(nd, Np)
    rng = np.random.default_rng(5)
    dev = _dev(_signed_host(e, rng, E))
    old = rng.standard_normal((nd, E, Np))
    bound = _same_as_axpby(e, dev, [old], KERNEL, AXPBY)
    assert _entry_points(bound)[-1] == "fe_einsum_contract_acc" and "fe_einsum_contract_acc" not in _entry_points(bound)[:-1]


# (subscripts, extents, dtypes)
REDUCTIONS = [
    ("ei,ei->", {"e": 4099, "i": 35}, ("float64", "float64")),
    ("ei,ei->", {"e": 4099, "i": 35}, ("float32", "float32")),
    ("ei,ei->", {"e": 4099, "i": 35}, ("float32", "float64")),
    ("ej,ej->j", {"e": 4099, "j": 35}, ("float64", "float64")),
    ("ej,ej->j", {"e": 4099, "j": 35}, ("float32", "float32")),
    ("ei,ej->ij", {"e": 4099, "i": 32, "j": 16}, ("float64", "float64")),
    ("ei,ej->ij", {"e": 4099, "i": 32, "j": 16}, ("float32", "float32")),
    ("e,ei,ei->", {"e": 1003, "i": 35}, ("float64", "float64", "float64")),
    ("e,ei,ei->", {"e": 1003, "i": 35}, ("float32", "float32", "float32")),
]


@pytest.mark.parametrize("subs,extent,dtypes", REDUCTIONS, ids=[f"{s}_{'_'.join(d[:2])}" for s, _, d in REDUCTIONS])
def test_reduction(subs, extent, dtypes):
    e = _expr(subs, extent, list(dtypes))
    dt = _out_dtype(e)
    shape = C.concrete(e.shape, 1)
    rng = np.random.default_rng(len(subs) + len(dtypes[0]))
    host = _int_host(e, rng)
    dev = _dev(host)
    old = _old(shape, dt)
    for alpha, beta in AB:                                    # powers of two and zero: exact
        bound, got = _launch(e, dev, [old], R_KERNEL, alpha, beta)
        assert bound.accumulate == "kernel" and bound.entry_point == "fe_einsum_reduce_acc"
        assert _entry_points(bound) == ["fe_einsum_reduce_acc"] and bound.workspace is not None
        want = _exact(e, host, [old], alpha, beta)[0]
        assert ref.bitwise_equal(got[0], want), (subs, dtypes, alpha, beta, got[0], want)
    path = _hip.einsum_reduce_plan(bound.launches[0][1])[0]
    assert path == ("mfma" if subs == "ei,ej->ij" else "valu"), path
    signed = rng.standard_normal(shape).astype(dt)
    sdev = _dev(_signed_host(e, rng))
    _same_as_axpby(e, sdev, [signed], R_KERNEL, R_AXPBY, tag=subs)
    # beta == 0: a NaN in the output does not reach the result
    _, got = _launch(e, sdev, [np.full(shape, np.nan, dt)], R_KERNEL, 0.5, 0.0)
    _, plain = _launch(e, sdev, [np.zeros(shape, dt)], "reduction", 1.0, 0.0)
    assert np.isfinite(got[0]).all() and np.array_equal(got[0], (dt.type(0.5) * plain[0]).astype(dt))
    assert ("reduce combine f64 acc" if dt == np.float64 else "reduce combine f32 acc") in _configured()


def test_capture_and_replay():
    M, N, K = 65, 63, 16
    e = _expr("ik,kj->ij", {"i": M, "j": N, "k": K})
    host = _int_host(e, np.random.default_rng(9))
    dev = _dev(host)
    old = _old((M, N), "float64")
    _launch(e, dev, [old], KERNEL, 1.0, 1.0)              # (the kernel is configured before the capture)
    out = torch.from_numpy(old).cuda()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    q = f.DeviceQueue(0, side)
    torch.cuda.synchronize()
    _, bound, _ = _bind(e, q, dev, {"_fe_out": out}, KERNEL, alpha=1.0, beta=1.0)
    assert bound.accumulate == "kernel" and not bound.intermediates
    assert len(bound.writes) == 1 and not bound.owned_arrays      # the output alone: no temporary
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        bound.launch(int(torch.cuda.current_stream().cuda_stream))
    out.copy_(torch.from_numpy(old))
    torch.cuda.synchronize()
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    E = np.einsum("ik,kj->ij", host["A"].astype(np.int64), host["B"].astype(np.int64)).astype(np.float64)
    assert ref.bitwise_equal(out.cpu().numpy(), old + 3 * E)


def test_refusals_leave_the_output_alone():
    rowsum = f.einsum("ij->i", f.array("A", (40, 6)))
    dev = {"A": torch.ones(40, 6, dtype=torch.float64, device="cuda")}
    planted = torch.full((40,), 7.0, dtype=torch.float64, device="cuda")
    with pytest.raises(NotImplementedError, match="no accumulating kernel"):
        f.evaluate(rowsum, 0, dev, out_dict={"_fe_out": planted}, transform=KERNEL, alpha=2.0, beta=1.0, wait=True)
    # a caller's schedule whose last step has one input: refused at bind, naming the step
    e = f.einsum("ik,kj->i", f.array("A", (33, 17)), f.array("B", (17, 20)))
    sched = ContractionSchedule(("ik,kj->ij", "ij->i"), ("t", "_fe_out"),
                                ((EinsumOperand(0), EinsumOperand(1)), (IntermediateResult("t"),)))
    dev2 = {"A": torch.ones(33, 17, dtype=torch.float64, device="cuda"), "B": torch.ones(17, 20, dtype=torch.float64, device="cuda")}
    planted2 = torch.full((33,), 7.0, dtype=torch.float64, device="cuda")
    with pytest.raises(NotImplementedError, match="'ij->i'"):
        f.evaluate(e, 0, dev2, out_dict={"_fe_out": planted2}, transform=KERNEL, schedule=sched, alpha=2.0, beta=1.0, wait=True)
    torch.cuda.synchronize()
    assert bool((planted == 7.0).all()) and bool((planted2 == 7.0).all())
    # the same call on the "axpby" route runs
    got = f.evaluate(e, 0, dev2, out_dict={"_fe_out": planted2}, transform=AXPBY, schedule=sched, alpha=2.0, beta=1.0, wait=True)
    assert bool((got["_fe_out"] == 7.0 + 2.0 * 17 * 20).all())


# Measured on MI355X with tools/bench_contraction_accumulate.py (profiles/contraction_accumulate/bench.jsonl, DESIGN.md section
# 3m): 'abcd,ea->ebcd' at 48^4 x 64, float64, (alpha, beta) = (1, 1) -- the "axpby" route, which is what the same call runs
# without the transform, 112.7 us over the kernel route's 101.1 us.  The largest ratio among the shapes measured; the floor is
# halfway between 1.0 and the measured ratio.
SPEED_MEASURED = 1.115


def test_kernel_route_is_faster_than_the_axpby_route():
    floor = (1.0 + SPEED_MEASURED) / 2
    extent = {"a": 48, "b": 48, "c": 48, "d": 48, "e": 64}
    e = _expr("abcd,ea->ebcd", extent)
    gen = torch.Generator(device="cuda").manual_seed(1)
    dev = {"A": torch.rand((48, 48, 48, 48), dtype=torch.float64, device="cuda", generator=gen) - 0.5,
           "B": torch.rand((64, 48), dtype=torch.float64, device="cuda", generator=gen) - 0.5}
    out = torch.zeros((64, 48, 48, 48), dtype=torch.float64, device="cuda")
    q, fallback, _ = _bind(e, 0, dev, {"_fe_out": out}, AXPBY, alpha=1.0, beta=1.0)
    _, kernel, _ = _bind(e, 0, dev, {"_fe_out": out}, KERNEL, alpha=1.0, beta=1.0)
    assert fallback.accumulate == "axpby" and kernel.accumulate == "kernel"

    def seconds(launch, min_seconds=0.25):
        for _ in range(3):
            launch()
        torch.cuda.synchronize()
        reps = 20
        while True:
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(reps):
                launch()
            t1.record()
            t1.synchronize()
            total = t0.elapsed_time(t1) * 1e-3
            if total >= min_seconds:
                return total / reps
            reps *= 4

    b = seconds(lambda: fallback.launch(q.stream_ptr))
    c = seconds(lambda: kernel.launch(q.stream_ptr))
    print(f"abcd,ea->ebcd: axpby route {b * 1e6:.1f} us, kernel route {c * 1e6:.1f} us, ratio {b / c:.3f} (floor {floor:.3f})")
    assert b / c > floor, (b, c)
