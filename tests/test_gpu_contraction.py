"""The "contraction" transform on the device (fe_einsum_contract, csrc/fe_contract.h): the MFMA fragment layouts on
exact data, ragged and strided shapes, index groups, batch counts above the grid limit, schedules of three operands,
arrays past 2^31 elements, write bounds, streams and graph capture, and the speed-up over the generic kernel."""

import itertools
import threading

import numpy as np
import pytest

import feinsum_amd as f
from feinsum_amd import _hip
from feinsum_amd.contraction_schedule import ContractionSchedule, EinsumOperand, IntermediateResult
from feinsum_amd.measure import generate_host_input_arrays

import dg

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    _hip.load_library()
    return torch


def _oracle(expr, host):
    from oracle import np_oracle

    return {name: np_oracle.reference_outputs(expr.get_subscripts(), [[host[a.name] for a in row]])[0]
            for name, row in zip(expr.output_names, expr.args)}


def _assert_close(got, ref, dtype=np.float64):
    from oracle import np_oracle

    assert set(got) == set(ref)
    for k in ref:
        assert got[k].shape == ref[k].shape and got[k].dtype == ref[k].dtype
        assert np.isfinite(got[k]).all()
        if dtype == np.float64:
            assert np_oracle.max_rel_err(got[k], ref[k]) <= 1e-12, k
            if ref[k].size:   # inputs are positive: no cancellation
                np.testing.assert_allclose(got[k], ref[k], rtol=1e-11, atol=0)
        else:
            assert np_oracle.max_rel_err(got[k], ref[k]) <= 1e-5, k


def _run(torch, expr, host, transform="contraction", schedule=None):
    dev = {k: torch.from_numpy(v).cuda() for k, v in host.items()}
    outs = f.evaluate(expr, 0, dev, transform=transform, wait=True, schedule=schedule)
    return {k: v.cpu().numpy() for k, v in outs.items()}


def _check(torch, expr, E=1, transform="contraction", schedule=None, seed=0):
    host = generate_host_input_arrays(expr, E, np_seed=seed)
    dtype = next(iter(expr.arg_to_dtype.values()))
    _assert_close(_run(torch, expr, host, transform, schedule), _oracle(expr, host), dtype)


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("M, N, K", [(16, 16, 4), (32, 48, 12)])
@pytest.mark.parametrize("subs", ["ik,kj->ij", "ki,kj->ij", "ik,jk->ij", "ki,jk->ji"])
def test_mfma_layouts_on_exact_data(torch_cuda, dtype, M, N, K, subs):
    """Small integers: every product and sum is exact, so the result must equal the oracle bit for bit -- a wrong
    C/D row map (the f64 and f32 16x16x4 instructions differ) puts results in the wrong rows."""
    torch = torch_cuda
    rng = np.random.default_rng(M * N + K)
    ext = {"i": M, "j": N, "k": K}
    a_sub, b_sub = subs.split("->")[0].split(",")
    A = rng.integers(-4, 5, size=[ext[c] for c in a_sub]).astype(dtype)
    B = rng.integers(-4, 5, size=[ext[c] for c in b_sub]).astype(dtype)   # not symmetric
    expr = f.einsum(subs, f.array("A", A.shape, dtype), f.array("B", B.shape, dtype))
    got = _run(torch, expr, {"A": A, "B": B})["_fe_out"]
    ref = np.einsum(subs, A.astype(np.float64), B.astype(np.float64)).astype(dtype)
    assert np.array_equal(got, ref)


@pytest.mark.parametrize("M, N, K", [(1, 1, 1), (17, 33, 5), (1000, 7, 300), (129, 257, 65)])
@pytest.mark.parametrize("ta, tb, tc", list(itertools.product([False, True], repeat=3)))
def test_ragged_gemms(torch_cuda, M, N, K, ta, tb, tc):
    a = "ki" if ta else "ik"
    b = "jk" if tb else "kj"
    c = "ji" if tc else "ij"
    ext = {"i": M, "j": N, "k": K}
    for dtype in ("float64", "float32"):
        expr = f.einsum(f"{a},{b}->{c}", f.array("A", tuple(ext[x] for x in a), dtype),
                        f.array("B", tuple(ext[x] for x in b), dtype))
        _check(torch_cuda, expr, seed=M + N + K)


@pytest.mark.parametrize("subs, shapes", [
    ("abcd,ea->ebcd", [(6, 5, 4, 7), (9, 6)]),
    ("abc,bda->dc", [(5, 6, 7), (6, 8, 5)]),
    ("ijkl,klmn->ijmn", [(3, 4, 5, 6), (5, 6, 7, 2)]),
    ("ijkl,klmn->ijmn", [(8, 8, 8, 8), (8, 8, 8, 8)]),      # 16-byte groups on both operands
])
def test_multi_index_groups(torch_cuda, subs, shapes):
    for dtype in ("float64", "float32"):
        expr = f.einsum(subs, *[f.array(n, s, dtype) for n, s in zip("AB", shapes)])
        _check(torch_cuda, expr)


@pytest.mark.timeout(300)
def test_batch_indices(torch_cuda):
    E = 100_003
    cases = [
        f.einsum("bij,bjk->bik", f.array("A", ("E", 3, 4)), f.array("B", ("E", 4, 5))),   # 100 003 batches
        f.einsum("ej,ej->j", f.array("A", (7, "E")), f.array("B", (7, "E"))),            # batch j: 100 003
        f.einsum("ej,ej->j", f.array("A", ("E", 7)), f.array("B", ("E", 7))),            # k = e: 100 003 long
        f.einsum("ej,ej->e", f.array("A", ("E", 9)), f.array("B", ("E", 9))),
        f.einsum("bij,bjk->bik", f.array("A", (64, 70, 33)), f.array("B", (64, 33, 90))),
    ]
    for expr in cases:
        _check(torch_cuda, expr, E=E, seed=3)


def test_odd_indices(torch_cuda):
    torch = torch_cuda
    # a summed index present in one operand only
    _check(torch, f.einsum("ij,k->i", f.array("A", (100, 70)), f.array("w", (130,))))
    _check(torch, f.einsum("ik,kj->ij", f.array("A", (100, 1)), f.array("B", (1, 90))))   # K = 1
    # a stride-0 operand (an expand()-ed vector) straight through the C ABI: 'ij,kj->ik' with B[k, j] = w[j]
    rng = np.random.default_rng(5)
    A = torch.from_numpy(rng.random((300, 70))).cuda()
    w = torch.from_numpy(rng.random(70)).cuda()
    Bx = w.expand(90, 70)
    out = torch.empty(300, 90, dtype=torch.float64, device="cuda")
    d = _hip.EinsumDesc()
    d.n_operands, d.n_out, d.n_sum, d.dtype = 2, 2, 1, 0
    d.out_extent[0], d.out_extent[1], d.sum_extent[0] = 300, 90, 70
    d.op_out_stride[0][0], d.op_sum_stride[0][0] = A.stride(0), A.stride(1)
    d.op_out_stride[1][1], d.op_sum_stride[1][0] = Bx.stride(0), Bx.stride(1)
    assert Bx.stride(0) == 0
    _hip.einsum_contract(d, [A.data_ptr(), Bx.data_ptr()], out.data_ptr(), 0)
    torch.cuda.synchronize()
    ref = np.einsum("ij,kj->ik", A.cpu().numpy(), Bx.cpu().numpy())
    np.testing.assert_allclose(out.cpu().numpy(), ref, rtol=1e-12, atol=0)
    # buffers only 8-byte aligned (one float64 past a 256-byte boundary), vector-friendly shapes
    for subs, shapes in (("ik,kj->ij", [(130, 64), (64, 96)]), ("ki,kj->ij", [(64, 130), (64, 96)])):
        expr = f.einsum(subs, f.array("A", shapes[0]), f.array("B", shapes[1]))
        host = generate_host_input_arrays(expr, 1, np_seed=7)
        dev = {}
        for k, v in host.items():
            buf = torch.empty(v.size + 1, dtype=torch.float64, device="cuda")
            buf[1:] = torch.from_numpy(v).cuda().reshape(-1)
            dev[k] = buf[1:].view(v.shape)
        outs = f.evaluate(expr, 0, dev, transform="contraction", wait=True)
        _assert_close({k: v.cpu().numpy() for k, v in outs.items()}, _oracle(expr, host))


def test_degenerate_extents(torch_cuda):
    torch = torch_cuda
    # an empty k space: zeros, whatever the output held
    for subs, shapes in (("ij,ej->i", [(5, 7), ("E", 7)]), ("ek,kj->ej", [(70, "E"), ("E", 40)])):
        args = [f.array(f"a{k}", s) for k, s in enumerate(shapes)]
        expr = f.einsum(subs, *args)
        dev = {a.name: torch.zeros(tuple(0 if d == "E" else d for d in s), dtype=torch.float64, device="cuda")
               for a, s in zip(args, shapes)}
        shape = tuple(int(x) for x in expr.shape if not isinstance(x, f.SizeParam))
        out = torch.full(shape, 3.5, dtype=torch.float64, device="cuda")
        f.evaluate(expr, 0, dev, out_dict={"_fe_out": out}, transform="contraction", wait=True)
        assert out.numel() > 0 and bool((out == 0).all())
    # an empty output: nothing to launch
    expr = f.einsum("ek,kj->ej", f.array("A", ("E", 30)), f.array("B", (30, 40)))
    dev = {"A": torch.zeros(0, 30, dtype=torch.float64, device="cuda"),
           "B": torch.zeros(30, 40, dtype=torch.float64, device="cuda")}
    assert f.evaluate(expr, 0, dev, transform="contraction", wait=True)["_fe_out"].shape == (0, 40)


def test_row_batches(torch_cuda):
    expr = f.batched_einsum("ik,kj->ij", [[f.array(f"A{r}", (90, 70)), f.array(f"B{r}", (70, 50))] for r in range(3)])
    _check(torch_cuda, expr, seed=11)


def _chain_sched():
    return ContractionSchedule(("jk,kl->jl", "ij,jl->il"), ("t", "_fe_out"),
                               ((EinsumOperand(1), EinsumOperand(2)), (EinsumOperand(0), IntermediateResult("t"))))


@pytest.mark.timeout(300)
def test_through_the_schedule(torch_cuda):
    torch = torch_cuda
    chain = f.einsum("ij,jk,kl->il", f.array("A", (130, 70)), f.array("B", (70, 90)), f.array("C", (90, 40)))
    xie = f.einsum("xre,rij,ej->xie", f.array("J", (3, 3, "E")), f.array("R", (3, 20, 20)), f.array("u", ("E", 20)))
    for transform in ("contraction", "generic"):
        _check(torch, chain, transform=transform)
        _check(torch, chain, transform=transform, schedule=_chain_sched())
        _check(torch, xie, E=1003, transform=transform)
    for expr in (dg.grad(), dg.div(), dg.face_mass(4)):
        host = generate_host_input_arrays(expr, 1003, np_seed=2)
        got = _run(torch, expr, host, "contraction")
        _assert_close(got, _oracle(expr, host))
        fam = _run(torch, expr, host, "mfma")
        for k in fam:
            np.testing.assert_allclose(got[k], fam[k], rtol=1e-11, atol=0)


@pytest.mark.timeout(900)
def test_operand_beyond_two_to_the_31(torch_cuda):
    """'erj,rij->ei' at E = 2.1e7: u has 2.2e9 elements (17.6 GB), every offset past 2^31; sampled slices."""
    torch = torch_cuda
    E = 21_000_000
    free, _ = torch.cuda.mem_get_info()
    if free < 40 * 2**30:   # u 17.6 GB + out 5.9 GB, and room for the sampled copies
        pytest.skip("needs 40 GiB of free device memory (the arrays take ~24 GB)")
    gen = torch.Generator(device="cuda").manual_seed(17)
    u = torch.rand(E, 3, 35, dtype=torch.float64, device="cuda", generator=gen)
    D = torch.rand(3, 35, 35, dtype=torch.float64, device="cuda", generator=gen)
    assert u.numel() > 2**31
    expr = f.einsum("erj,rij->ei", f.array("u", ("E", 3, 35)), f.array("D", (3, 35, 35)))
    out = f.evaluate(expr, 0, {"u": u, "D": D}, transform="contraction", wait=True)["_fe_out"]
    Dh = D.cpu().numpy()
    for sl in (slice(0, 300), slice(E // 2, E // 2 + 300), slice(20_500_000, 20_500_300), slice(E - 300, E)):
        ref = np.einsum("erj,rij->ei", u[sl].cpu().numpy(), Dh)
        np.testing.assert_allclose(out[sl].cpu().numpy(), ref, rtol=1e-11, atol=0)


def test_writes_only_its_output(torch_cuda):
    torch = torch_cuda
    guard = 4096
    cases = [f.einsum("ik,kj->ij", f.array("A", (129, 65)), f.array("B", (65, 257))),
             f.einsum("ki,jk->ji", f.array("A", (33, 70)), f.array("B", (17, 33))),
             f.einsum("bij,bjk->bik", f.array("A", ("E", 3, 4)), f.array("B", ("E", 4, 5))),
             f.einsum("abcd,ea->ebcd", f.array("A", (6, 5, 4, 7)), f.array("B", (9, 6))),
             dg.grad()]
    for dtype in (torch.float64, torch.float32):
        for expr in cases:
            if dtype == torch.float32:
                expr = f.batched_einsum(expr.get_subscripts(), [[a.copy(dtype=np.dtype("float32")) for a in row]
                                                                for row in expr.args])
            host = generate_host_input_arrays(expr, 1003, np_seed=1)
            dev = {k: torch.from_numpy(v).cuda() for k, v in host.items()}
            shape = tuple(1003 if isinstance(d, f.SizeParam) else int(d) for d in expr.shape)
            n = int(np.prod(shape))
            buf = torch.full((n + 2 * guard,), -7.25, dtype=dtype, device="cuda")
            out = buf[guard:guard + n].view(shape)
            f.evaluate(expr, 0, dev, out_dict={"_fe_out": out}, transform="contraction", wait=True)
            assert bool((buf[:guard] == -7.25).all()) and bool((buf[guard + n:] == -7.25).all()), expr.get_subscripts()
            ref = _oracle(expr, host)["_fe_out"]
            assert np.allclose(out.cpu().numpy(), ref, rtol=1e-5 if dtype == torch.float32 else 1e-11, atol=0)


def test_streams_and_graph_capture(torch_cuda):
    torch = torch_cuda
    expr = f.einsum("ik,kj->ij", f.array("A", (300, 200)), f.array("B", (200, 170)))
    host = generate_host_input_arrays(expr, 1, np_seed=9)
    dev = {k: torch.from_numpy(v).cuda() for k, v in host.items()}
    eager = f.evaluate(expr, 0, dev, transform="contraction", wait=True)["_fe_out"].clone()
    # two host threads, two streams
    outs = [torch.full_like(eager, float("nan")) for _ in range(2)]
    errors = []

    def worker(t):
        try:
            s = torch.cuda.Stream()
            q = f.DeviceQueue(0, s)
            for _ in range(20):
                f.evaluate(expr, q, dev, out_dict={"_fe_out": outs[t]}, transform="contraction")
            q.finish()
        except Exception as exc:   # noqa: BLE001
            errors.append(exc)

    threads = [threading.Thread(target=worker, args=(t,)) for t in range(2)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
    for o in outs:
        assert torch.equal(o, eager)
    # a captured graph, replayed
    cap_out = torch.full_like(eager, float("nan"))
    s = torch.cuda.Stream()
    q = f.DeviceQueue(0, s)
    f.evaluate(expr, q, dev, out_dict={"_fe_out": cap_out}, transform="contraction", wait=True)   # configure first
    cap_out.fill_(float("nan"))
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        f.evaluate(expr, q, dev, out_dict={"_fe_out": cap_out}, transform="contraction")
    cap_out.fill_(float("nan"))
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(cap_out, eager)


@pytest.mark.parametrize("make", [
    lambda: f.einsum("ij,jk,kl->il", f.array("A", (300, 200)), f.array("B", (200, 170)), f.array("C", (170, 90))),
    dg.grad])
def test_two_streams_with_intermediates(torch_cuda, make):
    """Schedules allocate intermediates: two host threads on two streams, each binding and launching again and again
    while the other allocates, must not share an intermediate still in use (bitwise equal to an eager launch)."""
    torch = torch_cuda
    expr = make()
    host = generate_host_input_arrays(expr, 5003, np_seed=13)
    dev = {k: torch.from_numpy(v).cuda() for k, v in host.items()}
    eager = f.evaluate(expr, 0, dev, transform="contraction", wait=True)["_fe_out"].clone()
    outs = [[torch.full_like(eager, float("nan")) for _ in range(30)] for _ in range(2)]
    errors = []

    def worker(t):
        try:
            s = torch.cuda.Stream()
            q = f.DeviceQueue(0, s)
            for o in outs[t]:
                f.evaluate(expr, q, dev, out_dict={"_fe_out": o}, transform="contraction")
                torch.empty(1 << 20, dtype=torch.float64, device="cuda").fill_(-1.0)   # default-stream churn
            q.finish()
        except Exception as exc:   # noqa: BLE001
            errors.append(exc)

    threads = [threading.Thread(target=worker, args=(t,)) for t in range(2)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    torch.cuda.synchronize()
    assert not errors, errors
    for per_thread in outs:
        for o in per_thread:
            assert torch.equal(o, eager)


@pytest.mark.timeout(600)
def test_contraction_is_much_faster_than_generic(torch_cuda):
    from feinsum_amd.measure import timeit_details

    expr = f.einsum("ik,kj->ij", f.array("A", (1024, 1024)), f.array("B", (1024, 1024)))
    t = {v: timeit_details(expr, transform=v, min_rounds=10, min_secs=0.3).seconds_device
         for v in ("contraction", "generic")}
    assert 5 * t["contraction"] < t["generic"], t
