"""Einsums that mix float32 and float64 operands on the device: float64 compute with float32 operands widened as
they are loaded (FE_DTYPE_OPERAND_F32), on the generic, pointwise and contraction paths.  Exact data that neither
float32 compute nor a narrowed float64 operand reproduces, np.einsum at 1e-10, validation through every transform,
write bounds, streams and graph capture, bitwise agreement with the all-float64 kernel on pre-converted operands, and
the speed bars of DESIGN.md §3j."""

import threading

import numpy as np
import pytest

import feinsum_amd as f
from feinsum_amd import _hip
from feinsum_amd.contraction_schedule import ContractionSchedule, EinsumOperand, IntermediateResult
from feinsum_amd.measure import generate_host_input_arrays, validation_dtype

import dg

pytestmark = pytest.mark.gpu

F32, F64 = "float32", "float64"


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


def _run(torch, expr, host, transform="contraction", schedule=None):
    dev = {k: torch.from_numpy(v).cuda() for k, v in host.items()}
    outs = f.evaluate(expr, 0, dev, transform=transform, wait=True, schedule=schedule)
    return {k: v.cpu().numpy() for k, v in outs.items()}


def _check(torch, expr, E=1, transform="contraction", schedule=None, seed=0):
    host = generate_host_input_arrays(expr, E, np_seed=seed)
    got, ref = _run(torch, expr, host, transform, schedule), _oracle(expr, host)
    rows = dict(zip(expr.output_names, range(len(expr.args))))
    assert set(got) == set(ref)
    for k in ref:
        assert got[k].dtype == ref[k].dtype and got[k].shape == ref[k].shape, k
        tol = 1e-10 if validation_dtype(expr, rows[k]) == np.float64 else 1e-5
        np.testing.assert_allclose(got[k], ref[k], rtol=tol, atol=tol)


def _retyped(expr, dtypes):
    """*expr* with the operands named in *dtypes* re-declared in those dtypes."""
    return f.batched_einsum(expr.get_subscripts(), [[a.copy(dtype=np.dtype(dtypes.get(a.name, a.dtype))) for a in row]
                                                    for row in expr.args])


# --------------------------------------------------------------------------
# exact data
# --------------------------------------------------------------------------

@pytest.mark.parametrize("eps_b, K", [(2.0**-40, 2), (2.0**-30, 256)])
@pytest.mark.parametrize("transform, subs", [
    ("generic", "ik,kj->ij"),
    ("generic", "ik,jk->ij"),        # contiguous summed index: groups of lanes per output
    ("contraction", "ik,kj->ij"),
    ("contraction", "ki,jk->ji"),
    ("contraction", "ik,kj->ji"),    # the launcher swaps A and B
])
@pytest.mark.parametrize("f32_operand", ["A", "B"])
def test_exact_float64_products(torch_cuda, eps_b, K, transform, subs, f32_operand):
    """float32 entries 1 + 2^-12 times float64 entries 1 + eps: every product 1 + 2^-12 + eps + 2^-12 eps is exact in
    float64 and so is every partial sum of up to K of them (eps = 2^-40: K = 2; eps = 2^-30: any K <= 1024).  float32
    compute loses eps, and so does narrowing the float64 operand to float32."""
    torch = torch_cuda
    M, N = 70, 33
    ext = {"i": M, "j": N, "k": K}
    a_sub, b_sub = subs.split("->")[0].split(",")
    small, fine = np.float32(1 + 2.0**-12), np.float64(1 + eps_b)
    if f32_operand == "A":
        A = np.full([ext[c] for c in a_sub], small, np.float32)
        B = np.full([ext[c] for c in b_sub], fine, np.float64)
    else:
        A = np.full([ext[c] for c in a_sub], fine, np.float64)
        B = np.full([ext[c] for c in b_sub], small, np.float32)
    expr = f.einsum(subs, f.array("A", A.shape, A.dtype), f.array("B", B.shape, B.dtype))
    got = _run(torch, expr, {"A": A, "B": B}, transform)["_fe_out"]
    p = (1 + 2.0**-12) * (1 + eps_b)
    assert p == 1 + 2.0**-12 + eps_b + 2.0**-12 * eps_b   # exact
    assert got.dtype == np.float64
    assert np.array_equal(got, np.full(got.shape, K * p)), (got.flat[0] - K * p)
    # what the wrong precisions would give differs
    assert K * float(np.float32(p)) != K * p and K * float(np.float32(fine)) * float(small) != K * p


@pytest.mark.parametrize("f32_operands", [("A",), ("B",), ("A", "C")])
def test_exact_pointwise(torch_cuda, f32_operands):
    torch = torch_cuda
    n = 100_003   # odd: the scalar tail after the pairs
    vals = {"A": 1 + 2.0**-12, "B": 1 + 2.0**-40, "C": 1 + 2.0**-20}
    host = {k: np.full((n,), v, np.float32 if k in f32_operands else np.float64) for k, v in vals.items()}
    expr = f.einsum("e,e,e->e", *[f.array(k, ("E",), host[k].dtype) for k in "ABC"])
    got = _run(torch, expr, host, "generic")["_fe_out"]
    ref = host["A"].astype(np.float64) * host["B"].astype(np.float64) * host["C"].astype(np.float64)
    assert got.dtype == np.float64 and np.array_equal(got, ref)
    # the float64 values are not float32 ones: a narrowed or float32-computed product would differ
    assert not np.array_equal(ref, (host["A"].astype(np.float32) * host["B"].astype(np.float32)
                                    * host["C"].astype(np.float32)).astype(np.float64))
    # misaligned pairs: a float32 view 4 bytes in, a float64 one 8 bytes in (the scalar path)
    dev = {}
    for k, v in host.items():
        buf = torch.empty(v.size + 1, dtype=getattr(torch, v.dtype.name), device="cuda")
        buf[1:] = torch.from_numpy(v).cuda()
        dev[k] = buf[1:]
    out = f.evaluate(expr, 0, dev, transform="generic", wait=True)["_fe_out"]
    assert np.array_equal(out.cpu().numpy(), ref)


# --------------------------------------------------------------------------
# against np.einsum
# --------------------------------------------------------------------------

@pytest.mark.parametrize("da, db", [(F32, F64), (F64, F32), (F32, F32), (F64, F64)])
@pytest.mark.parametrize("M, N, K, ta, tb, tc", [
    (1000, 777, 513, False, False, False),
    (1000, 777, 513, True, True, False),
    (128, 96, 64, False, True, True),       # 16-byte groups, output transposed (A and B swap)
    (67, 64, 128, True, False, False),
    (64, 70, 36, False, False, True),
])
def test_gemms(torch_cuda, da, db, M, N, K, ta, tb, tc):
    a = "ki" if ta else "ik"
    b = "jk" if tb else "kj"
    c = "ji" if tc else "ij"
    ext = {"i": M, "j": N, "k": K}
    expr = f.einsum(f"{a},{b}->{c}", f.array("A", tuple(ext[x] for x in a), da),
                    f.array("B", tuple(ext[x] for x in b), db))
    _check(torch_cuda, expr, seed=M + N + K)
    if (da, db) in ((F32, F64), (F64, F32)) and M < 1000:
        _check(torch_cuda, expr, transform="generic", seed=1)


@pytest.mark.parametrize("subs, shapes", [
    ("abcd,ea->ebcd", [(6, 5, 4, 7), (9, 6)]),
    ("abc,bda->dc", [(5, 6, 7), (6, 8, 5)]),
    ("ijkl,klmn->ijmn", [(3, 4, 5, 6), (5, 6, 7, 2)]),
    ("ijkl,klmn->ijmn", [(8, 8, 8, 8), (8, 8, 8, 8)]),
])
@pytest.mark.parametrize("dts", [(F32, F64), (F64, F32)])
def test_multi_index_groups(torch_cuda, subs, shapes, dts):
    expr = f.einsum(subs, *[f.array(n, s, dt) for n, s, dt in zip("AB", shapes, dts)])
    _check(torch_cuda, expr)


@pytest.mark.timeout(300)
def test_long_and_batched(torch_cuda):
    erj = f.einsum("erj,rij->ei", f.array("u", ("E", 3, 35), F32), f.array("D", (3, 35, 35)))
    _check(torch_cuda, erj, E=100_007, seed=3)
    _check(torch_cuda, erj, E=100_007, transform="generic", seed=3)
    bij = f.einsum("bij,bjk->bik", f.array("A", ("E", 3, 4)), f.array("B", ("E", 4, 5), F32))
    _check(torch_cuda, bij, E=100_000, seed=4)
    bij = f.einsum("bij,bjk->bik", f.array("A", ("E", 8, 8), F32), f.array("B", ("E", 8, 8)))
    _check(torch_cuda, bij, E=100_000, seed=5)


def test_stride0_and_offset_operands(torch_cuda):
    torch = torch_cuda
    # 'ij,kj->ik' with B[k, j] = w[j] (float32, expanded: stride 0), straight through the C ABI
    rng = np.random.default_rng(5)
    A = torch.from_numpy(rng.random((300, 70))).cuda()
    w = torch.from_numpy(rng.random(70).astype(np.float32)).cuda()
    Bx = w.expand(90, 70)
    out = torch.empty(300, 90, dtype=torch.float64, device="cuda")
    d = _hip.EinsumDesc()
    d.n_operands, d.n_out, d.n_sum, d.dtype = 2, 2, 1, _hip.FE_DTYPE_F64 | _hip.FE_DTYPE_OPERAND_F32(1)
    d.out_extent[0], d.out_extent[1], d.sum_extent[0] = 300, 90, 70
    d.op_out_stride[0][0], d.op_sum_stride[0][0] = A.stride(0), A.stride(1)
    d.op_out_stride[1][1], d.op_sum_stride[1][0] = Bx.stride(0), Bx.stride(1)
    assert Bx.stride(0) == 0
    ref = np.einsum("ij,kj->ik", A.cpu().numpy(), Bx.cpu().numpy().astype(np.float64))
    for fn in (_hip.einsum_contract, _hip.einsum_generic):
        out.fill_(float("nan"))
        fn(d, [A.data_ptr(), Bx.data_ptr()], out.data_ptr(), 0)
        torch.cuda.synchronize()
        np.testing.assert_allclose(out.cpu().numpy(), ref, rtol=1e-12, atol=0)
    # float32 operands 4 bytes past a 16-byte boundary, float64 ones 8: only element alignment, vector-friendly shapes
    for subs, shapes in (("ik,kj->ij", [(130, 64), (64, 96)]), ("ki,kj->ij", [(64, 128), (64, 96)])):
        for dts in ((F32, F64), (F64, F32)):
            expr = f.einsum(subs, *[f.array(n, s, dt) for n, s, dt in zip("AB", shapes, dts)])
            host = generate_host_input_arrays(expr, 1, np_seed=7)
            dev = {}
            for k, v in host.items():
                buf = torch.empty(v.size + 1, dtype=getattr(torch, v.dtype.name), device="cuda")
                buf[1:] = torch.from_numpy(v).cuda().reshape(-1)
                dev[k] = buf[1:].view(v.shape)
            ref = _oracle(expr, host)["_fe_out"]
            for transform in ("contraction", "generic"):
                got = f.evaluate(expr, 0, dev, transform=transform, wait=True)["_fe_out"].cpu().numpy()
                np.testing.assert_allclose(got, ref, rtol=1e-10, atol=1e-10)


def _chain(dts):
    return f.einsum("ij,jk,kl->il", *[f.array(n, s, dt) for n, s, dt in zip("ABC", [(130, 70), (70, 90), (90, 40)], dts)])


def _chain_sched():
    return ContractionSchedule(("ij,jk->ik", "ik,kl->il"), ("t", "_fe_out"),
                               ((EinsumOperand(0), EinsumOperand(1)), (IntermediateResult("t"), EinsumOperand(2))))


@pytest.mark.parametrize("dts", [(F32, F32, F64), (F64, F32, F32), (F32, F64, F32), (F64, F32, F64)])
def test_schedules(torch_cuda, dts):
    """Two float32 operands can meet in a step (a float32 intermediate, or numpy's own float32 step in the oracle):
    float32 tolerances then (measure.validation_dtype); one float32 operand: 1e-10."""
    expr = _chain(dts)
    for transform in ("contraction", "generic"):
        _check(torch_cuda, expr, transform=transform)
    _check(torch_cuda, expr, schedule=_chain_sched())   # (A B) first: a float32 intermediate when A, B are float32


@pytest.mark.timeout(300)
@pytest.mark.parametrize("make, f32", [(dg.grad, ("J",)), (dg.grad, ("u",)), (dg.div, ("J",)), (dg.div, ("u",))])
def test_dg_einsums(torch_cuda, make, f32):
    expr = _retyped(make(), {n: F32 for n in f32})
    from feinsum_amd.family import match_family

    assert match_family(expr) is None
    for transform in ("auto", "contraction"):
        _check(torch_cuda, expr, E=1003, transform=transform, seed=2)


@pytest.mark.parametrize("transform", [None, "generic", "contraction"])
def test_validate_transform(torch_cuda, transform):
    gemm = f.einsum("ik,kj->ij", f.array("A", (96, 64), F32), f.array("B", (64, 80)))
    erj = f.einsum("erj,rij->ei", f.array("u", ("E", 3, 35), F32), f.array("D", (3, 35, 35)))
    for expr in (gemm, erj, _chain((F64, F32, F32)), _retyped(dg.grad(), {"J": F32})):
        f.validate_batched_einsum_transform(expr, 0, transform)


# --------------------------------------------------------------------------
# bounds, streams, graphs
# --------------------------------------------------------------------------

def test_writes_only_its_output(torch_cuda):
    torch = torch_cuda
    guard = 4096
    cases = [f.einsum("ik,kj->ij", f.array("A", (129, 65), F32), f.array("B", (65, 257))),
             f.einsum("ki,jk->ji", f.array("A", (33, 70)), f.array("B", (17, 33), F32)),
             f.einsum("bij,bjk->bik", f.array("A", ("E", 3, 4), F32), f.array("B", ("E", 4, 5))),
             f.einsum("abcd,ea->ebcd", f.array("A", (6, 5, 4, 7)), f.array("B", (9, 6), F32)),
             f.einsum("ej,ej->ej", f.array("A", ("E", 7), F32), f.array("B", ("E", 7))),
             _retyped(dg.grad(), {"u": F32})]
    for transform in ("contraction", "generic"):
        for expr in cases:
            host = generate_host_input_arrays(expr, 1003, np_seed=1)
            dev = {k: torch.from_numpy(v).cuda() for k, v in host.items()}
            shape = tuple(1003 if isinstance(d, f.SizeParam) else int(d) for d in expr.shape)
            n = int(np.prod(shape))
            buf = torch.full((n + 2 * guard,), -7.25, dtype=torch.float64, device="cuda")
            out = buf[guard:guard + n].view(shape)
            f.evaluate(expr, 0, dev, out_dict={"_fe_out": out}, transform=transform, wait=True)
            assert bool((buf[:guard] == -7.25).all()) and bool((buf[guard + n:] == -7.25).all()), expr.get_subscripts()
            np.testing.assert_allclose(out.cpu().numpy(), _oracle(expr, host)["_fe_out"], rtol=1e-10, atol=1e-10)


def test_streams_and_graph_capture(torch_cuda):
    torch = torch_cuda
    expr = f.einsum("ik,kj->ij", f.array("A", (300, 200), F32), f.array("B", (200, 170)))
    host = generate_host_input_arrays(expr, 1, np_seed=9)
    dev = {k: torch.from_numpy(v).cuda() for k, v in host.items()}
    eager = f.evaluate(expr, 0, dev, transform="contraction", wait=True)["_fe_out"].clone()
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
    # one captured graph: a single launch, no parallel branches; replayed once
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


# --------------------------------------------------------------------------
# the same values in one dtype, and speed
# --------------------------------------------------------------------------

@pytest.mark.parametrize("case", ["gemm_a", "gemm_b", "erj"])
def test_bitwise_equal_to_preconverted(torch_cuda, case):
    """The mixed kernel and the all-float64 one on the float32 operand converted beforehand: same k order, same MFMA."""
    torch = torch_cuda
    if case == "erj":
        subs, shapes, f32 = "erj,rij->ei", {"A": (20_011, 3, 35), "B": (3, 35, 35)}, "A"
    else:
        subs, shapes, f32 = "ik,kj->ij", {"A": (700, 512), "B": (512, 388)}, case[-1].upper()
    gen = torch.Generator(device="cuda").manual_seed(23)
    dev = {k: torch.rand(s, dtype=torch.float64, device="cuda", generator=gen) for k, s in shapes.items()}
    dev[f32] = dev[f32].to(torch.float32)
    mixed = f.einsum(subs, *[f.array(k, s, F32 if k == f32 else F64) for k, s in shapes.items()])
    uniform = f.einsum(subs, *[f.array(k, s) for k, s in shapes.items()])
    got = f.evaluate(mixed, 0, dev, transform="contraction", wait=True)["_fe_out"]
    conv = dict(dev, **{f32: dev[f32].to(torch.float64)})
    ref = f.evaluate(uniform, 0, conv, transform="contraction", wait=True)["_fe_out"]
    assert got.dtype == torch.float64 and torch.equal(got, ref)


def _seconds(torch, launch, min_secs=0.3):
    launch()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    n, total = 0, 0.0
    while total < min_secs:
        t0.record()
        for _ in range(5):
            launch()
        t1.record()
        t1.synchronize()
        total += t0.elapsed_time(t1) * 1e-3
        n += 5
    return total / n


@pytest.mark.timeout(300)
def test_speed_bars(torch_cuda):
    torch = torch_cuda
    gen = torch.Generator(device="cuda").manual_seed(29)
    # erj,rij->ei at E = 1e6, u float32: the mixed launch beats cast + all-float64
    u = torch.rand(10**6, 3, 35, dtype=torch.float32, device="cuda", generator=gen)
    D = torch.rand(3, 35, 35, dtype=torch.float64, device="cuda", generator=gen)
    mixed = f.einsum("erj,rij->ei", f.array("u", ("E", 3, 35), F32), f.array("D", (3, 35, 35)))
    uniform = f.einsum("erj,rij->ei", f.array("u", ("E", 3, 35)), f.array("D", (3, 35, 35)))
    out = torch.empty(10**6, 35, dtype=torch.float64, device="cuda")
    t_mixed = _seconds(torch, lambda: f.evaluate(mixed, 0, {"u": u, "D": D}, out_dict={"_fe_out": out},
                                                 transform="contraction"))
    t_cast = _seconds(torch, lambda: f.evaluate(uniform, 0, {"u": u.to(torch.float64), "D": D},
                                                out_dict={"_fe_out": out}, transform="contraction"))
    assert t_mixed < t_cast, (t_mixed, t_cast)
    # ik,kj->ij 4096^3, A float32: at least 0.9x the all-float64 contraction's rate
    n = 4096
    A = torch.rand(n, n, dtype=torch.float32, device="cuda", generator=gen)
    B = torch.rand(n, n, dtype=torch.float64, device="cuda", generator=gen)
    A64 = A.to(torch.float64)
    C = torch.empty(n, n, dtype=torch.float64, device="cuda")
    mixed = f.einsum("ik,kj->ij", f.array("A", (n, n), F32), f.array("B", (n, n)))
    uniform = f.einsum("ik,kj->ij", f.array("A", (n, n)), f.array("B", (n, n)))
    t_mixed = _seconds(torch, lambda: f.evaluate(mixed, 0, {"A": A, "B": B}, out_dict={"_fe_out": C},
                                                 transform="contraction"), 1.0)
    t_f64 = _seconds(torch, lambda: f.evaluate(uniform, 0, {"A": A64, "B": B}, out_dict={"_fe_out": C},
                                               transform="contraction"), 1.0)
    assert t_mixed <= t_f64 / 0.9, (t_mixed, t_f64)
