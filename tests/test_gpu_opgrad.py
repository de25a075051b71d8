"""Operator gradients (dD, dR) on the matrix cores, on the device: exact on integer data through
``evaluate(transform="operator_adjoint")`` and ``.backward()`` with ``operator_gradients="kernel"``, within
``gamma(n, u) absref`` of the long-double reference on signed data, guard bands and planted NaNs through the C ABI,
reproducibility across runs, threads and a graph replay, routing and the aliasing refusal."""

import threading

import numpy as np
import pytest

import autograd_cases as C
import feinsum_amd as f
from feinsum_amd import _hip, autograd
from feinsum_amd.autograd import adjoint_einsums, output_grad_name
from feinsum_amd.diagnostics import InvalidParameterError
from oracle import einsum_ref as ref

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SMALL_E = [0, 1, 3, 4, 5, 15, 16, 17, 63, 64, 65]
S2_E = 65                    # smallest E with two slices (fe_opgrad_plan: S = min(1024, ceil(E / 64)))
CAP_E = 64 * 1023 + 1        # smallest E at which S reaches its cap
PLAN_E = [S2_E, S2_E + 1, CAP_E, CAP_E + 17]
BITS = 4                     # |mantissa| < 2^4 per operand: E X 2^(3 BITS) stays below 2^53 for every E here
FWD = [(n, e) for n, e in C.dg_cases() if "noj" not in n]


def test_sizes_follow_the_plan_and_the_bit_budget():
    assert _hip.opgrad_plan(S2_E - 1, 48)[0] == 1 and _hip.opgrad_plan(S2_E, 48)[0] == 2
    assert _hip.opgrad_plan(CAP_E - 1, 48)[0] == 1023 and _hip.opgrad_plan(CAP_E, 48)[0] == 1024 == _hip.opgrad_plan(10 ** 7, 48)[0]
    assert ref.bits_fit([BITS] * 3, max(PLAN_E) * 3 * 17, 53)       # (17 rows of a batched term included)


def _term(name, e):
    (t,) = adjoint_einsums(e, "R" if name.startswith("facemass") else "D")
    return t


def _ints(t, E, seed):
    rng = np.random.default_rng(seed)
    top = (1 << BITS) - 1
    return {n: rng.integers(-top, top + 1, size=C.concrete(t.arg_to_shape[n], E)).astype(np.float64)
            for n in sorted(t.all_args)}


def _int_reference(t, host):
    sub = t.get_subscripts().replace(" ", "")
    return [np.einsum(sub, *[host[a.name].astype(np.int64) for a in row], optimize=True).astype(np.float64) for row in t.args]


def _dev(host):
    return {n: torch.from_numpy(v).cuda() for n, v in host.items()}


@pytest.mark.parametrize("name,e", FWD, ids=[n for n, _ in FWD])
def test_exact_through_the_transform(name, e):
    t = _term(name, e)
    for E in SMALL_E + PLAN_E:
        host = _ints(t, E, E)
        outs = f.evaluate(t, 0, _dev(host), transform="operator_adjoint")
        for out_name, want in zip(t.output_names, _int_reference(t, host)):
            got = outs[out_name].cpu().numpy()
            assert ref.bitwise_equal(got, want), (name, E, int((got != want).sum()))


@pytest.mark.parametrize("b", [1, 8, 9, 17])
@pytest.mark.parametrize("jl,rl", C.FM_LAYOUTS)
def test_exact_backward_of_face_mass(b, jl, rl):
    _backward_is_exact(C.face_mass(35, 4, 15, b, jl, rl), "R", 133, {"facemass_v": b, "facemass_j": 1, "opgrad_r": 1})


@pytest.mark.parametrize("name,e,counts", [
    ("grad", C.grad(3, 35), {"geomadj": 1, "family": 1, "opgrad_d": 1}),
    ("grad_rji", C.grad(3, 20, "rji"), {"geomadj": 1, "family": 1, "opgrad_d": 1}),
    ("div", C.div(3, 35), {"geomadj": 1, "family": 1, "opgrad_d": 1}),
    ("div_tri", C.div(2, 21, "rji"), {"geomadj": 1, "family": 1, "opgrad_d": 1}),
    ("divcomp_er", C.divcomp(3, 10, "er", "rji"), {"geomadj": 1, "family": 1, "opgrad_d": 1}),
    ("matapply", C.matapply(15, "ji"), {"geomadj": 1, "family": 1, "opgrad_d": 1})], ids=lambda v: v if isinstance(v, str) else "")
def test_exact_backward_of_the_volume_families(name, e, counts):
    _backward_is_exact(e, "D", 133, counts)


def _backward_is_exact(e, op, E, counts):
    rng = np.random.default_rng(E)
    top = (1 << BITS) - 1
    host = {n: rng.integers(-top, top + 1, size=C.concrete(e.arg_to_shape[n], E)).astype(np.float64) for n in sorted(e.all_args)}
    gout = {n: rng.integers(-top, top + 1, size=C.concrete(e.shape, E)).astype(np.float64) for n in e.output_names}
    dev = {n: torch.from_numpy(v).cuda().requires_grad_(True) for n, v in host.items()}
    outs = f.evaluate_differentiable(e, 0, dev, operator_gradients="kernel")
    before = dict(autograd.launch_counts)
    torch.autograd.backward([outs[n] for n in e.output_names], [torch.from_numpy(gout[n]).cuda() for n in e.output_names])
    delta = {k: v - before.get(k, 0) for k, v in autograd.launch_counts.items() if v != before.get(k, 0)}
    assert delta == counts
    want = C.numpy_adjoint_grad(e, op, host, gout)      # small integers: float64 sums are exact in any order
    assert ref.bitwise_equal(dev[op].grad.cpu().numpy(), want)


def test_default_routes_are_unchanged_and_fall_back():
    for e, kw, expect in ((C.grad(3, 35), {}, {"geomadj": 1, "family": 1, "auto": 1}),
                          (C.grad(3, 56), {"operator_gradients": "kernel"}, None)):
        host = C.random_inputs(e, 70, integer=True)
        dev = {n: torch.from_numpy(v).cuda().requires_grad_(True) for n, v in host.items()}
        gout = C.random_output_grads(e, 70, integer=True)
        before = dict(autograd.launch_counts)
        outs = f.evaluate_differentiable(e, 0, dev, **kw)
        outs["_fe_out"].backward(torch.from_numpy(gout["_fe_out"]).cuda())
        delta = {k: v - before.get(k, 0) for k, v in autograd.launch_counts.items() if v != before.get(k, 0)}
        assert "opgrad_d" not in delta and (expect is None or delta == expect)
        assert ref.bitwise_equal(dev["D"].grad.cpu().numpy(), C.numpy_adjoint_grad(e, "D", host, gout))
    # float32 under "kernel": today's route, today's gradient
    e = f.einsum("xre,rij,ej->xei", f.array("J", (3, 3, "E"), "float32"), f.array("D", (3, 35, 35), "float32"),
                 f.array("u", ("E", 35), "float32"))
    host = C.random_inputs(e, 70, integer=True)
    gout = C.random_output_grads(e, 70, integer=True)
    grads = []
    for mode in ("auto", "kernel"):
        dev = {n: torch.from_numpy(v).cuda().requires_grad_(True) for n, v in host.items()}
        f.evaluate_differentiable(e, 0, dev, operator_gradients=mode)["_fe_out"].backward(torch.from_numpy(gout["_fe_out"]).cuda())
        grads.append(dev["D"].grad.cpu().numpy())
    assert np.array_equal(grads[0], grads[1])


@pytest.mark.parametrize("name,e,E", [("grad_p4", C.grad(3, 35), 1003), ("div_p3", C.div(3, 20, "rji"), 517),
                                      ("facemass_b4", C.face_mass(35, 4, 15, 4, "fe", "jfi"), 777)], ids=lambda v: v if isinstance(v, str) else "")
def test_signed_data_within_the_bound(name, e, E):
    t = _term(name if name.startswith("facemass") else "grad", e)
    host = C.random_inputs(t, E, seed=3)
    outs = f.evaluate(t, 0, _dev(host), transform="operator_adjoint")
    sub = t.get_subscripts().replace(" ", "")
    X = 3 if "x" in sub else 1
    slices = _hip.opgrad_plan(E, 48)[0]
    n = 2 + E * X + 6 + -(-slices // 64)     # products per entry + the combine: a lane's slices in order, six butterfly steps
    for out_name, row in zip(t.output_names, t.args):
        r, absr = ref.bounded_reference(sub, [host[a.name] for a in row])
        assert ref.bound_violations(outs[out_name].cpu().numpy(), r, absr, n, 2.0 ** -53) == 0
    if not name.startswith("facemass"):      # dD from "kernel" and from "auto" agree within the same bound
        auto = f.evaluate(t, 0, _dev(host))["_fe_out"].cpu().numpy()
        r, absr = ref.bounded_reference(sub, [host[a.name] for a in t.args[0]])
        assert ref.bound_violations(auto, r, absr, n, 2.0 ** -53) == 0


def test_backward_under_kernel_and_auto_agree_within_the_bound():
    e, E = C.grad(3, 35), 1003
    host, gout = C.random_inputs(e, E, seed=7), C.random_output_grads(e, E, seed=8)
    dD = {}
    for mode in ("auto", "kernel"):
        dev = {n: torch.from_numpy(v).cuda().requires_grad_(True) for n, v in host.items()}
        f.evaluate_differentiable(e, 0, dev, operator_gradients=mode)["_fe_out"].backward(torch.from_numpy(gout["_fe_out"]).cuda())
        dD[mode] = dev["D"].grad.cpu().numpy().astype(np.longdouble)
    _, absr = ref.bounded_reference("xre,ej,xei->rij", [host["J"], host["u"], gout["_fe_out"]])
    n = 2 + 3 * E + 6 + -(-_hip.opgrad_plan(E, 48)[0] // 64)
    # each is within gamma(n, u) absref of the exact value (both sum 3 E products per entry, "auto" with no deeper a tree than
    # E): they differ by at most twice that
    assert (np.abs(dD["kernel"] - dD["auto"]) <= 2 * np.longdouble(ref.gamma(n, 2.0 ** -53)) * absr).all()


def _banded(arr, band=37):
    """*arr* inside a larger NaN-filled device buffer (an odd number of elements in front: 8-byte alignment only)."""
    buf = torch.full((arr.size + 2 * band,), float("nan"), dtype=torch.float64, device="cuda")
    buf[band:band + arr.size] = torch.from_numpy(np.ascontiguousarray(arr).reshape(-1)).cuda()
    return buf, buf[band:band + arr.size]


def _bands_untouched(buf, band=37):
    return bool(torch.isnan(buf[:band]).all() and torch.isnan(buf[-band:]).all())


_J_STRIDES = {"xre": lambda R, E: (R * E, E, 1), "re": lambda R, E: (0, E, 1), "er": lambda R, E: (0, 1, R),
              "e": lambda R, E: (0, 0, 1)}


def _run_banded(launch, operands, n_out, entries, E):
    """*launch*(operand pointers, out pointer, workspace pointer, bytes) with every array between NaN bands: the output as
    a flat array, after checking that no band and nothing behind the workspace's planned bytes was written."""
    bufs = [_banded(v) for v in operands]
    obuf, od = _banded(np.full(n_out, np.nan))
    nbytes = _hip.opgrad_plan(E, entries)[1]
    ws = torch.full((nbytes // 8 + 32,), float("nan"), dtype=torch.float64, device="cuda")
    launch([d.data_ptr() for _, d in bufs], od.data_ptr(), ws.data_ptr() if nbytes else None, nbytes)
    got = od.cpu().numpy()
    assert all(_bands_untouched(buf) for buf, _ in bufs) and _bands_untouched(obuf)
    assert bool(torch.isnan(ws[nbytes // 8:]).all())
    return got


@pytest.mark.parametrize("Np,X,R,jl,ol", [(3, 2, 2, "xre", "rqp"), (4, 3, 3, "xre", "rpq"), (6, 1, 2, "re", "rpq"),
                                         (10, 1, 3, "er", "rqp"), (15, 1, 1, "e", "rpq"), (20, 3, 3, "xre", "rqp"),
                                         (21, 2, 2, "xre", "rpq"), (35, 3, 3, "xre", "rpq"), (35, 1, 3, "er", "rqp"),
                                         (35, 1, 3, "re", "rpq")])
def test_c_abi_between_guard_bands_with_planted_nans(Np, X, R, jl, ol):
    rng = np.random.default_rng(Np)
    stream = torch.cuda.current_stream().cuda_stream
    ostrides = (Np * Np, Np, 1) if ol == "rpq" else (Np * Np, 1, Np)
    for E in SMALL_E + PLAN_E[:2]:
        J = rng.integers(-3, 4, size=(X, R, E)).astype(np.float64)
        a = rng.integers(-3, 4, size=(E, Np)).astype(np.float64)
        b = rng.integers(-3, 4, size=(X, E, Np)).astype(np.float64)
        want = np.einsum("xre,eq,xep->rpq", J, a, b)
        plants = [None] + ([("a", E - 1, Np - 1), ("a", E // 2, 0), ("J", E // 2, R - 1)] if E else [])
        for plant in plants:
            Jh, ah = J.copy(), a.copy()
            nan = np.zeros((R, Np, Np), dtype=bool)
            if plant and plant[0] == "a":
                ah[plant[1], plant[2]] = np.nan
                nan[:, :, plant[2]] = True
            if plant and plant[0] == "J":
                Jh[X - 1, plant[2], plant[1]] = np.nan
                nan[plant[2]] = True
            Jstored = np.ascontiguousarray(Jh[0].T) if jl == "er" else Jh

            def launch(ptrs, out, ws, nbytes):
                _hip.opgrad(ptrs[0], [ptrs[1]], [ptrs[2]], out, E, X, R, Np, _J_STRIDES[jl](R, E), ostrides, ws, nbytes,
                            stream=stream)

            got = _run_banded(launch, (Jstored, ah, b), R * Np * Np, R * Np * Np, E).reshape(R, Np, Np)
            got = got if ol == "rpq" else got.transpose(0, 2, 1)
            assert np.array_equal(np.isnan(got), nan), (E, plant)
            assert np.array_equal(got[~nan], want[~nan]), (E, plant)


_FM_PERM = {0: (0, 1, 2), f.family.FM_R_IFJ: (1, 0, 2), f.family.FM_R_T: (0, 2, 1),
            f.family.FM_R_IFJ | f.family.FM_R_T: (2, 0, 1)}       # dR [f][i][j] stored as 'fij', 'ifj', 'fji', 'jfi'
_FM_CASES = ([((4, 35, 15), flags, b) for flags in range(8) for b in (1, 8, 9, 17)]
             + [(shape, k % 8, (1, 9)[k % 2]) for k, shape in enumerate(f.family.FACEMASS_ADJ_SHAPES) if shape != (4, 35, 15)])


@pytest.mark.parametrize("shape,flags,b", _FM_CASES)
def test_face_mass_c_abi_between_guard_bands_with_planted_nans(shape, flags, b):
    nf, Np, Nfp = shape
    rng = np.random.default_rng(flags + 8 * b)
    stream = torch.cuda.current_stream().cuda_stream
    perm = _FM_PERM[flags & (f.family.FM_R_IFJ | f.family.FM_R_T)]
    for E in (SMALL_E + PLAN_E[:2]) if b == 1 else [0, 5, 17, 65, 66]:
        J = rng.integers(-3, 4, size=(E, nf)).astype(np.float64)
        g = rng.integers(-3, 4, size=(b, E, Np)).astype(np.float64)
        v = rng.integers(-3, 4, size=(b, nf, E, Nfp)).astype(np.float64)
        want = np.einsum("kei,ef,kfej->fij", g, J, v)
        plants = [None] + ([("g", E - 1, Np - 1), ("g", E // 2, 0), ("J", E // 2, nf - 1)] if E else [])
        for plant in plants:
            Jh, gh = J.copy(), g.copy()
            nan = np.zeros((nf, Np, Nfp), dtype=bool)
            if plant and plant[0] == "g":
                gh[b - 1, plant[1], plant[2]] = np.nan      # (the last field: past the first launch when b > 8)
                nan[:, plant[2], :] = True
            if plant and plant[0] == "J":
                Jh[plant[1], plant[2]] = np.nan
                nan[plant[2]] = True
            Jstored = np.ascontiguousarray(Jh.T) if flags & f.family.FM_J_FE else Jh

            def launch(ptrs, out, ws, nbytes):
                _hip.facemass_opgrad(ptrs[0], ptrs[1:1 + b], ptrs[1 + b:], out, E, Np, nf, Nfp, ws, nbytes,
                                     layout_flags=flags, stream=stream)

            got = _run_banded(launch, (Jstored, *gh, *v), nf * Np * Nfp, nf * Np * Nfp, E)
            got = got.reshape([(nf, Np, Nfp)[k] for k in perm]).transpose(np.argsort(perm))
            assert np.array_equal(np.isnan(got), nan), (E, plant)
            assert np.array_equal(got[~nan], want[~nan]), (E, plant)


@pytest.mark.parametrize("E", [37, 4099])
def test_bitwise_reproducible_across_runs_threads_and_a_graph_replay(E):
    t = _term("grad", C.grad(3, 35))
    host = C.random_inputs(t, E, seed=5)
    dev = _dev(host)
    first = f.evaluate(t, 0, dev, transform="operator_adjoint")["_fe_out"].clone()
    assert torch.equal(first, f.evaluate(t, 0, dev, transform="operator_adjoint")["_fe_out"])
    results = [None, None]

    def work(k):
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.default_stream())
        q = f.DeviceQueue(0, s)
        results[k] = f.evaluate(t, q, dev, transform="operator_adjoint", wait=True)["_fe_out"]

    threads = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    [th.start() for th in threads]
    [th.join() for th in threads]
    assert torch.equal(first, results[0]) and torch.equal(first, results[1])
    out = {"_fe_out": torch.zeros_like(first)}
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        f.evaluate(t, 0, dev, out_dict=out, transform="operator_adjoint")      # (kernels configured before the capture)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        f.evaluate(t, 0, dev, out_dict=out, transform="operator_adjoint")
    out["_fe_out"].zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(first, out["_fe_out"])


def test_an_output_overlapping_an_input_is_refused():
    t = _term("grad", C.grad(3, 35))
    dev = _dev(C.random_inputs(t, 35, seed=1))
    g = dev[output_grad_name("_fe_out")]          # [3][35][35] at E = 35: the output's own shape
    with pytest.raises(InvalidParameterError, match="shares memory"):
        f.evaluate(t, 0, dev, out_dict={"_fe_out": g.reshape(3, 35, 35)}, transform="operator_adjoint")


# half of the speed-ups over "auto" measured on MI355X at E = 10^6, p = 4 (profiles/autograd/bench_opgrad.jsonl)
SPEED_FLOORS = {"opgrad_d": 41.0, "opgrad_r_b4": 14.7}      # measured: 82.7x and 29.5x


def test_speed_floors_over_auto():
    from feinsum_amd.measure import _bind

    def seconds(launch, reps):
        launch()
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(reps):
            launch()
        t1.record()
        t1.synchronize()
        return t0.elapsed_time(t1) * 1e-3 / reps

    E = 10 ** 6
    for case, fwd, wrt in (("opgrad_d", C.grad(3, 35), "D"), ("opgrad_r_b4", C.face_mass(35, 4, 15, 4), "R")):
        (t,) = adjoint_einsums(fwd, wrt)
        rng = np.random.default_rng(0)
        dev = {n: torch.from_numpy(rng.standard_normal(C.concrete(t.arg_to_shape[n], E))).cuda() for n in sorted(t.all_args)}
        per = {}
        for transform, reps in (("operator_adjoint", 20), ("auto", 3)):
            q, bound, _ = _bind(t, 0, dev, None, transform)
            per[transform] = seconds(lambda: bound.launch(q.stream_ptr), reps)
        speedup = per["auto"] / per["operator_adjoint"]
        print(f"{case}: kernel {per['operator_adjoint'] * 1e3:.3f} ms, auto {per['auto'] * 1e3:.3f} ms, {speedup:.1f}x")
        assert speedup >= SPEED_FLOORS[case], (case, per, speedup)
        del dev
