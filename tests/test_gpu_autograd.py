"""evaluate_differentiable on the device: gradients of every DG family x order x layout against
torch.einsum autograd on the CPU, the two adjoint kernels bitwise exact on integer data, the forward bitwise that of
evaluate, reproducible gradients across runs and streams, untouched guard bands, gradcheck, partial gradients that
launch only what they need, and the adjoint kernels' speed floors."""

import numpy as np
import pytest

import autograd_cases as C
import feinsum_amd as f
from feinsum_amd import _hip, autograd
from feinsum_amd.autograd import adjoint_einsums, evaluate_differentiable

pytestmark = pytest.mark.gpu

E_ALL = (0, 1, 15, 16, 17, 100, 1000, 10007, 100007)
MAIN = [("grad_tet4", C.grad(3, 35)), ("div_tet4", C.div(3, 35)), ("divcomp_tet4", C.divcomp(3, 35)),
        ("matapply_tet4", C.matapply(35)), ("facemass_b1_tet4", C.face_mass(35, 4, 15, 1)),
        ("facemass_b4_fe_jfi_tet4", C.face_mass(35, 4, 15, 4, "fe", "jfi")), ("grad_tri5", C.grad(2, 21)),
        ("facemass_b4_tri5", C.face_mass(21, 3, 6, 4))]
EVERY = C.dg_cases()


@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    _hip.load_library()
    yield torch
    import gc

    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _device(torch, arrays, requires_grad=True):
    return {n: torch.from_numpy(np.ascontiguousarray(v)).to("cuda:0").requires_grad_(requires_grad)
            for n, v in arrays.items()}


def _device_grads(torch, einsum, inputs, gbar, q=None):
    dev = _device(torch, inputs)
    outs = evaluate_differentiable(einsum, q or 0, dev)
    torch.autograd.backward([outs[n] for n in einsum.output_names],
                            [torch.from_numpy(gbar[n]).to("cuda:0") for n in einsum.output_names])
    torch.cuda.synchronize()
    return {n: t.grad.cpu().numpy() for n, t in dev.items()}, outs


def _check_close(got, ref, what):
    err = np.abs(got - ref)
    scale = max(np.abs(ref).max(initial=0.0), 1e-300)
    assert err.max(initial=0.0) <= 1e-11 * scale, (what, err.max(initial=0.0) / scale)
    nref = np.linalg.norm(ref)
    if nref > 0:
        assert np.linalg.norm(got - ref) <= 1e-12 * nref, what


def _accuracy(torch, einsum, E, name):
    inputs = C.random_inputs(einsum, E)
    gbar = C.random_output_grads(einsum, E)
    got, _ = _device_grads(torch, einsum, inputs, gbar)
    ref = C.torch_reference_grads(einsum, inputs, gbar)
    for n in sorted(einsum.all_args):
        assert got[n].shape == ref[n].shape and got[n].dtype == np.dtype(einsum.arg_to_dtype[n])
        if got[n].dtype == np.float32:
            # a float32 operand's gradient is computed in float64 and rounded once: within half an ulp of float32
            scale = max(np.abs(ref[n]).max(initial=0.0), 1e-300)
            assert np.all(np.abs(got[n] - ref[n]) <= 2.0 ** -24 * np.abs(ref[n]) + 1e-11 * scale), (name, E, n)
        else:
            _check_close(got[n], ref[n], (name, E, n))


@pytest.mark.parametrize("E", E_ALL)
@pytest.mark.parametrize("name,einsum", MAIN, ids=[n for n, _ in MAIN])
def test_gradients_every_size(torch_cuda, name, einsum, E):
    _accuracy(torch_cuda, einsum, E, name)


@pytest.mark.parametrize("E", (17, 1000))
@pytest.mark.parametrize("name,einsum", EVERY, ids=[n for n, _ in EVERY])
def test_gradients_every_family_order_layout(torch_cuda, name, einsum, E):
    _accuracy(torch_cuda, einsum, E, name)


@pytest.mark.parametrize("name,einsum", C.other_cases(), ids=[n for n, _ in C.other_cases()])
def test_gradients_other_einsums(torch_cuda, name, einsum):
    _accuracy(torch_cuda, einsum, 1000, name)


def test_forward_is_bitwise_evaluate(torch_cuda):
    torch = torch_cuda
    for _, einsum in MAIN:
        inputs = C.random_inputs(einsum, 1003)
        dev = _device(torch, inputs)
        a = evaluate_differentiable(einsum, 0, dev)
        b = f.evaluate(einsum, 0, {n: t.detach() for n, t in dev.items()}, wait=True)
        for n in einsum.output_names:
            assert a[n].grad_fn is not None
            assert torch.equal(a[n].detach(), b[n])


@pytest.mark.parametrize("which", ("grad_J_tet4", "div_J_tri3", "divcomp_er_J_tet2", "matapply_J_tet3"))
def test_geomadj_exact_on_integers(torch_cuda, which):
    torch = torch_cuda
    ein = {"grad_J_tet4": C.grad(3, 35), "div_J_tri3": C.div(2, 10, "rji"), "divcomp_er_J_tet2": C.divcomp(3, 10, "er"),
           "matapply_J_tet3": C.matapply(20, "ji")}[which]
    (term,) = adjoint_einsums(ein, "J")
    for E in (1, 17, 1003):
        host = C.random_inputs(term, E, seed=7, integer=True)
        outs = f.evaluate(term, 0, _device(torch, host, False), transform="adjoint", wait=True)
        ref = C.numpy_forward(term, host)["_fe_out"]
        assert np.array_equal(outs["_fe_out"].cpu().numpy(), ref), (which, E)


@pytest.mark.parametrize("shape", ((35, 4, 15), (10, 4, 6), (21, 3, 6), (3, 3, 2)))
@pytest.mark.parametrize("layout", (("ef", "fij"), ("fe", "jfi")))
def test_facemass_adj_exact_on_integers(torch_cuda, shape, layout):
    torch = torch_cuda
    Np, nf, Nfp = shape
    fm = C.face_mass(Np, nf, Nfp, 3, *layout)
    (tv,) = adjoint_einsums(fm, "v1")
    (tj,) = adjoint_einsums(fm, "J")
    for E in (1, 17, 1003):
        host = C.random_inputs(fm, E, seed=8, integer=True)
        gb = C.random_output_grads(fm, E, seed=9, integer=True)
        arrays = dict(host, **{autograd.output_grad_name(n): v for n, v in gb.items()})
        dev = _device(torch, arrays, False)
        ov = f.evaluate(tv, 0, dev, transform="adjoint", wait=True)
        assert np.array_equal(ov["_fe_out"].cpu().numpy(), C.numpy_forward(tv, arrays)["_fe_out"])
        oj = f.evaluate(tj, 0, dev, transform="adjoint", wait=True)
        refj = C.numpy_forward(tj, arrays)
        for n in tj.output_names:
            assert np.array_equal(oj[n].cpu().numpy(), refj[n])
        # one launch: dv for every field and dJ summed over the fields
        J, R = dev["J"], dev["R"]
        g = [dev[autograd.output_grad_name(n)] for n in fm.output_names]
        v = [dev[f"v{k}"] for k in range(3)]
        dv = [torch.empty_like(x) for x in v]
        dJ = torch.empty_like(J)
        flags = (1 if layout[0] == "fe" else 0) | {"fij": 0, "ifj": 2, "fji": 4, "jfi": 6}[layout[1]]
        _hip.facemass_adj(J.data_ptr(), R.data_ptr(), [t.data_ptr() for t in g], [t.data_ptr() for t in v],
                          [t.data_ptr() for t in dv], dJ.data_ptr(), E, Np, nf, Nfp, flags)
        torch.cuda.synchronize()
        assert np.array_equal(dJ.cpu().numpy(), sum(refj[n] for n in tj.output_names))
        refv = adjoint_einsums(fm, "v2")[0]
        assert np.array_equal(dv[2].cpu().numpy(), C.numpy_forward(refv, arrays)["_fe_out"])


def test_gradients_reproducible_across_runs_and_streams(torch_cuda):
    torch = torch_cuda
    for _, einsum in MAIN:
        inputs = C.random_inputs(einsum, 10007)
        gbar = C.random_output_grads(einsum, 10007)
        first, _ = _device_grads(torch, einsum, inputs, gbar)
        again, _ = _device_grads(torch, einsum, inputs, gbar)
        side = torch.cuda.Stream()
        other, _ = _device_grads(torch, einsum, inputs, gbar, q=f.DeviceQueue(0, side))
        for n in first:
            assert np.array_equal(first[n], again[n]) and np.array_equal(first[n], other[n]), n


def test_guard_bands_untouched(torch_cuda):
    torch = torch_cuda
    E, Np, pad = 1003, 35, 4096
    rng = np.random.default_rng(3)
    D = torch.from_numpy(rng.standard_normal((3, Np, Np))).cuda()
    a = torch.from_numpy(rng.standard_normal((E, Np))).cuda()
    b = torch.from_numpy(rng.standard_normal((3, E, Np))).cuda()
    buf = torch.full((pad + 9 * E + pad,), float("nan"), dtype=torch.float64, device="cuda")
    out = buf[pad:pad + 9 * E]
    _hip.geomadj(D.data_ptr(), a.data_ptr(), b.data_ptr(), out.data_ptr(), E, 3, 3, Np, (3 * E, E, 1))
    torch.cuda.synchronize()
    assert torch.isnan(buf[:pad]).all() and torch.isnan(buf[pad + 9 * E:]).all()
    assert not torch.isnan(out).any()
    # face-mass adjoint: dv and dJ inside guard bands
    nf, Nfp = 4, 15
    R = torch.from_numpy(rng.standard_normal((nf, Np, Nfp))).cuda()
    J = torch.from_numpy(rng.standard_normal((E, nf))).cuda()
    g = torch.from_numpy(rng.standard_normal((E, Np))).cuda()
    v = torch.from_numpy(rng.standard_normal((nf, E, Nfp))).cuda()
    n_dv, n_dj = nf * E * Nfp, E * nf
    buf = torch.full((pad + n_dv + pad + n_dj + pad,), float("nan"), dtype=torch.float64, device="cuda")
    dv = buf[pad:pad + n_dv]
    dJ = buf[2 * pad + n_dv:2 * pad + n_dv + n_dj]
    _hip.facemass_adj(J.data_ptr(), R.data_ptr(), [g.data_ptr()], [v.data_ptr()], [dv.data_ptr()], dJ.data_ptr(),
                      E, Np, nf, Nfp)
    torch.cuda.synchronize()
    assert torch.isnan(buf[:pad]).all() and torch.isnan(buf[pad + n_dv:2 * pad + n_dv]).all()
    assert torch.isnan(buf[2 * pad + n_dv + n_dj:]).all()
    assert not torch.isnan(dv).any() and not torch.isnan(dJ).any()


@pytest.mark.parametrize("which", ("grad", "div", "facemass"))
def test_gradcheck(torch_cuda, which):
    torch = torch_cuda
    ein = {"grad": C.grad(3, 4), "div": C.div(3, 4), "facemass": C.face_mass(4, 4, 3, 2)}[which]
    names = sorted(ein.all_args)
    host = C.random_inputs(ein, 17, seed=11)
    tensors = [torch.from_numpy(host[n]).cuda().requires_grad_(True) for n in names]

    def fn(*ts):
        outs = evaluate_differentiable(ein, 0, dict(zip(names, ts)))
        return tuple(outs[n] for n in ein.output_names)

    assert torch.autograd.gradcheck(fn, tuple(tensors), eps=1e-6, atol=1e-8, rtol=1e-6)


def test_partial_gradients_launch_only_what_they_need(torch_cuda):
    torch = torch_cuda
    ein = C.grad(3, 35)
    host = C.random_inputs(ein, 1000)
    dev = _device(torch, host, False)
    dev["u"].requires_grad_(True)
    before = dict(autograd.launch_counts)
    out = evaluate_differentiable(ein, 0, dev)["_fe_out"]
    out.sum().backward()
    torch.cuda.synchronize()
    after = autograd.launch_counts
    assert after["geomadj"] == before.get("geomadj", 0)
    assert after["family"] == before.get("family", 0) + 1
    assert dev["J"].grad is None and dev["D"].grad is None and dev["u"].grad is not None
    with pytest.raises(RuntimeError):     # double backward is refused (once_differentiable)
        dev["u"].grad = None
        o2 = evaluate_differentiable(ein, 0, dev)["_fe_out"]
        (gu,) = torch.autograd.grad(o2.sum(), [dev["u"]], create_graph=True)
        gu.sum().backward()


# E = 10^6, p = 4: the adjoint kernels must stay above these fractions of the HBM roofline (8 TB/s): about half of
# what DESIGN.md §3l records
SPEED_FLOORS = {"geomadj": 0.22, "facemass_adj_dJ": 0.19}


def test_speed_floors(torch_cuda):
    torch = torch_cuda
    E, Np, nf, Nfp = 10 ** 6, 35, 4, 15
    rng = np.random.default_rng(0)
    dev = lambda *s: torch.from_numpy(rng.standard_normal(s)).cuda()   # noqa: E731
    D, a, b, out = dev(3, Np, Np), dev(E, Np), dev(3, E, Np), torch.empty((3, 3, E), dtype=torch.float64, device="cuda")
    R, J, g, v = dev(nf, Np, Nfp), dev(E, nf), dev(E, Np), dev(nf, E, Nfp)
    dv, dJ = torch.empty_like(v), torch.empty_like(J)
    runs = {
        "geomadj": (lambda: _hip.geomadj(D.data_ptr(), a.data_ptr(), b.data_ptr(), out.data_ptr(), E, 3, 3, Np,
                                         (3 * E, E, 1), stream=torch.cuda.current_stream().cuda_stream), 1192),
        "facemass_adj_dJ": (lambda: _hip.facemass_adj(J.data_ptr(), R.data_ptr(), [g.data_ptr()], [v.data_ptr()],
                                                      [dv.data_ptr()], dJ.data_ptr(), E, Np, nf, Nfp,
                                                      stream=torch.cuda.current_stream().cuda_stream), 1304),
    }
    for name, (run, nbytes) in runs.items():
        for _ in range(3):
            run()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(20):
            run()
        t1.record()
        t1.synchronize()
        sec = t0.elapsed_time(t1) * 1e-3 / 20
        frac = nbytes * E / 8e12 / sec
        assert frac >= SPEED_FLOORS[name], (name, sec, frac)
