"""Accumulating evaluation on the device: ``evaluate(..., alpha=, beta=)`` computes
``out_k <- alpha E_k + beta out_k`` -- inside the face-mass kernel (``bound.accumulate == "kernel"``) or through ``fe_axpby``
behind the ordinary launch (``"axpby"``).  Exact on integer data, the two routes bitwise alike for powers of two and within a
derived bound otherwise, ``beta == 0`` blind to what the output held, planted NaNs where they belong, guard bands through the
C ABI, refusals before anything runs, reproducible across runs, threads and a graph replay, and faster than the add passes
a caller had to run before."""

import threading

import numpy as np
import pytest

import autograd_cases as C
import feinsum_amd as f
from feinsum_amd import _hip
from feinsum_amd.diagnostics import InvalidParameterError
from feinsum_amd.measure import _bind
from oracle import einsum_ref as ref

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

BITS = 4          # |operands| and |old outputs| < 2^4
AB = [(1.0, 1.0), (-1.0, 1.0), (2.0, -0.5), (0.5, 0.0), (0.0, 1.0), (0.0, 0.0)]
FIELDS = [2, 3, 4, 5, 9]
# one layout at p = 1..3 (a different one each), all eight at p = 4
EXACT_CASES = [(1, "fe", "ifj"), (2, "ef", "fji"), (3, "fe", "jfi")] + [(4, jl, rl) for jl, rl in C.FM_LAYOUTS]
FUSED = {"accumulate": "kernel"}
FALLBACK = {"accumulate": "axpby"}


# This module runs first in the suite and allocates through torch only (under 1 GB).  It does NOT hand torch's cached blocks back to
# the driver when it ends: freed, they leave a hole at the start of the device memory in which the split allocator of the later
# modules begins its search for classes of physical memory (seen: a third class of a few hundred MiB that never comes back, and
# 0.3 s more of the allocator's 4 s search budget, of which tests/test_gpu_parity.py alone takes 2.7 s); kept, the later modules
# reuse the blocks and the driver's free memory is what it is when tests/test_gpu_autograd.py starts the suite.


@pytest.fixture(scope="module")
def own_streams():
    """Streams from torch's high-priority pool (handed out round robin per priority): the streams the other modules take from
    the default pool stay the ones they were without this module."""
    yield [torch.cuda.Stream(priority=-1) for _ in range(3)]
    torch.cuda.synchronize()


def _dev(host):
    return {n: torch.from_numpy(np.ascontiguousarray(v)).cuda() for n, v in host.items()}


_GEOMETRY = {}


def geometry(p):
    """``(TEL, E2)`` of order p, read from what the launcher reports: the wave tile TEL = E / tiles, and E2 = an element count
    at which some wave of the full grid walks a second tile (waves x TEL + TEL + 5), checked against the launch at E2."""
    if p not in _GEOMETRY:
        _, Np, nf, Nfp = C.TETS[p]
        e = C.face_mass(Np, nf, Nfp, 2)
        E = 4096
        dev = _dev(C.random_inputs(e, E, integer=True))
        outs = {n: torch.zeros(E, Np, dtype=torch.float64, device="cuda") for n in e.output_names}
        f.evaluate(e, 0, dev, out_dict=outs, alpha=1.0, beta=1.0, wait=True)
        tel = E // _hip.last_launch_info()["tiles"]
        assert tel % 16 == 0 and E % tel == 0
        waves = 2 * torch.cuda.get_device_properties(0).multi_processor_count * 4      # two blocks of four waves per CU
        E2 = waves * tel + tel + 5
        assert E2 <= 2 * 10 ** 5
        dev = _dev(C.random_inputs(e, E2, integer=True))
        outs = {n: torch.zeros(E2, Np, dtype=torch.float64, device="cuda") for n in e.output_names}
        f.evaluate(e, 0, dev, out_dict=outs, alpha=1.0, beta=1.0, wait=True)
        info = _hip.last_launch_info()
        assert info["tiles"] == E2 // tel > info["blocks"] * info["waves_per_block"], info   # some wave walks a second tile
        _GEOMETRY[p] = (tel, E2)
    return _GEOMETRY[p]


def sizes(p):
    tel, _ = geometry(p)
    return sorted({0, 1, 15, 16, 17, tel - 1, tel, tel + 1, 2 * tel + 3, 4099})


def _ints(rng, shape):
    top = (1 << BITS) - 1
    return rng.integers(-top, top + 1, size=shape).astype(np.float64)


def _int_problem(p, jl, rl, b, E, seed):
    """Integer operands, old outputs and the int64 face-mass sums of b fields."""
    _, Np, nf, Nfp = C.TETS[p]
    e = C.face_mass(Np, nf, Nfp, b, jl, rl)
    rng = np.random.default_rng(seed)
    host = {n: _ints(rng, C.concrete(e.arg_to_shape[n], E)) for n in sorted(e.all_args)}
    old = [_ints(rng, (E, Np)) for _ in range(b)]
    J = host["J"].astype(np.int64) if jl == "ef" else host["J"].astype(np.int64).T                      # [e][f]
    R = host["R"].astype(np.int64).transpose({"fij": (0, 1, 2), "ifj": (1, 0, 2), "fji": (0, 2, 1), "jfi": (1, 2, 0)}[rl])   # [f][i][j]
    Rm = R.transpose(0, 2, 1).reshape(nf * Nfp, Np)
    sums = []
    for k in range(b):
        jv = (J.T[:, :, None] * host[f"v{k}"].astype(np.int64)).transpose(1, 0, 2).reshape(E, nf * Nfp)
        sums.append(jv @ Rm)
    return e, host, old, sums


def test_bit_budget():
    # 60 products of three 4-bit integers, doubled by alpha = 2, plus an old output: exact in float64, halves included
    assert ref.bits_fit([BITS] * 3, 2 * 4 * 15 * 2 + 1, 52)


def _check_exact(e, dev, old, sums, b, alpha, beta, tag):
    outs = {n: torch.from_numpy(old[k]).cuda() for k, n in enumerate(e.output_names)}
    q, bound, _ = _bind(e, 0, dev, outs, None, alpha=alpha, beta=beta)
    assert bound.accumulate == "kernel", tag
    bound.launch(q.stream_ptr)
    for k, n in enumerate(e.output_names):
        want = alpha * sums[k].astype(np.float64) + beta * old[k]         # exact: small integers and halves
        got = outs[n].cpu().numpy()
        assert ref.bitwise_equal(got, want), (tag, k, int((got != want).sum()))


@pytest.mark.parametrize("p,jl,rl", EXACT_CASES, ids=[f"p{p}_{jl}_{rl}" for p, jl, rl in EXACT_CASES])
def test_exact_on_integer_data(p, jl, rl):
    """Every size, every field count and every (alpha, beta): two of the six pairs per (size, field count), rotating, so that
    every pair meets every size and every field count.  The size at which a wave walks a second tile runs with b = 4."""
    for iE, E in enumerate(sizes(p)):
        e9, host, old, sums = _int_problem(p, jl, rl, max(FIELDS), E, 1000 * p + E)
        dev = _dev(host)
        for ib, b in enumerate(FIELDS):
            _, Np, nf, Nfp = C.TETS[p]
            e = C.face_mass(Np, nf, Nfp, b, jl, rl)       # the first b fields of the nine
            for t in (0, 3):
                alpha, beta = AB[(iE + ib + t) % len(AB)]
                _check_exact(e, dev, old, sums, b, alpha, beta, (p, jl, rl, E, b, alpha, beta))
    E2 = geometry(p)[1]
    e, host, old, sums = _int_problem(p, jl, rl, 4, E2, 7)
    dev = _dev(host)
    for alpha, beta in ((1.0, 1.0), (2.0, -0.5)):
        _check_exact(e, dev, old, sums, 4, alpha, beta, (p, jl, rl, E2, alpha, beta))


def _signed_problem(p, b, E, seed, jl="ef", rl="fij"):
    _, Np, nf, Nfp = C.TETS[p]
    e = C.face_mass(Np, nf, Nfp, b, jl, rl)
    host = C.random_inputs(e, E, seed=seed)
    rng = np.random.default_rng(seed + 1)
    old = [rng.standard_normal((E, Np)) for _ in range(b)]
    return e, host, old


def _accumulate(e, dev, old, alpha, beta, transform, expect):
    outs = {n: torch.from_numpy(old[k]).cuda() for k, n in enumerate(e.output_names)}
    q, bound, _ = _bind(e, 0, dev, outs, transform, alpha=alpha, beta=beta)
    assert bound.accumulate == expect
    bound.launch(q.stream_ptr)
    q.finish()
    return [outs[n] for n in e.output_names]


@pytest.mark.parametrize("p,b,jl,rl", [(1, 2, "ef", "fij"), (2, 3, "fe", "ifj"), (3, 4, "ef", "jfi"), (4, 4, "fe", "fji"), (4, 9, "ef", "fij")])
def test_fused_and_fallback_agree(p, b, jl, rl):
    tel, _ = geometry(p)
    for E in (tel + 1, 4099):
        e, host, old = _signed_problem(p, b, E, 11 * p + b, jl, rl)
        dev = _dev(host)
        plain = f.evaluate(e, 0, dev, wait=True)
        for alpha, beta in ((2.0, -0.5), (-1.0, 1.0), (0.25, 4.0)):       # signed powers of two: both products exact
            fused = _accumulate(e, dev, old, alpha, beta, FUSED, "kernel")
            fallback = _accumulate(e, dev, old, alpha, beta, FALLBACK, "axpby")
            for k, n in enumerate(e.output_names):
                two_pass = alpha * plain[n] + beta * torch.from_numpy(old[k]).cuda()
                assert torch.equal(fused[k], fallback[k]) and torch.equal(fused[k], two_pass), (E, alpha, beta, k)
        # general factors: within gamma(K + 2, u) (|alpha| absref + |beta| |old|) of the long-double value, K = the nf Nfp
        # summed products -- derived: the kernel's sum is within gamma(K + 2) absref (test_gpu_dg_exact), the combine
        # multiplies old by beta (one rounding) and rounds fma(alpha, sum, .) once, which gamma's slack covers
        alpha, beta = 0.3, -1.7
        fused = _accumulate(e, dev, old, alpha, beta, FUSED, "kernel")
        sub = e.get_subscripts().replace(" ", "")
        K = C.TETS[p][2] * C.TETS[p][3]
        for k, row in enumerate(e.args):
            r, absr = ref.bounded_reference(sub, [host[a.name] for a in row])
            o = old[k].astype(np.longdouble)
            want = np.longdouble(alpha) * r + np.longdouble(beta) * o
            bound = abs(np.longdouble(alpha)) * absr + abs(np.longdouble(beta)) * np.abs(o)
            assert ref.bound_violations(fused[k].cpu().numpy(), want, bound, K + 2, 2.0 ** -53) == 0, (E, k)


@pytest.mark.parametrize("transform,expect", [(FUSED, "kernel"), (FALLBACK, "axpby")], ids=["kernel", "axpby"])
def test_beta_zero_does_not_read_the_output(transform, expect):
    for p, b in ((4, 4), (2, 3)):
        tel, _ = geometry(p)
        for E in (5, tel + 1, 4099):
            e, host, old = _signed_problem(p, b, E, 3)
            dev = _dev(host)
            plain = f.evaluate(e, 0, dev, wait=True)
            got = _accumulate(e, dev, [np.full_like(o, np.nan) for o in old], 0.5, 0.0, transform, expect)
            for k, n in enumerate(e.output_names):
                assert bool(torch.isfinite(got[k]).all()) and torch.equal(got[k], 0.5 * plain[n]), (p, E, k)


@pytest.mark.parametrize("p,b", [(4, 4), (4, 5), (1, 2), (3, 3)])
def test_non_finite_values_stay_where_they_belong(p, b):
    tel, _ = geometry(p)
    _, Np, nf, Nfp = C.TETS[p]
    for E in (7, tel + 1, 2 * tel + 3, 4099):
        e, host, old, sums = _int_problem(p, "ef", "fij", b, E, E)
        rng = np.random.default_rng(E)
        host["R"] = np.where(host["R"] == 0, 1.0, host["R"])      # every output entry of an element depends on every v of it
        host["J"] = np.where(host["J"] == 0, 1.0, host["J"])
        clean = [o.cpu().numpy() for o in _accumulate(e, _dev(host), old, 1.0, 1.0, None, "kernel")]
        for ee in sorted({0, E // 2, E - 1}):
            k = int(rng.integers(b))
            # a NaN in one entry of v_k reaches exactly row ee of out_k
            planted = {n: v.copy() for n, v in host.items()}
            planted[f"v{k}"][int(rng.integers(nf)), ee, int(rng.integers(Nfp))] = np.nan
            got = [o.cpu().numpy() for o in _accumulate(e, _dev(planted), old, 1.0, 1.0, None, "kernel")]
            for m in range(b):
                dep = np.zeros((E, Np), dtype=bool)
                dep[ee] = m == k
                assert ref.nonfinite_violations(got[m], clean[m], dep, np.nan) == 0, (E, ee, k, m)
            # a NaN in the old output stays exactly where it was
            i = int(rng.integers(Np))
            old_nan = [o.copy() for o in old]
            old_nan[k][ee, i] = np.nan
            got = [o.cpu().numpy() for o in _accumulate(e, _dev(host), old_nan, 1.0, 1.0, None, "kernel")]
            for m in range(b):
                dep = np.zeros((E, Np), dtype=bool)
                dep[ee, i] = m == k
                assert ref.nonfinite_violations(got[m], clean[m], dep, np.nan) == 0, (E, ee, k, m)


BAND = 37          # odd: with one more double in front of an output it is 8-byte but not 16-byte aligned


def _banded(arr, lead=BAND):
    buf = torch.full((arr.size + lead + BAND,), float("nan"), dtype=torch.float64, device="cuda")
    buf[lead:lead + arr.size] = torch.from_numpy(np.ascontiguousarray(arr).reshape(-1)).cuda()
    return buf, buf[lead:lead + arr.size], lead


def _bands_untouched(buf, lead):
    return bool(torch.isnan(buf[:lead]).all() and torch.isnan(buf[-BAND:]).all())


@pytest.mark.parametrize("p,b,flags", [(4, 4, 0), (4, 3, 5), (4, 5, 3), (3, 2, 6), (2, 4, 1), (1, 3, 7)])
def test_c_abi_between_guard_bands(p, b, flags):
    """The outputs carved out of sentinel-filled buffers, once 16-byte aligned and once one double further (8-byte aligned
    only): right values inside, nothing written outside."""
    _, Np, nf, Nfp = C.TETS[p]
    jl = "fe" if flags & f.family.FM_J_FE else "ef"
    rl = {0: "fij", f.family.FM_R_IFJ: "ifj", f.family.FM_R_T: "fji", f.family.FM_R_IFJ | f.family.FM_R_T: "jfi"}[flags & 6]
    stream = torch.cuda.current_stream().cuda_stream
    for E in (geometry(p)[0] + 1, 4099):
        e, host, old, sums = _int_problem(p, jl, rl, b, E, E + flags)
        ins = {n: _banded(v, BAND + 1) for n, v in host.items()}
        for lead in (BAND + 1, BAND):
            outs = [_banded(o, lead) for o in old]
            assert all(d.data_ptr() % 16 == (8 if lead == BAND else 0) for _, d, _ in outs)
            _hip.facemass_acc(ins["J"][1].data_ptr(), ins["R"][1].data_ptr(), [ins[f"v{k}"][1].data_ptr() for k in range(b)],
                              [d.data_ptr() for _, d, _ in outs], E, Np, nf, Nfp, 2.0, -0.5, layout_flags=flags, stream=stream)
            torch.cuda.synchronize()
            for k, (buf, d, ld) in enumerate(outs):
                assert _bands_untouched(buf, ld), (E, lead, k)
                want = 2.0 * sums[k].astype(np.float64) - 0.5 * old[k]
                assert ref.bitwise_equal(d.cpu().numpy().reshape(E, Np), want), (E, lead, k)
        assert all(_bands_untouched(buf, ld) for buf, _, ld in ins.values())


def _fallback_cases():
    f32 = "float32"
    return [
        ("grad", C.grad(3, 35), None, 133),
        ("div", C.div(3, 20, "rji"), None, 133),
        ("contraction", f.einsum("ik,kj->ij", f.array("A", (64, 64)), f.array("B", (64, 64))), "contraction", 0),
        ("reduction", f.einsum("ei,ei->i", f.array("A", ("E", 6)), f.array("B", ("E", 6))), "reduction", 5000),
        ("mixed", f.einsum("ij,j->i", f.array("A", ("E", 6), f32), f.array("x", (6,))), None, 133),
        ("facemass_f32", f.batched_einsum("ef,fij,fej->ei", [[f.array("J", ("E", 4), f32), f.array("R", (4, 35, 15), f32),
                                                              f.array(f"v{k}", (4, "E", 15), f32)] for k in range(4)]), None, 133),
        ("facemass_tri", C.face_mass(10, 3, 4, 4), None, 133),
        ("facemass_b1", C.face_mass(35, 4, 15, 1), None, 133),
        ("facemass_tiled", C.face_mass(35, 4, 15, 4), "tiled", 133),
    ]


@pytest.mark.parametrize("name,e,transform,E", _fallback_cases(), ids=[c[0] for c in _fallback_cases()])
def test_every_other_kind_takes_the_fallback(name, e, transform, E):
    host = C.random_inputs(e, E, seed=2)
    dev = _dev(host)
    plain = f.evaluate(e, 0, dev, transform=transform, wait=True)
    old = {n: torch.randn_like(t) for n, t in plain.items()}
    outs = {n: t.clone() for n, t in old.items()}
    q, bound, _ = _bind(e, 0, dev, outs, transform, alpha=2.0, beta=1.0)
    assert bound.accumulate == "axpby"
    bound.launch(q.stream_ptr)
    q.finish()
    for n in e.output_names:
        assert outs[n].dtype == plain[n].dtype
        assert torch.equal(outs[n], 2.0 * plain[n] + old[n]), name      # 2 E is exact: one rounding, as fma(2, E, old)


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_axpby_alone(dtype):
    """Powers of two at every size and offset against torch's own two products and one sum (the products are exact, so that
    is fma's single rounding too); general factors in float64 against exact rational arithmetic."""
    from fractions import Fraction

    tdt = getattr(torch, dtype)
    size = torch.empty((), dtype=tdt).element_size()
    stream = torch.cuda.current_stream().cuda_stream
    g = torch.Generator(device="cuda").manual_seed(1)
    for n in (0, 1, 2, 3, 255, 256, 257, 2 ** 16 + 1):
        for off_out, off_x in ((0, 0), (1, 1), (1, 0), (0, 1), (3, 3), (2, 3)):      # elements in front: alike and unlike within 16 bytes
            for alpha, beta in ((2.0, 1.0), (-0.25, 4.0), (0.5, 0.0), (0.3, -1.7)):
                if (alpha, beta) == (0.3, -1.7) and (dtype != "float64" or n > 257):
                    continue
                x = torch.randn(n + 8, dtype=tdt, device="cuda", generator=g)
                out = torch.randn(n + 8, dtype=tdt, device="cuda", generator=g)
                if beta == 0.0:
                    out[off_out:off_out + n] = float("nan")          # not read
                before = out.clone()
                _hip.axpby(out.data_ptr() + off_out * size, x.data_ptr() + off_x * size, n, alpha, beta, dtype == "float64", stream)
                xs, old = x[off_x:off_x + n], before[off_out:off_out + n]
                if beta == 0.0:
                    want = alpha * xs
                elif (alpha, beta) == (0.3, -1.7):      # fl(alpha x + fl(beta old)): Fraction -> float rounds correctly
                    prod = beta * old.cpu().numpy()
                    want = torch.tensor([float(Fraction(alpha) * Fraction(float(a)) + Fraction(float(b)))
                                         for a, b in zip(xs.cpu().numpy(), prod)], dtype=tdt).reshape(n).cuda()
                else:
                    want = alpha * xs + beta * old
                assert torch.equal(out[off_out:off_out + n], want), (n, off_out, off_x, alpha, beta)
                assert torch.equal(out[:off_out], before[:off_out]) and torch.equal(out[off_out + n:], before[off_out + n:])


def test_refusals_launch_nothing():
    e = C.face_mass(35, 4, 15, 4)
    E = 133
    dev = _dev(C.random_inputs(e, E, seed=4))
    planted = {n: torch.full((E, 35), 7.0, dtype=torch.float64, device="cuda") for n in e.output_names}
    with pytest.raises(InvalidParameterError, match="out_dict"):            # beta != 0 and an output missing
        f.evaluate(e, 0, dev, out_dict={n: planted[n] for n in e.output_names[:3]}, alpha=1.0, beta=1.0)
    with pytest.raises(InvalidParameterError, match="out_dict"):
        f.evaluate(C.grad(3, 35), 0, _dev(C.random_inputs(C.grad(3, 35), E)), beta=0.5)
    for bad in (float("nan"), float("inf")):
        with pytest.raises(InvalidParameterError, match="finite"):
            f.evaluate(e, 0, dev, out_dict=planted, alpha=bad, beta=1.0)
        with pytest.raises(InvalidParameterError, match="finite"):
            f.evaluate(e, 0, dev, out_dict=planted, alpha=1.0, beta=bad, transform=FALLBACK)
    with pytest.raises(InvalidParameterError, match="shares memory"):       # an output that is an input
        f.evaluate(e, 0, dev, out_dict={**planted, "_fe_out": dev["v0"].reshape(-1)[:E * 35].reshape(E, 35)}, alpha=1.0, beta=1.0)
    with pytest.raises(InvalidParameterError, match="shares memory"):       # two outputs sharing bytes
        f.evaluate(e, 0, dev, out_dict={**planted, "_fe_out_1": planted["_fe_out"]}, alpha=2.0, beta=0.0)
    with pytest.raises(NotImplementedError, match="do not accumulate"):
        f.bind_operator([(e, dev)], 0, out_dicts=[planted], beta=1.0)
    torch.cuda.synchronize()
    assert all(bool((t == 7.0).all()) for t in planted.values())
    # without beta the missing outputs are allocated as ever
    outs = f.evaluate(e, 0, dev, alpha=0.5, wait=True)
    plain = f.evaluate(e, 0, dev, wait=True)
    assert all(torch.equal(outs[n], 0.5 * plain[n]) for n in e.output_names)


@pytest.mark.parametrize("transform,expect", [(None, "kernel"), (FALLBACK, "axpby")], ids=["kernel", "axpby"])
def test_reproducible_across_runs_threads_and_a_graph_replay(transform, expect, own_streams):
    e, host, old = _signed_problem(4, 4, 4099, 5)
    dev = _dev(host)
    alpha, beta = 0.3, -1.7

    def run(q, outs):
        _, bound, _ = _bind(e, q, dev, outs, transform, alpha=alpha, beta=beta)
        assert bound.accumulate == expect
        bound.launch(f.measure._as_queue(q).stream_ptr)
        return bound

    def fresh():
        return {n: torch.from_numpy(old[k]).cuda() for k, n in enumerate(e.output_names)}

    first = fresh()
    run(0, first)
    again = fresh()
    run(0, again)
    torch.cuda.synchronize()
    assert all(torch.equal(first[n], again[n]) for n in e.output_names)
    results = [fresh(), fresh()]
    torch.cuda.synchronize()

    def work(k):
        q = f.DeviceQueue(0, own_streams[k])
        run(q, results[k])
        q.finish()

    threads = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    [th.start() for th in threads]
    [th.join() for th in threads]
    assert all(torch.equal(first[n], results[k][n]) for n in e.output_names for k in range(2))
    # a captured and replayed launch: the fallback's temporaries were allocated when the launch was bound
    outs = fresh()
    q = f.DeviceQueue(0, own_streams[2])
    own_streams[2].wait_stream(torch.cuda.current_stream())
    _, bound, _ = _bind(e, q, dev, outs, transform, alpha=alpha, beta=beta)
    bound.launch(q.stream_ptr)                  # (kernels configured before the capture)
    q.finish()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=own_streams[2]):
        bound.launch(int(torch.cuda.current_stream().cuda_stream))
    for k, n in enumerate(e.output_names):
        outs[n].copy_(torch.from_numpy(old[k]))
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(first[n], outs[n]) for n in e.output_names)


# Measured on MI355X with tools/bench_accumulate.py (profiles/accumulate/bench_accumulate.jsonl): at
# p = 4, b = 4, E = 2 10^5 evaluate + four torch.add(out=) take 230.3 us and the accumulating kernel 148.1 us; the floor is
# halfway between that ratio and 1.0
SPEED_MEASURED = 1.556
SPEED_FLOOR = (1.0 + SPEED_MEASURED) / 2


def test_fused_is_faster_than_evaluate_plus_four_adds():
    E = 2 * 10 ** 5
    e, host, old = _signed_problem(4, 4, E, 9)
    dev = _dev(host)
    rhs = {n: torch.from_numpy(old[k]).cuda() for k, n in enumerate(e.output_names)}
    lift = {n: torch.empty_like(t) for n, t in rhs.items()}
    q, plain, _ = _bind(e, 0, dev, lift, None)
    _, fused, _ = _bind(e, 0, dev, rhs, FUSED, alpha=1.0, beta=1.0)
    assert fused.accumulate == "kernel"

    def before():           # what a caller did without alpha / beta
        plain.launch(q.stream_ptr)
        for n in e.output_names:
            torch.add(rhs[n], lift[n], out=rhs[n])

    def seconds(launch, min_seconds=0.25):
        for _ in range(3):
            launch()
        torch.cuda.synchronize()
        reps, total = 20, 0.0
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

    a = seconds(before)
    c = seconds(lambda: fused.launch(q.stream_ptr))
    print(f"evaluate + 4 adds {a * 1e6:.1f} us, accumulating kernel {c * 1e6:.1f} us, ratio {a / c:.2f} (floor {SPEED_FLOOR:.2f})")
    assert a / c > SPEED_FLOOR, (a, c)
