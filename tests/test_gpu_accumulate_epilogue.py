"""The accumulating grad and div kernels on the device: under ``transform={"accumulate": "epilogue"}``
``evaluate(..., alpha=, beta=)`` computes ``out <- alpha E + beta out`` inside the matrix-core kernel, reading the old output
where it stores the new one (``bound.accumulate == "epilogue"``).  Exact on integer data at every order, size, factor pair and
operator layout; bitwise the ``"axpby"`` route (the combine is the same code) and within a derived bound of the long-double
value; ``beta == 0`` blind to what the output held; planted NaNs where they belong; guard bands through the C ABI; refusals
before anything runs; reproducible across runs, a side stream and a graph replay; faster than the route the same call takes
without the transform."""

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
AB = [(1.0, 1.0), (-1.0, 1.0), (2.0, -0.5), (0.5, 0.0), (0.0, 1.0), (0.0, 0.0)]      # the pairs of tests/test_gpu_accumulate.py
EPILOGUE = {"accumulate": "epilogue"}
FALLBACK = {"accumulate": "axpby"}
FAMILIES = {"grad": C.grad, "div": C.div}
CASES = [(fam, p) for fam in FAMILIES for p in (1, 2, 3, 4)]
IDS = [f"{fam}_p{p}" for fam, p in CASES]
SUBSCRIPTS = {"grad": "xre,rij,ej->xei", "div": "xre,rij,xej->ei"}


def _einsum(fam, p, d="rij"):
    return FAMILIES[fam](3, C.TETS[p][1], d)


def _dev(host):
    return {n: torch.from_numpy(np.ascontiguousarray(v)).cuda() for n, v in host.items()}


def _ints(rng, shape):
    top = (1 << BITS) - 1
    return rng.integers(-top, top + 1, size=shape).astype(np.float64)


def _out_shape(fam, p, E):
    Np = C.TETS[p][1]
    return (3, E, Np) if fam == "grad" else (E, Np)


def _launch(e, dev, old, alpha, beta, transform=EPILOGUE, expect="epilogue", q=0):
    """One accumulating evaluation onto a copy of *old*; returns the output (a device tensor)."""
    out = torch.from_numpy(old).cuda()
    q, bound, _ = _bind(e, q, dev, {e.output_names[0]: out}, transform, alpha=alpha, beta=beta)
    assert bound.accumulate == expect
    bound.launch(q.stream_ptr)
    q.finish()
    return out


_GEOMETRY = {}


def geometry(fam, p):
    """``(TEL, E2)``: the wave tile, TEL = E / tiles as the launcher reports them, and E2 = waves x TEL + TEL + 5, an element count
    at which some wave of the full grid walks a second tile -- asserted from the launch at E2."""
    if (fam, p) not in _GEOMETRY:
        e = _einsum(fam, p)
        found = []
        for E in (4800, None):             # 4800 = 2^6 3 5^2: a multiple of every wave tile (16, 32, 48, 80 elements)
            if E is None:
                waves = 2 * torch.cuda.get_device_properties(0).multi_processor_count * 4   # two blocks of four waves per CU
                E = waves * found[0] + found[0] + 5
                assert E <= 2 * 10 ** 5
            dev = _dev(C.random_inputs(e, E, integer=True))
            _launch(e, dev, np.zeros(_out_shape(fam, p, E)), 1.0, 1.0)
            info = _hip.last_launch_info()
            if not found:
                tel = E // info["tiles"]
                assert tel % 16 == 0 and E % tel == 0 and not info["dynamic_walk"], info
                found.append(tel)
            else:
                assert info["tiles"] == E // found[0] > info["blocks"] * info["waves_per_block"], info   # a second tile
                assert not (info["dynamic_walk"] or info["write_through_stores"] or info["quarter_tail"] or info["staggered_start"]), info
                found.append(E)
        _GEOMETRY[fam, p] = tuple(found)
    return _GEOMETRY[fam, p]


def sizes(fam, p):
    tel, _ = geometry(fam, p)
    return sorted({0, 1, 15, 16, 17, tel - 1, tel, tel + 1, 2 * tel + 3, 4099})


def _int_problem(fam, p, d, E, seed):
    """Integer operands, an integer old output and the int64 sums."""
    e = _einsum(fam, p, d)
    rng = np.random.default_rng(seed)
    host = {n: _ints(rng, C.concrete(e.arg_to_shape[n], E)) for n in sorted(e.all_args)}
    old = _ints(rng, _out_shape(fam, p, E))
    ops = [host[a.name].astype(np.int64) for a in e.args[0]]
    sums = np.einsum(e.get_subscripts().replace(" ", ""), *ops)
    return e, host, old, sums


def test_bit_budget():
    # div sums 9 Np = 315 products of three 4-bit integers (grad: 3 Np), doubled by alpha = 2, plus an old output: exact in
    # float64, halves included
    assert ref.bits_fit([BITS] * 3, 2 * 9 * 35 + 1, 52)


@pytest.mark.parametrize("fam,p", CASES, ids=IDS)
def test_exact_on_integer_data(fam, p):
    """Every size with two of the six (alpha, beta) pairs, rotating, and the operator layouts alternating with them, so that
    every pair and both layouts meet sizes below one tile, a whole number of tiles and tiles with a remainder; the size at which
    a wave walks a second tile runs both layouts."""
    for iE, E in enumerate(sizes(fam, p)):
        for t in (0, 3):
            d = ("rij", "rji")[(iE + t // 3) % 2]
            e, host, old, sums = _int_problem(fam, p, d, E, 1000 * p + E + t)
            alpha, beta = AB[(iE + t) % len(AB)]
            got = _launch(e, _dev(host), old, alpha, beta).cpu().numpy()
            want = alpha * sums.astype(np.float64) + beta * old           # exact: small integers and halves
            assert ref.bitwise_equal(got, want), (fam, p, d, E, alpha, beta, int((got != want).sum()))
    E2 = geometry(fam, p)[1]
    for d, (alpha, beta) in (("rij", (1.0, 1.0)), ("rji", (2.0, -0.5))):
        e, host, old, sums = _int_problem(fam, p, d, E2, 7)
        got = _launch(e, _dev(host), old, alpha, beta).cpu().numpy()
        info = _hip.last_launch_info()
        assert info["tiles"] > info["blocks"] * info["waves_per_block"], info
        want = alpha * sums.astype(np.float64) + beta * old
        assert ref.bitwise_equal(got, want), (fam, p, d, E2, alpha, beta, int((got != want).sum()))


def _signed_problem(fam, p, E, seed, d="rij"):
    e = _einsum(fam, p, d)
    host = C.random_inputs(e, E, seed=seed)
    old = np.random.default_rng(seed + 1).standard_normal(_out_shape(fam, p, E))
    return e, host, old


@pytest.mark.parametrize("fam,p", CASES, ids=IDS)
def test_epilogue_and_fallback_agree(fam, p):
    tel, _ = geometry(fam, p)
    for E, d in ((tel + 1, "rji"), (4099, "rij")):
        e, host, old = _signed_problem(fam, p, E, 11 * p + len(fam), d)
        dev = _dev(host)
        n = e.output_names[0]
        plain = f.evaluate(e, 0, dev, wait=True)[n]
        for alpha, beta in ((2.0, -0.5), (-1.0, 1.0), (0.25, 4.0)):       # signed powers of two: both products exact
            epi = _launch(e, dev, old, alpha, beta)
            fallback = _launch(e, dev, old, alpha, beta, FALLBACK, "axpby")
            two_pass = alpha * plain + beta * torch.from_numpy(old).cuda()
            assert torch.equal(epi, fallback) and torch.equal(epi, two_pass), (E, alpha, beta)
        # general factors: bitwise the fallback (the combine is the same code on the same sum) ...
        alpha, beta = 0.3, -1.7
        epi = _launch(e, dev, old, alpha, beta)
        assert torch.equal(epi, _launch(e, dev, old, alpha, beta, FALLBACK, "axpby")), E
        # ... and within gamma(K + 2, u) (|alpha| absref + |beta| |old|) of the long-double value, K = 3 Np summed products --
        # derived as in tests/test_gpu_accumulate.py: the kernel's sum is within gamma(K + 2) absref (test_gpu_dg_exact), the
        # combine multiplies old by beta (one rounding) and rounds fma(alpha, sum, .) once, which gamma's slack covers
        K = 3 * C.TETS[p][1]
        r, absr = ref.bounded_reference(SUBSCRIPTS[fam].replace("rij", d), [host[a.name] for a in e.args[0]])
        o = old.astype(np.longdouble)
        want = np.longdouble(alpha) * r + np.longdouble(beta) * o
        bound = abs(np.longdouble(alpha)) * absr + abs(np.longdouble(beta)) * np.abs(o)
        assert ref.bound_violations(epi.cpu().numpy(), want, bound, K + 2, 2.0 ** -53) == 0, E


@pytest.mark.parametrize("fam,p", [("grad", 4), ("div", 4), ("grad", 2), ("div", 1)])
def test_beta_zero_does_not_read_the_output(fam, p):
    tel, _ = geometry(fam, p)
    for E in (5, tel + 1, 4099):
        e, host, old = _signed_problem(fam, p, E, 3)
        dev = _dev(host)
        plain = f.evaluate(e, 0, dev, wait=True)[e.output_names[0]]
        poison = np.full_like(old, np.nan)
        poison.reshape(-1)[1::2] = np.inf
        poison.reshape(-1)[2::4] = -np.inf
        got = _launch(e, dev, poison, 0.5, 0.0)
        assert bool(torch.isfinite(got).all()) and torch.equal(got, 0.5 * plain), (E,)


@pytest.mark.parametrize("fam,p", CASES, ids=IDS)
def test_non_finite_values_stay_where_they_belong(fam, p):
    """Below one tile (7 elements), in full tiles and in the remainder behind them (element 0, the middle, the last)."""
    tel, _ = geometry(fam, p)
    Np = C.TETS[p][1]
    for E in (7, 2 * tel + 3):
        e, host, old, sums = _int_problem(fam, p, "rij", E, E)
        rng = np.random.default_rng(E)
        host["D"] = np.where(host["D"] == 0, 1.0, host["D"])      # every output entry of an element depends on every u of it
        host["J"] = np.where(host["J"] == 0, 1.0, host["J"])
        clean = _launch(e, _dev(host), old, 1.0, 1.0).cpu().numpy()
        for ee in sorted({0, E // 2, E - 1}):
            # a NaN in one entry of u reaches exactly element ee's rows (of every plane of grad)
            planted = {n: v.copy() for n, v in host.items()}
            at = (ee, int(rng.integers(Np))) if fam == "grad" else (int(rng.integers(3)), ee, int(rng.integers(Np)))
            planted["u"][at] = np.nan
            got = _launch(e, _dev(planted), old, 1.0, 1.0).cpu().numpy()
            dep = np.zeros(old.shape, dtype=bool)
            dep[..., ee, :] = True
            assert ref.nonfinite_violations(got, clean, dep, np.nan) == 0, (E, ee)
            # a NaN in the old output stays exactly where it was
            where = ((int(rng.integers(3)),) if fam == "grad" else ()) + (ee, int(rng.integers(Np)))
            old_nan = old.copy()
            old_nan[where] = np.nan
            got = _launch(e, _dev(host), old_nan, 1.0, 1.0).cpu().numpy()
            dep = np.zeros(old.shape, dtype=bool)
            dep[where] = True
            assert ref.nonfinite_violations(got, clean, dep, np.nan) == 0, (E, ee)


BAND = 64          # doubles of sentinel on either side; a band of 64 + 1 puts the array 8 bytes past a 256-byte boundary


def _banded(arr, lead, fill):
    """*arr* inside a buffer of *fill*: the buffer itself starts on a 256-byte boundary."""
    raw = torch.full((arr.size + lead + BAND + 32,), fill, dtype=torch.float64, device="cuda")
    shift = (-raw.data_ptr() // 8) % 32                       # doubles up to the next 256-byte boundary
    buf = raw[shift:shift + arr.size + lead + BAND]
    assert buf.data_ptr() % 256 == 0
    buf[lead:lead + arr.size] = torch.from_numpy(np.ascontiguousarray(arr).reshape(-1)).cuda()
    return buf, buf[lead:lead + arr.size], lead


def _bands(buf, lead):
    return torch.cat([buf[:lead], buf[-BAND:]]).clone()


@pytest.mark.parametrize("fam,p,flags", [("grad", 4, 0), ("div", 4, 1), ("grad", 3, 1), ("div", 2, 0), ("grad", 1, 0), ("div", 3, 1),
                                         ("grad", 2, 1), ("div", 1, 0)])
def test_c_abi_between_guard_bands(fam, p, flags):
    """The output between sentinel bands and the inputs between NaN bands, compared bitwise with a snapshot afterwards: right
    values inside, nothing written outside.  Once everything on 256-byte boundaries, once with out and u 8 bytes past one and
    an odd E (4099; Np = 35 is odd too), so that grad's plane x = 1 starts 8 bytes off a 16-byte boundary."""
    Np = C.TETS[p][1]
    entry = _hip.grad3d_acc if fam == "grad" else _hip.div3d_acc
    stream = torch.cuda.current_stream().cuda_stream
    SENTINEL = -12345.0
    for E in (geometry(fam, p)[0] + 1, 4099):
        e, host, old, sums = _int_problem(fam, p, "rji" if flags else "rij", E, E + flags)
        want = 2.0 * sums.astype(np.float64) - 0.5 * old
        for lead in (BAND, BAND + 1):
            ins = {n: _banded(v, lead if n == "u" else BAND, float("nan")) for n, v in host.items()}
            obuf, out, _ = _banded(old, lead, SENTINEL)
            assert out.data_ptr() % 256 == (8 if lead == BAND + 1 else 0) == ins["u"][1].data_ptr() % 256
            before = {n: _bands(b, ld) for n, (b, _, ld) in ins.items()}
            inside = {n: v.clone() for n, (_, v, _) in ins.items()}
            entry(ins["J"][1].data_ptr(), ins["D"][1].data_ptr(), ins["u"][1].data_ptr(), out.data_ptr(), E, Np, 2.0, -0.5,
                  op_flags=flags, stream=stream)
            torch.cuda.synchronize()
            assert bool((_bands(obuf, lead) == SENTINEL).all()), (E, lead)
            assert ref.bitwise_equal(out.cpu().numpy().reshape(old.shape), want), (E, lead)
            for n, (b, v, ld) in ins.items():
                assert torch.equal(_bands(b, ld).view(torch.int64), before[n].view(torch.int64)), (E, lead, n)
                assert torch.equal(v, inside[n]), (E, lead, n)


def test_refusals_launch_nothing():
    e = C.grad(3, 35)
    E = 133
    dev = _dev(C.random_inputs(e, E, seed=4))
    planted = torch.full((3, E, 35), 7.0, dtype=torch.float64, device="cuda")
    with pytest.raises(InvalidParameterError, match="out_dict"):            # beta != 0 without the output
        f.evaluate(e, 0, dev, transform=EPILOGUE, alpha=1.0, beta=1.0)
    with pytest.raises(InvalidParameterError, match="shares memory"):       # an output that overlaps an input
        whole = torch.full((3, E, 35), 7.0, dtype=torch.float64, device="cuda")      # u is its first plane
        f.evaluate(e, 0, {**dev, "u": whole[0]}, out_dict={"_fe_out": whole}, transform=EPILOGUE, alpha=1.0, beta=1.0)
    assert bool((whole == 7.0).all())
    div = C.div(3, 35)
    ddev = _dev(C.random_inputs(div, E, seed=5))
    with pytest.raises(InvalidParameterError, match="shares memory"):
        f.evaluate(div, 0, ddev, out_dict={"_fe_out": ddev["u"][1]}, transform=EPILOGUE, alpha=2.0, beta=1.0)
    # "epilogue" where it does not exist: face-mass, p = 5, triangles, a forced tiled variant
    fm = C.face_mass(35, 4, 15, 4)
    fdev = _dev(C.random_inputs(fm, E, seed=6))
    fouts = {n: torch.full((E, 35), 7.0, dtype=torch.float64, device="cuda") for n in fm.output_names}
    with pytest.raises(NotImplementedError, match='"kernel"'):
        f.evaluate(fm, 0, fdev, out_dict=fouts, transform=EPILOGUE, alpha=1.0, beta=1.0)
    with pytest.raises(NotImplementedError, match="no accumulating epilogue"):
        f.evaluate(e, 0, dev, out_dict={"_fe_out": planted}, transform={**EPILOGUE, "variant": "tiled"}, alpha=1.0, beta=1.0)
    tri = C.grad(2, 10)
    tout = torch.full((2, E, 10), 7.0, dtype=torch.float64, device="cuda")
    with pytest.raises(NotImplementedError, match="no accumulating epilogue"):
        f.evaluate(tri, 0, _dev(C.random_inputs(tri, E)), out_dict={"_fe_out": tout}, transform=EPILOGUE, alpha=1.0, beta=1.0)
    with pytest.raises(NotImplementedError, match="do not accumulate"):
        f.bind_operator([(e, dev)], 0, out_dicts=[{"_fe_out": planted}], transform=EPILOGUE)
    torch.cuda.synchronize()
    assert bool((planted == 7.0).all()) and bool((tout == 7.0).all()) and all(bool((t == 7.0).all()) for t in fouts.values())
    # the default route of the same call is what it was, and so is {"accumulate": "kernel"} on grad
    _, bound, _ = _bind(e, 0, dev, {"_fe_out": planted}, None, alpha=2.0, beta=1.0)
    assert bound.accumulate == "axpby"
    with pytest.raises(NotImplementedError, match="no accumulating kernel"):
        _bind(e, 0, dev, {"_fe_out": planted}, {"accumulate": "kernel"}, alpha=2.0, beta=1.0)


@pytest.mark.parametrize("fam", ["grad", "div"])
def test_reproducible_across_runs_a_side_stream_and_a_graph_replay(fam):
    e, host, old = _signed_problem(fam, 4, 4099, 5)
    dev = _dev(host)
    n = e.output_names[0]
    alpha, beta = 0.3, -1.7
    first = _launch(e, dev, old, alpha, beta)
    again = _launch(e, dev, old, alpha, beta)
    assert torch.equal(first, again)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    q = f.DeviceQueue(0, side)
    on_side = _launch(e, dev, old, alpha, beta, q=q)
    assert torch.equal(first, on_side)
    # a captured and replayed bound launch (the kernel was configured by the launches above)
    out = torch.from_numpy(old).cuda()
    torch.cuda.synchronize()
    _, bound, _ = _bind(e, q, dev, {n: out}, EPILOGUE, alpha=alpha, beta=beta)
    assert bound.accumulate == "epilogue"
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        bound.launch(int(torch.cuda.current_stream().cuda_stream))
    out.copy_(torch.from_numpy(old))
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(first, out)


# Measured on MI355X with tools/bench_accumulate.py (profiles/accumulate/bench_accumulate.jsonl) at p = 4,
# E = 2 10^5: the time of the "axpby" route -- what the same call runs without the transform -- over the time of "epilogue".
# The floor is halfway between the measured ratio and 1.0.
# Measured: grad 114.2 us over 71.7 us, div 66.2 us over 48.6 us.
SPEED_MEASURED = {"grad": 1.592, "div": 1.364}


@pytest.mark.parametrize("fam", ["grad", "div"])
def test_epilogue_is_faster_than_the_axpby_route(fam):
    floor = (1.0 + SPEED_MEASURED[fam]) / 2
    E = 2 * 10 ** 5
    e, host, old = _signed_problem(fam, 4, E, 9)
    dev = _dev(host)
    n = e.output_names[0]
    rhs = torch.from_numpy(old).cuda()
    q, fallback, _ = _bind(e, 0, dev, {n: rhs}, FALLBACK, alpha=0.5, beta=1.0)
    _, epilogue, _ = _bind(e, 0, dev, {n: rhs}, EPILOGUE, alpha=0.5, beta=1.0)
    assert fallback.accumulate == "axpby" and epilogue.accumulate == "epilogue"

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

    a = seconds(lambda: fallback.launch(q.stream_ptr))
    c = seconds(lambda: epilogue.launch(q.stream_ptr))
    print(f"{fam}: axpby route {a * 1e6:.1f} us, epilogue {c * 1e6:.1f} us, ratio {a / c:.2f} (floor {floor:.2f})")
    assert a / c > floor, (a, c)
