"""Arrays the library allocates on the caller's behalf -- outputs of ``evaluate`` / ``bind_operator``, prepared-operator
buffers, the zero fills of ``generate_out_arrays`` -- on a ``DeviceQueue`` whose stream is NOT the thread's current
stream ("whose stream an array belongs to").  Such an array belongs to the queue's stream: it is
allocated and filled there, and when its last tensor goes, the next owner -- whatever stream it is on -- is ordered
behind the work of that stream.  A violation is silent, depends on timing and mixes two correct results, so every
scenario here HOLDS a stream busy with filler work (``stream_lifetime_cases.hold``; ten times the host time of a serial
run of the scenario, at least 50 ms) and asserts that the filler is still unfinished where the hazard would occur.

Every expected value is the int64 einsum of oracle/einsum_ref.py on exact data (stream_lifetime_cases.py).

(a) ``evaluate`` returns while the held stream is busy (no host synchronisation anywhere), results exact
(b) an output dropped while its stream is busy, a new array of that size from the same source on the current stream
(c) the same with the next owner another queue's ``evaluate``
(d) prepared-operator buffers outlive the launches that read them
(e) the zero fill of ``generate_out_arrays`` is ordered with the launch
(f) two host threads, forty evaluations each, nothing waited for (depends on timing; (b)-(e) are deterministic)
(g) controls: the queue's stream current, inside ``torch.cuda.stream``, an integer queue; recycling as before

One report line per scenario and path (``-s`` shows them): allocator, same-address / other-address outcome, hold."""

import gc
import threading

import pytest

import stream_lifetime_cases as C
from stream_lifetime_cases import PATH_NAMES, PREPARED, SINGLE

import feinsum_amd as f
from feinsum_amd import _hip, placement

pytestmark = pytest.mark.gpu

DROPPABLE = tuple(n for n in PATH_NAMES if n != "differentiable")


@pytest.fixture(scope="module")
def env():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    torch.cuda.set_device(0)

    class Env:
        pass

    e = Env()
    e.torch = torch
    # three streams of the test's own: the thread's CURRENT stream inside every scenario, and two queue streams
    e.cur, e.a, e.b = torch.cuda.Stream(), torch.cuda.Stream(), torch.cuda.Stream()
    e.qa, e.qb = f.DeviceQueue(0, stream=e.a), f.DeviceQueue(0, stream=e.b)
    yield e
    C.clear()
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _report(scenario, path, alloc, same, other, seconds):
    print(f"\n[stream-lifetime] ({scenario}) {path}: allocator={alloc} same-address={same} other-address={other}"
          f" hold={seconds * 1e3:.0f} ms", flush=True)


def _alloc_of(tensors):
    kinds = sorted({"split" if placement.is_split(t) else "torch" for t in tensors})
    return "+".join(kinds)


def _clones(env, stream, tensors):
    with env.torch.cuda.stream(stream):
        return [t.clone() for t in tensors]


# --------------------------------------------------------------------------
# (a)
# --------------------------------------------------------------------------

@pytest.mark.timeout(600)
@pytest.mark.parametrize("name", PATH_NAMES)
def test_a_evaluate_stays_asynchronous(env, name):
    """With stream A held busy, the call returns before the filler finishes (a fix by host synchronisation would not),
    and the results -- cloned on A -- are bitwise the oracle's."""
    torch, path = env.torch, C.get_path(env.torch, name)

    def body(seconds):
        with torch.cuda.stream(env.cur):
            ev = C.hold(torch, env.a, seconds) if seconds else None
            outs = path.run(env.qa, 0)
            if ev is not None:
                C.still_busy(ev, f"{name} returned: it waited for its stream on the host")
            alloc = _alloc_of(outs)
            keep = _clones(env, env.a, outs)
            del outs
        torch.cuda.synchronize()
        return C.mismatches(keep, path.refs(0)), alloc

    (bad, alloc), seconds = C.run_held(torch, body)
    _report("a", name, alloc, "-", "-", seconds)
    assert not bad, (name, bad)


# --------------------------------------------------------------------------
# (b)
# --------------------------------------------------------------------------

def _same_source(torch, t):
    """A new uninitialised array of *t*'s byte size from the source *t* came from."""
    if placement.is_split(t):
        return placement.empty(tuple(t.shape), t.dtype, t.device)
    return torch.empty(tuple(t.shape), dtype=t.dtype, device=t.device)


@pytest.mark.timeout(600)
@pytest.mark.parametrize("name", DROPPABLE)
def test_b_released_output_new_owner_on_another_stream(env, name):
    """Stream A busy; the output of ``evaluate(P, qA, ...)`` is cloned on A and dropped; the current stream takes an
    array of the same size from the same source and fills it with a sentinel.  The clone is the oracle's result, and a
    new array at the old address holds the sentinel everywhere: the launch on A did not write behind its new owner."""
    torch, path = env.torch, C.get_path(env.torch, name)

    def body(seconds):
        with torch.cuda.stream(env.cur):
            ev = C.hold(torch, env.a, seconds) if seconds else None
            outs = path.run(env.qa, 0)
            alloc = _alloc_of(outs)
            keep = _clones(env, env.a, outs)
            old = [t.data_ptr() for t in outs]
            news = []
            while outs:                       # drop every output, then take its successor
                t = outs.pop()
                shape, dtype, split = tuple(t.shape), t.dtype, placement.is_split(t)
                del t
                new = placement.empty(shape, dtype, "cuda:0") if split else torch.empty(shape, dtype=dtype, device="cuda:0")
                assert placement.is_split(new) == split, "the new array is not from the same source"
                news.append(new.fill_(C.SENTINEL))
            if ev is not None:
                C.still_busy(ev, "the new owner filled its array")
        torch.cuda.synchronize()
        bad = C.mismatches(keep, path.refs(0))
        same = [n for n in news if n.data_ptr() in old]
        for n in same:
            wrong = int((n != C.SENTINEL).sum())
            if wrong:
                bad.append(f"new array at the released address {n.data_ptr():#x}: {wrong} of {n.numel()} entries are not the "
                           "sentinel -- the launch on the held stream wrote into it behind its new owner")
        return bad, alloc, len(same), len(news) - len(same)

    (bad, alloc, same, other), seconds = C.run_held(torch, body)
    _report("b", name, alloc, same, other, seconds)
    assert not bad, (name, bad)


# --------------------------------------------------------------------------
# (c)
# --------------------------------------------------------------------------

@pytest.mark.timeout(600)
@pytest.mark.parametrize("name", DROPPABLE)
def test_c_two_queues(env, name):
    """``evaluate(P, qA, in1)`` cloned on A and dropped, then ``evaluate(P, qB, in2)`` at once, A held busy: the clone
    is the oracle's result of in1, and the second call's own output that of in2 after everything has finished."""
    torch, path = env.torch, C.get_path(env.torch, name)

    def body(seconds):
        with torch.cuda.stream(env.cur):
            ev = C.hold(torch, env.a, seconds) if seconds else None
            outs1 = path.run(env.qa, 0)
            alloc = _alloc_of(outs1)
            keep1 = _clones(env, env.a, outs1)
            old = [t.data_ptr() for t in outs1]
            del outs1
            outs2 = path.run(env.qb, 1)
            if ev is not None:
                C.still_busy(ev, "the second queue's evaluate returned")
        torch.cuda.synchronize()
        bad = ["first: " + m for m in C.mismatches(keep1, path.refs(0))] + \
              ["second: " + m for m in C.mismatches(outs2, path.refs(1))]
        same = sum(t.data_ptr() in old for t in outs2)
        return bad, alloc, same, len(outs2) - same

    (bad, alloc, same, other), seconds = C.run_held(torch, body)
    _report("c", name, alloc, same, other, seconds)
    assert not bad, (name, bad)


# --------------------------------------------------------------------------
# (d)
# --------------------------------------------------------------------------

def _zeroed_prepared_sized(torch, n=8):
    """*n* zeroed byte arrays of a prepared-operator buffer's size on the current stream.  (fe_prepare_operator writes
    operator VALUES in fragment order into that buffer -- grad_prepare_kernel / div_prepare_kernel /
    facemass_prepare_kernel store doubles of D / R and nothing else, no index or offset -- so a launch that reads zeros
    instead computes zeros; it cannot address anything with them.  Zeros only: never another bit pattern.)"""
    return [torch.zeros(_hip.PREPARED_OPERATOR_BYTES, dtype=torch.uint8, device="cuda:0") for _ in range(n)]


@pytest.mark.timeout(600)
@pytest.mark.parametrize("name", PREPARED)
def test_d_prepared_buffer_outlives_evaluate(env, name):
    """``evaluate(..., transform={"prepared": True})`` with A busy: the bound launch, and with it the prepared buffer,
    dies when ``evaluate`` returns; arrays of the buffer's size zeroed on the current stream must not be that buffer
    while the launch on A has not read it.  (With a buffer taken from the current stream's pool this form still computes
    the right result whenever the zero fills run at once: ``fe_prepare_operator``'s kernels and the launch are BOTH
    enqueued on A behind the filler, so the zeros land before the prepare kernel rewrites the buffer.  The harmful
    order -- zeros between the two -- is what the ``bind_operator`` form below arranges, by preparing before A is held.)"""
    torch, path = env.torch, C.get_path(env.torch, name)

    def body(seconds):
        with torch.cuda.stream(env.cur):
            ev = C.hold(torch, env.a, seconds) if seconds else None
            outs = path.run(env.qa, 0)
            zeros = _zeroed_prepared_sized(torch)
            if ev is not None:
                C.still_busy(ev, "the zeroed arrays were taken")
        torch.cuda.synchronize()
        del zeros
        return C.mismatches(outs, path.refs(0)), _alloc_of(outs)

    (bad, alloc), seconds = C.run_held(torch, body)
    _report("d/evaluate", name, alloc, "-", "-", seconds)
    assert not bad, (name, bad)


@pytest.mark.timeout(600)
@pytest.mark.parametrize("name", PREPARED)
def test_d_prepared_buffer_outlives_a_deleted_operator(env, name):
    """The same through ``bind_operator(..., prepare=True)``: the operator is launched with A busy and deleted."""
    torch, path = env.torch, C.get_path(env.torch, name)

    def body(seconds):
        with torch.cuda.stream(env.cur):
            op = f.bind_operator([(path.expr, path.args(0))], env.qa, prepare=True)
            assert any(b._prepared for b in op._stages), "nothing was prepared"
            ev = C.hold(torch, env.a, seconds) if seconds else None
            with torch.cuda.device(0):
                op.launch()
            outs = [op.outputs[0][n] for n in path.expr.output_names]
            del op
            gc.collect()
            zeros = _zeroed_prepared_sized(torch)
            if ev is not None:
                C.still_busy(ev, "the zeroed arrays were taken")
        torch.cuda.synchronize()
        del zeros
        return C.mismatches(outs, path.refs(0)), _alloc_of(outs)

    (bad, alloc), seconds = C.run_held(torch, body)
    _report("d/bind_operator", name, alloc, "-", "-", seconds)
    assert not bad, (name, bad)


# --------------------------------------------------------------------------
# (e)
# --------------------------------------------------------------------------

@pytest.mark.timeout(600)
@pytest.mark.parametrize("split", [True, False])
@pytest.mark.parametrize("name", SINGLE)
def test_e_zero_fill_is_ordered_with_the_launch(env, name, split):
    """The CURRENT stream busy: ``generate_out_arrays(qA, ...)`` then ``evaluate(..., qA, out_dict=outs)``.  The zero
    fill belongs to the queue's stream, so the result is the oracle's -- not zeros written after the launch."""
    torch, path = env.torch, C.get_path(env.torch, name)

    def body(seconds):
        with torch.cuda.stream(env.cur):
            ev = C.hold(torch, env.cur, seconds) if seconds else None
            outs = f.generate_out_arrays(env.qa, path.expr, path.E, split=split)
            f.evaluate(path.expr, env.qa, path.args(0), out_dict=outs, transform=path.transform)
            if ev is not None:
                C.still_busy(ev, "evaluate returned")
        torch.cuda.synchronize()
        got = [outs[n] for n in path.expr.output_names]
        return C.mismatches(got, path.refs(0)), _alloc_of(got)

    (bad, alloc), seconds = C.run_held(torch, body)
    _report(f"e/split={split}", name, alloc, "-", "-", seconds)
    assert not bad, (name, split, bad)


# --------------------------------------------------------------------------
# (f)
# --------------------------------------------------------------------------

@pytest.mark.timeout(900)
def test_f_two_host_threads_forty_evaluations_each(env):
    """Two host threads, a stream and a queue each (neither stream current), forty alternating grad / div / face-mass
    ``evaluate`` calls with library-allocated outputs; each result is cloned on the thread's stream and dropped, nothing
    is waited for; thread t works on data set t.  Every clone is the oracle's."""
    torch = env.torch
    paths = [C.get_path(torch, n) for n in ("grad_split", "prepared_div", "facemass4")]
    for p in paths:                      # data, references and first use outside the threads
        for i in (0, 1):
            p.refs(i)
            p.run(0, i)
    torch.cuda.synchronize()
    results, errors = {}, []
    start = threading.Barrier(2)

    def worker(tid):
        try:
            torch.cuda.set_device(0)
            stream = torch.cuda.Stream()
            q = f.DeviceQueue(0, stream=stream)
            kept = []
            start.wait()
            for k in range(40):
                p = paths[(k + tid) % 3]
                outs = f.evaluate(p.expr, q, p.args(tid))
                outs = [outs[n] for n in p.expr.output_names]
                with torch.cuda.stream(stream):
                    kept.append((p, [t.clone() for t in outs]))
                del outs
            results[tid] = kept
        except Exception as exc:      # noqa: BLE001
            errors.append(exc)
            start.abort()

    threads = [threading.Thread(target=worker, args=(t,)) for t in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    torch.cuda.synchronize()
    assert not errors, errors
    bad = [(tid, k, p.name, m) for tid in (0, 1) for k, (p, got) in enumerate(results[tid]) for m in C.mismatches(got, p.refs(tid))]
    stats = placement.recycle_stats()
    print(f"\n[stream-lifetime] (f) two threads x 40: allocator=split+torch recycled={stats['reused']} mismatching={len(bad)}", flush=True)
    assert not bad, bad[:6]
    assert stats["free_failures"] == 0, stats
    assert _hip.tail_check()["dirty_words"] == 0


# --------------------------------------------------------------------------
# (g)
# --------------------------------------------------------------------------

@pytest.mark.timeout(600)
@pytest.mark.parametrize("name", PATH_NAMES)
def test_g_controls_the_default_path(env, name):
    """The queue's stream current, an integer queue inside ``torch.cuda.stream``, an integer queue on the default
    stream: all three bitwise the oracle's (and so each other's)."""
    torch, path = env.torch, C.get_path(env.torch, name)
    refs = path.refs(0)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        got = path.run(f.DeviceQueue(0, stream=s), 0)
        alloc = _alloc_of(got)
    torch.cuda.synchronize()
    assert not C.mismatches(got, refs), ("queue's stream current", name)
    with torch.cuda.stream(s):
        got = path.run(0, 0)
    torch.cuda.synchronize()
    assert not C.mismatches(got, refs), ("inside torch.cuda.stream", name)
    got = path.run(0, 0)
    torch.cuda.synchronize()
    assert not C.mismatches(got, refs), ("integer queue", name)
    _report("g", name, alloc, "-", "-", 0.0)


@pytest.mark.timeout(600)
@pytest.mark.parametrize("side", [False, True])
def test_g_outputs_are_still_recycled(env, side):
    """What tests/test_placement.py::test_evaluate_without_out_dict_recycles_its_outputs asserts, on the default queue and
    on a side-stream queue: twenty asynchronous calls that each drop the previous output take turns on at most two
    arrays, and the allocator reserves no more address space after the first calls."""
    torch, path = env.torch, C.get_path(env.torch, "grad_split")
    q = env.qa if side else 0
    placement.recycle_trim(0)
    torch.cuda.synchronize()
    s0 = placement.recycle_stats()
    ptrs = set()
    for k in range(20):
        out = path.run(q, 0)[0]
        assert placement.is_split(out)
        ptrs.add(out.data_ptr())
        if k == 4:
            va_early = placement.split_stats(0)["address_space_reserved"]
    torch.cuda.synchronize()
    s1 = placement.recycle_stats()
    assert not C.mismatches([out], path.refs(0))
    assert len(ptrs) <= 2 and s1["reused"] - s0["reused"] >= 18, (ptrs, s0, s1)
    assert placement.split_stats(0)["address_space_reserved"] == va_early
    _report("g/recycling", "grad_split" + (" side-stream queue" if side else ""), "split", len(ptrs), 0, 0.0)
