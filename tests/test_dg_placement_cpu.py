"""The placement pass of the DG sweep (tools/fuzz_dg.py: operands at every accepted address offset) without a GPU: the
fixed case list reaches every coverage minimum, every ``REPRO`` line round-trips, the embedding helper puts arrays at
the requested address between the bands its checkers look at, and the checkers reject planted errors."""

import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parents[1] / "tools"))
import fuzz_autograd as A  # noqa: E402
import fuzz_dg as D  # noqa: E402

SEED = 20261018   # tests/test_gpu_dg_placement.py sweeps the same cases
PARTS = ("exact", "signed", "large")
LARGE = {("grad", 100_007), ("div", 100_007), ("grad", 170_003)}

torch = pytest.importorskip("torch")


# --------------------------------------------------------------------------
# the case list
# --------------------------------------------------------------------------

@pytest.mark.parametrize("part", PARTS)
def test_case_list_reaches_every_minimum(part):
    cnt = D.placement_coverage(SEED, part)
    missing = D.missing_buckets(cnt, D.PLACEMENT_MINIMUMS[part])
    assert not missing, missing


def test_minimums_name_every_kind_role_pair_and_float32_shift():
    m = D.PLACEMENT_MINIMUMS["exact"]
    for kind in D.KINDS + ("pipeline",):
        assert {f"role:{kind}:{r}" for r in ("operator", "field", "output")} <= set(m)
        assert (f"role:{kind}:geometry" in m) == (kind != "apply")        # "ij,ej->ei" has no geometric factor
    for kind in ("bgrad", "bdiv", "divcomp", "cross", "fm", "fm_ifj", "fm_jfi", "fm_fji", "mass", "lift2", "pipeline"):
        assert {f"role:{kind}:last-field", f"role:{kind}:last-output"} <= set(m)
    assert {f"shift:f32:{n}:{fam}" for n in (4, 8, 12) for fam in ("grad", "div", "fm")} <= set(m)
    assert {"place:" + p for p in D.PLACEMENTS} <= set(m)
    assert {"shift:f64:8", "shift:f32:4", "shift:f32:8", "shift:f32:12", "path:f32-pointer-fallback",
            "path:lds-dma-8"} <= set(m)
    assert all(v >= 1 for part in PARTS for v in D.PLACEMENT_MINIMUMS[part].values())


def test_case_list_is_the_one_the_pass_is_meant_to_run():
    cases = D.placement_cases(SEED)
    small = cases["small"]
    assert {c.kind for c in small} == set(D.KINDS) | {"pipeline"}
    assert {c.fuse for c in small if c.kind == "pipeline"} == {True, False}
    f64 = [c for c in small if c.dtype == "float64"]
    assert {c.E for c in f64} == {1, 5, 16, 17, 64, 65, 1003, 4099}
    assert {(c.Np, c.Nfp) for c in f64 if not c.kind.endswith("2")} >= set(D.ORDERS3[:5])
    assert any(c.Np in (7, 13) for c in f64) and any(c.kind.endswith("2") for c in f64)
    f32 = [c for c in small if c.dtype == "float32"]
    assert {c.E for c in f32} == {16, 64, 1024, 4096, 17, 1003}
    for fam in ("grad", "div", "fm"):
        assert {c.E for c in f32 if c.kind == fam} >= {16, 64, 1024, 4096}
        assert {(c.Np, c.Nfp) for c in f32 if c.kind == fam} == set(D.F32_MFMA_ORDERS)
    assert any(c.b > D.K_MAX_FIELDS for c in f64) and any(c.b > D.K_MAX_FIELDS for c in f32)
    assert {(c.dtype, c.scale) for c in cases["range"]} == {(d, s) for d in ("float64", "float32")
                                                            for s in ("overflow", "subnormal")}
    assert {(c.kind, c.dtype, c.Np) for c in cases["rounds"]} == {("grad", "float64", 35), ("div", "float64", 35),
                                                                  ("fm", "float64", 35), ("grad", "float32", 20)}
    assert all(c.E == 20_004 for c in cases["rounds"])
    assert {(c.kind, c.E) for c in cases["large"]} == LARGE
    assert all(c.dtype == "float64" and c.Np == 35 for c in cases["large"])


def test_only_the_three_large_cases_exceed_20004_elements():
    for part in PARTS:
        for runs in D.placement_runs(SEED, part):
            for run in runs:
                assert run.case.E <= 20_004 or (part == "large" and (run.case.kind, run.case.E) in LARGE)
    assert all(c.E <= 4099 for runs in D.placement_runs(SEED, "signed") for c in [runs[0].case])
    large = D.placement_runs(SEED, "large")
    assert [[r.placement for r in runs] for runs in large] == [["aligned", "all"]] * 3
    assert dict(large[0][0].knobs) == {"tail_rounds": -1, "quarter_tail": True, "staggered_start": False}
    assert large[2][0].knobs == ()


def test_placements_of_a_case():
    """The full set: "aligned" in front, one "only:" per geometry and operator array, first / last field and output, a
    field and an output of the second launch group, "all" with every array shifted, "mixed" with some."""
    case = next(c for c in D.placement_cases(SEED)["small"] if c.kind == "fm" and c.b == 9 and c.dtype == "float64")
    ins, outs = D.slots_of(case)
    assert [role for _, role, _, _ in ins] == ["geometry", "operator"] + ["field"] * 9 and len(outs) == 9
    pl = D.placements_of(case, True)
    assert pl[0] == ("aligned", ())
    only = [(n, s) for n, s in pl if n.startswith("only:")]
    assert all(len(s) == 1 and s[0][1] == 1 for _, s in only)
    assert [(n, s[0][0]) for n, s in only] == [
        ("only:geometry", "J"), ("only:operator", "R"), ("only:field", "v0"), ("only:last-field", "v8"),
        ("only:field", "v8"), ("only:output", "out:0:" + outs[0][2]), ("only:last-output", "out:0:" + outs[8][2]),
        ("only:output", "out:0:" + outs[8][2])]
    every = {k for k, *_ in ins} | {slot for slot, *_ in outs}
    assert {k for k, _ in dict(pl)["all"]} == every
    mixed = {k for k, _ in dict(pl)["mixed"]}
    assert mixed and mixed < every
    assert [n for n, _ in D.placements_of(case, False)] == ["aligned", "all"]
    comp = next(c for c in D.placement_cases(SEED)["small"] if c.kind == "divcomp")
    assert [s[0][0] for n, s in D.placements_of(comp, True) if n == "only:geometry"] == ["Jx", "Jy", "Jz"]
    # float32: shifts of 1, 2 and 3 elements among the "only:" placements of one case; non-zero everywhere in "all"
    f32 = next(c for c in D.placement_cases(SEED)["small"] if c.dtype == "float32" and c.kind == "grad")
    pl = D.placements_of(f32, True)
    assert {s[0][1] for n, s in pl if n.startswith("only:")} == {1, 2, 3}
    assert all(1 <= v <= 3 for _, v in dict(pl)["all"])
    # mixed cases: float32 fields, float64 elsewhere
    mx = next(c for c in D.placement_cases(SEED)["small"] if c.dtype == "mixed" and c.kind == "grad")
    assert {k: dt.itemsize for k, _, dt, _ in D.slots_of(mx)[0]} == {"J": 8, "R": 8, "u0": 4}
    assert dict(dict(D.placements_of(mx, True))["all"])["J"] == 1
    # runs: the full set under "auto" and "mfma", "aligned" and "all" under the other transforms
    runs = next(r for r in D.placement_runs(SEED, "exact") if r[0].case == case)
    by_t = {}
    for r in runs:
        by_t.setdefault(r.transform, []).append(r.placement)
    assert set(by_t) == set(D.TRANSFORMS)
    assert all(v[0] == "aligned" for v in by_t.values())
    assert by_t["auto"] == by_t["mfma"] == [n for n, _ in D.placements_of(case, True)]
    assert all(by_t[t] == ["aligned", "all"] for t in ("tiled", "generic", "mfma_split", "prepared"))


def test_every_repro_line_round_trips():
    n = 0
    for part in PARTS:
        for runs in D.placement_runs(SEED, part):
            for run in runs:
                back = D.PlacedRun.from_repro(run.repro())
                assert back == run and back.repro() == run.repro()
                n += 1
    assert n > 1000
    # a replayed line makes the same placement, shifts included, without the generator
    run = next(r for runs in D.placement_runs(SEED, "exact") for r in runs if r.placement == "mixed"
               and r.case.dtype == "float32")
    assert dict(D.PlacedRun.from_repro(run.repro()).shifts) == dict(run.shifts) and run.shifts


def test_path_buckets():
    runs = [r for rs in D.placement_runs(SEED, "exact") for r in rs]
    fb = [r for r in runs if "path:f32-pointer-fallback" in D.placement_buckets(r)]
    assert fb and all(r.case.dtype == "float32" and r.case.E % 4 == 0 and r.case.E >= 16 and r.shifts
                      and r.transform in ("auto", "mfma") and (r.case.Np, r.case.Nfp) in D.F32_MFMA_ORDERS for r in fb)
    # each pointer of the launcher's predicate is the only unaligned one in some run
    assert {r.placement for r in fb} >= {"only:geometry", "only:operator", "only:field", "only:last-field",
                                         "only:output", "only:last-output"}
    dma = [r for r in runs if "path:lds-dma-8" in D.placement_buckets(r)]
    assert dma and all(r.case.kind in ("grad", "bgrad") and r.case.dtype == "float64" and r.transform in ("auto", "mfma")
                       and any(k.startswith("u") for k, _ in r.shifts) for r in dma)
    assert {r.case.Np for r in dma} == set(D.PADDED_ORDERS)
    assert any(r.case.E == 20_004 for r in dma)


# --------------------------------------------------------------------------
# the embedding helper
# --------------------------------------------------------------------------

@pytest.mark.parametrize("dtype,shift", [("float64", 0), ("float64", 1), ("float32", 0), ("float32", 1),
                                         ("float32", 2), ("float32", 3)])
@pytest.mark.parametrize("role", ["in", "out"])
def test_embed_address_shape_and_bands(dtype, shift, role):
    dt = getattr(torch, dtype)
    esize = 4 if dtype == "float32" else 8
    for shape in [(5,), (3, 7, 11), (1, 1), (4, 17)]:
        values = torch.arange(int(np.prod(shape)), dtype=dt).reshape(shape) + 1
        emb = D.embed(torch, shape, dt, shift, role, values if role == "in" else None, device="cpu")
        assert emb.view.data_ptr() % 16 == shift * esize % 16 and emb.view.data_ptr() % 256 == shift * esize
        assert emb.view.is_contiguous() and tuple(emb.view.shape) == shape and emb.view.dtype == dt
        assert emb.view.data_ptr() == emb.buf.data_ptr() + emb.lead * esize
        lo, hi = emb.bands()
        assert lo.numel() >= D.BAND >= D.GUARD and hi.numel() >= D.BAND
        assert lo.numel() + emb.n + hi.numel() == emb.buf.numel()
        ints = emb.ints()
        if role == "in":
            assert torch.equal(emb.view, values)
            assert bool((ints[:emb.lead] == D.IN_NAN[esize]).all()) and bool((ints[emb.lead + emb.n:] == D.IN_NAN[esize]).all())
            assert bool(torch.isnan(lo).all()) and bool(torch.isnan(hi).all())
        else:
            assert bool((lo == D.SENTINEL).all()) and bool((hi == D.SENTINEL).all()) and emb.guards_intact()
            assert bool((ints[emb.lead:emb.lead + emb.n] == D.OUT_NAN[esize]).all()) and bool(torch.isnan(emb.view).all())
            # the view is the payload: writing all of it leaves the bands alone, one element further does not
            emb.view.fill_(1.0)
            assert emb.guards_intact() and not bool(torch.isnan(emb.buf).any())


def test_embed_refuses_shifts_the_dtype_does_not_have():
    with pytest.raises(AssertionError):
        D.embed(torch, (4,), torch.float64, 2, "out", device="cpu")
    with pytest.raises(AssertionError):
        D.embed(torch, (4,), torch.float32, 4, "out", device="cpu")


def test_checksum_sees_what_a_copy_sees():
    rng = np.random.default_rng(3)
    for n in (1, 2, 3, 7, 64, 1001):
        a = torch.from_numpy(rng.integers(-2**62, 2**62, size=n))
        total, xor = D._checksum(a)
        assert xor == int(np.bitwise_xor.reduce(a.numpy())) and total == int(a.numpy().sum())
        b = a.clone()
        b[n // 2] ^= 1 << 40
        assert D._checksum(b) != (total, xor)


# --------------------------------------------------------------------------
# the checkers reject planted errors
# --------------------------------------------------------------------------

def _quiet(st):
    st.fail = lambda line, _st=st: setattr(_st, "failures", _st.failures + 1) or _st.lines.append(line)
    st.lines = []
    return st


def _stats():
    return _quiet(D.Stats("planted"))


def _small():
    """A float64 grad case on the host: inputs embedded on the CPU, the exact reference, a run to name in lines."""
    case = D.DGCase("grad", 10, 6, 1, "rij", "float64", 17, "ragged", 3)
    arrays, mants, scales, sig = D.host_data(case)
    expr, keys = case.stages()[0]
    ks = [keys[a.name] for a in expr.args[0]]
    ref = D.ref_.int_reference(expr.get_subscripts(), [mants[k] for k in ks], sum(scales[k] for k in ks), np.float64, sig)
    run = D.PlacedRun(case, "exact", "mfma", "all", tuple(sorted((s, 1) for s in ks + ["out:0:" + expr.output_names[0]])))
    ins = {}
    for key, _, dt, shape in D.slots_of(case)[0]:
        emb = D.embed(torch, shape, torch.float64, 1, "in", torch.from_numpy(arrays[key]), device="cpu")
        ins[key] = (emb, emb.snapshot())
    name = expr.output_names[0]
    return case, run, ins, name, torch.from_numpy(ref)


def _output(name, ref, shift=1):
    emb = D.embed(torch, tuple(ref.shape), ref.dtype, shift, "out", device="cpu")
    emb.view.copy_(ref)
    return [{name: emb}]


@pytest.mark.parametrize("checksum", [False, True])
def test_input_checker_rejects_a_changed_payload_or_band_element(checksum):
    case, run, ins, name, ref = _small()
    if checksum:
        ins = {k: (emb, emb.snapshot(True)) for k, (emb, _) in ins.items()}
    st = _stats()
    assert D.check_inputs(st, "clean", run, ins) and st.failures == 0
    emb = ins["u0"][0]
    # one payload element changed (by one ulp)
    old = emb.view[3, 4].clone()
    emb.view[3, 4] = torch.nextafter(old, old + 1)
    assert not D.check_inputs(st, "payload", run, ins) and st.failures == 1
    assert "input u0 changed" in st.lines[-1] and run.repro() in st.lines[-1]
    if not checksum:
        assert f"element {3 * 10 + 4})" in st.lines[-1]
    emb.view[3, 4] = old
    assert D.check_inputs(st, "restored", run, ins) and st.failures == 1
    # one band element changed to another NaN bit pattern (still a NaN: only the integer view can tell)
    for at in (emb.lead - 1, emb.lead + emb.n, 0, emb.buf.numel() - 1):
        emb.ints()[at] = 0x7FF8_0000_0000_0000
        assert bool(torch.isnan(emb.buf[at]))
        assert not D.check_inputs(st, "band", run, ins)
        emb.ints()[at] = D.IN_NAN[8]
    assert st.failures == 5 and D.check_inputs(st, "restored", run, ins)


def test_output_checker_rejects_an_overwritten_band_element():
    case, run, ins, name, ref = _small()
    for at in (-1, 0):    # the last element in front of the output, the first behind it
        st = _stats()
        outs = _output(name, ref)
        assert D.check_outputs(st, "clean", run, outs, [{name: ref}]) and st.failures == 0
        emb = outs[0][name]
        emb.buf[emb.lead - 1 if at else emb.lead + emb.n] = 0.0
        assert not D.check_outputs(st, "band", run, outs, [{name: ref}])
        assert st.failures == 1 and "wrote outside its output" in st.lines[-1] and run.repro() in st.lines[-1]


def test_a_nan_in_an_output_lands_in_the_leak_bucket():
    case, run, ins, name, ref = _small()
    st = _stats()
    outs = _output(name, ref)
    outs[0][name].view[1, 5, 2] = float("nan")
    assert not D.check_outputs(st, "leak", run, outs, [{name: ref}])
    assert st.cov["leak:nan-entries"] == 1 and "unwritten:entries" not in st.cov
    assert any("over-read" in line for line in st.lines)
    assert st.exact_runs == 1 and st.exact_equal == 0
    # an entry the launch never wrote still holds the output's own NaN: not an over-read
    st = _stats()
    outs = _output(name, ref)
    outs[0][name].ints()[outs[0][name].lead + 7] = D.OUT_NAN[8]
    assert not D.check_outputs(st, "unwritten", run, outs, [{name: ref}])
    assert st.cov["unwritten:entries"] == 1 and st.cov["leak:nan-entries"] == 0
    # signed data (no exact reference): the same buckets
    st = _stats()
    outs = _output(name, ref)
    outs[0][name].view[0, 0, 0] = float("nan")
    assert not D.check_outputs(st, "leak", run, outs)
    assert st.cov["leak:nan-entries"] == 1


def test_one_ulp_off_the_aligned_launch_is_rejected_though_inside_the_bound():
    case, run, ins, name, _ = _small()
    expr, keys = case.stages()[0]
    rng = np.random.default_rng(11)
    host = [(rng.random(D._shape(expr, a.name, case.E)) * 2 - 1) for a in expr.args[0]]
    r, ar = D.ref_.bounded_reference(expr.get_subscripts(), host)
    nb = D.ref_.bound_terms(expr.get_subscripts(), D._extent(expr, case.E), 3)
    got = torch.from_numpy(np.einsum(expr.get_subscripts(), *host, optimize=True))
    base = [{name: got.clone().view(torch.int64)}]
    st = _stats()
    assert D.check_outputs(st, "same", run, _output(name, got), None, base) and st.exact_runs == st.exact_equal == 1
    off = got.clone()
    k = int(torch.argmax(off.abs()))
    off.view(-1)[k] = torch.nextafter(off.view(-1)[k], torch.tensor(np.inf, dtype=torch.float64))
    assert D.ref_.bound_ratio(off.numpy(), r, ar, nb, D.ref_.U64) <= 1          # inside the bound
    assert not D.check_outputs(st, "ulp", run, _output(name, off), None, base)
    assert st.failures == 1 and st.exact_runs == 2 and st.exact_equal == 1
    assert "differ bitwise from the aligned launch" in st.lines[-1] and run.repro() in st.lines[-1]


# --------------------------------------------------------------------------
# the adjoint kernels
# --------------------------------------------------------------------------

def test_kernel_shifts_by_role():
    ins = [("J", "geometry"), ("R", "operator"), ("g0", "field"), ("g1", "field"), ("v0", "field"), ("v1", "field")]
    outs = ["dv0", "dv1", "dJ"]
    one = lambda p: [n for n, s in A.kernel_shifts(p, ins, outs).items() if s]   # noqa: E731
    assert one("aligned") == [] and one(None) == []
    assert one("all") == [n for n, _ in ins] + outs
    assert [one("only:" + r) for r in ("geometry", "operator", "field", "last-field", "output", "last-output")] == \
        [["J"], ["R"], ["g0"], ["v1"], ["dv0"], ["dJ"]]
    assert one("only:geometry") == ["J"]
    assert A.kernel_shifts("only:geometry", [("D", "operator"), ("a", "field"), ("b", "field")], ["out"]) == \
        {"D": 0, "a": 0, "b": 0, "out": 0}
    with pytest.raises(AssertionError):
        A.kernel_shifts("only:nothing", ins, outs)


def test_kernel_placement_runs_cover_every_layout():
    from feinsum_amd.family import FACEMASS_ADJ_SHAPES, GEOMADJ_NP

    geom, fm = A.placement_kernel_runs(SEED)
    full = A.geomadj_runs(SEED)
    assert set(geom) <= set(full) and len(geom) < len(full) / 2
    assert {(Np, lay, op) for Np, _, _, op, lay, _, _ in geom} == {(Np, lay, op) for Np in GEOMADJ_NP
                                                                   for lay in A.GEOM_LAYOUTS for op in (0, 1)}
    assert {(X, R) for _, X, R, _, lay, _, _ in geom if lay == "xre"} == {(x, r) for x in (1, 2, 3) for r in (1, 2, 3)}
    assert {(s, lay[2]) for s, lay, *_ in fm} == {(s, fl) for s in FACEMASS_ADJ_SHAPES for _, _, fl in A.FM_LAYOUT_FLAGS}
    assert {b for _, _, b, *_ in fm} == {1, 2, 4, 9}
    for s in FACEMASS_ADJ_SHAPES:
        assert {b for sh, _, b, *_ in fm if sh == s} >= {1, 2, 4}
    assert {w for _, _, _, w, _, _ in fm} == {"dv", "dJ", "both"}
    assert {E for *_, E, _ in geom} | {E for *_, E, _ in fm} <= set(A.KERNEL_E)


def test_operator_gradient_placement_runs_cover_every_layout():
    """The counts tests/test_gpu_dg_placement.py asks of the operator-gradient kernels, from the run lists alone:
    "aligned" and "all" run every run, each of the six "only:" placements every third one."""
    from collections import Counter

    og, fm = A.placement_opgrad_runs(SEED)
    assert len(og) == 32 and len(fm) == 16
    cnt = Counter()
    for k, placement in enumerate(A.KERNEL_PLACEMENTS):
        every = placement in ("aligned", "all")
        for Np, X, R, lay, ol, nk, E, s in (og if every else og[k % 3::3]):
            cnt.update([f"opgrad:{lay},{ol}", f"opgrad:E{E}", "place:" + placement, "opgrad:workspace"])
        for shape, (jl, rl, flags), b, E, s in (fm if every else fm[k % 3::3]):
            cnt.update([f"opgrad_fm:{jl},{rl}", f"opgrad_fm:b{b}", f"opgrad:E{E}", "place:" + placement, "opgrad:workspace"])
    assert all(cnt[f"opgrad:{lay},{ol}"] >= 8 for lay in A.GEOM_LAYOUTS for ol in A.OPGRAD_OUT_LAYOUTS)
    assert all(cnt[f"opgrad_fm:{jl},{rl}"] >= 4 for jl, rl, _ in A.FM_LAYOUT_FLAGS)
    assert all(cnt[f"opgrad_fm:b{b}"] >= 16 for b in (1, 2, 4, 9)) and all(cnt[f"opgrad:E{E}"] >= 8 for E in A.OPGRAD_E)
    assert all(cnt["place:" + p] >= 15 for p in A.KERNEL_PLACEMENTS) and cnt["place:aligned"] == cnt["place:all"] == 48
    assert cnt["opgrad:workspace"] >= 192
    # the workspace (256-byte aligned by contract) is never shifted: every placement leaves it on its boundary
    outs, _ = A._with_workspace({"out": (3, 4, 4)}, 65, 48)
    x = {"J": np.zeros((3, 3, 65)), "a0": np.zeros((65, 4)), "b0": np.zeros((3, 65, 4))}
    ins = [("J", "geometry"), ("a0", "field"), ("b0", "field")]
    saved, A.DEVICE = A.DEVICE, "cpu"
    try:
        for placement in A.KERNEL_PLACEMENTS:
            arrays = A._KernelArrays(torch, placement, x, ins, outs)
            assert arrays.out["ws"].data_ptr() % 256 == 0 and arrays.out["ws"].numel() * 8 == A._with_workspace({}, 65, 48)[1]
            assert arrays.out["out"].data_ptr() % 256 == (8 if placement in ("all", "only:output", "only:last-output") else 0)
            assert arrays.d["b0"].data_ptr() % 256 == (8 if placement in ("all", "only:last-field") else 0)
            arrays.out["ws"].fill_(1.0)
            assert arrays.guards_intact()
            arrays._outs["ws"].buf[arrays._outs["ws"].lead + arrays._outs["ws"].n] = 0.0      # one element behind the planned bytes
            assert not arrays.guards_intact()
    finally:
        A.DEVICE = saved
