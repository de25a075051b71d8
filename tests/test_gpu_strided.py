"""grad, div and face-mass on element slices of larger arrays, on the device: every family, order,
size, field count, layout and placement of tools/fuzz_strided.py against the contiguous launch (bitwise) and the int64 einsum
(exact), with NaN around the inputs and a sentinel around the outputs; what is refused; aliasing; two streams; operators."""
import sys
from pathlib import Path

import pytest
import torch

import feinsum_amd as f
from feinsum_amd import _hip

sys.path.insert(0, str(Path(__file__).resolve().parents[1] / "tools"))
import fuzz_strided as fs   # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.mark.parametrize("p", (1, 2, 3, 4))
@pytest.mark.parametrize("family", ("grad", "div", "fm"))
def test_slices_match_the_contiguous_launch_and_the_exact_einsum(family, p):
    cases = fs.cases_of(family, p)
    assert {c.n for c in cases} == set(fs.sizes(family, p)) and {c.placement for c in cases} == set(fs.PLACEMENTS)
    assert {(c.b, c.layout) for c in cases} == {(b, lay) for b in fs.FIELDS[family] for lay in fs.LAYOUTS[family]}
    failures = []
    del fs.LAUNCHES[:]
    for k, case in enumerate(cases):
        failures += fs.run_case(torch, case, DEV, transform=("auto", "mfma")[k % 2], seed=100 * p + k)
    assert not failures, "\n".join(failures[:20])
    walks = {bool(info["dynamic_walk"]) for _label, info in fs.LAUNCHES}
    # both walks are reached: the static one at every order, the dynamic one from the large sizes of p = 4 on
    assert False in walks and (p < 4 or True in walks), sorted({(label, info["dynamic_walk"]) for label, info in fs.LAUNCHES})[-12:]


@pytest.mark.parametrize("role", ("J", "in", "out"))
@pytest.mark.parametrize("family", ("grad", "div", "fm"))
def test_one_sliced_operand_among_whole_arrays(family, role):
    b, layout = fs.FIELDS[family][-1], fs.LAYOUTS[family][-1]      # (face-mass: J stored fe, the only J layout with an ld)
    failures = []
    for p, n in ((4, 83), (2, 131)):
        failures += fs.run_case(torch, fs.Case(family, p, n, b, layout, "odd", only=role), DEV, seed=7)
    assert not failures, "\n".join(failures)


def _whole(case, kind="real", seed=3):
    """Contiguous operands of a case on the device: (expr, inputs, values)."""
    vals = fs.make_values(torch, case, kind, seed, DEV)
    return fs.expression(case), vals


@pytest.mark.parametrize("family,p,n,b,layout", [("grad", 4, 1003, 3, "rji"), ("grad", 2, 100, 1, "rij"), ("div", 4, 1003, 3, "rij"),
                                                 ("div", 1, 7, 1, "rji"), ("fm", 4, 1003, 4, "fe,jfi"), ("fm", 3, 33, 2, "ef,fij")])
def test_every_ld_equal_to_n_is_the_contiguous_entry_point_bitwise(family, p, n, b, layout):
    case = fs.Case(family, p, n, b, layout, "zero")
    expr, vals = _whole(case)
    ref = f.evaluate(expr, 0, vals, wait=True)
    Np, Nfp = fs.ORDERS[p]
    plan = f.match_family(expr)
    outs = [torch.full_like(ref[name], float("nan")) for name in expr.output_names]
    u, o = [vals[f"v{k}"].data_ptr() for k in range(b)], [t.data_ptr() for t in outs]
    if family == "grad":
        _hip.grad3d_strided(vals["J"].data_ptr(), n, vals["A"].data_ptr(), u, o, n, n, Np, plan.layout_flags)
    elif family == "div":
        _hip.div3d_strided(vals["J"].data_ptr(), n, vals["A"].data_ptr(), u, n, o, n, Np, plan.layout_flags)
    else:
        _hip.facemass_strided(vals["J"].data_ptr(), n, vals["A"].data_ptr(), u, n, o, n, Np, 4, Nfp, plan.layout_flags)
    info = _hip.last_launch_info()
    torch.cuda.synchronize()
    if n >= 16 * fs.SUBTILES[family][p - 1]:
        assert info["element_slice"] and info["tiles"] > 0 and not info["dynamic_walk"]
    for name, got in zip(expr.output_names, outs):
        assert torch.equal(got.view(torch.int64), ref[name].view(torch.int64)), (family, name)


# ---- refusals: InvalidParameterError before anything is launched ---------------------------------------------------

def _sliced_grad(n=100, p=4, dtype=torch.float64):
    """grad with every operand a slice; (expr, args, out_dict, output bases)."""
    case = fs.Case("grad", p, n, 1, "rij", "odd")
    vals = fs.make_values(torch, case, "real", 11, DEV)
    ins, outs = fs.bind_sliced(torch, case, vals, DEV)
    expr = fs.expression(case)
    return case, expr, {k: op.view for k, op in ins.items()}, {expr.output_names[0]: outs[0].view}, outs


def _refused(expr, args, out_dict, outs, match="contiguous", **kw):
    with pytest.raises(f.InvalidParameterError, match=match):
        f.evaluate(expr, 0, args, out_dict=out_dict, **kw)
    torch.cuda.synchronize()
    assert all(o.outside_is(torch, fs.SENTINEL) and bool((o.view.contiguous().view(torch.int64) == fs.SENTINEL).all()) for o in outs)


def test_what_does_not_take_slices_is_refused_with_the_outputs_intact():
    case, expr, args, out_dict, outs = _sliced_grad()
    f.evaluate(expr, 0, args, out_dict=out_dict, wait=True)             # (the slices themselves are fine)
    outs[0].base.view(torch.int64).fill_(fs.SENTINEL)
    n = case.n
    stepped = torch.zeros((2 * n, 35), dtype=torch.float64, device=DEV)[::2]
    _refused(expr, {**args, "v0": stepped}, out_dict, outs)                                   # a stepped slice
    bigD = torch.zeros((3, 40, 35), dtype=torch.float64, device=DEV)
    _refused(expr, {**args, "A": bigD.narrow(1, 2, 35)}, out_dict, outs)                      # a sliced D
    _refused(expr, {**args, "A": args["A"].transpose(1, 2)}, out_dict, outs)
    _refused(expr, args, out_dict, outs, alpha=2.0)                                           # alpha / beta with a slice
    _refused(expr, args, out_dict, outs, beta=1.0)
    _refused(expr, args, out_dict, outs, alpha=0.5, beta=-1.0, transform={"accumulate": "epilogue"})
    for transform in ("generic", "tiled", "mixed_family"):
        _refused(expr, args, out_dict, outs, transform=transform)
    # float32 with a slice
    e32 = f.einsum("xre,rij,ej->xei", f.array("J", (3, 3, "E"), "float32"), f.array("A", (3, 35, 35), "float32"),
                   f.array("v0", ("E", 35), "float32"))
    a32 = {"J": torch.zeros((3, 3, 2 * n), dtype=torch.float32, device=DEV).narrow(2, 1, n),
           "A": torch.zeros((3, 35, 35), dtype=torch.float32, device=DEV), "v0": torch.zeros((n, 35), dtype=torch.float32, device=DEV)}
    with pytest.raises(f.InvalidParameterError, match="contiguous"):
        f.evaluate(e32, 0, a32)
    # float32 fields in float64 geometry ("mixed_family")
    emx = f.einsum("xre,rij,ej->xei", f.array("J", (3, 3, "E")), f.array("A", (3, 35, 35)), f.array("v0", ("E", 35), "float32"))
    with pytest.raises(f.InvalidParameterError, match="contiguous"):
        f.evaluate(emx, 0, {"J": args["J"], "A": args["A"], "v0": a32["v0"]}, transform="mixed_family")
    # face-mass of one field
    c1 = fs.Case("fm", 4, n, 1, "fe,fij", "odd")
    v1 = fs.make_values(torch, c1, "real", 5, DEV)
    ins1, outs1 = fs.bind_sliced(torch, c1, v1, DEV)
    e1 = fs.expression(c1)
    _refused(e1, {k: op.view for k, op in ins1.items()}, {e1.output_names[0]: outs1[0].view}, outs1)
    # the adjoint kernels
    with pytest.raises(f.InvalidParameterError, match="contiguous"):
        f.evaluate_differentiable(expr, 0, args)
    # p = 5 and triangles
    e5 = f.einsum("xre,rij,ej->xei", f.array("J", (3, 3, "E")), f.array("A", (3, 56, 56)), f.array("v0", ("E", 56)))
    with pytest.raises(f.InvalidParameterError, match="contiguous"):
        f.evaluate(e5, 0, {"J": args["J"], "A": torch.zeros((3, 56, 56), dtype=torch.float64, device=DEV),
                           "v0": torch.zeros((n, 56), dtype=torch.float64, device=DEV)})


def test_an_output_range_that_shares_an_element_with_an_input_range_is_refused():
    n, Np = 64, 35
    expr = f.einsum("xre,rij,xej->ei", f.array("J", (3, 3, "E")), f.array("A", (3, Np, Np)), f.array("v0", (3, "E", Np)))
    # div reads (3, E, Np) and writes (E, Np): plane 0 of one base array holds the field's first plane AND the output
    base = torch.randn((3, 4 * n, Np), dtype=torch.float64, device=DEV)
    args = {"J": torch.randn((3, 3, n), dtype=torch.float64, device=DEV), "A": torch.randn((3, Np, Np), dtype=torch.float64, device=DEV),
            "v0": base.narrow(1, 0, n)}
    name = expr.output_names[0]
    with pytest.raises(f.InvalidParameterError, match="shares memory"):
        f.evaluate(expr, 0, args, out_dict={name: base[0].narrow(0, n - 1, n)})       # one element shared
    adjacent = base[0].narrow(0, n, n)                                                   # elements n .. 2n of plane 0: adjacent
    want = f.evaluate(expr, 0, {k: v.contiguous() for k, v in args.items()}, wait=True)[name]
    keep = base.clone()
    f.evaluate(expr, 0, args, out_dict={name: adjacent}, wait=True)
    assert torch.equal(adjacent.view(torch.int64), want.view(torch.int64))
    keep[0, n:2 * n] = want
    assert torch.equal(base.view(torch.int64), keep.view(torch.int64))
    # between the planes of the field lies memory that is not the field's: an output there overlaps nothing
    gap = base[1].narrow(0, 2 * n, n)
    f.evaluate(expr, 0, args, out_dict={name: gap}, wait=True)
    assert torch.equal(gap.view(torch.int64), want.view(torch.int64))


def test_two_streams_write_disjoint_ranges_of_the_same_outputs():
    n1, n2, Np = 160, 147, 35
    E = n1 + n2
    case = fs.Case("grad", 4, E, 1, "rij", "zero")
    expr = fs.expression(case)
    vals = fs.make_values(torch, case, "real", 21, DEV)
    name = expr.output_names[0]
    out = torch.full((3, E, Np), float("nan"), dtype=torch.float64, device=DEV)
    torch.cuda.synchronize()
    queues = [f.DeviceQueue(0, stream=torch.cuda.Stream(DEV)) for _ in range(2)]
    parts = []
    for q, (a, n) in zip(queues, ((0, n1), (n1, n2))):
        args = {"J": vals["J"].narrow(2, a, n), "A": vals["A"], "v0": vals["v0"].narrow(0, a, n)}
        f.evaluate(expr, q, args, out_dict={name: out.narrow(1, a, n)})
        parts.append(args)
    for q in queues:
        q.finish()
    for args, (a, n) in zip(parts, ((0, n1), (n1, n2))):
        ref = f.evaluate(expr, 0, {k: v.contiguous() for k, v in args.items()}, wait=True)[name]
        assert torch.equal(out.narrow(1, a, n).contiguous().view(torch.int64), ref.view(torch.int64))


def test_a_sliced_stage_of_an_operator_is_a_launch_of_its_own():
    n, Np = 400, 35
    J = torch.randn((3, 3, 2 * n + 1), dtype=torch.float64, device=DEV)
    D = torch.randn((3, Np, Np), dtype=torch.float64, device=DEV)
    u = torch.randn((n, Np), dtype=torch.float64, device=DEV)
    w = torch.randn((3, n, Np), dtype=torch.float64, device=DEV)
    grad = f.einsum("xre,rij,ej->xei", f.array("J", (3, 3, "E")), f.array("D", (3, Np, Np)), f.array("u", ("E", Np)))
    div = f.einsum("xre,rij,xej->ei", f.array("J", (3, 3, "E")), f.array("D", (3, Np, Np)), f.array("w", (3, "E", Np)))
    Jw = J.narrow(2, 0, n).contiguous()
    whole = f.bind_operator([(grad, {"J": Jw, "D": D, "u": u}), (div, {"J": Jw, "D": D, "w": w})], 0)
    assert len(whole.launches) == 1                                      # contiguous stages fuse
    stages = [(grad, {"J": J.narrow(2, 1, n), "D": D, "u": u}), (div, {"J": Jw, "D": D, "w": w})]
    op = f.bind_operator(stages, 0)
    assert len(op.launches) == 2 and op.entry_points[0] == "fe_grad3d_strided_f64"
    op.launch()
    op.queue.finish()
    want = [f.evaluate(expr, 0, {k: v.contiguous() for k, v in arrays.items()}, wait=True) for expr, arrays in stages]
    for got, ref in zip(op.outputs, want):
        for name in ref:
            assert torch.equal(got[name].view(torch.int64), ref[name].view(torch.int64))
    for got in op.outputs:
        for t in got.values():
            t.fill_(float("nan"))
    op.capture()
    op.replay()
    torch.cuda.synchronize()
    for got, ref in zip(op.outputs, want):
        for name in ref:
            assert torch.equal(got[name].view(torch.int64), ref[name].view(torch.int64))
    op.release_graph()


def _fields_from_bases(family, p, n, lengths, seed=31):
    """A launch group whose fields (and outputs) are slices of bases of the given lengths, field k out of lengths[k]:
    (expr, args, out_dict, output operands, dense values)."""
    case = fs.Case(family, p, n, len(lengths), fs.LAYOUTS[family][-1], "odd")
    vals = fs.make_values(torch, case, "real", seed, DEV)
    r = fs.roles_of(case)
    expr = fs.expression(case)
    ins = {"J": fs.Operand(torch, r["J"][1], r["J"][2], 3, n + 8, vals["J"], fs.IN_NAN, DEV),
           "A": fs.Operand(torch, r["op"][1], None, 0, 0, vals["A"], fs.IN_NAN, DEV)}
    outs = []
    for k, ld in enumerate(lengths):
        ins[f"v{k}"] = fs.Operand(torch, r["in"][1], r["in"][2], 1, ld, vals[f"v{k}"], fs.IN_NAN, DEV)
        outs.append(fs.Operand(torch, r["out"][1], r["out"][2], 2, ld + 1, None, fs.SENTINEL, DEV))
    return expr, {k: o.view for k, o in ins.items()}, {name: o.view for name, o in zip(expr.output_names, outs)}, outs, vals


@pytest.mark.parametrize("family,lengths,launches", [("grad", (150, 150, 161), 2), ("div", (150, 161, 150, 161), 2),
                                                      ("fm", (150, 161, 150, 161), 2), ("fm", (150, 150, 161, 161, 161), 2)])
def test_fields_of_one_group_from_bases_of_different_length_run_as_one_launch_per_length(family, lengths, launches):
    n = 131
    expr, args, out_dict, outs, vals = _fields_from_bases(family, 2, n, lengths)
    from feinsum_amd.measure import _bind
    _, bound, _ = _bind(expr, 0, args, out_dict, None)
    assert len(bound.calls) == launches and sorted(m for rows in bound.rows for m in rows) == list(range(len(lengths)))
    for rows in bound.rows:                                   # a launch holds the fields of ONE base length
        assert len({lengths[m] for m in rows}) == 1
    f.evaluate(expr, 0, args, out_dict=out_dict, wait=True)
    ref = {name: torch.empty_like(o.view, memory_format=torch.contiguous_format) for name, o in zip(expr.output_names, outs)}
    f.evaluate(expr, 0, vals, out_dict=ref, wait=True)
    for name, o in zip(expr.output_names, outs):
        assert torch.equal(o.view.contiguous().view(torch.int64), ref[name].view(torch.int64)), name
        assert o.outside_is(torch, fs.SENTINEL)


def test_a_face_mass_field_alone_with_its_leading_dimension_is_refused_before_anything_is_allocated():
    n = 131
    expr, args, out_dict, outs, _vals = _fields_from_bases("fm", 2, n, (150, 150, 161))
    _refused(expr, args, out_dict, outs, match="alone in its launch group")
    # ... also where the outputs are the library's to allocate: refused before it allocates them
    before = torch.cuda.memory_allocated()
    with pytest.raises(f.InvalidParameterError, match="contiguous"):
        f.evaluate(expr, 0, args)
    assert torch.cuda.memory_allocated() == before
