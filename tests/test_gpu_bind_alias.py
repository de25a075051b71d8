"""The aliasing rule of ``evaluate`` / ``bind_operator``: an evaluation whose outputs share a byte with any of its
inputs, or with each other, is refused (``InvalidParameterError``) before anything is allocated, prepared or launched,
and nothing has changed afterwards; views that merely touch are accepted and exact.  Small-integer data: every sum is
exact in float32 and float64, the reference is numpy's int64 einsum."""

import numpy as np
import pytest

import feinsum_amd as f
from feinsum_amd.diagnostics import InvalidParameterError

pytestmark = pytest.mark.gpu

NP, NFP = 4, 3          # p = 1: every array of every family is a whole number of 16-byte units
KINDS = {   # kind -> (subscripts, shapes by role in operand order, roles)
    "grad": ("xre,rij,ej->xei", ((3, 3, "E"), (3, NP, NP), ("E", NP)), ("J", "D", "u")),
    "div": ("xre,rij,xej->ei", ((3, 3, "E"), (3, NP, NP), (3, "E", NP)), ("J", "D", "u")),
    "divcomp": ("re,rij,ej->ei", ((3, "E"), (3, NP, NP), ("E", NP)), ("J", "D", "u")),
    "facemass": ("ef,fij,fej->ei", (("E", 4), (4, NP, NFP), (4, "E", NFP)), ("J", "D", "u")),
    "mass": ("e,ij,ej->ei", (("E",), (NP, NP), ("E", NP)), ("J", "D", "u")),
    "apply": ("ij,ej->ei", ((NP, NP), ("E", NP)), ("D", "u")),
}
SAME_SHAPE = ("apply", "mass", "divcomp")     # the output has the field's shape
SIZES = (5, 17, 1003)
DTYPES = ("float64", "float32")
every = pytest.mark.parametrize("kind,dtype,E", [(k, d, E) for k in KINDS for d in DTYPES for E in SIZES])


@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def _expr(kind, dtype, b=1):
    subs, shapes, roles = KINDS[kind]
    rows = [[f.array(r if (r != "u" or b == 1) else f"u{k}", s, dtype) for r, s in zip(roles, shapes)] for k in range(b)]
    return f.batched_einsum(subs, rows)


def _concrete(shape, E):
    return tuple(E if d == "E" else d for d in shape)


def _host(expr, E, seed):
    rng = np.random.default_rng(seed)
    return {nm: rng.integers(-2, 3, size=_concrete(tuple("E" if isinstance(d, f.SizeParam) else int(d) for d in shp), E))
            for nm, shp in sorted(expr.arg_to_shape.items())}


def _out_shape(expr, E):
    return tuple(E if isinstance(d, f.SizeParam) else int(d) for d in expr.shape)


def _reference(torch, expr, host, dtype, row=0):
    ints = np.einsum(expr.get_subscripts(), *[host[a.name] for a in expr.args[row]])
    return torch.from_numpy(np.asarray(ints).astype(dtype)).cuda()


def _views(torch, dtype, first, second, overlap):
    """Two views of one buffer: *first* (a shape) at its start, *second* right behind it, *overlap* elements earlier."""
    n1, n2 = int(np.prod(first)), int(np.prod(second))
    buf = torch.zeros(n1 + n2 - overlap, dtype=getattr(torch, dtype), device="cuda")
    return buf, buf[:n1].view(first), buf[n1 - overlap:n1 - overlap + n2].view(second)


def _refused(torch, expr, dev, out_dict, names, keep, transform=None):
    """The evaluation raises, its message names both arrays, and every tensor of *keep* is bitwise what it was."""
    before = [t.clone() for t in keep]
    with pytest.raises(InvalidParameterError) as err:
        f.evaluate(expr, 0, dev, out_dict=out_dict, transform=transform, wait=True)
    torch.cuda.synchronize()
    for nm in names:
        assert f"'{nm}'" in str(err.value), (nm, str(err.value))
    for t, b in zip(keep, before):
        assert torch.equal(t, b)


@pytest.mark.parametrize("kind,dtype,E", [(k, d, E) for k in SAME_SHAPE for d in DTYPES for E in SIZES])
def test_output_that_is_an_input_is_refused(torch_cuda, kind, dtype, E):
    torch = torch_cuda
    expr = _expr(kind, dtype)
    dev = {nm: torch.from_numpy(a.astype(dtype)).cuda() for nm, a in _host(expr, E, 1).items()}
    for transform in (None, "generic", "tiled", {"prepared": True}):
        _refused(torch, expr, dev, {"_fe_out": dev["u"]}, ("_fe_out", "u"), list(dev.values()), transform)


@every
def test_output_overlapping_an_input_by_one_element_is_refused(torch_cuda, kind, dtype, E):
    torch = torch_cuda
    expr = _expr(kind, dtype)
    host = _host(expr, E, 2)
    for role in KINDS[kind][2]:
        for out_first in (False, True):
            dev = {nm: torch.from_numpy(a.astype(dtype)).cuda() for nm, a in host.items()}
            in_shape, out_shape = tuple(host[role].shape), _out_shape(expr, E)
            if out_first:
                buf, out, view = _views(torch, dtype, out_shape, in_shape, 1)
            else:
                buf, view, out = _views(torch, dtype, in_shape, out_shape, 1)
            view.copy_(dev[role])
            dev[role] = view
            _refused(torch, expr, dev, {"_fe_out": out}, ("_fe_out", role), [buf] + list(dev.values()))


@every
def test_two_outputs_overlapping_by_one_element_are_refused(torch_cuda, kind, dtype, E):
    torch = torch_cuda
    expr = _expr(kind, dtype, b=2)
    dev = {nm: torch.from_numpy(a.astype(dtype)).cuda() for nm, a in _host(expr, E, 3).items()}
    shape = _out_shape(expr, E)
    buf, out0, out1 = _views(torch, dtype, shape, shape, 1)
    buf.fill_(float("nan"))
    _refused(torch, expr, dev, {"_fe_out": out0, "_fe_out_0": out1}, ("_fe_out", "_fe_out_0"), list(dev.values()))
    assert bool(torch.isnan(buf).all())
    _refused(torch, expr, dev, {"_fe_out": out0, "_fe_out_0": out0}, ("_fe_out", "_fe_out_0"), list(dev.values()))
    assert bool(torch.isnan(buf).all())


@every
def test_touching_views_are_accepted_and_exact(torch_cuda, kind, dtype, E):
    """The output ends exactly where the operator begins, and the other way round: no shared byte, so it runs."""
    torch = torch_cuda
    expr = _expr(kind, dtype)
    host = _host(expr, E, 4)
    ref = _reference(torch, expr, host, dtype)
    for out_first in (False, True):
        dev = {nm: torch.from_numpy(a.astype(dtype)).cuda() for nm, a in host.items()}
        d_shape, out_shape = tuple(host["D"].shape), _out_shape(expr, E)
        if out_first:
            buf, out, view = _views(torch, dtype, out_shape, d_shape, 0)
        else:
            buf, view, out = _views(torch, dtype, d_shape, out_shape, 0)
        assert out.data_ptr() + out.numel() * out.element_size() == view.data_ptr() if out_first else \
            view.data_ptr() + view.numel() * view.element_size() == out.data_ptr()
        view.copy_(dev["D"])
        dev["D"] = view
        out.fill_(float("nan"))
        got = f.evaluate(expr, 0, dev, out_dict={"_fe_out": out}, wait=True)["_fe_out"]
        assert got.data_ptr() == out.data_ptr()
        assert torch.equal(got, ref), (kind, dtype, E, out_first)
        assert torch.equal(view, torch.from_numpy(host["D"].astype(dtype)).cuda())


def test_zero_size_arrays_overlap_nothing(torch_cuda):
    torch = torch_cuda
    expr = _expr("mass", "float64")
    dev = {nm: torch.from_numpy(a.astype("float64")).cuda() for nm, a in _host(expr, 0, 5).items()}
    op = f.bind_operator([(expr, dev)], 0, out_dicts=[{"_fe_out": dev["u"]}])      # bound, not refused (nothing to launch)
    assert tuple(op.outputs[0]["_fe_out"].shape) == (0, NP)


@pytest.mark.parametrize("subs,shapes,transform", [
    ("xre,rij,ej->xie", ((3, 3, "E"), (3, NP, NP), ("E", NP)), None),          # outside the families: the generic kernel
    ("xre,rij,ej->xie", ((3, 3, "E"), (3, NP, NP), ("E", NP)), "generic"),
    ("ei,ij->ej", (("E", NP), (NP, NP)), "contraction"),
    ("ei,ei->i", (("E", NP), ("E", NP)), "reduction"),
])
def test_other_kernels_refuse_an_aliased_output(torch_cuda, subs, shapes, transform):
    torch = torch_cuda
    E = 37
    names = ["A", "B", "C"][:len(shapes)]
    expr = f.einsum(subs, *[f.array(nm, s, "float64") for nm, s in zip(names, shapes)])
    rng = np.random.default_rng(6)
    dev = {nm: torch.from_numpy(rng.integers(-2, 3, size=_concrete(s, E)).astype("float64")).cuda()
           for nm, s in zip(names, shapes)}
    victim = names[-1]                                  # the output begins on the last entry of the last operand
    buf, view, out = _views(torch, "float64", tuple(dev[victim].shape), _out_shape(expr, E), 1)
    view.copy_(dev[victim])
    dev[victim] = view
    _refused(torch, expr, dev, {"_fe_out": out}, ("_fe_out", victim), [buf] + list(dev.values()), transform)


def test_operator_stage_that_writes_what_it_reads_is_refused(torch_cuda):
    torch = torch_cuda
    E = 100
    grad, mass = _expr("grad", "float64"), _expr("mass", "float64")
    gdev = {nm: torch.from_numpy(a.astype("float64")).cuda() for nm, a in _host(grad, E, 7).items()}
    mdev = {nm: torch.from_numpy(a.astype("float64")).cuda() for nm, a in _host(mass, E, 8).items()}
    before = [t.clone() for t in list(gdev.values()) + list(mdev.values())]
    for call in (f.bind_operator, f.evaluate_operator):
        for fuse in (True, False):
            with pytest.raises(InvalidParameterError, match="'u'"):
                call([(grad, gdev), (mass, mdev)], 0, out_dicts=[None, {"_fe_out": mdev["u"]}], fuse=fuse)
    torch.cuda.synchronize()
    for t, b in zip(list(gdev.values()) + list(mdev.values()), before):
        assert torch.equal(t, b)


@pytest.mark.parametrize("E", [17, 1003])
def test_laplacian_staging_still_runs_as_two_launches_and_is_exact(torch_cuda, E):
    """grad, then div OF that gradient: stage 2 reads what stage 1 writes -- legal across stages, never one launch."""
    torch = torch_cuda
    grad, div = _expr("grad", "float64"), _expr("div", "float64")
    host = _host(grad, E, 9)
    dev = {nm: torch.from_numpy(a.astype("float64")).cuda() for nm, a in host.items()}
    g = torch.full((3, E, NP), float("nan"), dtype=torch.float64, device="cuda")
    stages = [(grad, dev), (div, {"J": dev["J"], "D": dev["D"], "u": g})]
    op = f.bind_operator(stages, 0, out_dicts=[{"_fe_out": g}, None], fuse=True)
    assert op.entry_points == ("fe_grad", "fe_div")
    outs = f.evaluate_operator(stages, 0, out_dicts=[{"_fe_out": g}, None], fuse=True, wait=True)
    gref = np.einsum("xre,rij,ej->xei", host["J"], host["D"], host["u"])
    lref = np.einsum("xre,rij,xej->ei", host["J"], host["D"], gref)
    assert torch.equal(g, torch.from_numpy(gref.astype("float64")).cuda())
    assert torch.equal(outs[1]["_fe_out"], torch.from_numpy(lref.astype("float64")).cuda())
