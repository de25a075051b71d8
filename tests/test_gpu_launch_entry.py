"""``fe_launch`` against the named entry points on the device: every route a bound DG launch used to pick in Python, once
through the entry point it named and once through the pack, on the same arrays -- bitwise the same outputs and the same
``fe_last_launch_info``.

Shapes are the smallest that reach the tile loop, the remainder behind the last tile and the sub-tile path: tetrahedra
p = 1 (wave tile of grad and div: 80 elements) at E = 165 and E = 7, p = 4 (16 elements) at E = 37; triangles p = 1 (128
elements) at E = 265; float32 at two wave tiles of its geometry plus 4 (a multiple of 4, which the float32 matrix-core
kernels need), and at E = 37 for the tiled fallback."""

import ctypes

import pytest
import torch

from feinsum_amd import _hip
from feinsum_amd.family import (FAMILY_DIV, FAMILY_DIVCOMP, FAMILY_FACEMASS, FAMILY_GRAD, FAMILY_GRADPLANES,
                                FAMILY_MATAPPLY)

pytestmark = pytest.mark.gpu

F32, ACC = _hip.FAMILY_F32, _hip.FAMILY_ACC
NF = 4
TETS = [(4, 3, 165), (4, 3, 7), (35, 15, 37)]          # (Np, Nfp, E)
ALPHA, BETA = 0.75, -1.5


class Arrays:
    """Device arrays of one case, drawn once; ``ptrs`` builds host tables of device pointers and keeps them alive."""

    def __init__(self, dtype=torch.float64, seed=0):
        self.gen = torch.Generator(device="cuda").manual_seed(seed)
        self.dtype, self.keep, self.outs = dtype, [], []

    def rand(self, *shape):
        t = torch.rand(shape, dtype=self.dtype, device="cuda", generator=self.gen) - 0.5
        self.keep.append(t)
        return t

    def out(self, *shape):
        t = self.rand(*shape)        # what an accumulating launch adds onto; everyone else overwrites it
        self.outs.append(t)
        return t

    def ptrs(self, tensors):
        arr = _hip._ptr_array([t.data_ptr() if t is not None else None for t in tensors])
        self.keep.append(arr)
        return arr


def _pack(E, Np, b, **fields):
    pack = _hip.ArgPack()
    pack.E, pack.Np, pack.b, pack.ndim = E, Np, b, 3
    for key, value in fields.items():
        setattr(pack, key, value)
    return pack


def _same_through_both(arrays, named, family, pack):
    """Launch through *named* (a call of the entry point the Python dispatcher used to pick), then through ``fe_launch``
    with *family* and *pack*, each time from the same initial outputs."""
    lib = _hip.load_library()
    stream = torch.cuda.current_stream().cuda_stream
    initial = [t.clone() for t in arrays.outs]
    got = []
    for call in (named, lambda lib, stream: lib.fe_launch(family, ctypes.byref(pack), stream)):
        for t, t0 in zip(arrays.outs, initial):
            t.copy_(t0)
        rc = call(lib, stream)
        if isinstance(rc, int):
            _hip.check(rc)
        torch.cuda.synchronize()
        got.append(([t.clone() for t in arrays.outs], _hip.last_launch_info()))
    (outs_named, info_named), (outs_pack, info_pack) = got
    for k, (a, b, t0) in enumerate(zip(outs_named, outs_pack, initial)):
        ints = torch.int64 if a.dtype == torch.float64 else torch.int32
        assert torch.equal(a.view(ints), b.view(ints)), f"output {k} differs between the entry point and fe_launch"
        assert not torch.equal(a.view(ints), t0.view(ints)), f"output {k} was not written"
        assert torch.isfinite(a).all()
    assert info_named == info_pack
    return info_pack


def _geometry(a, Np, E, nd=3):
    return a.rand(nd, nd, E), a.rand(nd, Np, Np)


def _prepare(a, family, op, Np, nf=0, Nfp=0):
    buf = torch.empty(_hip.PREPARED_OPERATOR_BYTES, dtype=torch.uint8, device="cuda")
    a.keep.append(buf)
    _hip.prepare_operator(family, op.data_ptr(), Np, nf, Nfp, 0, buf.data_ptr(), torch.cuda.current_stream().cuda_stream)
    return buf.data_ptr()


@pytest.mark.parametrize("Np,Nfp,E", TETS)
@pytest.mark.parametrize("family", [FAMILY_GRAD, FAMILY_DIV], ids=["grad", "div"])
@pytest.mark.parametrize("b,prepared", [(1, False), (2, False), (1, True), (2, True)],
                         ids=["b1", "b2", "b1-prepared", "b2-prepared"])
def test_grad_and_div_of_tetrahedra(family, b, prepared, Np, Nfp, E):
    a = Arrays()
    J, D = _geometry(a, Np, E)
    grad = family == FAMILY_GRAD
    u = [a.rand(E, Np) if grad else a.rand(3, E, Np) for _ in range(b)]
    out = [a.out(3, E, Np) if grad else a.out(E, Np) for _ in range(b)]
    v, outs = a.ptrs(u), a.ptrs(out)
    prep = _prepare(a, family, D, Np) if prepared else None
    args = (J.data_ptr(), D.data_ptr())
    if prepared:
        entry = "fe_grad3d_prepared_f64" if grad else "fe_div3d_prepared_f64"
        named = lambda lib, s: getattr(lib, entry)(*args, prep, v, outs, E, Np, b, 0, 0, s)     # noqa: E731
    else:
        entry = "fe_grad_f64" if grad else "fe_div_f64"
        named = lambda lib, s: getattr(lib, entry)(*args, v, outs, E, 3, Np, b, 0, 0, s)        # noqa: E731
    pack = _pack(E, Np, b, J=args[0], D=args[1], u=u[0].data_ptr(), out=out[0].data_ptr(), v=v, outs=outs, prepared=prep)
    info = _same_through_both(a, named, family, pack)
    assert bool(info) == (E >= 16 * (5 if Np == 4 else 1))     # a full wave tile: the matrix-core kernel reports itself
    if prepared:
        _hip.release_prepared(prep)


@pytest.mark.parametrize("Np,Nfp,E", TETS)
@pytest.mark.parametrize("family", [FAMILY_GRAD, FAMILY_DIV], ids=["grad", "div"])
def test_accumulating_grad_and_div(family, Np, Nfp, E):
    a = Arrays()
    J, D = _geometry(a, Np, E)
    grad = family == FAMILY_GRAD
    u = [a.rand(E, Np) if grad else a.rand(3, E, Np) for _ in range(2)]
    out = [a.out(3, E, Np) if grad else a.out(E, Np) for _ in range(2)]      # pre-filled: beta != 0 reads them
    v, outs = a.ptrs(u), a.ptrs(out)

    def named(lib, s):     # the loop the Python dispatcher ran: one accumulating launch per field
        entry = lib.fe_grad3d_acc_f64 if grad else lib.fe_div3d_acc_f64
        for k in range(2):
            _hip.check(entry(J.data_ptr(), D.data_ptr(), u[k].data_ptr(), out[k].data_ptr(), E, Np, 0, ALPHA, BETA, s))

    pack = _pack(E, Np, 2, J=J.data_ptr(), D=D.data_ptr(), v=v, outs=outs, alpha=ALPHA, beta=BETA)
    _same_through_both(a, named, family | ACC, pack)


@pytest.mark.parametrize("Np,Nfp,E", TETS)
@pytest.mark.parametrize("route", ["plain", "prepared", "accumulating"])
def test_face_mass(route, Np, Nfp, E):
    a = Arrays()
    J, R = a.rand(E, NF), a.rand(NF, Np, Nfp)
    fields = [a.rand(NF, E, Nfp) for _ in range(2)]
    out = [a.out(E, Np) for _ in range(2)]
    v, outs = a.ptrs(fields), a.ptrs(out)
    prep = _prepare(a, FAMILY_FACEMASS, R, Np, NF, Nfp) if route == "prepared" else None
    args = (J.data_ptr(), R.data_ptr())
    if route == "accumulating":
        named = lambda lib, s: lib.fe_facemass_acc_f64(*args, v, outs, E, Np, NF, Nfp, 2, 0, ALPHA, BETA, s)   # noqa: E731
    else:
        named = lambda lib, s: lib.fe_facemass_prepared_f64(*args, prep, v, outs, E, Np, NF, Nfp, 2, 0, 0, s)  # noqa: E731
    pack = _pack(E, Np, 2, J=args[0], D=args[1], v=v, outs=outs, nf=NF, Nfp=Nfp, prepared=prep, alpha=ALPHA, beta=BETA)
    _same_through_both(a, named, FAMILY_FACEMASS | (ACC if route == "accumulating" else 0), pack)
    if prep:
        _hip.release_prepared(prep)


@pytest.mark.parametrize("Np,Nfp,E", TETS)
def test_grad_planes(Np, Nfp, E):
    a = Arrays()
    J3, D = [a.rand(3, E) for _ in range(3)], a.rand(3, Np, Np)
    u = [a.rand(E, Np) for _ in range(2)]
    planes = [a.out(E, Np) for _ in range(6)]
    j3, v, outs = a.ptrs(J3), a.ptrs(u), a.ptrs(planes)
    named = lambda lib, s: lib.fe_gradplanes3d_f64(j3, D.data_ptr(), v, outs, E, Np, 2, 0, 0, s)   # noqa: E731
    _same_through_both(a, named, FAMILY_GRADPLANES, _pack(E, Np, 2, D=D.data_ptr(), j3=j3, v=v, outs=outs))


@pytest.mark.parametrize("Np,Nfp,E", TETS)
@pytest.mark.parametrize("with_j", [True, False], ids=["J", "no-J"])
def test_matapply(with_j, Np, Nfp, E):
    a = Arrays()
    J, D = (a.rand(E).data_ptr() if with_j else None), a.rand(Np, Np)
    u, out = [a.rand(E, Np) for _ in range(2)], [a.out(E, Np) for _ in range(2)]
    v, outs = a.ptrs(u), a.ptrs(out)
    named = lambda lib, s: lib.fe_matapply_f64(J, D.data_ptr(), v, outs, E, Np, 2, 0, 0, s)   # noqa: E731
    _same_through_both(a, named, FAMILY_MATAPPLY, _pack(E, Np, 2, J=J, D=D.data_ptr(), v=v, outs=outs))


@pytest.mark.parametrize("nd,Np,E", [(3, 4, 165), (3, 4, 7), (3, 35, 37), (2, 3, 265)],
                         ids=["p1-E165", "p1-E7", "p4-E37", "triangles-E265"])
def test_div_component(nd, Np, E):
    a = Arrays()
    J, D, u, out = a.rand(nd, E), a.rand(nd, Np, Np), a.rand(E, Np), a.out(E, Np)
    args = (J.data_ptr(), D.data_ptr(), u.data_ptr(), out.data_ptr())
    named = lambda lib, s: lib.fe_divcomp_f64(*args, E, nd, Np, 0, 0, s)   # noqa: E731
    pack = _pack(E, Np, 1, J=args[0], D=args[1], u=args[2], out=args[3], ndim=nd)
    _same_through_both(a, named, FAMILY_DIVCOMP, pack)


@pytest.mark.parametrize("family", [FAMILY_GRAD, FAMILY_DIV], ids=["grad", "div"])
def test_grad_and_div_of_triangles(family):
    Np, E, b = 3, 2 * 128 + 9, 2            # two wave tiles of 16 * 8 elements and a ragged rest
    a = Arrays()
    J, D = _geometry(a, Np, E, nd=2)
    grad = family == FAMILY_GRAD
    u = [a.rand(E, Np) if grad else a.rand(2, E, Np) for _ in range(b)]
    out = [a.out(2, E, Np) if grad else a.out(E, Np) for _ in range(b)]
    v, outs = a.ptrs(u), a.ptrs(out)
    entry = "fe_grad_f64" if grad else "fe_div_f64"
    named = lambda lib, s: getattr(lib, entry)(J.data_ptr(), D.data_ptr(), v, outs, E, 2, Np, b, 0, 0, s)   # noqa: E731
    pack = _pack(E, Np, b, J=J.data_ptr(), D=D.data_ptr(), v=v, outs=outs, ndim=2)
    assert _same_through_both(a, named, family, pack)


#: float32: (family, Np, Nfp, elements per wave tile of the float32 geometry: 16 M)
F32_TILES = [(FAMILY_GRAD, 4, 3, 128), (FAMILY_GRAD, 35, 15, 16), (FAMILY_DIV, 4, 3, 80), (FAMILY_DIV, 35, 15, 16),
             (FAMILY_FACEMASS, 4, 3, 64), (FAMILY_FACEMASS, 35, 15, 16)]
F32_CASES = [(fam, Np, Nfp, 2 * tel + 4, 0) for fam, Np, Nfp, tel in F32_TILES] \
    + [(FAMILY_GRAD, 35, 15, 37, 0), (FAMILY_DIV, 35, 15, 36, _hip.VARIANT_TILED)]     # the tiled kernel in float
_NAMES = {FAMILY_GRAD: "grad", FAMILY_DIV: "div", FAMILY_FACEMASS: "facemass"}


@pytest.mark.parametrize("family,Np,Nfp,E,variant", F32_CASES,
                         ids=[f"{_NAMES[c[0]]}-Np{c[1]}-E{c[3]}-v{c[4]}" for c in F32_CASES])
def test_float32(family, Np, Nfp, E, variant):
    a = Arrays(torch.float32)
    b = 2
    if family == FAMILY_FACEMASS:
        J, D = a.rand(E, NF), a.rand(NF, Np, Nfp)
        u, out = [a.rand(NF, E, Nfp) for _ in range(b)], [a.out(E, Np) for _ in range(b)]
    else:
        J, D = _geometry(a, Np, E)
        grad = family == FAMILY_GRAD
        u = [a.rand(E, Np) if grad else a.rand(3, E, Np) for _ in range(b)]
        out = [a.out(3, E, Np) if grad else a.out(E, Np) for _ in range(b)]
    v, outs = a.ptrs(u), a.ptrs(out)
    pack = _pack(E, Np, b, J=J.data_ptr(), D=D.data_ptr(), u=u[0].data_ptr(), out=out[0].data_ptr(), v=v, outs=outs,
                 nf=NF if family == FAMILY_FACEMASS else 0, Nfp=Nfp if family == FAMILY_FACEMASS else 0, variant=variant)
    named = lambda lib, s: lib.fe_launch_f32(family, ctypes.byref(pack), s)   # noqa: E731
    _same_through_both(a, named, family | F32, pack)
