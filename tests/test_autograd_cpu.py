"""Adjoint einsums on the host: their numpy evaluation equals torch.einsum autograd, they satisfy the linearity
identity, and they route to the kernels DESIGN.md section 3l names -- without changing what match_family matches."""

import numpy as np
import pytest

import feinsum_amd as f
from feinsum_amd.autograd import adjoint_einsums, adjoint_terms, output_grad_name
from feinsum_amd.family import (ADJ_FACEMASS_J, ADJ_FACEMASS_V, ADJ_GEOM, FAMILY_DIV, FAMILY_GRAD, OP_TRANSPOSED,
                                match_adjoint_family, match_family)
import autograd_cases as C

E = 7
ALL = C.dg_cases({"tet": [1, 2], "tri": [1, 2]}) + C.other_cases()


def _rel(a, b):
    scale = max(np.abs(b).max(), 1e-300)
    return np.abs(np.asarray(a, dtype=np.float64) - b).max() / scale


@pytest.mark.parametrize("name,einsum", ALL, ids=[n for n, _ in ALL])
def test_adjoint_einsums_match_torch_autograd(name, einsum):
    inputs = C.random_inputs(einsum, E)
    gbar = C.random_output_grads(einsum, E)
    ref = C.torch_reference_grads(einsum, inputs, gbar)
    for wrt in sorted(einsum.all_args):
        got = C.numpy_adjoint_grad(einsum, wrt, inputs, gbar)
        assert got.shape == ref[wrt].shape
        assert _rel(got, ref[wrt]) <= 1e-13, (name, wrt)


@pytest.mark.parametrize("name,einsum", ALL, ids=[n for n, _ in ALL])
def test_linearity_identity(name, einsum):
    inputs = C.random_inputs(einsum, E, seed=3)
    gbar = C.random_output_grads(einsum, E, seed=4)
    rng = np.random.default_rng(5)
    base = C.numpy_forward(einsum, inputs)
    for wrt in sorted(einsum.all_args):
        delta = rng.standard_normal(np.shape(inputs[wrt]))
        moved = dict(inputs, **{wrt: np.asarray(inputs[wrt], dtype=np.float64) + delta})
        after = C.numpy_forward(einsum, moved)
        lhs = sum(float(np.sum(gbar[n] * (after[n] - base[n]))) for n in einsum.output_names)
        rhs = float(np.sum(C.numpy_adjoint_grad(einsum, wrt, inputs, gbar) * delta))
        # the forward is linear in each operand only: a repeated operand adds a term quadratic in delta
        n_occ = sum(a.name == wrt for row in einsum.args for a in row) // einsum.b
        if n_occ == 1:
            assert abs(lhs - rhs) <= 1e-10 * max(1.0, abs(lhs)), (name, wrt)


def test_one_term_per_occurrence_and_reserved_names():
    ein = f.einsum("ei,ei->", f.array("u", ("E", 5)), f.array("u", ("E", 5)))
    terms = adjoint_terms(ein, "u")
    assert [t.einsum.get_subscripts() for t in terms] == ["ei, -> ei", "ei, -> ei"]
    assert terms[0].einsum.arg_to_shape[output_grad_name("_fe_out")] == ()
    fm = C.face_mass(35, 4, 15, b=4)
    (jterm,) = adjoint_einsums(fm, "J")
    assert jterm.b == 4 and jterm.get_subscripts() == "fij,fej,ei -> ef"
    assert len(adjoint_einsums(fm, "v2")) == 1 and adjoint_einsums(fm, "v2")[0].b == 1
    bad = f.einsum("ij,j->i", f.array("_fe_grad_x", (3, 3)), f.array("y", (3,)))
    with pytest.raises(ValueError, match="reserved"):
        adjoint_einsums(bad, "y")


def test_summed_index_is_broadcast():
    ein = f.einsum("ij->i", f.array("A", ("E", 6)))
    (term,) = adjoint_terms(ein, "A")
    assert term.einsum.out_idx_set == ("i",) and term.wrt_subscripts == ("i", "j")


def test_repeated_index_raises_only_for_that_operand():
    ein = f.einsum("ii,i->i", f.array("A", (4, 4)), f.array("x", (4,)))
    with pytest.raises(NotImplementedError, match="'A'"):
        adjoint_einsums(ein, "A")
    (term,) = adjoint_einsums(ein, "x")      # x itself has no repeated index
    assert term.get_subscripts() == "ii,i -> i"
    with pytest.raises(NotImplementedError, match="'A'"):
        adjoint_einsums(f.einsum("ii->i", f.array("A", (4, 4))), "A")


def test_routing_of_the_adjoint_terms():
    # grad's u-adjoint is div with the transposed operator
    (t,) = adjoint_einsums(C.grad(3, 35), "u")
    plan = match_family(t)
    assert plan is not None and plan.family == FAMILY_DIV and plan.layout_flags == OP_TRANSPOSED
    # div's u-adjoint is grad with the transposed operator
    (t,) = adjoint_einsums(C.div(3, 35), "u")
    plan = match_family(t)
    assert plan is not None and plan.family == FAMILY_GRAD and plan.layout_flags == OP_TRANSPOSED
    # the J-adjoints: the geometric-factor adjoint kernel, in every family and layout, and not a family einsum
    for ein in (C.grad(3, 35), C.grad(3, 35, "rji"), C.div(3, 35), C.div(2, 21, "rji"), C.divcomp(3, 20),
                C.divcomp(2, 6, "er", "rji"), C.matapply(10), C.matapply(15, "ji")):
        (t,) = adjoint_einsums(ein, "J")
        plan = match_adjoint_family(t)
        assert plan is not None and plan.kind == ADJ_GEOM, t.get_subscripts()
        assert match_family(t) is None
    # face-mass: v- and J-adjoints on the face-mass adjoint kernel
    for jl, rl in C.FM_LAYOUTS:
        fm = C.face_mass(35, 4, 15, 4, jl, rl)
        (tv,) = adjoint_einsums(fm, "v1")
        (tj,) = adjoint_einsums(fm, "J")
        pv, pj = match_adjoint_family(tv), match_adjoint_family(tj)
        assert pv is not None and pv.kind == ADJ_FACEMASS_V
        assert pj is not None and pj.kind == ADJ_FACEMASS_J
        assert match_family(tv) is None and match_family(tj) is None
    # p = 5 tetrahedra are not compiled: those terms stay on the existing routes
    (t,) = adjoint_einsums(C.grad(3, 56), "J")
    assert match_adjoint_family(t) is None


def test_transform_adjoint_refuses_other_shapes():
    from feinsum_amd.measure import launch_kind

    with pytest.raises(NotImplementedError, match="adjoint"):
        launch_kind(C.grad(3, 35), "adjoint", {"E": 10})
    (t,) = adjoint_einsums(C.grad(3, 35), "J")
    assert launch_kind(t, "adjoint", {"E": 10}) == "adjoint"
    assert launch_kind(t, None, {"E": 10}) != "adjoint"      # "auto" keeps its kernels


def test_adjoint_kernels_argument_checks_without_gpu():
    from feinsum_amd import _hip

    with pytest.raises(NotImplementedError, match="Np = 56"):
        _hip.geomadj(8, 8, 8, 8, 10, 3, 3, 56, (1, 1, 1))
    with pytest.raises(NotImplementedError, match="not compiled"):
        _hip.facemass_adj(8, 8, [8], None, [8], None, 10, 56, 4, 21)
    with pytest.raises(f.InvalidParameterError, match="neither"):
        _hip.facemass_adj(8, 8, [8], None, None, None, 10, 35, 4, 15)
    _hip.geomadj(0, 0, 0, 0, 0, 3, 3, 35, (1, 1, 1))           # E == 0: no launch
    _hip.facemass_adj(0, 0, [0], None, [0], None, 0, 35, 4, 15)
