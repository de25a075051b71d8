"""The einsums whose gradients the autograd tests check (tests/test_autograd_cpu.py, tests/test_gpu_autograd.py), and
host-side helpers: random inputs, the torch.einsum autograd reference and the numpy evaluation of the adjoint einsums."""

import numpy as np

import feinsum_amd as f
from feinsum_amd.autograd import adjoint_terms, expand_to_operand, output_grad_name

# tetrahedra p = 1..4 and triangles p = 1..5: (ndim, Np, nf, Nfp)
TETS = {1: (3, 4, 4, 3), 2: (3, 10, 4, 6), 3: (3, 20, 4, 10), 4: (3, 35, 4, 15)}
TRIS = {1: (2, 3, 3, 2), 2: (2, 6, 3, 3), 3: (2, 10, 3, 4), 4: (2, 15, 3, 5), 5: (2, 21, 3, 6)}
FM_LAYOUTS = [(j, r) for j in ("ef", "fe") for r in ("fij", "ifj", "fji", "jfi")]


def grad(nd, Np, d="rij"):
    return f.einsum(f"xre,{d},ej->xei", f.array("J", (nd, nd, "E")), f.array("D", (nd, Np, Np)),
                    f.array("u", ("E", Np)))


def div(nd, Np, d="rij"):
    return f.einsum(f"xre,{d},xej->ei", f.array("J", (nd, nd, "E")), f.array("D", (nd, Np, Np)),
                    f.array("u", (nd, "E", Np)))


def divcomp(nd, Np, j="re", d="rij"):
    jshape = (nd, "E") if j == "re" else ("E", nd)
    return f.einsum(f"{j},{d},ej->ei", f.array("J", jshape), f.array("D", (nd, Np, Np)), f.array("u", ("E", Np)))


def matapply(Np, d="ij", with_j=True):
    if with_j:
        return f.einsum(f"e,{d},ej->ei", f.array("J", ("E",)), f.array("D", (Np, Np)), f.array("u", ("E", Np)))
    return f.einsum(f"{d},ej->ei", f.array("D", (Np, Np)), f.array("u", ("E", Np)))


def face_mass(Np, nf, Nfp, b=1, jl="ef", rl="fij"):
    jshape = ("E", nf) if jl == "ef" else (nf, "E")
    rshape = {"fij": (nf, Np, Nfp), "ifj": (Np, nf, Nfp), "fji": (nf, Nfp, Np), "jfi": (Nfp, nf, Np)}[rl]
    return f.batched_einsum(f"{jl},{rl},fej->ei",
                            [[f.array("J", jshape), f.array("R", rshape), f.array(f"v{k}", (nf, "E", Nfp))]
                             for k in range(b)])


def dg_cases(orders=None):
    """(name, einsum) of every DG family x layout at the given orders ({"tet": [...], "tri": [...]})."""
    orders = orders or {"tet": [1, 2, 3, 4], "tri": [1, 2, 3, 4, 5]}
    out = []
    for kind, table in (("tet", TETS), ("tri", TRIS)):
        for p in orders.get(kind, []):
            nd, Np, nf, Nfp = table[p]
            tag = f"{kind}{p}"
            for d in ("rij", "rji"):
                out.append((f"grad_{d}_{tag}", grad(nd, Np, d)))
                out.append((f"div_{d}_{tag}", div(nd, Np, d)))
                for j in ("re", "er"):
                    out.append((f"divcomp_{j}_{d}_{tag}", divcomp(nd, Np, j, d)))
            for d in ("ij", "ji"):
                out.append((f"matapply_{d}_{tag}", matapply(Np, d)))
            out.append((f"matapply_noj_{tag}", matapply(Np, with_j=False)))
            for jl, rl in FM_LAYOUTS:
                for b in (1, 4):
                    out.append((f"facemass_{jl}_{rl}_b{b}_{tag}", face_mass(Np, nf, Nfp, b, jl, rl)))
    return out


def other_cases():
    return [
        ("dot_twice", f.einsum("ei,ei->", f.array("u", ("E", 5)), f.array("u", ("E", 5)))),
        ("quadratic_form", f.einsum("e,ij,ei,ej->", f.array("w", ("E",)), f.array("A", (4, 4)),
                                     f.array("x", ("E", 4)), f.array("y", ("E", 4)))),
        ("gemm", f.einsum("ij,jk->ik", f.array("A", ("E", 6)), f.array("B", (6, 7)))),
        ("rowsum", f.einsum("ij->i", f.array("A", ("E", 6)))),
        ("mixed", f.einsum("ij,j->i", f.array("A", ("E", 6), "float32"), f.array("x", (6,)))),
    ]


def concrete(shape, E):
    return tuple(E if isinstance(d, f.SizeParam) else int(d) for d in shape)


def random_inputs(einsum, E, seed=0, integer=False):
    rng = np.random.default_rng(seed)
    out = {}
    for name in sorted(einsum.all_args):
        shape = concrete(einsum.arg_to_shape[name], E)
        x = rng.integers(-3, 4, size=shape).astype(np.float64) if integer else rng.standard_normal(shape)
        out[name] = x.astype(einsum.arg_to_dtype[name])
    return out


def random_output_grads(einsum, E, seed=1, integer=False):
    rng = np.random.default_rng(seed)
    shape = concrete(einsum.shape, E)
    out = {}
    for k, name in enumerate(einsum.output_names):
        x = rng.integers(-3, 4, size=shape).astype(np.float64) if integer else rng.standard_normal(shape)
        out[name] = np.asarray(x, dtype=np.result_type(*[a.dtype for a in einsum.args[k]]))
    return out


def torch_reference_grads(einsum, inputs, out_grads):
    """Gradients of sum_k <g_k, out_k> by torch.einsum autograd, on the CPU in float64."""
    import torch

    leaves = {n: torch.tensor(np.asarray(v, dtype=np.float64), requires_grad=True) for n, v in inputs.items()}
    sub = einsum.get_subscripts().replace(" ", "")
    loss = 0
    for k, row in enumerate(einsum.args):
        y = torch.einsum(sub, *[leaves[a.name] for a in row])
        loss = loss + (y * torch.tensor(np.asarray(out_grads[einsum.output_names[k]], dtype=np.float64))).sum()
    grads = torch.autograd.grad(loss, [leaves[n] for n in sorted(leaves)])
    return {n: g.numpy() for n, g in zip(sorted(leaves), grads)}


def numpy_adjoint_grad(einsum, wrt, inputs, out_grads):
    """The vector-Jacobian product for *wrt* as the sum of its adjoint einsums, each evaluated with numpy in float64."""
    arrays = {n: np.asarray(v, dtype=np.float64) for n, v in inputs.items()}
    for name, g in out_grads.items():
        arrays[output_grad_name(name)] = np.asarray(g, dtype=np.float64)
    shape = arrays[wrt].shape
    total = np.zeros(shape)
    for term in adjoint_terms(einsum, wrt):
        sub = term.einsum.get_subscripts().replace(" ", "")
        for row in term.einsum.args:
            val = np.einsum(sub, *[arrays[a.name] for a in row])
            total = total + expand_to_operand(val, term.einsum.out_idx_set, term.wrt_subscripts, shape)
    return total


def numpy_forward(einsum, inputs):
    sub = einsum.get_subscripts().replace(" ", "")
    return {name: np.einsum(sub, *[np.asarray(inputs[a.name], dtype=np.float64) for a in row])
            for name, row in zip(einsum.output_names, einsum.args)}
