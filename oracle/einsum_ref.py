"""
References for random einsums outside the DG families.  TEST INFRASTRUCTURE ONLY: imported by tests/ and
tools/fuzz_einsum.py, never by feinsum_amd/.

Two references, for two kinds of data.

Exact data (:func:`exact_operands`, :func:`exact_reference`)
    Operand p holds ``m * 2**s_p``: ``m`` a signed integer of at most ``bits[p]`` bits, ``s_p`` one power-of-two scale
    per operand.  Every term of the einsum is then an integer multiple of ``2**sum(s_p)``, and :func:`exact_bits`
    picks the bits so that the absolute sum of all terms of an output entry fits the significand of the dtype the
    kernel computes in (every intermediate of a schedule included).  Any partial sum, in any order, is then exact; the
    kernel result must be *bitwise* the reference, which is the einsum of the integer mantissas in int64, scaled back.
    A missing, duplicated or misindexed term, a lost sign or a float32 accumulator in a float64 path changes it.

Error-bounded reference (:func:`bounded_reference`, :func:`bound_violations`)
    For continuous signed data: ``ref`` is the einsum of the operands in ``np.longdouble``, ``absref`` the einsum of
    their absolute values, and every entry must satisfy ``|got - ref| <= gamma(n, u) * absref`` with
    ``gamma(n, u) = n u / (1 - n u)`` (the classical bound of a sum of products evaluated in any order),
    ``n = operands - 1 + summed points per entry + schedule steps``.
"""

from __future__ import annotations

import math
from typing import List, Mapping, Optional, Sequence, Tuple

import numpy as np

#: significand bits of each compute dtype (the implicit bit included)
SIGNIFICAND = {np.dtype("float64"): 53, np.dtype("float32"): 24}
U64, U32 = 2.0 ** -53, 2.0 ** -24


def _split(subscripts: str) -> Tuple[List[str], str]:
    lhs, rhs = subscripts.replace(" ", "").split("->")
    return lhs.split(","), rhs


def summed_points(subscripts: str, extent: Mapping[str, int]) -> int:
    """Terms per output entry: the product of the extents of the indices that are not in the output."""
    ins, out = _split(subscripts)
    n = 1
    for c in dict.fromkeys("".join(ins)):
        if c not in out:
            n *= int(extent[c])
    return n


def compute_significand(dtypes: Sequence, f32_step: bool = False) -> int:
    """Bits every partial sum must fit: 24 when the einsum computes in float32, or when a schedule can meet float32
    operands only in one of its steps (*f32_step*: the rule of ``measure.validation_dtype``), else 53."""
    dt = np.result_type(*[np.dtype(d) for d in dtypes])
    return 24 if (dt == np.dtype("float32") or f32_step) else 53


def exact_bits(n_ops: int, dtypes: Sequence, n_terms: int, significand: int,
               rng: np.random.Generator) -> List[int]:
    """Mantissa bits per operand: ``prod(2**b_p - 1) * n_terms <= 2**significand`` (checked with Python integers),
    float32 operands at most 24 bits, each at least 1 bit.  The budget is spent: with 53 bits the operands need more
    than 24 bits together whenever the summation length leaves room (``needs_more_than_f32``)."""
    head = max(int(n_terms), 1).bit_length()          # 2**head > n_terms
    budget = max(significand - head, n_ops)
    # a random share per operand, every operand >= 1 bit, float32 operands <= 24
    w = rng.random(n_ops) + 0.25
    bits = [max(1, int(budget * x / w.sum())) for x in w]
    for p, dt in enumerate(dtypes):
        if np.dtype(dt) == np.dtype("float32"):
            bits[p] = min(bits[p], 24)
    # hand out what rounding down left over, to operands that can take it
    spare = budget - sum(bits)
    for p in rng.permutation(n_ops):
        cap = 24 if np.dtype(dtypes[p]) == np.dtype("float32") else significand
        add = max(0, min(spare, cap - bits[p]))
        bits[p] += add
        spare -= add
    while not bits_fit(bits, n_terms, significand):   # (budget < n_ops: give back bits until it fits)
        p = int(np.argmax(bits))
        if bits[p] == 1:
            break
        bits[p] -= 1
    return bits


def bits_fit(bits: Sequence[int], n_terms: int, significand: int) -> bool:
    """Whether every partial sum of ``n_terms`` products of mantissas of these bits is exact: the largest possible
    absolute sum, ``prod(2**b - 1) * n_terms``, is at most ``2**significand`` (Python integers, no rounding)."""
    worst = max(int(n_terms), 1)
    for b in bits:
        worst *= (1 << int(b)) - 1
    return worst <= (1 << significand)


def exact_operands(shapes: Sequence[Tuple[int, ...]], dtypes: Sequence, bits: Sequence[int],
                   scales: Sequence[int], rng: np.random.Generator) -> Tuple[List[np.ndarray], List[np.ndarray]]:
    """``(mantissas int64, operands)``: operand p is ``m * 2**scales[p]`` in ``dtypes[p]``, ``|m| < 2**bits[p]``, signed.
    Half of the entries of an operand of 3 or more bits use its full width (the top bit set), so the budget is used."""
    mants, arrays = [], []
    for shape, dt, b, s in zip(shapes, dtypes, bits, scales):
        top = (1 << int(b)) - 1
        m = rng.integers(-top, top + 1, size=shape, dtype=np.int64)
        if b >= 3:
            full = rng.random(shape) < 0.5
            hi = rng.integers(1 << (int(b) - 1), top + 1, size=shape, dtype=np.int64)
            m = np.where(full, np.where(rng.random(shape) < 0.5, -hi, hi), m)
        x = np.ldexp(m.astype(np.float64), int(s)).astype(np.dtype(dt))
        assert np.array_equal(np.ldexp(x.astype(np.float64), -int(s)), m.astype(np.float64)), "operand not exact"
        mants.append(m)
        arrays.append(x)
    return mants, arrays


def exact_reference(subscripts: str, mants: Sequence[np.ndarray], scales: Sequence[int],
                    out_dtype, significand: int) -> np.ndarray:
    """The einsum of the integer mantissas in int64, scaled back by ``2**sum(scales)`` into *out_dtype*.  Asserts
    that the absolute einsum stays within ``2**significand`` (so that the int64 sum and the scaled value are exact)."""
    absum = np.einsum(subscripts, *[np.abs(m) for m in mants], optimize=False)
    assert (np.asarray(absum) <= (1 << significand)).all(), "exact-data budget exceeded"
    ints = np.asarray(np.einsum(subscripts, *mants, optimize=False), dtype=np.int64)
    return np.ldexp(ints.astype(np.float64), int(sum(scales))).astype(np.dtype(out_dtype))


def needs_more_than_f32(ref: np.ndarray) -> bool:
    """Whether some entry of a float64 result needs more than 24 significant bits (rounding it to float32 changes it)."""
    r = np.asarray(ref, dtype=np.float64)
    return bool(r.size) and bool((r.astype(np.float32).astype(np.float64) != r).any())


def bitwise_equal(got: np.ndarray, ref: np.ndarray) -> bool:
    """Same dtype, shape and bits (``-0.0`` and ``0.0`` are equal: the sums are exact, their signs of zero are not
    specified)."""
    got, ref = np.asarray(got), np.asarray(ref)
    return got.dtype == ref.dtype and got.shape == ref.shape and bool((got == ref).all())


# --------------------------------------------------------------------------
# error-bounded reference
# --------------------------------------------------------------------------

def gamma(n: int, u: float) -> float:
    nu = n * u
    assert nu < 1, "error bound undefined (n u >= 1)"
    return nu / (1 - nu)


def bound_terms(subscripts: str, extent: Mapping[str, int], n_ops: int, schedule_steps: int = 0) -> int:
    """``n`` of the bound: ``operands - 1 + summed points per entry + schedule steps``."""
    return n_ops - 1 + summed_points(subscripts, extent) + schedule_steps


def bounded_reference(subscripts: str, arrays: Sequence[np.ndarray]) -> Tuple[np.ndarray, np.ndarray]:
    """``(ref, absref)`` in ``np.longdouble``."""
    ld = [np.asarray(a).astype(np.longdouble) for a in arrays]
    ref = np.einsum(subscripts, *ld, optimize=False)
    absref = np.einsum(subscripts, *[np.abs(a) for a in ld], optimize=False)
    return np.asarray(ref), np.asarray(absref)


def bound_ratio(got: np.ndarray, ref: np.ndarray, absref: np.ndarray, n: int, u: float) -> float:
    """``max |got - ref| / (gamma(n, u) absref)`` over the entries (``inf`` where the bound is 0 and the error not; NaN
    anywhere in *got* is ``inf``).  At most 1 passes."""
    got = np.asarray(got)
    if got.shape != ref.shape:
        return math.inf
    if got.size == 0:
        return 0.0
    g = got.astype(np.longdouble)
    if not np.isfinite(g).all():
        return math.inf
    err = np.abs(g - ref)
    bound = np.longdouble(gamma(n, u)) * absref
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err == 0, np.longdouble(0), err / bound)
    return float(np.max(ratio))


def bound_violations(got: np.ndarray, ref: np.ndarray, absref: np.ndarray, n: int, u: float) -> int:
    """Entries where ``|got - ref| > gamma(n, u) absref`` (every entry when the shapes differ)."""
    got = np.asarray(got)
    if got.shape != ref.shape:
        return max(int(ref.size), 1)
    g = got.astype(np.longdouble)
    bad = ~np.isfinite(g) | (np.abs(g - ref) > np.longdouble(gamma(n, u)) * absref)
    return int(bad.sum())


def unit_roundoff(dtypes: Sequence, n_ops: int) -> float:
    """``u`` of the bound: 2^-24 when the einsum computes in float32 or when a float64 result of three or more
    operands has two or more float32 operands (a schedule step can then be float32: ``measure.validation_dtype``), else
    2^-53."""
    dts = [np.dtype(d) for d in dtypes]
    n_f32 = sum(d == np.dtype("float32") for d in dts)
    if np.result_type(*dts) == np.dtype("float32") or (n_ops >= 3 and n_f32 >= 2):
        return U32
    return U64


def f32_step_possible(dtypes: Sequence, n_ops: int) -> bool:
    """The same rule for the exact-data budget: a step of a schedule may compute in float32."""
    return unit_roundoff(dtypes, n_ops) == U32


def _xp(a):
    """numpy for numpy arrays, torch for torch tensors (the checkers below take either, on any device)."""
    if isinstance(a, np.ndarray):
        return np
    import torch

    return torch


def differing_entries(got, ref) -> int:
    """Entries of *got* that are not bitwise *ref* (``-0.0`` and ``0.0`` are equal, as in :func:`bitwise_equal`;
    a NaN anywhere differs); every entry when the shapes or dtypes differ.  numpy arrays or torch tensors."""
    n = int(np.prod(tuple(ref.shape), dtype=np.int64))
    if tuple(got.shape) != tuple(ref.shape) or got.dtype != ref.dtype:
        return max(n, 1)
    return int((got != ref).sum())


def nonfinite_violations(got, ref, dep, planted: float) -> int:
    """Entries that break the rule of a planted non-finite value: for a NaN exactly the dependency set *dep* is NaN,
    for an Inf exactly *dep* is non-finite (NaN or either infinity: the kernel may bracket the sum differently from
    numpy), and every other entry is bitwise the exact reference *ref*.  Every entry when the shapes differ.  numpy
    arrays or torch tensors (the GPU sweep calls it on device tensors)."""
    n = int(np.prod(tuple(ref.shape), dtype=np.int64))
    if tuple(got.shape) != tuple(ref.shape) or tuple(dep.shape) != tuple(ref.shape):
        return max(n, 1)
    xp = _xp(got)
    hit = xp.isnan(got) if math.isnan(planted) else ~xp.isfinite(got)
    return int((hit != dep).sum()) + int((got[~dep] != ref[~dep]).sum())


# --------------------------------------------------------------------------
# DG einsums: arrays shared by name, range cases, dependency sets, a device reference
# --------------------------------------------------------------------------

#: (exponent of the largest total, exponent of the subnormal quantum) per dtype: the range cases
RANGE = {np.dtype("float64"): (900, -1074), np.dtype("float32"): (100, -149)}


def rows_fit(rows: Sequence[Tuple[Sequence[str], int]], bits: Mapping[str, int], significand: int) -> bool:
    """Whether :func:`bits_fit` holds for every row: ``(names of its operands, terms per output entry)``."""
    return all(bits_fit([bits[nm] for nm in names], n_terms, significand) for names, n_terms in rows)


def shared_exact_bits(rows: Sequence[Tuple[Sequence[str], int]], f32_names: Sequence[str], significand: int,
                      rng: np.random.Generator) -> dict:
    """Mantissa bits per array NAME for einsums whose rows (and stages) share arrays: the budget of :func:`bits_fit`
    holds for every row that reads the array.  Each name starts at its share of the tightest row it is in; the bits
    left are then handed out one at a time in random order while every row still fits.  float32 names take at most 24
    bits, every name at least 1."""
    names = list(dict.fromkeys(nm for r, _ in rows for nm in r))
    w = {nm: float(rng.random()) + 0.25 for nm in names}
    cap = {nm: 24 if nm in f32_names else significand for nm in names}
    bits = {}
    for nm in names:
        share = []
        for r, n_terms in rows:
            if nm in r:
                budget = max(significand - max(int(n_terms), 1).bit_length(), len(r))
                share.append(budget * w[nm] / sum(w[x] for x in r))
        bits[nm] = max(1, min(cap[nm], int(min(share))))
    while not rows_fit(rows, bits, significand):   # (tiny budgets: give back until it fits)
        nm = max(bits, key=lambda x: bits[x])
        if bits[nm] == 1:
            raise AssertionError("no bit budget fits these rows")
        bits[nm] -= 1
    grown = True
    while grown:
        grown = False
        for k in rng.permutation(len(names)):
            nm = names[int(k)]
            if bits[nm] < cap[nm]:
                bits[nm] += 1
                if rows_fit(rows, bits, significand):
                    grown = True
                else:
                    bits[nm] -= 1
    return bits


def range_scales(positions: Sequence[Sequence[str]], bits: Mapping[str, int], significand: int, dtype, kind: str,
                 rng: np.random.Generator) -> dict:
    """Power-of-two scale per array name.  *positions* lists the names each operand position can hold (every row
    takes one name per position, so every row has the same total scale).  *kind*:

    ``"normal"``     scales in [-8, 8];
    ``"overflow"``   all scales >= 0, totals near ``2**900`` (float64) / ``2**100`` (float32);
    ``"subnormal"``  all scales <= 0, their sum the subnormal quantum ``-1074`` / ``-149``.

    Under one sign every partial product lies between 1 and the final result, so the exactness argument of the bit
    budget holds unchanged; subnormal arithmetic is fixed point, so those results are exact too (pass a *significand*
    a few bits short of the dtype's to keep every sum below the smallest normal)."""
    top, quantum = RANGE[np.dtype(dtype)]
    n = len(positions)
    if kind == "normal":
        per = [int(s) for s in rng.integers(-8, 9, size=n)]
    else:
        total = top - significand if kind == "overflow" else quantum
        w = rng.random(n) + 0.1
        per = [int(total * x / w.sum()) for x in w]
        per[int(rng.integers(n))] += total - sum(per)
        assert sum(per) == total and all((s >= 0) if kind == "overflow" else (s <= 0) for s in per)
    return {nm: per[p] for p, names in enumerate(positions) for nm in names}


def dependency_set(subscripts: str, shapes: Sequence[Tuple[int, ...]], operand: int, index: Tuple[int, ...]) -> np.ndarray:
    """Output entries that structurally depend on entry *index* of operand *operand*: the nonzero entries of the
    einsum of a one-hot array there with all-ones arrays for the other operands (a sum of non-negative terms is zero
    only when it has no term)."""
    ops = [np.ones(s) for s in shapes]
    ops[operand] = np.zeros(shapes[operand])
    ops[operand][tuple(index)] = 1.0
    return np.asarray(np.einsum(subscripts, *ops, optimize=True)) != 0


def int_reference(subscripts: str, mants: Sequence[np.ndarray], scale: int, out_dtype, significand: int) -> np.ndarray:
    """:func:`exact_reference` with one total *scale*, in any contraction order (integer sums are exact in any order:
    every partial sum is bounded by the absolute einsum, at most ``2**significand``)."""
    absum = np.einsum(subscripts, *[np.abs(m) for m in mants], optimize=True)
    assert (np.asarray(absum) <= (1 << significand)).all(), "exact-data budget exceeded"
    ints = np.asarray(np.einsum(subscripts, *mants, optimize=True), dtype=np.int64)
    return np.ldexp(ints.astype(np.float64), int(scale)).astype(np.dtype(out_dtype))


def torch_exact_reference(torch, subscripts: str, operands: Sequence, e_axes: Sequence[Optional[int]], out_e_axis: int,
                          out_dtype, chunk: int = 1 << 16):
    """Whole-array reference on the device for exact data: torch's float64 ``einsum`` of the operands (every partial
    sum of exact data fits the significand, so any order is exact), in chunks of *chunk* elements along E (*e_axes*:
    each operand's E axis, ``None`` for operands without one).  float32 data is widened and the result cast back,
    which is exact.  Not trusted on its own: :func:`check_torch_reference` compares it with :func:`int_reference`."""
    E = next(int(t.shape[a]) for t, a in zip(operands, e_axes) if a is not None)
    wide = [t.to(torch.float64) for t in operands]
    parts = []
    for e0 in range(0, max(E, 1), chunk):
        sl = [t if a is None else t.narrow(a, e0, min(chunk, E - e0)) for t, a in zip(wide, e_axes)]
        parts.append(torch.einsum(subscripts, *sl))
    return torch.cat(parts, dim=out_e_axis).to(getattr(torch, np.dtype(out_dtype).name))


__all__ = ["SIGNIFICAND", "U64", "U32", "summed_points", "compute_significand", "exact_bits", "bits_fit",
           "exact_operands", "exact_reference", "needs_more_than_f32", "bitwise_equal", "gamma", "bound_terms",
           "bounded_reference", "bound_ratio", "bound_violations", "unit_roundoff", "f32_step_possible", "RANGE", "rows_fit",
           "shared_exact_bits", "range_scales", "dependency_set", "int_reference", "torch_exact_reference",
           "nonfinite_violations", "differing_entries"]
