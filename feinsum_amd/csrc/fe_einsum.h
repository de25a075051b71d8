// fe_einsum.h -- generic einsum kernel: any explicit-mode einsum, one thread (or a group of
// G lanes) per output entry, loop over the flattened summation space.
// It is the device restatement of the single-instruction loop nest feinsum's
// generate_loopy emits for the trivial schedule (codegen/loopy.py:242-305):
//   out[o...] = sum_{s...} prod_p operand_p[o..., s...]
// and exists so that every BatchedEinsum the builders accept can be validated
// and timed through the same boundary; the DG families never take this path.
#pragma once
#include "../../include/feinsum_hip.h"
#include "fe_common.h"

namespace fe {

// G lanes share one output entry: lane l of the group takes summation points l, l + G, ... (last
// summation index fastest) and the partial sums are combined with wave shuffles.  The host
// picks G > 1 when the fastest summation index is contiguous in an operand, so that a group reads
// consecutive addresses (one thread per output walks that operand with a stride of a whole row
// per lane: 64 cache lines per load instruction).  G = 1 is the plain restatement.
//
// MIXED (T = double): an einsum whose operands are float64 or float32 each (d.dtype's FE_DTYPE_OPERAND_F32 flags: uniform over
// the grid, a scalar branch per load); a float32 value is widened when it is loaded.
template <typename T, int G, bool MIXED = false>
__global__ __launch_bounds__(256) void einsum_generic_kernel(fe_einsum_desc d, fe_einsum_ptrs ops,
                                                             T* __restrict__ out,
                                                             int64_t n_out_entries, int64_t n_sum_points) {
    const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t idx = tid / G;
    const int part = (int)(tid % G);
    const bool live = idx < n_out_entries;   // whole groups are live or dead; dead lanes still shuffle
    // output multi-index (last index fastest) -> base offset of every operand
    int64_t base[FE_MAX_EINSUM_OPERANDS];
    for (int p = 0; p < d.n_operands; ++p) base[p] = 0;
    int64_t rem = live ? idx : 0;
    for (int k = d.n_out - 1; k >= 0; --k) {
        const int64_t ok = rem % d.out_extent[k];
        rem /= d.out_extent[k];
        for (int p = 0; p < d.n_operands; ++p) base[p] += ok * d.op_out_stride[p][k];
    }
    T acc = T(0);
    int64_t sidx[FE_MAX_EINSUM_INDICES];
    for (int k = 0; k < d.n_sum; ++k) sidx[k] = 0;
    auto carry = [&]() {   // odometer, last summation index fastest
        for (int k = d.n_sum - 1; k > 0; --k)
            while (sidx[k] >= d.sum_extent[k]) {
                sidx[k] -= d.sum_extent[k];
                ++sidx[k - 1];
            }
    };
    if (d.n_sum > 0 && n_sum_points > 0) {   // (an empty summation space has zero extents: carry() would not end)
        sidx[d.n_sum - 1] = part;
        carry();
    }
    for (int64_t s = part; live && s < n_sum_points; s += G) {
        T prod = T(1);
        for (int p = 0; p < d.n_operands; ++p) {
            int64_t off = base[p];
            for (int k = 0; k < d.n_sum; ++k) off += sidx[k] * d.op_sum_stride[p][k];
            if (MIXED && (d.dtype & FE_DTYPE_OPERAND_F32(p)))
                prod *= T(static_cast<const float*>(ops.p[p])[off]);
            else
                prod *= static_cast<const T*>(ops.p[p])[off];
        }
        acc += prod;
        if (d.n_sum > 0) {
            sidx[d.n_sum - 1] += G;
            carry();
        }
    }
#pragma unroll
    for (int w = G / 2; w >= 1; w /= 2) acc += __shfl_xor(acc, w, 64);
    if (live && part == 0) out[idx] = acc;
}

// Pointwise product of operands that all have the output's own contiguous layout
// ('ij,ij->ij', 'ijk,ijk->ijk': tuning/impls/ij_ij_to_ij.py, ijk_ijk_to_ijk.py): a pure
// stream, two values per lane and iteration.
template <typename T>
__global__ __launch_bounds__(256) void einsum_pointwise_kernel(fe_einsum_ptrs ops, int n_operands,
                                                               T* __restrict__ out, int64_t n) {
    typedef T v2 __attribute__((ext_vector_type(2)));
    const int64_t pairs = n / 2;
    const bool aligned = [&] {
        uintptr_t bits = reinterpret_cast<uintptr_t>(out);
        for (int p = 0; p < n_operands; ++p) bits |= reinterpret_cast<uintptr_t>(ops.p[p]);
        return (bits & (2 * sizeof(T) - 1)) == 0;
    }();
    const int64_t stride = (int64_t)gridDim.x * 256;
    if (aligned) {
        for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < pairs; q += stride) {
            v2 acc = __builtin_nontemporal_load(static_cast<const v2*>(ops.p[0]) + q);
            for (int p = 1; p < n_operands; ++p) acc *= __builtin_nontemporal_load(static_cast<const v2*>(ops.p[p]) + q);
            __builtin_nontemporal_store(acc, reinterpret_cast<v2*>(out) + q);
        }
    }
    for (int64_t i = (aligned ? 2 * pairs : 0) + (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
        T acc = static_cast<const T*>(ops.p[0])[i];
        for (int p = 1; p < n_operands; ++p) acc *= static_cast<const T*>(ops.p[p])[i];
        out[i] = acc;
    }
}

// out <- alpha x + beta out over n contiguous entries (fe_axpby: the second pass of an accumulating evaluation whose kernel
// has no accumulating form).  A stream like the one above: 16 bytes per lane and iteration where out and x sit alike within
// 16 bytes -- a scalar head up to the first 16-byte boundary, a scalar tail behind the last whole vector -- and entry by entry
// where they do not.  beta == 0 does not read out.  The combine is axpby_combine (fe_common.h), as in the face-mass kernel.
template <typename T>
__global__ __launch_bounds__(256) void axpby_kernel(T* __restrict__ out, const T* __restrict__ x, int64_t n, T alpha, T beta) {
    constexpr int W = 16 / (int)sizeof(T);
    typedef T vw __attribute__((ext_vector_type(W)));
    const uintptr_t ao = reinterpret_cast<uintptr_t>(out) & 15, ax = reinterpret_cast<uintptr_t>(x) & 15;
    const bool alike = ao == ax;
    int64_t head = alike ? (int64_t)(((16 - ao) & 15) / sizeof(T)) : n;
    head = head < n ? head : n;
    const int64_t vecs = (n - head) / W;
    const int64_t stride = (int64_t)gridDim.x * 256, t0 = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool reads = beta != T(0);
    vw av, bv;
    for (int w = 0; w < W; ++w) { av[w] = alpha; bv[w] = beta; }
    for (int64_t q = t0; q < vecs; q += stride) {
        vw* o = reinterpret_cast<vw*>(out + head) + q;
        const vw xv = __builtin_nontemporal_load(reinterpret_cast<const vw*>(x + head) + q);
        const vw r = reads ? axpby_combine(av, xv, bv, __builtin_nontemporal_load(o)) : av * xv;
        __builtin_nontemporal_store(r, o);
    }
    for (int64_t i = t0; i < n - vecs * W; i += stride) {   // the head, then the tail
        const int64_t e = i < head ? i : i + vecs * W;
        out[e] = reads ? axpby_combine(alpha, x[e], beta, out[e]) : alpha * x[e];
    }
}

// The pointwise stream of a float64 einsum with float32 operands (bit p of f32_mask: operand p is float32): pairs of
// 16 bytes (float64) or 8 bytes (float32) per operand, each operand aligned to its own pair size.
__global__ __launch_bounds__(256) void einsum_pointwise_mixed_kernel(fe_einsum_ptrs ops, int n_operands,
                                                                     unsigned f32_mask, double* __restrict__ out,
                                                                     int64_t n) {
    typedef double d2 __attribute__((ext_vector_type(2)));
    typedef float f2 __attribute__((ext_vector_type(2)));
    const int64_t pairs = n / 2;
    const bool aligned = [&] {
        bool ok = (reinterpret_cast<uintptr_t>(out) & 15) == 0;
        for (int p = 0; p < n_operands; ++p)
            ok &= (reinterpret_cast<uintptr_t>(ops.p[p]) & ((f32_mask >> p & 1) ? 7 : 15)) == 0;
        return ok;
    }();
    auto pair = [&](int p, int64_t q) -> d2 {
        if (f32_mask >> p & 1) {
            const f2 x = __builtin_nontemporal_load(static_cast<const f2*>(ops.p[p]) + q);
            return d2{x[0], x[1]};
        }
        return __builtin_nontemporal_load(static_cast<const d2*>(ops.p[p]) + q);
    };
    auto one = [&](int p, int64_t i) -> double {
        return (f32_mask >> p & 1) ? double(static_cast<const float*>(ops.p[p])[i])
                                   : static_cast<const double*>(ops.p[p])[i];
    };
    const int64_t stride = (int64_t)gridDim.x * 256;
    if (aligned) {
        for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < pairs; q += stride) {
            d2 acc = pair(0, q);
            for (int p = 1; p < n_operands; ++p) acc *= pair(p, q);
            __builtin_nontemporal_store(acc, reinterpret_cast<d2*>(out) + q);
        }
    }
    for (int64_t i = (aligned ? 2 * pairs : 0) + (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
        double acc = one(0, i);
        for (int p = 1; p < n_operands; ++p) acc *= one(p, i);
        out[i] = acc;
    }
}

}  // namespace fe
