// fe_reduce.h -- split reductions: einsums that sum a long summation space into a small output
// ('ei,ei->', 'ej,ej->j', 'e,ei,ei->').  The generic kernel gives each output entry one lane group that
// walks the whole summation space, so such an einsum runs on one wave; here the flattened summation space
// (last index fastest) is cut into S contiguous slices, one block reduces one slice for a chunk of output
// entries and writes one partial per (slice, output entry) into a workspace, and a second launch sums the
// partials of every output entry in a fixed order (fe_einsum_reduce, fe_einsum_reduce_plan).
//
// S, the slices and every summation order depend on the plan alone (the host derives it from the
// descriptor, never from the device), so a result is bitwise the same across runs, streams, graph
// replays and devices of one architecture.  No atomics.
//
// Block of the partial kernel: C output entries x R summation walkers (C R <= 256).  Thread (r, j) takes
// output entry chunk C + j and the summation points r, r + R, ... of its slice; the R sums of an entry are
// then added in a fixed tree through LDS.  The host picks C = 1 when the summation index is the contiguous
// one (lanes read consecutive summation points) and C = min(n_out, 256) when an output index is (lanes read
// consecutive output entries of one summation row).  Offsets advance by a mixed-radix add of the step R:
// one compare per summation index and iteration, no division in the loop.  VEC: the summation space is one
// unit-stride index in every operand (after the host merged what is contiguous) -- V consecutive points per
// lane and operand are one 16-byte load (8 bytes for a float32 operand of a float64 einsum).
#pragma once
#include "../../include/feinsum_hip.h"
#include "fe_common.h"

namespace fe {

constexpr int kRdThreads = 256;
constexpr int kRdMaxIdx = FE_MAX_EINSUM_INDICES;
constexpr int kRdMaxOps = FE_MAX_EINSUM_OPERANDS;

struct ReducePlan {
    int32_t n_ops, n_out, n_sum;         // operands, output indices, summation indices (merged, extents > 1)
    int32_t C, R, R2;                    // output entries per block, walkers per entry, R rounded up to a power of 2
    uint32_t f32_mask;                   // bit p: operand p is float32 (float64 compute)
    int32_t vec;                         // (VEC kernels) every operand 16-byte aligned at every output entry
    int64_t n_out_entries, n_sum_points, slices, slice_len;
    int64_t out_ext[kRdMaxIdx], sum_ext[kRdMaxIdx];
    int64_t out_st[kRdMaxOps][kRdMaxIdx], sum_st[kRdMaxOps][kRdMaxIdx];
    int64_t step_dig[kRdMaxIdx];         // digit t of R (t = 0: the fastest summation index)
    int64_t step_off[kRdMaxOps];         // offset of one step of R points, without wraps
    int64_t wrap_off[kRdMaxOps][kRdMaxIdx];   // [p][k]: offset change when index k wraps into index k - 1
};

template <typename T, bool MIXED>
__device__ __forceinline__ T rd_load(const fe_einsum_ptrs& ops, uint32_t f32_mask, int p, int64_t off) {
    if (MIXED && (f32_mask >> p & 1)) return T(static_cast<const float*>(ops.p[p])[off]);
    return static_cast<const T*>(ops.p[p])[off];
}

// Partials: ws[slice * n_out_entries + o] = sum over the slice's points of prod_p operand_p[o, s].
// Grid: (slices, ceil(n_out_entries / C)).
template <typename T, bool MIXED, bool VEC>
__global__ __launch_bounds__(kRdThreads) void reduce_partial_kernel(ReducePlan P, fe_einsum_ptrs ops, T* __restrict__ ws) {
    __shared__ T red[kRdThreads];
    const int tid = threadIdx.x;
    const int j = tid % P.C, r = tid / P.C;
    const int64_t slice = blockIdx.x;
    const int64_t o = (int64_t)blockIdx.y * P.C + j;
    const bool live = r < P.R && o < P.n_out_entries;
    const int64_t s0 = slice * P.slice_len;
    const int64_t s1 = s0 + P.slice_len < P.n_sum_points ? s0 + P.slice_len : P.n_sum_points;
    T acc = T(0);
    if (live && s0 + r < s1) {
        int64_t off[kRdMaxOps];
        int64_t rem = o;
#pragma unroll
        for (int p = 0; p < kRdMaxOps; ++p) off[p] = 0;
#pragma unroll
        for (int t = 0; t < kRdMaxIdx; ++t) {   // output entry -> base offsets (last output index fastest)
            const int k = P.n_out - 1 - t;
            if (k >= 0) {
                const int64_t q = rem / P.out_ext[k], x = rem - q * P.out_ext[k];
                rem = q;
#pragma unroll
                for (int p = 0; p < kRdMaxOps; ++p)
                    if (p < P.n_ops) off[p] += x * P.out_st[p][k];
            }
        }
        if (VEC) {   // one unit-stride summation index: V points per lane and step
            constexpr int V = sizeof(T) == 8 ? 2 : 4;
            typedef T vt __attribute__((ext_vector_type(V)));
            typedef float vf __attribute__((ext_vector_type(V)));
            const int64_t sv = s0 + (s1 - s0) / V * V;   // (s0 is a multiple of V: the slice length is)
            for (int64_t s = s0 + (int64_t)r * V; s < sv; s += (int64_t)P.R * V) {
                vt prod = T(1);
#pragma unroll
                for (int p = 0; p < kRdMaxOps; ++p) {
                    if (p < P.n_ops) {
                        vt x;
                        if (MIXED && (P.f32_mask >> p & 1)) {
                            const vf y = *reinterpret_cast<const vf*>(static_cast<const float*>(ops.p[p]) + off[p] + s);
#pragma unroll
                            for (int v = 0; v < V; ++v) x[v] = T(y[v]);
                        } else {
                            x = *reinterpret_cast<const vt*>(static_cast<const T*>(ops.p[p]) + off[p] + s);
                        }
                        prod *= x;
                    }
                }
#pragma unroll
                for (int v = 0; v < V; ++v) acc += prod[v];
            }
            for (int64_t s = sv + r; s < s1; s += P.R) {   // the slice's last s1 - sv < V points
                T prod = T(1);
#pragma unroll
                for (int p = 0; p < kRdMaxOps; ++p)
                    if (p < P.n_ops) prod *= rd_load<T, MIXED>(ops, P.f32_mask, p, off[p] + s);
                acc += prod;
            }
        } else {
            int64_t sidx[kRdMaxIdx];   // sidx[t]: position in summation index n_sum - 1 - t
            rem = s0 + r;
#pragma unroll
            for (int t = 0; t < kRdMaxIdx; ++t) {
                sidx[t] = 0;
                const int k = P.n_sum - 1 - t;
                if (k >= 0) {
                    if (k > 0) {
                        const int64_t q = rem / P.sum_ext[k];
                        sidx[t] = rem - q * P.sum_ext[k];
                        rem = q;
                    } else {
                        sidx[t] = rem;   // (the outermost index takes the rest)
                    }
#pragma unroll
                    for (int p = 0; p < kRdMaxOps; ++p)
                        if (p < P.n_ops) off[p] += sidx[t] * P.sum_st[p][k];
                }
            }
            for (int64_t s = s0 + r; s < s1; s += P.R) {
                T prod = T(1);
#pragma unroll
                for (int p = 0; p < kRdMaxOps; ++p)
                    if (p < P.n_ops) prod *= rd_load<T, MIXED>(ops, P.f32_mask, p, off[p]);
                acc += prod;
                // advance by R points: digit t of R plus the carry; a digit below its extent wraps at most once
                int carry = 0;
#pragma unroll
                for (int t = 0; t < kRdMaxIdx; ++t) {
                    const int k = P.n_sum - 1 - t;
                    if (k >= 0) {
                        int64_t v = sidx[t] + P.step_dig[t] + carry;
                        carry = 0;
                        if (k > 0 && v >= P.sum_ext[k]) {
                            v -= P.sum_ext[k];
                            carry = 1;
#pragma unroll
                            for (int p = 0; p < kRdMaxOps; ++p)
                                if (p < P.n_ops) off[p] += P.wrap_off[p][k];
                        }
                        sidx[t] = v;
                    }
                }
#pragma unroll
                for (int p = 0; p < kRdMaxOps; ++p)
                    if (p < P.n_ops) off[p] += P.step_off[p];
            }
        }
    }
    // the R walkers of each entry: a fixed tree (R need not be a power of 2)
    red[tid] = acc;
    __syncthreads();
    for (int h = P.R2 / 2; h >= 1; h /= 2) {
        if (r < h && r + h < P.R && j < P.C) red[tid] += red[tid + h * P.C];
        __syncthreads();
    }
    if (r == 0 && o < P.n_out_entries) ws[slice * P.n_out_entries + o] = red[j];
}

// out[o] = sum_s ws[s * n_out + o]: one wave per output entry, lane l adds slices l, l + 64, ... in order, then
// a fixed butterfly.  Grid: ceil(n_out / 4) blocks of 256.
// ACC (fe_einsum_reduce_acc): out[o] <- alpha (that sum) + beta out[o], two more arguments of type T behind `slices`
// (SCALE...: empty without ACC); beta == 0 does not read out (axpby_combine, fe_common.h).  The sum is the same.
template <typename T, bool ACC = false, typename... SCALE>
__global__ __launch_bounds__(kRdThreads) void reduce_combine_kernel(const T* __restrict__ ws, T* __restrict__ out,
                                                                    int64_t n_out, int64_t slices, SCALE... scale) {
    static_assert(sizeof...(SCALE) == (ACC ? 2 : 0), "ACC: (alpha, beta) behind slices; nothing otherwise");
    const int64_t o = (int64_t)blockIdx.x * (kRdThreads / 64) + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    T acc = T(0);
    if (o < n_out)
        for (int64_t s = lane; s < slices; s += 64) acc += ws[s * n_out + o];
#pragma unroll
    for (int w = 32; w >= 1; w /= 2) acc += __shfl_xor(acc, w, 64);
    if constexpr (ACC) {
        const T ab[2] = {T(scale)...};
        const T alpha = ab[0], beta = ab[1];
        if (o < n_out && lane == 0) out[o] = beta != T(0) ? axpby_combine(alpha, acc, beta, out[o]) : alpha * acc;
    } else {
        if (o < n_out && lane == 0) out[o] = acc;
    }
}

}  // namespace fe
