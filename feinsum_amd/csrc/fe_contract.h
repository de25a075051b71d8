// fe_contract.h -- strided batched tensor contraction (GETT) on the matrix cores.
// Any two-operand einsum is, after its indices are grouped (host: fe_einsum_contract),
//   C[b, m, n] = sum_k A[b, m, k] * B[b, n, k]
// with b, m, n, k multi-indices of up to FE_MAX_EINSUM_INDICES einsum indices, each with its own
// element strides per operand (0 = the operand does not carry the index).  The class of einsum the
// reference's TTGT / COGENT transforms take (tuning/impls/ttgt.py, cogent.py), on
// v_mfma_f64_16x16x4_f64 / v_mfma_f32_16x16x4_f32.
//
// Block: 256 threads, a 64 x 64 tile of C (2 x 2 waves of 32 x 32, four 16 x 16 accumulators per
// wave); k in steps of 16 through LDS, two buffers: the global loads of step s + 1 are in flight
// in registers while the MFMAs of step s read LDS.  The grid is persistent and 1-D over
// (batch, m tile, n tile), so a batch count of 10^6 needs no gridDim.y / z.
//
// Loads: each thread owns ONE k column per operand and 4 / V groups of V elements along the
// operand's fast direction -- V consecutive k of one row (k-fast) or V consecutive rows at one k
// (m-fast).  The row offsets are decoded once per tile, the k offset by an odometer that is
// advanced by 16 per step (a division only when an index wraps).  V > 1 only when the fast
// direction's innermost extent is a multiple of V (so a group never straddles an index or the
// ragged edge); the group is then one vector load when its stride is 1 and the host found the
// operand 16-byte aligned, V strided scalar loads otherwise.  All offsets are int64.
//
// Mixed operands: contract_mfma_kernel<double, VA, TA, TB, VB> with A or B stored as float.  Each operand has its own
// group width (16 bytes of ITS elements: 4 floats, 2 doubles) and loads its own type; stage() widens a float to double
// as it writes LDS, so the LDS image, the f64 MFMA loop and the stores are those of the all-double kernel.  With the
// defaults (TA = TB = T, VB = V) the template is the uniform kernel, instruction for instruction.
#pragma once
#include "fe_common.h"

namespace fe {

constexpr int kCtMaxIdx = 8;     // FE_MAX_EINSUM_INDICES
constexpr int kCtBM = 64;        // rows of a C tile (m) = columns (n)
constexpr int kCtBK = 16;        // k per LDS step
constexpr int kCtThreads = 256;
constexpr int kCtBlocksPerCu = 2;

// The grouped einsum (filled by the host; by value in the kernel arguments).
struct ContractPlan {
    int32_t nb, nm, nn, nk;              // indices per group (innermost last)
    int32_t a_mfast, b_mfast;            // operand walks its rows (1) or its k (0) fastest
    int32_t a_vec, b_vec;                // V-groups are single vector loads
    int64_t a_vstep, b_vstep;            // element stride inside a V-group
    int64_t M, N, K, tiles_m, tiles_n, n_tiles;
    int64_t b_ext[kCtMaxIdx], b_sa[kCtMaxIdx], b_sb[kCtMaxIdx], b_sc[kCtMaxIdx];
    int64_t m_ext[kCtMaxIdx], m_sa[kCtMaxIdx], m_sc[kCtMaxIdx];
    int64_t n_ext[kCtMaxIdx], n_sb[kCtMaxIdx], n_sc[kCtMaxIdx];
    int64_t k_ext[kCtMaxIdx], k_sa[kCtMaxIdx], k_sb[kCtMaxIdx];
    int64_t k_slices, k_slice_len, c_size;   // split-K only: k slices (of a multiple of kCtBK), entries of C
};

template <typename T>
struct CtMfma;
// C/D layouts differ: f64 row = (lane >> 4) + 4 reg, f32 row = 4 (lane >> 4) + reg; col = lane & 15 for both.
template <>
struct CtMfma<double> {
    typedef double acc_t __attribute__((ext_vector_type(4)));
    static __device__ __forceinline__ acc_t step(double a, double b, acc_t c) {
        return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
    }
    static __device__ __forceinline__ int row(int lane, int r) { return (lane >> 4) + 4 * r; }
};
template <>
struct CtMfma<float> {
    typedef float acc_t __attribute__((ext_vector_type(4)));
    static __device__ __forceinline__ acc_t step(float a, float b, acc_t c) {
        return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
    }
    static __device__ __forceinline__ int row(int lane, int r) { return 4 * (lane >> 4) + r; }
};

// Offsets of linear position x of a group (last index fastest) under up to three stride sets.
__device__ __forceinline__ void ct_decode(int64_t x, int n, const int64_t* ext, const int64_t* s0, const int64_t* s1,
                                          const int64_t* s2, int64_t& o0, int64_t& o1, int64_t& o2) {
    o0 = o1 = o2 = 0;
#pragma unroll
    for (int t = 0; t < kCtMaxIdx; ++t) {
        const int j = n - 1 - t;
        if (j >= 0) {
            const int64_t q = x / ext[j];
            const int64_t r = x - q * ext[j];
            o0 += r * s0[j];
            o1 += r * s1[j];
            o2 += r * s2[j];
            x = q;
        }
    }
}

// k odometer: idx[t] is the position in index n - 1 - t (registers: t is a compile-time constant).
__device__ __forceinline__ void ct_advance(int64_t (&idx)[kCtMaxIdx], int n, const int64_t* ext, int64_t carry) {
#pragma unroll
    for (int t = 0; t < kCtMaxIdx; ++t) {
        const int j = n - 1 - t;
        if (j >= 0 && carry != 0) {
            const int64_t v = idx[t] + carry;
            if (v < ext[j]) {
                idx[t] = v;
                carry = 0;
            } else {
                carry = v / ext[j];
                idx[t] = v - carry * ext[j];
            }
        }
    }
}

__device__ __forceinline__ int64_t ct_koff(const int64_t (&idx)[kCtMaxIdx], int n, const int64_t* s) {
    int64_t o = 0;
#pragma unroll
    for (int t = 0; t < kCtMaxIdx; ++t)
        if (n - 1 - t >= 0) o += idx[t] * s[n - 1 - t];
    return o;
}

// SPLIT (split-K, fe_einsum_reduce): a work item is (batch, m tile, n tile, k slice); the item sums the k of its slice
// only, [kb, ke), and writes its masked partial tile into slice ks of the workspace C[ks * c_size + ...] (the layout of
// the output), which reduce_combine_kernel then sums in slice order.  The MFMA loop, the staging and the loads are
// those of the plain kernel; SPLIT = false is the plain kernel.
//
// ACC (fe_einsum_contract_acc): C <- alpha E + beta C, E the sum above.  The kernel then takes two more arguments behind
// C, alpha and beta of type T (SCALE...: empty without ACC, so the plain and the split-K instantiations keep their
// argument list).  Only the store epilogue differs.  beta != 0 (block-uniform: one scalar branch per tile): a thread
// first loads all of its up to 16 old values -- under the guards, at the addresses and through the row map of its stores,
// so every entry is read and written by one thread and nothing is ordered across threads -- and then stores
// axpby_combine(alpha, E, beta, old); the loads are issued before the first store, so their latency is paid once per
// tile.  beta == 0: alpha E is stored and nothing is read.  The loads stand behind the k loop's last barrier.
template <typename T, int V, typename TA = T, typename TB = T, int VB = V, bool SPLIT = false, bool ACC = false,
          typename... SCALE>
__global__ __launch_bounds__(kCtThreads) void contract_mfma_kernel(ContractPlan P, const TA* __restrict__ A,
                                                                   const TB* __restrict__ B, T* __restrict__ C,
                                                                   SCALE... scale) {
    static_assert(!(SPLIT && ACC), "the split-K partials are combined by reduce_combine_kernel, which accumulates");
    static_assert(sizeof...(SCALE) == (ACC ? 2 : 0), "ACC: (alpha, beta) behind C; nothing otherwise");
    typedef CtMfma<T> Mfma;
    typedef typename Mfma::acc_t acc_t;
    constexpr int VA = V;
    typedef TA veca_t __attribute__((ext_vector_type(VA)));
    typedef TB vecb_t __attribute__((ext_vector_type(VB)));
    constexpr int RA = 4 / VA, RB = 4 / VB;        // V-groups per thread and operand
    constexpr int R = RA > RB ? RA : RB;
    constexpr int RSTEPA = 16 * VA, RSTEPB = 16 * VB;   // rows between a thread's groups
    constexpr int LD = kCtBM + 64 / (int)sizeof(T);   // padded LDS row: k rows 0..3 of an MFMA read hit distinct banks
    __shared__ T lds[2][2][kCtBK][LD];             // [buffer][A, B][k][row]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    // loading slot of operand X: its k column kk and first row rr
    const int kkA = P.a_mfast ? tid >> 4 : VA * (tid % (16 / VA));
    const int rrA = P.a_mfast ? VA * (tid & 15) : tid / (16 / VA);
    const int kkB = P.b_mfast ? tid >> 4 : VB * (tid % (16 / VB));
    const int rrB = P.b_mfast ? VB * (tid & 15) : tid / (16 / VB);
    const int64_t n_items = SPLIT ? P.n_tiles * P.k_slices : P.n_tiles;

    for (int64_t item = blockIdx.x; item < n_items; item += gridDim.x) {
        const int64_t tile = SPLIT ? item % P.n_tiles : item;
        const int64_t ks = SPLIT ? item / P.n_tiles : 0;
        const int64_t kb = SPLIT ? ks * P.k_slice_len : 0;   // the item's k: [kb, ke)
        const int64_t ke = SPLIT ? (kb + P.k_slice_len < P.K ? kb + P.k_slice_len : P.K) : P.K;
        const int64_t nsteps = (ke - kb + kCtBK - 1) / kCtBK;
        T* __restrict__ Cs = SPLIT ? C + ks * P.c_size : C;
        const int64_t tn = tile % P.tiles_n, rest = tile / P.tiles_n;
        const int64_t tm = rest % P.tiles_m, bi = rest / P.tiles_m;
        const int64_t m0 = tm * kCtBM, n0 = tn * kCtBM;
        int64_t boffA, boffB, boffC;
        ct_decode(bi, P.nb, P.b_ext, P.b_sa, P.b_sb, P.b_sc, boffA, boffB, boffC);

        int64_t rowA[R], rowB[R], unused0, unused1;
        bool rvA[R], rvB[R];
#pragma unroll
        for (int g = 0; g < R; ++g) {
            const int64_t ra = m0 + rrA + g * RSTEPA, rb = n0 + rrB + g * RSTEPB;
            rvA[g] = g < RA && ra < P.M;   // (g >= RA / RB: only when the operands' V differ)
            rvB[g] = g < RB && rb < P.N;
            rowA[g] = rowB[g] = 0;
            if (rvA[g]) ct_decode(ra, P.nm, P.m_ext, P.m_sa, P.m_sa, P.m_sa, rowA[g], unused0, unused1);
            if (rvB[g]) ct_decode(rb, P.nn, P.n_ext, P.n_sb, P.n_sb, P.n_sb, rowB[g], unused0, unused1);
        }

        int64_t kiA[kCtMaxIdx], kiB[kCtMaxIdx];
#pragma unroll
        for (int t = 0; t < kCtMaxIdx; ++t) kiA[t] = kiB[t] = 0;
        if (nsteps > 0) {   // (an extent of 0 would divide by zero)
            ct_advance(kiA, P.nk, P.k_ext, kb + kkA);
            ct_advance(kiB, P.nk, P.k_ext, kb + kkB);
        }

        TA ra[R][VA];
        TB rb[R][VB];
        auto load = [&](int64_t k0) {
            const int64_t koA = ct_koff(kiA, P.nk, P.k_sa), koB = ct_koff(kiB, P.nk, P.k_sb);
            const bool kvA = k0 + kkA < ke, kvB = k0 + kkB < ke;
#pragma unroll
            for (int g = 0; g < R; ++g) {
                if (rvA[g] && kvA) {
                    const TA* p = A + (boffA + rowA[g] + koA);
                    if (VA > 1 && P.a_vec) {
                        const veca_t x = *reinterpret_cast<const veca_t*>(p);
#pragma unroll
                        for (int v = 0; v < VA; ++v) ra[g][v] = x[v];
                    } else {
#pragma unroll
                        for (int v = 0; v < VA; ++v) ra[g][v] = p[v * P.a_vstep];
                    }
                } else {
#pragma unroll
                    for (int v = 0; v < VA; ++v) ra[g][v] = TA(0);
                }
                if (rvB[g] && kvB) {
                    const TB* p = B + (boffB + rowB[g] + koB);
                    if (VB > 1 && P.b_vec) {
                        const vecb_t x = *reinterpret_cast<const vecb_t*>(p);
#pragma unroll
                        for (int v = 0; v < VB; ++v) rb[g][v] = x[v];
                    } else {
#pragma unroll
                        for (int v = 0; v < VB; ++v) rb[g][v] = p[v * P.b_vstep];
                    }
                } else {
#pragma unroll
                    for (int v = 0; v < VB; ++v) rb[g][v] = TB(0);
                }
            }
        };
        auto stage = [&](int buf) {   // T(x): a float operand of a double contraction is widened here
#pragma unroll
            for (int g = 0; g < R; ++g)
#pragma unroll
                for (int v = 0; v < (VA > VB ? VA : VB); ++v) {
                    if (g < RA && v < VA) {
                        if (P.a_mfast) lds[buf][0][kkA][rrA + g * RSTEPA + v] = T(ra[g][v]);
                        else lds[buf][0][kkA + v][rrA + g * RSTEPA] = T(ra[g][v]);
                    }
                    if (g < RB && v < VB) {
                        if (P.b_mfast) lds[buf][1][kkB][rrB + g * RSTEPB + v] = T(rb[g][v]);
                        else lds[buf][1][kkB + v][rrB + g * RSTEPB] = T(rb[g][v]);
                    }
                }
        };

        acc_t acc[2][2];
#pragma unroll
        for (int f = 0; f < 2; ++f)
#pragma unroll
            for (int g = 0; g < 2; ++g) acc[f][g] = acc_t{0, 0, 0, 0};

        if (nsteps > 0) {
            load(kb);
            stage(0);
            __syncthreads();
        }
        for (int64_t s = 0; s < nsteps; ++s) {
            const int cur = (int)(s & 1);
            const bool more = s + 1 < nsteps;
            if (more) {
                ct_advance(kiA, P.nk, P.k_ext, kCtBK);
                ct_advance(kiB, P.nk, P.k_ext, kCtBK);
                load(kb + (s + 1) * kCtBK);
            }
#pragma unroll
            for (int ks = 0; ks < kCtBK / 4; ++ks) {
                const int kr = 4 * ks + (lane >> 4);
                T a[2], b[2];
#pragma unroll
                for (int f = 0; f < 2; ++f) a[f] = lds[cur][0][kr][32 * wm + 16 * f + (lane & 15)];
#pragma unroll
                for (int g = 0; g < 2; ++g) b[g] = lds[cur][1][kr][32 * wn + 16 * g + (lane & 15)];
#pragma unroll
                for (int f = 0; f < 2; ++f)
#pragma unroll
                    for (int g = 0; g < 2; ++g) acc[f][g] = Mfma::step(a[f], b[g], acc[f][g]);
            }
            if (more) stage(cur ^ 1);
            __syncthreads();   // (every tile ends on a barrier: the next tile's first stage may overwrite buffer 0)
        }

        // C: column (n) on the lane, rows in the registers
        int64_t colC[2];
        bool cv[2];
#pragma unroll
        for (int g = 0; g < 2; ++g) {
            const int64_t col = n0 + 32 * wn + 16 * g + (lane & 15);
            cv[g] = col < P.N;
            colC[g] = 0;
            if (cv[g]) ct_decode(col, P.nn, P.n_ext, P.n_sc, P.n_sc, P.n_sc, colC[g], unused0, unused1);
        }
        if constexpr (ACC) {
            const T ab[2] = {T(scale)...};
            const T alpha = ab[0], beta = ab[1];
            int64_t offC[2][4];
            bool rv[2][4];
#pragma unroll
            for (int f = 0; f < 2; ++f)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int64_t row = m0 + 32 * wm + 16 * f + Mfma::row(lane, r);
                    rv[f][r] = row < P.M;
                    int64_t rowC = 0;
                    if (rv[f][r]) ct_decode(row, P.nm, P.m_ext, P.m_sc, P.m_sc, P.m_sc, rowC, unused0, unused1);
                    offC[f][r] = boffC + rowC;
                }
            if (beta != T(0)) {
                // Loads, then the 16 combines in straight-line code, then the stores: the one wait for the old values stands
                // in front of the combines.  (A combine inside a store's own guard put a wait -- which counts the earlier
                // stores too -- in front of every store: 16 round trips per tile, 8 % on a 1024^3 GEMM.)  A tile inside C,
                // which is block-uniform, needs no guard at all: its loads and stores are straight-line code as well.
                const bool full = m0 + kCtBM <= P.M && n0 + kCtBM <= P.N;
                T val[2][4][2];
                if (full) {
#pragma unroll
                    for (int f = 0; f < 2; ++f)
#pragma unroll
                        for (int r = 0; r < 4; ++r)
#pragma unroll
                            for (int g = 0; g < 2; ++g) val[f][r][g] = Cs[offC[f][r] + colC[g]];
                } else {
#pragma unroll
                    for (int f = 0; f < 2; ++f)
#pragma unroll
                        for (int r = 0; r < 4; ++r)
#pragma unroll
                            for (int g = 0; g < 2; ++g) val[f][r][g] = rv[f][r] && cv[g] ? Cs[offC[f][r] + colC[g]] : T(0);
                }
#pragma unroll
                for (int f = 0; f < 2; ++f)
#pragma unroll
                    for (int r = 0; r < 4; ++r)
#pragma unroll
                        for (int g = 0; g < 2; ++g) val[f][r][g] = axpby_combine(alpha, acc[f][g][r], beta, val[f][r][g]);
                if (full) {
#pragma unroll
                    for (int f = 0; f < 2; ++f)
#pragma unroll
                        for (int r = 0; r < 4; ++r)
#pragma unroll
                            for (int g = 0; g < 2; ++g) Cs[offC[f][r] + colC[g]] = val[f][r][g];
                } else {
#pragma unroll
                    for (int f = 0; f < 2; ++f)
#pragma unroll
                        for (int r = 0; r < 4; ++r)
#pragma unroll
                            for (int g = 0; g < 2; ++g)
                                if (rv[f][r] && cv[g]) Cs[offC[f][r] + colC[g]] = val[f][r][g];
                }
            } else {
#pragma unroll
                for (int f = 0; f < 2; ++f)
#pragma unroll
                    for (int r = 0; r < 4; ++r)
#pragma unroll
                        for (int g = 0; g < 2; ++g)
                            if (rv[f][r] && cv[g]) Cs[offC[f][r] + colC[g]] = alpha * acc[f][g][r];
            }
        } else {
#pragma unroll
            for (int f = 0; f < 2; ++f)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int64_t row = m0 + 32 * wm + 16 * f + Mfma::row(lane, r);
                    if (row >= P.M) continue;
                    int64_t rowC;
                    ct_decode(row, P.nm, P.m_ext, P.m_sc, P.m_sc, P.m_sc, rowC, unused0, unused1);
#pragma unroll
                    for (int g = 0; g < 2; ++g)
                        if (cv[g]) Cs[boffC + rowC + colC[g]] = acc[f][g][r];
                }
        }
    }
}

}  // namespace fe
