// fe_weightgrad.h -- the gradient of the weighted element operator with respect to its weight:
//
//   dW[e, q] = sum_k (sum_i P[i, q] g_k[e, i]) (sum_j A[q, j] u_k[e, j])          einsum iq,qj,ej,ei->eq, rows summed; k < nb
//
// P [Ni][Nq] (stored [Nq][Ni] with FE_WO_P_T), A [Nq][Nj] (stored [Nj][Nq] with FE_WO_A_T), u_k [E][Nj], g_k [E][Ni] (the
// gradient of fe_weightedop.h's output k), dW [E][Nq]: two interpolations to the quadrature grid and a pointwise product,
// summed over the fields -- what two launches of fe_elemop.h and a multiply compute through two E x Nq arrays in memory per
// field, here without them.
//
// Size rule (weightgrad_supported; family.WEIGHTED_WEIGHT_ADJOINT_RULE in Python): 1 <= Ni, Nj <= 48, 1 <= Nq <= 64, and the
// block's dynamic LDS -- the image of A (ceil(Nq/16) ceil(Nj/4) fragments of 512 bytes), the image of P^T (ceil(Nq/16)
// ceil(Ni/4) fragments) and four wave buffers of max(16 Nj + 2, 16 Ni + 2, 16 (Nq | 1)) doubles, rounded up to even -- at most
// 80 KiB: two blocks per CU.  Every shape of fe_weightedop.h's rule is inside.
//
// Why the product costs nothing.  Both chains, t = A u_k and s = P^T g_k, have Nq rows and the tile's 16 elements as columns:
// accumulator register acc[t][r] of v_mfma_f64_16x16x4_f64 holds row 16 t + 4 r + (lane >> 4), column lane & 15 in both.  The
// product of the two and the sum over the fields are one lane-local fused multiply-add per register.
//
// Schedule.  fe_weightedop.h's.  A wave owns a tile of 16 elements and walks the ITEMS of the tile innermost: u_0, g_0, u_1,
// g_1, ... -- each ONE contiguous span of 16 Nj or 16 Ni doubles, brought by 16-byte non-temporal loads cut at the 16-byte
// boundaries of memory, one item ahead (the next item of this tile, or u_0 of the wave's next tile), and landed in the wave's
// one buffer.  Blocks of four waves walk the tiles statically over a persistent grid of two blocks per CU.  Both operators are
// staged once per block into LDS in A-fragment order, [k step][row tile][lane], padding written as selected zeros, every global
// load issued before the first LDS write; the storage flags change the index used while staging and nothing else.  After the
// last field dW leaves as fe_weightedop.h's output does: transposed through the buffer at stride Nq | 1, read back in memory
// order, the next item LANDED BEFORE the stores are issued (one counter orders loads and stores: section 3q), then 16-byte
// non-temporal stores.
//
// Arithmetic.  t[e, q] is summed k steps ascending, four j per MFMA; s[e, q] likewise, four i per MFMA; dW[e, q] =
// fma(s, t, dW), fields ascending from +0.  B fragments are selected to zero for columns past Nj / Ni and elements past E; rows
// q >= Nq of the accumulators and elements past E are never stored, so nothing else needs selecting.  Entry (e, q) depends on
// column q of P, row q of A, u_k[e, :] and g_k[e, :] only; results are bitwise independent of E, of the tile an element falls
// into and of where the arrays lie.
//
// Template on RQ = ceil(Nq/16) alone (the accumulators of a chain, t kept over the g item, dW: 24 RQ VGPRs): four
// instantiations.  The k steps are bounded by the rule (12: Ni, Nj <= 48), run-time and wave-uniform below that, and ONE chain
// serves both items: the image, the width and the k steps are selected per item.  amdgpu_waves_per_eu(2), no scratch.
#pragma once
#include "../../include/feinsum_hip.h"
#include "fe_common.h"
#include "fe_elemop.h"
#include "fe_weightedop.h"

namespace fe {

constexpr int kWGradThreads = 256;   // four waves per block
constexpr int kWGradWaves = kWGradThreads / 64;
constexpr int kWGradMaxN = 48;       // Ni, Nj
constexpr int kWGradMaxQ = 64;       // Nq
constexpr int kWGradMaxLds = 80 * 1024;
constexpr int kWGradMaxK = kWGradMaxN / 4;   // k steps of either chain

__host__ __device__ constexpr int weightgrad_buffer_doubles(int Ni, int Nq, int Nj) {
    const int u = 16 * Nj + 2, g = 16 * Ni + 2, out = 16 * (Nq | 1);
    const int in = u > g ? u : g;
    return ((in > out ? in : out) + 1) & ~1;
}
__host__ __device__ constexpr int weightgrad_lds_bytes(int Ni, int Nq, int Nj) {
    return (elemop_row_tiles(Nq) * (elemop_k_steps(Nj) + elemop_k_steps(Ni)) * 64
            + kWGradWaves * weightgrad_buffer_doubles(Ni, Nq, Nj)) * (int)sizeof(double);
}
__host__ __device__ constexpr bool weightgrad_supported(int Ni, int Nq, int Nj) {
    return Ni >= 1 && Nq >= 1 && Nj >= 1 && Ni <= kWGradMaxN && Nj <= kWGradMaxN && Nq <= kWGradMaxQ
           && weightgrad_lds_bytes(Ni, Nq, Nj) <= kWGradMaxLds;
}

template <int RQ>
struct WGradGeom {
    static constexpr int KMAX = kWGradMaxK;
    static constexpr int PF = (8 * kWGradMaxN + 1 + 63) / 64;      // 16-byte chunks per lane of a u or g tile (one more for an odd start)
    static constexpr int OC = (8 * 16 * RQ + 1 + 63) / 64;         // ... of a dW tile
    static constexpr int ST = (RQ * KMAX * 64) / kWGradThreads;    // staged doubles per thread and image
};

struct WGradArgs {
    const double* P;   // [Ni][Nq] (pT: [Nq][Ni])
    const double* A;   // [Nq][Nj] (aT: [Nj][Nq])
    double* dW;        // [E][Nq]
    const double* item[2 * kMaxFields];   // item 2 k: u_k [E][Nj];  item 2 k + 1: g_k [E][Ni]
    int64_t E, n_tiles;
    int Ni, Nq, Nj, KI, KJ, nb, pT, aT, buf_doubles;
    unsigned magic_nq;   // ceil(2^20 / Nq): d / Nq = (d magic_nq) >> 20 for every d < 16 (Nq | 1)
};

// Item `it` of the launch, wave-uniform and only known at run time: a select chain over the kernel arguments (field_in's way).
__device__ __forceinline__ const double* wgrad_item(const WGradArgs& g, int it) {
    const double* p = g.item[0];
#pragma unroll
    for (int q = 1; q < 2 * kMaxFields; ++q) p = (it == q) ? g.item[q] : p;
    return p;
}

template <int RQ>
__global__ __launch_bounds__(kWGradThreads) __attribute__((amdgpu_waves_per_eu(2))) void wgrad_kernel(WGradArgs g) {
    using G = WGradGeom<RQ>;
    extern __shared__ __attribute__((aligned(16))) char wgrad_sm[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int Ni = g.Ni, Nq = g.Nq, Nj = g.Nj, KI = g.KI, KJ = g.KJ, n_items = 2 * g.nb;
    double* Af = reinterpret_cast<double*>(wgrad_sm);   // [KJ][RQ][64]: A
    double* Pf = Af + RQ * KJ * 64;                     // [KI][RQ][64]: P^T
    double* buf = Pf + RQ * KI * 64 + wave * g.buf_doubles;
    const int64_t E = g.E, n_tiles = g.n_tiles;
    const int64_t stride = (int64_t)gridDim.x * kWGradWaves;

    // the items of this wave: tile w + 4 blockIdx + 4 gridDim k, and under a tile u_0, g_0, u_1, g_1, ..., innermost
    int64_t tile = (int64_t)blockIdx.x * kWGradWaves + wave;
    int item = 0;

    // the item in flight: its span in registers
    v2d pf[G::PF];
    auto elements = [&](int64_t tl) { return E - tl * 16 < 16 ? (int)(E - tl * 16) : 16; };
    auto width = [&](int it) { return (it & 1) ? Ni : Nj; };
    auto mis_of = [&](int it) { return (int)((reinterpret_cast<uintptr_t>(wgrad_item(g, it)) >> 3) & 1); };
    auto request = [&](int it, int64_t tl, int ln) {
        const int n = width(it);
        elemop_load_span<G::PF>(wgrad_item(g, it) + tl * 16 * n, elements(tl) * n, mis_of(it), ln, pf);
    };
    auto land = [&](int it, int64_t tl, int ln) { wtop_land_span<G::PF>(buf, elements(tl) * width(it), mis_of(it), ln, pf); };
    const bool any = tile < n_tiles;
    if (any) request(0, tile, lane);

    // ---- both operators -> LDS in fragment order (the storage flags only change the index; the padding is written, not
    // read).  Every load is issued before the first LDS write, so that their latencies overlap
    {
        const int na = RQ * KJ * 64, np = RQ * KI * 64;
        double sa[G::ST], sp[G::ST];
#pragma unroll
        for (int k = 0; k < G::ST; ++k) {
            const int idx = tid + k * kWGradThreads;
            const int ks = idx / (RQ * 64), rem = idx - ks * (RQ * 64);
            const int t = rem >> 6, l = rem & 63;
            const int q = 16 * t + (l & 15), j = 4 * ks + (l >> 4);
            double v = 0.0;
            if (idx < na && q < Nq && j < Nj) v = g.A[g.aT ? j * Nq + q : q * Nj + j];
            sa[k] = v;
        }
#pragma unroll
        for (int k = 0; k < G::ST; ++k) {
            const int idx = tid + k * kWGradThreads;
            const int ks = idx / (RQ * 64), rem = idx - ks * (RQ * 64);
            const int t = rem >> 6, l = rem & 63;
            const int q = 16 * t + (l & 15), i = 4 * ks + (l >> 4);
            double v = 0.0;
            if (idx < np && q < Nq && i < Ni) v = g.P[g.pT ? q * Ni + i : i * Nq + q];
            sp[k] = v;
        }
#pragma unroll
        for (int k = 0; k < G::ST; ++k) {
            const int idx = tid + k * kWGradThreads;
            if (idx < na) Af[idx] = sa[k];
        }
#pragma unroll
        for (int k = 0; k < G::ST; ++k) {
            const int idx = tid + k * kWGradThreads;
            if (idx < np) Pf[idx] = sp[k];
        }
    }
    if (any) land(0, tile, lane);
    __syncthreads();

    const int So = Nq | 1;
    v4d tq[RQ], dw[RQ];   // t = A u_k of the field whose g item comes next; dW of the tile so far
#pragma unroll
    for (int t = 0; t < RQ; ++t) tq[t] = dw[t] = v4d{0.0, 0.0, 0.0, 0.0};
    while (tile < n_tiles) {
        // The lane number, opaque to the compiler once per phase (fe_weightedop.h: left loop-invariant, everything derived
        // from it is hoisted in front of the loop and held in registers across it)
        auto fresh_lane = [&] {
            int ln = lane;
            asm volatile("" : "+v"(ln));
            return ln;
        };
        int ln = fresh_lane();
        const int c = ln & 15, h = ln >> 4;
        const bool is_g = (item & 1) != 0;
        const int N = is_g ? Ni : Nj, K = is_g ? KI : KJ;
        const double* ar = (is_g ? Pf : Af) + ln;
        const int ne = elements(tile);
        const bool ok = c < ne;

        // ---- all B fragments of the item into registers; elements past E and columns past its width are selected to zero
        // (the reads are unconditional, at an address inside the tile: they issue back to back)
        const int mis = mis_of(item);
        double bf[G::KMAX];
#pragma unroll
        for (int ks = 0; ks < G::KMAX; ++ks) {
            const int j = 4 * ks + h;
            const bool valid = ok && j < N;
            const double v = buf[valid ? c * N + j + mis : 0];
            bf[ks] = valid ? v : 0.0;
        }
        wave_lds_fence();

        // ---- the next item of this wave on the way while this one is computed
        const bool last = item + 1 == n_items;
        const int item_n = last ? 0 : item + 1;
        const int64_t tile_n = last ? tile + stride : tile;
        const bool more = tile_n < n_tiles;
        if (more) request(item_n, tile_n, ln);

        // ---- the chain of the item, A u_k or P^T g_k: the fragments of k step ks + 1 are read while the MFMAs of ks run
        v4d acc[RQ];
        {
            double a_cur[RQ];
#pragma unroll
            for (int t = 0; t < RQ; ++t) {
                acc[t] = v4d{0.0, 0.0, 0.0, 0.0};
                a_cur[t] = ar[t * 64];
            }
#pragma unroll
            for (int ks = 0; ks < G::KMAX; ++ks) {
                if (ks < K) {   // (wave-uniform; not a `break`: the loop must unroll so that bf[] stays in registers)
                    const int nx = ks + 1 < K ? ks + 1 : ks;
                    double a_nxt[RQ];
#pragma unroll
                    for (int t = 0; t < RQ; ++t) a_nxt[t] = ar[(nx * RQ + t) * 64];
#pragma unroll
                    for (int t = 0; t < RQ; ++t) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a_cur[t], bf[ks], acc[t], 0, 0, 0);
#pragma unroll
                    for (int t = 0; t < RQ; ++t) a_cur[t] = a_nxt[t];
                }
            }
        }

        // ---- u_k: keep t.  g_k: the product and the sum over the fields, lane-local -- both chains have one layout
        if (!is_g) {
#pragma unroll
            for (int t = 0; t < RQ; ++t) tq[t] = acc[t];
        } else {
#pragma unroll
            for (int t = 0; t < RQ; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) dw[t][r] = __builtin_fma(acc[t][r], tq[t][r], dw[t][r]);
        }

        if (!last) {
            // (the buffer is free since the B fragments were lifted)
            if (more) land(item_n, tile_n, fresh_lane());
            wave_lds_fence();
        } else {
            // ---- transposition through the buffer, rows So apart; the dW span comes back into registers in the order it
            // has in memory.  Rows q >= Nq are not written, columns past E not read back
            ln = fresh_lane();
#pragma unroll
            for (int t = 0; t < RQ; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int q = 16 * t + (ln >> 4) + 4 * r;
                    if (q < Nq) buf[(ln & 15) * So + q] = dw[t][r];
                    dw[t][r] = 0.0;
                }
            wave_lds_fence();
            const int n = ne * Nq;
            const int mo = (int)((reinterpret_cast<uintptr_t>(g.dW) >> 3) & 1);
            const int n_chunks = (n + mo + 1) >> 1;
            auto held = [&](int d) {   // double d of the dW span, 0 <= d < n
                const int row = (int)(((unsigned)d * g.magic_nq) >> 20);
                return buf[row * So + (d - row * Nq)];
            };
            v2d oc[G::OC];
#pragma unroll
            for (int cc = 0; cc < G::OC; ++cc) {
                const int d0 = 2 * (cc * 64 + ln) - mo, d1 = d0 + 1;
                if (cc * 64 < n_chunks) oc[cc] = v2d{held(d0 < 0 ? 0 : d0 < n ? d0 : n - 1), held(d1 < n ? d1 : n - 1)};
            }
            wave_lds_fence();
            // ---- the next item lands in the buffer BEFORE these stores are issued: the wait for its loads is then not a wait
            // for the stores (one counter orders both), and the stores fly while the next item is computed
            if (more) land(item_n, tile_n, fresh_lane());
            wave_lds_fence();
            double* span = g.dW + tile * 16 * Nq;
            ln = fresh_lane();
#pragma unroll
            for (int cc = 0; cc < G::OC; ++cc) {
                const int q = cc * 64 + ln;
                if (cc * 64 < n_chunks && q < n_chunks) {
                    const int d0 = 2 * q - mo, d1 = d0 + 1;
                    if (d0 >= 0 && d1 < n) {
                        __builtin_nontemporal_store(oc[cc], reinterpret_cast<v2d*>(span + d0));
                    } else {
                        if (d0 >= 0) __builtin_nontemporal_store(oc[cc][0], span + d0);
                        if (d1 < n) __builtin_nontemporal_store(oc[cc][1], span + d1);
                    }
                }
            }
        }
        item = item_n;
        tile = tile_n;
    }
}

}  // namespace fe
