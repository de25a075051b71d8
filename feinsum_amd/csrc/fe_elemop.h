// fe_elemop.h -- the element-local operator of any shape on the matrix cores:
//
//   out_k[e, i] = sum_j A[i, j] u_k[e, j]                 A [Ni][Nj], or stored [Nj][Ni] with opT; k < nb fields
//   out_k[e, i] = J[e] * (sum_j A[i, j] u_k[e, j])        with J: ONE MORE ROUNDING than the sum -- the factor is applied to
//                                                          the finished sum, lane-locally (the MFMA column is the element)
//
// Size rule (elemop_supported; family.ELEMENT_OPERATOR_RULE in Python): 1 <= Ni, Nj <= 96 and RT KS <= 64, RT = ceil(Ni / 16)
// row tiles, KS = ceil(Nj / 4) k steps -- the operator image of RT KS 512 bytes is at most 32 KiB, and with the four wave
// buffers a block stays under 80 KiB: two blocks per CU.
//
// Schedule.  A wave owns a tile of 16 elements; blocks of four waves walk the (field, tile) pairs statically over a persistent
// grid of two blocks per CU.  The operator is staged into LDS once per block in the A-fragment order of v_mfma_f64_16x16x4_f64,
// [k step][row tile][lane], rows and columns past the shape written as zeros (selected, never read): each lane reads its
// fragment with one conflict-free 8-byte LDS read per MFMA, the fragments of k step ks + 1 while the MFMAs of ks run.  A tile
// of u is ONE contiguous span of 16 Nj doubles: it comes by 16-byte non-temporal loads into registers -- one tile ahead, issued
// in front of the MFMAs of the tile before -- and goes into the wave's LDS buffer as it lies in memory.  A span starts 0 or 8 bytes past a 16-byte boundary
// (the arrays are 8-byte aligned and no more): the chunks are cut at the 16-byte boundaries of MEMORY, so an odd start leaves
// one scalar double at the head and one at the tail.  All KS B fragments are lifted from the buffer into registers (lane l:
// element l & 15, k = 4 ks + (l >> 4)), which frees it: the accumulators (row tile t, register q: row 16 t + (l >> 4) + 4 q,
// column l & 15) are transposed through the same buffer, rows Ni | 1 doubles apart (an odd stride: the 16 lanes of a store group
// fall on 16 different banks), come back into registers in memory order, and leave as one contiguous span of 16 Ni doubles by
// 16-byte non-temporal stores, cut like the loads.  The NEXT tile is written into the buffer between that read-back and the
// stores: one counter (vmcnt) orders loads and stores, the chunk counts are run-time, so the compiler's wait for the prefetched
// loads is a wait for everything older -- placed there it finds no store of this tile, and the stores fly under the next MFMAs.
// The last tile of an array (and E < 16) runs through the same code: its loads and stores are guarded entry by entry, and the
// B values of elements past E -- like those of columns past Nj -- are SELECTED to zero, so that nothing behind an array's
// end is read and no NaN there could reach a result.
//
// Arithmetic.  Entry (e, i) is summed k steps ascending, four j per MFMA; it depends on A's row i, u's row e and J[e] only:
// bitwise reproducible, whatever E, the tile an element falls into, where the arrays lie, and the number of fields.
//
// Template on RT alone (the accumulators: 8 VGPRs per row tile); Ni, Nj, KS, the presence of J and opT are run-time and
// wave-uniform.  RT fixes the largest KS of the rule, 64 / RT (at most 24), hence the registers of the B fragments, of the
// prefetched tile and of the output tile.  amdgpu_waves_per_eu(2): the residency the persistent grid assumes (no scratch).
#pragma once
#include "../../include/feinsum_hip.h"
#include "fe_common.h"

namespace fe {

constexpr int kElemOpThreads = 256;   // four waves per block
constexpr int kElemOpWaves = kElemOpThreads / 64;
constexpr int kElemOpMaxN = 96;
constexpr int kElemOpMaxFragments = 64;   // RT KS

__host__ __device__ constexpr int elemop_row_tiles(int Ni) { return (Ni + 15) / 16; }
__host__ __device__ constexpr int elemop_k_steps(int Nj) { return (Nj + 3) / 4; }
__host__ __device__ constexpr bool elemop_supported(int Ni, int Nj) {
    return Ni >= 1 && Nj >= 1 && Ni <= kElemOpMaxN && Nj <= kElemOpMaxN
           && elemop_row_tiles(Ni) * elemop_k_steps(Nj) <= kElemOpMaxFragments;
}
// doubles of a wave's buffer: a u tile as it lies in memory behind at most one double of head (and one of tail), or the
// output tile in rows of Ni | 1; even, so that every buffer starts on a 16-byte boundary
__host__ __device__ constexpr int elemop_buffer_doubles(int Ni, int Nj) {
    const int in = 16 * Nj + 2, out = 16 * (Ni | 1);
    return ((in > out ? in : out) + 1) & ~1;
}
__host__ __device__ constexpr int elemop_lds_bytes(int Ni, int Nj) {
    return (elemop_row_tiles(Ni) * elemop_k_steps(Nj) * 64 + kElemOpWaves * elemop_buffer_doubles(Ni, Nj)) * (int)sizeof(double);
}

template <int RT>
struct ElemOpGeom {
    static constexpr int KSMAX = kElemOpMaxFragments / RT < kElemOpMaxN / 4 ? kElemOpMaxFragments / RT : kElemOpMaxN / 4;
    static constexpr int NJMAX = 4 * KSMAX;
    static constexpr int PF = (8 * NJMAX + 1 + 63) / 64;   // 16-byte chunks per lane of a u tile (one more chunk for an odd start)
    static constexpr int NIMAX = 16 * RT < kElemOpMaxN ? 16 * RT : kElemOpMaxN;
    static constexpr int OC = (8 * NIMAX + 1 + 63) / 64;   // ... and of an output tile
};

struct ElemOpArgs {
    const double* J;   // [E], or null
    const double* A;   // [Ni][Nj] (opT: [Nj][Ni])
    FieldPtrs f;       // v[k]: u_k [E][Nj];  out[k]: out_k [E][Ni]
    int64_t E, n_tiles;
    int Ni, Nj, KS, nb, opT, buf_doubles;
    unsigned magic_ni;   // ceil(2^20 / Ni): d / Ni = (d magic_ni) >> 20 for every d < 16 (Ni | 1)
};

// The chunks of the span [span, span + n) into registers: chunk q holds the doubles 2 q - mis and 2 q - mis + 1 of the span
// (mis: the span starts 8 bytes past a 16-byte boundary), zero where the span has none.
template <int PF>
__device__ __forceinline__ void elemop_load_span(const double* span, int n, int mis, int lane, v2d (&pf)[PF]) {
    const int n_chunks = (n + mis + 1) >> 1;
#pragma unroll
    for (int cc = 0; cc < PF; ++cc) {
        v2d v = v2d{0.0, 0.0};
        const int q = cc * 64 + lane;
        if (cc * 64 < n_chunks && q < n_chunks) {
            const int d0 = 2 * q - mis, d1 = d0 + 1;
            if (d0 >= 0 && d1 < n) {
                v = __builtin_nontemporal_load(reinterpret_cast<const v2d*>(span + d0));
            } else {
                if (d0 >= 0) v[0] = __builtin_nontemporal_load(span + d0);
                if (d1 < n) v[1] = __builtin_nontemporal_load(span + d1);
            }
        }
        pf[cc] = v;
    }
}

template <int RT>
__global__ __launch_bounds__(kElemOpThreads) __attribute__((amdgpu_waves_per_eu(2))) void elemop_kernel(ElemOpArgs g) {
    using G = ElemOpGeom<RT>;
    extern __shared__ __attribute__((aligned(16))) char elemop_sm[];
    double* Af = reinterpret_cast<double*>(elemop_sm);   // [KS][RT][64]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int Ni = g.Ni, Nj = g.Nj, KS = g.KS, nb = g.nb;
    double* buf = Af + RT * KS * 64 + wave * g.buf_doubles;
    const int c = lane & 15, h = lane >> 4;
    const int64_t E = g.E, n_tiles = g.n_tiles;
    const int64_t stride = (int64_t)gridDim.x * kElemOpWaves;
    const bool with_j = g.J != nullptr;

    // the (field, tile) pairs of this wave: pair w + 4 blockIdx + 4 gridDim k of the nb n_tiles pairs, fields outermost
    int field = 0;
    int64_t tile = (int64_t)blockIdx.x * kElemOpWaves + wave;
    while (field < nb && tile >= n_tiles) { tile -= n_tiles; ++field; }

    // the tile in flight: its u span in registers and its J (the element of this lane's MFMA column)
    v2d pf[G::PF];
    double jn = 0.0;
    auto request = [&](int fld, int64_t tl) {
        const double* u = field_in(g.f, fld);
        const int64_t e0 = tl * 16;
        const int ne = E - e0 < 16 ? (int)(E - e0) : 16;
        elemop_load_span<G::PF>(u + e0 * Nj, ne * Nj, (int)((reinterpret_cast<uintptr_t>(u) >> 3) & 1), lane, pf);
        jn = (with_j && c < ne) ? g.J[e0 + c] : 0.0;
    };
    // ... into the wave's buffer, as it lies in memory (double d of the span at buf[d + mis])
    auto land = [&](int fld, int64_t tl) {
        const int64_t e0 = tl * 16;
        const int ne = E - e0 < 16 ? (int)(E - e0) : 16;
        const int mis = (int)((reinterpret_cast<uintptr_t>(field_in(g.f, fld)) >> 3) & 1);
        const int n_chunks = (ne * Nj + mis + 1) >> 1;
#pragma unroll
        for (int cc = 0; cc < G::PF; ++cc) {
            const int q = cc * 64 + lane;
            if (cc * 64 < n_chunks && q < n_chunks) *reinterpret_cast<v2d*>(buf + 2 * q) = pf[cc];
        }
    };
    if (field < nb) request(field, tile);

    // ---- operator -> LDS in fragment order (opT only changes the index; the padding is written, not read).  Every load is
    // issued before the first LDS write, so that their latencies overlap (fe_common.h, stage_operator)
    {
        constexpr int kPer = kElemOpMaxFragments * 64 / kElemOpThreads;
        const int n = RT * KS * 64;
        double staged[kPer];
#pragma unroll
        for (int k = 0; k < kPer; ++k) {
            const int idx = tid + k * kElemOpThreads;
            const int ks = idx / (RT * 64), rem = idx - ks * (RT * 64);
            const int t = rem >> 6, l = rem & 63;
            const int i = 16 * t + (l & 15), j = 4 * ks + (l >> 4);
            double v = 0.0;
            if (idx < n && i < Ni && j < Nj) v = g.A[g.opT ? j * Ni + i : i * Nj + j];
            staged[k] = v;
        }
#pragma unroll
        for (int k = 0; k < kPer; ++k) {
            const int idx = tid + k * kElemOpThreads;
            if (idx < n) Af[idx] = staged[k];
        }
    }
    if (field < nb) land(field, tile);
    __syncthreads();

    const int So = Ni | 1;
    const double* ar = Af + lane;
    while (field < nb) {
        double* out = field_out(g.f, field);
        const int64_t e0 = tile * 16;
        const int ne = E - e0 < 16 ? (int)(E - e0) : 16;
        const bool ok = c < ne;
        const double jv = jn;

        // ---- all B fragments into registers; elements past E and columns past Nj are selected to zero (the reads are
        // unconditional, at an address inside the tile: they issue back to back)
        const int mis = (int)((reinterpret_cast<uintptr_t>(field_in(g.f, field)) >> 3) & 1);
        double bf[G::KSMAX];
#pragma unroll
        for (int ks = 0; ks < G::KSMAX; ++ks) {
            const int j = 4 * ks + h;
            const bool valid = ok && j < Nj;
            const double v = buf[valid ? c * Nj + j + mis : 0];
            bf[ks] = valid ? v : 0.0;
        }
        wave_lds_fence();

        // ---- the next pair of this wave, and its tile on the way while this one is computed
        int field_n = field;
        int64_t tile_n = tile + stride;
        while (field_n < nb && tile_n >= n_tiles) { tile_n -= n_tiles; ++field_n; }
        if (field_n < nb) request(field_n, tile_n);

        // ---- the A fragments of k step ks + 1 are read while the MFMAs of ks run (the last step reads its own again)
        v4d acc[RT];
        double a_cur[RT];
#pragma unroll
        for (int t = 0; t < RT; ++t) {
            acc[t] = v4d{0.0, 0.0, 0.0, 0.0};
            a_cur[t] = ar[t * 64];
        }
#pragma unroll
        for (int ks = 0; ks < G::KSMAX; ++ks) {
            if (ks < KS) {   // (wave-uniform; not a `break`: the loop must unroll so that bf[] stays in registers)
                const int nx = ks + 1 < KS ? ks + 1 : ks;
                double a_nxt[RT];
#pragma unroll
                for (int t = 0; t < RT; ++t) a_nxt[t] = ar[(nx * RT + t) * 64];
#pragma unroll
                for (int t = 0; t < RT; ++t) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a_cur[t], bf[ks], acc[t], 0, 0, 0);
#pragma unroll
                for (int t = 0; t < RT; ++t) a_cur[t] = a_nxt[t];
            }
        }
        if (with_j) {
#pragma unroll
            for (int t = 0; t < RT; ++t) acc[t] *= jv;
        }

        // ---- transposition through the buffer (free: every B fragment is in registers), rows So apart; the output span
        // comes back into registers in the order it has in memory
#pragma unroll
        for (int t = 0; t < RT; ++t)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int i = 16 * t + h + 4 * q;
                if (i < Ni) buf[c * So + i] = acc[t][q];
            }
        wave_lds_fence();
        const int n = ne * Ni;
        const int mo = (int)((reinterpret_cast<uintptr_t>(out) >> 3) & 1);
        const int n_chunks = (n + mo + 1) >> 1;
        auto held = [&](int d) {   // double d of the output span, 0 <= d < n
            const int row = (int)(((unsigned)d * g.magic_ni) >> 20);
            return buf[row * So + (d - row * Ni)];
        };
        v2d oc[G::OC];
#pragma unroll
        for (int cc = 0; cc < G::OC; ++cc) {
            const int d0 = 2 * (cc * 64 + lane) - mo, d1 = d0 + 1;
            if (cc * 64 < n_chunks) oc[cc] = v2d{held(d0 < 0 ? 0 : d0 < n ? d0 : n - 1), held(d1 < n ? d1 : n - 1)};
        }
        wave_lds_fence();
        // ---- the next tile lands in the buffer BEFORE this tile's stores are issued: the wait for its loads is then not
        // a wait for these stores (one counter orders both), and the stores fly while the next tile is computed
        if (field_n < nb) land(field_n, tile_n);
        wave_lds_fence();
        double* span = out + e0 * Ni;
#pragma unroll
        for (int cc = 0; cc < G::OC; ++cc) {
            const int q = cc * 64 + lane;
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
        field = field_n;
        tile = tile_n;
    }
}

}  // namespace fe
