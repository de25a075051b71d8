// fe_weightedop.h -- the weighted element operator in one matrix-core kernel:
//
//   out_k[e, i] = sum_q P[i, q] W[e, q] (sum_j A[q, j] u_k[e, j])        einsum iq,eq,qj,ej->ei; k < nb fields
//
// P [Ni][Nq] (stored [Nq][Ni] with FE_WO_P_T), A [Nq][Nj] (stored [Nj][Nq] with FE_WO_A_T), W [E][Nq], u_k [E][Nj],
// out_k [E][Ni]: interpolation to a quadrature grid, a pointwise weight per element and point, projection back -- the two
// halves fe_elemop.h runs as two launches with a multiply between them, here without the E x Nq arrays in memory.
//
// Size rule (weightedop_supported; family.WEIGHTED_ELEMENT_OPERATOR_RULE in Python): 1 <= Ni, Nj <= 48, 1 <= Nq <= 64, and the
// block's dynamic LDS -- the image of A (ceil(Nq/16) ceil(Nj/4) fragments of 512 bytes), the image of P (ceil(Ni/16) ceil(Nq/4)
// fragments) and four wave buffers of max(16 Nj + 2, 16 Nq + 2, 16 (Ni | 1)) doubles, rounded up to even -- at most 80 KiB: two
// blocks per CU.
//
// Why the fusion costs nothing.  Accumulator register acc[t][r] of v_mfma_f64_16x16x4_f64 holds row 16 t + 4 r + (lane >> 4),
// column lane & 15.  The B fragment of k step ks holds k = 4 ks + (lane >> 4), element lane & 15.  With ks = 4 t + r these are
// the same: the accumulators of the first product ARE the B operands of the second, register for register, and W[e, q] in that
// layout is what a wave lifts from its LDS buffer like a u fragment.  Between the two MFMA chains stands one lane-local multiply.
//
// Schedule.  fe_elemop.h's, with a second staged operator and a second input span.  A wave owns a tile of 16 elements and walks
// its FIELDS INNERMOST: the W fragments of a tile are lifted once and stay in registers over the nb fields of that tile, so a
// launch reads W once per tile, not once per field -- 8 (nb (Ni + Nj) + Nq) E bytes in all.  Blocks of four waves walk the tiles
// statically over a persistent grid of two blocks per CU.  Both operators are staged once per block into LDS in A-fragment order,
// [k step][row tile][lane], padding written as selected zeros, every global load issued before the first LDS write; the storage
// flags change the index used while staging and nothing else.  A tile of u (16 Nj doubles) and a tile of W (16 Nq doubles) are
// each ONE contiguous span: they come by 16-byte non-temporal loads cut at the 16-byte boundaries of memory, one item ahead
// (the next field of this tile, or field 0 and W of the wave's next tile), and land in the wave's one buffer -- W first, lifted
// at once into registers, then u over it.  The output leaves as in fe_elemop.h: transposed through the buffer at stride Ni | 1,
// read back in memory order, the next item LANDED BEFORE this item's stores are issued (one counter orders loads and stores:
// section 3q), then 16-byte non-temporal stores.
//
// Arithmetic.  t[e, q] is summed k steps ascending, four j per MFMA; s = W t costs one rounding; out[e, i] is summed k steps
// ascending over q, four q per MFMA.  Between the products s = valid ? W t : 0, valid: q < Nq and e < E -- SELECTED, not multiplied
// by zero: a padded row of A's image times a NaN of u is a NaN, and it must not reach the second chain.  Entry (e, i) depends
// on row i of P, on A, on u_k[e, :] and on W[e, :] only; results are bitwise independent of E, of the tile an element falls
// into, of where the arrays lie and of the number of fields.
//
// Template on the row-tile counts of the two products, RQ = ceil(Nq/16) (accumulators of the first, W fragments, k steps of
// the second: 4 RQ) and RI = ceil(Ni/16) (accumulators of the second, the output tile): twelve instantiations, each unrolled for
// its own tile counts.  The k steps of the first product are bounded by the rule alone (12: Nj <= 48), run-time and wave-uniform
// below that; registers did not ask for a template parameter there (DESIGN.md section 3r has the table: 118 to 247 VGPRs).
// amdgpu_waves_per_eu(2), no scratch.
#pragma once
#include "../../include/feinsum_hip.h"
#include "fe_common.h"
#include "fe_elemop.h"

namespace fe {

constexpr int kWtOpThreads = 256;   // four waves per block
constexpr int kWtOpWaves = kWtOpThreads / 64;
constexpr int kWtOpMaxN = 48;       // Ni, Nj
constexpr int kWtOpMaxQ = 64;       // Nq
constexpr int kWtOpMaxLds = 80 * 1024;
constexpr int kWtOpMaxKJ = kWtOpMaxN / 4;   // k steps of the first product

__host__ __device__ constexpr int weightedop_buffer_doubles(int Ni, int Nq, int Nj) {
    const int u = 16 * Nj + 2, w = 16 * Nq + 2, out = 16 * (Ni | 1);
    const int in = u > w ? u : w;
    return ((in > out ? in : out) + 1) & ~1;
}
__host__ __device__ constexpr int weightedop_lds_bytes(int Ni, int Nq, int Nj) {
    return ((elemop_row_tiles(Nq) * elemop_k_steps(Nj) + elemop_row_tiles(Ni) * elemop_k_steps(Nq)) * 64
            + kWtOpWaves * weightedop_buffer_doubles(Ni, Nq, Nj)) * (int)sizeof(double);
}
__host__ __device__ constexpr bool weightedop_supported(int Ni, int Nq, int Nj) {
    return Ni >= 1 && Nq >= 1 && Nj >= 1 && Ni <= kWtOpMaxN && Nj <= kWtOpMaxN && Nq <= kWtOpMaxQ
           && weightedop_lds_bytes(Ni, Nq, Nj) <= kWtOpMaxLds;
}

template <int RQ, int RI>
struct WtOpGeom {
    static constexpr int KJMAX = kWtOpMaxKJ;
    static constexpr int KQMAX = 4 * RQ;                          // k steps of the second product: one per accumulator register
    static constexpr int PFU = (8 * kWtOpMaxN + 1 + 63) / 64;     // 16-byte chunks per lane of a u tile (one more for an odd start)
    static constexpr int PFW = (8 * 16 * RQ + 1 + 63) / 64;       // ... of a W tile
    static constexpr int OC = (8 * 16 * RI + 1 + 63) / 64;        // ... of an output tile
    static constexpr int SA = (RQ * KJMAX * 64) / kWtOpThreads;   // staged doubles per thread: A's image
    static constexpr int SP = (RI * KQMAX * 64) / kWtOpThreads;   // ... P's image
};

struct WtOpArgs {
    const double* P;   // [Ni][Nq] (pT: [Nq][Ni])
    const double* W;   // [E][Nq]
    const double* A;   // [Nq][Nj] (aT: [Nj][Nq])
    FieldPtrs f;       // v[k]: u_k [E][Nj];  out[k]: out_k [E][Ni]
    int64_t E, n_tiles;
    int Ni, Nq, Nj, KJ, KQ, nb, pT, aT, buf_doubles;
    unsigned magic_ni;   // ceil(2^20 / Ni): d / Ni = (d magic_ni) >> 20 for every d < 16 (Ni | 1)
};

// The chunks in registers into the wave's buffer, as the span lies in memory (double d of the span at buf[d + mis]).
template <int PF>
__device__ __forceinline__ void wtop_land_span(double* buf, int n, int mis, int lane, const v2d (&pf)[PF]) {
    const int n_chunks = (n + mis + 1) >> 1;
#pragma unroll
    for (int cc = 0; cc < PF; ++cc) {
        const int q = cc * 64 + lane;
        if (cc * 64 < n_chunks && q < n_chunks) *reinterpret_cast<v2d*>(buf + 2 * q) = pf[cc];
    }
}

template <int RQ, int RI>
__global__ __launch_bounds__(kWtOpThreads) __attribute__((amdgpu_waves_per_eu(2))) void weightedop_kernel(WtOpArgs g) {
    using G = WtOpGeom<RQ, RI>;
    extern __shared__ __attribute__((aligned(16))) char wtop_sm[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int Ni = g.Ni, Nq = g.Nq, Nj = g.Nj, KJ = g.KJ, KQ = g.KQ, nb = g.nb;
    double* Af = reinterpret_cast<double*>(wtop_sm);   // [KJ][RQ][64]
    double* Pf = Af + RQ * KJ * 64;                    // [KQ][RI][64]
    double* buf = Pf + RI * KQ * 64 + wave * g.buf_doubles;
    const int64_t E = g.E, n_tiles = g.n_tiles;
    const int64_t stride = (int64_t)gridDim.x * kWtOpWaves;
    const int mis_w = (int)((reinterpret_cast<uintptr_t>(g.W) >> 3) & 1);

    // the items of this wave: tile w + 4 blockIdx + 4 gridDim k, and under a tile its nb fields, innermost
    int64_t tile = (int64_t)blockIdx.x * kWtOpWaves + wave;
    int field = 0;

    // the item in flight: its u span and, where it opens a tile, that tile's W span, in registers
    v2d pfu[G::PFU], pfw[G::PFW];
    auto elements = [&](int64_t tl) { return E - tl * 16 < 16 ? (int)(E - tl * 16) : 16; };
    auto mis_of = [&](int fld) { return (int)((reinterpret_cast<uintptr_t>(field_in(g.f, fld)) >> 3) & 1); };
    auto request = [&](int fld, int64_t tl, int ln) {
        elemop_load_span<G::PFU>(field_in(g.f, fld) + tl * 16 * Nj, elements(tl) * Nj, mis_of(fld), ln, pfu);
    };
    auto request_w = [&](int64_t tl, int ln) { elemop_load_span<G::PFW>(g.W + tl * 16 * Nq, elements(tl) * Nq, mis_w, ln, pfw); };
    // W fragment ks of the tile in the buffer: W[e0 + c][4 ks + h], selected to zero past Nq and past E
    double wf[G::KQMAX];
    auto land = [&](int fld, int64_t tl, int ln) {
        const int ne = elements(tl);
        const int c = ln & 15, h = ln >> 4;
        if (fld == 0) {
            wtop_land_span<G::PFW>(buf, ne * Nq, mis_w, ln, pfw);
            wave_lds_fence();
#pragma unroll
            for (int ks = 0; ks < G::KQMAX; ++ks) {
                const int q = 4 * ks + h;
                const bool valid = c < ne && q < Nq;
                const double v = buf[valid ? c * Nq + q + mis_w : 0];
                wf[ks] = valid ? v : 0.0;
            }
            wave_lds_fence();
        }
        wtop_land_span<G::PFU>(buf, ne * Nj, mis_of(fld), ln, pfu);
    };
    const bool any = tile < n_tiles;
    if (any) request(0, tile, lane), request_w(tile, lane);

    // ---- both operators -> LDS in fragment order (the storage flags only change the index; the padding is written, not
    // read).  Every load is issued before the first LDS write, so that their latencies overlap
    {
        const int na = RQ * KJ * 64, np = RI * KQ * 64;
        double sa[G::SA], sp[G::SP];
#pragma unroll
        for (int k = 0; k < G::SA; ++k) {
            const int idx = tid + k * kWtOpThreads;
            const int ks = idx / (RQ * 64), rem = idx - ks * (RQ * 64);
            const int t = rem >> 6, l = rem & 63;
            const int q = 16 * t + (l & 15), j = 4 * ks + (l >> 4);
            double v = 0.0;
            if (idx < na && q < Nq && j < Nj) v = g.A[g.aT ? j * Nq + q : q * Nj + j];
            sa[k] = v;
        }
#pragma unroll
        for (int k = 0; k < G::SP; ++k) {
            const int idx = tid + k * kWtOpThreads;
            const int ks = idx / (RI * 64), rem = idx - ks * (RI * 64);
            const int t = rem >> 6, l = rem & 63;
            const int i = 16 * t + (l & 15), q = 4 * ks + (l >> 4);
            double v = 0.0;
            if (idx < np && i < Ni && q < Nq) v = g.P[g.pT ? q * Ni + i : i * Nq + q];
            sp[k] = v;
        }
#pragma unroll
        for (int k = 0; k < G::SA; ++k) {
            const int idx = tid + k * kWtOpThreads;
            if (idx < na) Af[idx] = sa[k];
        }
#pragma unroll
        for (int k = 0; k < G::SP; ++k) {
            const int idx = tid + k * kWtOpThreads;
            if (idx < np) Pf[idx] = sp[k];
        }
    }
    if (any) land(0, tile, lane);
    __syncthreads();

    const int So = Ni | 1;
    while (tile < n_tiles) {
        // The lane number, opaque to the compiler once per phase: what it derives from it -- the LDS addresses and masks of the
        // fragments, the chunk indices of the spans -- is then computed where it is used.  Left loop-invariant, all of it is
        // hoisted in front of the loop and held in registers across it, which alone costs more than two waves per SIMD leave.
        auto fresh_lane = [&] {
            int ln = lane;
            asm volatile("" : "+v"(ln));
            return ln;
        };
        int ln = fresh_lane();
        const int c = ln & 15, h = ln >> 4;
        const double* ar = Af + ln;
        double* out = field_out(g.f, field);
        const int64_t e0 = tile * 16;
        const int ne = elements(tile);
        const bool ok = c < ne;

        // ---- all B fragments of u into registers; elements past E and columns past Nj are selected to zero (the reads are
        // unconditional, at an address inside the tile: they issue back to back)
        const int mis = mis_of(field);
        double bf[G::KJMAX];
#pragma unroll
        for (int ks = 0; ks < G::KJMAX; ++ks) {
            const int j = 4 * ks + h;
            const bool valid = ok && j < Nj;
            const double v = buf[valid ? c * Nj + j + mis : 0];
            bf[ks] = valid ? v : 0.0;
        }
        wave_lds_fence();

        // ---- the next item of this wave on the way while this one is computed
        const int field_n = field + 1 < nb ? field + 1 : 0;
        const int64_t tile_n = field + 1 < nb ? tile : tile + stride;
        const bool more = tile_n < n_tiles;
        if (more) request(field_n, tile_n, ln);

        // ---- first product, t = A u: the A fragments of k step ks + 1 are read while the MFMAs of ks run
        v4d acc[RQ];
        {
            double a_cur[RQ];
#pragma unroll
            for (int t = 0; t < RQ; ++t) {
                acc[t] = v4d{0.0, 0.0, 0.0, 0.0};
                a_cur[t] = ar[t * 64];
            }
#pragma unroll
            for (int ks = 0; ks < G::KJMAX; ++ks) {
                if (ks < KJ) {   // (wave-uniform; not a `break`: the loop must unroll so that bf[] stays in registers)
                    const int nx = ks + 1 < KJ ? ks + 1 : ks;
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

        // (the W span of a new tile is asked for here, not with its u span: in front of the first chain its registers would be
        // live beside the u fragments, the accumulators and this tile's W fragments, more than two waves per SIMD leave)
        if (more && field_n == 0) request_w(tile_n, ln);

        // ---- the weight, lane-local: accumulator register r of row tile t is the B fragment of k step 4 t + r.  Selected:
        // a padded row (q >= Nq) or an element past E carries exactly zero into the second chain, whatever t holds there
        double sf[G::KQMAX];
#pragma unroll
        for (int t = 0; t < RQ; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int ks = 4 * t + r;
                const bool valid = ok && 4 * ks + h < Nq;
                const double s = wf[ks] * acc[t][r];
                sf[ks] = valid ? s : 0.0;
            }

        // ---- second product, out = P s
        v4d res[RI];
        {
            const double* pr = Pf + ln;
            double p_cur[RI];
#pragma unroll
            for (int t = 0; t < RI; ++t) {
                res[t] = v4d{0.0, 0.0, 0.0, 0.0};
                p_cur[t] = pr[t * 64];
            }
#pragma unroll
            for (int ks = 0; ks < G::KQMAX; ++ks) {
                if (ks < KQ) {
                    const int nx = ks + 1 < KQ ? ks + 1 : ks;
                    double p_nxt[RI];
#pragma unroll
                    for (int t = 0; t < RI; ++t) p_nxt[t] = pr[(nx * RI + t) * 64];
#pragma unroll
                    for (int t = 0; t < RI; ++t) res[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(p_cur[t], sf[ks], res[t], 0, 0, 0);
#pragma unroll
                    for (int t = 0; t < RI; ++t) p_cur[t] = p_nxt[t];
                }
            }
        }

        // ---- transposition through the buffer (free: every B fragment is in registers), rows So apart; the output span
        // comes back into registers in the order it has in memory
        ln = fresh_lane();
#pragma unroll
        for (int t = 0; t < RI; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int i = 16 * t + (ln >> 4) + 4 * r;
                if (i < Ni) buf[(ln & 15) * So + i] = res[t][r];
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
            const int d0 = 2 * (cc * 64 + ln) - mo, d1 = d0 + 1;
            if (cc * 64 < n_chunks) oc[cc] = v2d{held(d0 < 0 ? 0 : d0 < n ? d0 : n - 1), held(d1 < n ? d1 : n - 1)};
        }
        wave_lds_fence();
        // ---- the next item lands in the buffer BEFORE this item's stores are issued: the wait for its loads is then not a
        // wait for these stores (one counter orders both), and the stores fly while the next item is computed
        if (more) land(field_n, tile_n, fresh_lane());
        wave_lds_fence();
        double* span = out + e0 * Ni;
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
        field = field_n;
        tile = tile_n;
    }
}

}  // namespace fe
