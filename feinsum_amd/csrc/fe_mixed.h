// fe_mixed.h -- grad 'xre,rij,ej->xei', div 'xre,rij,xej->ei' and face-mass 'ef,fij,fej->ei' x b with FLOAT32 FIELDS and float64
// geometry factors, operators and outputs, on the float64 matrix cores (tetrahedra p = 1 ... 4: Np = 4, 10, 20, 35; Nfp = 3, 6, 10,
// 15; 4 faces).  div and face-mass are described first; grad is at the end of the file.
//
// The kernels are the simple form of fe_div_f32.h / fe_facemass_f32.h (one wave = one tile of M sixteen-element sub-tiles, blocks
// of four waves, two blocks per CU, a persistent grid walked statically) with the arithmetic of fe_div.h / fe_facemass.h:
//   * a field value is widened to float64 where it is read out of LDS (exact); every product and sum after that is float64:
//     the B fragments on the VALU (div: one multiply and two explicit fused multiply-adds over x; face-mass: one multiply),
//     the contraction with the operator on v_mfma_f64_16x16x4_f64 (A resident in registers) and, for the rows behind the last
//     16-row tile, on v_mfma_f64_4x4x4_4b_f64 with its 4-row A slices in LDS, as in fe_div.h;
//   * padding (operator rows >= Np, k >= Np) is a select of 0.0 on BOTH operands behind an index clamped into the tile: no value
//     from outside an array is read and no 0 * x product can make a NaN;
//   * nothing is narrowed.
// f64 MFMA layouts (g = lane >> 4, n = lane & 15): A: lane supplies A[row n][k = g] (4x4x4_4b: A[row n & 3][k = g]), B: B[k = g]
// [column n], C/D of 16x16x4: rows g + 4 q (q = 0..3) of column n; of 4x4x4_4b: row g of column n.
//
// Data movement.  The field tiles enter LDS as float32, J as float64, in a ring of two slots per wave.  Two forms of the FIELD
// loads, chosen per launch (template parameter PLAIN):
//   * LDS-DMA, 16 bytes per lane (glds16_nt), counted waits -- when every field plane / face slab of the launch starts on an
//     8-byte boundary, the only source alignment of 16-byte LDS-DMA this project has verified (tools/align_test.hip).  A tile's
//     offset inside a plane is a multiple of 64 bytes, so the plane's start decides;
//   * ordinary 4-byte loads through registers into the same LDS image, waited for with vmcnt(0) -- otherwise (a float32 plane
//     x E Np 4 is only 4-byte aligned whenever E Np is odd).  Same arithmetic, same bits; slower.
// J (float64, every row 8-byte aligned) always comes by LDS-DMA.  Outputs leave through a wave-private transposition buffer as
// 16-byte non-temporal stores.  The elements behind the last full tile, and launches below one tile: remainder_items.
//
// div at p = 4: two float32 slots (3 x 2240 + 1152 B), a float64 output buffer (4480 B) and the 4-row A slices (3456 B per block)
// are 84 352 B per block, over the 80 KB of two blocks per CU.  The output buffer therefore ALIASES the u planes of the slot whose
// B fragments have just been built, and that slot is handed back to the loads only behind the tile's stores.  A wave still has
// the next tile in flight during a tile's MFMAs, which fe_div.h (one buffer) has not.  Vector-memory order: L(t) S(t-1) L(t+1) |
// top of tile t.  Face-mass has room for its own output buffer and keeps fe_facemass_f32.h's order L(m) S(m-2) L(m+1) S(m-1).
#pragma once
#include "fe_common.h"
#include "fe_grad.h"       // grad_row_tiles
#include "fe_grad_f32.h"   // v4f
#include <type_traits>

namespace fe {

constexpr int kLaunchMixedFields = 32, kLaunchPlainFieldLoads = 64;   // `kind` bits of fe_last_launch_info
constexpr int kLaunchFloat32Results = 256, kLaunchDwordStores = 512;  // ... of the float32-result kernels (OUT = float below)
// Float32 results (the kernels' template parameter OUT = float): the same arithmetic up to the float64 value that goes into the
// wave's transposition buffer; that value is narrowed there by a plain (float) cast -- one round-to-nearest-even -- so the buffer
// holds floats and is half the size.  Two forms of the non-temporal stores, chosen per launch by the rule of the load forms and
// passed as a wave-uniform bit of the kernel's flag word (one scalar branch per store group, as kOpLoadsTemporal):
//   * 16 bytes per lane -- when every output plane of the launch starts on an 8-byte boundary (the only alignment of 16-byte
//     global stores this project has verified, tools/align_test.hip; a tile's offset in a plane is a multiple of 64 bytes);
//   * kOpDwordStores: one float per lane, consecutive lanes consecutive floats -- otherwise (grad's planes x E Np 4 at odd E Np).
//     This form waits for its loads with vmcnt(0), like the register form of the field loads.
constexpr int kOpDwordStores = 2;    // in the opT word of grad and div, in the jfe word of face-mass

template <typename OUT>
constexpr bool kFloat32Results = std::is_same<OUT, float>::value;

// the float out tile of COUNT values from the wave's transposition buffer to global memory, non-temporal; INSTR16: the store
// instructions of the 16-byte form as the geometry counts them for its vmcnt
template <int COUNT, int INSTR16>
__device__ __forceinline__ void wave_store_f32(const float* ob, float* op, int lane, bool dwords) {
    static_assert(COUNT % 4 == 0 && INSTR16 == (COUNT / 4 + 63) / 64, "the counted vmcnt: one 16-byte store per 64 chunks of four floats");
    if (dwords) {
        constexpr int INSTR = (COUNT + 63) / 64;
#pragma unroll
        for (int c = 0; c < INSTR; ++c) {
            const int i = c * 64 + lane;
            if ((c + 1) * 64 <= COUNT || i < COUNT) __builtin_nontemporal_store(ob[i], op + i);
        }
    } else {
        constexpr int CHUNKS = COUNT / 4, INSTR = (CHUNKS + 63) / 64;
#pragma unroll
        for (int c = 0; c < INSTR; ++c) {
            const int q = c * 64 + lane;
            if ((c + 1) * 64 <= CHUNKS || q < CHUNKS) {
                const v4f val = *reinterpret_cast<const v4f*>(ob + 4 * q);
                __builtin_nontemporal_store(val, reinterpret_cast<v4f*>(op + 4 * q));
            }
        }
    }
}

template <int NP>
struct MixedRows {
    static constexpr int BT = NP / 16, NR = NP - 16 * BT, NS = (NR + 3) / 4;
};

// `count` floats from g (4-byte aligned) to lds, by one wave, through registers
template <int COUNT>
__device__ __forceinline__ void wave_copy_f32(const float* __restrict__ g, float* lds, int lane) {
    constexpr int INSTR = (COUNT + 63) / 64;
    float held[INSTR];
#pragma unroll
    for (int c = 0; c < INSTR; ++c) {
        const int i = c * 64 + lane;
        held[c] = ((c + 1) * 64 <= COUNT || i < COUNT) ? g[i] : 0.f;
    }
#pragma unroll
    for (int c = 0; c < INSTR; ++c) {
        const int i = c * 64 + lane;
        if ((c + 1) * 64 <= COUNT || i < COUNT) lds[i] = held[c];
    }
}

// ---------------------------------------------------------------------------------------------------------------- div

template <int NP_, int M_, typename OUT = double>
struct DivMixedGeomT : MixedRows<NP_> {
    using MixedRows<NP_>::NS;
    static constexpr int NP = NP_, M = M_, TEL = 16 * M;
    static constexpr int KSJ = (NP + 3) / 4, KS = 3 * KSJ;          // k-step 3 jq + r
    static constexpr int PLANE_F = TEL * NP, P_CHUNKS = PLANE_F / 4, P_INSTR = (P_CHUNKS + 63) / 64;   // one float32 u plane of a tile
    static constexpr int J_ROW_CHUNKS = TEL / 2, J_CHUNKS = 9 * J_ROW_CHUNKS, J_INSTR = (J_CHUNKS + 63) / 64;
    static constexpr int O_CHUNKS = PLANE_F * (int)sizeof(OUT) / 16, O_INSTR = (O_CHUNKS + 63) / 64;   // the out tile, 16-byte chunks
    static constexpr int LOADS = 3 * P_INSTR + J_INSTR, STORES = O_INSTR;
    struct Slot {
        float u[3][PLANE_F];     // u[x][e0 .. e0+TEL-1][0..Np-1]; once consumed: the out tile, OUT [TEL][Np]
        double j[9 * TEL];       // J[x*3+r][e0 .. e0+TEL-1]
    };
    struct WaveIn {
        Slot s[2];
    };
    static constexpr int WAVES = 4;
    static constexpr int OP_D = 3 * NP * NP;
    static constexpr int ASMALL_D = KS * NS * 16;                   // [k-step][group][g][row] doubles, per block
    static constexpr int IN_BYTES = (int)sizeof(WaveIn) * WAVES;    // (the operator is staged over it before the first loads)
    static constexpr int LDS_BYTES = (IN_BYTES > OP_D * 8 ? IN_BYTES : OP_D * 8) + ASMALL_D * 8;
    static constexpr int BLOCKS_PER_CU = 2;
    static_assert(PLANE_F % 4 == 0 && sizeof(Slot) % 16 == 0 && (3 * PLANE_F * 4) % 16 == 0, "16-byte LDS-DMA chunks");
    static_assert(PLANE_F * sizeof(OUT) <= 3 * PLANE_F * sizeof(float) && (PLANE_F * sizeof(OUT)) % 16 == 0,
                  "the out tile (OUT [TEL][Np], whole 16-byte chunks) fits the consumed u planes");
    static_assert(BLOCKS_PER_CU * LDS_BYTES <= 160 * 1024, "two blocks per CU");
    static_assert(STORES + LOADS <= 60, "counted vmcnt must fit the 6-bit field");
};

template <typename OUT>
__device__ __forceinline__ void div3d_item_mixed(const double* __restrict__ J, const double* __restrict__ D,
                                                 const float* __restrict__ u, OUT* __restrict__ out, int64_t E, int Np,
                                                 int64_t e, int i, int opT) {
    const int si = opT ? 1 : Np, sj = opT ? Np : 1;
    double jac[9];
    for (int k = 0; k < 9; ++k) jac[k] = J[(int64_t)k * E + e];
    double acc = 0.0;
    for (int j = 0; j < Np; ++j) {
        double ux[3];
        for (int x = 0; x < 3; ++x) ux[x] = (double)u[((int64_t)x * E + e) * Np + j];
        for (int r = 0; r < 3; ++r) {
            const double ju = __builtin_fma(jac[6 + r], ux[2], __builtin_fma(jac[3 + r], ux[1], jac[r] * ux[0]));
            acc = __builtin_fma(D[(int64_t)r * Np * Np + (int64_t)i * si + (int64_t)j * sj], ju, acc);
        }
    }
    out[e * Np + i] = (OUT)acc;
}

// OUT = float: float32 results; op_flags then also carries kOpDwordStores
template <int NP_, int M_, bool PLAIN, typename OUT = double>
__global__ __launch_bounds__(256, 2) void div3d_mixed_kernel(const double* __restrict__ J, const double* __restrict__ D,
                                                             const float* __restrict__ u, OUT* __restrict__ out, int64_t E,
                                                             int64_t nTiles, int op_flags) {
    using G = DivMixedGeomT<NP_, M_, OUT>;
    const int opT = kFloat32Results<OUT> ? (op_flags & 1) : op_flags;
    const bool dwords = kFloat32Results<OUT> && (op_flags & kOpDwordStores) != 0;
    constexpr int NP = G::NP, M = G::M;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    typename G::WaveIn* L = reinterpret_cast<typename G::WaveIn*>(smem) + wave;
    double* asmall = reinterpret_cast<double*>(smem + (G::LDS_BYTES - G::ASMALL_D * 8));
    const int n = lane & 15, g = lane >> 4;
    const unsigned bid = blockIdx.x, nblk = gridDim.x;
    const int64_t stride = (int64_t)nblk * G::WAVES, tEnd = nTiles;
    int64_t tile = (int64_t)bid * G::WAVES + wave;
    const unsigned lds_s0 = lds_addr_uniform(&L->s[0]);

    auto issue_loads = [&](int64_t t, int slot) {
        const unsigned lds_u = lds_s0 + slot * (unsigned)sizeof(typename G::Slot), lds_j = lds_u + 3 * G::PLANE_F * 4;
#pragma unroll
        for (int x = 0; x < 3; ++x) {
            const float* up = u + ((int64_t)x * E + t * G::TEL) * NP;
            if constexpr (PLAIN) {
                wave_copy_f32<G::PLANE_F>(up, L->s[slot].u[x], lane);
            } else {
#pragma unroll
                for (int c = 0; c < G::P_INSTR; ++c)
                    if ((c + 1) * 64 <= G::P_CHUNKS || c * 64 + lane < G::P_CHUNKS)
                        glds16_nt(reinterpret_cast<const char*>(up) + lane * 16 + c * 1024, lds_u + x * (G::PLANE_F * 4) + c * 1024);
            }
        }
#pragma unroll
        for (int c = 0; c < G::J_INSTR; ++c) {
            const int q = c * 64 + lane;
            const int row = q / G::J_ROW_CHUNKS, col = q - row * G::J_ROW_CHUNKS;
            if ((c + 1) * 64 <= G::J_CHUNKS || q < G::J_CHUNKS)
                glds16(reinterpret_cast<const char*>(J + (int64_t)row * E + t * G::TEL) + col * 16, lds_j + c * 1024);
        }
    };

    // ---- the operator -> LDS (over the waves' slots, which are empty yet), then the A fragments
    const double* dl = reinterpret_cast<const double*>(smem);
    stage_operator<G::OP_D>(D, reinterpret_cast<double*>(smem));
    __syncthreads();
    // 16x16x4: lane (g, n) supplies A[row 16 t + n][k = g] of k-step (jq, r): D[r][16 t + n][4 jq + g]
    double abig[G::BT > 0 ? G::BT : 1][G::KS];
    const int istride = opT ? 1 : NP, jstride = opT ? NP : 1;   // opT: D stored as [r][j][i]
#pragma unroll
    for (int t = 0; t < G::BT; ++t)
#pragma unroll
        for (int jq = 0; jq < G::KSJ; ++jq) {
            const int j = 4 * jq + g;
            const double* col = dl + (16 * t + n) * istride + (j < NP ? j : 0) * jstride;
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                const double val = col[r * (NP * NP)];
                abig[t][jq * 3 + r] = j < NP ? val : 0.0;
            }
        }
    // 4x4x4_4b group q: A[row 16 BT + 4 q + row4][k = gg], one copy per block in LDS (broadcast reads)
    for (int idx = threadIdx.x; idx < G::ASMALL_D; idx += 256) {
        const int row4 = idx & 3, gg = (idx >> 2) & 3, q = (idx >> 4) % G::NS, ks = (idx >> 4) / G::NS;
        const int i = 16 * G::BT + 4 * q + row4, j = 4 * (ks / 3) + gg, r = ks % 3;
        const bool in = i < NP && j < NP;
        const double val = dl[r * (NP * NP) + (in ? i : 0) * istride + (in ? j : 0) * jstride];
        asmall[idx] = in ? val : 0.0;
    }
    // the elements behind the last full tile, with the operator from the block's LDS copy
    remainder_items(nTiles * G::TEL, E, NP, bid, nblk, [&](int64_t e, int i) { div3d_item_mixed(J, dl, u, out, E, NP, e, i, opT); });
    __syncthreads();   // the staging area becomes the waves' slots
    const double* as_lane = asmall + g * 4 + (n & 3);

    if (tile < tEnd) issue_loads(tile, 0);
    if (tile + stride < tEnd) issue_loads(tile + stride, 1);

    const bool younger_half = bid >= (nblk + 1) / 2;
    int iteration = 0, slot = 0;
    while (tile < tEnd) {
        balance_priority(younger_half, iteration);
        // vector-memory ops in issue order: L(t) S(t-1) L(t+1); the plain form waits for everything
        if (!PLAIN && !dwords && iteration >= 1 && tile + stride < tEnd) wait_vmcnt<G::STORES + G::LOADS>();
        else wait_vmcnt<0>();
        if constexpr (PLAIN) wave_lds_fence();
        ++iteration;
        typename G::Slot* S = &L->s[slot];

        // ---- all B fragments of the tile: Ju[(jq, r)][e] = sum_x J[x,r,e] * (double) u[x,e,4 jq + g]
        double bfrag[M][G::KSJ][3];
#pragma unroll
        for (int m = 0; m < M; ++m) {
            double jac[9];
#pragma unroll
            for (int k = 0; k < 9; ++k) jac[k] = S->j[k * G::TEL + 16 * m + n];
#pragma unroll
            for (int jq = 0; jq < G::KSJ; ++jq) {
                const int j = 4 * jq + g, jc = j < NP ? j : 0;
                double ux[3];
#pragma unroll
                for (int x = 0; x < 3; ++x) ux[x] = (double)S->u[x][(16 * m + n) * NP + jc];
#pragma unroll
                for (int r = 0; r < 3; ++r) {
                    const double ju = __builtin_fma(jac[6 + r], ux[2], __builtin_fma(jac[3 + r], ux[1], jac[r] * ux[0]));
                    bfrag[m][jq][r] = j < NP ? ju : 0.0;
                }
            }
        }
        wave_lds_fence();   // the u planes are in registers: they become the out tile
        OUT* ob = reinterpret_cast<OUT*>(&S->u[0][0]);

#pragma unroll
        for (int m = 0; m < M; ++m) {
            v4d acc[G::BT > 0 ? G::BT : 1];
            double accs[G::NS > 0 ? G::NS : 1];
#pragma unroll
            for (int t = 0; t < G::BT; ++t) acc[t] = v4d{0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int q = 0; q < G::NS; ++q) accs[q] = 0.0;
#pragma unroll
            for (int jq = 0; jq < G::KSJ; ++jq)
#pragma unroll
                for (int r = 0; r < 3; ++r) {
#pragma unroll
                    for (int t = 0; t < G::BT; ++t)
                        acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(abig[t][jq * 3 + r], bfrag[m][jq][r], acc[t], 0, 0, 0);
#pragma unroll
                    for (int q = 0; q < G::NS; ++q)
                        accs[q] = __builtin_amdgcn_mfma_f64_4x4x4f64(as_lane[((jq * 3 + r) * G::NS + q) * 16], bfrag[m][jq][r], accs[q], 0, 0, 0);
                }
            // ---- into the transposition buffer: 16x16x4: lane (g, n) holds out[e0 + 16 m + n][16 t + g + 4 q']; group q of
            //      4x4x4_4b: out[e0 + 16 m + n][16 BT + 4 q + g]
#pragma unroll
            for (int t = 0; t < G::BT; ++t)
#pragma unroll
                for (int qq = 0; qq < 4; ++qq) ob[(16 * m + n) * NP + 16 * t + g + 4 * qq] = (OUT)acc[t][qq];
#pragma unroll
            for (int q = 0; q < G::NS; ++q) {
                const int i = 16 * G::BT + 4 * q + g;
                if (16 * G::BT + 4 * q + 3 < NP || i < NP) ob[(16 * m + n) * NP + i] = (OUT)accs[q];
            }
        }
        wave_lds_fence();
        OUT* op = out + tile * (G::TEL * NP);
        if constexpr (kFloat32Results<OUT>) {
            wave_store_f32<G::PLANE_F, G::STORES>(ob, op, lane, dwords);
        } else {
#pragma unroll
            for (int c = 0; c < G::O_INSTR; ++c) {
                const int q = c * 64 + lane;
                if ((c + 1) * 64 <= G::O_CHUNKS || q < G::O_CHUNKS) {
                    const v2d val = *reinterpret_cast<const v2d*>(ob + 2 * q);
                    __builtin_nontemporal_store(val, reinterpret_cast<v2d*>(op + 2 * q));
                }
            }
        }
        wave_lds_fence();
        // the out tile has left LDS (every store holds its data): the slot goes back to the loads
        if (tile + 2 * stride < tEnd) issue_loads(tile + 2 * stride, slot);
        tile += stride;
        slot ^= 1;
    }
}

// ---------------------------------------------------------------------------------------------------------- face-mass

template <int NP_, int NFP_, int M_, typename OUT = double>
struct FmMixedGeomT : MixedRows<NP_> {
    using MixedRows<NP_>::NS;
    static constexpr int NP = NP_, NFP = NFP_, NF = 4, M = M_, TEL = 16 * M;
    static constexpr int K = NF * NFP, KS = K / 4;
    static constexpr int SLAB_F = TEL * NFP, UNIT_F = NF * SLAB_F;  // floats per face slab of a unit, per unit
    static constexpr int SLAB_CHUNKS = SLAB_F / 4, SLAB_INSTR = (SLAB_CHUNKS + 63) / 64;
    static constexpr int J_CHUNKS = NF * TEL / 2, J_INSTR = (J_CHUNKS + 63) / 64;
    static constexpr int SUB_D = TEL * NP, SUB_CHUNKS = SUB_D * (int)sizeof(OUT) / 16, SUB_INSTR = (SUB_CHUNKS + 63) / 64;   // the out tile of a unit
    static constexpr int UNIT_LOADS = NF * SLAB_INSTR, UNIT_STORES = SUB_INSTR;
    struct WaveIn {
        float v[2][UNIT_F];      // ring of field slabs: v[slot][f][e][j]
        double j[2][NF * TEL];   // J tile of the unit in that slot, [e][f] or [f][e] as in global memory
        OUT o[SUB_D];            // output transposition buffer
    };
    static constexpr int WAVES = 4;
    static constexpr int OP_D = NF * NP * NFP;
    static constexpr int ASMALL_D = KS * NS * 16;
    static constexpr int IN_BYTES = (int)sizeof(WaveIn) * WAVES;
    static constexpr int LDS_BYTES = (IN_BYTES > OP_D * 8 ? IN_BYTES : OP_D * 8) + ASMALL_D * 8;
    static constexpr int BLOCKS_PER_CU = 2;
    static_assert(K % 4 == 0 && SLAB_F % 4 == 0 && (SUB_D * sizeof(OUT)) % 16 == 0 && (UNIT_F * 4) % 16 == 0 && sizeof(WaveIn) % 16 == 0, "geometry");
    static_assert(BLOCKS_PER_CU * LDS_BYTES <= 160 * 1024, "two blocks per CU");
    static_assert(2 * UNIT_STORES + UNIT_LOADS + J_INSTR <= 60, "counted vmcnt must fit the 6-bit field");
};

// field k of a mixed launch: float32 in, float64 or float32 out (FieldPtrs carries both as double*: the argument pack is untyped)
__device__ __forceinline__ const float* field_in_mixed(const FieldPtrs& P, int k) { return reinterpret_cast<const float*>(field_in(P, k)); }
template <typename OUT>
__device__ __forceinline__ OUT* field_out_mixed(const FieldPtrs& P, int k) { return reinterpret_cast<OUT*>(field_out(P, k)); }

// OUT = float: float32 results (P.out holds float*); jfe_flags then also carries kOpDwordStores
template <int NP_, int NFP_, int M_, bool PLAIN, typename OUT = double>
__global__ __launch_bounds__(256, 2) void facemass_mixed_kernel(const double* __restrict__ J, const double* __restrict__ R, FieldPtrs P,
                                                                int nb, int64_t E, int64_t nTiles, int jfe_flags, int rlayout) {
    using G = FmMixedGeomT<NP_, NFP_, M_, OUT>;
    const int jfe = kFloat32Results<OUT> ? (jfe_flags & 1) : jfe_flags;
    const bool dwords = kFloat32Results<OUT> && (jfe_flags & kOpDwordStores) != 0;
    constexpr int NP = G::NP, NFP = G::NFP, NF = G::NF, M = G::M;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    typename G::WaveIn* L = reinterpret_cast<typename G::WaveIn*>(smem) + wave;
    double* asmall = reinterpret_cast<double*>(smem + (G::LDS_BYTES - G::ASMALL_D * 8));
    OUT* ob = L->o;
    const int n = lane & 15, g = lane >> 4;
    const unsigned bid = blockIdx.x, nblk = gridDim.x;
    const int64_t stride = (int64_t)nblk * G::WAVES, tEnd = nTiles;
    const int64_t first = (int64_t)bid * G::WAVES + wave;
    const unsigned lds_v0 = lds_addr_uniform(L->v[0]), lds_j0 = lds_addr_uniform(L->j[0]);

    auto issue_unit = [&](int64_t t, int k, int slot) {
        const int64_t e0 = t * G::TEL;
        const float* vk = field_in_mixed(P, k) + e0 * NFP;
#pragma unroll
        for (int f = 0; f < NF; ++f) {
            const float* slab = vk + (int64_t)f * E * NFP;
            if constexpr (PLAIN) {
                wave_copy_f32<G::SLAB_F>(slab, L->v[slot] + f * G::SLAB_F, lane);
            } else {
#pragma unroll
                for (int c = 0; c < G::SLAB_INSTR; ++c)
                    if ((c + 1) * 64 <= G::SLAB_CHUNKS || c * 64 + lane < G::SLAB_CHUNKS)
                        glds16_nt(reinterpret_cast<const char*>(slab) + lane * 16 + c * 1024,
                                  lds_v0 + slot * (G::UNIT_F * 4) + f * (G::SLAB_F * 4) + c * 1024);
            }
        }
        if (k == 0) {   // the tile's J: "fe": 4 rows of TEL doubles, else TEL x 4 contiguous doubles
#pragma unroll
            for (int c = 0; c < G::J_INSTR; ++c) {
                const int q = c * 64 + lane;
                const int row = q / (G::TEL / 2), col = q - row * (G::TEL / 2);
                const char* src = jfe ? reinterpret_cast<const char*>(J + (int64_t)row * E + e0) + col * 16
                                      : reinterpret_cast<const char*>(J + e0 * NF) + q * 16;
                if ((c + 1) * 64 <= G::J_CHUNKS || q < G::J_CHUNKS) glds16(src, lds_j0 + slot * (NF * G::TEL * 8) + c * 1024);
            }
        }
    };
    auto advance = [&](int64_t& t, int& k) {
        if (++k == nb) { k = 0; t += stride; }
    };

    // ---- the operator -> LDS (over the waves' buffers, which are empty yet), then the A fragments
    const double* rl = reinterpret_cast<const double*>(smem);
    stage_operator<G::OP_D>(R, reinterpret_cast<double*>(smem));
    __syncthreads();
    // operator layouts: 0 R[f][i][j], 1 L[i][f][j], 2 R[f][j][i], 3 L[j][f][i] -> strides of f, i, j
    const int sF = rlayout == 0 ? NP * NFP : rlayout == 1 ? NFP : rlayout == 2 ? NFP * NP : NP;
    const int sI = rlayout == 0 ? NFP : rlayout == 1 ? NF * NFP : 1;
    const int sJ = rlayout == 0 || rlayout == 1 ? 1 : rlayout == 2 ? NP : NF * NP;
    // per-lane K decomposition (k = 4 ks + g = Nfp f + j: offsets of sub-tile 0) and the 16-row A fragments
    int voff[G::KS], joff[G::KS];
    double abig[G::BT > 0 ? G::BT : 1][G::KS];
#pragma unroll
    for (int ks = 0; ks < G::KS; ++ks) {
        const int k = 4 * ks + g, f = k / NFP, j = k - f * NFP;
        voff[ks] = f * G::SLAB_F + n * NFP + j;
        joff[ks] = jfe ? f * G::TEL + n : n * NF + f;
#pragma unroll
        for (int t = 0; t < G::BT; ++t) abig[t][ks] = rl[f * sF + (16 * t + n) * sI + j * sJ];
    }
    for (int idx = threadIdx.x; idx < G::ASMALL_D; idx += 256) {
        const int row4 = idx & 3, gg = (idx >> 2) & 3, q = (idx >> 4) % G::NS, ks = (idx >> 4) / G::NS;
        const int i = 16 * G::BT + 4 * q + row4, k = 4 * ks + gg, f = k / NFP, j = k - f * NFP;
        const double val = rl[f * sF + (i < NP ? i : 0) * sI + j * sJ];
        asmall[idx] = i < NP ? val : 0.0;
    }
    {   // the elements behind the last full tile, with the operator from the block's LDS copy
        const int64_t jEs = jfe ? 1 : NF, jFs = jfe ? E : 1;
        remainder_items(nTiles * G::TEL, E, NP, bid, nblk, [&](int64_t e, int i) {
            for (int k = 0; k < nb; ++k) {
                const float* vk = field_in_mixed(P, k);
                double acc = 0.0;
                for (int f = 0; f < NF; ++f) {
                    const double jf = J[e * jEs + f * jFs];
                    for (int j = 0; j < NFP; ++j)
                        acc = __builtin_fma(rl[f * sF + i * sI + j * sJ], jf * (double)vk[((int64_t)f * E + e) * NFP + j], acc);
                }
                field_out_mixed<OUT>(P, k)[e * NP + i] = (OUT)acc;
            }
        });
    }
    __syncthreads();   // the staging area becomes the waves' buffers
    const double* as_lane = asmall + g * 4 + (n & 3);

    // ---- units 0 and 1 of this wave
    int64_t tile = first, t1 = first, t2;
    int fk = 0, k1 = 0, k2;
    advance(t1, k1);
    t2 = t1, k2 = k1;
    advance(t2, k2);
    if (tile < tEnd) {
        issue_unit(tile, 0, 0);
        if (t1 < tEnd) issue_unit(t1, k1, 1);
    }

    int slot = 0, done = 0, iteration = 0;
    double jv[M][G::KS];
    const bool younger_half = bid >= (nblk + 1) / 2;
    while (tile < tEnd) {
        if (fk == 0) balance_priority(younger_half, iteration++);
        // ---- wait for this unit's loads; younger ops: S(m-2), L(m+1), S(m-1); the plain form waits for everything
        if (!PLAIN && !dwords && done >= 2 && t1 < tEnd) {
            if (k1 == 0) wait_vmcnt<2 * G::UNIT_STORES + G::UNIT_LOADS + G::J_INSTR>();
            else wait_vmcnt<2 * G::UNIT_STORES + G::UNIT_LOADS>();
        } else {
            wait_vmcnt<0>();
        }
        if constexpr (PLAIN) wave_lds_fence();
        const float* vs = L->v[slot];
        if (fk == 0) {
            const double* js = L->j[slot];
#pragma unroll
            for (int m = 0; m < M; ++m)
#pragma unroll
                for (int ks = 0; ks < G::KS; ++ks) jv[m][ks] = js[joff[ks] + (jfe ? 16 * m : 16 * m * NF)];
        }
        double bfrag[M][G::KS];
#pragma unroll
        for (int m = 0; m < M; ++m)
#pragma unroll
            for (int ks = 0; ks < G::KS; ++ks) bfrag[m][ks] = jv[m][ks] * (double)vs[voff[ks] + 16 * m * NFP];
        // the slabs (and, at a tile start, the J tile) are in registers before the slot is handed back to the loads
        wave_lds_fence();
        __builtin_amdgcn_s_waitcnt(0xC07F);   // lgkmcnt(0)
        if (t2 < tEnd) issue_unit(t2, k2, slot);

#pragma unroll
        for (int m = 0; m < M; ++m) {
            v4d acc[G::BT > 0 ? G::BT : 1];
            double accs[G::NS > 0 ? G::NS : 1];
#pragma unroll
            for (int t = 0; t < G::BT; ++t) acc[t] = v4d{0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int q = 0; q < G::NS; ++q) accs[q] = 0.0;
#pragma unroll
            for (int ks = 0; ks < G::KS; ++ks) {
#pragma unroll
                for (int t = 0; t < G::BT; ++t) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(abig[t][ks], bfrag[m][ks], acc[t], 0, 0, 0);
#pragma unroll
                for (int q = 0; q < G::NS; ++q)
                    accs[q] = __builtin_amdgcn_mfma_f64_4x4x4f64(as_lane[(ks * G::NS + q) * 16], bfrag[m][ks], accs[q], 0, 0, 0);
            }
#pragma unroll
            for (int t = 0; t < G::BT; ++t)
#pragma unroll
                for (int qq = 0; qq < 4; ++qq) ob[(16 * m + n) * NP + 16 * t + g + 4 * qq] = (OUT)acc[t][qq];
#pragma unroll
            for (int q = 0; q < G::NS; ++q) {
                const int i = 16 * G::BT + 4 * q + g;
                if (16 * G::BT + 4 * q + 3 < NP || i < NP) ob[(16 * m + n) * NP + i] = (OUT)accs[q];
            }
        }
        wave_lds_fence();
        OUT* op = field_out_mixed<OUT>(P, fk) + tile * (G::TEL * NP);
        if constexpr (kFloat32Results<OUT>) {
            wave_store_f32<G::SUB_D, G::UNIT_STORES>(ob, op, lane, dwords);
        } else {
#pragma unroll
            for (int c = 0; c < G::SUB_INSTR; ++c) {
                const int q = c * 64 + lane;
                if ((c + 1) * 64 <= G::SUB_CHUNKS || q < G::SUB_CHUNKS) {
                    const v2d val = *reinterpret_cast<const v2d*>(ob + 2 * q);
                    __builtin_nontemporal_store(val, reinterpret_cast<v2d*>(op + 2 * q));
                }
            }
        }
        wave_lds_fence();
        tile = t1, fk = k1;
        t1 = t2, k1 = k2;
        advance(t2, k2);
        slot ^= 1;
        ++done;
    }
}

// --------------------------------------------------------------------------------------------------------------- grad

// grad 'xre,rij,ej->xei': stage 1  tmp[(r,i), e] = sum_j D[(r,i), j] * (double) u[e, j]  on v_mfma_f64_16x16x4_f64 with the
// row permutation of fe_grad.h (slot s = 4 t + q of lane group g is (r, i) = (s % 3, TG g + s / 3), so that every lane owns all
// three r of TG consecutive i of one element), stage 2  out[x,e,i] = sum_r J[x,r,e] * tmp  lane-local on the VALU (one multiply,
// two explicit fused multiply-adds).  The float32 u tile is widened where the B fragments are read.  Data movement is
// fe_grad_f32.h's static walk: loads one tile ahead into a double buffer, L(t) S(t-1) L(t+1) | wait L(t).
template <int M_, int NP_, typename OUT = double>
struct GradMixedGeomT {
    static constexpr int M = M_, NP = NP_, TEL = 16 * M, RT = grad_row_tiles(NP_), TG = (4 * RT) / 3, KS = (NP_ + 3) / 4;
    static constexpr int TILE_F = TEL * NP;             // floats of the u tile = values of one out plane of a tile
    static constexpr int U_CHUNKS = TILE_F / 4, U_INSTR = (U_CHUNKS + 63) / 64;
    static constexpr int J_ROW_CHUNKS = TEL / 2, J_CHUNKS = 9 * J_ROW_CHUNKS, J_INSTR = (J_CHUNKS + 63) / 64;
    static constexpr int O_CHUNKS = TILE_F * (int)sizeof(OUT) / 16, PLANE_STORES = (O_CHUNKS + 63) / 64;
    static constexpr int LOADS = U_INSTR + J_INSTR, STORES = 3 * PLANE_STORES;
    struct WaveLds {
        float u[2][TILE_F];      // prefetch double buffer
        double j[2][9 * TEL];    // J[x*3+r][e0 .. e0+TEL-1], double buffered
    };
    struct WaveOut {
        OUT o[2][TILE_F];        // output transposition buffers (a whole plane of the tile), alternating
    };
    static constexpr int WAVES = 4;
    static constexpr int OP_D = 3 * NP * NP;
    static constexpr int IN_BYTES = (int)sizeof(WaveLds) * WAVES;
    static constexpr int OUT_BYTES = (int)sizeof(WaveOut) * WAVES;
    static constexpr int LDS_BYTES = IN_BYTES + (OUT_BYTES > OP_D * 8 ? OUT_BYTES : OP_D * 8);   // (the operator is staged over the output buffers)
    static constexpr int BLOCKS_PER_CU = 2;
    static_assert(TILE_F % 4 == 0 && (TILE_F * 4) % 16 == 0 && sizeof(WaveLds) % 16 == 0 && sizeof(WaveOut) % 16 == 0, "16-byte chunks");
    static_assert(BLOCKS_PER_CU * LDS_BYTES <= 160 * 1024, "two blocks per CU");
    static_assert(LOADS + STORES <= 60, "counted vmcnt must fit the 6-bit field");
};

template <typename OUT>
__device__ __forceinline__ void grad3d_item_mixed(const double* __restrict__ J, const double* __restrict__ D,
                                                  const float* __restrict__ u, OUT* __restrict__ out, int64_t E, int Np,
                                                  int64_t e, int i, int opT) {
    double t0 = 0.0, t1 = 0.0, t2 = 0.0;
    const float* ue = u + e * Np;
    const int si = opT ? 1 : Np, sj = opT ? Np : 1;
    const double* d0 = D + (int64_t)i * si;
    const double* d1 = d0 + (int64_t)Np * Np;
    const double* d2 = d1 + (int64_t)Np * Np;
    for (int j = 0; j < Np; ++j) {
        const double uj = (double)ue[j];
        t0 = __builtin_fma(d0[j * sj], uj, t0);
        t1 = __builtin_fma(d1[j * sj], uj, t1);
        t2 = __builtin_fma(d2[j * sj], uj, t2);
    }
    for (int x = 0; x < 3; ++x)
        out[((int64_t)x * E + e) * Np + i] =
            (OUT)__builtin_fma(J[(int64_t)(x * 3 + 2) * E + e], t2,
                               __builtin_fma(J[(int64_t)(x * 3 + 1) * E + e], t1, J[(int64_t)(x * 3 + 0) * E + e] * t0));
}

// OUT = float: float32 results; op_flags then also carries kOpDwordStores
template <int M, int NP_, bool PLAIN, typename OUT = double>
__global__ __launch_bounds__(256, 2) void grad3d_mixed_kernel(const double* __restrict__ J, const double* __restrict__ D,
                                                              const float* __restrict__ u, OUT* __restrict__ out, int64_t E,
                                                              int64_t nTiles, int op_flags) {
    using G = GradMixedGeomT<M, NP_, OUT>;
    const int opT = kFloat32Results<OUT> ? (op_flags & 1) : op_flags;
    const bool dwords = kFloat32Results<OUT> && (op_flags & kOpDwordStores) != 0;
    constexpr int NP = G::NP;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    typename G::WaveLds* L = reinterpret_cast<typename G::WaveLds*>(smem) + wave;
    typename G::WaveOut* LO = reinterpret_cast<typename G::WaveOut*>(smem + G::IN_BYTES) + wave;
    const int n = lane & 15, g = lane >> 4;
    const unsigned bid = blockIdx.x, nblk = gridDim.x;
    const int64_t stride = (int64_t)nblk * G::WAVES, tEnd = nTiles;
    int64_t tile = (int64_t)bid * G::WAVES + wave;

    auto issue_loads = [&](int64_t t, int buf) {
        const float* ut = u + t * G::TILE_F;
        if constexpr (PLAIN) {
            wave_copy_f32<G::TILE_F>(ut, L->u[buf], lane);
        } else {
            const unsigned lds_u = lds_addr_uniform(L->u[buf]);
#pragma unroll
            for (int c = 0; c < G::U_INSTR; ++c)
                if ((c + 1) * 64 <= G::U_CHUNKS || c * 64 + lane < G::U_CHUNKS)
                    glds16_nt(reinterpret_cast<const char*>(ut) + lane * 16 + c * 1024, lds_u + c * 1024);
        }
        const unsigned lds_j = lds_addr_uniform(L->j[buf]);
#pragma unroll
        for (int c = 0; c < G::J_INSTR; ++c) {
            const int q = c * 64 + lane;
            const int row = q / G::J_ROW_CHUNKS, col = q - row * G::J_ROW_CHUNKS;   // chunk -> (row x*3 + r, column chunk)
            const char* src = reinterpret_cast<const char*>(J + (int64_t)row * E + t * G::TEL) + col * 16;
            if ((c + 1) * 64 <= G::J_CHUNKS || q < G::J_CHUNKS) glds16(src, lds_j + c * 1024);
        }
    };

    // ---- the loads of this wave's first two tiles, and behind them the operator -> LDS (over the output buffers)
    bool pre = false;
    if (tile < tEnd) {
        issue_loads(tile, 0);
        if (tile + stride < tEnd) {
            issue_loads(tile + stride, 1);
            pre = true;
        }
    }
    const double* dl = reinterpret_cast<const double*>(smem + G::IN_BYTES);
    stage_operator<G::OP_D>(D, reinterpret_cast<double*>(smem + G::IN_BYTES));
    __syncthreads();

    // ---- A fragments: lane (g, n) supplies A[row n of tile t][k = 4 ks + g]; float64 C/D rows are g' + 4 q, so row n = g' + 4 q
    //      ->  slot s = 4 t + q of lane group g'  ->  (r, i) = (s % 3, TG g' + s / 3)
    double afrag[G::RT][G::KS];
    {
        const int gp = n & 3, q = n >> 2;
        const int istride = opT ? 1 : NP, jstride = opT ? NP : 1;   // opT: D stored as [r][j][i]
#pragma unroll
        for (int t = 0; t < G::RT; ++t) {
            const int s = 4 * t + q;
            const int r = s % 3, i = G::TG * gp + s / 3;
            const bool rowok = (s < 3 * G::TG) && (i < NP);
            const double* row = dl + (rowok ? r : 0) * (NP * NP) + (rowok ? i : 0) * istride;
#pragma unroll
            for (int ks = 0; ks < G::KS; ++ks) {
                const int j = 4 * ks + g;
                const double val = row[(j < NP ? j : 0) * jstride];
                afrag[t][ks] = (rowok && j < NP) ? val : 0.0;
            }
        }
    }
    remainder_items(nTiles * G::TEL, E, NP, bid, nblk, [&](int64_t e, int i) { grad3d_item_mixed(J, dl, u, out, E, NP, e, i, opT); });
    __syncthreads();   // the staging area becomes the waves' output buffers

    const bool younger_half = bid >= (nblk + 1) / 2;
    int buf = 0, iteration = 0;
    bool first = true;
    while (tile < tEnd) {
        balance_priority(younger_half, iteration++);
        // vector-memory ops in issue order: L(tile) S(previous tile) L(next tile) | wait L(tile); the plain form waits for everything
        const int64_t nt = tile + stride;
        if (nt < tEnd && !pre) issue_loads(nt, buf ^ 1);
        if constexpr (PLAIN) {
            wait_vmcnt<0>();
            wave_lds_fence();
        } else if (dwords) {
            wait_vmcnt<0>();
        } else if (nt < tEnd) {
            if (first) wait_vmcnt<G::LOADS>();
            else wait_vmcnt<G::LOADS + G::STORES>();
        } else {
            if (first) wait_vmcnt<0>();
            else wait_vmcnt<G::STORES>();
        }
        first = false;
        pre = false;
        const float* ut = L->u[buf];
        const double* jt = L->j[buf];

        // ---- stage 1, sub-tile by sub-tile
        v4d acc[M][G::RT];
#pragma unroll
        for (int m = 0; m < M; ++m) {
            double bfrag[G::KS];
#pragma unroll
            for (int ks = 0; ks < G::KS; ++ks) {
                const int j = 4 * ks + g;
                const double b = (double)ut[(16 * m + n) * NP + (j < NP ? j : 0)];
                bfrag[ks] = (j < NP) ? b : 0.0;
            }
#pragma unroll
            for (int t = 0; t < G::RT; ++t) acc[m][t] = v4d{0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int ks = 0; ks < G::KS; ++ks)
#pragma unroll
                for (int t = 0; t < G::RT; ++t) acc[m][t] = __builtin_amdgcn_mfma_f64_16x16x4f64(afrag[t][ks], bfrag[ks], acc[m][t], 0, 0, 0);
        }

        // ---- stage 2 + transposed store, plane by plane
        const int64_t e0 = tile * G::TEL;
#pragma unroll
        for (int x = 0; x < 3; ++x) {
            OUT* ob = LO->o[x & 1];
#pragma unroll
            for (int m = 0; m < M; ++m) {
                const double j0 = jt[(x * 3 + 0) * G::TEL + 16 * m + n];
                const double j1 = jt[(x * 3 + 1) * G::TEL + 16 * m + n];
                const double j2 = jt[(x * 3 + 2) * G::TEL + 16 * m + n];
#pragma unroll
                for (int k = 0; k < G::TG; ++k) {
                    const int s = 3 * k;
                    const double t0 = acc[m][(s + 0) >> 2][(s + 0) & 3];
                    const double t1 = acc[m][(s + 1) >> 2][(s + 1) & 3];
                    const double t2 = acc[m][(s + 2) >> 2][(s + 2) & 3];
                    const double val = __builtin_fma(j2, t2, __builtin_fma(j1, t1, j0 * t0));
                    const int i = G::TG * g + k;
                    if (G::TG * 3 + k < NP || i < NP) ob[(16 * m + n) * NP + i] = (OUT)val;
                }
            }
            wave_lds_fence();
            OUT* op = out + ((int64_t)x * E + e0) * NP;
            if constexpr (kFloat32Results<OUT>) {
                wave_store_f32<G::TILE_F, G::PLANE_STORES>(ob, op, lane, dwords);
            } else {
#pragma unroll
                for (int c = 0; c < G::PLANE_STORES; ++c) {
                    const int q = c * 64 + lane;
                    if ((c + 1) * 64 <= G::O_CHUNKS || q < G::O_CHUNKS) {
                        const v2d val = *reinterpret_cast<const v2d*>(ob + 2 * q);
                        __builtin_nontemporal_store(val, reinterpret_cast<v2d*>(op + 2 * q));
                    }
                }
            }
            wave_lds_fence();
        }
        tile = nt;
        buf ^= 1;
    }
}

}  // namespace fe
