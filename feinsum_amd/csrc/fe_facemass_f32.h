// fe_facemass_f32.h -- face-mass (lift) einsum in float32 on the matrix cores (tetrahedra p = 1 ... 4: (Np, Nfp) = (4, 3),
// (10, 6), (20, 10), (35, 15), 4 faces), nb fields sharing J and R:
//   out_k[e,i] = sum_{f,j} J[e,f] R[f,i,j] v_k[f,e,j]      ('ef,fij,fej->ei' x b and its layout siblings 'ifj,fe,fej->ei' /
//   'jfi,fe,fej->ei': the layouts of fe_facemass.h).
//
// The float32 counterpart of fe_facemass.h's register-fragment kernel, a wave tile of M sixteen-element sub-tiles:
//   B fragments  Jv_k[(f,j), e] = J[e,f] * v_k[f,e,j]   (one multiply, VALU, produced in MFMA B layout; k = Nfp f + j = 4 ks + g),
//   out_k[i, e] = sum_k R'[i, k] * Jv_k[k, e]   on the matrix cores: K = 4 Nfp = 12 / 24 / 40 / 60 is a whole number of k-steps
//   at every order; A = R' resident in registers, the Np rows as 16-row tiles and 4-row groups (F32Rows, fe_div_f32.h); Np = 35:
//   45 floats per lane, 2 x 15 MFMAs of 32 cycles and 15 of 8 cycles per (sub-tile, field).
// M = 1 / 1 / 2 / 4 for p = 4 / 3 / 2 / 1 (as fe_facemass.h).
// Data movement: a unit's four face slabs (Np = 35: 4 x 960 contiguous bytes) come in by LDS-DMA into a 2-slot ring two units
// ahead -- the loads of unit m + 2 are issued as soon as unit m's B fragments are in registers, before its MFMAs and stores; J
// for a tile comes with the tile's first unit (into the J buffer of that unit's slot) and is kept in registers for the tile's
// other fields; results leave through a wave-private LDS transposition buffer as 1-KiB contiguous non-temporal stores.
// Np = 35: twelve waves per CU (40 KB of LDS per block of four).  The number of fields is a run-time argument (1..8): units are
// walked (tile, field), field fastest.
// A third 16-row tile for rows 32..34 of Np = 35 instead of the 4-row group was measured and rejected in round 3: the same
// time from the split allocator, 0.3005 against 0.2613 ms at E = 1e6 from separate allocations
// (profiles/r03/float32_div_facemass.txt).  The lower orders ran on the tiled VALU kernel in float before round 5.
// Np = 35: 1536 B and 17 040 flops per element at four fields: HBM roofline 88.7 TFLOP/s.  Operands must be 16-byte aligned
// with E a multiple of 4; the elements behind the last full tile: remainder_items (fe_common.h).
#pragma once
#include "fe_div_f32.h"   // F32Rows

namespace fe {

template <int NP_, int NFP_, int M_>
struct FmF32GeomT : F32Rows<NP_> {
    static constexpr int NP = NP_, NFP = NFP_, NF = 4, M = M_, TEL = 16 * M;
    static constexpr int K = NF * NFP, KS = K / 4;
    static constexpr int SLAB_F = TEL * NFP, UNIT_F = NF * SLAB_F;  // floats per face slab of a unit, per unit
    static constexpr int SLAB_CHUNKS = SLAB_F / 4, SLAB_INSTR = (SLAB_CHUNKS + 63) / 64;
    static constexpr int J_CHUNKS = NF * TEL / 4, J_INSTR = (J_CHUNKS + 63) / 64;
    static constexpr int SUB_F = TEL * NP, SUB_CHUNKS = SUB_F / 4, SUB_INSTR = (SUB_CHUNKS + 63) / 64;   // the out tile of a unit
    static constexpr int UNIT_LOADS = NF * SLAB_INSTR, UNIT_STORES = SUB_INSTR;
    struct WaveIn {
        float v[2][UNIT_F];      // ring of field slabs: v[slot][f][e][j]
        float j[2][NF * TEL];    // J tile of the unit in that slot, [e][f] or [f][e] as in global memory
    };
    static constexpr int WAVES = 4;
    static constexpr int OP_F = NF * NP * NFP;
    static constexpr int IN_BYTES = (int)sizeof(WaveIn) * WAVES;
    static constexpr int OUT_BYTES = SUB_F * 4 * WAVES;
    static constexpr int OP_BYTES = (OP_F * 4 + 15) / 16 * 16;
    static constexpr int LDS_BYTES = IN_BYTES + (OUT_BYTES > OP_BYTES ? OUT_BYTES : OP_BYTES);
    static constexpr int BLOCKS_PER_CU = 3 * LDS_BYTES <= 160 * 1024 ? 3 : 2;
    static constexpr int LAUNCH_BLOCKS = NP == 35 ? 3 : 2;          // __launch_bounds__: p = 4 is held to the registers of three blocks per CU
                                                                    // (round 3), the lower orders to those of two (round 5)
    static_assert(K % 4 == 0 && SLAB_F % 4 == 0 && SUB_F % 4 == 0, "geometry");
    static_assert(BLOCKS_PER_CU * LDS_BYTES <= 160 * 1024, "blocks per CU");
    static_assert(2 * UNIT_STORES + UNIT_LOADS + J_INSTR <= 60, "counted vmcnt must fit the 6-bit field");
};

// field k of a launch as float pointers (FieldPtrs carries them as double*: the C ABI's argument pack is untyped)
__device__ __forceinline__ const float* field_in_f32(const FieldPtrs& P, int k) { return reinterpret_cast<const float*>(field_in(P, k)); }
__device__ __forceinline__ float* field_out_f32(const FieldPtrs& P, int k) { return reinterpret_cast<float*>(field_out(P, k)); }

template <int NP_, int NFP_, int M_>
__global__ __launch_bounds__(256, (FmF32GeomT<NP_, NFP_, M_>::LAUNCH_BLOCKS)) void facemass_mfma_f32_kernel(
    const float* __restrict__ J, const float* __restrict__ R, FieldPtrs P, int nb, int64_t E, int64_t nTiles, int jfe, int rlayout) {
    using G = FmF32GeomT<NP_, NFP_, M_>;
    constexpr int NP = G::NP, NFP = G::NFP, NF = G::NF, M = G::M;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    typename G::WaveIn* L = reinterpret_cast<typename G::WaveIn*>(smem) + wave;
    float* ob = reinterpret_cast<float*>(smem + G::IN_BYTES) + wave * G::SUB_F;
    const int n = lane & 15, g = lane >> 4;
    const unsigned bid = blockIdx.x, nblk = gridDim.x;
    const int64_t stride = (int64_t)nblk * G::WAVES, tEnd = nTiles;
    const int64_t first = (int64_t)bid * G::WAVES + wave;
    const unsigned lds_v0 = lds_addr_uniform(L->v[0]), lds_j0 = lds_addr_uniform(L->j[0]);

    auto issue_unit = [&](int64_t t, int k, int slot) {
        const int64_t e0 = t * G::TEL;
        const char* vb = reinterpret_cast<const char*>(field_in_f32(P, k) + e0 * NFP) + lane * 16;
#pragma unroll
        for (int f = 0; f < NF; ++f)
#pragma unroll
            for (int c = 0; c < G::SLAB_INSTR; ++c)
                if ((c + 1) * 64 <= G::SLAB_CHUNKS || c * 64 + lane < G::SLAB_CHUNKS)
                    glds16_nt(vb + (int64_t)f * E * (NFP * 4) + c * 1024, lds_v0 + slot * (G::UNIT_F * 4) + f * (G::SLAB_F * 4) + c * 1024);
        if (k == 0) {   // the tile's J: "fe": 4 rows of TEL floats, else TEL x 4 contiguous floats
#pragma unroll
            for (int c = 0; c < G::J_INSTR; ++c) {
                const int q = c * 64 + lane;
                const int row = q / (G::TEL / 4), col = q - row * (G::TEL / 4);
                const char* src = jfe ? reinterpret_cast<const char*>(J + (int64_t)row * E + e0) + col * 16
                                      : reinterpret_cast<const char*>(J + e0 * NF) + q * 16;
                if ((c + 1) * 64 <= G::J_CHUNKS || q < G::J_CHUNKS) glds16(src, lds_j0 + slot * (NF * G::TEL * 4) + c * 1024);
            }
        }
    };
    auto advance = [&](int64_t& t, int& k) {
        if (++k == nb) { k = 0; t += stride; }
    };

    // ---- units 0 and 1 of this wave, and behind them the operator -> LDS (over the output buffers; through registers, as in fe_div_f32.h)
    int64_t tile = first, t1 = first, t2;
    int fk = 0, k1 = 0, k2;
    advance(t1, k1);
    t2 = t1, k2 = k1;
    advance(t2, k2);
    if (tile < tEnd) {
        issue_unit(tile, 0, 0);
        if (t1 < tEnd) issue_unit(t1, k1, 1);
    }
    const float* rl = reinterpret_cast<const float*>(smem + G::IN_BYTES);
    stage_operator<G::OP_F>(R, reinterpret_cast<float*>(smem + G::IN_BYTES));
    __syncthreads();

    // operator layouts: 0 R[f][i][j], 1 L[i][f][j], 2 R[f][j][i], 3 L[j][f][i] -> strides of f, i, j
    const int sF = rlayout == 0 ? NP * NFP : rlayout == 1 ? NFP : rlayout == 2 ? NFP * NP : NP;
    const int sI = rlayout == 0 ? NFP : rlayout == 1 ? NF * NFP : 1;
    const int sJ = rlayout == 0 || rlayout == 1 ? 1 : rlayout == 2 ? NP : NF * NP;
    // ---- per-lane K decomposition (k = 4 ks + g = Nfp f + j: offsets of sub-tile 0) and A fragments: lane (g, n) supplies
    //      A[row 16 t + n][k = g] of a 16-row tile, A[row 16 BT + 4 q + n % 4][k = g] of 4-row group q
    int voff[G::KS], joff[G::KS];
    float abig[G::BT > 0 ? G::BT : 1][G::KS], asmall[G::NS > 0 ? G::NS : 1][G::KS];
#pragma unroll
    for (int ks = 0; ks < G::KS; ++ks) {
        const int k = 4 * ks + g, f = k / NFP, j = k - f * NFP;
        voff[ks] = f * G::SLAB_F + n * NFP + j;
        joff[ks] = jfe ? f * G::TEL + n : n * NF + f;
#pragma unroll
        for (int t = 0; t < G::BT + G::NS; ++t) {   // the 16-row tiles, then the 4-row groups
            constexpr int BT = G::BT;
            const bool big = t < BT;
            const int i = big ? 16 * t + n : 16 * BT + 4 * (t - BT) + (n & 3);
            const float a = rl[f * sF + (i < NP ? i : 0) * sI + j * sJ];
            (big ? abig[big ? t : 0] : asmall[big ? 0 : t - BT])[ks] = i < NP ? a : 0.f;   // (the clamps keep the dead arm in bounds)
        }
    }
    {   // the elements behind the last full tile, with the operator from the block's LDS copy (see fe_grad_f32.h)
        const int64_t jEs = jfe ? 1 : NF, jFs = jfe ? E : 1;
        remainder_items(nTiles * G::TEL, E, NP, bid, nblk, [&](int64_t e, int i) {
            for (int k = 0; k < nb; ++k) {
                const float* vk = field_in_f32(P, k);
                float acc = 0.f;
                for (int f = 0; f < NF; ++f) {
                    const float jf = J[e * jEs + f * jFs];
                    for (int j = 0; j < NFP; ++j)
                        acc = __builtin_fmaf(rl[f * sF + i * sI + j * sJ], jf * vk[((int64_t)f * E + e) * NFP + j], acc);
                }
                field_out_f32(P, k)[e * NP + i] = acc;
            }
        });
    }
    __syncthreads();   // the staging area becomes the waves' output buffers

    int slot = 0, done = 0, iteration = 0;
    float jv[M][G::KS];
    const bool younger_half = bid >= (nblk + 1) / 2;
    while (tile < tEnd) {
        if (fk == 0) balance_priority(younger_half, iteration++);
        // ---- wait for this unit's loads; younger ops: S(m-2), L(m+1), S(m-1)
        if (done >= 2 && t1 < tEnd) {
            if (k1 == 0) wait_vmcnt<2 * G::UNIT_STORES + G::UNIT_LOADS + G::J_INSTR>();
            else wait_vmcnt<2 * G::UNIT_STORES + G::UNIT_LOADS>();
        } else {
            wait_vmcnt<0>();
        }
        const float* vs = L->v[slot];
        if (fk == 0) {
            const float* js = L->j[slot];
#pragma unroll
            for (int m = 0; m < M; ++m)
#pragma unroll
                for (int ks = 0; ks < G::KS; ++ks) jv[m][ks] = js[joff[ks] + (jfe ? 16 * m : 16 * m * NF)];
        }
        float bfrag[M][G::KS];
#pragma unroll
        for (int m = 0; m < M; ++m)
#pragma unroll
            for (int ks = 0; ks < G::KS; ++ks) bfrag[m][ks] = jv[m][ks] * vs[voff[ks] + 16 * m * NFP];
        // the slabs (and, at a tile start, the J tile) are in registers before the slot is handed back to the DMA engine
#pragma unroll
        for (int m = 0; m < M; ++m)
#pragma unroll
            for (int ks = 0; ks < G::KS; ++ks) asm volatile("" : "+v"(bfrag[m][ks]));
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        if (t2 < tEnd) issue_unit(t2, k2, slot);

#pragma unroll
        for (int m = 0; m < M; ++m) {
            v4f accb[G::BT > 0 ? G::BT : 1], accq[G::NS > 0 ? G::NS : 1];
#pragma unroll
            for (int t = 0; t < G::BT; ++t) accb[t] = v4f{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int q = 0; q < G::NS; ++q) accq[q] = v4f{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < G::KS; ++ks) {
#pragma unroll
                for (int t = 0; t < G::BT; ++t) accb[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(abig[t][ks], bfrag[m][ks], accb[t], 0, 0, 0);
#pragma unroll
                for (int q = 0; q < G::NS; ++q) accq[q] = __builtin_amdgcn_mfma_f32_4x4x1f32(asmall[q][ks], bfrag[m][ks], accq[q], 0, 0, 0);
            }
            // ---- into the transposition buffer, as in fe_div_f32.h
#pragma unroll
            for (int t = 0; t < G::BT; ++t)
#pragma unroll
                for (int v = 0; v < 4; ++v) ob[(16 * m + n) * NP + 16 * t + 4 * g + v] = accb[t][v];
#pragma unroll
            for (int q = 0; q < G::NS; ++q)
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    if (16 * G::BT + 4 * q + v < NP) {
                        float x = accq[q][v];
                        x += __shfl_xor(x, 16);
                        x += __shfl_xor(x, 32);
                        if (g == 0) ob[(16 * m + n) * NP + 16 * G::BT + 4 * q + v] = x;
                    }
                }
        }
        wave_lds_fence();
        float* op = field_out_f32(P, fk) + tile * (G::TEL * NP);
#pragma unroll
        for (int c = 0; c < G::SUB_INSTR; ++c) {
            const int q = c * 64 + lane;
            if ((c + 1) * 64 <= G::SUB_CHUNKS || q < G::SUB_CHUNKS) {
                const v4f val = *reinterpret_cast<const v4f*>(ob + 4 * q);
                __builtin_nontemporal_store(val, reinterpret_cast<v4f*>(op + 4 * q));
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

}  // namespace fe
