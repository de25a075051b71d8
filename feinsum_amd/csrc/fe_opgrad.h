// fe_opgrad.h -- the gradients of the DG families with respect to their operator matrices:
// the element axis is summed into a small [R][Np][Np] (face-mass: [nf][Np][Nfp]) output on the matrix cores.
//
//   volume     out[r sr + p sp + q sq] = sum_k sum_e (sum_x J[x jx + r jr + e je] b_k[x][e][p]) a_k[e][q]
//              b carries the X planes (grad: the output gradient, div: u; X = 1 for the div component and the
//              element-local operator), a is the plain [E][Np] factor; (sp, sq) express the i / j role swap and a
//              transposed operator, the J strides its layouts 'xre', 're', 'er', 'e'.
//   face-mass  dR[f sr + j sp + i sq]  = sum_k sum_e (J[f jr + e je] v_k[f][e][j]) g_k[e][i]
//              the same kernel with r = f, X = 1, rows j < Nfp of plane f of v_k, columns i < Np of g_k.
//
// Schedule.  The element axis is the k dimension of v_mfma_f64_16x16x4_f64: four elements per instruction.  E is cut
// into S slices of slice_len elements (a multiple of 16; S and slice_len come from fe_opgrad_plan: E alone decides
// them, never the device).  Block s of 256 threads owns slice s.  Per chunk of 16 elements and per field it stages
// a_k (16 rows), the planes of b_k and the chunk's J values into LDS (the spans are contiguous in global memory),
// elements at or past E selected to zero and never loaded.  Rows of a and b lie in LDS with a stride of 16 or 48
// doubles (= 16 mod 32: the two rows a half-wave reads cover all 64 banks once) whose columns past the shape stay
// zero.  The four waves split the (r, row tile) pairs.  For a pair a lane forms the J-weighted factor
// W[e][p] = sum_x J[x, r, e] b[x][e][p] on the VALU, already in the A-fragment layout (lane l: row p = 16 t + (l & 15),
// k = l >> 4), and reuses it over the column tiles, whose B fragments (a[e][q], q = 16 t' + (l & 15)) are shared by the
// wave's pairs.  The accumulator of lane l, register i is row (l >> 4) + 4 i, column l & 15 of its tile.
// After its slice a block writes the live entries of its tiles into slice s of the workspace, in the output's layout;
// the combine of fe_reduce.h then sums the slices of every entry in slice order with its fixed tree.  No atomics:
// chunks, fields (in their order inside a chunk), planes and slices are summed in a fixed order, so the result is
// bitwise reproducible.  More than kOgMaxFields fields take several launches; the later ones add to their own slice.
#pragma once
#include "../../include/feinsum_hip.h"
#include "fe_common.h"

namespace fe {

constexpr int kOgThreads = 256;   // four waves per block
constexpr int kOgWaves = kOgThreads / 64;
constexpr int kOgChunk = 16;      // elements per staged chunk (four k steps)
constexpr int kOgMaxFields = 8;
constexpr int kOgMaxR = 4;        // r < 3 (volume), f < 4 (face-mass)

constexpr int og_row_stride(int n) {   // >= 16 ceil(n / 16) and = 16 mod 32
    const int t = (n + 15) / 16 * 16;
    return t % 32 == 0 ? t + 16 : t;
}

template <int NM, int NN, bool FACE>
struct OpGradGeom {
    static constexpr int TM = (NM + 15) / 16, TN = (NN + 15) / 16;   // row / column tiles
    static constexpr int SB = og_row_stride(NM), SA = og_row_stride(NN);
    static constexpr int PL = FACE ? kOgMaxR : 3;                    // planes of b staged per chunk, at most
    static constexpr int MAXR = FACE ? kOgMaxR : 3;
    static constexpr int MAXP = (MAXR * TM + kOgWaves - 1) / kOgWaves;   // (r, row tile) pairs per wave, at most
    static constexpr int LDS_DOUBLES = kOgChunk * SA + PL * kOgChunk * SB + 3 * MAXR * kOgChunk;
};

struct OpGradArgs {
    const double* J;                  // J[x jx + r jr + e je]
    const double* a[kOgMaxFields];    // a_k [E][NN]
    const double* b[kOgMaxFields];    // b_k: plane (x resp. f) at pl * E * NM, then [E][NM]
    double* ws;                       // [S][n_out]
    int64_t E, slice_len, n_out;
    int64_t jx, jr, je, sr, sp, sq;
    int X, R, nb, accumulate;
};

__device__ __forceinline__ const double* og_field(const double* const (&P)[kOgMaxFields], int k) {   // see field_in
    const double* p = P[0];
#pragma unroll
    for (int q = 1; q < kOgMaxFields; ++q) p = (k == q) ? P[q] : p;
    return p;
}

template <int NM, int NN, bool FACE>
__global__ __launch_bounds__(kOgThreads, 4) void opgrad_partial_kernel(OpGradArgs g) {
    using G = OpGradGeom<NM, NN, FACE>;
    extern __shared__ __attribute__((aligned(16))) char og_sm[];
    double* La = reinterpret_cast<double*>(og_sm);   // [16][SA]
    double* Lb = La + kOgChunk * G::SA;              // [planes][16][SB]
    double* Lj = Lb + G::PL * kOgChunk * G::SB;      // [x R + r][16]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c = lane & 15, h = lane >> 4;
    const int X = FACE ? 1 : g.X, R = g.R;
    const int planes = FACE ? R : X;
    const int64_t E = g.E;

    for (int idx = tid; idx < G::LDS_DOUBLES; idx += kOgThreads) La[idx] = 0.0;   // the padding columns stay zero

    v4d acc[G::MAXP][G::TN];
#pragma unroll
    for (int m = 0; m < G::MAXP; ++m)
#pragma unroll
        for (int t = 0; t < G::TN; ++t) acc[m][t] = v4d{0.0, 0.0, 0.0, 0.0};

    const int64_t e_begin = (int64_t)blockIdx.x * g.slice_len;
    const int64_t e_stop = e_begin + g.slice_len < E ? e_begin + g.slice_len : E;
    for (int64_t e0 = e_begin; e0 < e_stop; e0 += kOgChunk) {
        for (int k = 0; k < g.nb; ++k) {
            const double* ak = og_field(g.a, k);
            const double* bk = og_field(g.b, k);
            __syncthreads();   // the chunk before this one has been read (and the zero fill is done)
            for (int idx = tid; idx < kOgChunk * NN; idx += kOgThreads) {
                const int e = idx / NN, q = idx - e * NN;
                La[e * G::SA + q] = e0 + e < E ? ak[e0 * NN + idx] : 0.0;
            }
            for (int idx = tid; idx < planes * (kOgChunk * NM); idx += kOgThreads) {
                const int pl = idx / (kOgChunk * NM), rem = idx - pl * (kOgChunk * NM);
                const int e = rem / NM, p = rem - e * NM;
                Lb[(pl * kOgChunk + e) * G::SB + p] = e0 + e < E ? bk[((int64_t)pl * E + e0) * NM + rem] : 0.0;
            }
            if (tid < X * R * kOgChunk) {
                const int xr = tid >> 4, e = tid & 15;
                const int x = xr / R, r = xr - x * R;
                Lj[tid] = e0 + e < E ? g.J[x * g.jx + r * g.jr + (e0 + e) * g.je] : 0.0;
            }
            __syncthreads();
#pragma unroll
            for (int ks = 0; ks < kOgChunk / 4; ++ks) {
                const int e = 4 * ks + h;
                double bf[G::TN];
#pragma unroll
                for (int t = 0; t < G::TN; ++t) bf[t] = La[e * G::SA + 16 * t + c];
#pragma unroll
                for (int m = 0; m < G::MAXP; ++m) {
                    const int pair = wave + kOgWaves * m;   // wave-uniform
                    if (pair >= R * G::TM) break;
                    const int r = pair / G::TM, tp = pair - r * G::TM;
                    double w;
                    if (FACE) {
                        w = Lj[r * kOgChunk + e] * Lb[(r * kOgChunk + e) * G::SB + 16 * tp + c];
                    } else {
                        w = 0.0;
                        for (int x = 0; x < X; ++x)
                            w = fma(Lj[(x * R + r) * kOgChunk + e], Lb[(x * kOgChunk + e) * G::SB + 16 * tp + c], w);
                    }
#pragma unroll
                    for (int t = 0; t < G::TN; ++t)
                        acc[m][t] = __builtin_amdgcn_mfma_f64_16x16x4f64(w, bf[t], acc[m][t], 0, 0, 0);
                }
            }
        }
    }

    double* ws = g.ws + (int64_t)blockIdx.x * g.n_out;
#pragma unroll
    for (int m = 0; m < G::MAXP; ++m) {
        const int pair = wave + kOgWaves * m;
        if (pair >= R * G::TM) break;
        const int r = pair / G::TM, tp = pair - r * G::TM;
#pragma unroll
        for (int t = 0; t < G::TN; ++t)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int p = 16 * tp + h + 4 * i, q = 16 * t + c;
                if (p < NM && q < NN) {   // padded rows and columns are never stored
                    double* d = ws + r * g.sr + p * g.sp + q * g.sq;
                    *d = g.accumulate ? *d + acc[m][t][i] : acc[m][t][i];
                }
            }
    }
}

}  // namespace fe
