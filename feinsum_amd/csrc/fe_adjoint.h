// fe_adjoint.h -- the two adjoint kernels of the DG families that no forward kernel covers.
//
//   geomadj       out[x, r, e] = sum_i (sum_j K[r, i, j] a[e, j]) b[x, e, i]          X, R in {1, 2, 3}
//                 K = D ([R][Np][Np]) or, with opT, D with its last two axes swapped.  It is the gradient of every
//                 DG family with respect to its geometric factors: grad (a = u, b = dout), div (K = D^T, a = dout,
//                 b = u), the div component (X = 1) and the element-local operator (X = R = 1).
//   facemass_adj  w_k[f, j, e] = sum_i R[f, i, j] g_k[e, i]
//                 dv_k[f, e, j] = J[e, f] w_k[f, j, e]                                (dv: optional)
//                 dJ[e, f]      = sum_k sum_j w_k[f, j, e] v_k[f, e, j]               (v: optional)
//
// Schedule (both).  A wave owns a tile of 16 elements; a block of four waves walks the tiles statically (tile
// w + 4 blockIdx + 4 gridDim k) over a persistent grid, so the operator is staged into LDS once per block, already in
// the A-fragment order of v_mfma_f64_16x16x4_f64 ([r][row tile][k step][lane], zero-padded rows and columns): each
// lane reads its fragment with one conflict-free 8-byte LDS read.  The element-local factor (a, resp. g_k) is the B
// operand, read straight from global memory: lane l takes column e = 16 tile + (l & 15) and k = 4 ks + (l >> 4),
// four consecutive doubles per element per instruction.  The accumulator of row tile t holds, in lane l and register
// q, the product for row 16 t + (l >> 4) + 4 q and column (element) l & 15.
//   geomadj then multiplies with b[x, e, row] (VALU), sums the lane's four rows of every row tile and the four lanes of
//   an element (two xor shuffles over 16 and 32 lanes); the lanes of the first quarter write out[x, r, e].
//   facemass_adj maps row -> (f, j) = (row / Nfp, row % Nfp) over the nf Nfp rows of R^T, writes J[e, f] w to dv_k and
//   sums w v_k per face in registers; dJ is reduced like geomadj's output.  The fields are summed in their order,
//   the rows in a fixed order and the lanes by a fixed shuffle tree, so every output is bitwise reproducible.
// Rows and columns past the shape are zero in the fragments and guarded at the loads and stores; so are elements
// past E -- a partial last tile costs no separate path.
#pragma once
#include "../../include/feinsum_hip.h"
#include "fe_common.h"

namespace fe {

constexpr int kAdjThreads = 256;   // four waves per block
constexpr int kAdjWaves = kAdjThreads / 64;

template <int NP>
struct GeomAdjGeom {
    static constexpr int T = (NP + 15) / 16;   // row tiles of K (rows i)
    static constexpr int KS = (NP + 3) / 4;    // k steps (columns j)
    static constexpr int LDS_DOUBLES_PER_R = T * KS * 64;
};

struct GeomAdjArgs {
    const double* D;   // [R][Np][Np] (opT: [R][Np(j)][Np(i)])
    const double* a;   // [E][Np]
    const double* b;   // [X][E][Np]
    double* out;       // out[x * sx + r * sr + e * se]
    int64_t E, sx, sr, se;
    int X, R, opT;
};

template <int NP>
__global__ __launch_bounds__(kAdjThreads) void geomadj_kernel(GeomAdjArgs g) {
    using G = GeomAdjGeom<NP>;
    extern __shared__ __attribute__((aligned(16))) char adj_sm[];
    double* Af = reinterpret_cast<double*>(adj_sm);   // [R][T][KS][64]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int X = g.X, R = g.R;

    // ---- operator -> LDS in fragment order
    for (int idx = tid; idx < R * G::LDS_DOUBLES_PER_R; idx += kAdjThreads) {
        const int r = idx / G::LDS_DOUBLES_PER_R, rem = idx - r * G::LDS_DOUBLES_PER_R;
        const int t = rem / (G::KS * 64), rem2 = rem - t * (G::KS * 64);
        const int ks = rem2 >> 6, l = rem2 & 63;
        const int i = 16 * t + (l & 15), j = 4 * ks + (l >> 4);
        double v = 0.0;
        if (i < NP && j < NP) v = g.D[(int64_t)r * NP * NP + (g.opT ? j * NP + i : i * NP + j)];
        Af[idx] = v;
    }
    __syncthreads();

    const int c = lane & 15, h = lane >> 4;
    const int64_t E = g.E;
    const int64_t n_tiles = (E + 15) / 16;
    for (int64_t tile = (int64_t)blockIdx.x * kAdjWaves + wave; tile < n_tiles; tile += (int64_t)gridDim.x * kAdjWaves) {
        const int64_t e = tile * 16 + c;
        const bool ok = e < E;
        double bfrag[G::KS];
#pragma unroll
        for (int ks = 0; ks < G::KS; ++ks) {
            const int j = 4 * ks + h;
            bfrag[ks] = (ok && j < NP) ? g.a[e * NP + j] : 0.0;
        }
        double bv[3][G::T][4];
#pragma unroll
        for (int x = 0; x < 3; ++x)
#pragma unroll
            for (int t = 0; t < G::T; ++t)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int i = 16 * t + h + 4 * q;
                    bv[x][t][q] = (x < X && ok && i < NP) ? g.b[((int64_t)x * E + e) * NP + i] : 0.0;
                }
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            if (r >= R) break;
            v4d acc[G::T];
#pragma unroll
            for (int t = 0; t < G::T; ++t) acc[t] = v4d{0.0, 0.0, 0.0, 0.0};
            const double* ar = Af + r * G::LDS_DOUBLES_PER_R + lane;
#pragma unroll
            for (int ks = 0; ks < G::KS; ++ks)
#pragma unroll
                for (int t = 0; t < G::T; ++t)
                    acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(ar[(t * G::KS + ks) * 64], bfrag[ks], acc[t], 0, 0, 0);
#pragma unroll
            for (int x = 0; x < 3; ++x) {
                if (x >= X) break;
                double s = 0.0;
#pragma unroll
                for (int t = 0; t < G::T; ++t)
#pragma unroll
                    for (int q = 0; q < 4; ++q) s = fma(acc[t][q], bv[x][t][q], s);
                s += __shfl_xor(s, 16, 64);
                s += __shfl_xor(s, 32, 64);
                if (h == 0 && ok) g.out[x * g.sx + r * g.sr + e * g.se] = s;
            }
        }
    }
}

template <int NP, int NFP, int NF>
struct FmAdjGeom {
    static constexpr int NR = NF * NFP;        // rows (f, j) of R^T
    static constexpr int T = (NR + 15) / 16;   // row tiles
    static constexpr int KS = (NP + 3) / 4;    // k steps (i)
    static constexpr int LDS_DOUBLES = T * KS * 64;
};

struct FmAdjArgs {
    const double* J;       // J[e * sje + f * sjf] (read for dv only)
    const double* R;       // R[f * sF + i * sI + j * sJ]
    FieldPtrs g;           // g.v[k]: dout_k [E][Np];  g.out[k]: dv_k [nf][E][Nfp] or all null
    FieldPtrs v;           // v.v[k]: v_k [nf][E][Nfp] (read for dJ only)
    double* dJ;            // dJ[e * sje + f * sjf], or null
    int64_t E, sje, sjf;
    int sF, sI, sJ, nb, with_dv, accumulate;   // accumulate: dJ += (a second chunk of fields)
};

template <int NP, int NFP, int NF>
__global__ __launch_bounds__(kAdjThreads) void facemass_adj_kernel(FmAdjArgs g) {
    using G = FmAdjGeom<NP, NFP, NF>;
    extern __shared__ __attribute__((aligned(16))) char adj_sm[];
    double* Af = reinterpret_cast<double*>(adj_sm);   // [T][KS][64]: A[row = (f, j)][k = i] = R[f, i, j]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

    for (int idx = tid; idx < G::LDS_DOUBLES; idx += kAdjThreads) {
        const int t = idx / (G::KS * 64), rem = idx - t * (G::KS * 64);
        const int ks = rem >> 6, l = rem & 63;
        const int row = 16 * t + (l & 15), i = 4 * ks + (l >> 4);
        double val = 0.0;
        if (row < G::NR && i < NP) {
            const int f = row / NFP, j = row - f * NFP;
            val = g.R[(int64_t)f * g.sF + (int64_t)i * g.sI + (int64_t)j * g.sJ];
        }
        Af[idx] = val;
    }
    __syncthreads();

    const int c = lane & 15, h = lane >> 4;
    const int64_t E = g.E;
    const int64_t n_tiles = (E + 15) / 16;
    const bool with_dJ = g.dJ != nullptr;
    for (int64_t tile = (int64_t)blockIdx.x * kAdjWaves + wave; tile < n_tiles; tile += (int64_t)gridDim.x * kAdjWaves) {
        const int64_t e = tile * 16 + c;
        const bool ok = e < E;
        double jv[NF];
#pragma unroll
        for (int f = 0; f < NF; ++f) jv[f] = (g.with_dv && ok) ? g.J[e * g.sje + f * g.sjf] : 0.0;
        double pf[NF];
#pragma unroll
        for (int f = 0; f < NF; ++f) pf[f] = 0.0;
        for (int k = 0; k < g.nb; ++k) {
            const double* gk = field_in(g.g, k);
            double bfrag[G::KS];
#pragma unroll
            for (int ks = 0; ks < G::KS; ++ks) {
                const int i = 4 * ks + h;
                bfrag[ks] = (ok && i < NP) ? gk[e * NP + i] : 0.0;
            }
            v4d acc[G::T];
#pragma unroll
            for (int t = 0; t < G::T; ++t) acc[t] = v4d{0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int ks = 0; ks < G::KS; ++ks)
#pragma unroll
                for (int t = 0; t < G::T; ++t)
                    acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(Af[(t * G::KS + ks) * 64 + lane], bfrag[ks], acc[t], 0, 0, 0);
            double* dvk = g.with_dv ? field_out(g.g, k) : nullptr;
            const double* vk = with_dJ ? field_in(g.v, k) : nullptr;
#pragma unroll
            for (int t = 0; t < G::T; ++t)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int row = 16 * t + h + 4 * q;
                    if (!ok || row >= G::NR) continue;
                    const int f = row / NFP, j = row - f * NFP;
                    const int64_t at = ((int64_t)f * E + e) * NFP + j;
                    const double w = acc[t][q];
                    if (g.with_dv) {
                        double jf = jv[0];
#pragma unroll
                        for (int ff = 1; ff < NF; ++ff) jf = f == ff ? jv[ff] : jf;
                        dvk[at] = jf * w;
                    }
                    if (with_dJ) {
                        const double p = w * vk[at];
#pragma unroll
                        for (int ff = 0; ff < NF; ++ff)
                            if (f == ff) pf[ff] += p;
                    }
                }
        }
        if (with_dJ) {
#pragma unroll
            for (int f = 0; f < NF; ++f) {
                double s = pf[f];
                s += __shfl_xor(s, 16, 64);
                s += __shfl_xor(s, 32, 64);
                if (h == 0 && ok) {
                    double* d = g.dJ + e * g.sje + f * g.sjf;
                    *d = g.accumulate ? *d + s : s;
                }
            }
        }
    }
}

}  // namespace fe
