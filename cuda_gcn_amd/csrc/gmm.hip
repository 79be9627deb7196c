// gmm.hip — a Gaussian mixture (diagonal or spherical covariances) of the rows of a trained model's hidden layer by expectation
// maximisation: soft clusters, a density per row, a likelihood to compare k by.  Beyond the reference, which never looks at its hidden
// matrix.  include/gcnhip_driver.h has the call contracts.
//
// Rows.  The table contract is kmeans.hip's: f32 [n_table x ld], 1 <= dim <= 256, dim <= ld, rows of any stride and alignment, columns
// [dim, ld) never read; d_rows a device int32 list of n positions (repeats are points of their own; NULL: rows 0 .. n - 1), an entry
// outside [0, n_table) is no point.  1 <= k <= 256.  All arithmetic is on the SHIFTED row x'[j] = (T[r][j] . inv_norm[r]) - shift[j]:
// one rounded f32 multiply (none with inv_norm == NULL) and one rounded f32 subtract when a row is staged; shift [dim] is the caller's
// (the f32-rounded mean of the rows: ReLU rows sit far from the origin, and both the expanded form below and S2 / N - mu^2 cancel
// badly without it).  Means live shifted as well, mu' = mu - shift.
// Operands of a component c, written by gcnhip_gmm_finalize in float64 and rounded to f32 once: prec[c][j] = 1 / var, mprec[c][j] =
// mu' / var, cst[c] = log w_c - (sum_j (mu'^2 / var + log var) + dim log 2 pi) / 2, the sum in column order.
//
// gcnhip_gmm_estep   lj[i][c] = fma(-0.5, q(i, c), cst[c]) (one rounding), q ONE chain of v_mfma_f32_16x16x4_f32 over 2 G 16-column
//   groups, G = ceil(dim / 16): group g < G takes A = prec[c][16 g ..], B = x'^2 (the rounded f32 square, formed from the registers
//   as it is used), group G + g takes A = -2 mprec[c][16 g ..] (exact), B = x'; inside a group step s = 0..3 with k-slot kg = 0..3 on
//   column 16 g + 4 kg + s; columns >= dim are zeros.  So q has 32 G fma steps, and with u = 2^-24 and
//   a(i, c) = sum_j (x'^2 prec + 2 |x' mprec|) / 2 over the f32 operands, |lj - lj_exact| <= gamma(32 G + 2) a + u |cst|,
//   gamma(m) = m u / (1 - m u): the chain, the rounding of the square, and the final fma's rounding split over its two terms.
//   A workgroup of 256 threads owns 64 list positions (grid-stride over position tiles); wave w owns positions 16 w .. 16 w + 15 and
//   lane (kg, l15) holds x' of position 16 w + l15, columns 16 g + 4 kg .. + 3, as the B operand in REGISTERS.  Components stream
//   through LDS in tiles of 64 rows [prec | -2 mprec] of 2 (dpad + 4) floats, dpad = 16 G: one buffer for dim > 128 (133 KB at 256),
//   two for dim <= 128 with the next tile's loads in flight across the products; with k <= 64 the tile is loaded once per workgroup.
//   Each lane then holds 16 entries of its one row per tile: component 64 t + 16 a + 4 kg + r.  Per tile: the tile's maximum; if it
//   exceeds the running maximum m the running sum s is rescaled by expf(m - max); then s += expf(lj - m) in ascending component.
//   The four lane groups of a row meet by two shuffles: M = max(m, m'), s = s expf(m - M) + s' expf(m' - M) (a group that holds
//   nothing but -inf adds 0).  lse = M + logf(s); assign = the largest lj, lowest component on a tie; max_resp = expf(lj_max - lse).
//   The order is a function of k alone, never of the launch.  A position that is no point: lj, lse, max_resp NaN, assign -1.
//   lse_sum: float64, per part of GM_PART positions thread t adds positions t, t + 256, t + 512, t + 768 of the part in order (no
//   point: nothing), a tree over the 256 threads (t += t + w, w = 128 .. 1); then thread t adds partials t, t + 256, .. and the same tree.
// gcnhip_gmm_mstep   sums[c][0] = N_c = sum_i r_ic, sums[c][1 + j] = sum_i r_ic x'_ij, sums[c][1 + dim + j] = sum_i r_ic x'_ij^2,
//   r_ic = (double)expf(lj_ic - lse_i), or with lj == NULL the indicator assign[i] == c; x' widened, its square taken in float64
//   (exact).  Products and sums are float64 on v_mfma_f64_16x16x4_f64: A = 16 components x 4 positions of r, B = 4 positions x 16
//   columns of [1 | x' | x'^2]; a position that is no point and one past the end enter as exact zeros.  The list is cut into parts of
//   GM_PART positions; a workgroup owns (part, 16 components), wave w the column slabs w, w + 4, .., and adds the part's positions in
//   ascending order, four per MFMA.  The parts' partials are added in part order by a second launch; a call handles as many parts per
//   launch as its scratch holds: less scratch, more launches, the same sequence of additions.
// gcnhip_gmm_finalize  per component, float64: N < 10 . 2^-52 . n: not fitted — mu', var and the operands stay, weight 0, cst -inf, so
//   it never wins and never makes a NaN.  Else w = N / sum_c N (ascending c), mu' = S1 / N, var = max(S2 / N - mu'^2, 0) + reg_covar,
//   spherical: the mean of the row's var in column order, in every column.  With sums == NULL the operands are made from mu', var and
//   weights as they lie (f32, widened): the form a fit handed back takes.
// No float atomics, no allocation, no synchronisation; every output's bits are a function of the arguments' contents alone.
// -Rpass-analysis=kernel-resource-usage for gfx950: DESIGN 4.30 has the table; no kernel of this file uses scratch.
#include "common.h"
#include <algorithm>
#include <cmath>
#include <cstdio>

using f32x4 = __attribute__((ext_vector_type(4))) float;
using f64x4 = __attribute__((ext_vector_type(4))) double;

constexpr int GM_T = 64;                          // list positions per workgroup tile, components per LDS tile
constexpr int GM_MAX_DIM = 256, GM_MAX_K = 256;
constexpr int GM_PART = 1024;                     // positions per part (part of the definition of the sums' order)
constexpr int GM_FOLD = 16;                       // partials a fold thread has in flight (no part of any sum's order)

struct GmTable {
    const float *data;
    int ld, n, dim;
    const float *inv_norm;
    const int32_t *rows;
    int vec_ok, nch;                              // rows are 16-byte aligned; 16-column groups that hold a column below dim
};

__device__ __forceinline__ int gm_list_row(const GmTable &T, int i) {
    const int r = T.rows ? T.rows[i] : i;
    return r >= 0 && r < T.n ? r : -1;
}

// columns col .. col + 3 of a row of `dim` values at p; zeros past dim
__device__ __forceinline__ f32x4 gm_load4(const float *__restrict__ p, int col, int dim, int vec_ok) {
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (vec_ok && col + 3 < dim) return *(const f32x4 *)(p + col);
    if (col < dim) v.x = p[col];
    if (col + 1 < dim) v.y = p[col + 1];
    if (col + 2 < dim) v.z = p[col + 2];
    if (col + 3 < dim) v.w = p[col + 3];
    return v;
}

// x' of one entry: the rounded product, then the rounded difference — never one fma (the rounding intrinsics of this toolchain are
// plain operators, which the compiler may contract)
__device__ __forceinline__ float gm_shifted(float x, float inv, float shift) {
#pragma clang fp contract(off)
    const float p = x * inv;
    return p - shift;
}

// ---- E-step -------------------------------------------------------------------------------------------------------------------

struct GmComp {                                   // the component operands
    const float *prec, *mprec, *cst;
    int ldc, k, vec_ok;
};

// float4 `idx` of component tile ct, idx < 64 . DP / 2: row = idx / (DP / 2), then [prec | -2 mprec] of DP / 4 float4 each
template <int DP>
__device__ __forceinline__ f32x4 gm_comp_load(const GmComp &K, int dim, int ct, int idx) {
    const int row = idx / (DP / 2), c4 = idx % (DP / 2), second = c4 >= DP / 4, col = 4 * (c4 % (DP / 4));
    const int c = ct * GM_T + row;
    if (c >= K.k) return f32x4{0.f, 0.f, 0.f, 0.f};
    const f32x4 v = gm_load4((second ? K.mprec : K.prec) + (size_t)c * K.ldc, col, dim, K.vec_ok);
    return second ? -2.f * v : v;
}
template <int DP>
__device__ __forceinline__ void gm_comp_store(float *__restrict__ Cs, int half, int idx, f32x4 v) {
    const int row = idx / (DP / 2), c4 = idx % (DP / 2), second = c4 >= DP / 4, col = 4 * (c4 % (DP / 4));
    *(f32x4 *)(Cs + row * 2 * half + second * half + col) = v;
}
// a whole tile, memory to LDS
template <int DP>
__device__ __forceinline__ void gm_comp_copy(const GmComp &K, int dim, int nch, int ct, float *__restrict__ Cs, float *__restrict__ Ks) {
    const int half = 16 * nch + 4;
#pragma unroll 4
    for (int u = 0; u < DP / 8; u++) {
        const int idx = threadIdx.x + 256 * u;
        if (4 * (idx % (DP / 4)) < 16 * nch) gm_comp_store<DP>(Cs, half, idx, gm_comp_load<DP>(K, dim, ct, idx));
    }
    if (threadIdx.x < GM_T) {
        const int c = ct * GM_T + (int)threadIdx.x;
        Ks[threadIdx.x] = c < K.k ? K.cst[c] : -INFINITY;
    }
}

// THE product body: acc[a][r] = q(this lane's row, component 16 a + 4 kg + r of the tile), one MFMA chain per entry
template <int DP>
__device__ __forceinline__ void gm_products(const float *__restrict__ Cs, const f32x4 (&b)[DP / 16], f32x4 (&acc)[4], int nch, int kg, int l15) {
    const int half = 16 * nch + 4, S = 2 * half;
#pragma unroll
    for (int a = 0; a < 4; a++) acc[a] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int h = 0; h < 2; h++)
#pragma unroll
        for (int g = 0; g < DP / 16; g++) {
            if (g >= nch) continue;                              // the same for every thread (no break: b[] keeps static indices)
            f32x4 bv = b[g];
            if (h == 0) {
#pragma unroll
                for (int s = 0; s < 4; s++) bv[s] = __fmul_rn(bv[s], bv[s]);
            }
            f32x4 av[4];
#pragma unroll
            for (int a = 0; a < 4; a++) av[a] = *(const f32x4 *)(Cs + (16 * a + l15) * S + h * half + 16 * g + 4 * kg);
#pragma unroll
            for (int s = 0; s < 4; s++)
#pragma unroll
                for (int a = 0; a < 4; a++) acc[a] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[a][s], bv[s], acc[a], 0, 0, 0);
        }
}

// grid-stride over position tiles.  DB: two component buffers (dim <= 128)
template <int DP, bool DB>
__global__ __launch_bounds__(256) void gmm_estep_kernel(GmTable T, int n, const float *__restrict__ shift, GmComp K, float *__restrict__ lse,
                                                        int32_t *__restrict__ assign, float *__restrict__ max_resp, float *__restrict__ lj) {
#pragma clang fp contract(off)                                  // the log-sum-exp as written: its four lane groups end on the same bits
    extern __shared__ __align__(16) unsigned char smem[];
    constexpr int BUFS = DB ? 2 : 1;
    const int nch = T.nch, dpad = 16 * nch, half = dpad + 4, tile_floats = GM_T * 2 * half;
    float *Cs = (float *)smem;                                  // [BUFS][64][2 (dpad + 4)]
    float *Ks = Cs + BUFS * tile_floats;                        // [BUFS][64] cst, -inf past k
    float *Sh = Ks + BUFS * GM_T;                               // [dpad] the shift, zero past dim
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, kg = lane >> 4, l15 = lane & 15;
    const int k = K.k, n_tiles = (n + GM_T - 1) / GM_T, n_ct = (k + GM_T - 1) / GM_T;

    for (int j = threadIdx.x; j < dpad; j += 256) Sh[j] = j < T.dim ? shift[j] : 0.f;
    gm_comp_copy<DP>(K, T.dim, nch, 0, Cs, Ks);
    __syncthreads();
    int buf = 0, have = 0;                                      // the buffer that holds the tile of this step; the tile a single buffer holds

    for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int i = tile * GM_T + 16 * wave + l15;
        const int row = i < n ? gm_list_row(T, i) : -1;
        const float inv = row >= 0 && T.inv_norm ? T.inv_norm[row] : 1.f;
        f32x4 b[DP / 16];
#pragma unroll
        for (int g = 0; g < DP / 16; g++) {
            b[g] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (g < nch && row >= 0) {
                const int col = 16 * g + 4 * kg;
                const f32x4 v = gm_load4(T.data + (size_t)row * T.ld, col, T.dim, T.vec_ok);
#pragma unroll
                for (int s = 0; s < 4; s++) b[g][s] = gm_shifted(v[s], inv, Sh[col + s]);   // past dim: 0 . inv - 0
            }
        }
        float m = -INFINITY, sum = 0.f, best = -INFINITY;
        int best_c = 0;
        for (int ct = 0; ct < n_ct; ct++) {
            const bool more = n_ct > 1 && !(ct == n_ct - 1 && tile + (int)gridDim.x >= n_tiles);   // a step follows this one
            f32x4 stage[DB ? DP / 8 : 1];
            if constexpr (DB) {
                if (more) {                                     // in flight across the products below
#pragma unroll
                    for (int u = 0; u < DP / 8; u++) {
                        const int idx = threadIdx.x + 256 * u;
                        if (4 * (idx % (DP / 4)) < dpad) stage[u] = gm_comp_load<DP>(K, T.dim, (ct + 1) % n_ct, idx);
                    }
                }
            } else {
                if (have != ct) {
                    __syncthreads();                            // the products with the tile before this one are done
                    gm_comp_copy<DP>(K, T.dim, nch, ct, Cs, Ks);
                    __syncthreads();
                    have = ct;
                }
            }
            f32x4 acc[4];
            gm_products<DP>(Cs + buf * tile_floats, b, acc, nch, kg, l15);
            const float *Kc = Ks + buf * GM_T;
            float lv[16], tmax = -INFINITY;
#pragma unroll
            for (int a = 0; a < 4; a++)
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const int cc = 16 * a + 4 * kg + r, c = ct * GM_T + cc;
                    const float v = c < k ? __fmaf_rn(-0.5f, acc[a][r], Kc[cc]) : -INFINITY;
                    lv[4 * a + r] = v;
                    if (v > best) { best = v; best_c = c; }     // ascending c: the lowest on a tie
                    tmax = fmaxf(tmax, v);
                    if (lj && i < n && c < k) lj[(size_t)i * k + c] = row >= 0 ? v : NAN;
                }
            if (tmax > m) { sum *= expf(m - tmax); m = tmax; }
            if (m > -INFINITY) {
#pragma unroll
                for (int e = 0; e < 16; e++) sum += expf(lv[e] - m);
            }
            if constexpr (DB) {
                if (more) {
                    float *Cn = Cs + (buf ^ 1) * tile_floats;
#pragma unroll
                    for (int u = 0; u < DP / 8; u++) {
                        const int idx = threadIdx.x + 256 * u;
                        if (4 * (idx % (DP / 4)) < dpad) gm_comp_store<DP>(Cn, half, idx, stage[u]);
                    }
                    if (threadIdx.x < GM_T) {
                        const int c = ((ct + 1) % n_ct) * GM_T + (int)threadIdx.x;
                        Ks[(buf ^ 1) * GM_T + threadIdx.x] = c < k ? K.cst[c] : -INFINITY;
                    }
                    __syncthreads();                            // this step's tile is done with, the next is in place
                    buf ^= 1;
                }
            }
        }
#pragma unroll
        for (int off = 16; off < 64; off <<= 1) {               // the four lane groups of a row
            const float om = __shfl_xor(m, off, WAVE), os = __shfl_xor(sum, off, WAVE), ob = __shfl_xor(best, off, WAVE);
            const int oc = __shfl_xor(best_c, off, WAVE);
            const float M = fmaxf(m, om);
            const float mine = m > -INFINITY ? sum * expf(m - M) : 0.f, theirs = om > -INFINITY ? os * expf(om - M) : 0.f;
            sum = mine + theirs;
            m = M;
            if (ob > best || (ob == best && oc < best_c)) { best = ob; best_c = oc; }
        }
        if (kg == 0 && i < n) {
            const float l = m + logf(sum);
            lse[i] = row >= 0 ? l : NAN;
            assign[i] = row >= 0 ? best_c : -1;
            max_resp[i] = row >= 0 ? expf(best - l) : NAN;
        }
    }
}

// block = part: the part's float64 sum of lse over its points
__global__ __launch_bounds__(256) void gmm_lsepart_kernel(const float *__restrict__ lse, int n, double *__restrict__ partials) {
    __shared__ double red[256];
    const int t = threadIdx.x;
    double s = 0.0;
    for (int b = 0; b < GM_PART / 256; b++) {
        const int i = blockIdx.x * GM_PART + b * 256 + t;
        const float v = i < n ? lse[i] : NAN;
        if (v == v) s += (double)v;
    }
    red[t] = s;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (t < w) red[t] += red[t + w];
        __syncthreads();
    }
    if (t == 0) partials[blockIdx.x] = red[0];
}
__global__ __launch_bounds__(256) void gmm_lsefinal_kernel(const double *__restrict__ partials, int parts, double *__restrict__ out) {
    __shared__ double red[256];
    const int t = threadIdx.x;
    double s = 0.0;
    for (int p = t; p < parts; p += 256) s += partials[p];
    red[t] = s;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (t < w) red[t] += red[t + w];
        __syncthreads();
    }
    if (t == 0) *out = red[0];
}

// ---- M-step -------------------------------------------------------------------------------------------------------------------

// grid (parts of the batch, blocks of 16 components).  partials [part of the batch][component block][slab][reg . 64 + lane].
// lj is indexed from position pos0; lse and assign from position 0.
template <int NSL>
__global__ __launch_bounds__(256) void gmm_mstep_kernel(GmTable T, int n, const float *__restrict__ shift, const float *__restrict__ lj,
                                                        const float *__restrict__ lse, const int32_t *__restrict__ assign, int k, int pos0,
                                                        int part0, double *__restrict__ partials) {
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), kg = lane >> 4, l15 = lane & 15;
    const int W = 1 + 2 * T.dim, n_slab = (W + 15) / 16;
    const int part = part0 + blockIdx.x, first = part * GM_PART, left_all = min(GM_PART, n - first);
    const int c = 16 * blockIdx.y + l15;
    int col[NSL], kind[NSL];                                    // by slot: the table column, and 0 nothing, 1 one, 2 x', 3 x'^2
    float sh[NSL];
    f64x4 acc[NSL];
#pragma unroll
    for (int s = 0; s < NSL; s++) {
        const int e = 16 * (wave + 4 * s) + l15;
        kind[s] = e == 0 ? 1 : e <= T.dim ? 2 : e < W ? 3 : 0;
        col[s] = kind[s] == 2 ? e - 1 : kind[s] == 3 ? e - 1 - T.dim : 0;
        sh[s] = kind[s] >= 2 ? shift[col[s]] : 0.f;
        acc[s] = f64x4{0.0, 0.0, 0.0, 0.0};
    }
    for (int p0 = 0; p0 < left_all; p0 += WAVE) {
        const int i_mine = first + p0 + lane;
        const int r_mine = p0 + lane < left_all ? gm_list_row(T, i_mine) : -1;
        const float f_mine = r_mine >= 0 && T.inv_norm ? T.inv_norm[r_mine] : 1.f;
        const float l_mine = r_mine >= 0 && lj ? lse[i_mine] : 0.f;
        const int a_mine = r_mine >= 0 && !lj ? assign[i_mine] : -1;
        const int steps = min(WAVE, left_all - p0 + 3) / 4;
#pragma unroll 4
        for (int step = 0; step < steps; step++) {
            const int src = 4 * step + kg;
            const int r = __shfl(r_mine, src, WAVE);
            const float f = __shfl(f_mine, src, WAVE), l = __shfl(l_mine, src, WAVE);
            const int as = __shfl(a_mine, src, WAVE);
            double a = 0.0;
            if (r >= 0 && c < k) a = lj ? (double)expf(lj[(size_t)(first + p0 + src - pos0) * k + c] - l) : (as == c ? 1.0 : 0.0);
#pragma unroll
            for (int s = 0; s < NSL; s++) {
                if (wave + 4 * s < n_slab) {                    // the same for every lane of the wave
                    double bv = 0.0;
                    if (r >= 0 && kind[s] == 1) bv = 1.0;
                    if (r >= 0 && kind[s] >= 2) {
                        const double x = (double)gm_shifted(T.data[(size_t)r * T.ld + col[s]], f, sh[s]);
                        bv = kind[s] == 2 ? x : x * x;
                    }
                    acc[s] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, bv, acc[s], 0, 0, 0);
                }
            }
        }
    }
#pragma unroll
    for (int s = 0; s < NSL; s++) {
        const int slab = wave + 4 * s;
        if (slab < n_slab) {
            double *out = partials + (((size_t)blockIdx.x * gridDim.y + blockIdx.y) * n_slab + slab) * 256;
#pragma unroll
            for (int r = 0; r < 4; r++) out[r * 64 + lane] = acc[s][r];   // D[component kg + 4 r][column l15]: the f64 map
        }
    }
}

// grid (component blocks, slabs), thread = element of the tile: the batch's partials in part order onto the running sum
__global__ __launch_bounds__(256) void gmm_fold_kernel(const double *__restrict__ partials, int parts, int k, int W, int from_zero,
                                                       double *__restrict__ sums) {
    const int e = threadIdx.x, lane = e & 63, reg = e >> 6;
    const int a = 16 * blockIdx.x + (lane >> 4) + 4 * reg, b = 16 * blockIdx.y + (lane & 15);
    if (a >= k || b >= W) return;
    const size_t stride = (size_t)gridDim.x * gridDim.y * 256, at = ((size_t)blockIdx.x * gridDim.y + blockIdx.y) * 256 + e;
    double s = from_zero ? 0.0 : sums[(size_t)a * W + b];
    for (int p0 = 0; p0 < parts; p0 += GM_FOLD) {               // GM_FOLD loads in flight, then their additions in order
        double v[GM_FOLD];
#pragma unroll
        for (int u = 0; u < GM_FOLD; u++) v[u] = p0 + u < parts ? partials[(size_t)(p0 + u) * stride + at] : 0.0;
#pragma unroll
        for (int u = 0; u < GM_FOLD; u++)
            if (p0 + u < parts) s += v[u];
    }
    sums[(size_t)a * W + b] = s;
}

// ---- finalize -----------------------------------------------------------------------------------------------------------------

// block = component, thread = column
__global__ __launch_bounds__(256) void gmm_finalize_kernel(const double *__restrict__ sums, int n, int k, int dim, int spherical, double reg_covar,
                                                           float *__restrict__ mu, float *__restrict__ var, float *__restrict__ weights,
                                                           float *__restrict__ prec, float *__restrict__ mprec, int ldc, float *__restrict__ cst) {
    __shared__ double red[GM_MAX_DIM];
    const int c = blockIdx.x, t = threadIdx.x, W = 1 + 2 * dim;
    const size_t at = (size_t)c * ldc + t;
    double m = 0.0, v = 1.0, w = 0.0;
    if (sums) {
        double total = 0.0;
        for (int cc = 0; cc < k; cc++) total += sums[(size_t)cc * W];
        const double N = sums[(size_t)c * W];
        if (!(N >= 10.0 * 0x1p-52 * (double)n)) {               // not fitted: mu', var and the operands stay
            if (t == 0) { weights[c] = 0.f; cst[c] = -INFINITY; }
            return;
        }
        w = N / total;
        if (t < dim) {
            m = sums[(size_t)c * W + 1 + t] / N;
            v = fmax(sums[(size_t)c * W + 1 + dim + t] / N - m * m, 0.0) + reg_covar;
        }
        if (spherical) {
            red[t] = v;
            __syncthreads();
            double s = 0.0;
            for (int j = 0; j < dim; j++) s += red[j];
            v = s / (double)dim;
            __syncthreads();
        }
        if (t < dim) { mu[at] = (float)m; var[at] = (float)v; }
        if (t == 0) weights[c] = (float)w;
    } else {
        w = (double)weights[c];
        if (t < dim) { m = (double)mu[at]; v = (double)var[at]; }
    }
    if (t < dim) { prec[at] = (float)(1.0 / v); mprec[at] = (float)(m / v); }
    red[t] = t < dim ? m * m / v + log(v) : 0.0;
    __syncthreads();
    if (t == 0) {
        double s = 0.0;
        for (int j = 0; j < dim; j++) s += red[j];
        cst[c] = (float)(log(w) - 0.5 * (s + (double)dim * 1.8378770664093453));   // log 2 pi
    }
}

// ---- entry points ------------------------------------------------------------------------------------------------------------

static int gm_refuse(const char *name, const char *why) {
    static thread_local char msg[200];
    snprintf(msg, sizeof msg, "%s: %s", name, why);
    return gcnhip_fail(msg);
}
static const char *gm_common(const gcnhip_ctx *c, const void *table, int ld, int n_table, int dim, const int32_t *d_rows, int n, int k) {
    if (!c || !table || n_table < 0 || n < 0) return "invalid argument";
    if (dim < 1 || dim > GM_MAX_DIM) return "1 <= dim <= 256";
    if (ld < dim) return "the row stride is below dim";
    if (k < 1 || k > GM_MAX_K) return "1 <= k <= 256";
    if (!d_rows && n > n_table) return "without a row list n is at most n_table";
    return nullptr;
}
static GmTable gm_table(const float *table, int ld, int n_table, int dim, const float *inv_norm, const int32_t *d_rows) {
    return GmTable{table, ld, n_table, dim, inv_norm, d_rows, ld % 4 == 0 && aligned16(table) ? 1 : 0, (dim + 15) / 16};
}
static size_t gm_up256(size_t b) { return (b + 255) / 256 * 256; }
static size_t gm_part_bytes(int k, int dim) { return (size_t)ceil_div(k, 16) * ceil_div(1 + 2 * dim, 16) * 256 * sizeof(double); }

template <int DP, bool DB>
static int gm_estep_launch(gcnhip_ctx *c, const GmTable &T, int n, const float *shift, const GmComp &K, float *lse, int32_t *assign, float *max_resp,
                           float *lj) {
    const int dpad = 16 * T.nch;
    const size_t lds = sizeof(float) * ((size_t)(DB ? 2 : 1) * (GM_T * 2 * (dpad + 4) + GM_T) + dpad);
    auto kern = gmm_estep_kernel<DP, DB>;
    if (lds > 64 * 1024) GCNHIP_TRY(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    const int blocks = std::min(ceil_div(n, GM_T), c->n_cu > 0 ? c->n_cu : 128);
    kern<<<blocks, 256, lds, c->stream>>>(T, n, shift, K, lse, assign, max_resp, lj);
    GCNHIP_LAUNCH_CHECK();
    return 0;
}

extern "C" {

int gcnhip_gmm_plan(int n, int k, int dim, size_t *estep_bytes, size_t *mstep_bytes, size_t *mstep_bytes_min) {
    if (n < 0 || dim < 1 || dim > GM_MAX_DIM) return gm_refuse("gcnhip_gmm_plan", "invalid argument (n >= 0, 1 <= dim <= 256)");
    if (k < 1 || k > GM_MAX_K) return gm_refuse("gcnhip_gmm_plan", "1 <= k <= 256");
    const size_t parts = (size_t)std::max(ceil_div(n, GM_PART), 1);
    if (estep_bytes) *estep_bytes = gm_up256(parts * sizeof(double));
    if (mstep_bytes) *mstep_bytes = parts * gm_part_bytes(k, dim);
    if (mstep_bytes_min) *mstep_bytes_min = gm_part_bytes(k, dim);
    return 0;
}

int gcnhip_gmm_estep(gcnhip_ctx *c, const float *table, int ld, int n_table, int dim, const float *inv_norm, const int32_t *d_rows, int n,
                     const float *shift, const float *prec, const float *mprec, int ldc, const float *cst, int k, float *lse, int32_t *assign,
                     float *max_resp, float *lj, double *lse_sum, void *scratch, size_t scratch_bytes) {
    const char *name = "gcnhip_gmm_estep";
    if (const char *why = gm_common(c, table, ld, n_table, dim, d_rows, n, k)) return gm_refuse(name, why);
    if (!shift || !prec || !mprec || !cst || (n > 0 && (!lse || !assign || !max_resp))) return gm_refuse(name, "invalid argument (a NULL operand or output)");
    if (ldc < dim) return gm_refuse(name, "the row stride of the operands is below dim");
    size_t need = 0;
    if (gcnhip_gmm_plan(n, k, dim, &need, nullptr, nullptr) != 0) return -1;
    if (lse_sum && (!scratch || scratch_bytes < need || !aligned16(scratch)))
        return gm_refuse(name, "the scratch of the sum is missing, unaligned or below what gcnhip_gmm_plan tells");
    const int parts = std::max(ceil_div(n, GM_PART), 1);
    if (n > 0) {
        const GmTable T = gm_table(table, ld, n_table, dim, inv_norm, d_rows);
        const GmComp K{prec, mprec, cst, ldc, k, ldc % 4 == 0 && aligned16(prec) && aligned16(mprec) ? 1 : 0};
        const int rc = dim <= 128 ? gm_estep_launch<128, true>(c, T, n, shift, K, lse, assign, max_resp, lj)
                                  : gm_estep_launch<256, false>(c, T, n, shift, K, lse, assign, max_resp, lj);
        if (rc != 0) return rc;
    }
    if (lse_sum) {
        gmm_lsepart_kernel<<<parts, 256, 0, c->stream>>>(lse, n, (double *)scratch);
        GCNHIP_LAUNCH_CHECK();
        gmm_lsefinal_kernel<<<1, 256, 0, c->stream>>>((const double *)scratch, parts, lse_sum);
        GCNHIP_LAUNCH_CHECK();
    }
    return 0;
}

int gcnhip_gmm_mstep(gcnhip_ctx *c, const float *table, int ld, int n_table, int dim, const float *inv_norm, const int32_t *d_rows, int n,
                     const float *shift, const float *lj, const float *lse, const int32_t *assign, int k, int pos0, int pos1, double *sums,
                     void *scratch, size_t scratch_bytes) {
    const char *name = "gcnhip_gmm_mstep";
    if (const char *why = gm_common(c, table, ld, n_table, dim, d_rows, n, k)) return gm_refuse(name, why);
    if (!shift || !sums || !scratch) return gm_refuse(name, "invalid argument (a NULL operand, output or scratch)");
    if (lj ? !lse : !assign) return gm_refuse(name, "lj needs lse beside it; without lj the indicator needs assign");
    if (pos0 < 0 || pos1 < pos0 || pos1 > n || pos0 % GM_PART != 0 || (pos1 % GM_PART != 0 && pos1 != n))
        return gm_refuse(name, "positions [pos0, pos1) must lie in the list and start and end on parts of 1024 (or at the end)");
    if (!aligned16(scratch)) return gm_refuse(name, "the scratch is not 16-byte aligned");
    const size_t per_part = gm_part_bytes(k, dim);
    if (scratch_bytes < per_part) return gm_refuse(name, "the scratch is below the minimum (gcnhip_gmm_plan tells the bytes)");
    const GmTable T = gm_table(table, ld, n_table, dim, inv_norm, d_rows);
    const int W = 1 + 2 * dim, kb = ceil_div(k, 16), n_slab = ceil_div(W, 16);
    const int p_first = pos0 / GM_PART, p_end = std::max(ceil_div(pos1, GM_PART), p_first);
    const int batch = (int)std::min<size_t>(scratch_bytes / per_part, 65535);
    if (p_first == p_end && pos0 == 0) {                        // no positions: the sums are zeros
        gmm_fold_kernel<<<dim3(kb, n_slab), 256, 0, c->stream>>>((const double *)scratch, 0, k, W, 1, sums);
        GCNHIP_LAUNCH_CHECK();
    }
    for (int q0 = p_first; q0 < p_end; q0 += batch) {
        const int q1 = std::min(p_end, q0 + batch);
        if (n_slab <= 20)
            gmm_mstep_kernel<5><<<dim3(q1 - q0, kb), 256, 0, c->stream>>>(T, pos1, shift, lj, lse, assign, k, pos0, q0, (double *)scratch);
        else
            gmm_mstep_kernel<9><<<dim3(q1 - q0, kb), 256, 0, c->stream>>>(T, pos1, shift, lj, lse, assign, k, pos0, q0, (double *)scratch);
        GCNHIP_LAUNCH_CHECK();
        gmm_fold_kernel<<<dim3(kb, n_slab), 256, 0, c->stream>>>((const double *)scratch, q1 - q0, k, W, q0 == 0 ? 1 : 0, sums);
        GCNHIP_LAUNCH_CHECK();
    }
    return 0;
}

int gcnhip_gmm_finalize(gcnhip_ctx *c, const double *sums, int n, int k, int dim, int spherical, double reg_covar, float *mu, float *var,
                        float *weights, float *prec, float *mprec, int ldc, float *cst) {
    const char *name = "gcnhip_gmm_finalize";
    if (!c || !mu || !var || !weights || !prec || !mprec || !cst || n < 0) return gm_refuse(name, "invalid argument");
    if (dim < 1 || dim > GM_MAX_DIM) return gm_refuse(name, "1 <= dim <= 256");
    if (k < 1 || k > GM_MAX_K) return gm_refuse(name, "1 <= k <= 256");
    if (ldc < dim) return gm_refuse(name, "the row stride of the operands is below dim");
    if (sums && (!(reg_covar > 0.0) || !std::isfinite(reg_covar))) return gm_refuse(name, "reg_covar must be finite and above 0");
    gmm_finalize_kernel<<<k, 256, 0, c->stream>>>(sums, n, k, dim, spherical, reg_covar, mu, var, weights, prec, mprec, ldc, cst);
    GCNHIP_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
