// tsne.hip — exact t-SNE of a table's rows (van der Maaten & Hinton, 2008; scikit-learn's TSNE(method="exact") rules), matrix-free:
// P is never stored, every iteration recomputes each high-dimensional distance on the MFMA and turns it into p_ij in registers.
// Beyond the reference, which never looks at its hidden matrix.  include/gcnhip_driver.h has the definitions.
//
// The table contract is silhouette.hip's (f32 [n_table x ld], 1 <= dim <= 256, d_rows or NULL, inv_norm or NULL; two positions that
// name one row are two points; a position without a row is no point).  No float atomics, no allocation, no synchronisation; every
// output's bits are a function of the arguments' contents alone.
//
// gcnhip_tsne_pack        gathers the listed rows once into the PACK: {header | X [n_pad x DP] | S [n_pad] | valid [n_pad]}, n_pad =
//   n rounded up to 64, DP = dim rounded up to 16, 32, 64, 128 or 256 (zero padded: a zero column adds +0 to a dot), S = {xn, beta,
//   m, 1 / Z} in f32.  xn has the bits sil_stage gives it.  The gradient launches read aligned tiles of it.
// tsne_walk_kernel        ONE body for the two n x n x dim walks.  Grid (row tiles of 64 positions, column parts of 2048 positions),
//   four waves, wave w owns rows 16w .. 16w + 15.  The x^ of the workgroup's rows live in REGISTERS (DP / 4 VGPRs per lane: the B
//   operand of lane (l15, kg) of v_mfma_f32_16x16x4_f32), so LDS holds TWO column tiles of 64 x (DP + 4) floats with their scalars;
//   the global loads of tile t + 1 are issued into registers before the products and exponentials of tile t and stored to the other
//   buffer behind them: one barrier per tile.  The dot is silhouette's f32 fma chain in column order.
//     SLAB      d2(i, j) of a batch of rows to scratch, +inf at the self pair and at a column that is no point.
//     GRADIENT  per entry d2, two f32 exponentials, p, w, then float64 accumulators of p w (y_i - y_j), w^2 (y_i - y_j), w and with
//               want_kl of p ln(p / w) and p.  A lane adds in ascending column, tile after tile through the part; the four lane
//               groups of a row combine as (g0 + g1) + (g2 + g3): one partial per (row, part).
// tsne_search_kernel      a wave per row over its slab row: lanes strided over the columns, a fixed shuffle tree, float64.
// tsne_fold_kernel        a row's part partials in part order.  tsne_step_kernel: one workgroup, thread t of 256 adds positions t,
//   t + 256, .. and then a fixed tree (Zq, KL, the gradient norm), and applies the update rule.
#include "bucket.h"
#include "tsne_pack.h"
#include <algorithm>
#include <cmath>
#include <cstdio>

using f32x4 = __attribute__((ext_vector_type(4))) float;

constexpr int TS_CT = 64;                         // positions per column tile
constexpr int TS_PART = 2048;                     // positions per column part (part of the definition of the sums' order)
constexpr int TS_NACC = 9;                        // {p w dy [3] | w^2 dy [3] | w | p ln(p / w) | p}
enum { TS_SLAB = 0, TS_GRAD = 1 };

// a wave per position of the padded list: x^ zero-padded to dp, xn by sil_stage's order (columns lane, lane + 64, .., then the tree)
__global__ __launch_bounds__(256) void tsne_pack_kernel(const float *__restrict__ table, int ld, int n_table, int dim, int dp,
                                                        const float *__restrict__ inv_norm, const int32_t *__restrict__ d_rows, int n, int n_pad,
                                                        float *__restrict__ X, float4 *__restrict__ S, int32_t *__restrict__ valid) {
    const int lane = threadIdx.x & 63, i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= n_pad) return;
    const int r = i < n ? list_row(d_rows, i, n_table) : -1;
    const float f = r >= 0 && inv_norm ? inv_norm[r] : 1.f;
    float s = 0.f;
#pragma unroll
    for (int u = 0; u < 4; u++) {
        const int col = lane + WAVE * u;
        const float v = r >= 0 && col < dim ? table[(size_t)r * ld + col] : 0.f;
        if (col < dp) X[(size_t)i * dp + col] = __fmul_rn(v, f);
        s += v * v;
    }
    s = wave_sum(s);
    if (lane == 0) {
        S[i] = make_float4((s * f) * f, 0.f, 0.f, 0.f);
        valid[i] = r >= 0;
    }
}

// one workgroup: the points, and the unconverged counter's zero
__global__ __launch_bounds__(256) void tsne_count_kernel(const int32_t *__restrict__ valid, int n, int32_t *__restrict__ hdr, int32_t *__restrict__ n_points) {
    __shared__ int red[256];
    const int t = threadIdx.x;
    int c = 0;
    for (int i = t; i < n; i += 256) c += valid[i];
    red[t] = c;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (t < w) red[t] += red[t + w];
        __syncthreads();
    }
    if (t == 0) {
        hdr[0] = red[0];
        if (n_points) *n_points = red[0];
    }
}

template <int DP>
struct TsTile {                                                 // what a thread holds of a column tile between its loads and its LDS stores
    f32x4 x[DP / 16];
    float4 s;
    float y[4];
};

template <int DP, int K>
__device__ __forceinline__ void ts_tile_load(TsTile<DP> &T, const float *__restrict__ X, const float4 *__restrict__ S, const int32_t *__restrict__ valid,
                                             const float *__restrict__ y, int n, int c0) {
    const f32x4 *src = (const f32x4 *)(X + (size_t)c0 * DP);    // the tile is 64 . DP contiguous floats
#pragma unroll
    for (int u = 0; u < DP / 16; u++) T.x[u] = src[threadIdx.x + 256 * u];
    if (threadIdx.x < TS_CT) {
        const int col = c0 + threadIdx.x;
        T.s = S[col];
        const bool ok = valid[col] != 0;                        // col < n_pad; a padding position is no point
        T.y[3] = ok ? 1.f : 0.f;
#pragma unroll
        for (int c = 0; c < 3; c++) T.y[c] = c < K && y && ok && col < n ? y[(size_t)col * K + c] : 0.f;
    }
}

template <int DP>
__device__ __forceinline__ void ts_tile_store(const TsTile<DP> &T, float *__restrict__ Cs, float4 *__restrict__ Ss, float4 *__restrict__ Ys) {
    constexpr int QLD = DP + 4;
#pragma unroll
    for (int u = 0; u < DP / 16; u++) {
        const int idx = threadIdx.x + 256 * u, row = idx / (DP / 4), c4 = idx % (DP / 4);
        *(f32x4 *)(Cs + row * QLD + 4 * c4) = T.x[u];
    }
    if (threadIdx.x < TS_CT) {
        Ss[threadIdx.x] = T.s;
        Ys[threadIdx.x] = make_float4(T.y[0], T.y[1], T.y[2], T.y[3]);
    }
}

// grid (row tiles of the batch, column parts).  SLAB: slab [batch rows x n_pad].  GRADIENT: partials [part][batch_rows][TS_NACC].
template <int DP, int K, int MODE>
__global__ __launch_bounds__(256) void tsne_walk_kernel(const int32_t *__restrict__ hdr, const float *__restrict__ X, const float4 *__restrict__ S,
                                                        const int32_t *__restrict__ valid, const float *__restrict__ y, int n, int n_pad, int row0,
                                                        int batch_rows, int want_kl, float *__restrict__ slab, double *__restrict__ partials) {
    extern __shared__ __align__(16) unsigned char smem[];
    constexpr int QLD = DP + 4, NCH = DP / 16;
    float *Cs = (float *)smem;                                  // [2][64][QLD]
    float4 *Ss = (float4 *)(Cs + 2 * TS_CT * QLD);              // [2][64] {xn, beta, m, 1 / Z}
    float4 *Ys = Ss + 2 * TS_CT;                                // [2][64] {y0, y1, y2, 1 for a point}
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int kg = lane >> 4, l15 = lane & 15;
    const int i_local = blockIdx.x * TS_RT + 16 * wave + l15, i = row0 + i_local;     // i < n_pad: batches are whole row tiles
    const int c_lo = blockIdx.y * TS_PART, c_hi = min(c_lo + TS_PART, n_pad);
    const int n_tiles = (c_hi - c_lo) / TS_CT;

    f32x4 b[NCH];                                               // the row operand: x^_i[16c + 4kg .. + 3]
#pragma unroll
    for (int c = 0; c < NCH; c++) b[c] = *(const f32x4 *)(X + (size_t)i * DP + 16 * c + 4 * kg);
    const float4 si = S[i];
    const bool vi = valid[i] != 0;
    float yi[K];
#pragma unroll
    for (int c = 0; c < K; c++) yi[c] = MODE == TS_GRAD && vi && i < n ? y[(size_t)i * K + c] : 0.f;
    const float inv2n = MODE == TS_GRAD ? (float)(1.0 / (2.0 * (double)hdr[0])) : 0.f;
    const float pi_scale = si.w * inv2n;                        // (e_i(j) / Z_i) / (2 n): one product less per entry
    double acc_a[K] = {}, acc_r[K] = {}, acc_w = 0.0, acc_kl = 0.0, acc_p = 0.0;

    TsTile<DP> T;
    ts_tile_load<DP, K>(T, X, S, valid, y, n, c_lo);
    ts_tile_store<DP>(T, Cs, Ss, Ys);
    __syncthreads();
    for (int t = 0; t < n_tiles; t++) {
        const int buf = t & 1, c0 = c_lo + t * TS_CT;
        if (t + 1 < n_tiles) ts_tile_load<DP, K>(T, X, S, valid, y, n, c0 + TS_CT);      // in flight across the products below
        const float *C = Cs + buf * TS_CT * QLD;
        const float4 *Sc = Ss + buf * TS_CT, *Yc = Ys + buf * TS_CT;
        f32x4 acc[4] = {};
#pragma unroll
        for (int c = 0; c < NCH; c++) {
            f32x4 a[4];
#pragma unroll
            for (int g = 0; g < 4; g++) a[g] = *(const f32x4 *)(C + (16 * g + l15) * QLD + 16 * c + 4 * kg);
#pragma unroll
            for (int s = 0; s < 4; s++)
#pragma unroll
                for (int g = 0; g < 4; g++) acc[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[g][s], b[c][s], acc[g], 0, 0, 0);
        }
#pragma unroll
        for (int g = 0; g < 4; g++)
#pragma unroll
            for (int r = 0; r < 4; r++) {                       // D[row 4kg + r][col l15]: column 16g + 4kg + r of the tile, this lane's row
                const int cc = 16 * g + 4 * kg + r, j = c0 + cc;
                const float4 sj = Sc[cc], yj = Yc[cc];
                const bool ok = yj.w != 0.f && j != i;          // a point, and not the self pair BY POSITION
                const float d2 = fmaxf((si.x + sj.x) - 2.f * acc[g][r], 0.f);
                if (MODE == TS_SLAB) {
                    slab[(size_t)i_local * n_pad + j] = ok ? d2 : INFINITY;
                } else {
                    const float ei = expf(-si.y * (d2 - si.z)), ej = expf(-sj.y * (d2 - sj.z));
                    const float p = ok ? ei * pi_scale + ej * (sj.w * inv2n) : 0.f;
                    float dy[K], dist = 0.f;
#pragma unroll
                    for (int c = 0; c < K; c++) {
                        dy[c] = yi[c] - (c == 0 ? yj.x : c == 1 ? yj.y : yj.z);
                        dist = fmaf(dy[c], dy[c], dist);
                    }
                    const float w = ok ? __builtin_amdgcn_rcpf(1.f + dist) : 0.f;
                    const float pw = p * w, ww = w * w;
#pragma unroll
                    for (int c = 0; c < K; c++) {
                        acc_a[c] = fma((double)pw, (double)dy[c], acc_a[c]);
                        acc_r[c] = fma((double)ww, (double)dy[c], acc_r[c]);
                    }
                    acc_w += (double)w;
                    if (want_kl && p > 0.f) {                   // a logarithm per pair: only where the caller asks
                        acc_kl = fma((double)p, log((double)p / (double)w), acc_kl);
                        acc_p += (double)p;
                    }
                }
            }
        if (t + 1 < n_tiles) ts_tile_store<DP>(T, Cs + (buf ^ 1) * TS_CT * QLD, Ss + (buf ^ 1) * TS_CT, Ys + (buf ^ 1) * TS_CT);
        __syncthreads();                                        // tile t is done with, tile t + 1 is in place
    }
    if (MODE == TS_GRAD) {
        double out[TS_NACC] = {};
#pragma unroll
        for (int c = 0; c < K; c++) { out[c] = acc_a[c]; out[3 + c] = acc_r[c]; }
        out[6] = acc_w; out[7] = acc_kl; out[8] = acc_p;
#pragma unroll
        for (int a = 0; a < TS_NACC; a++) {
            out[a] += __shfl_xor(out[a], 16, WAVE);             // (g0 + g1), (g2 + g3)
            out[a] += __shfl_xor(out[a], 32, WAVE);             // their sum
        }
        if (kg == 0) {
            double *dst = partials + ((size_t)blockIdx.y * batch_rows + i_local) * TS_NACC;
#pragma unroll
            for (int a = 0; a < TS_NACC; a++) dst[a] = out[a];
        }
    }
}

__device__ inline double ts_tree(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, WAVE);
    return v;
}

// a wave per row of the batch: m, then scikit-learn's search for beta in float64 on the f32 d2 of the slab row
__global__ __launch_bounds__(256) void tsne_search_kernel(const float *__restrict__ slab, int n, int n_pad, int row0, int rows_here,
                                                          const int32_t *__restrict__ valid, double target, float4 *__restrict__ S,
                                                          double *__restrict__ beta, float *__restrict__ m_out, double *__restrict__ inv_z,
                                                          int32_t *__restrict__ unconverged) {
    const int lane = threadIdx.x & 63, i_local = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i_local >= rows_here) return;
    const int i = row0 + i_local;
    if (!valid[i]) {
        if (lane == 0) { beta[i] = NAN; m_out[i] = NAN; inv_z[i] = NAN; }
        return;
    }
    const float *row = slab + (size_t)i_local * n_pad;
    float mn = INFINITY;
    for (int j = lane; j < n; j += WAVE) mn = fminf(mn, row[j]);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) mn = fminf(mn, __shfl_xor(mn, off, WAVE));
    double bt = 1.0, lo = -INFINITY, hi = INFINITY, z = 1.0;
    bool conv = false;
    for (int step = 0; step < 100; step++) {
        double zs = 0.0, ds = 0.0;
        for (int j = lane; j < n; j += WAVE) {
            const float d = row[j];
            if (d < INFINITY) {
                const double dd = (double)d - (double)mn;
                const double e = exp(-bt * dd);
                zs += e;
                ds = fma(dd, e, ds);
            }
        }
        z = ts_tree(zs);
        ds = ts_tree(ds);
        const double diff = (log(z) + bt * ds / z) - target;
        if (fabs(diff) <= 1e-5) { conv = true; break; }
        if (step == 99) break;                                  // the last beta that was evaluated stays, with its Z
        if (diff > 0.0) { lo = bt; bt = hi == INFINITY ? bt * 2.0 : (bt + hi) * 0.5; }
        else { hi = bt; bt = lo == -INFINITY ? bt * 0.5 : (bt + lo) * 0.5; }
    }
    if (lane == 0) {
        const double iz = 1.0 / z;
        beta[i] = bt;
        m_out[i] = mn;
        inv_z[i] = iz;
        const float xn = S[i].x;
        S[i] = make_float4(xn, (float)bt, mn, (float)iz);
        if (!conv) atomicAdd(unconverged, 1);                   // an integer count
    }
}

__global__ void tsne_zero_kernel(int32_t *p) { *p = 0; }

// rowsums[i][a] = the partials of row i in part order
__global__ __launch_bounds__(256) void tsne_fold_kernel(const double *__restrict__ partials, int n_parts, int row0, int rows_here, int batch_rows,
                                                        double *__restrict__ rowsums) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= rows_here * TS_NACC) return;
    const int i_local = e / TS_NACC, a = e % TS_NACC;
    double s = 0.0;
    for (int p = 0; p < n_parts; p++) s += partials[((size_t)p * batch_rows + i_local) * TS_NACC + a];
    rowsums[(size_t)(row0 + i_local) * TS_NACC + a] = s;
}

__device__ inline double ts_block_sum(double v, double *red) {
    const int t = threadIdx.x;
    __syncthreads();
    red[t] = v;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (t < w) red[t] += red[t + w];
        __syncthreads();
    }
    return red[0];
}

// one workgroup: Zq, KL, the gradient, its norm, and with `apply` scikit-learn's update of {y | update | gain} and the f32 copy of y
template <int K>
__global__ __launch_bounds__(256) void tsne_step_kernel(const double *__restrict__ rowsums, const int32_t *__restrict__ valid, int n, double exaggeration,
                                                        double momentum, double lr, int apply, double *__restrict__ state, float *__restrict__ y32,
                                                        double *__restrict__ grad, double *__restrict__ stats) {
    __shared__ double red[256];
    const int t = threadIdx.x;
    double zq = 0.0, ka = 0.0, kb = 0.0;
    for (int i = t; i < n; i += 256)
        if (valid[i]) {
            const double *r = rowsums + (size_t)i * TS_NACC;
            zq += r[6]; ka += r[7]; kb += r[8];
        }
    zq = ts_block_sum(zq, red);
    ka = ts_block_sum(ka, red);
    kb = ts_block_sum(kb, red);
    double *yy = state, *up = state + (size_t)n * K, *gain = state + 2 * (size_t)n * K;
    double gsq = 0.0;
    for (int i = t; i < n; i += 256) {
        const double *r = rowsums + (size_t)i * TS_NACC;
        const bool ok = valid[i] != 0;
#pragma unroll
        for (int c = 0; c < K; c++) {
            const size_t e = (size_t)i * K + c;
            const double g = ok ? 4.0 * (exaggeration * r[c] - r[3 + c] / zq) : NAN;
            if (ok) gsq = fma(g, g, gsq);
            if (grad) grad[e] = g;
            if (apply) {
                if (ok) {
                    const double u0 = up[e];
                    double gn = u0 * g < 0.0 ? gain[e] + 0.2 : gain[e] * 0.8;
                    gn = fmax(gn, 0.01);
                    const double u = momentum * u0 - lr * (gn * g);
                    const double v = yy[e] + u;
                    gain[e] = gn; up[e] = u; yy[e] = v;
                    y32[e] = (float)v;
                } else {
                    yy[e] = NAN;
                    y32[e] = NAN;
                }
            }
        }
    }
    gsq = ts_block_sum(gsq, red);
    if (t == 0 && stats) {
        stats[0] = ka + log(zq) * kb;                           // KL = sum p ln(p Zq / w)
        stats[1] = sqrt(gsq);
        stats[2] = zq;
    }
}

// ---- entry points ------------------------------------------------------------------------------------------------------------

template <int DP, int K, int MODE>
static int ts_walk_launch(gcnhip_ctx *c, const TsPack &P, const float *y, int n, int n_pad, int row0, int batch_rows, int tiles, int want_kl, float *slab,
                          double *partials) {
    const size_t lds = sizeof(float) * (size_t)(2 * TS_CT * (DP + 4)) + 4 * TS_CT * sizeof(float4);
    auto kern = tsne_walk_kernel<DP, K, MODE>;
    if (lds > 64 * 1024) GCNHIP_TRY(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    kern<<<dim3(tiles, ceil_div(n_pad, TS_PART)), 256, lds, c->stream>>>(P.hdr, P.X, P.S, P.valid, y, n, n_pad, row0, batch_rows, want_kl, slab, partials);
    GCNHIP_LAUNCH_CHECK();
    return 0;
}
template <int K, int MODE, typename... A>
static int ts_walk(int dp, A... a) {
    switch (dp) {
    case 16: return ts_walk_launch<16, K, MODE>(a...);
    case 32: return ts_walk_launch<32, K, MODE>(a...);
    case 64: return ts_walk_launch<64, K, MODE>(a...);
    case 128: return ts_walk_launch<128, K, MODE>(a...);
    default: return ts_walk_launch<256, K, MODE>(a...);
    }
}

static size_t ts_slab_bytes(int n, int rows) { return (size_t)rows * (size_t)ts_npad(n) * sizeof(float); }
static size_t ts_part_bytes(int n, int rows) { return (size_t)rows * (size_t)ceil_div(ts_npad(n), TS_PART) * TS_NACC * sizeof(double); }

extern "C" {

int gcnhip_tsne_plan(int n, int dim, size_t *pack_bytes, size_t *bytes, size_t *bytes_min) {
    if (n < 0 || dim < 1 || dim > TS_MAX_DIM) return gcnhip_fail("gcnhip_tsne_plan: invalid argument (n >= 0, 1 <= dim <= 256)");
    const int n_pad = ts_npad(n);
    if (pack_bytes) *pack_bytes = ts_pack(nullptr, n, dim).bytes;
    if (bytes) *bytes = std::max(ts_slab_bytes(n, n_pad), ts_part_bytes(n, n_pad));
    if (bytes_min) *bytes_min = std::max(ts_slab_bytes(n, TS_RT), ts_part_bytes(n, TS_RT));
    return 0;
}

int gcnhip_tsne_pack(gcnhip_ctx *c, const float *table, int ld, int n_table, int dim, const float *inv_norm, const int32_t *d_rows, int n, void *pack,
                     size_t pack_bytes, int32_t *n_points) {
    if (!c || !table || !pack || n_table < 0 || n < 0) return gcnhip_fail("gcnhip_tsne_pack: invalid argument");
    if (dim < 1 || dim > TS_MAX_DIM) return gcnhip_fail("gcnhip_tsne_pack: 1 <= dim <= 256");
    if (ld < dim) return gcnhip_fail("gcnhip_tsne_pack: the row stride is below dim");
    if (!d_rows && n > n_table) return gcnhip_fail("gcnhip_tsne_pack: without a row list n is at most n_table");
    if (!aligned16(pack)) return gcnhip_fail("gcnhip_tsne_pack: the pack is not 16-byte aligned");
    const TsPack P = ts_pack(pack, n, dim);
    if (pack_bytes < P.bytes) return gcnhip_fail("gcnhip_tsne_pack: the pack is too small (gcnhip_tsne_plan tells the bytes)");
    const int n_pad = ts_npad(n);
    tsne_pack_kernel<<<n_pad / 4, 256, 0, c->stream>>>(table, ld, n_table, dim, ts_dp(dim), inv_norm, d_rows, n, n_pad, P.X, P.S, P.valid);
    GCNHIP_LAUNCH_CHECK();
    tsne_count_kernel<<<1, 256, 0, c->stream>>>(P.valid, n, P.hdr, n_points);
    GCNHIP_LAUNCH_CHECK();
    return 0;
}

int gcnhip_tsne_bandwidths(gcnhip_ctx *c, void *pack, int n, int dim, int n_points, double perplexity, double *beta, float *m, double *inv_z,
                           int32_t *unconverged, void *scratch, size_t scratch_bytes) {
    if (!c || !pack || !beta || !m || !inv_z || !unconverged || !scratch || n < 1 || n_points > n)
        return gcnhip_fail("gcnhip_tsne_bandwidths: invalid argument");
    if (dim < 1 || dim > TS_MAX_DIM) return gcnhip_fail("gcnhip_tsne_bandwidths: 1 <= dim <= 256");
    if (!(perplexity >= 1.0) || !(perplexity < (double)n_points - 1.0))
        return gcnhip_fail("gcnhip_tsne_bandwidths: perplexity must be in [1, n_points - 1)");
    if (!aligned16(scratch)) return gcnhip_fail("gcnhip_tsne_bandwidths: the scratch is not 16-byte aligned");
    const int n_pad = ts_npad(n);
    if (scratch_bytes < ts_slab_bytes(n, TS_RT))
        return gcnhip_fail("gcnhip_tsne_bandwidths: the scratch is below the minimum (gcnhip_tsne_plan tells the bytes)");
    const TsPack P = ts_pack(pack, n, dim);
    const int batch_rows = (int)std::min<size_t>(scratch_bytes / ts_slab_bytes(n, TS_RT), (size_t)(n_pad / TS_RT)) * TS_RT;
    float *slab = (float *)scratch;
    tsne_zero_kernel<<<1, 1, 0, c->stream>>>(unconverged);
    GCNHIP_LAUNCH_CHECK();
    for (int row0 = 0; row0 < n; row0 += batch_rows) {
        const int rows_here = std::min(batch_rows, n - row0);
        if (ts_walk<2, TS_SLAB>(ts_dp(dim), c, P, (const float *)nullptr, n, n_pad, row0, batch_rows, ceil_div(rows_here, TS_RT), 0, slab,
                                (double *)nullptr) != 0)
            return gcnhip_fail("gcnhip_tsne_bandwidths: the distance launch failed");
        tsne_search_kernel<<<ceil_div(rows_here, 4), 256, 0, c->stream>>>(slab, n, n_pad, row0, rows_here, P.valid, std::log(perplexity), P.S, beta, m,
                                                                          inv_z, unconverged);
        GCNHIP_LAUNCH_CHECK();
    }
    return 0;
}

int gcnhip_tsne_gradient(gcnhip_ctx *c, const void *pack, int n, int dim, const float *y, int k, int want_kl, double *rowsums, void *scratch,
                         size_t scratch_bytes) {
    if (!c || !pack || !y || !rowsums || !scratch || n < 1) return gcnhip_fail("gcnhip_tsne_gradient: invalid argument");
    if (dim < 1 || dim > TS_MAX_DIM) return gcnhip_fail("gcnhip_tsne_gradient: 1 <= dim <= 256");
    if (k != 2 && k != 3) return gcnhip_fail("gcnhip_tsne_gradient: k must be 2 or 3");
    if (!aligned16(scratch)) return gcnhip_fail("gcnhip_tsne_gradient: the scratch is not 16-byte aligned");
    const int n_pad = ts_npad(n), n_parts = ceil_div(n_pad, TS_PART);
    if (scratch_bytes < ts_part_bytes(n, TS_RT))
        return gcnhip_fail("gcnhip_tsne_gradient: the scratch is below the minimum (gcnhip_tsne_plan tells the bytes)");
    const TsPack P = ts_pack((void *)pack, n, dim);
    const int batch_rows = (int)std::min<size_t>(scratch_bytes / ts_part_bytes(n, TS_RT), (size_t)(n_pad / TS_RT)) * TS_RT;
    double *partials = (double *)scratch;
    for (int row0 = 0; row0 < n; row0 += batch_rows) {
        const int rows_here = std::min(batch_rows, n - row0), tiles = ceil_div(rows_here, TS_RT);
        const int rc = k == 2 ? ts_walk<2, TS_GRAD>(ts_dp(dim), c, P, y, n, n_pad, row0, batch_rows, tiles, want_kl, (float *)nullptr, partials)
                              : ts_walk<3, TS_GRAD>(ts_dp(dim), c, P, y, n, n_pad, row0, batch_rows, tiles, want_kl, (float *)nullptr, partials);
        if (rc != 0) return gcnhip_fail("gcnhip_tsne_gradient: the launch failed");
        tsne_fold_kernel<<<ceil_div((int64_t)rows_here * TS_NACC, 256), 256, 0, c->stream>>>(partials, n_parts, row0, rows_here, batch_rows, rowsums);
        GCNHIP_LAUNCH_CHECK();
    }
    return 0;
}

int gcnhip_tsne_update(gcnhip_ctx *c, const void *pack, int n, int dim, int k, const double *rowsums, double exaggeration, double momentum,
                       double learning_rate, int apply, double *state, float *y, double *grad, double *stats) {
    if (!c || !pack || !rowsums || n < 1 || (apply && (!state || !y))) return gcnhip_fail("gcnhip_tsne_update: invalid argument");
    if (dim < 1 || dim > TS_MAX_DIM) return gcnhip_fail("gcnhip_tsne_update: 1 <= dim <= 256");
    if (k != 2 && k != 3) return gcnhip_fail("gcnhip_tsne_update: k must be 2 or 3");
    const TsPack P = ts_pack((void *)pack, n, dim);
    if (k == 2) tsne_step_kernel<2><<<1, 256, 0, c->stream>>>(rowsums, P.valid, n, exaggeration, momentum, learning_rate, apply, state, y, grad, stats);
    else tsne_step_kernel<3><<<1, 256, 0, c->stream>>>(rowsums, P.valid, n, exaggeration, momentum, learning_rate, apply, state, y, grad, stats);
    GCNHIP_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
