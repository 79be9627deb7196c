// silhouette.hip — the silhouette widths of a labelling of a table's rows (Rousseeuw, 1987; scikit-learn's silhouette_samples with
// the Euclidean metric).  Beyond the reference, which never looks at its hidden matrix.
//
// The table contract is kmeans.hip's: f32 [n_table x ld], 1 <= dim <= 256, dim <= ld, rows of any stride and alignment; columns
// [dim, ld) are never read as values.  d_rows is a device int32 list of n rows (repeats allowed; NULL: rows 0 .. n - 1); the row
// used is x^ = (float)(x . inv_norm[r]) (inv_norm == NULL: x itself).  1 <= k <= 256.  No float atomics, no allocation, no
// synchronisation; every output's bits are a function of the arguments' contents alone.
//
// The POINTS are the list positions i with a label L[i] in [0, k) and a row in the table.  d(i, j) = sqrtf(max(0, (xn_i + xn_j) -
// 2 . dot_f32(x^_i, x^_j))), xn = (sumsq_f32(x) . inv) . inv as kmeans_assign_kernel forms it, the dot the exact f32 fma chain in
// column order.  S(i, c) = the sum of d(i, j) over the points j of label c, j != i BY POSITION.
//
// gcnhip_silhouette_sums   (1) the points are bucketed by label with kmeans.hip's histogram / scan / scatter (bucket.h): a stable
//   bucketing, so the members of a label are in ascending position; (2) every label's member list is cut into segments of SIL_SEG
//   members; (3) a workgroup of 256 threads stages 64 list positions in LDS once and walks a group of segments, each in tiles of
//   64 members gathered through the member list; wave w owns positions 16w .. 16w + 15: v_mfma_f32_16x16x4_f32 with A = 16
//   members, B = its 16 rows, four independent accumulators, so that lane (l15, kg) holds the dots of row l15 with members
//   16t + 4kg + r of the tile; (4) the lane adds (double)d of its entries in ascending member index, tile after tile of the
//   segment; at the segment's end the four lane groups of a row are added as (g0 + g1) + (g2 + g3): the (row, segment) partial;
//   (5) a fold adds a label's segment partials in order into sums.  Rows are taken in batches of as many 64-row tiles as the
//   caller's scratch holds: fewer bytes, more launches, the same sequence of additions.  How many segments a workgroup walks is
//   chosen by the size of the launch and changes no bits either.
// gcnhip_silhouette_rows   a wave per position: a = S(i, A) / (n_A - 1), b = the lowest S(i, c) / n_c over c != A with n_c > 0
//   (the lowest c on equal means), s = (b - a) / max(a, b), each ONE float64 expression.  cluster_sum and total: a workgroup per
//   label (and one for all) adds s in a fixed strided order and a fixed tree.
#include "bucket.h"
#include <algorithm>
#include <climits>
#include <cstdio>

using f32x4 = __attribute__((ext_vector_type(4))) float;

constexpr int SIL_MAX_DIM = 256;
constexpr int SIL_RT = 64;                        // list positions per row tile
constexpr int SIL_CT = 64;                        // members per LDS tile
constexpr int SIL_SEG = 512;                      // members per segment (part of the definition of the sums' order)
constexpr int SIL_MAX_GROUP = 16;                 // segments a workgroup walks at most

// A wave stages 16 rows, lanes along a row: lane l15 (of every group) names the list position of row 16 . wave + l15 (-1: none).
// dst [64][qld] gets the scaled rows, zero-padded to dpad; dxn their squared norms; dpos the positions.
__device__ __forceinline__ void sil_stage(const float *__restrict__ table, int ld, int n_table, int dim, int dpad, int qld,
                                 const float *__restrict__ inv_norm, const int32_t *__restrict__ d_rows, int pos_mine, float *__restrict__ dst,
                                 float *__restrict__ dxn, int *__restrict__ dpos, int wave, int lane) {
    const int r_mine = pos_mine >= 0 ? list_row(d_rows, pos_mine, n_table) : -1;
    const float f_mine = r_mine >= 0 && inv_norm ? inv_norm[r_mine] : 1.f;
    float v[16][4];                                             // every load of the 16 rows is issued before the first sum
#pragma unroll
    for (int rr = 0; rr < 16; rr++) {
        const int r = __shfl(r_mine, rr, WAVE);
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int col = lane + WAVE * u;
            v[rr][u] = r >= 0 && col < dim ? table[(size_t)r * ld + col] : 0.f;
        }
    }
#pragma unroll
    for (int rr = 0; rr < 16; rr++) {
        const int q = 16 * wave + rr;
        const float f = __shfl(f_mine, rr, WAVE);
        float s = 0.f;
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int col = lane + WAVE * u;
            if (col < dpad) dst[q * qld + col] = __fmul_rn(v[rr][u], f);
            s += v[rr][u] * v[rr][u];                           // columns lane, lane + 64, ..: the order of the assign kernel
        }
        s = wave_sum(s);
        if (lane == rr) {
            dpos[q] = r_mine >= 0 ? pos_mine : -1;
            dxn[q] = (s * f_mine) * f_mine;
        }
    }
}

// grid (row tiles of the batch, groups of `group` segments): partials[seg][position - row0], a batch of batch_rows positions
__global__ __launch_bounds__(256) void sil_sums_kernel(const float *__restrict__ table, int ld, int n_table, int dim,
                                                       const float *__restrict__ inv_norm, const int32_t *__restrict__ d_rows, int n,
                                                       const int32_t *__restrict__ order, const int32_t *__restrict__ cstart,
                                                       const int32_t *__restrict__ segstart, int k, int row0, int batch_rows, int group,
                                                       double *__restrict__ partials) {
    extern __shared__ __align__(16) unsigned char smem[];
    const int n_seg = segstart[k];
    const int seg_lo = blockIdx.y * group, seg_hi = min(seg_lo + group, n_seg);
    if (seg_lo >= n_seg) return;                                // the same for every thread of the workgroup
    const int dpad = (dim + 15) / 16 * 16, qld = dpad + 4;
    float *Xs = (float *)smem;                                  // [64][qld] the tile's rows, scaled, zero-padded
    float *Cs = Xs + SIL_RT * qld;                              // [64][qld] a tile of members
    float *xxn = Cs + SIL_CT * qld;                             // [64] squared norms of the rows
    float *cxn = xxn + SIL_RT;                                  // [64] of the members
    int *xpos = (int *)(cxn + SIL_CT);                          // [64] list position of a row, -1: none
    int *cpos = xpos + SIL_RT;                                  // [64] of a member, -1: padding
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int kg = lane >> 4, l15 = lane & 15;
    const int q = 16 * wave + l15;
    const int i_local = blockIdx.x * SIL_RT + q, i = row0 + i_local;

    sil_stage(table, ld, n_table, dim, dpad, qld, inv_norm, d_rows, i < n ? i : -1, Xs, xxn, xpos, wave, lane);
    const float *xrow = Xs + q * qld;
    for (int seg = seg_lo; seg < seg_hi; seg++) {
        const int c = segment_key(segstart, k, seg);
        const int first = cstart[c] + (seg - segstart[c]) * SIL_SEG;
        const int count = min(SIL_SEG, cstart[c + 1] - first);
        double sum = 0.0;
        for (int m0 = 0; m0 < count; m0 += SIL_CT) {
            __syncthreads();                                    // the products with the tile before this one are done
            const int m = m0 + q;
            sil_stage(table, ld, n_table, dim, dpad, qld, inv_norm, d_rows, m < count ? order[first + m] : -1, Cs, cxn, cpos, wave, lane);
            __syncthreads();
            f32x4 acc[4] = {};
            for (int j0 = 0; j0 < dpad; j0 += 16) {
                const int col = j0 + 4 * kg;
                const f32x4 b = *(const f32x4 *)(xrow + col);
                f32x4 a[4];
#pragma unroll
                for (int t = 0; t < 4; t++) a[t] = *(const f32x4 *)(Cs + (16 * t + l15) * qld + col);
#pragma unroll
                for (int s = 0; s < 4; s++)
#pragma unroll
                    for (int t = 0; t < 4; t++) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[t][s], b[s], acc[t], 0, 0, 0);
            }
            const float xni = xxn[q];
            const int ipos = xpos[q];
#pragma unroll
            for (int t = 0; t < 4; t++)
#pragma unroll
                for (int r = 0; r < 4; r++) {                   // D[row 4kg + r][col l15]: member 16t + 4kg + r, this lane's row
                    const int cc = 16 * t + 4 * kg + r;
                    const int j = cpos[cc];
                    const float d2 = (xni + cxn[cc]) - 2.f * acc[t][r];
                    const float d = sqrtf(fmaxf(d2, 0.f));
                    sum += j >= 0 && j != ipos ? (double)d : 0.0;     // padding and the self pair, by index: + 0 changes no bit
                }
        }
        sum += __shfl_xor(sum, 16, WAVE);                       // (g0 + g1), (g2 + g3)
        sum += __shfl_xor(sum, 32, WAVE);                       // their sum
        if (kg == 0) partials[(size_t)seg * batch_rows + i_local] = sum;
    }
}

// grid (positions of the batch / 256, k): the partials of label c in segment order; a position that is not a point gets 0
__global__ __launch_bounds__(256) void sil_fold_kernel(const double *__restrict__ partials, const int32_t *__restrict__ segstart,
                                                       const int32_t *__restrict__ labels, const int32_t *__restrict__ d_rows, int n, int n_table,
                                                       int k, int row0, int rows_here, int batch_rows, double *__restrict__ sums) {
    const int i_local = blockIdx.x * 256 + threadIdx.x, c = blockIdx.y;
    if (i_local >= rows_here) return;
    const int i = row0 + i_local;
    double a = 0.0;
    if (member_centre(labels, d_rows, i, n, n_table, k) >= 0)
        for (int s = segstart[c]; s < segstart[c + 1]; s++) a += partials[(size_t)s * batch_rows + i_local];
    sums[(size_t)i * k + c] = a;
}

__device__ inline bool mean_before(double ma, int ca, double mb, int cb) { return ma < mb || (ma == mb && ca < cb); }

// a wave per position
__global__ __launch_bounds__(256) void sil_rows_kernel(const double *__restrict__ sums, const int32_t *__restrict__ labels,
                                                       const int32_t *__restrict__ sizes, const int32_t *__restrict__ d_rows, int n_table, int n,
                                                       int k, double *__restrict__ s, double *__restrict__ a, double *__restrict__ b,
                                                       int32_t *__restrict__ neighbor) {
    __shared__ int sz[KM_MAX_K];
    __shared__ int nonempty_s;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (threadIdx.x < k) sz[threadIdx.x] = sizes[threadIdx.x];
    __syncthreads();
    if (threadIdx.x == 0) {
        int ne = 0;
        for (int c = 0; c < k; c++) ne += sz[c] > 0;
        nonempty_s = ne;
    }
    __syncthreads();
    const int i = blockIdx.x * 4 + wave;
    if (i >= n) return;
    const int A = member_centre(labels, d_rows, i, n, n_table, k);
    if (A < 0) {
        if (lane == 0) { s[i] = NAN; a[i] = NAN; b[i] = NAN; neighbor[i] = -1; }
        return;
    }
    const double *row = sums + (size_t)i * k;
    double bm = INFINITY;
    int bc = INT_MAX;
    for (int c = lane; c < k; c += WAVE)
        if (c != A && sz[c] > 0) {
            const double m = row[c] / (double)sz[c];
            if (mean_before(m, c, bm, bc)) { bm = m; bc = c; }
        }
#pragma unroll
    for (int off = 1; off < WAVE; off <<= 1) {
        const double om = __shfl_xor(bm, off, WAVE);
        const int oc = __shfl_xor(bc, off, WAVE);
        if (mean_before(om, oc, bm, bc)) { bm = om; bc = oc; }
    }
    if (lane == 0) {
        const int nA = sz[A];
        const double av = nA > 1 ? row[A] / (double)(nA - 1) : 0.0;
        double bv = 0.0, sv = 0.0;
        int nb = -1;
        if (nonempty_s >= 2) {
            bv = bm;
            nb = bc;
            const double mx = fmax(av, bv);
            sv = nA > 1 && mx > 0.0 ? (bv - av) / mx : 0.0;
        }
        s[i] = sv;
        a[i] = av;
        b[i] = bv;
        neighbor[i] = nb;
    }
}

// block c < k: the sum of s over the points of label c; block k: over every point, and the counts.  Thread t adds positions
// t, t + 256, .. in order, then a fixed tree.
__global__ __launch_bounds__(256) void sil_totals_kernel(const double *__restrict__ s, const int32_t *__restrict__ labels,
                                                         const int32_t *__restrict__ sizes, const int32_t *__restrict__ d_rows, int n_table, int n,
                                                         int k, double *__restrict__ cluster_sum, double *__restrict__ total,
                                                         int32_t *__restrict__ counts) {
    __shared__ double red[256];
    __shared__ int pts[256];
    const int c = blockIdx.x, t = threadIdx.x;
    double sum = 0.0;
    int points = 0;
    for (int i = t; i < n; i += 256) {
        const int A = member_centre(labels, d_rows, i, n, n_table, k);
        if (A >= 0 && (c == k || A == c)) { sum += s[i]; points++; }
    }
    red[t] = sum;
    pts[t] = points;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (t < w) { red[t] += red[t + w]; pts[t] += pts[t + w]; }
        __syncthreads();
    }
    if (t == 0) {
        if (c < k) cluster_sum[c] = red[0];
        else {
            int ne = 0;
            for (int j = 0; j < k; j++) ne += sizes[j] > 0;
            *total = red[0];
            counts[0] = pts[0];
            counts[1] = n - pts[0];
            counts[2] = ne;
        }
    }
}

// ---- entry points ------------------------------------------------------------------------------------------------------------

static size_t up256(size_t b) { return (b + 255) / 256 * 256; }

// the sums' scratch: {hist | cstart, segstart | order | dpart | partials [seg_max x batch rows]}
struct SilLayout {
    int n_chunks, seg_max, rows_full;
    size_t hist, starts, order, dpart, partials;
};
static SilLayout sil_layout(int n, int k) {
    SilLayout L;
    L.n_chunks = std::max(ceil_div(n, KM_CHUNK), 1);
    L.seg_max = n / SIL_SEG + k;                                // the sum of ceil(size_c / SIL_SEG) is at most this
    L.rows_full = std::max(ceil_div(n, SIL_RT), 1) * SIL_RT;
    L.hist = 0;
    L.starts = L.hist + up256((size_t)L.n_chunks * k * sizeof(int32_t));
    L.order = L.starts + up256(2 * (size_t)(k + 1) * sizeof(int32_t));
    L.dpart = L.order + up256((size_t)std::max(n, 1) * sizeof(int32_t));
    L.partials = L.dpart + up256((size_t)L.n_chunks * sizeof(double));
    return L;
}

extern "C" {

int gcnhip_silhouette_plan(int n, int k, int dim, size_t *bytes, size_t *bytes_min) {
    if (n < 0 || dim < 1 || dim > SIL_MAX_DIM) return gcnhip_fail("gcnhip_silhouette_plan: invalid argument (n >= 0, 1 <= dim <= 256)");
    if (k < 1 || k > KM_MAX_K) return gcnhip_fail("gcnhip_silhouette_plan: 1 <= k <= 256");
    const SilLayout L = sil_layout(n, k);
    const size_t per_row = (size_t)L.seg_max * sizeof(double);
    if (bytes) *bytes = L.partials + per_row * (size_t)L.rows_full;
    if (bytes_min) *bytes_min = L.partials + per_row * SIL_RT;
    return 0;
}

int gcnhip_silhouette_sums(gcnhip_ctx *c, const float *table, int ld, int n_table, int dim, const float *inv_norm, const int32_t *d_rows, int n,
                           const int32_t *labels, int k, double *sums, int32_t *sizes, void *scratch, size_t scratch_bytes) {
    if (!c || !table || !sizes || !scratch || n_table < 0 || n < 0 || (n > 0 && (!labels || !sums)))
        return gcnhip_fail("gcnhip_silhouette_sums: invalid argument");
    if (dim < 1 || dim > SIL_MAX_DIM) return gcnhip_fail("gcnhip_silhouette_sums: 1 <= dim <= 256");
    if (ld < dim) return gcnhip_fail("gcnhip_silhouette_sums: the row stride is below dim");
    if (k < 1 || k > KM_MAX_K) return gcnhip_fail("gcnhip_silhouette_sums: 1 <= k <= 256");
    if (!d_rows && n > n_table) return gcnhip_fail("gcnhip_silhouette_sums: without a row list n is at most n_table");
    if (!aligned16(scratch)) return gcnhip_fail("gcnhip_silhouette_sums: the scratch is not 16-byte aligned");
    size_t need_min = 0;
    if (gcnhip_silhouette_plan(n, k, dim, nullptr, &need_min) != 0) return -1;
    if (scratch_bytes < need_min) return gcnhip_fail("gcnhip_silhouette_sums: the scratch is below the minimum (gcnhip_silhouette_plan tells the bytes)");
    const SilLayout L = sil_layout(n, k);
    unsigned char *base = (unsigned char *)scratch;
    int32_t *hist = (int32_t *)(base + L.hist), *cstart = (int32_t *)(base + L.starts), *segstart = cstart + (k + 1);
    int32_t *order = (int32_t *)(base + L.order);
    double *dpart = (double *)(base + L.dpart), *partials = (double *)(base + L.partials);
    const size_t per_tile = (size_t)L.seg_max * SIL_RT * sizeof(double);
    const int batch_rows = (int)std::min<size_t>((scratch_bytes - L.partials) / per_tile, (size_t)(L.rows_full / SIL_RT)) * SIL_RT;

    kmeans_hist_kernel<<<L.n_chunks, 256, 0, c->stream>>>(labels, d_rows, nullptr, n, n_table, k, hist, dpart);
    GCNHIP_LAUNCH_CHECK();
    kmeans_scan_kernel<<<1, 256, 0, c->stream>>>(hist, L.n_chunks, k, SIL_SEG, sizes, cstart, segstart);
    GCNHIP_LAUNCH_CHECK();
    if (n == 0) return 0;
    kmeans_scatter_kernel<<<L.n_chunks, 64, 0, c->stream>>>(labels, d_rows, n, n_table, k, hist, cstart, order);
    GCNHIP_LAUNCH_CHECK();
    const int dpad = (dim + 15) / 16 * 16;
    const size_t lds = sizeof(float) * ((size_t)(SIL_RT + SIL_CT) * (dpad + 4) + 2 * (SIL_RT + SIL_CT));
    if (lds > 64 * 1024) GCNHIP_TRY(hipFuncSetAttribute((const void *)sil_sums_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    const int n_cu = c->n_cu > 0 ? c->n_cu : 128;
    for (int row0 = 0; row0 < n; row0 += batch_rows) {
        const int rows_here = std::min(batch_rows, n - row0);
        const int tiles = ceil_div(rows_here, SIL_RT);
        int group = (int)std::min<int64_t>(std::max<int64_t>((int64_t)tiles * L.seg_max / (8 * (int64_t)n_cu), 1), SIL_MAX_GROUP);
        group = std::max(group, ceil_div(L.seg_max, 65535));   // the grid's second dimension
        sil_sums_kernel<<<dim3(tiles, ceil_div(L.seg_max, group)), 256, lds, c->stream>>>(table, ld, n_table, dim, inv_norm, d_rows, n, order, cstart,
                                                                                       segstart, k, row0, batch_rows, group, partials);
        GCNHIP_LAUNCH_CHECK();
        sil_fold_kernel<<<dim3(ceil_div(rows_here, 256), k), 256, 0, c->stream>>>(partials, segstart, labels, d_rows, n, n_table, k, row0, rows_here,
                                                                               batch_rows, sums);
        GCNHIP_LAUNCH_CHECK();
    }
    return 0;
}

int gcnhip_silhouette_rows(gcnhip_ctx *c, const double *sums, const int32_t *labels, const int32_t *sizes, const int32_t *d_rows, int n_table, int n,
                           int k, double *s, double *a, double *b, int32_t *neighbor, double *cluster_sum, double *total, int32_t *counts) {
    if (!c || !sizes || !cluster_sum || !total || !counts || n_table < 0 || n < 0 || (n > 0 && (!sums || !labels || !s || !a || !b || !neighbor)))
        return gcnhip_fail("gcnhip_silhouette_rows: invalid argument");
    if (k < 1 || k > KM_MAX_K) return gcnhip_fail("gcnhip_silhouette_rows: 1 <= k <= 256");
    if (!d_rows && n > n_table) return gcnhip_fail("gcnhip_silhouette_rows: without a row list n is at most n_table");
    if (n > 0) {
        sil_rows_kernel<<<ceil_div(n, 4), 256, 0, c->stream>>>(sums, labels, sizes, d_rows, n_table, n, k, s, a, b, neighbor);
        GCNHIP_LAUNCH_CHECK();
    }
    sil_totals_kernel<<<k + 1, 256, 0, c->stream>>>(s, labels, sizes, d_rows, n_table, n, k, cluster_sum, total, counts);
    GCNHIP_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
