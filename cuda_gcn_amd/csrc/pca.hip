// pca.hip — principal component analysis of the rows of a trained model's hidden layer: the float64 mean, the float64 scatter
// matrix on the f64 MFMA, and the projection of rows onto a given basis.  The symmetric eigenproblem between the second and the
// third is the host's (host/pca.h).  Beyond the reference, which never looks at its hidden matrix.
//
// Rows.  The table contract is embed.hip's: f32 [n_table x ld], 1 <= dim <= 256, dim <= ld, rows of any stride and alignment;
// columns [dim, ld) are never read as values.  d_rows is a device int32 list of n positions (repeats count as often as listed;
// NULL: rows 0 .. n - 1); an entry outside [0, n_table) is skipped and leaves a NaN row in a projection.  The row used is
// x_i[a] = T[r][a] . inv_norm[r], one rounded f32 product — the bits embed(normalize) exports — and T[r][a] itself with
// inv_norm == NULL.  count = the number of valid positions.
// Mean.  mean[a] = (the float64 sum of (double)x_i[a] over the valid positions) / count; count == 0 gives NaN.
// Scatter.  S[a][b] = sum_i c_ia . c_ib, c_ia = (double)x_i[a] - mean[a] formed in float64 (mean == NULL: c = x, the uncentred
//   Gram matrix); products and sums are float64 on v_mfma_f64_16x16x4_f64.  Only the 16 x 16 tile pairs on or above the diagonal
//   are computed, and of a diagonal tile only the entries with a <= b are used: the rest of S is their mirror, so S is symmetric
//   bit for bit.
// Order of summation.  No float atomics; every output's bits are a function of the arguments' contents alone, not of launch
//   geometry, scratch size or block order.  The list is cut into parts of PCA_PART positions (part of the definition, as KM_CHUNK
//   / KM_SEG are in kmeans.hip).  A part's partial is accumulated in ascending position — for the mean one addition per
//   position, for the scatter one MFMA per four consecutive positions (a skipped position and one past the end enter as exact
//   zeros) — and the partials are added, from +0, in ascending part order.  A call handles as many parts per launch as its
//   scratch holds: less scratch, more launches of fewer parts, the same sequence of additions.
//   gcnhip_pca_plan: T = t (t + 1) / 2 upper tiles, t = ceil(dim / 16); a part's partial is T . 256 doubles;
//   bytes_full = max(ceil(n / PCA_PART), 1) . T . 2048, bytes_min = T . 2048.  The mean uses dim doubles per part of the same
//   scratch and as many parts per launch as the scatter would.
// Projection.  y[i][j] = (float)(scale[j] . sum_a c_ia . V[a][j]) for j < k <= dim, V = basis [dim x ldv] float64; the sum is one
//   float64 fma chain in ascending a from +0, so a row's bits do not depend on the batch it is in.  scale == NULL: no factor.
//
// The scatter kernel.  A workgroup of 8 waves owns one part.  It stages tiles of PCA_RT = 64 positions in LDS as f32 (the same
// tile as doubles would be twice the bytes), dim padded to a multiple of 16 with zeros in LDS, not in memory; the mean sits
// beside it as doubles (zero in the padding, so a padded column is c = 0).  Register budget: dim = 256 has 136 upper tiles of 8
// registers a lane each; of the three ways to hold them — 8 waves, AGPR accumulators at one wave per SIMD, tile pairs split over
// gridDim.y — this is the first: wave w keeps upper tiles w, w + 8, .. in accumulators, at most 17, 136 registers of the 256 a
// wave has at two waves per SIMD.  An operand is widened and centred as it is read:
// A[l & 15][l >> 4] = c[position 4 . step + (l >> 4)][16 ti + (l & 15)], B likewise with tj, and the result tile is read by the
// f64 map (col = lane & 15, row = (lane >> 4) + 4 . reg), not the f32 one.  The kernel is instantiated for 1, 2, 5, 10 and 17
// tiles a wave (dim <= 32, 64, 128, 192, 256); which instance runs changes no bit.
// -Rpass-analysis=kernel-resource-usage for gfx950, pca_scatter_kernel<1 / 2 / 5 / 10 / 17>: 42 / 54 / 90 / 155 / 253 VGPRs, no
// AGPRs, 0 bytes of scratch in every instance (and in every other kernel of this file); LDS is dynamic: 8 dpad + 256 (dpad + 16)
// + 256 bytes, 72 KB at dim = 256, 37 KB at 128.  The step loop is not unrolled and the operands of four tiles at a time are in
// flight (a scheduling barrier): unrolled, the instance of 17 spilled.
#include "common.h"
#include <algorithm>
#include <cstdio>

using f64x4 = __attribute__((ext_vector_type(4))) double;

constexpr int PCA_MAX_DIM = 256;
constexpr int PCA_PART = 1024;                    // positions per part (part of the definition of the sums' order)
constexpr int PCA_RT = 64;                        // positions per LDS tile of the scatter kernel
constexpr int PCA_WAVES = 8;                      // waves of a scatter workgroup
constexpr int PCA_PT = 16;                        // positions per workgroup of the projection
constexpr int PCA_FOLD = 32;                      // partials a fold thread has in flight (no part of any sum's order)

__device__ inline int pca_list_row(const int32_t *__restrict__ d_rows, int i, int n_table) {
    const int r = d_rows ? d_rows[i] : i;
    return r >= 0 && r < n_table ? r : -1;
}

// upper tile t of a matrix of nt x nt tiles, row-major over the pairs ti <= tj
__device__ inline void pca_tile_pair(int t, int nt, int &ti, int &tj) {
    int i = 0, left = nt;
    while (t >= left) { t -= left; left--; i++; }
    ti = i;
    tj = i + t;
}

// ---- mean -------------------------------------------------------------------------------------------------------------------

// block = part.  Tiles of 64 positions go through LDS: wave w loads rows 16w .. 16w + 15 of the tile, lanes along a row and every
// load issued before the first store, then thread j adds column j of the 64 rows in order — the one float64 chain of a column
// never waits on memory.  A skipped position and one past the end are rows of +0 (x + 0 = x: the chain's bits are those of the
// valid positions alone).  Each wave counts the valid positions it staged (an integer atomic).
__global__ __launch_bounds__(256) void pca_partsum_kernel(const float *__restrict__ table, int ld, int n_table, int dim,
                                                          const float *__restrict__ inv_norm, const int32_t *__restrict__ d_rows, int n,
                                                          int part0, double *__restrict__ partials, int32_t *__restrict__ count) {
    extern __shared__ __align__(16) unsigned char smem[];
    float *Xs = (float *)smem;                                  // [64][dim]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int part = part0 + blockIdx.x;
    const int first = part * PCA_PART, left_all = min(PCA_PART, n - first);
    double sum = 0.0;
    int valid = 0;
    for (int p0 = 0; p0 < left_all; p0 += PCA_RT) {
        __syncthreads();                                        // the sums of the previous tile are done
        const int q_mine = 16 * wave + (lane & 15);
        const int r_mine = p0 + q_mine < left_all ? pca_list_row(d_rows, first + p0 + q_mine, n_table) : -1;
        const float f_mine = r_mine >= 0 && inv_norm ? inv_norm[r_mine] : 1.f;
        valid += __popcll(__ballot(lane < 16 && r_mine >= 0));
        float v[16][4];
#pragma unroll
        for (int rr = 0; rr < 16; rr++) {
            const int r = __shfl(r_mine, rr, WAVE);
            const float f = __shfl(f_mine, rr, WAVE);
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const int col = lane + WAVE * u;
                v[rr][u] = r >= 0 && col < dim ? __fmul_rn(table[(size_t)r * ld + col], f) : 0.f;
            }
        }
#pragma unroll
        for (int rr = 0; rr < 16; rr++)
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const int col = lane + WAVE * u;
                if (col < dim) Xs[(16 * wave + rr) * dim + col] = v[rr][u];
            }
        __syncthreads();
        if ((int)threadIdx.x < dim) {
#pragma unroll 16
            for (int q = 0; q < PCA_RT; q++) sum += (double)Xs[q * dim + threadIdx.x];
        }
    }
    if ((int)threadIdx.x < dim) partials[(size_t)blockIdx.x * dim + threadIdx.x] = sum;
    if (lane == 0 && valid) atomicAdd(count, valid);
}

// thread j: the batch's partials in order onto the running sum
__global__ __launch_bounds__(256) void pca_meanfold_kernel(const double *__restrict__ partials, int parts, int dim, double *__restrict__ mean) {
    const int j = threadIdx.x;
    if (j >= dim) return;
    double a = mean[j];
    for (int p0 = 0; p0 < parts; p0 += PCA_FOLD) {             // PCA_FOLD loads in flight, then their additions in order
        double t[PCA_FOLD];
#pragma unroll
        for (int u = 0; u < PCA_FOLD; u++) t[u] = p0 + u < parts ? partials[(size_t)(p0 + u) * dim + j] : 0.0;
#pragma unroll
        for (int u = 0; u < PCA_FOLD; u++)
            if (p0 + u < parts) a += t[u];
    }
    mean[j] = a;
}

__global__ __launch_bounds__(256) void pca_meandiv_kernel(int dim, const int32_t *__restrict__ count, double *__restrict__ mean) {
    const int j = threadIdx.x;
    if (j < dim) mean[j] = mean[j] / (double)*count;
}

// ---- scatter ----------------------------------------------------------------------------------------------------------------

// block = part.  partials [part of the batch][upper tile][reg . 64 + lane]
template <int NS>
__global__ __launch_bounds__(64 * PCA_WAVES) void pca_scatter_kernel(const float *__restrict__ table, int ld, int n_table, int dim,
                                                                     const float *__restrict__ inv_norm, const int32_t *__restrict__ d_rows,
                                                                     int n, const double *__restrict__ mean, int part0,
                                                                     double *__restrict__ partials) {
    extern __shared__ __align__(16) unsigned char smem[];
    const int dpad = (dim + 15) / 16 * 16, qld = dpad + 16;     // 16 floats of padding: the four positions of a step in four bank groups
    double *Ms = (double *)smem;                                // [dpad] the mean, zero past dim (and everywhere without one)
    float *Xs = (float *)(Ms + dpad);                           // [64][qld] the tile's rows, zero-padded
    int *ok = (int *)(Xs + PCA_RT * qld);                       // [64] the position names a row of the table
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int kg = lane >> 4, l15 = lane & 15;
    const int nt = dpad / 16, T = nt * (nt + 1) / 2;
    const int part = part0 + blockIdx.x;
    const int first = part * PCA_PART, left_all = min(PCA_PART, n - first);

    for (int a = threadIdx.x; a < dpad; a += 64 * PCA_WAVES) Ms[a] = mean && a < dim ? mean[a] : 0.0;
    int ca[NS], cb[NS];                                         // first column of the tile's rows and of its columns, by slot
#pragma unroll
    for (int s = 0; s < NS; s++) {
        int ti = 0, tj = 0;
        if (wave + PCA_WAVES * s < T) pca_tile_pair(wave + PCA_WAVES * s, nt, ti, tj);
        ca[s] = 16 * ti;
        cb[s] = 16 * tj;
    }
    f64x4 acc[NS];
#pragma unroll
    for (int s = 0; s < NS; s++) acc[s] = f64x4{0.0, 0.0, 0.0, 0.0};

    constexpr int RW = PCA_RT / PCA_WAVES;                      // positions a wave stages
    for (int p0 = 0; p0 < left_all; p0 += PCA_RT) {
        __syncthreads();                                        // every wave is done with the previous tile (and Ms is written)
        {                                                       // a wave stages its own 8 positions, lanes along a row
            const int q_mine = RW * wave + (lane & (RW - 1));
            const int r_mine = p0 + q_mine < left_all ? pca_list_row(d_rows, first + p0 + q_mine, n_table) : -1;
            const float f_mine = r_mine >= 0 && inv_norm ? inv_norm[r_mine] : 1.f;
#pragma unroll 1
            for (int h = 0; h < RW / 4; h++) {                  // four rows at a time (the instance of 17 tiles has no registers for eight):
                float v[4][4];                                  // every load of them is issued before the first store
#pragma unroll
                for (int rr = 0; rr < 4; rr++) {
                    const int r = __shfl(r_mine, 4 * h + rr, WAVE);
                    const float f = __shfl(f_mine, 4 * h + rr, WAVE);
#pragma unroll
                    for (int u = 0; u < 4; u++) {
                        const int col = lane + WAVE * u;
                        v[rr][u] = r >= 0 && col < dim ? __fmul_rn(table[(size_t)r * ld + col], f) : 0.f;
                    }
                }
#pragma unroll
                for (int rr = 0; rr < 4; rr++) {
                    const int q = RW * wave + 4 * h + rr;
#pragma unroll
                    for (int u = 0; u < 4; u++) {
                        const int col = lane + WAVE * u;
                        if (col < dpad) Xs[q * qld + col] = v[rr][u];
                    }
                }
            }
            if (lane < RW) ok[q_mine] = r_mine >= 0;
        }
        __syncthreads();
#pragma unroll 1
        for (int step = 0; step < PCA_RT / 4; step++) {         // not unrolled: the operands of one step are all a wave keeps beside its tiles
            const int q = 4 * step + kg;
            const bool valid = ok[q] != 0;
            const float *xrow = Xs + q * qld + l15;
#pragma unroll
            for (int s = 0; s < NS; s++) {
                if (wave + PCA_WAVES * s < T) {                 // the same for every lane of the wave
                    const double a = valid ? (double)xrow[ca[s]] - Ms[ca[s] + l15] : 0.0;
                    const double b = valid ? (double)xrow[cb[s]] - Ms[cb[s] + l15] : 0.0;
                    acc[s] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[s], 0, 0, 0);
                }
                if (s % 4 == 3) __builtin_amdgcn_sched_barrier(0);   // the operands of four tiles in flight, not of all seventeen
            }
        }
    }
#pragma unroll
    for (int s = 0; s < NS; s++) {
        const int t = wave + PCA_WAVES * s;
        if (t < T) {
            double *out = partials + ((size_t)blockIdx.x * T + t) * 256;
#pragma unroll
            for (int r = 0; r < 4; r++) out[r * 64 + lane] = acc[s][r];   // D[row kg + 4r][col l15]: the f64 map
        }
    }
}

// thread = (upper tile, element): the batch's partials in order onto the running S[a][b], for a <= b < dim alone
__global__ __launch_bounds__(256) void pca_scatterfold_kernel(const double *__restrict__ partials, int parts, int dim, double *__restrict__ S) {
    const int nt = (dim + 15) / 16, T = nt * (nt + 1) / 2;
    const int t = blockIdx.x, e = threadIdx.x;
    int ti, tj;
    pca_tile_pair(t, nt, ti, tj);
    const int lane = e & 63, r = e >> 6;
    const int a = 16 * ti + (lane >> 4) + 4 * r, b = 16 * tj + (lane & 15);
    if (a > b || b >= dim) return;
    double s = S[(size_t)a * dim + b];
    for (int p0 = 0; p0 < parts; p0 += PCA_FOLD) {             // PCA_FOLD loads in flight, then their additions in order
        double v[PCA_FOLD];
#pragma unroll
        for (int u = 0; u < PCA_FOLD; u++) v[u] = p0 + u < parts ? partials[((size_t)(p0 + u) * T + t) * 256 + e] : 0.0;
#pragma unroll
        for (int u = 0; u < PCA_FOLD; u++)
            if (p0 + u < parts) s += v[u];
    }
    S[(size_t)a * dim + b] = s;
}

__global__ __launch_bounds__(256) void pca_mirror_kernel(int dim, double *__restrict__ S) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= dim * dim) return;
    const int a = e / dim, b = e % dim;
    if (a > b) S[(size_t)a * dim + b] = S[(size_t)b * dim + a];
}

// ---- projection -------------------------------------------------------------------------------------------------------------

// block = 16 positions, centred in LDS as doubles; thread (position t / 16, component t % 16, + 16, ..): one fma chain in column order
__global__ __launch_bounds__(256) void pca_project_kernel(const float *__restrict__ table, int ld, int n_table, int dim,
                                                          const float *__restrict__ inv_norm, const int32_t *__restrict__ d_rows, int n,
                                                          const double *__restrict__ mean, const double *__restrict__ basis, int ldv, int k,
                                                          const double *__restrict__ scale, float *__restrict__ out, int ldy) {
    __shared__ double Cs[PCA_PT][PCA_MAX_DIM + 1];
    __shared__ int rok[PCA_PT];
    const int i0 = blockIdx.x * PCA_PT;
    for (int e = threadIdx.x; e < PCA_PT * dim; e += 256) {
        const int q = e / dim, a = e % dim;
        const int r = i0 + q < n ? pca_list_row(d_rows, i0 + q, n_table) : -1;
        double c = 0.0;
        if (r >= 0) {
            const float x = inv_norm ? __fmul_rn(table[(size_t)r * ld + a], inv_norm[r]) : table[(size_t)r * ld + a];
            c = (double)x - (mean ? mean[a] : 0.0);
        }
        Cs[q][a] = c;
        if (a == 0) rok[q] = r >= 0;
    }
    __syncthreads();
    const int q = threadIdx.x >> 4, i = i0 + q;
    if (i >= n) return;
    for (int j = threadIdx.x & 15; j < k; j += 16) {
        double s = 0.0;
#pragma unroll 16
        for (int a = 0; a < dim; a++) s = fma(Cs[q][a], basis[(size_t)a * ldv + j], s);   // the loads run ahead of the one chain
        if (scale) s = scale[j] * s;
        out[(size_t)i * ldy + j] = rok[q] ? (float)s : NAN;
    }
}

// ---- entry points ------------------------------------------------------------------------------------------------------------

static const char *pca_refusal(const void *table, int ld, int n_table, int dim, const int32_t *d_rows, int n) {
    if (!table || n_table < 0 || n < 0) return "invalid argument";
    if (dim < 1 || dim > PCA_MAX_DIM) return "1 <= dim <= 256";
    if (ld < dim) return "the row stride is below dim";
    if (!d_rows && n > n_table) return "without a row list n is at most n_table";
    return nullptr;
}
#define PCA_REFUSE(NAME, WHY)                                                     \
    do {                                                                          \
        char msg[160];                                                            \
        snprintf(msg, sizeof msg, "%s: %s", NAME, WHY);                           \
        return gcnhip_fail(msg);                                                  \
    } while (0)

static size_t pca_part_bytes(int dim) {
    const size_t nt = (size_t)(dim + 15) / 16;
    return nt * (nt + 1) / 2 * 256 * sizeof(double);
}

template <int NS>
static int pca_scatter_launch(gcnhip_ctx *c, int parts, size_t lds, const float *table, int ld, int n_table, int dim, const float *inv_norm,
                              const int32_t *d_rows, int n, const double *mean, int part0, double *partials) {
    if (lds > 64 * 1024) GCNHIP_TRY(hipFuncSetAttribute((const void *)pca_scatter_kernel<NS>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    pca_scatter_kernel<NS><<<parts, 64 * PCA_WAVES, lds, c->stream>>>(table, ld, n_table, dim, inv_norm, d_rows, n, mean, part0, partials);
    GCNHIP_LAUNCH_CHECK();
    return 0;
}

extern "C" {

int gcnhip_pca_plan(int n, int dim, size_t *bytes_full, size_t *bytes_min) {
    if (n < 0 || dim < 1 || dim > PCA_MAX_DIM) return gcnhip_fail("gcnhip_pca_plan: invalid argument (n >= 0, 1 <= dim <= 256)");
    const size_t per = pca_part_bytes(dim);
    if (bytes_full) *bytes_full = per * (size_t)std::max(ceil_div(n, PCA_PART), 1);
    if (bytes_min) *bytes_min = per;
    return 0;
}

int gcnhip_pca_mean(gcnhip_ctx *c, const float *table, int ld, int n_table, int dim, const float *inv_norm, const int32_t *d_rows, int n,
                    double *mean, int32_t *count, void *scratch, size_t scratch_bytes) {
    if (!c || !mean || !count || !scratch) return gcnhip_fail("gcnhip_pca_mean: invalid argument");
    if (const char *why = pca_refusal(table, ld, n_table, dim, d_rows, n)) PCA_REFUSE("gcnhip_pca_mean", why);
    if (!aligned16(scratch)) return gcnhip_fail("gcnhip_pca_mean: the scratch is not 16-byte aligned");
    const size_t per = pca_part_bytes(dim);
    if (scratch_bytes < per) return gcnhip_fail("gcnhip_pca_mean: the scratch is below the minimum (gcnhip_pca_plan tells the bytes)");
    const int parts = ceil_div(n, PCA_PART);
    const int batch = (int)std::min<size_t>(scratch_bytes / per, (size_t)std::max(parts, 1));
    const size_t mean_lds = (size_t)PCA_RT * dim * sizeof(float);
    if (mean_lds > 64 * 1024) GCNHIP_TRY(hipFuncSetAttribute((const void *)pca_partsum_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)mean_lds));
    GCNHIP_TRY(hipMemsetAsync(mean, 0, (size_t)dim * sizeof(double), c->stream));
    GCNHIP_TRY(hipMemsetAsync(count, 0, sizeof(int32_t), c->stream));
    for (int p0 = 0; p0 < parts; p0 += batch) {
        const int np = std::min(batch, parts - p0);
        pca_partsum_kernel<<<np, 256, mean_lds, c->stream>>>(table, ld, n_table, dim, inv_norm, d_rows, n, p0, (double *)scratch, count);
        GCNHIP_LAUNCH_CHECK();
        pca_meanfold_kernel<<<1, 256, 0, c->stream>>>((const double *)scratch, np, dim, mean);
        GCNHIP_LAUNCH_CHECK();
    }
    pca_meandiv_kernel<<<1, 256, 0, c->stream>>>(dim, count, mean);
    GCNHIP_LAUNCH_CHECK();
    return 0;
}

int gcnhip_pca_scatter(gcnhip_ctx *c, const float *table, int ld, int n_table, int dim, const float *inv_norm, const int32_t *d_rows, int n,
                       const double *mean, double *scatter, void *scratch, size_t scratch_bytes) {
    if (!c || !scatter || !scratch) return gcnhip_fail("gcnhip_pca_scatter: invalid argument");
    if (const char *why = pca_refusal(table, ld, n_table, dim, d_rows, n)) PCA_REFUSE("gcnhip_pca_scatter", why);
    if (!aligned16(scratch)) return gcnhip_fail("gcnhip_pca_scatter: the scratch is not 16-byte aligned");
    const size_t per = pca_part_bytes(dim);
    if (scratch_bytes < per) return gcnhip_fail("gcnhip_pca_scatter: the scratch is below the minimum (gcnhip_pca_plan tells the bytes)");
    const int parts = ceil_div(n, PCA_PART);
    const int batch = (int)std::min<size_t>(scratch_bytes / per, (size_t)std::max(parts, 1));
    const int dpad = (dim + 15) / 16 * 16, nt = dpad / 16, T = nt * (nt + 1) / 2;
    const size_t lds = (size_t)dpad * sizeof(double) + (size_t)PCA_RT * (dpad + 16) * sizeof(float) + PCA_RT * sizeof(int);
    GCNHIP_TRY(hipMemsetAsync(scatter, 0, (size_t)dim * dim * sizeof(double), c->stream));
    for (int p0 = 0; p0 < parts; p0 += batch) {
        const int np = std::min(batch, parts - p0);
        double *partials = (double *)scratch;
        int rc;
        if (nt <= 2) rc = pca_scatter_launch<1>(c, np, lds, table, ld, n_table, dim, inv_norm, d_rows, n, mean, p0, partials);
        else if (nt <= 4) rc = pca_scatter_launch<2>(c, np, lds, table, ld, n_table, dim, inv_norm, d_rows, n, mean, p0, partials);
        else if (nt <= 8) rc = pca_scatter_launch<5>(c, np, lds, table, ld, n_table, dim, inv_norm, d_rows, n, mean, p0, partials);
        else if (nt <= 12) rc = pca_scatter_launch<10>(c, np, lds, table, ld, n_table, dim, inv_norm, d_rows, n, mean, p0, partials);
        else rc = pca_scatter_launch<17>(c, np, lds, table, ld, n_table, dim, inv_norm, d_rows, n, mean, p0, partials);
        if (rc != 0) return rc;
        pca_scatterfold_kernel<<<T, 256, 0, c->stream>>>(partials, np, dim, scatter);
        GCNHIP_LAUNCH_CHECK();
    }
    pca_mirror_kernel<<<ceil_div(dim * dim, 256), 256, 0, c->stream>>>(dim, scatter);
    GCNHIP_LAUNCH_CHECK();
    return 0;
}

int gcnhip_pca_project(gcnhip_ctx *c, const float *table, int ld, int n_table, int dim, const float *inv_norm, const int32_t *d_rows, int n,
                       const double *mean, const double *basis, int ldv, int k, const double *scale, float *out, int ldy) {
    if (!c || !basis || (n > 0 && !out)) return gcnhip_fail("gcnhip_pca_project: invalid argument");
    if (const char *why = pca_refusal(table, ld, n_table, dim, d_rows, n)) PCA_REFUSE("gcnhip_pca_project", why);
    if (k < 1 || k > dim) return gcnhip_fail("gcnhip_pca_project: 1 <= k <= dim");
    if (ldv < k || ldy < k) return gcnhip_fail("gcnhip_pca_project: a row stride is below k");
    if (n == 0) return 0;
    pca_project_kernel<<<ceil_div(n, PCA_PT), 256, 0, c->stream>>>(table, ld, n_table, dim, inv_norm, d_rows, n, mean, basis, ldv, k, scale, out, ldy);
    GCNHIP_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
