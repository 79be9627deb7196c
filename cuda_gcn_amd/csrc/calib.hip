// calib.hip — temperature scaling (Guo et al., 2017) and the reliability diagram, as row-local passes over the log-softmax rows
// a prediction forward leaves on the device (gcnhip_graphsum_predict's logp).  Beyond the reference, which stops at accuracy.
//
// Layout: smooth.hip's — one wave64 per row, lane j on class j (C <= 64: a row is one register), rows of any stride.  With
// l_j = logp[r, j], beta = 1 / T and s_j = beta . l_j:  m = max_j s_j,  e_j = expf(s_j - m),  Z = sum_j e_j,  p_j = e_j / Z.
// Lanes past C hold e = 0 and take part in no maximum.  An entry with p_j == 0 (a column at -1e4) is left out of every sum.
//
// Sums over rows are deterministic: per-row values are f32 and identical on every lane (xor butterflies), a wave adds its rows
// in row order into double accumulators, the four waves of a block are added in a fixed tree, and the block partials (doubles,
// in the upper half of the context's reduction scratch) are added in block order by a one-block finalize launch.  The grid
// depends on the row count (and, for the bins, their number) alone; no float or double atomics anywhere.
#include "common.h"
#include <algorithm>
#include <cstdio>
#pragma clang fp contract(off)

constexpr int CALIB_MAX_BLOCKS = 256;            // x 4 waves x 16 rows: above 16384 rows the grid-stride loop does the rest
constexpr int CALIB_ROWS_PER_BLOCK = 4 * 16;
constexpr int CALIB_PART_FLOATS = 8192;          // the partials start here in red_f: past the loss kernels' [2048, 6144)
constexpr int CALIB_PART_DOUBLES = 4096;         // ... and end with it (RED_SLOTS * 4 floats)
static_assert(CALIB_PART_FLOATS * sizeof(float) + CALIB_PART_DOUBLES * sizeof(double) == RED_SLOTS * 4 * sizeof(float), "scratch layout");
static_assert(CALIB_MAX_BLOCKS * 4 <= CALIB_PART_DOUBLES, "nll partials");

__device__ inline float wave_max(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, WAVE));
    return v;
}

// the softmax of beta . l across the wave: e_j (0 past C), the maximum m of s and Z; every lane gets the same m and Z
struct RowSoftmax { float s, e, m, z; };
__device__ inline RowSoftmax row_softmax(float l, bool live, float beta) {
    RowSoftmax q;
    q.s = beta * l;
    q.m = wave_max(live ? q.s : -INFINITY);
    q.e = live ? expf(q.s - q.m) : 0.f;
    q.z = wave_sum(q.e);
    return q;
}

// row q of the list -> its table row, or -1 (wave-uniform: no id can index past the tables)
__device__ inline int listed_row(const int32_t *rows, int q, int n_table) {
    const int r = rows ? rows[q] : q;
    return r >= 0 && r < n_table ? r : -1;
}

__global__ __launch_bounds__(256) void calib_nll_kernel(const float *__restrict__ logp, int ld, const int32_t *__restrict__ truth, int n_table,
                                                        const int32_t *__restrict__ rows, int n, int C, float beta, double *part) {
    __shared__ double sh[4][4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int waves_total = gridDim.x * 4;
    const bool live = lane < C;
    double a_nll = 0.0, a_g = 0.0, a_h = 0.0, a_n = 0.0;
    for (int q = blockIdx.x * 4 + wave; q < n; q += waves_total) {
        const int r = listed_row(rows, q, n_table);
        if (r < 0) continue;
        const int t = truth[r];
        if (t < 0 || t >= C) continue;
        const float l = live ? logp[(size_t)r * ld + lane] : 0.f;
        const RowSoftmax sm = row_softmax(l, live, beta);
        const float p = sm.e / sm.z;
        const float lt = __shfl(l, t, WAVE);
        const float nll = (logf(sm.z) + sm.m) - beta * lt;
        const float mu = wave_sum(p == 0.f ? 0.f : p * l);
        const float d = l - mu;
        const float h = wave_sum(p == 0.f ? 0.f : p * (d * d));
        a_nll += (double)nll;
        a_g += (double)(mu - lt);
        a_h += (double)h;
        a_n += 1.0;
    }
    if (lane == 0) { sh[wave][0] = a_nll; sh[wave][1] = a_g; sh[wave][2] = a_h; sh[wave][3] = a_n; }
    __syncthreads();
    if (threadIdx.x < 4) part[(size_t)blockIdx.x * 4 + threadIdx.x] = (sh[0][threadIdx.x] + sh[1][threadIdx.x]) + (sh[2][threadIdx.x] + sh[3][threadIdx.x]);
}

// out[k] = the partials of column k in block order, k < width (one thread per column: at most 256 adds each)
__global__ void calib_finalize_kernel(const double *part, int n_blocks, int width, double *out) {
    const int k = threadIdx.x;
    if (blockIdx.x != 0 || k >= width) return;
    double s = 0.0;
    for (int b = 0; b < n_blocks; b++) s += part[(size_t)b * width + k];
    out[k] = s;
}

// lane b of a wave keeps bin b of the rows its wave walks: count, correct and the confidence sum (a double, rows in row order)
__global__ __launch_bounds__(256) void calib_bins_kernel(const float *__restrict__ logp, int ld, const int32_t *__restrict__ truth, int n_table,
                                                         const int32_t *__restrict__ rows, int n, int C, float beta, int bins, int32_t *count,
                                                         int32_t *correct, double *part) {
    __shared__ int hist[2][WAVE];
    __shared__ double sh[4][WAVE];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int waves_total = gridDim.x * 4;
    const bool live = lane < C;
    if (threadIdx.x < 2 * WAVE) hist[threadIdx.x >> 6][lane] = 0;
    __syncthreads();
    int cnt = 0, cor = 0;
    double conf_sum = 0.0;
    for (int q = blockIdx.x * 4 + wave; q < n; q += waves_total) {
        const int r = listed_row(rows, q, n_table);
        if (r < 0) continue;
        const int t = truth[r];
        if (t < 0 || t >= C) continue;
        const float l = live ? logp[(size_t)r * ld + lane] : 0.f;
        const RowSoftmax sm = row_softmax(l, live, beta);
        const float conf = 1.f / sm.z;                         // max_j e_j / Z: the maximum's e is expf(0) = 1
        // the prediction is predict()'s: the largest logit, the lowest column on a tie — whatever beta > 0
        const float lmax = wave_max(live ? l : -INFINITY);
        const int pred = __ffsll((unsigned long long)__ballot(live && l == lmax)) - 1;
        int b = (int)ceilf(conf * (float)bins) - 1;
        b = b < 0 ? 0 : (b > bins - 1 ? bins - 1 : b);
        if (lane == b) {
            cnt += 1;
            cor += pred == t;
            conf_sum += (double)conf;
        }
    }
    sh[wave][lane] = conf_sum;
    if (cnt) atomicAdd(&hist[0][lane], cnt);
    if (cor) atomicAdd(&hist[1][lane], cor);
    __syncthreads();
    if (threadIdx.x < bins) {
        const int b = threadIdx.x;
        part[(size_t)blockIdx.x * bins + b] = (sh[0][b] + sh[1][b]) + (sh[2][b] + sh[3][b]);
        if (hist[0][b]) atomicAdd(&count[b], hist[0][b]);
        if (hist[1][b]) atomicAdd(&correct[b], hist[1][b]);
    }
}

// the whole row sits in the wave's registers before anything is stored: out may be logp
__global__ __launch_bounds__(256) void calib_scale_kernel(const float *logp, int ld, int n_table, const int32_t *__restrict__ rows, int n, int C,
                                                          float beta, float *out, int ld_out, float *prob) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int waves_total = gridDim.x * 4;
    const bool live = lane < C;
    for (int q = blockIdx.x * 4 + wave; q < n; q += waves_total) {
        const int r = listed_row(rows, q, n_table);
        if (r < 0) continue;
        const float l = live ? logp[(size_t)r * ld + lane] : 0.f;
        const RowSoftmax sm = row_softmax(l, live, beta);
        const float o = (sm.s - sm.m) - logf(sm.z);
        const float omax = wave_max(live ? o : -INFINITY);
        if (live) out[(size_t)r * ld_out + lane] = o;
        if (prob && lane == 0) prob[r] = expf(omax);
    }
}

static int calib_blocks(int n, int cap) {
    int blocks = ceil_div(n, CALIB_ROWS_PER_BLOCK);
    if (blocks > cap) blocks = cap;
    return blocks < 1 ? 1 : blocks;
}

// the refusals every entry point shares; NULL: the arguments are fine
static const char *calib_refusal(int n_table, int n, const int32_t *d_rows, int C, int ld, float beta) {
    if (n_table < 0 || n < 0) return "invalid argument";
    if (C < 1 || C > WAVE) return "1 <= num_classes <= 64 (lane j holds class j)";
    if (ld < C) return "a row stride is below num_classes";
    if (!(beta > 0.f) || !(beta <= GCNHIP_BETA_MAX)) return GCNHIP_BETA_REFUSAL;
    if (!d_rows && n > n_table) return "without a row list n is at most n_table";
    return nullptr;
}
#define CALIB_REFUSE(NAME, WHY)                                                   \
    do {                                                                          \
        char msg[160];                                                            \
        snprintf(msg, sizeof msg, "%s: %s", NAME, WHY);                           \
        return gcnhip_fail(msg);                                                  \
    } while (0)

extern "C" {

int gcnhip_calib_nll_rows(gcnhip_ctx *c, const float *logp, int ld, const int32_t *truth, int n_table, const int32_t *d_rows, int n,
                          int num_classes, float beta, double *d_out) {
    if (!c || !logp || !truth || !d_out) return gcnhip_fail("gcnhip_calib_nll_rows: invalid argument");
    if (const char *why = calib_refusal(n_table, n, d_rows, num_classes, ld, beta)) CALIB_REFUSE("gcnhip_calib_nll_rows", why);
    const int blocks = calib_blocks(n, CALIB_MAX_BLOCKS);
    double *part = (double *)(c->red_f + CALIB_PART_FLOATS);
    calib_nll_kernel<<<blocks, 256, 0, c->stream>>>(logp, ld, truth, n_table, d_rows, n, num_classes, beta, part);
    GCNHIP_LAUNCH_CHECK();
    calib_finalize_kernel<<<1, 64, 0, c->stream>>>(part, blocks, 4, d_out);
    GCNHIP_LAUNCH_CHECK();
    return 0;
}

int gcnhip_calib_bins_rows(gcnhip_ctx *c, const float *logp, int ld, const int32_t *truth, int n_table, const int32_t *d_rows, int n,
                           int num_classes, float beta, int bins, int32_t *d_count, int32_t *d_correct, double *d_conf_sum) {
    if (!c || !logp || !truth || !d_count || !d_correct || !d_conf_sum) return gcnhip_fail("gcnhip_calib_bins_rows: invalid argument");
    if (const char *why = calib_refusal(n_table, n, d_rows, num_classes, ld, beta)) CALIB_REFUSE("gcnhip_calib_bins_rows", why);
    if (bins < 1 || bins > WAVE) return gcnhip_fail("gcnhip_calib_bins_rows: 1 <= bins <= 64 (lane b holds bin b)");
    GCNHIP_TRY(hipMemsetAsync(d_count, 0, (size_t)bins * sizeof(int32_t), c->stream));
    GCNHIP_TRY(hipMemsetAsync(d_correct, 0, (size_t)bins * sizeof(int32_t), c->stream));
    const int blocks = calib_blocks(n, std::min(CALIB_MAX_BLOCKS, CALIB_PART_DOUBLES / bins));
    double *part = (double *)(c->red_f + CALIB_PART_FLOATS);
    calib_bins_kernel<<<blocks, 256, 0, c->stream>>>(logp, ld, truth, n_table, d_rows, n, num_classes, beta, bins, d_count, d_correct, part);
    GCNHIP_LAUNCH_CHECK();
    calib_finalize_kernel<<<1, 64, 0, c->stream>>>(part, blocks, bins, d_conf_sum);
    GCNHIP_LAUNCH_CHECK();
    return 0;
}

int gcnhip_calib_scale_rows(gcnhip_ctx *c, const float *logp, int ld, int n_table, const int32_t *d_rows, int n, int num_classes, float beta,
                            float *out_logp, int ld_out, float *d_prob) {
    if (!c || !logp || !out_logp) return gcnhip_fail("gcnhip_calib_scale_rows: invalid argument");
    if (const char *why = calib_refusal(n_table, n, d_rows, num_classes, std::min(ld, ld_out), beta)) CALIB_REFUSE("gcnhip_calib_scale_rows", why);
    if (n == 0) return 0;
    calib_scale_kernel<<<calib_blocks(n, 4 * CALIB_MAX_BLOCKS), 256, 0, c->stream>>>(logp, ld, n_table, d_rows, n, num_classes, beta, out_logp, ld_out, d_prob);
    GCNHIP_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
