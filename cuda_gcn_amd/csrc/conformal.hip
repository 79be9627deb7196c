// conformal.hip — split conformal prediction (Vovk et al.; LAC: Sadinle et al., 2019; APS / RAPS: Romano et al., 2020,
// Angelopoulos et al., 2021) as row-local passes over the log-softmax rows a prediction forward leaves on the device.  Beyond
// the reference, which stops at accuracy.
//
// Layout: calib.hip's — one wave64 per row, lane j on class j (C <= 64: a row is one register), rows of any stride.  With
// l_j = logp[r, j], beta = 1 / T and s_j = beta . l_j:  m = max_j s_j,  e_j = expf(s_j - m),  Z = sum_j e_j,  p_j = e_j / Z.
//
// Rank.  rank_j = #{k : l_k > l_j, or l_k == l_j and k < j}: taken on the f32 INPUTS, so the order is exact, never depends on a
// rounding of p, and ties go to the lower class as in predict().  It is a permutation of 0 .. C - 1 on every row without a NaN.
//
// Scores of class j:  LAC  1 - p_j;  APS  cum_j + lam . max(0, rank_j + 1 - k_reg)  with cum_j = sum of p_k over rank_k <= rank_j.
// cum: the p's are sent to the lane of their rank (one cross-lane permute), an inclusive Kogge-Stone scan adds them in one fixed
// tree — every result went through at most six additions, whatever C —, and each class reads the entry of its rank.  cum is
// clamped to 1 (the real sum never exceeds it), and the last-ranked class gets exactly 1.0f: a threshold at or above 1 gives the
// full set on every row instead of depending on the last ulp of sum p.
//
// Nothing here adds floats across rows; the counts of the sets launch are integers (report.hip's argument: integer adds commute),
// so two launches give the same bits.  No launch allocates or synchronises.
#include "common.h"
#include <algorithm>
#include <cstdio>
#pragma clang fp contract(off)

// Grids.  A row is one dependent chain (load, expf, butterflies, the rank loop), so a wave alone on its SIMD waits out every
// latency: the scores launch gives a wave two rows and fills the device (2048 blocks: 8 waves per SIMD on 256 CUs) before the
// grid-stride loop takes over; the sets launch flushes up to 4 + 3 C + 1 counts per block, so it keeps blocks fewer and rows per
// wave more.  Every cap is reached at 16384 rows, the calibration kernels' figure.
constexpr int CONFORMAL_SCORES_MAX_BLOCKS = 2048, CONFORMAL_SCORES_ROWS_PER_BLOCK = 4 * 2;
constexpr int CONFORMAL_SETS_MAX_BLOCKS = 512, CONFORMAL_SETS_ROWS_PER_BLOCK = 4 * 8;
constexpr int CONFORMAL_TRUE_MAX_BLOCKS = 64;     // one thread per list position: a gather of n floats, the same 16384
constexpr int CONFORMAL_COUNTS_MAX = 4 + 3 * WAVE + 1;

namespace {

__device__ inline float cf_wave_max(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, WAVE));
    return v;
}

// row q of the list -> its table row, or -1 (wave-uniform: no id can index past the tables)
__device__ inline int cf_listed_row(const int32_t *rows, int q, int n_table) {
    const int r = rows ? rows[q] : q;
    return r >= 0 && r < n_table ? r : -1;
}

// the rank of this lane's class among the C live lanes (lanes past C: their own lane, so that the ranks stay a permutation)
__device__ inline int cf_rank(float l, int lane, int C) {
    int rank = 0;
    for (int k = 0; k < C; k++) {
        const float lk = __shfl(l, k, WAVE);
        rank += (lk > l) || (lk == l && k < lane);
    }
    return lane < C ? rank : lane;
}

}  // namespace

__global__ __launch_bounds__(256) void conformal_scores_kernel(const float *__restrict__ logp, int ld, int n_table, const int32_t *__restrict__ rows,
                                                               int n, int C, float beta, int method, float lam, int k_reg, float *__restrict__ out,
                                                               int ld_out) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int waves_total = gridDim.x * 4;
    const bool live = lane < C;
    for (int q = blockIdx.x * 4 + wave; q < n; q += waves_total) {
        const int r = cf_listed_row(rows, q, n_table);
        if (r < 0) continue;
        const float l = live ? logp[(size_t)r * ld + lane] : 0.f;
        const float s = beta * l;
        const float m = cf_wave_max(live ? s : -INFINITY);
        const float e = live ? expf(s - m) : 0.f;
        const float z = wave_sum(e);
        const float p = e / z;
        float score;
        if (method == 0) {
            score = 1.f - p;
        } else {
            const int rank = cf_rank(l, lane, C);              // < 64 on every lane, NaN rows included: the permutes stay inside the wave
            // lane i <- the p of rank i (a push: each lane names its destination)
            float v = __int_as_float(__builtin_amdgcn_ds_permute(rank << 2, __float_as_int(p)));
#pragma unroll
            for (int off = 1; off < WAVE; off <<= 1) {
                const float t = __shfl_up(v, off, WAVE);
                if (lane >= off) v += t;
            }
            float cum = __shfl(v, rank, WAVE);
            cum = fminf(cum, 1.f);
            if (rank == C - 1) cum = 1.f;
            const int over = rank + 1 - k_reg;
            const float pen = lam * (float)(over > 0 ? over : 0);
            score = cum + pen;
        }
        if (live) out[(size_t)r * ld_out + lane] = score;
    }
}

// one thread per list position
__global__ __launch_bounds__(256) void conformal_true_scores_kernel(const float *__restrict__ table, int ld, const int32_t *__restrict__ truth,
                                                                    int n_table, const int32_t *__restrict__ rows, int n, int C,
                                                                    float *__restrict__ score) {
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
        const int r = rows ? rows[i] : i;
        float v = -1.f;
        if (r >= 0 && r < n_table) {
            const int t = truth[r];
            if (t >= 0 && t < C) v = table[(size_t)r * ld + t];
        }
        score[i] = v;
    }
}

// A lane keeps the counts of its class (support, covered) and of the set size equal to its lane over the rows its wave walks;
// the wave-uniform counts sit in lane-uniform registers.  The four waves add into the block's LDS copy, and the block adds its
// non-zero cells to global memory: integer adds all the way.
__global__ __launch_bounds__(256) void conformal_sets_kernel(const float *__restrict__ table, int ld, int n_table, const int32_t *__restrict__ rows,
                                                             int n, int C, const float *__restrict__ thresh, const int32_t *__restrict__ truth,
                                                             uint32_t *__restrict__ bits, int32_t *__restrict__ size, int32_t *counts) {
    __shared__ int sh[CONFORMAL_COUNTS_MAX];
    const int cells = 4 + 3 * C + 1;
    if (counts) {
        for (int c = threadIdx.x; c < cells; c += 256) sh[c] = 0;
        __syncthreads();
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int waves_total = gridDim.x * 4;
    const bool live = lane < C;
    const int wpr = (C + 31) >> 5;
    const float th = live ? thresh[lane] : 0.f;
    int in_table = 0, labelled = 0, covered = 0, empty = 0, full64 = 0;
    int hist = 0, support = 0, class_cov = 0;
    for (int q = blockIdx.x * 4 + wave; q < n; q += waves_total) {
        const int r = cf_listed_row(rows, q, n_table);
        if (r < 0) {
            if (lane < wpr && bits) bits[(size_t)q * wpr + lane] = 0u;
            if (lane == 0 && size) size[q] = -1;
            continue;
        }
        const float s = live ? table[(size_t)r * ld + lane] : 0.f;
        const unsigned long long mask = __ballot(live && s <= th);
        const int sz = (int)__popcll(mask);
        if (lane < wpr && bits) bits[(size_t)q * wpr + lane] = (uint32_t)(mask >> (32 * lane));
        if (lane == 0 && size) size[q] = sz;
        if (counts) {
            in_table++;
            empty += sz == 0;
            hist += sz == lane;
            full64 += sz == WAVE;
            const int t = truth ? truth[r] : -1;
            if (t >= 0 && t < C) {
                const int hit = (int)((mask >> t) & 1ull);
                labelled++;
                covered += hit;
                support += t == lane;
                class_cov += t == lane && hit;
            }
        }
    }
    if (!counts) return;
    if (lane == 0) {
        if (in_table) atomicAdd(&sh[0], in_table);
        if (labelled) atomicAdd(&sh[1], labelled);
        if (covered) atomicAdd(&sh[2], covered);
        if (empty) atomicAdd(&sh[3], empty);
        if (full64 && C == WAVE) atomicAdd(&sh[4 + WAVE], full64);
    }
    if (lane <= C && hist) atomicAdd(&sh[4 + lane], hist);     // lane 63 at most: size 64 is full64's
    if (live && support) atomicAdd(&sh[4 + C + 1 + lane], support);
    if (live && class_cov) atomicAdd(&sh[4 + 2 * C + 1 + lane], class_cov);
    __syncthreads();
    for (int c = threadIdx.x; c < cells; c += 256) {
        const int v = sh[c];
        if (v) atomicAdd(&counts[c], v);
    }
}

static int conformal_blocks(int n, int rows_per_block, int cap) {
    int blocks = ceil_div(n, rows_per_block);
    if (blocks > cap) blocks = cap;
    return blocks < 1 ? 1 : blocks;
}

// the refusals every entry point shares; NULL: the arguments are fine
static const char *conformal_refusal(int n_table, int n, const int32_t *d_rows, int C, int ld) {
    if (n_table < 0 || n < 0) return "invalid argument";
    if (C < 1 || C > WAVE) return "1 <= num_classes <= 64 (lane j holds class j)";
    if (ld < C) return "a row stride is below num_classes";
    if (!d_rows && n > n_table) return "without a row list n is at most n_table";
    return nullptr;
}
#define CONFORMAL_REFUSE(NAME, WHY)                                               \
    do {                                                                          \
        char msg[160];                                                            \
        snprintf(msg, sizeof msg, "%s: %s", NAME, WHY);                           \
        return gcnhip_fail(msg);                                                  \
    } while (0)

extern "C" {

int gcnhip_conformal_scores(gcnhip_ctx *c, const float *logp, int ld, int n_table, const int32_t *d_rows, int n, int num_classes, float beta,
                            int method, float lam, int k_reg, float *out, int ld_out) {
    if (!c || !logp || !out) return gcnhip_fail("gcnhip_conformal_scores: invalid argument");
    if (const char *why = conformal_refusal(n_table, n, d_rows, num_classes, std::min(ld, ld_out))) CONFORMAL_REFUSE("gcnhip_conformal_scores", why);
    if (!(beta > 0.f) || !(beta <= GCNHIP_BETA_MAX)) CONFORMAL_REFUSE("gcnhip_conformal_scores", GCNHIP_BETA_REFUSAL);
    if (method != 0 && method != 1) return gcnhip_fail("gcnhip_conformal_scores: method is 0 (lac) or 1 (aps)");
    if (!(lam >= 0.f) || !(lam <= 3.402823466e38f)) return gcnhip_fail("gcnhip_conformal_scores: lam must be finite and >= 0");
    if (k_reg < 0) return gcnhip_fail("gcnhip_conformal_scores: k_reg must be >= 0");
    if (out == logp) return gcnhip_fail("gcnhip_conformal_scores: out must not be logp");
    if (n == 0) return 0;
    const int blocks = conformal_blocks(n, CONFORMAL_SCORES_ROWS_PER_BLOCK, CONFORMAL_SCORES_MAX_BLOCKS);
    conformal_scores_kernel<<<blocks, 256, 0, c->stream>>>(logp, ld, n_table, d_rows, n, num_classes, beta, method, lam, k_reg, out, ld_out);
    GCNHIP_LAUNCH_CHECK();
    return 0;
}

int gcnhip_conformal_true_scores(gcnhip_ctx *c, const float *table, int ld, const int32_t *truth, int n_table, const int32_t *d_rows, int n,
                                 int num_classes, float *d_score) {
    if (!c || !table || !truth || !d_score) return gcnhip_fail("gcnhip_conformal_true_scores: invalid argument");
    if (const char *why = conformal_refusal(n_table, n, d_rows, num_classes, ld)) CONFORMAL_REFUSE("gcnhip_conformal_true_scores", why);
    if (n == 0) return 0;
    const int blocks = std::min(ceil_div(n, 256), CONFORMAL_TRUE_MAX_BLOCKS);
    conformal_true_scores_kernel<<<blocks, 256, 0, c->stream>>>(table, ld, truth, n_table, d_rows, n, num_classes, d_score);
    GCNHIP_LAUNCH_CHECK();
    return 0;
}

int gcnhip_conformal_sets_rows(gcnhip_ctx *c, const float *table, int ld, int n_table, const int32_t *d_rows, int n, int num_classes,
                               const float *d_thresh, const int32_t *truth, uint32_t *d_bits, int32_t *d_size, int32_t *d_counts) {
    if (!c || !table || !d_thresh) return gcnhip_fail("gcnhip_conformal_sets_rows: invalid argument");
    if (const char *why = conformal_refusal(n_table, n, d_rows, num_classes, ld)) CONFORMAL_REFUSE("gcnhip_conformal_sets_rows", why);
    if (d_counts) GCNHIP_TRY(hipMemsetAsync(d_counts, 0, (size_t)(4 + 3 * num_classes + 1) * sizeof(int32_t), c->stream));
    if (n == 0 || (!d_bits && !d_size && !d_counts)) return 0;
    const int blocks = conformal_blocks(n, CONFORMAL_SETS_ROWS_PER_BLOCK, CONFORMAL_SETS_MAX_BLOCKS);
    conformal_sets_kernel<<<blocks, 256, 0, c->stream>>>(table, ld, n_table, d_rows, n, num_classes, d_thresh, truth, d_bits, d_size, d_counts);
    GCNHIP_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
