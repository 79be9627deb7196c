// report.hip — per-class evaluation counts: the confusion matrix of a single-label model and the TP / FP / FN of every class
// of a multi-label one, formed on the GPU from what the prediction paths already produce (the pred array of
// gcnhip_graphsum_predict; a logit table and the multi-hot truth words of bce.hip).  Beyond the reference, which reports
// one accuracy per split.  Off the epoch path: nothing here is launched by train_epoch / eval.
//
// Every count is an integer and integer addition commutes and associates, so the result depends neither on the order in which
// blocks run nor on the order in which atomics arrive: two launches on the same inputs give identical output.  (The float
// sums of the loss kernels need their fixed block order for that; these do not.)  LDS and global accumulation use atomicAdd
// on int.
#include "common.h"
#include <algorithm>

constexpr int CONF_MAXC = 64;              // the limit of gcnhip_graphsum_predict: C x C ints = 16 KB of LDS at most
constexpr int CONF_ROWS_PER_THREAD = 4;    // independent rows[i] -> pred / truth chains in flight per lane
constexpr int CONF_MAX_BLOCKS = 512;
constexpr int CNT_MAXC_REG = 4;            // 4 x 64 = 256 classes, the limit of gcnhip_bce_fwd_rows
constexpr int CNT_MAX_BLOCKS = 512;

// both outputs of a launch zeroed by one small launch in front of it (a memset per array would be a launch each)
__global__ __launch_bounds__(256) void report_zero_kernel(int32_t *counts, int n, int32_t *extra) {
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) counts[i] = 0;
    if (extra && blockIdx.x == 0 && threadIdx.x == 0) *extra = 0;
}

// One C x C histogram per block in LDS; a block walks a contiguous range of the row list, then adds its non-zero cells to
// the global matrix.  Same-address LDS atomics serialise, and a trained model puts most rows of a large class into ONE cell
// (its diagonal entry): before the per-lane atomics, the lanes that share lane 0's cell are counted with a ballot and added
// by one lane.  On uniform cells that costs a ballot per step; on a dominant cell it replaces up to 64 serialised adds by one.
__global__ __launch_bounds__(256) void confusion_rows_kernel(const int32_t *__restrict__ pred, const int32_t *__restrict__ truth,
                                                             int n_table, const int32_t *__restrict__ rows, int n, int C,
                                                             int rows_per_block, int32_t *counts, int32_t *out_of_range) {
    __shared__ int hist[CONF_MAXC * CONF_MAXC];
    __shared__ int sh_bad;
    const int cells = C * C;
    for (int c = threadIdx.x; c < cells; c += 256) hist[c] = 0;
    if (threadIdx.x == 0) sh_bad = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int64_t begin = (int64_t)blockIdx.x * rows_per_block;
    const int64_t end = begin + rows_per_block < n ? begin + rows_per_block : n;
    int bad = 0;
    // the trip count is the same for every lane of the block (ballots below see whole waves)
    for (int64_t base = begin; base < end; base += 256 * CONF_ROWS_PER_THREAD) {
        int cell[CONF_ROWS_PER_THREAD];
#pragma unroll
        for (int k = 0; k < CONF_ROWS_PER_THREAD; k++) {
            const int64_t i = base + k * 256 + threadIdx.x;
            cell[k] = -2;                                      // -2: no row; -1: a row that is not counted in the matrix
            if (i < end) {
                const int r = rows ? rows[i] : (int)i;
                cell[k] = -1;
                if (r >= 0 && r < n_table) {
                    const int t = truth[r], p = pred[r];
                    if (t >= 0 && t < C && p >= 0 && p < C) cell[k] = t * C + p;
                }
            }
        }
#pragma unroll
        for (int k = 0; k < CONF_ROWS_PER_THREAD; k++) {
            const int mine = cell[k];
            bad += mine == -1;
            const int lead = __builtin_amdgcn_readfirstlane(mine);
            const unsigned long long same = __ballot(mine == lead);
            if (lead >= 0) {
                if (lane == 0) atomicAdd(&hist[lead], (int)__popcll(same));
                if (mine >= 0 && mine != lead) atomicAdd(&hist[mine], 1);
            } else if (mine >= 0) {
                atomicAdd(&hist[mine], 1);
            }
        }
    }
    bad = wave_sum_i(bad);
    if (lane == 0 && bad) atomicAdd(&sh_bad, bad);
    __syncthreads();
    for (int c = threadIdx.x; c < cells; c += 256) {
        const int v = hist[c];
        if (v) atomicAdd(&counts[c], v);
    }
    if (threadIdx.x == 0 && sh_bad) atomicAdd(out_of_range, sh_bad);
}

// bce.hip's layout: one wave64 per listed row, lane j on classes j, j + 64, j + 128, j + 192.  A lane keeps TP / FP / FN of its
// (up to) four classes in registers over all the rows its wave walks; the four waves of a block add them in LDS, and one
// atomic per class, count and block goes to global memory.  The next row is loaded while this one is counted.
__global__ __launch_bounds__(256) void bce_class_counts_kernel(const float *__restrict__ logits, int ld, const uint32_t *__restrict__ truth,
                                                               int wpr, const int32_t *__restrict__ rows, int n, int C, int32_t *counts) {
    __shared__ int sh[3 * CNT_MAXC_REG * WAVE];
    for (int c = threadIdx.x; c < 3 * CNT_MAXC_REG * WAVE; c += 256) sh[c] = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int waves_total = gridDim.x * 4;
    int tp[CNT_MAXC_REG] = {}, fp[CNT_MAXC_REG] = {}, fn[CNT_MAXC_REG] = {};
    float nv[CNT_MAXC_REG];
    uint32_t nw[CNT_MAXC_REG];
    auto prefetch = [&](int q) {
        const int r = rows ? rows[q] : q;
        const float *lg = logits + (size_t)r * ld;
        const uint32_t *tw = truth + (size_t)r * wpr;
#pragma unroll
        for (int k = 0; k < CNT_MAXC_REG; k++) {
            const int j = lane + k * WAVE;
            nv[k] = j < C ? lg[j] : 0.f;
            nw[k] = j < C ? tw[j >> 5] : 0u;
        }
    };
    int q = blockIdx.x * 4 + wave;
    if (q < n) prefetch(q);
    for (; q < n; q += waves_total) {
        float v[CNT_MAXC_REG];
        uint32_t w[CNT_MAXC_REG];
#pragma unroll
        for (int k = 0; k < CNT_MAXC_REG; k++) { v[k] = nv[k]; w[k] = nw[k]; }
        if (q + waves_total < n) prefetch(q + waves_total);
#pragma unroll
        for (int k = 0; k < CNT_MAXC_REG; k++) {
            const int j = lane + k * WAVE;
            if (j >= C) continue;
            const bool y = (w[k] >> (j & 31)) & 1u;
            const bool pos = v[k] > 0.f;                       // the rule of bce_fwd_kernel and bce_predict_kernel
            tp[k] += pos && y;
            fp[k] += pos && !y;
            fn[k] += !pos && y;
        }
    }
#pragma unroll
    for (int k = 0; k < CNT_MAXC_REG; k++) {
        const int j = lane + k * WAVE;
        if (j >= C) continue;
        if (tp[k]) atomicAdd(&sh[j], tp[k]);
        if (fp[k]) atomicAdd(&sh[CNT_MAXC_REG * WAVE + j], fp[k]);
        if (fn[k]) atomicAdd(&sh[2 * CNT_MAXC_REG * WAVE + j], fn[k]);
    }
    __syncthreads();
    for (int c = threadIdx.x; c < 3 * CNT_MAXC_REG * WAVE; c += 256) {
        const int which = c / (CNT_MAXC_REG * WAVE), j = c % (CNT_MAXC_REG * WAVE);
        const int v = sh[c];
        if (j < C && v) atomicAdd(&counts[which * C + j], v);
    }
}

extern "C" {

int gcnhip_confusion_rows(gcnhip_ctx *c, const int32_t *pred, const int32_t *truth, int n_table, const int32_t *d_rows, int n,
                          int num_classes, int32_t *counts, int32_t *out_of_range) {
    if (!c || !pred || !truth || !counts || !out_of_range || n_table < 0 || n < 0 || num_classes < 1) return -1;
    if (num_classes > CONF_MAXC) return gcnhip_fail("gcnhip_confusion_rows: at most 64 classes (the limit of gcnhip_graphsum_predict; the block's matrix sits in LDS)");
    if (!d_rows && n > n_table) return -1;
    const int cells = num_classes * num_classes;
    report_zero_kernel<<<ceil_div(cells, 256), 256, 0, c->stream>>>(counts, cells, out_of_range);
    GCNHIP_LAUNCH_CHECK();
    if (n == 0) return 0;
    // a block's flush costs up to C x C global atomics: give it at least as many rows
    const int step = 256 * CONF_ROWS_PER_THREAD;
    int rows_per_block = std::max(step, cells);
    rows_per_block = std::max(rows_per_block, ceil_div(n, CONF_MAX_BLOCKS));
    rows_per_block = ceil_div(rows_per_block, step) * step;
    const int blocks = ceil_div(n, rows_per_block);
    confusion_rows_kernel<<<blocks, 256, 0, c->stream>>>(pred, truth, n_table, d_rows, n, num_classes, rows_per_block, counts, out_of_range);
    GCNHIP_LAUNCH_CHECK();
    return 0;
}

int gcnhip_bce_class_counts_rows(gcnhip_ctx *c, const float *logits, int ld, const uint32_t *truth_bits, int words_per_row,
                                 const int32_t *d_rows, int n, int num_classes, int32_t *counts) {
    if (!c || !logits || !truth_bits || !counts || n < 0 || num_classes < 1 || ld < num_classes) return -1;
    if (num_classes > CNT_MAXC_REG * WAVE) return gcnhip_fail("gcnhip_bce_class_counts_rows: at most 256 classes (the limit of gcnhip_bce_fwd_rows)");
    if (words_per_row < (num_classes + 31) / 32) return -1;
    report_zero_kernel<<<ceil_div(3 * num_classes, 256), 256, 0, c->stream>>>(counts, 3 * num_classes, nullptr);
    GCNHIP_LAUNCH_CHECK();
    if (n == 0) return 0;
    int blocks = ceil_div(n, 4 * 16);                      // ~16 rows per wave; the cap decides on large inputs
    if (blocks > CNT_MAX_BLOCKS) blocks = CNT_MAX_BLOCKS;
    bce_class_counts_kernel<<<blocks, 256, 0, c->stream>>>(logits, ld, truth_bits, words_per_row, d_rows, n, num_classes, counts);
    GCNHIP_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
