// wloss.hip — class-weighted losses over a list of rows (beyond the reference, whose loss weighs every row equally):
//   gcnhip_wxent_fwd_rows  softmax cross-entropy with a weight per class, w[truth] of the row scaling its term and its
//                          gradient row; the mean is the weighted one (sum of w . term / sum of w), accuracy is not weighted;
//   gcnhip_wbce_fwd_rows   per-class sigmoid cross-entropy with a weight per class on the positive term (pos_weight).
//
// Layouts are those of the unweighted kernels (xent.hip, bce.hip), which this file does not touch: a lane per row for
// C <= 64 with whole aligned float4 rows, else a wave per row up to 256 classes; same grids, same lane -> row assignment,
// same order of additions — with every weight 1.0f gcnhip_wxent_fwd_rows returns the bits of gcnhip_xent_fwd_rows_scaled
// (a multiplication by 1.0f is exact).  The weight table (at most 1 KB) is a gather w[t] per row (single-label) or four
// registers per lane loaded once (multi-label): no LDS.  Block partials are added in block order by a one-block finalize
// launch (the form of bce.hip), which also writes an armed metrics-ring row: two calls give the same bits.  Plain C++.
#include "common.h"
#include <stdlib.h>
#pragma clang fp contract(off)

constexpr int WL_MAXC_REG = 4;           // 4 x 64 = 256 classes in registers
constexpr int WX_MAX_BLOCKS = 2048;      // part_i holds 2 ints per block: red_i[0, 4096)
constexpr int WB_MAX_BLOCKS = 1024;      // part_i holds 3 ints per block: red_i[0, 3072)

struct WxArgs {
    float *logits;
    float *grad;
    const int32_t *truth;
    const int32_t *rows;
    const float *grad_row_scale;
    const float *weight;        // [C]
    float weight_sum;           // sum of w[truth] over the scored split's rows of all ranks: the gradient's divisor
    int ld, ld_grad, n_rows, C;
    int training, shift;
    float *part_f;              // [blocks] sum of w . term
    float *part_w;              // [blocks] sum of w
    int32_t *part_i;            // [blocks * 2] {correct, total}
};

// the ring row of gcnhip_metrics_record (elementwise.hip), written by the finalize launches below when one is armed
struct WlRing {
    float *ring; int capacity, slot; const uint32_t *epoch; const float *sumsq;
};

__device__ inline void wl_ring_row(const WlRing &g, const float r[4]) {
    if (!g.ring) return;
    const uint32_t e = g.epoch ? *g.epoch : 0u;
    float *row = g.ring + ((size_t)(e % (uint32_t)g.capacity) * 4 + g.slot) * 8;
    row[0] = r[0]; row[1] = r[1]; row[2] = r[2]; row[3] = r[3];
    row[4] = g.sumsq ? *g.sumsq : 0.f;
    row[5] = (float)e; row[6] = 0.f; row[7] = 0.f;
}

__device__ inline float wl_wave_max(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, WAVE));
    return v;
}

// thread 0 stores the block's totals for wxent_finalize_kernel
__device__ inline void wx_block_partials(const WxArgs &a, float loss, float ws, int correct, int total) {
    __shared__ float sh_f[4], sh_w[4];
    __shared__ int sh_i[8];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) { sh_f[wave] = loss; sh_w[wave] = ws; sh_i[wave * 2] = correct; sh_i[wave * 2 + 1] = total; }
    __syncthreads();
    if (threadIdx.x == 0) {
        a.part_f[blockIdx.x] = (sh_f[0] + sh_f[1]) + (sh_f[2] + sh_f[3]);
        a.part_w[blockIdx.x] = (sh_w[0] + sh_w[1]) + (sh_w[2] + sh_w[3]);
        a.part_i[blockIdx.x * 2] = sh_i[0] + sh_i[2] + sh_i[4] + sh_i[6];
        a.part_i[blockIdx.x * 2 + 1] = sh_i[1] + sh_i[3] + sh_i[5] + sh_i[7];
    }
}

// one wave per row (xent_kernel's walk): lane j holds logits j, j + 64, j + 128, j + 192
__global__ __launch_bounds__(256) void wxent_kernel(WxArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int waves_total = gridDim.x * 4;
    const int rows_per_wave = (a.n_rows + waves_total - 1) / waves_total;
    const int gw = blockIdx.x * 4 + wave;
    const int r0 = gw * rows_per_wave, r1 = min(a.n_rows, r0 + rows_per_wave);
    float loss = 0.f, ws = 0.f;
    int correct = 0, total = 0;
    float nv[WL_MAXC_REG];
    int nt = -1;
    auto prefetch = [&](int q) {
        const int r = a.rows ? a.rows[q] : q;
        nt = a.truth[r];
        const float *lg = a.logits + (size_t)r * a.ld;
#pragma unroll
        for (int k = 0; k < WL_MAXC_REG; k++) {
            const int j = lane + k * WAVE;
            nv[k] = j < a.C ? lg[j] : -INFINITY;
        }
    };
    if (r0 < r1) prefetch(r0);
    for (int q = r0; q < r1; q++) {
        const int r = a.rows ? a.rows[q] : q;
        const int t = nt;
        float v[WL_MAXC_REG];
#pragma unroll
        for (int k = 0; k < WL_MAXC_REG; k++) v[k] = nv[k];
        if (q + 1 < r1) prefetch(q + 1);
        float *lg = a.logits + (size_t)r * a.ld;
        float *gr = a.grad ? a.grad + (size_t)r * a.ld_grad : nullptr;
        if (t < 0 || t >= a.C) {                       // no class, no weight: the row's gradient is zero and nothing is counted
            if (a.training && gr)
                for (int j = lane; j < a.C; j += WAVE) gr[j] = 0.f;
            continue;
        }
        const float w = a.weight[t];
        total++;
        float mx = -1e30f;
#pragma unroll
        for (int k = 0; k < WL_MAXC_REG; k++) {
            const int j = lane + k * WAVE;
            if (j < a.C) mx = fmaxf(mx, v[k]);
        }
        mx = wl_wave_max(mx);
        float tv = -INFINITY;
#pragma unroll
        for (int k = 0; k < WL_MAXC_REG; k++)
            if (t / WAVE == k) tv = __shfl(v[k], t % WAVE, WAVE);
        if (!(mx > tv)) correct++;                     // accuracy is not weighted
        float se = 0.f;
        float ex[WL_MAXC_REG];
#pragma unroll
        for (int k = 0; k < WL_MAXC_REG; k++) {
            const int j = lane + k * WAVE;
            v[k] -= mx;
            ex[k] = j < a.C ? expf(v[k]) : 0.f;
            se += ex[k];
            if (a.shift && j < a.C) lg[j] = v[k];
        }
        se = wave_sum(se);
        loss += w * (logf(se) - (tv - mx));
        ws += w;
        if (a.training && gr) {
#pragma unroll
            for (int k = 0; k < WL_MAXC_REG; k++) {
                const int j = lane + k * WAVE;
                if (j < a.C) {
                    float p = ex[k] / se;
                    if (j == t) p = (float)((double)p - 1.0);
                    const float g = (w * p) / a.weight_sum;
                    gr[j] = a.grad_row_scale ? g * a.grad_row_scale[r] : g;
                }
            }
        }
    }
    wx_block_partials(a, loss, ws, correct, total);
}

// one lane per row (xent_lane_kernel's walk): C <= 64, rows of whole aligned float4 pieces
template <int NV4>
__global__ __launch_bounds__(256) void wxent_lane_kernel(WxArgs a) {
    float loss = 0.f, ws = 0.f;
    int correct = 0, total = 0;
    for (int q = blockIdx.x * 256 + threadIdx.x; q < a.n_rows; q += gridDim.x * 256) {
        const int r = a.rows ? a.rows[q] : q;
        const int t = a.truth[r];
        float *lg = a.logits + (size_t)r * a.ld;
        float *gr = a.grad ? a.grad + (size_t)r * a.ld_grad : nullptr;
        if (t < 0 || t >= a.C) {
            if (a.training && gr)
#pragma unroll
                for (int k = 0; k < NV4; k++) reinterpret_cast<float4 *>(gr)[k] = make_float4(0.f, 0.f, 0.f, 0.f);
            continue;
        }
        const float w = a.weight[t];                   // a gather into a table of at most 256 bytes here: it stays in cache
        float v[4 * NV4];
#pragma unroll
        for (int k = 0; k < NV4; k++) {
            const float4 x = reinterpret_cast<const float4 *>(lg)[k];
            v[4 * k] = x.x; v[4 * k + 1] = x.y; v[4 * k + 2] = x.z; v[4 * k + 3] = x.w;
        }
        total++;
        float mx = -1e30f, tv = -INFINITY;
#pragma unroll
        for (int j = 0; j < 4 * NV4; j++) {
            if (j < a.C) mx = fmaxf(mx, v[j]);
            tv = j == t ? v[j] : tv;
        }
        if (!(mx > tv)) correct++;
        float se = 0.f;
#pragma unroll
        for (int j = 0; j < 4 * NV4; j++) {
            v[j] -= mx;
            if (a.shift && j < a.C) lg[j] = v[j];
            v[j] = j < a.C ? expf(v[j]) : 0.f;
            se += v[j];                                // left to right
        }
        loss += w * (logf(se) - (tv - mx));
        ws += w;
        if (a.training && gr) {
            const float gs = a.grad_row_scale ? a.grad_row_scale[r] : 1.f;
#pragma unroll
            for (int j = 0; j < 4 * NV4; j++) {
                float p = v[j] / se;
                if (j == t) p = (float)((double)p - 1.0);
                const float g = (w * p) / a.weight_sum;
                v[j] = j < a.C ? (a.grad_row_scale ? g * gs : g) : 0.f;      // the padding columns stay zero
            }
#pragma unroll
            for (int k = 0; k < NV4; k++)
                reinterpret_cast<float4 *>(gr)[k] = make_float4(v[4 * k], v[4 * k + 1], v[4 * k + 2], v[4 * k + 3]);
        }
    }
    loss = wave_sum(loss); ws = wave_sum(ws); correct = wave_sum_i(correct); total = wave_sum_i(total);
    wx_block_partials(a, loss, ws, correct, total);
}

// fixed-order sum of the block partials (xent_finalize_kernel's order); d_result = {sum w . term, sum w, correct, total}
__global__ __launch_bounds__(256) void wxent_finalize_kernel(const float *part_f, const float *part_w, const int32_t *part_i, int n,
                                                             float *res, int32_t *res_i, WlRing ring) {
    __shared__ float shf[4], shw[4];
    __shared__ int shi[8];
    float l = 0.f, w = 0.f;
    int c = 0, t = 0;
    for (int i = threadIdx.x; i < n; i += 256) { l += part_f[i]; w += part_w[i]; c += part_i[2 * i]; t += part_i[2 * i + 1]; }
    l = wave_sum(l); w = wave_sum(w); c = wave_sum_i(c); t = wave_sum_i(t);
    const int wv = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { shf[wv] = l; shw[wv] = w; shi[2 * wv] = c; shi[2 * wv + 1] = t; }
    __syncthreads();
    if (threadIdx.x != 0) return;
    const int cc = shi[0] + shi[2] + shi[4] + shi[6], tt = shi[1] + shi[3] + shi[5] + shi[7];
    const float r[4] = {(shf[0] + shf[1]) + (shf[2] + shf[3]), (shw[0] + shw[1]) + (shw[2] + shw[3]), (float)cc, (float)tt};
    if (res_i) { res_i[0] = cc; res_i[1] = tt; }
    res[0] = r[0]; res[1] = r[1]; res[2] = r[2]; res[3] = r[3];
    wl_ring_row(ring, r);
}

// ---- multi-label: bce_fwd_kernel's layout (a wave per listed row, lane j on classes j, j + 64, ...), the positive term and
// the positive gradient multiplied by the class's weight, which a lane holds in registers for the whole launch
struct WbArgs {
    const float *logits;
    float *grad;
    const uint32_t *truth;
    const int32_t *rows;
    const float *grad_row_scale;
    const float *pos_weight;    // [C]
    int ld, ld_grad, wpr, n_rows, C;
    float denom;                // count * C
    float *part_f;
    int32_t *part_i;            // [blocks * 3] {TP, FP, FN}
};

__device__ inline float wb_sigmoid(float z) {
    if (z >= 0.f) return 1.f / (1.f + expf(-z));
    const float e = expf(z);
    return e / (1.f + e);
}

__global__ __launch_bounds__(256) void wbce_fwd_kernel(WbArgs a) {
    __shared__ float sh_f[4];
    __shared__ int sh_i[12];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int waves_total = gridDim.x * 4;
    float loss = 0.f;
    int tp = 0, fp = 0, fn = 0;
    float pw[WL_MAXC_REG];
#pragma unroll
    for (int k = 0; k < WL_MAXC_REG; k++) {
        const int j = lane + k * WAVE;
        pw[k] = j < a.C ? a.pos_weight[j] : 0.f;
    }
    float nv[WL_MAXC_REG];
    uint32_t nw[WL_MAXC_REG];
    auto prefetch = [&](int q) {
        const int r = a.rows ? a.rows[q] : q;
        const float *lg = a.logits + (size_t)r * a.ld;
        const uint32_t *tw = a.truth + (size_t)r * a.wpr;
#pragma unroll
        for (int k = 0; k < WL_MAXC_REG; k++) {
            const int j = lane + k * WAVE;
            nv[k] = j < a.C ? lg[j] : 0.f;
            nw[k] = j < a.C ? tw[j >> 5] : 0u;
        }
    };
    int q = blockIdx.x * 4 + wave;
    if (q < a.n_rows) prefetch(q);
    for (; q < a.n_rows; q += waves_total) {
        const int r = a.rows ? a.rows[q] : q;
        float v[WL_MAXC_REG];
        uint32_t w[WL_MAXC_REG];
#pragma unroll
        for (int k = 0; k < WL_MAXC_REG; k++) { v[k] = nv[k]; w[k] = nw[k]; }
        if (q + waves_total < a.n_rows) prefetch(q + waves_total);
        float *gr = a.grad ? a.grad + (size_t)r * a.ld_grad : nullptr;
        const float gs = a.grad_row_scale && gr ? a.grad_row_scale[r] : 1.f;
#pragma unroll
        for (int k = 0; k < WL_MAXC_REG; k++) {
            const int j = lane + k * WAVE;
            if (j >= a.C) continue;
            const float z = v[k];
            const bool y = (w[k] >> (j & 31)) & 1u;
            // pw . y . softplus(-z) + (1 - y) . softplus(z), softplus(x) = max(x, 0) + log1p(exp(-|x|)): finite for every finite z
            const float l1p = log1pf(expf(-fabsf(z)));
            loss += y ? pw[k] * (fmaxf(-z, 0.f) + l1p) : fmaxf(z, 0.f) + l1p;
            const bool pos = z > 0.f;
            tp += pos && y;
            fp += pos && !y;
            fn += !pos && y;
            if (gr) {
                const float g = (y ? -(pw[k] * wb_sigmoid(-z)) : wb_sigmoid(z)) / a.denom;   // no cancellation (bce.hip)
                gr[j] = a.grad_row_scale ? g * gs : g;
            }
        }
    }
    loss = wave_sum(loss); tp = wave_sum_i(tp); fp = wave_sum_i(fp); fn = wave_sum_i(fn);
    if (lane == 0) { sh_f[wave] = loss; sh_i[wave * 3] = tp; sh_i[wave * 3 + 1] = fp; sh_i[wave * 3 + 2] = fn; }
    __syncthreads();
    if (threadIdx.x == 0) {
        a.part_f[blockIdx.x] = (sh_f[0] + sh_f[1]) + (sh_f[2] + sh_f[3]);
#pragma unroll
        for (int k = 0; k < 3; k++) a.part_i[blockIdx.x * 3 + k] = sh_i[k] + sh_i[3 + k] + sh_i[6 + k] + sh_i[9 + k];
    }
}

// d_result = {loss_sum, n_rows * C, 2 TP, 2 TP + FP + FN}, d_result_i = {TP, FP, FN, n_rows}: bce_finalize_kernel's
__global__ __launch_bounds__(256) void wbce_finalize_kernel(const float *part_f, const int32_t *part_i, int n, int n_rows, int C,
                                                            float *res, int32_t *res_i, WlRing ring) {
    __shared__ float shf[4];
    __shared__ int shi[12];
    float l = 0.f;
    int tp = 0, fp = 0, fn = 0;
    for (int i = threadIdx.x; i < n; i += 256) { l += part_f[i]; tp += part_i[3 * i]; fp += part_i[3 * i + 1]; fn += part_i[3 * i + 2]; }
    l = wave_sum(l); tp = wave_sum_i(tp); fp = wave_sum_i(fp); fn = wave_sum_i(fn);
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { shf[w] = l; shi[3 * w] = tp; shi[3 * w + 1] = fp; shi[3 * w + 2] = fn; }
    __syncthreads();
    if (threadIdx.x != 0) return;
    const int TP = shi[0] + shi[3] + shi[6] + shi[9], FP = shi[1] + shi[4] + shi[7] + shi[10], FN = shi[2] + shi[5] + shi[8] + shi[11];
    const float r[4] = {(shf[0] + shf[1]) + (shf[2] + shf[3]), (float)((double)n_rows * C), (float)(2.0 * TP), (float)(2.0 * TP + FP + FN)};
    res[0] = r[0]; res[1] = r[1]; res[2] = r[2]; res[3] = r[3];
    if (res_i) { res_i[0] = TP; res_i[1] = FP; res_i[2] = FN; res_i[3] = n_rows; }
    wl_ring_row(ring, r);
}

// gcnhip_metrics_record_with_next_loss: the finalize launch of this loss writes the row
static WlRing wl_take_ring(gcnhip_ctx *c) {
    WlRing g = {nullptr, 1, 0, nullptr, nullptr};
    if (c->rec_armed) {
        g.ring = c->rec_ring; g.capacity = c->rec_capacity; g.slot = c->rec_slot; g.epoch = c->rec_epoch; g.sumsq = c->rec_sumsq;
        c->rec_armed = false;
    }
    return g;
}

extern "C" {

int gcnhip_wxent_fwd_rows(gcnhip_ctx *c, float *logits, int ld, float *grad, int ld_grad,
                          const int32_t *truth, const int32_t *d_rows, int n_listed, int num_classes, int training,
                          int count, int shift_in_place, float *d_result, int32_t *d_result_i, const float *d_grad_row_scale,
                          const float *d_class_weight, float weight_sum) {
    if (!c || !logits || !truth || !d_result || !d_class_weight || num_classes <= 0 || ld < num_classes || n_listed < 0 || count <= 0) return -1;
    if (num_classes > WL_MAXC_REG * WAVE) return gcnhip_fail("gcnhip_wxent_fwd_rows: more than 256 classes");
    if (n_listed > 0 && !d_rows) return -1;
    if (training && (!grad || ld_grad < num_classes)) return -1;
    if (training && !(weight_sum > 0.f)) return gcnhip_fail("gcnhip_wxent_fwd_rows: weight_sum must be positive when training");
    WxArgs a;
    a.logits = logits; a.grad = training ? grad : nullptr; a.truth = truth; a.rows = d_rows;
    a.grad_row_scale = d_grad_row_scale; a.weight = d_class_weight; a.weight_sum = weight_sum;
    a.ld = ld; a.ld_grad = ld_grad; a.n_rows = n_listed; a.C = num_classes;
    a.training = training; a.shift = shift_in_place;
    a.part_f = c->red_f + 2048; a.part_w = c->red_f + 4096; a.part_i = c->red_i;
    // the grids of xent_launch: the partials then add up in the unweighted kernel's order
    int blocks;
    const int nv4 = (num_classes + 3) / 4;
    const bool lanes = num_classes <= 64 && n_listed > 0 && ld % 4 == 0 && ld >= 4 * nv4 && aligned16(logits) &&
                       (!a.grad || (ld_grad % 4 == 0 && ld_grad >= 4 * nv4 && aligned16(a.grad)));
    if (lanes) {
        blocks = ceil_div(n_listed, 256);
        if (blocks > WX_MAX_BLOCKS) blocks = WX_MAX_BLOCKS;
        switch (nv4) {
#define WXL(N) case N: wxent_lane_kernel<N><<<blocks, 256, 0, c->stream>>>(a); break;
            WXL(1) WXL(2) WXL(3) WXL(4) WXL(5) WXL(6) WXL(7) WXL(8) WXL(9) WXL(10) WXL(11) WXL(12) WXL(13) WXL(14) WXL(15) WXL(16)
#undef WXL
        }
    } else {
        blocks = ceil_div(n_listed, 4 * 2);
        if (blocks < 1) blocks = 1;                     // a rank that owns no rows still reports zeros
        if (blocks > WX_MAX_BLOCKS) blocks = WX_MAX_BLOCKS;
        wxent_kernel<<<blocks, 256, 0, c->stream>>>(a);
    }
    GCNHIP_LAUNCH_CHECK();
    wxent_finalize_kernel<<<1, 256, 0, c->stream>>>(a.part_f, a.part_w, a.part_i, blocks, d_result, d_result_i, wl_take_ring(c));
    GCNHIP_LAUNCH_CHECK();
    return 0;
}

int gcnhip_wbce_fwd_rows(gcnhip_ctx *c, const float *logits, int ld, float *grad, int ld_grad,
                         const uint32_t *truth_bits, int words_per_row, const int32_t *d_rows, int n_listed,
                         int num_classes, int training, int count, const float *d_grad_row_scale,
                         float *d_result, int32_t *d_result_i, const float *d_pos_weight) {
    if (!c || !logits || !truth_bits || !d_result || !d_pos_weight || num_classes < 1 || ld < num_classes) return -1;
    if (num_classes > WL_MAXC_REG * WAVE) return gcnhip_fail("gcnhip_wbce_fwd_rows: more than 256 classes");
    if (words_per_row < (num_classes + 31) / 32 || n_listed < 0 || (n_listed > 0 && !d_rows)) return -1;
    if (training && (!grad || ld_grad < num_classes || count <= 0)) return -1;
    WbArgs a;
    a.logits = logits; a.grad = training ? grad : nullptr; a.truth = truth_bits; a.rows = d_rows;
    a.grad_row_scale = d_grad_row_scale; a.pos_weight = d_pos_weight;
    a.ld = ld; a.ld_grad = ld_grad; a.wpr = words_per_row; a.n_rows = n_listed; a.C = num_classes;
    a.denom = (float)((double)(count > 0 ? count : 1) * num_classes);
    int blocks = ceil_div(n_listed, 4 * 4);
    if (blocks > WB_MAX_BLOCKS) blocks = WB_MAX_BLOCKS;
    if (blocks < 1) blocks = 1;
    a.part_f = c->red_f + 2048;
    a.part_i = c->red_i;
    wbce_fwd_kernel<<<blocks, 256, 0, c->stream>>>(a);
    GCNHIP_LAUNCH_CHECK();
    wbce_finalize_kernel<<<1, 256, 0, c->stream>>>(a.part_f, a.part_i, blocks, n_listed, num_classes, d_result, d_result_i, wl_take_ring(c));
    GCNHIP_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
