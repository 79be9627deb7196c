// attach.hip — gather for rows that are NOT rows of an adjacency object: new nodes attached to a trained graph
// (ModelQueries::predict_new).  Beyond the reference, which can only score the nodes it was built with.
//
//   out[i, 0:dim] = epilogue( sum_{e in [ptr[i], ptr[i+1])} coef[e] * row(col[e]) )
//   row(c) = table_a[c, :] for c < n_a,  table_b[c - n_a, :] for n_a <= c < n_a + m
//
// Two tables read where they lie (the dataset nodes' rows of a forward, and the rows the call itself made for the new nodes):
// no concatenated copy, no gcnhip_graph object and none of its host planning.  The per-edge coefficient stream lets one kernel
// serve the factored and the per-edge form of the model; it is 4 bytes per edge against a gathered row of 164 bytes and more.
//
// Layout: graphsum.hip's.  A wave reads 64 (col, coef) pairs with one coalesced load each and hands them to its lane groups by
// shuffle; a lane group of L lanes holds a slice of up to 64 columns, 4 per lane, so a wave instruction reads 64 / L rows.  Where
// both tables' rows are 16-byte aligned a lane's 4 columns are one 16-byte load, else four guarded 4-byte loads — the same lanes,
// the same edges, the same order, so the two paths give the same bits.  dim > 64: the slices of 64 columns one after the other
// (the pairs are read again per slice).  Up to 4 row loads per lane group are in flight.
//
// Reduction order of a row (it depends on the row's own edge list and on dim, on nothing else: not on m, not on the row's
// position, not on the other rows — a row has the same bits alone, in any batch, on every launch):
//   * the edges in chunks of 64; inside a chunk lane group g of G = 64 / L takes edges g, g + G, ... in order, each into one
//     f32 accumulator per column (multiply, then add: fp contract off);
//   * a row of at most ATTACH_LONG_ROW edges: one wave walks its chunks in order, the accumulators carried from chunk to chunk,
//     then the G groups are added by the xor tree L, 2L, ... 32;
//   * a longer row: the four waves of a block, wave w walking chunks w, w + 4, ... the same way, then (w0 + w1) + (w2 + w3)
//     through LDS.  So a hub row costs a quarter of its length in dependent steps and never holds up a wave that has short
//     rows: a block first gives each of its 4 rows that is short to one wave, then takes its long rows one by one with all
//     four.  No row list, no atomics, one launch, and the launch needs to know nothing about the lengths.
// Epilogues: none; ReLU (v > 0 ? v : 0); predict (dim <= 64) — argmax (lowest class on a tie), its probability and optionally
// the log-softmax row, by the statements of graphsum.hip's predict_row_epilogue (max, exp of the shifted logits, their sum left
// to right, prob = 1 / sum, logp = (z - max) - log(sum)), followed at beta != 1 by those of calib.hip's calib_scale_kernel on
// that row (s = beta . logp, logp' = (s - max s) - log(sum exp(s - max s)), prob = exp(max logp')) — with ONE difference: the
// sum runs left to right here, where calib_scale_kernel adds in a shuffle tree, so the two agree within the rounding of a sum
// (an ulp or two of logp'), not bit for bit; tests/test_softmax_gpu.py holds both to float64.
// The launch allocates nothing, does not synchronise and trusts col to be in [0, n_a + m): the host validates (host/attach.h).
#include "common.h"
#include <cmath>
#include <cstdio>
#pragma clang fp contract(off)

constexpr int ATTACH_LONG_ROW = 512;             // edges; above it a row is summed by the 4 waves of its block
constexpr int ATTACH_U = 4;                      // row loads in flight per lane group

struct AttachArgs {
    const int32_t *ptr, *col;
    const float *coef;
    const float *ta, *tb;
    int n_a, m, ld_a, ld_b, dim;
    float *out;
    int ld_out, epilogue;
    int32_t *pred;
    float *prob, *logp;
    int ld_logp;
    float beta;
};

// columns c0 .. c0 + 3 of row j of the two tables (columns past dim: 0)
template <bool VEC>
__device__ __forceinline__ float4 attach_row4(const AttachArgs &a, int j, int c0) {
    const float *p = j < a.n_a ? a.ta + (size_t)j * a.ld_a : a.tb + (size_t)(j - a.n_a) * a.ld_b;
    if (VEC) {
        // a lane without columns reads the row's first piece and keeps none of it (ld % 4 == 0 and ld >= dim: c0 + 4 <= ld)
        const float4 v = *reinterpret_cast<const float4 *>(p + (c0 < a.dim ? c0 : 0));
        return c0 < a.dim ? v : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    float4 v;
    v.x = c0 + 0 < a.dim ? p[c0 + 0] : 0.f;
    v.y = c0 + 1 < a.dim ? p[c0 + 1] : 0.f;
    v.z = c0 + 2 < a.dim ? p[c0 + 2] : 0.f;
    v.w = c0 + 3 < a.dim ? p[c0 + 3] : 0.f;
    return v;
}

__device__ __forceinline__ float4 attach_fma(float c, float4 v, float4 acc) {
    acc.x += c * v.x; acc.y += c * v.y; acc.z += c * v.z; acc.w += c * v.w;
    return acc;
}
__device__ __forceinline__ float4 attach_add(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }

// one chunk of cnt <= 64 edges from `base` on: acc += the chunk, lane group g taking edges g, g + G, ... in order
template <int L, bool VEC>
__device__ __forceinline__ float4 attach_chunk(const AttachArgs &a, int base, int cnt, int lane, int g, int c0, float4 acc) {
    constexpr int G = WAVE / L;
    int my_idx = 0;
    float my_c = 0.f;
    if (lane < cnt) { my_idx = a.col[base + lane]; my_c = a.coef[base + lane]; }
    const int iters = (cnt + G - 1) / G;
    int k = 0;
    for (; (k + ATTACH_U) * G <= cnt; k += ATTACH_U) {         // every lane group has a real edge in each of the next U steps
        float4 v[ATTACH_U];
        float cc[ATTACH_U];
#pragma unroll
        for (int u = 0; u < ATTACH_U; u++) {
            const int src = (k + u) * G + g;
            const int j = __shfl(my_idx, src, WAVE);
            cc[u] = __shfl(my_c, src, WAVE);
            v[u] = attach_row4<VEC>(a, j, c0);
        }
#pragma unroll
        for (int u = 0; u < ATTACH_U; u++) acc = attach_fma(cc[u], v[u], acc);
    }
    const int j_safe = __shfl(my_idx, 0, WAVE);               // cnt >= 1: a lane without an edge reads the chunk's first row
    for (; k < iters; k++) {
        const int src = k * G + g;
        const bool on = src < cnt;
        const int j = __shfl(my_idx, src & 63, WAVE);
        const float c = __shfl(my_c, src & 63, WAVE);
        const float4 n = attach_fma(c, attach_row4<VEC>(a, on ? j : j_safe, c0), acc);
        acc.x = on ? n.x : acc.x; acc.y = on ? n.y : acc.y; acc.z = on ? n.z : acc.z; acc.w = on ? n.w : acc.w;
    }
    return acc;
}

// the chunks first, first + step, ... of the edges [e0, e1), then the lane groups added: every lane ends with the sum
template <int L, bool VEC>
__device__ __forceinline__ float4 attach_sum(const AttachArgs &a, int e0, int e1, int first, int step, int lane, int g, int c0) {
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int64_t base = (int64_t)e0 + first * WAVE; base < e1; base += step * WAVE)      // 64 bits: e1 may sit just below 2^31
        acc = attach_chunk<L, VEC>(a, (int)base, (int)min((int64_t)WAVE, e1 - base), lane, g, c0, acc);
#pragma unroll
    for (int s = L; s < WAVE; s <<= 1)
        acc = attach_add(acc, make_float4(__shfl_xor(acc.x, s, WAVE), __shfl_xor(acc.y, s, WAVE), __shfl_xor(acc.z, s, WAVE), __shfl_xor(acc.w, s, WAVE)));
    return acc;
}

enum { ATTACH_NONE = 0, ATTACH_RELU = 1, ATTACH_PREDICT = 2 };

__device__ __forceinline__ void attach_argmax_merge(float &bv, int &bi, float ov, int oi) {
    if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
}

// the epilogue of one slice of a row; the whole wave calls, every lane holding the sums of its columns c0 .. c0 + 3
template <int L>
__device__ __forceinline__ void attach_finish(const AttachArgs &a, int row, float4 acc, int lane, int g, int l, int c0) {
    float x[4] = {acc.x, acc.y, acc.z, acc.w};
    if (a.epilogue == ATTACH_RELU) {
#pragma unroll
        for (int i = 0; i < 4; i++) x[i] = x[i] > 0.f ? x[i] : 0.f;
    }
    if (a.out && g == 0) {
        float *o = a.out + (size_t)row * a.ld_out;
#pragma unroll
        for (int i = 0; i < 4; i++)
            if (c0 + i < a.dim) o[c0 + i] = x[i];
    }
    if (a.epilogue != ATTACH_PREDICT) return;
    // dim <= 64: one slice, lane q of group 0 holds columns 4q .. 4q + 3
    const int nv4 = (a.dim + 3) >> 2;
    float mx = -1e30f, bv = -INFINITY;
    int bi = 0x7FFFFFFF;
#pragma unroll
    for (int i = 0; i < 4; i++)
        if (c0 + i < a.dim) {
            mx = fmaxf(mx, x[i]);
            if (bi == 0x7FFFFFFF || x[i] > bv) { bv = x[i]; bi = c0 + i; }
        }
#pragma unroll
    for (int s = 1; s < L; s <<= 1) {
        mx = fmaxf(mx, __shfl_xor(mx, s, WAVE));
        attach_argmax_merge(bv, bi, __shfl_xor(bv, s, WAVE), __shfl_xor(bi, s, WAVE));
    }
    mx = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(mx)));       // lane 0 is in group 0
    bi = __builtin_amdgcn_readfirstlane(bi);
    float ex[4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        x[i] -= mx;
        ex[i] = c0 + i < a.dim ? expf(x[i]) : 0.f;
    }
    float se = 0.f;
    for (int q = 0; q < nv4; q++) {
#pragma unroll
        for (int i = 0; i < 4; i++) se += __int_as_float(__builtin_amdgcn_readlane(__float_as_int(ex[i]), q));
    }
    float prob = 1.f / se;
    const float ls = logf(se);
#pragma unroll
    for (int i = 0; i < 4; i++) x[i] -= ls;                    // the log-softmax row of z
    if (a.beta != 1.f) {                                       // ... and of beta . z, from that row by calib_scale_kernel's statements (sum left to right)
        float sm = -INFINITY;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            x[i] = a.beta * x[i];
            if (c0 + i < a.dim) sm = fmaxf(sm, x[i]);
        }
#pragma unroll
        for (int s = 1; s < L; s <<= 1) sm = fmaxf(sm, __shfl_xor(sm, s, WAVE));
        sm = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(sm)));
#pragma unroll
        for (int i = 0; i < 4; i++) {
            x[i] -= sm;
            ex[i] = c0 + i < a.dim ? expf(x[i]) : 0.f;
        }
        float z = 0.f;
        for (int q = 0; q < nv4; q++) {
#pragma unroll
            for (int i = 0; i < 4; i++) z += __int_as_float(__builtin_amdgcn_readlane(__float_as_int(ex[i]), q));
        }
        const float lz = logf(z);
        float om = -INFINITY;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            x[i] -= lz;
            if (c0 + i < a.dim) om = fmaxf(om, x[i]);
        }
#pragma unroll
        for (int s = 1; s < L; s <<= 1) om = fmaxf(om, __shfl_xor(om, s, WAVE));
        prob = expf(__int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(om))));
    }
    if (lane == 0) { a.pred[row] = bi; a.prob[row] = prob; }
    if (a.logp && g == 0 && l < nv4) {
        float *o = a.logp + (size_t)row * a.ld_logp + c0;
#pragma unroll
        for (int i = 0; i < 4; i++)
            if (c0 + i < a.dim) o[i] = x[i];
    }
}

// L lanes per row slice (1, 2, 4, 8 for dim <= 4, 8, 16, 32; else 16); a block of 4 waves owns rows 4 b .. 4 b + 3
template <int L, bool VEC>
__global__ __launch_bounds__(256) void attach_gather_kernel(AttachArgs a) {
    __shared__ float4 sh[4][16];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int g = lane / L, l = lane % L;
    const int row0 = blockIdx.x * 4;
    const int n_slices = (a.dim + 63) / 64;
    // short rows: a wave each
    const int mine = row0 + wave;
    if (mine < a.m) {
        const int e0 = a.ptr[mine], e1 = a.ptr[mine + 1];
        if (e1 - e0 <= ATTACH_LONG_ROW)
            for (int s = 0; s < n_slices; s++) {
                const int c0 = s * 64 + l * 4;
                attach_finish<L>(a, mine, attach_sum<L, VEC>(a, e0, e1, 0, 1, lane, g, c0), lane, g, l, c0);
            }
    }
    // long rows: the block each (every test here is the same in all 256 threads)
    for (int w = 0; w < 4 && row0 + w < a.m; w++) {
        const int row = row0 + w;
        const int e0 = a.ptr[row], e1 = a.ptr[row + 1];
        if (e1 - e0 <= ATTACH_LONG_ROW) continue;
        for (int s = 0; s < n_slices; s++) {
            const int c0 = s * 64 + l * 4;
            const float4 part = attach_sum<L, VEC>(a, e0, e1, wave, 4, lane, g, c0);
            if (g == 0) sh[wave][l] = part;
            __syncthreads();
            if (wave == 0) attach_finish<L>(a, row, attach_add(attach_add(sh[0][l], sh[1][l]), attach_add(sh[2][l], sh[3][l])), lane, g, l, c0);
            __syncthreads();
        }
    }
}

template <int L>
static void attach_launch(gcnhip_ctx *c, const AttachArgs &a, bool vec) {
    const int blocks = ceil_div(a.m, 4);
    if (vec) attach_gather_kernel<L, true><<<blocks, 256, 0, c->stream>>>(a);
    else attach_gather_kernel<L, false><<<blocks, 256, 0, c->stream>>>(a);
}

static int attach_refuse(const char *why) {
    char msg[200];
    snprintf(msg, sizeof msg, "gcnhip_attach_gather: %s", why);
    return gcnhip_fail(msg);
}

extern "C" int gcnhip_attach_gather(gcnhip_ctx *c, const int32_t *d_ptr, const int32_t *d_col, const float *d_coef, int m, const float *table_a,
                                    int ld_a, int n_a, const float *table_b, int ld_b, int dim, int epilogue, float *out, int ld_out, int32_t *d_pred,
                                    float *d_prob, float *d_logp, int ld_logp, float beta) {
    if (!c || m < 0 || n_a < 0 || !d_ptr) return attach_refuse("invalid argument");
    if (dim < 1 || dim > 256) return attach_refuse("1 <= dim <= 256");
    if (epilogue != ATTACH_NONE && epilogue != ATTACH_RELU && epilogue != ATTACH_PREDICT) return attach_refuse("the epilogue is 0 (none), 1 (ReLU) or 2 (predict)");
    if ((n_a > 0 && (!table_a || ld_a < dim)) || (m > 0 && (!table_b || ld_b < dim))) return attach_refuse("a table is missing or its row stride is below dim");
    if (out && ld_out < dim) return attach_refuse("the row stride of out is below dim");
    if (out && (out == table_a || out == table_b)) return attach_refuse("out must not be one of the gathered tables");
    if (epilogue == ATTACH_PREDICT) {
        if (dim > 64) return attach_refuse("the predict epilogue takes at most 64 columns (the row of a node sits in one wave)");
        if (!d_pred || !d_prob || (d_logp && ld_logp < dim)) return attach_refuse("the predict epilogue needs pred and prob (and ld_logp >= dim)");
        if (!(beta > 0.f) || !(beta <= GCNHIP_BETA_MAX)) return attach_refuse(GCNHIP_BETA_REFUSAL);
    } else if (!out) {
        return attach_refuse("out is NULL and there is no predict epilogue");
    }
    if (m == 0) return 0;
    if (!d_col || !d_coef) return attach_refuse("invalid argument");
    AttachArgs a = {d_ptr, d_col, d_coef, table_a, table_b, n_a, m, ld_a, ld_b, dim, out, ld_out, epilogue, d_pred, d_prob, d_logp, ld_logp, beta};
    const bool vec = (!table_a || (aligned16(table_a) && ld_a % 4 == 0)) && aligned16(table_b) && ld_b % 4 == 0;
    if (dim <= 4) attach_launch<1>(c, a, vec);
    else if (dim <= 8) attach_launch<2>(c, a, vec);
    else if (dim <= 16) attach_launch<4>(c, a, vec);
    else if (dim <= 32) attach_launch<8>(c, a, vec);
    else attach_launch<16>(c, a, vec);
    GCNHIP_LAUNCH_CHECK();
    return 0;
}
