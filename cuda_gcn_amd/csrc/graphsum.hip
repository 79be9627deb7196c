// graphsum.hip — CSR row-gather  out[r,:] = sum_e coef(e) * in[col(e),:]
// (the reference's GraphSum forward AND backward: src/seq/module.cpp:83-119,
//  src/cuda/cuda_kernel.cu:126-162).
//
// Bound: gather bandwidth (0.5 FLOP/B).  Design for gfx950:
//  * one wave64 per row task; the wave reads 64 (index, coef) pairs with one
//    coalesced load each and hands them to its lane groups by cross-lane
//    shuffle, so the only per-edge memory instruction is the feature-row load;
//  * a feature row is read with 16-byte lane loads: L lanes per row slice,
//    64/L rows per wave instruction (d=128: 16 lanes per 64-float slice, 4 rows /
//    1 KiB per instruction); gather_chunk issues GS_U (4; 2 past the Infinity
//    Cache) row loads per lane group before the first is used, from a
//    wave-uniform loop so that no load sits inside a per-lane branch;
//  * partial sums of the lane groups are combined with wave shuffles (no LDS,
//    no atomics) — results are bitwise reproducible run to run;
//  * rows longer than SPLIT_EDGES are cut into segments processed by separate
//    waves (heavy segments dispatched first) and summed in segment order by a
//    small second kernel, so a hub row does not serialise the tail;
//  * XCD-aware launch for rows of whole 256-byte pieces: the columns are cut into
//    64-float (256-byte) slices and each slice is bound to the workgroups of one XCD
//    group (blockIdx % 8), so every XCD's private 4 MiB L2 caches 1/slices of the
//    table (d=128: half of it) and the (index, coef) stream is re-read once per slice;
//  * the ReLU + dropout of the first layer is an optional store epilogue.
// The reference launches one block per row with `dim` threads and does a
// global read-modify-write per edge (cuda_kernel.cu:126-143).
#include "dense_kernels.h"
#include <algorithm>
#include <stdlib.h>

struct GsArgs {
    const int *indptr, *indices;
    const float *coef;
    const int4 *tasks;
    int n_tasks, n_rows, nnz;
    size_t table_bytes;      // n_cols * ld_in * 4: decides the batch depth (cache-resident or HBM regime)
    const float *in;
    const uint16_t *in_bf;   // bf16 copy of the gathered table (opt-in storage format); row stride ld_in values
    float *out;
    float *partials;
    int ld_in, ld_out, part_ld, dim;
    int n_slices;     // >= 1: the columns are cut into n_slices slices of L*4 floats, one slice per XCD group
    int bounds[9];          // task range [bounds[g], bounds[g+1]) of XCD group g (equal edge counts)
    // epilogue
    int fuse, training, thr;
    float scale;
    uint64_t seed, elem_offset;
    const uint32_t *d_epoch;
    const uint8_t *keep_mask;
    const uint32_t *row_bits;   // optional: bit j == 0 -> row j of `in` is all zero and is not read
    const uint32_t *out_bits;   // optional: bit r == 0 -> nobody reads row r of `out`: it is not computed (left untouched)
    uint32_t *pos_bits;         // optional (fuse, dim % 32 == 0, vector kernel): bit (c & 31) of pos_bits[r * wpr + (c >> 5)] =
    int wpr;                    // (out[r, c] > 0) AFTER the ReLU/dropout epilogue — the mask their backward needs, so that it
                                // does not have to read the activations again (gcnhip_matmul_bwd_fused_bits)
    int accumulate;             // 1: out[r,:] = out[r,:] + sum (the second of two operators that share the rows of `out`:
                                // the remote-column part of a row-partitioned aggregation, gcnhip_graphsum_part)
    // factored coefficients (gcnhip_graphsum_ex): coef == NULL -> every edge counts 1 and the row's total is multiplied by
    // post[row] (NULL: by nothing) before the epilogue.  The input rows then hold dinv(col) * x.
    const float *post;
    // loss epilogue (gcnhip_gs_loss, gcnhip.h): xe_truth == NULL -> off.  dim <= 64: one lane group holds the row.
    const int32_t *xe_truth;
    float *xe_grad; int xe_ld_grad; int xe_training;
    float xe_count;
    const float *xe_grad_scale;
    float *xe_terms;
};

__device__ inline bool row_wanted(const GsArgs &a, int row) {
    return !a.out_bits || ((a.out_bits[row >> 5] >> (row & 31)) & 1u);
}

__device__ inline float4 f4_fma(float c, float4 v, float4 a) {
    a.x += c * v.x; a.y += c * v.y; a.z += c * v.z; a.w += c * v.w;
    return a;
}
__device__ inline float4 f4_add(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
__device__ inline float4 f4_shfl_xor(float4 v, int m) {
    return make_float4(__shfl_xor(v.x, m, WAVE), __shfl_xor(v.y, m, WAVE), __shfl_xor(v.z, m, WAVE), __shfl_xor(v.w, m, WAVE));
}

// ReLU (module.cpp:179-181: keep = x > 0) then dropout on one float4 of row r
__device__ inline float4 relu_dropout4(float4 v, const GsArgs &a, int64_t r, int col0) {
    float x[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int i = 0; i < 4; i++) x[i] = x[i] > 0.f ? x[i] : 0.f;
    if (a.training) {
        const uint32_t epoch = a.d_epoch ? *a.d_epoch : 0u;
        const int64_t e0 = r * a.dim + col0;          // element index inside this matrix
        uint32_t bits;
        if (a.keep_mask) {
            bits = 0;
#pragma unroll
            for (int i = 0; i < 4; i++) bits |= (col0 + i < a.dim && a.keep_mask[e0 + i] ? 1u : 0u) << i;
        } else {
            const uint64_t j0 = a.elem_offset + (uint64_t)e0;
            if ((j0 & 3) == 0) {
                bits = keep4(j0 >> 2, epoch, a.seed, a.thr);
            } else {
                bits = 0;
#pragma unroll
                for (int i = 0; i < 4; i++) bits |= (keep1(j0 + i, epoch, a.seed, a.thr) ? 1u : 0u) << i;
            }
        }
#pragma unroll
        for (int i = 0; i < 4; i++) x[i] *= (bits >> i & 1u) ? a.scale : 0.f;   // module.cpp:216
    }
    return make_float4(x[0], x[1], x[2], x[3]);
}

// ---- loss epilogue (gcnhip_gs_loss) ------------------------------------------------------------------------------------
// The arithmetic of xent_lane_kernel (xent.hip; CrossEntropyLoss::forward, module.cpp:124-161), statement for statement,
// on a row that sits in a wave's registers instead of in memory: max (order-free), exp of the shifted logits, their sum
// LEFT TO RIGHT (v_readlane of column after column into a wave-uniform chain of adds: the reference's order and
// xent_lane_kernel's), the loss term, the accuracy test, the gradient quad of each lane.  Same bits as the loss kernel run
// on the stored row.
// Layout A (vector kernel): lane l of group 0 holds columns 4l..4l+3 in z; every lane of the wave calls.
template <int L>
__device__ __forceinline__ void xent_row_epilogue4(const GsArgs &a, int row, float4 z, int lane, int l, int g, int col0) {
#pragma clang fp contract(off)
    const int t = a.xe_truth[row];                          // wave-uniform
    const int nv4 = (a.dim + 3) >> 2;
    float *gr = a.xe_grad ? a.xe_grad + (size_t)row * a.xe_ld_grad : nullptr;
    if (t < 0) {                                            // not scored: zero gradient row, zero terms (module.cpp:129,132)
        if (a.xe_training && gr && g == 0 && l < nv4) *reinterpret_cast<float4 *>(gr + col0) = make_float4(0.f, 0.f, 0.f, 0.f);
        if (lane == 0) *reinterpret_cast<float2 *>(a.xe_terms + 2 * (size_t)row) = make_float2(0.f, 0.f);
        return;
    }
    float x[4] = {z.x, z.y, z.z, z.w};
    float mx = -1e30f;                                      // module.cpp:135
#pragma unroll
    for (int i = 0; i < 4; i++) if (col0 + i < a.dim) mx = fmaxf(mx, x[i]);
#pragma unroll
    for (int m = 1; m < L; m <<= 1) mx = fmaxf(mx, __shfl_xor(mx, m, WAVE));
    mx = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(mx)));       // lane 0 is in group 0
    const int ti = t & 3;
    const float sel = ti == 0 ? x[0] : (ti == 1 ? x[1] : (ti == 2 ? x[2] : x[3]));
    const float tv = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(sel), t >> 2));
    const bool correct = !(mx > tv);                        // gcn.cpp:88-93
    float ex[4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        x[i] -= mx;                                         // module.cpp:140
        ex[i] = col0 + i < a.dim ? expf(x[i]) : 0.f;
    }
    float se = 0.f;
    for (int q = 0; q < nv4; q++) {                         // columns 4q .. 4q+3 live in lane q (group 0): left to right
#pragma unroll
        for (int i = 0; i < 4; i++) se += __int_as_float(__builtin_amdgcn_readlane(__float_as_int(ex[i]), q));
    }
    const float term = logf(se) - (tv - mx);                // module.cpp:143
    if (lane == 0) *reinterpret_cast<float2 *>(a.xe_terms + 2 * (size_t)row) = make_float2(term, correct ? 1.f : 0.f);
    if (a.xe_training && gr && g == 0 && l < nv4) {
        const float gs = a.xe_grad_scale ? a.xe_grad_scale[row] : 1.f;
        float o[4];
#pragma unroll
        for (int i = 0; i < 4; i++) {
            float p = ex[i] / se;                           // module.cpp:147
            if (col0 + i == t) p = (float)((double)p - 1.0);
            o[i] = col0 + i < a.dim ? (a.xe_grad_scale ? (p / a.xe_count) * gs : p / a.xe_count) : 0.f;   // module.cpp:157
        }
        *reinterpret_cast<float4 *>(gr + col0) = make_float4(o[0], o[1], o[2], o[3]);
    }
}
// Layout B (finalize kernel, split rows): lane c of the block's first wave holds column c in v; that whole wave calls.
__device__ __forceinline__ void xent_row_epilogue1(const GsArgs &a, int row, float v, int lane) {
#pragma clang fp contract(off)
    const int t = a.xe_truth[row];
    const int nv4 = (a.dim + 3) >> 2;
    float *gr = a.xe_grad ? a.xe_grad + (size_t)row * a.xe_ld_grad : nullptr;
    if (t < 0) {
        if (a.xe_training && gr && lane < 4 * nv4) gr[lane] = 0.f;
        if (lane == 0) *reinterpret_cast<float2 *>(a.xe_terms + 2 * (size_t)row) = make_float2(0.f, 0.f);
        return;
    }
    float mx = lane < a.dim ? fmaxf(-1e30f, v) : -1e30f;
#pragma unroll
    for (int m = 1; m < WAVE; m <<= 1) mx = fmaxf(mx, __shfl_xor(mx, m, WAVE));
    const float tv = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), t));
    const bool correct = !(mx > tv);
    const float x = v - mx;
    const float ex = lane < a.dim ? expf(x) : 0.f;
    float se = 0.f;
    for (int j = 0; j < 4 * nv4; j++) se += __int_as_float(__builtin_amdgcn_readlane(__float_as_int(ex), j));
    const float term = logf(se) - (tv - mx);
    if (lane == 0) *reinterpret_cast<float2 *>(a.xe_terms + 2 * (size_t)row) = make_float2(term, correct ? 1.f : 0.f);
    if (a.xe_training && gr && lane < 4 * nv4) {
        float p = ex / se;
        if (lane == t) p = (float)((double)p - 1.0);
        const float gs = a.xe_grad_scale ? a.xe_grad_scale[row] : 1.f;
        gr[lane] = lane < a.dim ? (a.xe_grad_scale ? (p / a.xe_count) * gs : p / a.xe_count) : 0.f;
    }
}

constexpr int GS_U = 4;        // row loads in flight per lane group when the table is cache resident (bf16 kernel: always)
// One chunk of <= 64 edges whose (index, coef) pairs sit in the wave's lanes: acc += sum over the chunk, lane group g
// taking edges g, g + G, ... in order (the order every form of the kernel keeps, so all of them agree bit for bit).
template <int L, int GS_U>
__device__ __forceinline__ float4 gather_chunk(const GsArgs &a, const float *in, int my_idx, float my_c, int cnt, int g, float4 acc) {
    constexpr int G = WAVE / L;
    const int iters = (cnt + G - 1) / G;
    // GS_U row loads per lane group are in flight together whenever the next GS_U iterations are all real edges
    // (a wave-uniform test, so the loads need no predicate and nothing has to wait inside a branch).  Until round
    // 2 this was a `#pragma unroll 8` over a loop with the load inside a per-lane branch: the compiler kept ONE
    // load in flight per wave — a 100-edge row was 13 dependent round trips — and the kernel was bound by
    // latency x resident waves (4 instead of 8 waves per SIMD: 1.08 -> 1.87 ms).  Same order of the sum.
    int k = 0;
    if (!a.row_bits) {
        for (; (k + GS_U) * G <= cnt; k += GS_U) {
            float4 v[GS_U];
            float cc[GS_U];
#pragma unroll
            for (int u = 0; u < GS_U; u++) {
                const int src = (k + u) * G + g;
                const int j = __shfl(my_idx, src, WAVE);
                cc[u] = __shfl(my_c, src, WAVE);
                v[u] = *reinterpret_cast<const float4 *>(in + (size_t)j * a.ld_in);
            }
#pragma unroll
            for (int u = 0; u < GS_U; u++) acc = f4_fma(cc[u], v[u], acc);
        }
    }
    // the tail of a row, and rows read through an input mask: the same batches, with the lanes that have no edge
    // (or an edge whose row is known to be zero) reading the chunk's first neighbour instead and keeping their sum
    const int j_safe = __shfl(my_idx, 0, WAVE);
    for (; k < iters; k += GS_U) {
        float4 v[GS_U];
        float cc[GS_U];
        bool on[GS_U];
#pragma unroll
        for (int u = 0; u < GS_U; u++) {
            const int src = (k + u) * G + g;
            const int j = __shfl(my_idx, src & 63, WAVE);
            cc[u] = __shfl(my_c, src & 63, WAVE);
            on[u] = src < cnt && cc[u] != 0.f;         // padded lanes and known-zero rows contribute nothing
            v[u] = *reinterpret_cast<const float4 *>(in + (size_t)(on[u] ? j : j_safe) * a.ld_in);
        }
#pragma unroll
        for (int u = 0; u < GS_U; u++) {
            const float4 n = f4_fma(cc[u], v[u], acc);
            acc.x = on[u] ? n.x : acc.x; acc.y = on[u] ? n.y : acc.y; acc.z = on[u] ? n.z : acc.z; acc.w = on[u] ? n.w : acc.w;
        }
    }
    return acc;
}

// ---- the pieces every gather kernel is made of -----------------------------------------------------------------------
// Each kernel below stays a kernel of its own: it calls these and then runs its own epilogue.

// A row task: the edges [e0, e1) of `row`.  slot >= 0: a segment of a split row, whose sum goes to partials[slot].
struct GsTask { int row, e0, e1, slot; };
__device__ __forceinline__ GsTask gs_task(const GsArgs &a, int t) {
    if (a.n_tasks) {
        const int4 tk = a.tasks[t];
        return {tk.x, tk.y, tk.z, tk.w};
    }
    return {t, a.indptr[t], a.indptr[t + 1], -1};
}

// XCD-aware mapping of a block's waves to (task t, column slice) — speed only, never correctness: workgroups are dealt
// round-robin over the 8 XCDs, so blockIdx % 8 names the group of blocks that share an L2.  Each group gets
//  (a) one column slice (wide rows, SLICED): its 4 MiB L2 then sees 1/n_slices of the gathered table;
//  (b) a CONTIGUOUS range of the task list, so rows that are neighbours in the node order —
//      the same community after reordering — are gathered through the same L2.
// false: the group has no task left for this wave (wave-uniform).
template <bool SLICED>
__device__ __forceinline__ bool gs_block_task(const GsArgs &a, int &t, int &cslice) {
    const int xcd = blockIdx.x & 7, q = blockIdx.x >> 3;
    cslice = SLICED ? xcd % a.n_slices : blockIdx.y;
    const int g_id = SLICED ? xcd / a.n_slices : xcd;      // which share of the tasks
    t = a.bounds[g_id] + q * (blockDim.x >> 6) + (threadIdx.x >> 6);
    return t < a.bounds[g_id + 1];
}

// One chunk of cnt <= 64 (index, coef) pairs, one pair per lane with one coalesced load each; lanes past cnt hold (0, 0).
__device__ __forceinline__ void gs_load_edges(const GsArgs &a, int base, int cnt, int lane, int &my_idx, float &my_c) {
    my_idx = 0;
    my_c = 0.f;
    if (lane < cnt) {
        my_idx = a.indices[base + lane];
        // > 0 for every real edge.  Factored operator (a.coef == NULL, wave-uniform): every edge counts 1 and no coefficient
        // stream is read — the saving is the stream (measured 0.756 -> 0.720 ms at Reddit scale); instantiations that also
        // drop the hand-out shuffle and the multiply measured the same 0.720 ms and were not kept
        my_c = a.coef ? a.coef[base + lane] : 1.f;
        if (a.row_bits && !((a.row_bits[my_idx >> 5] >> (my_idx & 31)) & 1u)) my_c = 0.f;   // wave-uniform test
    }
}

// The lane groups' partial sums combined by wave shuffles: every lane ends with the sum over all groups.
template <int L>
__device__ __forceinline__ float4 gs_group_sum(float4 acc) {
#pragma unroll
    for (int m = L; m < WAVE; m <<= 1) acc = f4_add(acc, f4_shfl_xor(acc, m));
    return acc;
}

// A segment's sum to its slot of the split-row scratch: a finalize launch adds the segments.
__device__ __forceinline__ void gs_store_partial(const GsArgs &a, int slot, int col0, float4 acc) {
    *reinterpret_cast<float4 *>(a.partials + (size_t)slot * a.part_ld + col0) = acc;
}
__device__ __forceinline__ void gs_store_partial(const GsArgs &a, int slot, int col0, float4 lo, float4 hi) {
    gs_store_partial(a, slot, col0, lo);
    gs_store_partial(a, slot, col0 + 4, hi);
}

// v + the segments [first, first + ns) of a split row at column col, left to right (ns >= 1).  Four partials in flight per
// batch, the tail by unconditional loads from clamped slots.
__device__ __forceinline__ float gs_segment_sum(const GsArgs &a, int first, int ns, int col, float v) {
    const float *pp = a.partials + (size_t)first * a.part_ld + col;
    int k = 0;
    for (; k + 4 <= ns; k += 4) {
        const float p0 = pp[(size_t)k * a.part_ld], p1 = pp[(size_t)(k + 1) * a.part_ld];
        const float p2 = pp[(size_t)(k + 2) * a.part_ld], p3 = pp[(size_t)(k + 3) * a.part_ld];
        v += p0; v += p1; v += p2; v += p3;
    }
    const float p0 = pp[(size_t)min(k, ns - 1) * a.part_ld], p1 = pp[(size_t)min(k + 1, ns - 1) * a.part_ld];
    const float p2 = pp[(size_t)min(k + 2, ns - 1) * a.part_ld];
    if (k < ns) v += p0;
    if (k + 1 < ns) v += p1;
    if (k + 2 < ns) v += p2;
    return v;
}

// The factored operator's row factor (a.post == NULL: none), and the store of a lane's quad at o = &out[row, col0]: whole,
// or the ragged tail of a row with dim % 4 != 0.
__device__ __forceinline__ float4 gs_post4(const GsArgs &a, int row, float4 acc) {
    if (a.post) { const float ps = a.post[row]; acc.x *= ps; acc.y *= ps; acc.z *= ps; acc.w *= ps; }
    return acc;
}
__device__ __forceinline__ void gs_store_row4(const GsArgs &a, float *o, int col0, float4 acc) {
    if (col0 + 4 <= a.dim) {
        *reinterpret_cast<float4 *>(o) = acc;
    } else {
        const float x[4] = {acc.x, acc.y, acc.z, acc.w};
        for (int i = 0; col0 + i < a.dim; i++) o[i] = x[i];
    }
}

// L lanes per feature row (float4 each), G = 64/L rows per wave instruction.
// SLICED: the launch binds one column slice to each XCD group (it only changes the block -> (tasks, columns) mapping; the
// flag is a template argument so that profiles name the hidden-width launches apart from the class-width ones).
template <int L, int U = GS_U, bool SLICED = false>
__global__ __launch_bounds__(256) void graphsum_vec_kernel(GsArgs a) {
    const int lane = threadIdx.x & 63;
    int t, cslice;
    if (!gs_block_task<SLICED>(a, t, cslice)) return;
    const auto [row, e0, e1, slot] = gs_task(a, t);
    if (!row_wanted(a, row)) return;                       // wave-uniform
    const int g = lane / L, l = lane % L;
    const int col0 = (cslice * L + l) * 4;                  // first column of this lane's float4
    const bool active = col0 < a.dim;
    const float *in = a.in + (active ? col0 : 0);           // lanes past the last column read (and discard) columns 0..3
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int base = e0; base < e1; base += WAVE) {
        const int cnt = min(WAVE, e1 - base);
        int my_idx;
        float my_c;
        gs_load_edges(a, base, cnt, lane, my_idx, my_c);
        acc = gather_chunk<L, U>(a, in, my_idx, my_c, cnt, g, acc);
    }
    if constexpr (L < WAVE) acc = gs_group_sum<L>(acc);    // L == 64: one lane group, nothing to combine (an empty call still moves registers)
    if (slot >= 0) {
        if (g == 0 && active) gs_store_partial(a, slot, col0, acc);
        return;
    }
    uint32_t nib = 0;                                       // this lane's four (out > 0) bits, at their place in the row's word
    if (g == 0 && active) {
        float *o = a.out + (size_t)row * a.ld_out + col0;
        if (a.accumulate && slot < 0) {                    // what the first operator left in this row, then this one's terms
            if (col0 + 4 <= a.dim) {
                acc = f4_add(*reinterpret_cast<const float4 *>(o), acc);
            } else {
                float x[4] = {acc.x, acc.y, acc.z, acc.w};
                for (int i = 0; col0 + i < a.dim; i++) x[i] = o[i] + x[i];
                acc = make_float4(x[0], x[1], x[2], x[3]);
            }
        }
        acc = gs_post4(a, row, acc);
        if (a.fuse) acc = relu_dropout4(acc, a, row, col0);
        gs_store_row4(a, o, col0, acc);
        nib = ((acc.x > 0.f ? 1u : 0u) | (acc.y > 0.f ? 2u : 0u) | (acc.z > 0.f ? 4u : 0u) | (acc.w > 0.f ? 8u : 0u)) << (4 * (l & 7));
    }
    if constexpr (!SLICED && L <= 16)
        if (a.xe_truth) xent_row_epilogue4<L>(a, row, acc, lane, l, g, col0);     // wave-uniform; one column chunk (launch site)
    if (L >= 8 && a.pos_bits) {                             // wave-uniform; dim % 32 == 0 (launch site): 8 lanes hold one word
        nib |= __shfl_xor(nib, 1, WAVE);
        nib |= __shfl_xor(nib, 2, WAVE);
        nib |= __shfl_xor(nib, 4, WAVE);
        if (g == 0 && active && (l & 7) == 0) a.pos_bits[(size_t)row * a.wpr + (col0 >> 5)] = nib;
    }
}

// ---- bf16 table, f32 accumulate (opt-in storage format) ------------------------
// The gathered rows are stored as bfloat16 (round-to-nearest-even of the f32 values, made by
// gcnhip_f32_to_bf16), so a row of d values is d*2 bytes: half the 128-byte lines per edge.  coef, the
// sum and the output stay f32.  L lanes per row slice, 8 values (16 bytes) per lane; slices of 64 columns
// = one line, bound to XCD groups like the f32 kernel.
__device__ inline void bf8_fma(float c, const uint4 v, float4 &lo, float4 &hi) {
    lo.x += c * __uint_as_float(v.x << 16); lo.y += c * __uint_as_float(v.x & 0xFFFF0000u);
    lo.z += c * __uint_as_float(v.y << 16); lo.w += c * __uint_as_float(v.y & 0xFFFF0000u);
    hi.x += c * __uint_as_float(v.z << 16); hi.y += c * __uint_as_float(v.z & 0xFFFF0000u);
    hi.z += c * __uint_as_float(v.w << 16); hi.w += c * __uint_as_float(v.w & 0xFFFF0000u);
}

// gather_chunk for the bf16 table: the same batches of GS_U row loads in flight, the same j_safe tail, the same order of the sum
template <int L>
__device__ __forceinline__ void gather_chunk_bf16(const GsArgs &a, const uint16_t *in, int my_idx, float my_c, int cnt, int g, float4 &lo, float4 &hi) {
    constexpr int G = WAVE / L;
    const int iters = (cnt + G - 1) / G;
    int k = 0;
    if (!a.row_bits) {
        for (; (k + GS_U) * G <= cnt; k += GS_U) {
            uint4 v[GS_U];
            float cc[GS_U];
#pragma unroll
            for (int u = 0; u < GS_U; u++) {
                const int src = (k + u) * G + g;
                const int j = __shfl(my_idx, src, WAVE);
                cc[u] = __shfl(my_c, src, WAVE);
                v[u] = *reinterpret_cast<const uint4 *>(in + (size_t)j * a.ld_in);
            }
#pragma unroll
            for (int u = 0; u < GS_U; u++) bf8_fma(cc[u], v[u], lo, hi);
        }
    }
    const int j_safe = __shfl(my_idx, 0, WAVE);
    for (; k < iters; k += GS_U) {
        uint4 v[GS_U];
        float cc[GS_U];
        bool on[GS_U];
#pragma unroll
        for (int u = 0; u < GS_U; u++) {
            const int src = (k + u) * G + g;
            const int j = __shfl(my_idx, src & 63, WAVE);
            cc[u] = __shfl(my_c, src & 63, WAVE);
            on[u] = src < cnt && cc[u] != 0.f;
            v[u] = *reinterpret_cast<const uint4 *>(in + (size_t)(on[u] ? j : j_safe) * a.ld_in);
        }
#pragma unroll
        for (int u = 0; u < GS_U; u++) {
            float4 nlo = lo, nhi = hi;
            bf8_fma(cc[u], v[u], nlo, nhi);
            lo.x = on[u] ? nlo.x : lo.x; lo.y = on[u] ? nlo.y : lo.y; lo.z = on[u] ? nlo.z : lo.z; lo.w = on[u] ? nlo.w : lo.w;
            hi.x = on[u] ? nhi.x : hi.x; hi.y = on[u] ? nhi.y : hi.y; hi.z = on[u] ? nhi.z : hi.z; hi.w = on[u] ? nhi.w : hi.w;
        }
    }
}

template <int L>
__global__ __launch_bounds__(256) void graphsum_bf16_kernel(GsArgs a) {
    const int lane = threadIdx.x & 63;
    int t, cslice;                                          // sliced or not is the launch's choice (a.n_slices), wave-uniform
    if (!(a.n_slices > 1 ? gs_block_task<true>(a, t, cslice) : gs_block_task<false>(a, t, cslice))) return;
    const auto [row, e0, e1, slot] = gs_task(a, t);
    if (!row_wanted(a, row)) return;                       // wave-uniform
    const int g = lane / L, l = lane % L;
    const int col0 = (cslice * L + l) * 8;
    const bool active = col0 < a.dim;
    const uint16_t *in = a.in_bf + (active ? col0 : 0);     // lanes past the last column read (and discard) columns 0..7
    float4 lo = make_float4(0.f, 0.f, 0.f, 0.f), hi = lo;
    for (int base = e0; base < e1; base += WAVE) {
        const int cnt = min(WAVE, e1 - base);
        int my_idx;
        float my_c;
        gs_load_edges(a, base, cnt, lane, my_idx, my_c);
        gather_chunk_bf16<L>(a, in, my_idx, my_c, cnt, g, lo, hi);
    }
    lo = gs_group_sum<L>(lo);
    hi = gs_group_sum<L>(hi);
    if (g == 0 && active) {
        if (slot >= 0) {
            gs_store_partial(a, slot, col0, lo, hi);
        } else {
            if (a.fuse) { lo = relu_dropout4(lo, a, row, col0); hi = relu_dropout4(hi, a, row, col0 + 4); }
            float *o = a.out + (size_t)row * a.ld_out + col0;
            const float x[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
            if (col0 + 8 <= a.dim && (a.ld_out & 3) == 0) {
                *reinterpret_cast<float4 *>(o) = lo;
                *reinterpret_cast<float4 *>(o + 4) = hi;
            } else {
                for (int i = 0; i < 8 && col0 + i < a.dim; i++) o[i] = x[i];
            }
        }
    }
}

// ---- prediction epilogue (gcnhip_graphsum_predict) ------------------------------------------------------------------
// The row reduction of the loss epilogue with a different output: pred[r] = argmax of the logit row (the LOWEST column on a
// tie, numpy.argmax's rule), prob[r] = 1 / sum_j exp(z_j - max) — max and the left-to-right sum are the loss epilogue's, so
// the bits of the sum are those of xent_row_epilogue*'s `se` — and optionally logp[r, :] = (z - max) - log(sum), the whole
// log-softmax row.  Kernels of their own (graphsum_predict_*) carry it.
struct PredArgs {
    int32_t *pred;          // [rows of out]
    float *prob;            // [rows of out]
    float *logp;            // NULL, or [rows of out x ld_logp]
    int ld_logp;
};

// (value, column) of the larger logit; on equal values the lower column
__device__ __forceinline__ void argmax_merge(float &bv, int &bi, float ov, int oi) {
    if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
}

// Layouts A (f32 vector kernel, K = 4) and C (bf16 kernel, K = 8): lane l of group 0 holds columns K*l .. K*l+K-1 of the
// row in z (one column chunk: dim <= 64, launch site); every lane of the wave calls.
template <int L, int K>
__device__ __forceinline__ void predict_row_epilogue(const GsArgs &a, const PredArgs &p, int row, const float (&z)[K], int lane, int l,
                                                     int g, int col0) {
#pragma clang fp contract(off)
    const int nvk = (a.dim + K - 1) / K;                    // lanes of group 0 that hold columns
    float x[K];
    float mx = -1e30f;                                      // as xent_row_epilogue4
    float bv = -INFINITY;
    int bi = 0x7FFFFFFF;
#pragma unroll
    for (int i = 0; i < K; i++) {
        x[i] = z[i];
        if (col0 + i < a.dim) {
            mx = fmaxf(mx, x[i]);
            if (bi == 0x7FFFFFFF || x[i] > bv) { bv = x[i]; bi = col0 + i; }
        }
    }
#pragma unroll
    for (int m = 1; m < L; m <<= 1) {
        mx = fmaxf(mx, __shfl_xor(mx, m, WAVE));
        argmax_merge(bv, bi, __shfl_xor(bv, m, WAVE), __shfl_xor(bi, m, WAVE));
    }
    mx = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(mx)));       // lane 0 is in group 0
    bi = __builtin_amdgcn_readfirstlane(bi);
    float ex[K];
#pragma unroll
    for (int i = 0; i < K; i++) {
        x[i] -= mx;
        ex[i] = col0 + i < a.dim ? expf(x[i]) : 0.f;
    }
    float se = 0.f;
    for (int q = 0; q < nvk; q++) {                         // columns K*q .. K*q+K-1 live in lane q (group 0): left to right
#pragma unroll
        for (int i = 0; i < K; i++) se += __int_as_float(__builtin_amdgcn_readlane(__float_as_int(ex[i]), q));
    }
    if (lane == 0) { p.pred[row] = bi; p.prob[row] = 1.f / se; }
    if (p.logp && g == 0 && l < nvk) {
        const float ls = logf(se);
        float *o = p.logp + (size_t)row * p.ld_logp + col0;
#pragma unroll
        for (int i = 0; i < K; i++) if (col0 + i < a.dim) o[i] = x[i] - ls;
    }
}
// Layout B (finalize kernel, split rows): lane c of the block's first wave holds column c in v; that whole wave calls.
__device__ __forceinline__ void predict_row_epilogue1(const GsArgs &a, const PredArgs &p, int row, float v, int lane) {
#pragma clang fp contract(off)
    const int nv4 = (a.dim + 3) >> 2;
    const bool in_row = lane < a.dim;
    float mx = in_row ? fmaxf(-1e30f, v) : -1e30f;          // as xent_row_epilogue1
    float bv = in_row ? v : -INFINITY;
    int bi = in_row ? lane : 0x7FFFFFFF;
#pragma unroll
    for (int m = 1; m < WAVE; m <<= 1) {
        mx = fmaxf(mx, __shfl_xor(mx, m, WAVE));
        argmax_merge(bv, bi, __shfl_xor(bv, m, WAVE), __shfl_xor(bi, m, WAVE));
    }
    const float x = v - mx;
    const float ex = in_row ? expf(x) : 0.f;
    float se = 0.f;
    for (int j = 0; j < 4 * nv4; j++) se += __int_as_float(__builtin_amdgcn_readlane(__float_as_int(ex), j));
    if (lane == 0) { p.pred[row] = bi; p.prob[row] = 1.f / se; }
    if (p.logp && in_row) p.logp[(size_t)row * p.ld_logp + lane] = x - logf(se);
}

// Prediction kernels: the pieces of graphsum_vec_kernel (one column chunk, not sliced), graphsum_bf16_kernel and
// graphsum_finalize_kernel — same lane groups, same edge order, same reduction tree and post factor, so the logits have the
// bits of those kernels — with the prediction epilogue in place of the ReLU / dropout / mask / loss options (which a
// prediction never takes, so those kernels do not carry it).  `out` may be NULL: the logits are not stored.
template <int L, int U>
__global__ __launch_bounds__(256) void graphsum_predict_vec_kernel(GsArgs a, PredArgs p) {
    const int lane = threadIdx.x & 63;
    int t, cslice;
    if (!gs_block_task<false>(a, t, cslice)) return;
    const auto [row, e0, e1, slot] = gs_task(a, t);
    const int g = lane / L, l = lane % L;
    const int col0 = l * 4;
    const bool active = col0 < a.dim;
    const float *in = a.in + (active ? col0 : 0);
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int base = e0; base < e1; base += WAVE) {
        const int cnt = min(WAVE, e1 - base);
        int my_idx;
        float my_c;
        gs_load_edges(a, base, cnt, lane, my_idx, my_c);
        acc = gather_chunk<L, U>(a, in, my_idx, my_c, cnt, g, acc);
    }
    acc = gs_group_sum<L>(acc);
    if (slot >= 0) {                                        // the finalize launch predicts
        if (g == 0 && active) gs_store_partial(a, slot, col0, acc);
        return;
    }
    if (g == 0 && active) {
        acc = gs_post4(a, row, acc);
        if (a.out) gs_store_row4(a, a.out + (size_t)row * a.ld_out + col0, col0, acc);
    }
    const float z[4] = {acc.x, acc.y, acc.z, acc.w};
    predict_row_epilogue<L, 4>(a, p, row, z, lane, l, g, col0);
}

template <int L>
__global__ __launch_bounds__(256) void graphsum_predict_bf16_kernel(GsArgs a, PredArgs p) {
    const int lane = threadIdx.x & 63;
    int t, cslice;
    if (!gs_block_task<false>(a, t, cslice)) return;
    const auto [row, e0, e1, slot] = gs_task(a, t);
    const int g = lane / L, l = lane % L;
    const int col0 = l * 8;
    const bool active = col0 < a.dim;
    const uint16_t *in = a.in_bf + (active ? col0 : 0);
    float4 lo = make_float4(0.f, 0.f, 0.f, 0.f), hi = lo;
    for (int base = e0; base < e1; base += WAVE) {
        const int cnt = min(WAVE, e1 - base);
        int my_idx;
        float my_c;
        gs_load_edges(a, base, cnt, lane, my_idx, my_c);
        gather_chunk_bf16<L>(a, in, my_idx, my_c, cnt, g, lo, hi);
    }
    lo = gs_group_sum<L>(lo);
    hi = gs_group_sum<L>(hi);
    if (slot >= 0) {
        if (g == 0 && active) gs_store_partial(a, slot, col0, lo, hi);
        return;
    }
    const float z[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
    if (g == 0 && active && a.out) {
        float *o = a.out + (size_t)row * a.ld_out + col0;
        for (int i = 0; i < 8 && col0 + i < a.dim; i++) o[i] = z[i];
    }
    predict_row_epilogue<L, 8>(a, p, row, z, lane, l, g, col0);
}

// f32 -> bf16 (round to nearest even; NaN stays NaN), columns dim..ld_dst-1 of every row written as 0
__global__ __launch_bounds__(256) void f32_to_bf16_kernel(const float *__restrict__ src, int ld_src, uint16_t *__restrict__ dst, int ld_dst,
                                                          int64_t rows, int dim) {
    const int per_row = ld_dst / 8;
    const int64_t total = rows * per_row;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = i / per_row;
        const int c0 = (int)(i % per_row) * 8;
        uint32_t h[8];
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const float f = c0 + k < dim ? src[r * ld_src + c0 + k] : 0.f;
            const uint32_t u = __float_as_uint(f);
            h[k] = (f != f) ? ((u >> 16) | 0x40u) : ((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16);
        }
        uint4 v;
        v.x = (h[0] & 0xFFFFu) | (h[1] << 16); v.y = (h[2] & 0xFFFFu) | (h[3] << 16);
        v.z = (h[4] & 0xFFFFu) | (h[5] << 16); v.w = (h[6] & 0xFFFFu) | (h[7] << 16);
        *reinterpret_cast<uint4 *>(dst + r * ld_dst + c0) = v;
    }
}

// ---- the pieces every launch is made of ------------------------------------------------------------------------------
// The rows a launch computes: every row of the adjacency object, or a registered subset of them.
struct GsRows {
    const int (*bounds)[9];
    const int4 *split_rows;
    int n_split_rows;
};

// The operator's part of GsArgs.  A registered row subset brings its own compacted task list (same order, same segment slots).
static GsRows gs_fill(GsArgs &a, const gcnhip_graph *g, const gcnhip_rowset *rs, int ld_in, int elem_bytes) {
    a.indptr = g->indptr; a.indices = g->indices; a.coef = g->coef;
    a.tasks = rs ? rs->tasks : g->tasks; a.n_tasks = rs ? rs->n_tasks : g->n_tasks; a.n_rows = g->n_rows; a.nnz = g->nnz;
    a.table_bytes = (size_t)g->n_cols * ld_in * elem_bytes;
    a.partials = g->partials; a.part_ld = g->part_ld;
    if (rs) return {rs->bounds, rs->split_rows, rs->n_split_rows};
    return {g->bounds, g->split_rows, g->n_split_rows};
}

// The segment scratch of split rows is sized when the object is built (256 columns) or by gcnhip_graph_reserve_width;
// a launch never allocates, synchronises or touches the object.
static bool gs_scratch_too_narrow(const gcnhip_graph *g, int dim) { return g->n_slots && g->part_ld < (dim + 7) / 8 * 8; }

// The task ranges of the 8 / n_slices XCD groups that share the task list; returns the blocks (of 4 waves) per XCD.
static int gs_bounds(GsArgs &a, const int (*xb)[9], int n_slices) {
    a.n_slices = n_slices;
    const int G = 8 / n_slices;
    const int lg = G == 8 ? 3 : (G == 4 ? 2 : (G == 2 ? 1 : 0));
    int max_blocks = 1;
    for (int k = 0; k <= 8; k++) a.bounds[k] = xb[lg][k];
    for (int k = 0; k < G; k++) max_blocks = std::max(max_blocks, ceil_div(a.bounds[k + 1] - a.bounds[k], 4));
    return max_blocks;
}

// Batch depth by regime.  A table that fits the 256 MiB Infinity Cache is gathered with 4 row loads in flight per lane
// group (latency-bound otherwise: 1.08 -> 0.85 ms at Reddit scale).  Past it the kernel is HBM-bound and 2 is the
// optimum (R-MAT scale 21, 1 GiB table, d = 128: 5.33 / 5.16 / 5.51 ms with 1 / 2 / 4 in flight).
static int gs_batch_depth(const gcnhip_ctx *c, const GsArgs &a) {
    return c->opt.gs_u ? c->opt.gs_u : (a.table_bytes > ((size_t)256 << 20) ? 2 : 4);
}

// After the gather launch: the finalize launch, when there are split rows.
template <class F>
static int gs_finish(int n_split_rows, F finalize) {
    GCNHIP_LAUNCH_CHECK();
    if (n_split_rows) {
        finalize();
        GCNHIP_LAUNCH_CHECK();
    }
    return 0;
}

template <int L>
static void launch_bf16(GsArgs a, const int (*xb)[9], hipStream_t s, const PredArgs *pred = nullptr) {
    const int ychunks = ceil_div(a.dim, L * 8);
    const bool sliced = ychunks > 1 && 8 % ychunks == 0;
    const int max_blocks = gs_bounds(a, xb, sliced ? ychunks : 1);
    if constexpr (L <= 8) {
        if (pred) { graphsum_predict_bf16_kernel<L><<<max_blocks * 8, 256, 0, s>>>(a, *pred); return; }   // dim <= 64: one chunk
    }
    graphsum_bf16_kernel<L><<<dim3(max_blocks * 8, sliced ? 1 : ychunks), 256, 0, s>>>(a);
}

// Any ld / alignment: scalar loads, lane l owns columns l, l+L, ...
template <int L>
__global__ __launch_bounds__(256) void graphsum_scalar_kernel(GsArgs a) {
    constexpr int G = WAVE / L;
    constexpr int MAXC = 4;                                // columns per lane per pass
    const int lane = threadIdx.x & 63;
    const int t = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const int nt = a.n_tasks ? a.n_tasks : a.n_rows;
    if (t >= nt) return;
    const auto [row, e0, e1, slot] = gs_task(a, t);
    if (!row_wanted(a, row)) return;                       // wave-uniform
    const int g = lane / L, l = lane % L;
    for (int cbase = 0; cbase < a.dim; cbase += L * MAXC) {
        float acc[MAXC] = {0.f, 0.f, 0.f, 0.f};
        for (int base = e0; base < e1; base += WAVE) {
            const int cnt = min(WAVE, e1 - base);
            int my_idx;
            float my_c;
            gs_load_edges(a, base, cnt, lane, my_idx, my_c);
            const int iters = (cnt + G - 1) / G;
#pragma unroll 4
            for (int k = 0; k < iters; k++) {
                const int src = k * G + g;
                const int j = __shfl(my_idx, src, WAVE);
                const float c = __shfl(my_c, src, WAVE);
                const float *p = a.in + (size_t)j * a.ld_in + cbase + l;
                if (src < cnt && c != 0.f) {
#pragma unroll
                    for (int q = 0; q < MAXC; q++)
                        if (cbase + l + q * L < a.dim) acc[q] += c * p[q * L];
                }
            }
        }
#pragma unroll
        for (int q = 0; q < MAXC; q++) {
#pragma unroll
            for (int m = L; m < WAVE; m <<= 1) acc[q] += __shfl_xor(acc[q], m, WAVE);
        }
        if (g == 0) {
#pragma unroll
            for (int q = 0; q < MAXC; q++) {
                const int col = cbase + l + q * L;
                if (col >= a.dim) continue;
                float v = acc[q];
                if (slot >= 0) {
                    a.partials[(size_t)slot * a.part_ld + col] = v;
                } else {
                    if (a.accumulate) v = a.out[(size_t)row * a.ld_out + col] + v;
                    if (a.fuse) {
                        v = v > 0.f ? v : 0.f;
                        if (a.training) {
                            const int64_t e = (int64_t)row * a.dim + col;
                            const bool keep = a.keep_mask ? a.keep_mask[e] != 0
                                                          : keep1(a.elem_offset + (uint64_t)e, a.d_epoch ? *a.d_epoch : 0u, a.seed, a.thr);
                            v *= keep ? a.scale : 0.f;
                        }
                    }
                    a.out[(size_t)row * a.ld_out + col] = v;
                }
            }
        }
    }
}

// sum the segment partials of each split row in segment order, apply the epilogue
__global__ __launch_bounds__(256) void graphsum_finalize_kernel(GsArgs a, const int4 *split_rows, int n_split_rows) {
    const int s = blockIdx.x;
    if (s >= n_split_rows) return;
    const int4 sr = split_rows[s];
    const int row = sr.x, first = sr.y, ns = sr.z;
    if (!row_wanted(a, row)) return;
    for (int c0 = 0; c0 < a.dim; c0 += blockDim.x) {        // whole waves stay in the loop: the ballot below needs them
        const int col = c0 + threadIdx.x;
        float v = 0.f;
        if (col < a.dim) {
            v = gs_segment_sum(a, first, ns, col, a.accumulate ? a.out[(size_t)row * a.ld_out + col] : 0.f);
            if (a.post) v *= a.post[row];
            if (a.fuse) {
                v = v > 0.f ? v : 0.f;
                if (a.training) {
                    const int64_t e = (int64_t)row * a.dim + col;
                    const bool keep = a.keep_mask ? a.keep_mask[e] != 0
                                                  : keep1(a.elem_offset + (uint64_t)e, a.d_epoch ? *a.d_epoch : 0u, a.seed, a.thr);
                    v *= keep ? a.scale : 0.f;
                }
            }
            a.out[(size_t)row * a.ld_out + col] = v;
        }
        if (a.xe_truth && threadIdx.x < WAVE) xent_row_epilogue1(a, row, v, threadIdx.x);   // dim <= 64 (launch site): the first wave holds the row
        if (a.pos_bits) {                                   // 64 consecutive columns per wave: two words of the row
            const uint64_t b = __ballot(col < a.dim && v > 0.f);
            const int w0 = (c0 + (int)(threadIdx.x & ~63u)) >> 5;
            if ((threadIdx.x & 63) == 0 && w0 < a.wpr) a.pos_bits[(size_t)row * a.wpr + w0] = (uint32_t)b;
            if ((threadIdx.x & 63) == 32 && w0 + 1 < a.wpr) a.pos_bits[(size_t)row * a.wpr + w0 + 1] = (uint32_t)(b >> 32);
        }
    }
}

// the segment sum (dim <= 64: one pass, the first wave holds the row) with the prediction epilogue
__global__ __launch_bounds__(256) void graphsum_finalize_predict_kernel(GsArgs a, PredArgs p, const int4 *split_rows, int n_split_rows) {
    const int s = blockIdx.x;
    if (s >= n_split_rows || threadIdx.x >= WAVE) return;  // whole wave 0 stays
    const int4 sr = split_rows[s];
    const int row = sr.x, first = sr.y, ns = sr.z;
    const int col = threadIdx.x;
    float v = 0.f;
    if (col < a.dim) {
        v = gs_segment_sum(a, first, ns, col, 0.f);
        if (a.post) v *= a.post[row];
        if (a.out) a.out[(size_t)row * a.ld_out + col] = v;
    }
    predict_row_epilogue1(a, p, row, v, col);
}

// ---- blend epilogue (gcnhip_graphsum_blend) -------------------------------------------------------------------------
// One step of label propagation / Correct & Smooth:  out[r, :] = clamp(alpha * (A^ . in)[r, :] + beta * base[r, :], lo, hi),
// optionally pred[r] = argmax of that row (the lowest column on a tie).  The gather is graphsum_predict_vec_kernel's — the same
// pieces: task list, lane groups, edge order, reduction tree and split-row scratch — with another epilogue in a kernel of its
// own.  The operator is taken UNFACTORED (per-edge coefficients, g->coef): at class width the 4-byte
// coefficient rides beside a 192-byte gathered row, and staying unscaled keeps the iterate in one form — the table a launch
// writes is the table the next one gathers, with no dinv-scaled copy to maintain between iterations.
struct BlendArgs {
    const float *base;      // [n_rows x ld_base]; may be the gathered table itself
    int ld_base;
    float alpha, beta, lo, hi;
    int32_t *pred;          // NULL, or [n_rows]
};

__device__ __forceinline__ float blend1(const BlendArgs &b, float sum, float base) {
#pragma clang fp contract(off)
    return fminf(fmaxf(b.alpha * sum + b.beta * base, b.lo), b.hi);
}

template <int L, int U>
__global__ __launch_bounds__(256) void graphsum_blend_vec_kernel(GsArgs a, BlendArgs b) {
    const int lane = threadIdx.x & 63;
    int t, cslice;
    if (!gs_block_task<false>(a, t, cslice)) return;
    const auto [row, e0, e1, slot] = gs_task(a, t);
    const int g = lane / L, l = lane % L;
    const int col0 = l * 4;
    const bool active = col0 < a.dim;
    const float *in = a.in + (active ? col0 : 0);
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int base = e0; base < e1; base += WAVE) {
        const int cnt = min(WAVE, e1 - base);
        int my_idx;
        float my_c;
        gs_load_edges(a, base, cnt, lane, my_idx, my_c);
        acc = gather_chunk<L, U>(a, in, my_idx, my_c, cnt, g, acc);
    }
    acc = gs_group_sum<L>(acc);
    if (slot >= 0) {                                        // the finalize launch blends
        if (g == 0 && active) gs_store_partial(a, slot, col0, acc);
        return;
    }
    float x[4] = {acc.x, acc.y, acc.z, acc.w};
    float bv = -INFINITY;
    int bi = 0x7FFFFFFF;
    if (g == 0 && active) {
        const float *bp = b.base + (size_t)row * b.ld_base + col0;
        float bb[4] = {0.f, 0.f, 0.f, 0.f};                 // ragged tail: the padding of base is not read, that of out not written
        if (col0 + 4 <= a.dim) {
            const float4 q = *reinterpret_cast<const float4 *>(bp);
            bb[0] = q.x; bb[1] = q.y; bb[2] = q.z; bb[3] = q.w;
        } else {
            for (int i = 0; col0 + i < a.dim; i++) bb[i] = bp[i];
        }
#pragma unroll
        for (int i = 0; i < 4; i++) x[i] = blend1(b, x[i], bb[i]);
        gs_store_row4(a, a.out + (size_t)row * a.ld_out + col0, col0, make_float4(x[0], x[1], x[2], x[3]));
#pragma unroll
        for (int i = 0; i < 4; i++)
            if (col0 + i < a.dim && (bi == 0x7FFFFFFF || x[i] > bv)) { bv = x[i]; bi = col0 + i; }
    }
    if (b.pred) {                                           // wave-uniform; lanes 0 .. L-1 are group 0
#pragma unroll
        for (int m = 1; m < L; m <<= 1) argmax_merge(bv, bi, __shfl_xor(bv, m, WAVE), __shfl_xor(bi, m, WAVE));
        if (lane == 0) b.pred[row] = bi;
    }
}

// the segment sum (one wave per split row, lane c on column c) with the blend epilogue
__global__ __launch_bounds__(64) void graphsum_finalize_blend_kernel(GsArgs a, BlendArgs b, const int4 *split_rows, int n_split_rows) {
    const int s = blockIdx.x;
    if (s >= n_split_rows || threadIdx.x >= WAVE) return;
    const int4 sr = split_rows[s];
    const int row = sr.x, first = sr.y, ns = sr.z;
    const int col = threadIdx.x;
    const bool in_row = col < a.dim;
    float v = 0.f;
    if (in_row) {
        v = gs_segment_sum(a, first, ns, col, 0.f);
        v = blend1(b, v, b.base[(size_t)row * b.ld_base + col]);
        a.out[(size_t)row * a.ld_out + col] = v;
    }
    if (b.pred) {
        float bv = in_row ? v : -INFINITY;
        int bi = in_row ? col : 0x7FFFFFFF;
#pragma unroll
        for (int m = 1; m < WAVE; m <<= 1) argmax_merge(bv, bi, __shfl_xor(bv, m, WAVE), __shfl_xor(bi, m, WAVE));
        if (col == 0) b.pred[row] = bi;
    }
}

template <int L>
static void launch_blend(const GsArgs &a, const BlendArgs &b, int blocks, int u, hipStream_t s) {
    if (u >= 4) graphsum_blend_vec_kernel<L, 4><<<blocks, 256, 0, s>>>(a, b);
    else graphsum_blend_vec_kernel<L, 2><<<blocks, 256, 0, s>>>(a, b);
}

template <int L>
static void launch_vec(GsArgs &a, const int (*xb)[9], const gcnhip_ctx *c, const PredArgs *pred = nullptr) {
    hipStream_t s = c->stream;
    const int ychunks = ceil_div(a.dim, L * 4);
    const bool sliced = ychunks > 1 && 8 % ychunks == 0;   // XCD-sliced columns (1-D grid)
    const int max_blocks = gs_bounds(a, xb, sliced ? ychunks : 1);
    const int u = gs_batch_depth(c, a);
    const dim3 grid(max_blocks * 8, sliced ? 1 : ychunks);
    if constexpr (L <= 16) {
        if (pred) {                                         // dim <= 64: one column chunk, never sliced; 1 or 2 loads in flight: same bits
            if (u >= 4) graphsum_predict_vec_kernel<L, 4><<<grid, 256, 0, s>>>(a, *pred);
            else graphsum_predict_vec_kernel<L, 2><<<grid, 256, 0, s>>>(a, *pred);
            return;
        }
    }
    if (sliced) {
        if (u >= 4) graphsum_vec_kernel<L, 4, true><<<grid, 256, 0, s>>>(a);
        else if (u >= 2) graphsum_vec_kernel<L, 2, true><<<grid, 256, 0, s>>>(a);
        else graphsum_vec_kernel<L, 1, true><<<grid, 256, 0, s>>>(a);
    } else {
        if (u >= 4) graphsum_vec_kernel<L, 4><<<grid, 256, 0, s>>>(a);
        else if (u >= 2) graphsum_vec_kernel<L, 2><<<grid, 256, 0, s>>>(a);
        else graphsum_vec_kernel<L, 1><<<grid, 256, 0, s>>>(a);
    }
}
template <int L>
static void launch_scalar(const GsArgs &a, int nt, hipStream_t s) {
    graphsum_scalar_kernel<L><<<ceil_div(nt, 4), 256, 0, s>>>(a);
}

// One aggregation launch as the entry points describe it: each names what it sets, the rest keeps its default.
struct GsCall {
    const float *in = nullptr;
    const uint16_t *in_bf = nullptr;                        // the bf16 table, in place of `in`
    float *out = nullptr;                                   // may be NULL with pred: the logits are not stored
    int ld_in = 0, ld_out = 0, dim = 0;
    const gcnhip_rowset *rs = nullptr;
    const uint32_t *row_bits = nullptr, *out_bits = nullptr;
    int accumulate = 0, scaling = 0;
    // the ReLU + dropout store epilogue (fuse), and the mask words its backward reads
    int fuse = 0, training = 0;
    float p = 0.f;
    uint64_t seed = 0, elem_offset = 0;
    const uint32_t *d_epoch = nullptr;
    const uint8_t *keep_mask = nullptr;
    uint32_t *pos_bits = nullptr;
    int wpr = 0;
    const gcnhip_gs_loss *loss = nullptr;
    const PredArgs *pred = nullptr;
};

static GsCall gs_call(const float *in, int ld_in, float *out, int ld_out, int dim) {
    GsCall k;
    k.in = in; k.ld_in = ld_in; k.out = out; k.ld_out = ld_out; k.dim = dim;
    return k;
}

static int graphsum_impl(gcnhip_ctx *c, const gcnhip_graph *g, const GsCall &k) {
    const float *in = k.in;
    const uint16_t *in_bf = k.in_bf;
    float *out = k.out;
    const int ld_in = k.ld_in, ld_out = k.ld_out, dim = k.dim, fuse = k.fuse;
    const gcnhip_rowset *rs = k.rs;
    const gcnhip_gs_loss *loss = k.loss;
    const PredArgs *pred = k.pred;
    uint32_t *pos_bits = k.pos_bits;
    if (!c || !g || (!in && !in_bf) || (!out && !pred) || dim <= 0 || ld_in < dim || ld_out < dim) return -1;
    if (k.scaling < 0 || k.scaling > 3) return -1;
    if (k.accumulate && in_bf) return -1;                   // the bf16 kernel has no accumulating store
    if (rs && rs->owner != g)                                // a subset brings task lists and segment slots of ITS adjacency object
        return gcnhip_fail("gcnhip_graphsum*: the row subset was registered on another adjacency object");
    if (in_bf && (ld_in % 8 != 0 || !aligned16(in_bf))) return -1;
    if (g->n_rows == 0 || (rs && rs->n_tasks == 0)) return 0;
    if (gs_scratch_too_narrow(g, dim))
        return gcnhip_fail("gcnhip_graphsum*: dim is wider than the split-row scratch of this adjacency object; call "
                           "gcnhip_graph_reserve_width(ctx, g, dim) once before the first launch (restricted objects: on them too)");
    GsArgs a = {};
    const GsRows rows = gs_fill(a, g, rs, ld_in, in_bf ? 2 : 4);
    const int (*xb)[9] = rows.bounds;
    a.in = in; a.in_bf = in_bf; a.out = out;
    a.ld_in = ld_in; a.ld_out = ld_out; a.dim = dim;
    a.fuse = fuse; a.training = k.training; a.thr = dropout_threshold(k.p);
    a.scale = 1 / (1 - k.p);                                // module.cpp:212
    a.seed = k.seed; a.elem_offset = k.elem_offset; a.d_epoch = k.d_epoch; a.keep_mask = k.keep_mask;
    a.row_bits = k.row_bits;
    a.out_bits = k.out_bits;
    a.accumulate = k.accumulate;
    a.pos_bits = pos_bits; a.wpr = k.wpr;
    const int nt = a.n_tasks ? a.n_tasks : g->n_rows;
    const bool vec = (ld_in % 4 == 0) && (ld_out % 4 == 0) && aligned16(in) && aligned16(out);
    a.xe_count = 1.f;
    if (loss) {
        const int w4 = (dim + 3) / 4 * 4;
        if (in_bf || !vec || dim > 64 || fuse || pos_bits || !loss->truth || !loss->row_terms || loss->count <= 0 || ((uintptr_t)loss->row_terms & 7))
            return gcnhip_fail("gcnhip_graphsum_ex: the loss epilogue needs f32 rows that are 16-byte aligned, dim <= 64, no relu_dropout, truth, row_terms and count > 0");
        if (loss->training && (!loss->grad || loss->ld_grad < w4 || loss->ld_grad % 4 != 0 || !aligned16(loss->grad)))
            return gcnhip_fail("gcnhip_graphsum_ex: the loss epilogue writes whole 16-byte quads of the gradient row: ld_grad % 4 == 0, ld_grad >= round_up(dim, 4)");
        a.xe_truth = loss->truth; a.xe_grad = loss->training ? loss->grad : nullptr; a.xe_ld_grad = loss->ld_grad; a.xe_training = loss->training ? 1 : 0;
        a.xe_count = (float)loss->count; a.xe_grad_scale = loss->grad_row_scale; a.xe_terms = loss->row_terms;
    }
    if (pred && (dim > 64 || fuse || pos_bits || loss || k.accumulate || k.row_bits || k.out_bits || (!in_bf && !vec)))
        return gcnhip_fail("gcnhip_graphsum_predict: needs dim <= 64 and f32 rows that are 16-byte aligned (ld % 4 == 0) or a bf16 table");
    if (k.scaling) {
        // the factored operator runs in the 16-byte-row f32 kernel only (what the model's layouts always are)
        if (in_bf || !vec) return gcnhip_fail("gcnhip_graphsum_ex: scaling != 0 needs f32 rows that are 16-byte aligned (ld % 4 == 0)");
        a.coef = nullptr;
        a.post = k.scaling == 1 ? g->dinv_row : (k.scaling == 2 ? g->dinv2_row : nullptr);
    }
    if (pos_bits && !(fuse && !in_bf && vec && dim % 32 == 0 && k.wpr * 32 >= dim))
        return gcnhip_fail("gcnhip_graphsum_relu_dropout_bits: needs the fused epilogue, 16-byte aligned rows, dim % 32 == 0 and words_per_row * 32 >= dim");
    const int d4 = (dim + 3) / 4;
    a.n_slices = 1;
    if (in_bf) {
        const int d8 = (dim + 7) / 8;                       // 16-byte pieces per row
        if (d8 <= 1) launch_bf16<1>(a, xb, c->stream, pred);
        else if (d8 <= 2) launch_bf16<2>(a, xb, c->stream, pred);
        else if (d8 <= 4) launch_bf16<4>(a, xb, c->stream, pred);
        else if (d8 % 16 == 0) launch_bf16<16>(a, xb, c->stream);   // 128-column (two-line) slices as in the f32 kernel: 305 -> 322 epochs/s
        else launch_bf16<8>(a, xb, c->stream, pred);               // 64-column (one line) slices, one per XCD group when 8 % slices == 0
    }
    const int gl = c->opt.gs_l;                             // narrower column slices than 64 floats (8: 32 floats, 4: 16 floats), round 5
    if (in_bf) {
    } else if (vec && !loss && !pred && (gl == 8 || (gl == 4 && !pos_bits)) && dim % (gl * 4) == 0 && dim / (gl * 4) > 1 && 8 % (dim / (gl * 4)) == 0) {
        // More slices = a smaller share of the table per XCD's L2 (what a structure-free graph's hub rows need) against more
        // re-reads of the index stream and shorter requests.  Measured per graph (tools/exp_structure.py); never the default.
        // (16-float slices hold half a mask word per lane group: with pos_bits they fall through to the 64-float slices below)
        if (gl == 8) launch_vec<8>(a, xb, c); else launch_vec<4>(a, xb, c);
    } else if (vec && dim % 64 == 0 && 8 % (dim / 64) == 0) {
        // rows of whole 128-byte lines: 64-float (two-line) column slices, one per XCD group, so each XCD's L2 holds
        // 1/slices of the table and the (index, coef) stream is re-read only once per slice.  Measured at Reddit scale
        // with 4 row loads in flight, 32- / 64- / 128-float slices: d = 64: 0.434 / 0.403 / - ms; d = 128: 0.843 / 0.760 /
        // 0.874; d = 256: 2.36 / 1.77 / 1.78; R-MAT scale 21 (HBM regime), d = 128: 5.20 / 4.57 ms.
        launch_vec<16>(a, xb, c, pred);
    } else if (vec) {
        if (d4 <= 1) launch_vec<1>(a, xb, c, pred);
        else if (d4 <= 2) launch_vec<2>(a, xb, c, pred);
        else if (d4 <= 4) launch_vec<4>(a, xb, c, pred);
        else if (d4 <= 8) launch_vec<8>(a, xb, c, pred);
        else if (d4 <= 16) launch_vec<16>(a, xb, c, pred);
        else if (d4 <= 32) launch_vec<32>(a, xb, c);
        else launch_vec<64>(a, xb, c);
    } else {
        if (dim <= 1) launch_scalar<1>(a, nt, c->stream);
        else if (dim <= 2) launch_scalar<2>(a, nt, c->stream);
        else if (dim <= 4) launch_scalar<4>(a, nt, c->stream);
        else if (dim <= 8) launch_scalar<8>(a, nt, c->stream);
        else if (dim <= 16) launch_scalar<16>(a, nt, c->stream);
        else if (dim <= 32) launch_scalar<32>(a, nt, c->stream);
        else launch_scalar<64>(a, nt, c->stream);
    }
    return gs_finish(rows.n_split_rows, [&] {
        if (pred) graphsum_finalize_predict_kernel<<<rows.n_split_rows, WAVE, 0, c->stream>>>(a, *pred, rows.split_rows, rows.n_split_rows);
        else graphsum_finalize_kernel<<<rows.n_split_rows, 256, 0, c->stream>>>(a, rows.split_rows, rows.n_split_rows);
    });
}

extern "C" {

int gcnhip_graphsum(gcnhip_ctx *c, const gcnhip_graph *g, const float *in, int ld_in,
                    float *out, int ld_out, int dim) {
    return graphsum_impl(c, g, gs_call(in, ld_in, out, ld_out, dim));
}

int gcnhip_graphsum_rowmask(gcnhip_ctx *c, const gcnhip_graph *g, const float *in, int ld_in,
                            float *out, int ld_out, int dim, const uint32_t *in_row_bits) {
    GsCall k = gs_call(in, ld_in, out, ld_out, dim);
    k.row_bits = in_row_bits;
    return graphsum_impl(c, g, k);
}

int gcnhip_graphsum_masked(gcnhip_ctx *c, const gcnhip_graph *g, const float *in, int ld_in,
                           float *out, int ld_out, int dim, const uint32_t *in_row_bits, const uint32_t *out_row_bits) {
    GsCall k = gs_call(in, ld_in, out, ld_out, dim);
    k.row_bits = in_row_bits; k.out_bits = out_row_bits;
    return graphsum_impl(c, g, k);
}

int gcnhip_graphsum_rowset(gcnhip_ctx *c, const gcnhip_graph *g, const gcnhip_rowset *rows, const float *in, int ld_in,
                           float *out, int ld_out, int dim, const uint32_t *in_row_bits) {
    if (!rows) return -1;
    GsCall k = gs_call(in, ld_in, out, ld_out, dim);
    k.row_bits = in_row_bits; k.rs = rows;
    return graphsum_impl(c, g, k);
}

int gcnhip_graphsum_relu_dropout(gcnhip_ctx *c, const gcnhip_graph *g, const float *in, int ld_in,
                                 float *out, int ld_out, int dim, int training, float p,
                                 uint64_t seed, const uint32_t *d_epoch, uint64_t elem_offset,
                                 const uint8_t *keep_mask) {
    if (training && !(p >= 0.f && p < 1.f)) return -1;
    GsCall k = gs_call(in, ld_in, out, ld_out, dim);
    k.fuse = 1; k.training = training; k.p = p;
    k.seed = seed; k.d_epoch = d_epoch; k.elem_offset = elem_offset; k.keep_mask = keep_mask;
    return graphsum_impl(c, g, k);
}

int gcnhip_graphsum_relu_dropout_bits(gcnhip_ctx *c, const gcnhip_graph *g, const float *in, int ld_in,
                                      float *out, int ld_out, int dim, int training, float p,
                                      uint64_t seed, const uint32_t *d_epoch, uint64_t elem_offset,
                                      const uint8_t *keep_mask, uint32_t *pos_bits, int words_per_row) {
    if (training && !(p >= 0.f && p < 1.f)) return -1;
    if (!pos_bits) return -1;
    GsCall k = gs_call(in, ld_in, out, ld_out, dim);
    k.fuse = 1; k.training = training; k.p = p;
    k.seed = seed; k.d_epoch = d_epoch; k.elem_offset = elem_offset; k.keep_mask = keep_mask;
    k.pos_bits = pos_bits; k.wpr = words_per_row;
    return graphsum_impl(c, g, k);
}

int gcnhip_graphsum_part(gcnhip_ctx *c, const gcnhip_graph *g, const gcnhip_rowset *rows, const float *in, int ld_in,
                         float *out, int ld_out, int dim, const uint32_t *in_row_bits, int accumulate,
                         int relu_dropout, int training, float p, uint64_t seed, const uint32_t *d_epoch,
                         uint64_t elem_offset, const uint8_t *keep_mask) {
    if (relu_dropout && training && !(p >= 0.f && p < 1.f)) return -1;
    GsCall k = gs_call(in, ld_in, out, ld_out, dim);
    k.fuse = relu_dropout ? 1 : 0; k.training = relu_dropout ? training : 0; k.p = relu_dropout ? p : 0.f;
    k.seed = seed; k.d_epoch = d_epoch; k.elem_offset = elem_offset; k.keep_mask = keep_mask;
    k.row_bits = in_row_bits; k.rs = rows; k.accumulate = accumulate ? 1 : 0;
    return graphsum_impl(c, g, k);
}

int gcnhip_graphsum_ex(gcnhip_ctx *c, const gcnhip_graph *g, const gcnhip_gs_opts *o, const float *in, int ld_in, float *out, int ld_out, int dim) {
    if (!o) return -1;
    if (o->relu_dropout && o->training && !(o->p >= 0.f && o->p < 1.f)) return -1;
    if (o->pos_bits && !o->relu_dropout) return -1;
    GsCall k = gs_call(in, ld_in, out, ld_out, dim);
    k.fuse = o->relu_dropout ? 1 : 0; k.training = o->relu_dropout ? o->training : 0; k.p = o->relu_dropout ? o->p : 0.f;
    k.seed = o->seed; k.d_epoch = o->d_epoch; k.elem_offset = o->elem_offset; k.keep_mask = o->keep_mask;
    k.row_bits = o->in_row_bits; k.rs = o->rows; k.accumulate = o->accumulate ? 1 : 0;
    k.pos_bits = o->pos_bits; k.wpr = o->words_per_row;
    k.scaling = o->scaling; k.loss = o->loss;
    return graphsum_impl(c, g, k);
}

int gcnhip_graphsum_predict(gcnhip_ctx *c, const gcnhip_graph *g, const gcnhip_rowset *rows, const float *in, const uint16_t *in_bf16,
                            int ld_in, float *out, int ld_out, int dim, int scaling, int32_t *pred, float *prob, float *logp, int ld_logp) {
    if (!pred || !prob || (in != nullptr) == (in_bf16 != nullptr)) return -1;
    if (logp && ld_logp < dim) return -1;
    if (in_bf16 && scaling) return gcnhip_fail("gcnhip_graphsum_predict: the factored operator (scaling != 0) gathers f32 rows only");
    const PredArgs pa = {pred, prob, logp, ld_logp};
    // (no logits stored: a stride that passes the 16-byte row test; nothing is written through it)
    GsCall k = gs_call(in, ld_in, out, out ? ld_out : (dim + 3) / 4 * 4, dim);
    k.in_bf = in_bf16; k.rs = rows; k.scaling = scaling; k.pred = &pa;
    return graphsum_impl(c, g, k);
}

int gcnhip_graphsum_blend(gcnhip_ctx *c, const gcnhip_graph *g, const float *in, int ld_in, const float *base, int ld_base,
                          float *out, int ld_out, int dim, float alpha, float beta, float lo, float hi, int32_t *pred) {
    if (!c || !g || !in || !base || !out) return gcnhip_fail("gcnhip_graphsum_blend: null argument");
    if (dim < 1 || dim > 64) return gcnhip_fail("gcnhip_graphsum_blend: 1 <= dim <= 64 (the row of a node sits in one lane group)");
    if (ld_in < dim || ld_base < dim || ld_out < dim || ld_in % 4 || ld_base % 4 || ld_out % 4 || !aligned16(in) || !aligned16(base) || !aligned16(out))
        return gcnhip_fail("gcnhip_graphsum_blend: needs f32 rows that are 16-byte aligned (ld % 4 == 0, ld >= dim)");
    if (out == in) return gcnhip_fail("gcnhip_graphsum_blend: out must not be in (other rows are still gathering it); base may be");
    if (g->n_rows == 0) return 0;
    if (gs_scratch_too_narrow(g, dim))
        return gcnhip_fail("gcnhip_graphsum_blend: dim is wider than the split-row scratch of this adjacency object; call gcnhip_graph_reserve_width");
    GsArgs a = {};
    const GsRows rows = gs_fill(a, g, nullptr, ld_in, 4);
    a.in = in; a.out = out;
    a.ld_in = ld_in; a.ld_out = ld_out; a.dim = dim;
    const int blocks = gs_bounds(a, rows.bounds, 1) * 8;
    const BlendArgs b = {base, ld_base, alpha, beta, lo, hi, pred};
    const int u = gs_batch_depth(c, a);
    const int d4 = (dim + 3) / 4;
    if (d4 <= 1) launch_blend<1>(a, b, blocks, u, c->stream);
    else if (d4 <= 2) launch_blend<2>(a, b, blocks, u, c->stream);
    else if (d4 <= 4) launch_blend<4>(a, b, blocks, u, c->stream);
    else if (d4 <= 8) launch_blend<8>(a, b, blocks, u, c->stream);
    else launch_blend<16>(a, b, blocks, u, c->stream);
    return gs_finish(rows.n_split_rows, [&] {
        graphsum_finalize_blend_kernel<<<rows.n_split_rows, WAVE, 0, c->stream>>>(a, b, rows.split_rows, rows.n_split_rows);
    });
}

int gcnhip_f32_to_bf16(gcnhip_ctx *c, const float *src, int ld_src, uint16_t *dst, int ld_dst, int64_t rows, int dim) {
    if (!c || !src || !dst || rows < 0 || dim <= 0 || ld_src < dim || ld_dst < dim || ld_dst % 8 != 0 || !aligned16(dst)) return -1;
    if (rows == 0) return 0;
    int64_t blocks = (rows * (ld_dst / 8) + 255) / 256;
    if (blocks > 65536) blocks = 65536;
    f32_to_bf16_kernel<<<(int)blocks, 256, 0, c->stream>>>(src, ld_src, dst, ld_dst, rows, dim);
    GCNHIP_LAUNCH_CHECK();
    return 0;
}

int gcnhip_graphsum_bf16(gcnhip_ctx *c, const gcnhip_graph *g, const uint16_t *in_bf16, int ld_in,
                         float *out, int ld_out, int dim, const uint32_t *in_row_bits, const gcnhip_rowset *out_rows,
                         int relu_dropout, int training, float p, uint64_t seed, const uint32_t *d_epoch,
                         uint64_t elem_offset, const uint8_t *keep_mask) {
    if (relu_dropout && training && !(p >= 0.f && p < 1.f)) return -1;
    GsCall k = gs_call(nullptr, ld_in, out, ld_out, dim);
    k.fuse = relu_dropout ? 1 : 0; k.training = training; k.p = relu_dropout ? p : 0.f;
    k.seed = seed; k.d_epoch = d_epoch; k.elem_offset = elem_offset; k.keep_mask = keep_mask;
    k.in_bf = in_bf16; k.row_bits = in_row_bits; k.rs = out_rows;
    return graphsum_impl(c, g, k);
}

}  // extern "C"

GCNHIP_DEFINE_PRELOAD(graphsum, graphsum_finalize_kernel)
