// louvain.hip — the graph's own grouping: multi-level Louvain (Blondel et al., 2008) with synchronous, deterministic local moving.
// Beyond the reference, which never looks at its adjacency after building it.  Every decision is made in exact integer
// arithmetic, so any grid, lane group, cut and hash size give the same labels, and tests/louvain_ref.py (the same definitions in
// Python integers and dicts) agrees label for label.
//
// DEFINITIONS (the contract)
//   A LEVEL is a weighted graph on n vertices: row pointers ptr int32 [n + 1]; len int32 [n] (NULL: ptr[v + 1] - ptr[v]) — row v is
//     idx[ptr[v] .. ptr[v] + len[v]), the form gcnhip_overlap_sets leaves; idx int32, distinct per row, no self entry; w uint32 > 0
//     (NULL: 1); self_w int64 per vertex (NULL: 0).  Level 0 is the canonical sets S(v) of overlap.hip with w = 1, self_w = 0.  No
//     transpose is built: a one-way entry counts in one row only, and the quantity below is the textbook modularity exactly when the
//     stored graph is symmetric.  Nothing checks that.
//   k[v] = self_w[v] + sum w(v, .);  M2 = sum k (< 2^31: `entries` of 2^31 or more are refused);  for a labelling comm:
//     tot[c] = sum of k over c;  in[c] = sum over v in c of (self_w[v] + sum of w(v, u), u in c);
//     num = M2 . sum in - sum tot^2, an exact int64 (both terms <= 2^62);  Q = num / M2^2 is formed on the host.
//   A SWEEP s = 0, 1, .. is synchronous: every vertex reads comm, tot and size as they stood at its start.  For v in community a the
//     candidates are the c != a with K(v, c) = sum of w(v, u), comm[u] = c, positive; only c > a on even s and c < a on odd s; not
//     when size[a] = 1, size[c] = 1 and c > a (two lone vertices never trade places).  gain(c) = K(v, c) . M2 - k[v] . tot[c];
//     stay = K(v, a) . M2 - k[v] . (tot[a] - k[v]).  v moves to the candidate of largest gain, ties to the smallest c, iff that gain
//     is strictly greater than stay.  After the moves tot, size and num are recomputed; a sweep after which num did not strictly
//     rise is undone.  A level starts from singletons and ends after two undone sweeps in a row or max_sweeps sweeps.
//   COARSENING: communities are renumbered by ascending smallest member; w(C, D) = sum of w(v, u), v in C, u in D, C != D;
//     self_w[C] = in[C]; rows sorted and duplicate-free again.  The coarse level is ragged like level 0: row C has room for
//     bound[C] = min(sum of its members' row lengths, coarse vertices - 1) entries, c_ptr = the prefix sums of bound, c_len the
//     entries it holds.  So one pass writes it, and its extent never exceeds the finer level's.
//
// THE MOVE (the hot path).  K(v, .) is accumulated in an open-addressing hash table keyed by community, sized to the next power of
//   two >= 2 x row length, with atomic adds of the uint32 weights; the owners then scan their own table for the arg-max.  Sums are
//   integers and the arg-max has a total order, so no insertion order shows.  Three row classes by length, listed once per level:
//     up to the group's share: a lane group of G lanes per vertex (G = 4, 16 or 64 by the mean row length: structure.hip's rule),
//       the table is the group's slice of the workgroup's LDS (4096 slots of {key, sum} between 256 / G groups), ds atomics;
//     up to half the workgroup table (default: the largest power of two the device's LDS holds, at most 16384 slots): a
//       workgroup per row, the table is all of its LDS;
//     longer: one workgroup takes them one after another with the table in global memory (the scratch).
//   The kernels write next[v] only.  The commit walk (structure.hip's idiom: registers, shuffles, LDS, one 64-bit atomic per
//   workgroup and total) adds k into the new tot and size, counts the moves and sums `in`; a pass over communities sums tot^2.  The
//   host reads three scalars per sweep and accepts by exchanging the two sets of arrays, or leaves them (the undo).
// COARSENING stays on the GPU: the smallest member by atomicMin, a flag-and-scan renumbering, a counting sort of the vertices by
//   label, then a workgroup per coarse row merges its members' entries in an LDS hash table keyed by coarse label (the diagonal
//   peeled into self_w) and sorts the table in place by a bitonic network with the empty key last.  gcnhip_sort_segments_u32 was
//   not used: it orders u32 keys without a payload, and a (C, D) key needs up to 62 bits beside its weight.  A coarse row whose
//   bound is above half the table is merged in a dense array of one uint32 per coarse vertex in global memory, one such row after
//   another, and compacted in index order.  Only the vertex count and the extent cross to the host.
// The entry points allocate nothing; the level call synchronises to read the sweep's scalars, the coarsening once, before its merge
// launches, for the coarse vertex count, the extent and the LDS the merge needs.
#include "common.h"
#include <algorithm>
#include <cstdio>

constexpr int LV_THREADS = 256, LV_WAVES = LV_THREADS / WAVE;
constexpr int LV_BLOCKS_PER_CU = 4;
constexpr int LV_GROUP_TABLE = 4096;                           // slots the lane groups of a workgroup share
constexpr int LV_MAX_TABLE = 16384, LV_MIN_TABLE = 256;        // the workgroup's table, slots
constexpr int LV_EMPTY = 0x7FFFFFFF;                           // no community has this key; sorts last
constexpr int LV_SCAN_THREADS = 1024, LV_SCAN_ITEMS = 4;

struct LvLevel {
    const int *__restrict__ ptr;
    const int32_t *__restrict__ len;
    const int *__restrict__ idx;
    const unsigned *__restrict__ w;
    const long long *__restrict__ self_w;
    int n;
};
__device__ inline int lv_len(const LvLevel &L, int v) { return L.len ? L.len[v] : L.ptr[v + 1] - L.ptr[v]; }
__device__ inline unsigned lv_w(const LvLevel &L, int e) { return L.w ? L.w[e] : 1u; }
__device__ inline long long lv_self(const LvLevel &L, int v) { return L.self_w ? L.self_w[v] : 0; }

// acc: {M2, sum in, sum tot^2, moved, workgroup rows, long rows, the longest workgroup row}
enum { LV_M2 = 0, LV_IN = 1, LV_TOT2 = 2, LV_MOVED = 3, LV_NWG = 4, LV_NLONG = 5, LV_WGMAX = 6, LV_ACC = 8 };

// registers -> shuffles -> LDS -> one 64-bit atomic per workgroup and total
template <int NV>
__device__ inline void lv_totals(const unsigned long long (&x)[NV], unsigned long long *__restrict__ dst) {
    __shared__ unsigned long long blk[NV];
    if (threadIdx.x < NV) blk[threadIdx.x] = 0;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < NV; k++) {
        unsigned long long s = x[k];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, WAVE);
        if ((threadIdx.x & (WAVE - 1)) == 0 && s) atomicAdd(&blk[k], s);
    }
    __syncthreads();
    if (threadIdx.x < NV && blk[threadIdx.x]) atomicAdd(&dst[threadIdx.x], blk[threadIdx.x]);
}

template <int G>
__device__ inline unsigned long long lv_group_sum(unsigned long long s) {
#pragma unroll
    for (int off = G / 2; off > 0; off >>= 1) s += __shfl_xor(s, off, WAVE);
    return s;
}

// ---- a level's start: k, singletons, the row classes ---------------------------------------------------------------------------
template <int G>
__global__ __launch_bounds__(LV_THREADS) void lv_init_kernel(LvLevel L, long long *__restrict__ k, long long *__restrict__ tot, int *__restrict__ comm,
                                                             int *__restrict__ size, int *__restrict__ wg_list, int *__restrict__ long_list, int group_cut,
                                                             int wg_max, unsigned long long *__restrict__ acc) {
    const int gl = threadIdx.x & (G - 1), gid = threadIdx.x / G;
    unsigned long long x[3] = {0, 0, 0};
    for (int64_t base = (int64_t)blockIdx.x * (LV_THREADS / G); base < L.n; base += (int64_t)gridDim.x * (LV_THREADS / G)) {
        const int64_t v64 = base + gid;
        if (v64 >= L.n) continue;                              // no barrier below
        const int v = (int)v64, e0 = L.ptr[v], len = lv_len(L, v);
        unsigned long long s = 0;
        for (int e = gl; e < len; e += G) s += lv_w(L, e0 + e);
        s = lv_group_sum<G>(s);
        if (gl) continue;
        const long long self = lv_self(L, v), kv = self + (long long)s;
        k[v] = kv; tot[v] = kv; comm[v] = v; size[v] = 1;
        x[0] += (unsigned long long)kv;
        x[1] += (unsigned long long)self;
        x[2] += (unsigned long long)kv * (unsigned long long)kv;
        if (len > wg_max) long_list[atomicAdd(&acc[LV_NLONG], 1ull)] = v;
        else if (len > group_cut) {
            wg_list[atomicAdd(&acc[LV_NWG], 1ull)] = v;
            atomicMax(&acc[LV_WGMAX], (unsigned long long)len);
        }
    }
    const unsigned long long y[3] = {x[0], x[1], x[2]};
    lv_totals<3>(y, acc);
}

__global__ void lv_clear_kernel(long long *__restrict__ tot, int *__restrict__ size, int n, unsigned long long *__restrict__ acc, int acc0, int acc1) {
    const int64_t i0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (int64_t i = i0; i < n; i += (int64_t)gridDim.x * blockDim.x) { tot[i] = 0; size[i] = 0; }
    if (i0 >= acc0 && i0 < acc1) acc[i0] = 0;
}

// ---- the move ------------------------------------------------------------------------------------------------------------------
struct LvMove {
    LvLevel L;
    const int *__restrict__ comm;
    const long long *__restrict__ tot, *__restrict__ k;
    const int *__restrict__ size;
    int *__restrict__ next;
    long long m2;
    int odd, group_cut, slice;
};

struct LvBest {
    long long gain;
    int c;                                                     // LV_EMPTY: none
    unsigned long long ka;                                     // K(v, a), with the lane that met a
};

__device__ inline unsigned lv_hash(int c) {
    const unsigned h = (unsigned)c * 0x9E3779B1u;
    return h ^ (h >> 15);
}
// keys / vals are LDS or global; the table holds fewer keys than half its slots, so the probe ends
template <class K, class V>
__device__ inline void lv_insert(K *keys, V *vals, unsigned mask, int c, unsigned w) {
    unsigned h = lv_hash(c) & mask;
    for (;;) {
        const int prev = atomicCAS(&keys[h], LV_EMPTY, c);
        if (prev == LV_EMPTY || prev == c) { atomicAdd(&vals[h], w); return; }
        h = (h + 1) & mask;
    }
}
__device__ inline int lv_table(int len) {                    // len < 2^30: gcnhip_louvain_plan refuses a level whose rows could be longer
    int P = 2;
    while (P < 2 * len) P <<= 1;
    return P;
}
__device__ inline void lv_better(LvBest &b, long long gain, int c) {
    if (c != LV_EMPTY && (b.c == LV_EMPTY || gain > b.gain || (gain == b.gain && c < b.c))) { b.gain = gain; b.c = c; }
}
template <int W>
__device__ inline LvBest lv_reduce(LvBest b) {
#pragma unroll
    for (int off = W / 2; off > 0; off >>= 1) {
        const long long g = __shfl_xor(b.gain, off, WAVE);
        const int c = __shfl_xor(b.c, off, WAVE);
        b.ka += __shfl_xor(b.ka, off, WAVE);
        lv_better(b, g, c);
    }
    return b;
}
// W lanes put row v's entries into the table
template <int W, class K, class V>
__device__ inline void lv_fill(const LvMove &g, int e0, int len, K *keys, V *vals, unsigned mask, int lane) {
    for (int e = lane; e < len; e += W) lv_insert(keys, vals, mask, g.comm[g.L.idx[e0 + e]], lv_w(g.L, e0 + e));
}
// W lanes scan the table's P slots: this lane's best candidate and K(v, a)
template <int W, class K, class V>
__device__ inline LvBest lv_scan_table(const LvMove &g, int a, long long kv, const K *keys, const V *vals, int P, int lane) {
    LvBest b = {0, LV_EMPTY, 0};
    const bool lone = g.size[a] == 1;
    for (int i = lane; i < P; i += W) {
        const int c = keys[i];
        if (c == LV_EMPTY) continue;
        if (c == a) { b.ka = vals[i]; continue; }
        if (g.odd ? c > a : c < a) continue;
        if (lone && c > a && g.size[c] == 1) continue;
        lv_better(b, (long long)vals[i] * g.m2 - kv * g.tot[c], c);
    }
    return b;
}
__device__ inline void lv_decide(const LvMove &g, int v, int a, long long kv, const LvBest &b) {
    const long long stay = (long long)b.ka * g.m2 - kv * (g.tot[a] - kv);
    g.next[v] = b.c != LV_EMPTY && b.gain > stay ? b.c : a;
}

template <int G>
__global__ __launch_bounds__(LV_THREADS) void lv_move_group_kernel(LvMove g) {
    extern __shared__ int lv_lds[];                            // [256 / G slices of {slice keys | slice sums}]
    const int gl = threadIdx.x & (G - 1), gid = threadIdx.x / G;
    int *keys = lv_lds + gid * 2 * g.slice;
    unsigned *vals = (unsigned *)(keys + g.slice);
    for (int64_t base = (int64_t)blockIdx.x * (LV_THREADS / G); base < g.L.n; base += (int64_t)gridDim.x * (LV_THREADS / G)) {
        const int64_t v64 = base + gid;
        const int v = (int)(v64 < g.L.n ? v64 : -1);
        int len = v >= 0 ? lv_len(g.L, v) : 0;
        if (len > g.group_cut) len = -1;                       // a workgroup's or a long row: not ours
        if (v >= 0 && len == 0 && gl == 0) g.next[v] = g.comm[v];
        const int P = len > 0 ? lv_table(len) : 0, e0 = len > 0 ? g.L.ptr[v] : 0;
        for (int i = gl; i < P; i += G) { keys[i] = LV_EMPTY; vals[i] = 0; }
        __syncthreads();
        if (len > 0) lv_fill<G>(g, e0, len, keys, vals, (unsigned)P - 1u, gl);
        __syncthreads();
        if (len > 0) {
            const int a = g.comm[v];
            const long long kv = g.k[v];
            const LvBest b = lv_reduce<G>(lv_scan_table<G>(g, a, kv, keys, vals, P, gl));
            if (gl == 0) lv_decide(g, v, a, kv, b);
        }
        __syncthreads();                                       // the slices are free again
    }
}

// a workgroup per listed row; GLOBAL: the table is gkeys / gvals and the grid is one workgroup
template <bool GLOBAL>
__global__ __launch_bounds__(LV_THREADS) void lv_move_wg_kernel(LvMove g, const int *__restrict__ list, int count, int table, int *gkeys, unsigned *gvals) {
    extern __shared__ int lv_lds[];
    __shared__ LvBest wave_best[LV_WAVES];
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
    for (int i = blockIdx.x; i < count; i += gridDim.x) {
        const int v = list[i], e0 = g.L.ptr[v], len = lv_len(g.L, v), P = lv_table(len), a = g.comm[v];
        const long long kv = g.k[v];
        LvBest b;
        if (GLOBAL) {
            for (int s = threadIdx.x; s < P; s += LV_THREADS) { gkeys[s] = LV_EMPTY; gvals[s] = 0; }
            __syncthreads();
            lv_fill<LV_THREADS>(g, e0, len, gkeys, gvals, (unsigned)P - 1u, threadIdx.x);
            __syncthreads();
            b = lv_scan_table<LV_THREADS>(g, a, kv, gkeys, gvals, P, threadIdx.x);
        } else {
            int *keys = lv_lds;
            unsigned *vals = (unsigned *)(lv_lds + table);
            for (int s = threadIdx.x; s < P; s += LV_THREADS) { keys[s] = LV_EMPTY; vals[s] = 0; }
            __syncthreads();
            lv_fill<LV_THREADS>(g, e0, len, keys, vals, (unsigned)P - 1u, threadIdx.x);
            __syncthreads();
            b = lv_scan_table<LV_THREADS>(g, a, kv, keys, vals, P, threadIdx.x);
        }
        b = lv_reduce<WAVE>(b);
        if (lane == 0) wave_best[wave] = b;
        __syncthreads();
        if (threadIdx.x == 0) {
            for (int w = 1; w < LV_WAVES; w++) {
                b.ka += wave_best[w].ka;
                lv_better(b, wave_best[w].gain, wave_best[w].c);
            }
            lv_decide(g, v, a, kv, b);
        }
        __syncthreads();                                       // the table and wave_best are free again
    }
}

// ---- the commit walk: the new tot and size, the moves, sum in --------------------------------------------------------------------
template <int G>
__global__ __launch_bounds__(LV_THREADS) void lv_commit_kernel(LvLevel L, const int *__restrict__ comm, const int *__restrict__ next, const long long *__restrict__ k,
                                                               long long *__restrict__ tot, int *__restrict__ size, unsigned long long *__restrict__ acc) {
    const int gl = threadIdx.x & (G - 1), gid = threadIdx.x / G;
    unsigned long long x[3] = {0, 0, 0};                       // {in, -, moved}
    for (int64_t base = (int64_t)blockIdx.x * (LV_THREADS / G); base < L.n; base += (int64_t)gridDim.x * (LV_THREADS / G)) {
        const int64_t v64 = base + gid;
        if (v64 >= L.n) continue;
        const int v = (int)v64, e0 = L.ptr[v], len = lv_len(L, v), c = next[v];
        unsigned long long s = 0;
        for (int e = gl; e < len; e += G)
            if (next[L.idx[e0 + e]] == c) s += lv_w(L, e0 + e);
        x[0] += s;                                             // every lane's share: the totals add them
        if (gl) continue;
        x[0] += (unsigned long long)lv_self(L, v);
        x[2] += c != comm[v];
        atomicAdd((unsigned long long *)&tot[c], (unsigned long long)k[v]);
        atomicAdd(&size[c], 1);
    }
    const unsigned long long y[3] = {x[0], 0, x[2]};
    lv_totals<3>(y, acc + LV_IN);
}

__global__ __launch_bounds__(LV_THREADS) void lv_tot2_kernel(const long long *__restrict__ tot, int n, unsigned long long *__restrict__ acc) {
    unsigned long long x[1] = {0};
    for (int64_t i = (int64_t)blockIdx.x * LV_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * LV_THREADS)
        x[0] += (unsigned long long)tot[i] * (unsigned long long)tot[i];
    const unsigned long long y[1] = {x[0]};
    lv_totals<1>(y, acc + LV_TOT2);
}

__global__ void lv_copy_kernel(const int *__restrict__ comm, int *__restrict__ comm_out, const long long *__restrict__ tot, long long *__restrict__ tot_out, int n) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        if (comm_out != comm) comm_out[i] = comm[i];
        if (tot_out != tot) tot_out[i] = tot[i];
    }
}

// ---- coarsening ------------------------------------------------------------------------------------------------------------------
// out[i] = in[0] + .. + in[i - 1] for i <= n; one workgroup, in place allowed (a thread writes only what it read)
__global__ __launch_bounds__(LV_SCAN_THREADS) void lv_scan_kernel(const int *in, int *out, int n) {
    __shared__ int wave_sum_s[LV_SCAN_THREADS / WAVE];
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
    int carry = 0;
    for (int64_t base = 0; base < n; base += LV_SCAN_THREADS * LV_SCAN_ITEMS) {
        const int64_t i0 = base + (int64_t)threadIdx.x * LV_SCAN_ITEMS;
        int x[LV_SCAN_ITEMS], s = 0;
#pragma unroll
        for (int j = 0; j < LV_SCAN_ITEMS; j++) { x[j] = i0 + j < n ? in[i0 + j] : 0; s += x[j]; }
        int incl = s;
#pragma unroll
        for (int off = 1; off < WAVE; off <<= 1) {
            const int y = __shfl_up(incl, off, WAVE);
            if (lane >= off) incl += y;
        }
        if (lane == WAVE - 1) wave_sum_s[wave] = incl;
        __syncthreads();
        int before = carry + incl - s, total = 0;
        for (int w = 0; w < LV_SCAN_THREADS / WAVE; w++) {
            if (w < wave) before += wave_sum_s[w];
            total += wave_sum_s[w];
        }
#pragma unroll
        for (int j = 0; j < LV_SCAN_ITEMS; j++) {
            if (i0 + j < n) out[i0 + j] = before;
            before += x[j];
        }
        carry += total;
        __syncthreads();
    }
    if (threadIdx.x == 0) out[n] = carry;
}

struct LvCoarse {
    LvLevel L;
    const int *__restrict__ comm;
    int *__restrict__ label;                                   // out: the renumbered community of every vertex
    int *__restrict__ minv, *__restrict__ rank, *__restrict__ off, *__restrict__ room, *__restrict__ cursor, *__restrict__ members, *__restrict__ long_list;
    unsigned *__restrict__ dense;
    int *__restrict__ n_long;                                  // {long rows, the largest room of the others}
    int *__restrict__ c_ptr, *__restrict__ c_len, *__restrict__ c_idx;
    unsigned *__restrict__ c_w;
    long long *__restrict__ c_self;
    int table, merge_slots;                                    // rows with room above table / 2 are the dense kernel's; the merge launch's LDS
};

__global__ void lv_coarse_init_kernel(LvCoarse g) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i <= g.L.n; i += (int64_t)gridDim.x * blockDim.x) {
        g.minv[i] = LV_EMPTY; g.off[i] = 0; g.room[i] = 0; g.cursor[i] = 0;
        if (i == 0) { g.n_long[0] = 0; g.n_long[1] = 0; }
    }
}
__global__ void lv_coarse_min_kernel(LvCoarse g) {
    for (int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; v < g.L.n; v += (int64_t)gridDim.x * blockDim.x) atomicMin(&g.minv[g.comm[v]], (int)v);
}
__global__ void lv_coarse_flag_kernel(LvCoarse g) {
    for (int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; v < g.L.n; v += (int64_t)gridDim.x * blockDim.x) g.rank[v] = g.minv[g.comm[v]] == v;
}
__global__ void lv_coarse_label_kernel(LvCoarse g) {
    for (int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; v < g.L.n; v += (int64_t)gridDim.x * blockDim.x) {
        const int C = g.rank[g.minv[g.comm[v]]];
        g.label[v] = C;
        atomicAdd(&g.off[C], 1);
        atomicAdd(&g.room[C], lv_len(g.L, (int)v));
    }
}
__global__ void lv_coarse_bound_kernel(LvCoarse g) {
    const int nc = g.rank[g.L.n];
    for (int64_t C = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; C < nc; C += (int64_t)gridDim.x * blockDim.x) {
        const int bound = min(g.room[C], nc - 1);
        g.room[C] = bound;
        if (bound > g.table / 2) g.long_list[atomicAdd(g.n_long, 1)] = (int)C;
        else atomicMax(g.n_long + 1, bound);
    }
}
__global__ void lv_coarse_members_kernel(LvCoarse g) {
    for (int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; v < g.L.n; v += (int64_t)gridDim.x * blockDim.x) {
        const int C = g.label[v];
        g.members[g.off[C] + atomicAdd(&g.cursor[C], 1)] = (int)v;
    }
}

// the waves take C's members in turn and pass every entry to visit(D, w); returns this thread's share of the diagonal
template <class F>
__device__ inline unsigned long long lv_coarse_walk(const LvCoarse &g, int C, F visit) {
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
    const int m0 = g.off[C], m1 = g.off[C + 1];
    unsigned long long diag = 0;
    for (int m = m0 + wave; m < m1; m += LV_WAVES) {
        const int v = g.members[m], e0 = g.L.ptr[v], len = lv_len(g.L, v);
        if (lane == 0) diag += (unsigned long long)lv_self(g.L, v);
        for (int e = lane; e < len; e += WAVE) {
            const int D = g.label[g.L.idx[e0 + e]];
            const unsigned w = lv_w(g.L, e0 + e);
            if (D == C) diag += w;
            else visit(D, w);
        }
    }
    return diag;
}
// the workgroup's sum of diag goes to c_self[C]; block_sum is the caller's LDS cell, zero on entry and on return
__device__ inline void lv_coarse_self(const LvCoarse &g, int C, unsigned long long diag, unsigned long long *block_sum) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) diag += __shfl_xor(diag, off, WAVE);
    if ((threadIdx.x & (WAVE - 1)) == 0 && diag) atomicAdd(block_sum, diag);
    __syncthreads();
    if (threadIdx.x == 0) { g.c_self[C] = (long long)*block_sum; *block_sum = 0; }
    __syncthreads();
}

__global__ __launch_bounds__(LV_THREADS) void lv_coarse_merge_kernel(LvCoarse g) {
    extern __shared__ int lv_lds[];
    __shared__ unsigned long long block_sum;
    int *keys = lv_lds;
    unsigned *vals = (unsigned *)(lv_lds + g.merge_slots);
    if (threadIdx.x == 0) block_sum = 0;
    const int nc = g.rank[g.L.n];
    for (int C = blockIdx.x; C < nc; C += gridDim.x) {
        const int p0 = g.c_ptr[C], bound = g.c_ptr[C + 1] - p0;
        if (bound > g.table / 2) continue;                     // uniform: the dense kernel's
        const int P = lv_table(bound);
        __syncthreads();                                       // the row before is out of LDS
        for (int s = threadIdx.x; s < P; s += LV_THREADS) { keys[s] = LV_EMPTY; vals[s] = 0; }
        __syncthreads();
        const unsigned long long diag = lv_coarse_walk(g, C, [&](int D, unsigned w) { lv_insert(keys, vals, (unsigned)P - 1u, D, w); });
        lv_coarse_self(g, C, diag, &block_sum);
        for (int k = 2; k <= P; k <<= 1)                       // the table in place, the empty key last
            for (int j = k >> 1; j > 0; j >>= 1) {
                __syncthreads();
                for (int i = threadIdx.x; i < P; i += LV_THREADS) {
                    const int p = i ^ j;
                    if (p > i) {
                        const int a = keys[i], b = keys[p];
                        if ((a > b) == ((i & k) == 0)) {
                            const unsigned va = vals[i], vb = vals[p];
                            keys[i] = b; keys[p] = a; vals[i] = vb; vals[p] = va;
                        }
                    }
                }
            }
        __syncthreads();
        if (threadIdx.x == 0 && keys[0] == LV_EMPTY) g.c_len[C] = 0;
        for (int i = threadIdx.x; i < P; i += LV_THREADS) {
            if (keys[i] == LV_EMPTY) continue;
            g.c_idx[p0 + i] = keys[i];
            g.c_w[p0 + i] = vals[i];
            if (i == P - 1 || keys[i + 1] == LV_EMPTY) g.c_len[C] = i + 1;
        }
    }
}

// one workgroup: the long coarse rows one after another in the dense array, compacted in index order
__global__ __launch_bounds__(LV_THREADS) void lv_coarse_dense_kernel(LvCoarse g) {
    __shared__ unsigned long long block_sum;
    __shared__ int wave_kept[LV_WAVES];
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
    if (threadIdx.x == 0) block_sum = 0;
    const int nc = g.rank[g.L.n], n_long = *g.n_long;
    for (int r = 0; r < n_long; r++) {
        const int C = g.long_list[r], p0 = g.c_ptr[C];
        __syncthreads();
        for (int s = threadIdx.x; s < nc; s += LV_THREADS) g.dense[s] = 0;
        __syncthreads();
        const unsigned long long diag = lv_coarse_walk(g, C, [&](int D, unsigned w) { atomicAdd(&g.dense[D], w); });
        lv_coarse_self(g, C, diag, &block_sum);
        int base = 0;
        for (int d0 = 0; d0 < nc; d0 += LV_THREADS) {          // uniform over the workgroup
            const int D = d0 + threadIdx.x;
            const unsigned w = D < nc ? g.dense[D] : 0u;
            const unsigned long long kept = __ballot(w != 0);
            if (lane == 0) wave_kept[wave] = __popcll(kept);
            __syncthreads();
            int at = base;
            for (int k = 0; k < wave; k++) at += wave_kept[k];
            if (w) {
                at += __popcll(kept & ((1ull << lane) - 1ull));
                g.c_idx[p0 + at] = D;
                g.c_w[p0 + at] = w;
            }
            for (int k = 0; k < LV_WAVES; k++) base += wave_kept[k];
            __syncthreads();
        }
        if (threadIdx.x == 0) g.c_len[C] = base;
    }
}

__global__ void lv_compose_kernel(int *__restrict__ labels, int n, const int *__restrict__ label, int n_label) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int c = labels[i];
        if ((unsigned)c < (unsigned)n_label) labels[i] = label[c];
    }
}

namespace {

int lv_refuse(const char *name, const char *why) {
    char msg[200];
    snprintf(msg, sizeof msg, "%s: %s", name, why);
    return gcnhip_fail(msg);
}

int64_t lv_r16(int64_t bytes) { return (bytes + 15) & ~(int64_t)15; }
int64_t lv_global_table(int n, int64_t entries) {
    int64_t t = 2;
    while (t < 2 * std::max<int64_t>(1, std::min<int64_t>(entries, n))) t <<= 1;
    return t;
}
int64_t lv_level_bytes(int n, int64_t entries) { return 64 + 2 * lv_r16(8 * (int64_t)n) + 5 * lv_r16(4 * (int64_t)n) + 2 * lv_r16(4 * lv_global_table(n, entries)); }
int64_t lv_coarse_bytes(int n) { return 64 + 8 * lv_r16(4 * ((int64_t)n + 1)); }

const char *lv_shape_refusal(int n, int64_t entries) {
    if (n < 0 || entries < 0) return "invalid argument";
    if (entries >= ((int64_t)1 << 31)) return "2^31 stored entries or more (M2 must stay below 2^31)";
    if (std::min<int64_t>(entries, n) >= ((int64_t)1 << 30)) return "a row could hold 2^30 entries or more (a table's slots are counted in 32 bits)";
    return nullptr;
}

struct Carve {
    char *p;
    template <class T>
    T *take(int64_t count) {
        T *out = (T *)p;
        p += lv_r16(count * (int64_t)sizeof(T));
        return out;
    }
};

int lv_default_table(const gcnhip_ctx *c) {
    int cap = 0;
    if (hipDeviceGetAttribute(&cap, hipDeviceAttributeMaxSharedMemoryPerBlock, c->device) != hipSuccess || cap <= 0) cap = 64 << 10;
    int t = LV_MAX_TABLE;
    while (t > LV_MIN_TABLE && (int64_t)t * 8 + 512 > cap) t >>= 1;
    return t;
}
int lv_table_arg(gcnhip_ctx *c, const char *name, int table, int *out) {
    const int dflt = lv_default_table(c);
    if (table == 0) table = dflt;
    if (table < LV_MIN_TABLE || table > dflt || (table & (table - 1)))
        return lv_refuse(name, "the table is 0 (the default) or a power of two from 256 slots to what the device's LDS holds (at most 16384)");
    *out = table;
    return 0;
}
int lv_slots(int64_t len) {                                    // the table a row of len entries needs, at least a wave's worth
    int P = WAVE;
    while (P < 2 * len) P <<= 1;
    return P;
}
int lv_group_rule(int n, int64_t entries) {
    const int64_t mean = n > 0 ? entries / n : 0;
    return mean <= 16 ? 4 : (mean <= 128 ? 16 : 64);
}
template <class K>
int lv_big_lds(K kernel, size_t lds) {
    if (lds > (size_t)(48 << 10)) GCNHIP_TRY(hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    return 0;
}

}  // namespace

extern "C" {

int gcnhip_louvain_plan(int n, int64_t entries, int64_t *scratch_bytes) {
    const char *name = "gcnhip_louvain_plan";
    if (!scratch_bytes) return lv_refuse(name, "invalid argument");
    if (const char *why = lv_shape_refusal(n, entries)) return lv_refuse(name, why);
    *scratch_bytes = std::max(lv_level_bytes(n, entries), lv_coarse_bytes(n));
    return 0;
}

int gcnhip_louvain_level_ex(gcnhip_ctx *c, int n, int64_t entries, const int32_t *ptr, const int32_t *len, const int32_t *idx, const uint32_t *w,
                            const int64_t *self_w, int max_sweeps, int32_t *comm, int64_t *tot, int64_t *info, void *scratch, int64_t scratch_bytes,
                            int group, int wg_cut, int table) {
    const char *name = "gcnhip_louvain_level";
    if (!c || !info || max_sweeps < 0) return lv_refuse(name, "invalid argument");
    if (const char *why = lv_shape_refusal(n, entries)) return lv_refuse(name, why);
    if (n > 0 && (!ptr || !comm || !tot || (entries > 0 && !idx))) return lv_refuse(name, "invalid argument");
    if (group != 0 && group != 4 && group != 16 && group != 64) return lv_refuse(name, "the lane group is 0 (by the mean row length), 4, 16 or 64");
    if (wg_cut < 0) return lv_refuse(name, "the workgroup cut is 0 (the default) or positive");
    if (lv_table_arg(c, name, table, &table) != 0) return -1;
    if (!scratch || scratch_bytes < lv_level_bytes(n, entries) || !aligned16(scratch)) return lv_refuse(name, "the scratch is below what gcnhip_louvain_plan tells, or not 16-byte aligned");
    std::fill(info, info + 8, (int64_t)0);
    if (n == 0) return 0;
    if (!group) group = lv_group_rule(n, entries);
    const int group_table = std::min(table, LV_GROUP_TABLE), slice = group_table / (LV_THREADS / group);
    const int group_cut = wg_cut ? std::min(wg_cut, slice / 2) : slice / 2;

    Carve cv = {(char *)scratch};
    unsigned long long *acc = cv.take<unsigned long long>(LV_ACC);
    long long *k = cv.take<long long>(n), *tot_b = cv.take<long long>(n), *tot_a = (long long *)tot;
    int *comm_a = comm, *comm_b = cv.take<int>(n), *size_a = cv.take<int>(n), *size_b = cv.take<int>(n);
    int *wg_list = cv.take<int>(n), *long_list = cv.take<int>(n);
    const int64_t gt = lv_global_table(n, entries);
    int *gkeys = cv.take<int>(gt);
    unsigned *gvals = cv.take<unsigned>(gt);

    const LvLevel L = {ptr, len, idx, w, (const long long *)self_w, n};
    const int blocks = std::max(c->n_cu, 1) * LV_BLOCKS_PER_CU, flat = std::min(ceil_div(n, LV_THREADS), blocks);
    const int row_grid = std::min(ceil_div(n, LV_THREADS / group), blocks);
    hipStream_t st = c->stream;
    lv_clear_kernel<<<1, 64, 0, st>>>(nullptr, nullptr, 0, acc, 0, LV_ACC);
    GCNHIP_LAUNCH_CHECK();
#define LV_BY_GROUP(KERNEL, GRID, LDS, ...)                                          \
    do {                                                                               \
        if (group == 4) KERNEL<4><<<GRID, LV_THREADS, LDS, st>>>(__VA_ARGS__);         \
        else if (group == 16) KERNEL<16><<<GRID, LV_THREADS, LDS, st>>>(__VA_ARGS__);  \
        else KERNEL<64><<<GRID, LV_THREADS, LDS, st>>>(__VA_ARGS__);                   \
        GCNHIP_LAUNCH_CHECK();                                                         \
    } while (0)
    LV_BY_GROUP(lv_init_kernel, row_grid, 0, L, k, tot_a, comm_a, size_a, wg_list, long_list, group_cut, table / 2, acc);
    unsigned long long h[LV_ACC];
    GCNHIP_TRY(hipMemcpyAsync(h, acc, sizeof h, hipMemcpyDeviceToHost, st));
    GCNHIP_TRY(hipStreamSynchronize(st));
    const long long m2 = (long long)h[LV_M2];
    long long num = m2 * (long long)h[LV_IN] - (long long)h[LV_TOT2];
    const int n_wg = (int)h[LV_NWG], n_long = (int)h[LV_NLONG];
    const int wg_table = lv_slots((int64_t)h[LV_WGMAX]);       // the launch's LDS by the longest listed row, not by the cut
    const size_t wg_lds = (size_t)wg_table * 8, group_lds = (size_t)group_table * 8;
    if (n_wg > 0 && lv_big_lds(lv_move_wg_kernel<false>, wg_lds) != 0) return lv_refuse(name, "the workgroup table does not fit the device's LDS");
    int sweeps = 0, undone = 0, moved_any = 0;
    long long sum_in = (long long)h[LV_IN], sum_tot2 = (long long)h[LV_TOT2];
    while (m2 > 0 && sweeps < max_sweeps && undone < 2) {
        lv_clear_kernel<<<flat, LV_THREADS, 0, st>>>(tot_b, size_b, n, acc, LV_IN, LV_MOVED + 1);
        GCNHIP_LAUNCH_CHECK();
        LvMove g = {L, comm_a, tot_a, k, size_a, comm_b, m2, sweeps & 1, group_cut, slice};
        LV_BY_GROUP(lv_move_group_kernel, row_grid, group_lds, g);
        if (n_wg > 0) {
            lv_move_wg_kernel<false><<<std::min(n_wg, blocks), LV_THREADS, wg_lds, st>>>(g, wg_list, n_wg, wg_table, nullptr, nullptr);
            GCNHIP_LAUNCH_CHECK();
        }
        if (n_long > 0) {
            lv_move_wg_kernel<true><<<1, LV_THREADS, 0, st>>>(g, long_list, n_long, 0, gkeys, gvals);
            GCNHIP_LAUNCH_CHECK();
        }
        LV_BY_GROUP(lv_commit_kernel, row_grid, 0, L, comm_a, comm_b, k, tot_b, size_b, acc);
        lv_tot2_kernel<<<flat, LV_THREADS, 0, st>>>(tot_b, n, acc);
        GCNHIP_LAUNCH_CHECK();
        GCNHIP_TRY(hipMemcpyAsync(h, acc, sizeof h, hipMemcpyDeviceToHost, st));
        GCNHIP_TRY(hipStreamSynchronize(st));
        const long long new_num = m2 * (long long)h[LV_IN] - (long long)h[LV_TOT2];
        sweeps++;
        if (h[LV_MOVED] > 0 && new_num > num) {
            std::swap(comm_a, comm_b); std::swap(tot_a, tot_b); std::swap(size_a, size_b);
            num = new_num; sum_in = (long long)h[LV_IN]; sum_tot2 = (long long)h[LV_TOT2];
            undone = 0; moved_any = 1;
        } else {
            undone++;
        }
    }
#undef LV_BY_GROUP
    if (comm_a != comm || tot_a != (long long *)tot) {
        lv_copy_kernel<<<flat, LV_THREADS, 0, st>>>(comm_a, comm, tot_a, (long long *)tot, n);
        GCNHIP_LAUNCH_CHECK();
        GCNHIP_TRY(hipStreamSynchronize(st));                  // the scratch may be handed to the next call at once
    }
    info[0] = sweeps; info[1] = moved_any; info[2] = num; info[3] = m2; info[4] = n_wg; info[5] = n_long; info[6] = sum_in; info[7] = sum_tot2;
    return 0;
}

int gcnhip_louvain_level(gcnhip_ctx *c, int n, int64_t entries, const int32_t *ptr, const int32_t *len, const int32_t *idx, const uint32_t *w,
                         const int64_t *self_w, int max_sweeps, int32_t *comm, int64_t *tot, int64_t *info, void *scratch, int64_t scratch_bytes) {
    return gcnhip_louvain_level_ex(c, n, entries, ptr, len, idx, w, self_w, max_sweeps, comm, tot, info, scratch, scratch_bytes, 0, 0, 0);
}

int gcnhip_louvain_coarsen(gcnhip_ctx *c, int n, int64_t entries, const int32_t *ptr, const int32_t *len, const int32_t *idx, const uint32_t *w,
                           const int64_t *self_w, const int32_t *comm, int32_t *label, int32_t *c_ptr, int32_t *c_len, int32_t *c_idx, uint32_t *c_w,
                           int64_t *c_self, int64_t *info, void *scratch, int64_t scratch_bytes, int table) {
    const char *name = "gcnhip_louvain_coarsen";
    if (!c || !info) return lv_refuse(name, "invalid argument");
    if (const char *why = lv_shape_refusal(n, entries)) return lv_refuse(name, why);
    if (n > 0 && (!ptr || !comm || !label || !c_ptr || !c_len || !c_self || (entries > 0 && (!idx || !c_idx || !c_w)))) return lv_refuse(name, "invalid argument");
    if (lv_table_arg(c, name, table, &table) != 0) return -1;
    if (!scratch || scratch_bytes < lv_coarse_bytes(n) || !aligned16(scratch)) return lv_refuse(name, "the scratch is below what gcnhip_louvain_plan tells, or not 16-byte aligned");
    info[0] = info[1] = 0;
    if (n == 0) return 0;
    Carve cv = {(char *)scratch};
    LvCoarse g = {};
    g.L = {ptr, len, idx, w, (const long long *)self_w, n};
    g.comm = comm; g.label = label;
    g.n_long = cv.take<int>(16);
    g.minv = cv.take<int>(n + 1); g.rank = cv.take<int>(n + 1); g.off = cv.take<int>(n + 1); g.room = cv.take<int>(n + 1);
    g.cursor = cv.take<int>(n + 1); g.members = cv.take<int>(n + 1); g.long_list = cv.take<int>(n + 1);
    g.dense = cv.take<unsigned>(n + 1);
    g.c_ptr = c_ptr; g.c_len = c_len; g.c_idx = c_idx; g.c_w = c_w; g.c_self = (long long *)c_self;
    g.table = table;
    const int blocks = std::max(c->n_cu, 1) * LV_BLOCKS_PER_CU, flat = std::min(ceil_div((int64_t)n + 1, LV_THREADS), blocks);
    hipStream_t st = c->stream;
    lv_coarse_init_kernel<<<flat, LV_THREADS, 0, st>>>(g);
    GCNHIP_LAUNCH_CHECK();
    lv_coarse_min_kernel<<<flat, LV_THREADS, 0, st>>>(g);
    GCNHIP_LAUNCH_CHECK();
    lv_coarse_flag_kernel<<<flat, LV_THREADS, 0, st>>>(g);
    GCNHIP_LAUNCH_CHECK();
    lv_scan_kernel<<<1, LV_SCAN_THREADS, 0, st>>>(g.rank, g.rank, n);
    GCNHIP_LAUNCH_CHECK();
    lv_coarse_label_kernel<<<flat, LV_THREADS, 0, st>>>(g);
    GCNHIP_LAUNCH_CHECK();
    lv_scan_kernel<<<1, LV_SCAN_THREADS, 0, st>>>(g.off, g.off, n);
    GCNHIP_LAUNCH_CHECK();
    lv_coarse_bound_kernel<<<flat, LV_THREADS, 0, st>>>(g);
    GCNHIP_LAUNCH_CHECK();
    lv_scan_kernel<<<1, LV_SCAN_THREADS, 0, st>>>(g.room, c_ptr, n);
    GCNHIP_LAUNCH_CHECK();
    lv_coarse_members_kernel<<<flat, LV_THREADS, 0, st>>>(g);
    GCNHIP_LAUNCH_CHECK();
    int h[4] = {0, 0, 0, 0};                                   // {coarse vertices, extent, long rows, the largest room of the others}
    GCNHIP_TRY(hipMemcpyAsync(&h[0], g.rank + n, sizeof(int), hipMemcpyDeviceToHost, st));
    GCNHIP_TRY(hipMemcpyAsync(&h[1], c_ptr + n, sizeof(int), hipMemcpyDeviceToHost, st));
    GCNHIP_TRY(hipMemcpyAsync(&h[2], g.n_long, 2 * sizeof(int), hipMemcpyDeviceToHost, st));
    GCNHIP_TRY(hipStreamSynchronize(st));
    g.merge_slots = lv_slots(h[3]);                            // the launch's LDS by the largest room it will meet
    const size_t lds = (size_t)g.merge_slots * 8;
    if (lv_big_lds(lv_coarse_merge_kernel, lds) != 0) return lv_refuse(name, "the table does not fit the device's LDS");
    lv_coarse_merge_kernel<<<std::min(std::max(h[0], 1), blocks), LV_THREADS, lds, st>>>(g);
    GCNHIP_LAUNCH_CHECK();
    if (h[2] > 0) {
        lv_coarse_dense_kernel<<<1, LV_THREADS, 0, st>>>(g);
        GCNHIP_LAUNCH_CHECK();
    }
    info[0] = h[0];
    info[1] = h[1];
    return 0;
}

int gcnhip_louvain_compose(gcnhip_ctx *c, int32_t *labels, int n, const int32_t *label, int n_label) {
    if (!c || n < 0 || n_label < 0 || (n > 0 && (!labels || !label))) return lv_refuse("gcnhip_louvain_compose", "invalid argument");
    if (n == 0) return 0;
    lv_compose_kernel<<<std::min(ceil_div(n, LV_THREADS), std::max(c->n_cu, 1) * LV_BLOCKS_PER_CU), LV_THREADS, 0, c->stream>>>(labels, n, label, n_label);
    GCNHIP_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
