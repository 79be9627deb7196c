// overlap.hip — which neighbourhoods overlap: the closed wedges (twice the triangles) through every listed row, and the common
// neighbours of listed pairs of rows with an integer weight summed over them (Adamic-Adar, resource allocation as fixed-point
// tables).  Beyond the reference, which never looks at its adjacency after building it.  The project's first walk that compares
// TWO rows: a row's neighbour set sits in LDS, as a sorted list or a bitmap, while the sets it lists stream past it.  Everything
// is an integer: any grid, any lane group, any cut and any launch give the same bits.
//
// DEFINITIONS (the contract; tests/overlap_ref.py states them again in Python sets and integers)
//   The adjacency object g holds stored rows as the loader made them: unsorted, repeated entries, the self entry and one-way
//   entries are allowed.  It is square, or has columns beyond its rows that name no row (n_cols >= n_rows).
//   NEIGHBOUR SET  S(v) = the distinct u stored in row v with u != v and 0 <= u < n_rows;  d(v) = |S(v)|.  No transpose is built:
//     a one-way entry is in one set only.
//   CLOSED WEDGES  t2(v) = sum over u in S(v) of |S(v) n S(u)|: on a symmetric graph twice the triangles through v.
//   WEDGES  D(v) = d(v) . (d(v) - 1);  the local clustering coefficient is c(v) = t2(v) / D(v), 0 when d(v) < 2.
//   A PAIR (a, b), a == b allowed:  cn = |S(a) n S(b)|,  un = d(a) + d(b) - cn,  wsum = sum over w in S(a) n S(b) of wt[w] with wt
//     a caller-given int64 per column (NULL: 0): an exact integer sum (modulo 2^64), so no arrival order shows in it.  A pair with
//     an end outside [0, n_rows) gives cn = un = wsum = 0 and counts in `skipped`.
//   A ROW QUERY lists n positions; d_rows[i] is the row of position i (NULL: row i); repeats count as often as listed; a position
//     whose row is outside [0, n_rows) counts in `skipped` and nowhere else (t2 = deg = 0).
//   totals [8] int64 = {listed rows in range, rows with d >= 2, sum d, sum D, sum t2, max t2, max d, ratio_sum}, ratio_sum = the sum
//     over the rows with d >= 2 of floor(t2 . 2^32 / D): the mean coefficient as an exact integer sum (structure.hip's idiom).
//     t2 . 2^32 does not fit 64 bits; D < 2^48 because a set holds fewer than 2^24 entries, so the quotient is formed by two 16-bit
//     long-division steps in 64-bit integers.  gcnhip_overlap_sets refuses an object with a row of 2^24 or more stored entries.
//
// gcnhip_overlap_sets   the canonical pass: row v's sorted set, without repeats, the self entry and entries outside the rows, goes
//   to set_idx[indptr[v] .. indptr[v] + set_len[v]): the object's own row pointers are reused, no prefix sum, no second pointer
//   array (the entries of a row's extent behind set_len[v] are unspecified).  Three row classes by STORED length:
//     up to 64 (one wave's worth): a wave per row, one key per lane, a bitonic network of cross-lane moves (21 compare steps),
//       repeats dropped by comparing with the lane below, the survivors placed by a ballot;
//     65 .. 4096: a workgroup per row sorts the row, padded to a power of two, in 16 KB of LDS and compacts it by ballots;
//     longer: one after the other through gcnhip_sort_segments_u32 with one segment (a copy launch that maps what is not in the
//       set to the sentinel, the sort in place in set_idx, a compaction launch).  The host finds them in the row pointers it keeps.
//   Rows are ragged, which is why the tile sort cannot serve the first two classes: it wants equal runs.
// gcnhip_overlap_rows   the triangle kernel.  A lane group of G lanes takes a listed row v; G = 4, 16 or 64 by the object's mean
//   stored row length (at most 16 / at most 128 / above: structure.hip's rule).  S(v) is read from memory ONCE into the group's
//   LDS slice (32 G entries by default) and stays there for the whole row; the sets S(u), u in S(v), stream past it as aligned
//   16-byte vectors (the entries before the first and after the last aligned quad one per lane), and every streamed element is
//   looked up in LDS by binary search.  When d(u) > 32 d(v) the search is turned round: the d(v) elements of S(v) are searched
//   in S(u) in global memory (d(v) log d(u) probes instead of d(u) log d(v)).  A row whose set is longer than the workgroup cut
//   (default: the slice) is left to the WHOLE WORKGROUP behind the group step, one such row after another: its set goes into an
//   LDS BITMAP of one bit per row of g when the device's LDS holds it beside the slices (29 KB on reddit-syn; the capacity is
//   what hipDeviceAttributeMaxSharedMemoryPerBlock reports), set from S(v) and cleared again from S(v), so a lookup is one LDS
//   read; else into the pooled slices (256 / G of them) as a sorted list; else — a set larger than the pool — it stays in global
//   memory and is searched there.  The four waves take the u of S(v) in turn.  Counts are reduced over a row's lanes by
//   shuffles; the totals as in structure.hip: registers, shuffles, LDS, ONE 64-bit atomic per workgroup and total.
// gcnhip_overlap_pairs  the same core with a lane group per pair: the shorter set is the one held and searched for in the longer.
// The _ex forms take G, the workgroup cut, the slice length and bitmap on / off, so that a test reaches every path on a small
// graph.  The entry points zero their own totals with a small launch, allocate nothing and synchronise nothing.
#include "common.h"
#include <algorithm>
#include <cstdio>

constexpr int OV_THREADS = 256, OV_WAVES = OV_THREADS / WAVE;
constexpr int OV_BLOCKS_PER_CU = 4;
constexpr int OV_SHORT = WAVE;                                 // stored lengths up to this: a wave sorts the row
constexpr int OV_MEDIUM = 4096;                                // up to this: a workgroup sorts it in LDS
constexpr int OV_MAX_ROW = 1 << 24;                            // stored entries of a row, exclusive
constexpr int OV_SWAP = 32;                                    // d(u) > OV_SWAP . d(v): search S(v) in S(u)
constexpr int OV_SLICE_PER_LANE = 32;                          // default slice: 32 G entries, 32 KB per workgroup
constexpr unsigned OV_NONE = 0xFFFFFFFFu;                      // the key of an entry that is not in the set; sorts last

struct OvSets {
    const int *__restrict__ indptr;
    const int *__restrict__ set_idx;
    const int32_t *__restrict__ set_len;
    int n_rows;
};

// ---- the canonical pass ------------------------------------------------------------------------------------------------------

__device__ inline unsigned ov_key(int u, int v, int n_rows) { return u == v || (unsigned)u >= (unsigned)n_rows ? OV_NONE : (unsigned)u; }

__global__ __launch_bounds__(OV_THREADS) void ov_sets_short_kernel(const int *__restrict__ indptr, const int *__restrict__ indices, int n_rows,
                                                                   int *__restrict__ set_idx, int32_t *__restrict__ set_len) {
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
    for (int64_t v = (int64_t)blockIdx.x * OV_WAVES + wave; v < n_rows; v += (int64_t)gridDim.x * OV_WAVES) {
        const int e0 = indptr[v], len = indptr[v + 1] - e0;
        if (len > OV_SHORT) continue;
        unsigned key = lane < len ? ov_key(indices[e0 + lane], (int)v, n_rows) : OV_NONE;
#pragma unroll
        for (int k = 2; k <= WAVE; k <<= 1)
#pragma unroll
            for (int j = k >> 1; j > 0; j >>= 1) {
                const unsigned other = __shfl_xor(key, j, WAVE);
                const bool keep_low = ((lane & k) == 0) == ((lane & j) == 0);
                key = keep_low ? min(key, other) : max(key, other);
            }
        const unsigned below = __shfl_up(key, 1, WAVE);
        const bool keep = key != OV_NONE && (lane == 0 || key != below);
        const unsigned long long kept = __ballot(keep);
        if (keep) set_idx[e0 + __popcll(kept & ((1ull << lane) - 1ull))] = (int)key;
        if (lane == 0) set_len[v] = __popcll(kept);
    }
}

// 256 threads compact the sorted keys [0, len) read through `key_at` into out[0 ..); returns the number kept (to every thread)
template <class F>
__device__ inline int ov_compact(int len, F key_at, int *__restrict__ out) {
    __shared__ int wave_kept[OV_WAVES];
    __shared__ unsigned carry;
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
    int base = 0;
    unsigned last = OV_NONE;                                   // the key before this chunk: nothing kept equals it
    for (int c0 = 0; c0 < len; c0 += OV_THREADS) {             // uniform over the workgroup
        const int idx = c0 + threadIdx.x;
        const unsigned key = idx < len ? key_at(idx) : OV_NONE;
        unsigned below = __shfl_up(key, 1, WAVE);
        __syncthreads();                                       // the chunk is read before anything of it is overwritten
        if (lane == WAVE - 1) wave_kept[wave] = (int)key;      // lent: the last key of each wave
        __syncthreads();
        if (lane == 0) below = wave ? (unsigned)wave_kept[wave - 1] : last;
        if (threadIdx.x == OV_THREADS - 1) carry = key;
        const bool keep = key != OV_NONE && key != below;
        const unsigned long long kept = __ballot(keep);
        __syncthreads();
        if (lane == 0) wave_kept[wave] = __popcll(kept);
        __syncthreads();
        int at = base;
        for (int w = 0; w < wave; w++) at += wave_kept[w];
        if (keep) out[at + __popcll(kept & ((1ull << lane) - 1ull))] = (int)key;
        for (int w = 0; w < OV_WAVES; w++) base += wave_kept[w];
        last = carry;
    }
    return base;
}

__global__ __launch_bounds__(OV_THREADS) void ov_sets_medium_kernel(const int *__restrict__ indptr, const int *__restrict__ indices, int n_rows,
                                                                    int *__restrict__ set_idx, int32_t *__restrict__ set_len) {
    __shared__ unsigned keys[OV_MEDIUM];
    for (int64_t v = blockIdx.x; v < n_rows; v += gridDim.x) {
        const int e0 = indptr[v], len = indptr[v + 1] - e0;
        if (len <= OV_SHORT || len > OV_MEDIUM) continue;      // uniform over the workgroup
        int P = 2 * OV_SHORT;
        while (P < len) P <<= 1;
        __syncthreads();                                       // the row before is out of LDS
        for (int i = threadIdx.x; i < P; i += OV_THREADS) keys[i] = i < len ? ov_key(indices[e0 + i], (int)v, n_rows) : OV_NONE;
        for (int k = 2; k <= P; k <<= 1)
            for (int j = k >> 1; j > 0; j >>= 1) {
                __syncthreads();
                for (int i = threadIdx.x; i < P; i += OV_THREADS) {
                    const int p = i ^ j;
                    if (p > i) {
                        const unsigned a = keys[i], b = keys[p];
                        if ((a > b) == ((i & k) == 0)) { keys[i] = b; keys[p] = a; }
                    }
                }
            }
        __syncthreads();
        const int kept = ov_compact(len, [&](int i) { return keys[i]; }, set_idx + e0);
        if (threadIdx.x == 0) set_len[v] = kept;
    }
}

__global__ __launch_bounds__(OV_THREADS) void ov_long_copy_kernel(const int *__restrict__ src, unsigned *__restrict__ dst, int len, int v, int n_rows) {
    for (int64_t i = (int64_t)blockIdx.x * OV_THREADS + threadIdx.x; i < len; i += (int64_t)gridDim.x * OV_THREADS) dst[i] = ov_key(src[i], v, n_rows);
}
// one workgroup, in place: a kept key lands at or before its own position, and a chunk is read before it is written
__global__ __launch_bounds__(OV_THREADS) void ov_long_compact_kernel(int *__restrict__ keys, int len, int32_t *__restrict__ out_len) {
    const unsigned *in = (const unsigned *)keys;
    const int kept = ov_compact(len, [&](int i) { return in[i]; }, keys);
    if (threadIdx.x == 0) *out_len = kept;
}

// ---- the intersection core ---------------------------------------------------------------------------------------------------

__device__ inline bool ov_find(const int *a, int n, int x) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (a[mid] < x) lo = mid + 1;
        else hi = mid;
    }
    return lo < n && a[lo] == x;
}

// what a lane has counted: the common elements and the sum of their weights
struct OvCount {
    unsigned long long cn, ws;
};

// W lanes (lane = 0 .. W - 1) pass the entries [e0, e1) of set_idx to `visit`: aligned 16-byte vectors between head and tail
template <int W, class F>
__device__ inline void ov_stream(const int *__restrict__ set_idx, int e0, int e1, int lane, F visit) {
    const int a0 = (e0 + 3) & ~3, a1 = e1 & ~3;                // the aligned quads are [a0, a1)
    if (a0 >= a1) {                                            // fewer than 7 entries
        for (int e = e0 + lane; e < e1; e += W) visit(set_idx[e]);
        return;
    }
    if (lane < a0 - e0) visit(set_idx[e0 + lane]);
    if (lane < e1 - a1) visit(set_idx[a1 + lane]);
    const int4 *__restrict__ quads = (const int4 *)set_idx;    // the entry point checked the alignment
    const int q1 = a1 >> 2;
    for (int q = (a0 >> 2) + lane; q < q1; q += W) {
        const int4 x = quads[q];
        visit(x.x); visit(x.y); visit(x.z); visit(x.w);
    }
}

// |A n S(u)| with A a sorted list of da entries (LDS or global) held by W lanes: S(u) streams past A, or A is searched in S(u)
template <int W, bool WS>
__device__ inline void ov_core(const int *a, int da, const OvSets &s, int u, int lane, const int64_t *__restrict__ wt, OvCount &c) {
    if ((unsigned)u >= (unsigned)s.n_rows) return;
    const int b0 = s.indptr[u], db = s.set_len[u];
    if (da <= 0 || db <= 0) return;
    auto hit = [&](int x) {
        c.cn++;
        if (WS && wt) c.ws += (unsigned long long)wt[x];
    };
    if ((int64_t)db > (int64_t)OV_SWAP * da) {
        for (int i = lane; i < da; i += W) {
            const int x = a[i];
            if (ov_find(s.set_idx + b0, db, x)) hit(x);
        }
        return;
    }
    ov_stream<W>(s.set_idx, b0, b0 + db, lane, [&](int x) { if (ov_find(a, da, x)) hit(x); });
}

template <int W>
__device__ inline OvCount ov_reduce(OvCount c) {
#pragma unroll
    for (int off = W / 2; off > 0; off >>= 1) {
        c.cn += __shfl_xor(c.cn, off, WAVE);
        c.ws += __shfl_xor(c.ws, off, WAVE);
    }
    return c;
}

struct OvArgs {
    OvSets s;
    const int32_t *__restrict__ first;                         // rows: d_rows (may be NULL); pairs: src
    const int32_t *__restrict__ second;                        // pairs: dst
    int n;
    const int64_t *__restrict__ wt;
    int64_t *__restrict__ out64;                               // rows: t2; pairs: wsum
    int32_t *__restrict__ out_a;                               // rows: deg; pairs: cn
    int32_t *__restrict__ out_b;                               // pairs: un
    unsigned long long *__restrict__ totals, *__restrict__ skipped;
    int slice, wg_cut, bm_words;                               // bm_words 0: no bitmap
};

struct OvTotals {
    unsigned long long v[9];                                   // the eight totals and the skipped positions ([5], [6] are maxima)
};

// floor(t2 . 2^32 / D) for t2 <= D < 2^48
__device__ inline unsigned long long ov_ratio(unsigned long long t2, unsigned long long D) {
    unsigned long long q = t2 / D, r = t2 % D;
#pragma unroll
    for (int step = 0; step < 2; step++) {
        r <<= 16;
        q = (q << 16) | (r / D);
        r %= D;
    }
    return q;
}

// one lane finishes position i: a is the held row, b the other end of a pair
template <bool PAIRS>
__device__ inline void ov_finish(const OvArgs &g, int i, int da, int db, const OvCount &c, OvTotals &t) {
    if (PAIRS) {
        if (g.out_a) g.out_a[i] = (int)c.cn;
        if (g.out_b) g.out_b[i] = da + db - (int)c.cn;
        if (g.out64) g.out64[i] = (int64_t)c.ws;
        return;
    }
    if (g.out64) g.out64[i] = (int64_t)c.cn;
    if (g.out_a) g.out_a[i] = da;
    const unsigned long long d = (unsigned)da, D = d * (d ? d - 1 : 0);
    t.v[0] += 1;
    t.v[2] += d;
    t.v[3] += D;
    t.v[4] += c.cn;
    t.v[5] = max(t.v[5], c.cn);
    t.v[6] = max(t.v[6], d);
    if (da >= 2) {
        t.v[1] += 1;
        t.v[7] += ov_ratio(min(c.cn, D), D);
    }
}

template <int G, bool PAIRS>
__global__ __launch_bounds__(OV_THREADS) void ov_kernel(OvArgs g) {
    extern __shared__ int ov_lds[];                            // [256 / G slices of g.slice entries | the bitmap]
    __shared__ int4 wg_rows[OV_THREADS / 4];                   // the positions left to the whole workgroup: {i, held row, other row, 0}
    __shared__ int wg_n[2];                                    // by the parity of the step
    __shared__ unsigned long long wg_count[2];
    __shared__ unsigned long long block_totals[9];
    constexpr int PER_BLOCK = OV_THREADS / G;
    const int pool_len = PER_BLOCK * g.slice;
    unsigned *bitmap = (unsigned *)(ov_lds + pool_len);
    for (int e = threadIdx.x; e < g.bm_words; e += OV_THREADS) bitmap[e] = 0;
    if (threadIdx.x < 9) block_totals[threadIdx.x] = 0;
    if (threadIdx.x < 2) { wg_n[threadIdx.x] = 0; wg_count[threadIdx.x] = 0; }
    __syncthreads();

    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE, gl = threadIdx.x & (G - 1), gid = threadIdx.x / G;
    int *mine = ov_lds + gid * g.slice;
    const OvSets &s = g.s;
    OvTotals t = {};
    int parity = 0;

    for (int64_t base = (int64_t)blockIdx.x * PER_BLOCK; base < g.n; base += (int64_t)gridDim.x * PER_BLOCK, parity ^= 1) {
        const int64_t i64 = base + gid;
        const int i = (int)(i64 < g.n ? i64 : -1);
        int va = -1, vb = -1, da = 0, db = 0, a0 = 0;
        if (i >= 0) {
            int ra = g.first ? g.first[i] : i, rb = PAIRS ? g.second[i] : ra;
            if ((unsigned)ra < (unsigned)s.n_rows && (unsigned)rb < (unsigned)s.n_rows) {
                da = s.set_len[ra];
                db = PAIRS ? s.set_len[rb] : da;
                if (da > db) {                                  // the shorter set is held
                    const int r = ra, d = da;
                    ra = rb; da = db; rb = r; db = d;
                }
                va = ra; vb = rb; a0 = s.indptr[ra];
            } else if (gl == 0) {
                t.v[8] += 1;
                if (g.out64) g.out64[i] = 0;
                if (g.out_a) g.out_a[i] = 0;
                if (PAIRS && g.out_b) g.out_b[i] = 0;
            }
        }
        const bool is_wg = va >= 0 && da > g.wg_cut, in_lds = va >= 0 && !is_wg && da <= g.slice;
        if (in_lds)
            for (int k = gl; k < da; k += G) mine[k] = s.set_idx[a0 + k];
        if (is_wg && gl == 0) wg_rows[atomicAdd(&wg_n[parity], 1)] = make_int4(i, va, vb, 0);
        __syncthreads();                                       // the slices are filled, the workgroup rows listed
        if (threadIdx.x == 0) wg_n[parity ^ 1] = 0;            // the next step's list; nobody adds to it before the barrier below

        if (va >= 0 && !is_wg) {
            const int *a = in_lds ? mine : s.set_idx + a0;
            OvCount c = {0, 0};
            if (PAIRS) {
                if (in_lds) ov_core<G, true>(mine, da, s, vb, gl, g.wt, c);
                else ov_core<G, true>(s.set_idx + a0, da, s, vb, gl, g.wt, c);
            } else if (in_lds) {
                for (int k = 0; k < da; k++) ov_core<G, false>(mine, da, s, mine[k], gl, nullptr, c);
            } else {
                for (int k = 0; k < da; k++) ov_core<G, false>(a, da, s, a[k], gl, nullptr, c);
            }
            c = ov_reduce<G>(c);
            if (gl == 0) ov_finish<PAIRS>(g, i, da, db, c, t);
        }
        __syncthreads();                                       // the groups are done with their slices

        const int n_wg = wg_n[parity];
        for (int w = 0; w < n_wg; w++) {                       // uniform over the workgroup
            const int4 row = wg_rows[w];
            const int wa0 = s.indptr[row.y], wda = s.set_len[row.y], wdb = s.set_len[row.z];
            const bool as_bits = g.bm_words > 0, as_list = !as_bits && wda <= pool_len;
            for (int k = threadIdx.x; k < wda; k += OV_THREADS) {
                const int x = s.set_idx[wa0 + k];
                if (as_list) ov_lds[k] = x;
                else if (as_bits && (unsigned)x < (unsigned)g.bm_words * 32u) atomicOr(&bitmap[x >> 5], 1u << (x & 31));
            }
            __syncthreads();
            OvCount c = {0, 0};
            const int n_other = PAIRS ? 1 : wda;
            for (int k = wave; k < n_other; k += OV_WAVES) {
                const int u = PAIRS ? row.z : (as_list ? ov_lds[k] : s.set_idx[wa0 + k]);
                if (as_bits) {
                    if ((unsigned)u >= (unsigned)s.n_rows) continue;
                    const int b0 = s.indptr[u];
                    ov_stream<WAVE>(s.set_idx, b0, b0 + s.set_len[u], lane, [&](int x) {
                        if ((unsigned)x < (unsigned)g.bm_words * 32u && (bitmap[x >> 5] >> (x & 31) & 1u)) {
                            c.cn++;
                            if (PAIRS && g.wt) c.ws += (unsigned long long)g.wt[x];
                        }
                    });
                } else if (as_list) {
                    ov_core<WAVE, PAIRS>(ov_lds, wda, s, u, lane, g.wt, c);
                } else {
                    ov_core<WAVE, PAIRS>(s.set_idx + wa0, wda, s, u, lane, g.wt, c);
                }
            }
            c = ov_reduce<WAVE>(c);
            if (lane == 0 && c.cn) atomicAdd(&wg_count[0], c.cn);
            if (lane == 0 && c.ws) atomicAdd(&wg_count[1], c.ws);
            __syncthreads();
            if (as_bits)
                for (int k = threadIdx.x; k < wda; k += OV_THREADS) {
                    const int x = s.set_idx[wa0 + k];
                    if ((unsigned)x < (unsigned)g.bm_words * 32u) bitmap[x >> 5] = 0;
                }
            if (threadIdx.x == 0) {
                const OvCount all = {wg_count[0], wg_count[1]};
                ov_finish<PAIRS>(g, row.x, wda, wdb, all, t);
                wg_count[0] = 0;
                wg_count[1] = 0;
            }
            __syncthreads();
        }
    }

#pragma unroll
    for (int k = 0; k < 9; k++) {
        unsigned long long x = t.v[k];
        const bool is_max = k == 5 || k == 6;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const unsigned lo = __shfl_xor((unsigned)x, off, WAVE), hi = __shfl_xor((unsigned)(x >> 32), off, WAVE);
            const unsigned long long y = ((unsigned long long)hi << 32) | lo;
            x = is_max ? max(x, y) : x + y;
        }
        if (lane == 0 && x) {
            if (is_max) atomicMax(&block_totals[k], x);
            else atomicAdd(&block_totals[k], x);
        }
    }
    __syncthreads();
    if (threadIdx.x < 9 && block_totals[threadIdx.x]) {
        const int k = threadIdx.x;
        if (k == 8) atomicAdd(g.skipped, block_totals[k]);
        else if (PAIRS) return;
        else if (k == 5 || k == 6) atomicMax(&g.totals[k], block_totals[k]);
        else atomicAdd(&g.totals[k], block_totals[k]);
    }
}

__global__ void ov_zero_kernel(unsigned long long *__restrict__ totals, unsigned long long *__restrict__ skipped) {
    if (totals && threadIdx.x < 8) totals[threadIdx.x] = 0;
    if (threadIdx.x == 8) *skipped = 0;
}

namespace {

int ov_refuse(const char *name, const char *why) {
    char msg[200];
    snprintf(msg, sizeof msg, "%s: %s", name, why);
    return gcnhip_fail(msg);
}

const char *ov_graph_refusal(const gcnhip_graph *g) {
    if (g->n_cols < g->n_rows) return "the adjacency object has fewer columns than rows (a row's entries name rows)";
    if ((int)g->h_indptr.size() != g->n_rows + 1) return "the adjacency object has no host row pointers";
    return nullptr;
}

int ov_lds_capacity(const gcnhip_ctx *c) {
    int cap = 0;
    if (hipDeviceGetAttribute(&cap, hipDeviceAttributeMaxSharedMemoryPerBlock, c->device) != hipSuccess || cap <= 0) cap = 64 << 10;
    return cap;
}

template <bool PAIRS>
int ov_launch(gcnhip_ctx *c, const char *name, const gcnhip_graph *g, OvArgs a, int group, int wg_cut, int slice, int bitmap) {
    if (const char *why = ov_graph_refusal(g)) return ov_refuse(name, why);
    if (!aligned16(a.s.set_idx)) return ov_refuse(name, "set_idx is not 16-byte aligned");
    if (group != 0 && group != 4 && group != 16 && group != 64) return ov_refuse(name, "the lane group is 0 (by the mean row length), 4, 16 or 64");
    if (wg_cut < 0 || slice < 0 || (bitmap != 0 && bitmap != 1)) return ov_refuse(name, "the workgroup cut and the slice are 0 (the default) or positive, bitmap is 0 or 1");
    if (!group) {
        const int64_t mean = g->n_rows > 0 ? (int64_t)g->nnz / g->n_rows : 0;
        group = mean <= 16 ? 4 : (mean <= 128 ? 16 : 64);
    }
    if (!slice) slice = OV_SLICE_PER_LANE * group;
    if (!wg_cut) wg_cut = slice;
    const int cap = ov_lds_capacity(c) - 2048;                 // the kernel's static tables
    const int64_t pool_bytes = (int64_t)(OV_THREADS / group) * slice * (int64_t)sizeof(int);
    if (pool_bytes > cap) return ov_refuse(name, "the slices do not fit the device's LDS");
    const int64_t bm_words = ((int64_t)g->n_rows + 31) / 32;
    a.slice = slice;
    a.wg_cut = wg_cut;
    a.bm_words = bitmap && pool_bytes + bm_words * 4 <= cap ? (int)bm_words : 0;
    ov_zero_kernel<<<1, 64, 0, c->stream>>>(a.totals, a.skipped);
    GCNHIP_LAUNCH_CHECK();
    if (a.n == 0) return 0;
    const size_t lds = (size_t)pool_bytes + (size_t)a.bm_words * 4;
    const int grid = std::max(1, std::min(ceil_div(a.n, OV_THREADS / group), std::max(c->n_cu, 1) * OV_BLOCKS_PER_CU));
    void (*kernel)(OvArgs) = group == 4 ? ov_kernel<4, PAIRS> : (group == 16 ? ov_kernel<16, PAIRS> : ov_kernel<64, PAIRS>);
    if (lds > (size_t)(48 << 10)) GCNHIP_TRY(hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    kernel<<<grid, OV_THREADS, lds, c->stream>>>(a);
    GCNHIP_LAUNCH_CHECK();
    return 0;
}

}  // namespace

extern "C" {

int gcnhip_overlap_plan(const gcnhip_graph *g, int64_t *scratch_bytes) {
    const char *name = "gcnhip_overlap_plan";
    if (!g || !scratch_bytes) return ov_refuse(name, "invalid argument");
    if (const char *why = ov_graph_refusal(g)) return ov_refuse(name, why);
    int64_t longest = 0;
    for (int v = 0; v < g->n_rows; v++) {
        const int64_t len = g->h_indptr[v + 1] - g->h_indptr[v];
        if (len >= OV_MAX_ROW) return ov_refuse(name, "a row of the adjacency object stores 2^24 entries or more");
        if (len > OV_MEDIUM) longest = std::max(longest, len);
    }
    *scratch_bytes = std::max<int64_t>(16, (longest * 4 + 15) & ~(int64_t)15);
    return 0;
}

int gcnhip_overlap_sets(gcnhip_ctx *c, const gcnhip_graph *g, int32_t *set_idx, int32_t *set_len, void *scratch, int64_t scratch_bytes) {
    const char *name = "gcnhip_overlap_sets";
    if (!c || !g || !set_len || (g->nnz > 0 && !set_idx)) return ov_refuse(name, "invalid argument");
    int64_t need = 0;
    if (gcnhip_overlap_plan(g, &need) != 0) return -1;
    if (!aligned16(set_idx)) return ov_refuse(name, "set_idx is not 16-byte aligned");
    if (need > 16 && (!scratch || scratch_bytes < need)) return ov_refuse(name, "the scratch is below what gcnhip_overlap_plan tells");
    if (g->n_rows == 0) return 0;
    const int *indptr = g->indptr, *indices = g->indices;
    const int blocks = std::max(c->n_cu, 1) * OV_BLOCKS_PER_CU;
    ov_sets_short_kernel<<<std::min(ceil_div(g->n_rows, OV_WAVES), blocks), OV_THREADS, 0, c->stream>>>(indptr, indices, g->n_rows, set_idx, set_len);
    GCNHIP_LAUNCH_CHECK();
    ov_sets_medium_kernel<<<std::min(g->n_rows, blocks), OV_THREADS, 0, c->stream>>>(indptr, indices, g->n_rows, set_idx, set_len);
    GCNHIP_LAUNCH_CHECK();
    for (int v = 0; v < g->n_rows; v++) {
        const int e0 = g->h_indptr[v], len = g->h_indptr[v + 1] - e0;
        if (len <= OV_MEDIUM) continue;
        ov_long_copy_kernel<<<std::min(ceil_div(len, OV_THREADS), blocks), OV_THREADS, 0, c->stream>>>(indices + e0, (unsigned *)set_idx + e0, len, v, g->n_rows);
        GCNHIP_LAUNCH_CHECK();
        const int rc = gcnhip_sort_segments_u32(c, (uint32_t *)set_idx + e0, (uint32_t *)scratch, len, 1, len);
        if (rc != 0) return rc;
        ov_long_compact_kernel<<<1, OV_THREADS, 0, c->stream>>>(set_idx + e0, len, set_len + v);
        GCNHIP_LAUNCH_CHECK();
    }
    return 0;
}

int gcnhip_overlap_rows_ex(gcnhip_ctx *c, const gcnhip_graph *g, const int32_t *set_idx, const int32_t *set_len, const int32_t *d_rows, int n,
                           int64_t *t2, int32_t *deg, int64_t *totals, int64_t *skipped, int group, int wg_cut, int slice, int bitmap) {
    const char *name = "gcnhip_overlap_rows";
    if (!c || !g || !set_len || (g->nnz > 0 && !set_idx) || !totals || !skipped || n < 0) return ov_refuse(name, "invalid argument");
    if (!d_rows && n > g->n_rows) return ov_refuse(name, "without a row list n is at most n_rows");
    OvArgs a = {};
    a.s = {g->indptr, set_idx, set_len, g->n_rows};
    a.first = d_rows; a.n = n; a.out64 = t2; a.out_a = deg;
    a.totals = (unsigned long long *)totals; a.skipped = (unsigned long long *)skipped;
    return ov_launch<false>(c, name, g, a, group, wg_cut, slice, bitmap);
}

int gcnhip_overlap_rows(gcnhip_ctx *c, const gcnhip_graph *g, const int32_t *set_idx, const int32_t *set_len, const int32_t *d_rows, int n, int64_t *t2,
                        int32_t *deg, int64_t *totals, int64_t *skipped) {
    return gcnhip_overlap_rows_ex(c, g, set_idx, set_len, d_rows, n, t2, deg, totals, skipped, 0, 0, 0, 1);
}

int gcnhip_overlap_pairs_ex(gcnhip_ctx *c, const gcnhip_graph *g, const int32_t *set_idx, const int32_t *set_len, const int32_t *src, const int32_t *dst,
                            int n_pairs, const int64_t *wt, int32_t *cn, int32_t *un, int64_t *wsum, int64_t *skipped, int group, int wg_cut, int slice,
                            int bitmap) {
    const char *name = "gcnhip_overlap_pairs";
    if (!c || !g || !set_len || (g->nnz > 0 && !set_idx) || !skipped || n_pairs < 0 || (n_pairs > 0 && (!src || !dst)))
        return ov_refuse(name, "invalid argument");
    OvArgs a = {};
    a.s = {g->indptr, set_idx, set_len, g->n_rows};
    a.first = src; a.second = dst; a.n = n_pairs; a.wt = wt; a.out64 = wsum; a.out_a = cn; a.out_b = un;
    a.skipped = (unsigned long long *)skipped;
    return ov_launch<true>(c, name, g, a, group, wg_cut, slice, bitmap);
}

int gcnhip_overlap_pairs(gcnhip_ctx *c, const gcnhip_graph *g, const int32_t *set_idx, const int32_t *set_len, const int32_t *src, const int32_t *dst,
                         int n_pairs, const int64_t *wt, int32_t *cn, int32_t *un, int64_t *wsum, int64_t *skipped) {
    return gcnhip_overlap_pairs_ex(c, g, set_idx, set_len, src, dst, n_pairs, wt, cn, un, wsum, skipped, 0, 0, 0, 1);
}

}  // extern "C"
