// reach.hip — how far every row is from a set of seed rows, and which rows hang together: a level-synchronous multi-source
// breadth-first search and a connected-components labelling over the stored rows of an adjacency object, and the accuracy of a
// prediction by that distance.  Beyond the reference, which never looks at its adjacency after building it.  The project's first
// ITERATIVE traversal: a call is a sequence of launches whose number depends on the graph.  Everything is an integer, every
// result is canonical (no arrival order can show in it): any grid, any lane grouping, any batching of the read-backs and any
// launch give the same bits.
//
// DEFINITIONS (the contract; tests/reach_ref.py states them again in Python integers)
//   The adjacency object g is square and holds stored rows as the loader made them: the self entry may be there, a repeated entry
//   changes nothing here, one-way entries are allowed.  An entry outside [0, n_rows) is passed over.
//   HOP DISTANCE from a seed list (repeats allowed; a seed outside [0, n_rows) counts in `skipped` and nowhere else):
//     dist[v] = 0 for a seed; otherwise dist[v] = 1 + min dist[u] over the stored entries u != v of ROW v with dist[u] >= 0 — the
//     direction an aggregation carries information: row v gathers from the entries it lists.  No transpose is used or built.
//     dist[v] = -1 when no seed reaches v, or none within max_hops (0: no limit).
//     nearest[v] = the lowest ROW INDEX among the seeds at distance dist[v] from v (-1 when dist[v] = -1).  Level by level:
//     nearest[s] = s for a seed, else the minimum over the entries u of row v with dist[u] == dist[v] - 1 of nearest[u].
//     levels = the largest distance assigned (0 without a reached row); level_counts[d] = the rows with dist == d.
//   COMPONENTS: comp[v] = the smallest row index in v's WEAKLY connected component: every stored entry u != v of row v joins u
//     and v, whichever of the two rows stores it.
//   COMPONENT COUNTS: size[r] = the rows with comp == r, marked[r] = those of them with mark != 0 (mark NULL: none); totals [6] =
//     {rows with comp in range, components (rows r with comp[r] == r), largest size, components without a marked row, rows in
//     those components, marked rows}.
//   DISTANCE STRATA of a query of n positions (d_rows[i] = the row of position i, NULL: row i; a row outside [0, n_rows) counts
//     nowhere): bucket b = dist for 0 <= dist < hops, hops for dist >= hops, hops + 1 for dist < 0; strata[b * 4 + k] counts
//     k = 0 the positions listed, 1 those whose truth is known (0 <= truth < num_classes), 2 of those the ones with pred == truth
//     (pred NULL: none), 3 of those the ones whose nearest row s is in range and has a known truth[s] == truth (nearest NULL:
//     none); *unlabelled = the listed positions without a known truth.
//
// gcnhip_hop_distance   One level is ONE launch: level L gives distance L to every row without a distance that stores an entry
//   of distance L - 1.  There is no grid-wide barrier, no spin wait and no cooperative launch anywhere: the order between levels
//   is the stream's.  Inside a launch rows read dist[] while other workgroups write it, and that is harmless: a racing read sees
//   -1 or L, and neither is L - 1; nearest[u] is read only for dist[u] == L - 1, which an earlier launch wrote.  So a level
//   launched after the frontier has emptied changes nothing, and the host may enqueue levels_per_sync launches, each adding its
//   newly reached rows to a counter of its own (one integer atomic per workgroup), before it reads the counters back once and
//   stops at the first zero.  A level walks only rows that have no distance yet (it still reads dist[] of every row: 4 bytes per
//   row and level).  The walk is structure.hip's: a lane group of 4, 16 or 64 lanes per row by the mean stored row length,
//   aligned 16-byte index loads, rows of more than 64 G entries left to the whole wave.  Without `nearest` a row stops at the
//   first vector step in which one of its lanes has a hit; with it the whole row is walked and the minimum taken by shuffles.
// gcnhip_components   min-label hooking and pointer jumping (Shiloach & Vishkin, 1982; FastSV: Zhang, Azad & Hu, 2020) on
//   comp[] itself as the parent array, parent[x] <= x always.  A round is three steps in stream order: clear the flag; HOOK —
//   every row v reads its label pv and, per entry u, pu; where they differ, atomicMin(&parent[max], min) and the flag is set;
//   JUMP — every row follows its parents to the root and stores it.  Labels only fall, so the parent links never form a cycle
//   and the chase ends; a link that a lower hook overwrites is found again by the edge that made it, in the next round.  After
//   JUMP every label is a root.  The routine ends after a round whose HOOK found pu == pv on EVERY stored entry — a full
//   verification, not a heuristic: the labels are then constant on each weak component, differ between components (a root is a
//   row of its own tree, and trees only join along entries) and, with parent[x] <= x, are the component's smallest row.
//   The flag (4 bytes) is all that is read back per round.
// Both SYNCHRONISE the context's stream (the host decides from the counters whether to go on) and allocate nothing: the counters
// live in caller-given scratch.  gcnhip_component_counts and gcnhip_distance_strata zero their own outputs, allocate nothing and
// synchronise nothing.
#include "common.h"
#include <algorithm>
#include <climits>
#include <cstdio>

constexpr int RC_THREADS = 256;
constexpr int RC_BLOCKS_PER_CU = 8;
constexpr int RC_MAX_HOPS_BUCKETS = 32;
constexpr int RC_MAX_SYNC = 64;                                // levels between two read-backs, and the counters in scratch
constexpr int RC_NONE = INT_MAX;                               // no hit

struct RcGraph {
    const int *__restrict__ indptr;
    const int *__restrict__ indices;
    int n_rows;
};

// ---- the traversal ---------------------------------------------------------------------------------------------------------

// what entry u gives row v at this level: nearest[u] (0 without `nearest`) when u is a frontier row, else RC_NONE
template <bool NEAREST>
__device__ inline int rc_hit(int u, int v, int want, int n_rows, const int32_t *dist, const int32_t *nearest) {
    if (u == v || (unsigned)u >= (unsigned)n_rows) return RC_NONE;
    if (dist[u] != want) return RC_NONE;
    return NEAREST ? nearest[u] : 0;
}

// W lanes (lane = 0 .. W - 1, gmask = their bits in the wave) walk the entries [e0, e1) of row v; returns this lane's minimum
template <int W, bool NEAREST>
__device__ inline int rc_walk(const int *__restrict__ indices, int e0, int e1, int lane, unsigned long long gmask, int v, int want, int n_rows,
                              const int32_t *dist, const int32_t *nearest) {
    int best = RC_NONE;
    const int a0 = (e0 + 3) & ~3, a1 = e1 & ~3;                 // the aligned quads are [a0, a1)
    if (a0 >= a1) {                                             // fewer than 7 entries
        for (int e = e0 + lane; e < e1; e += W) best = min(best, rc_hit<NEAREST>(indices[e], v, want, n_rows, dist, nearest));
        return best;
    }
    if (lane < a0 - e0) best = min(best, rc_hit<NEAREST>(indices[e0 + lane], v, want, n_rows, dist, nearest));
    if (lane < e1 - a1) best = min(best, rc_hit<NEAREST>(indices[a1 + lane], v, want, n_rows, dist, nearest));
    const int4 *__restrict__ quads = (const int4 *)indices;     // the index array is a device allocation: 256-byte aligned
    const int q1 = a1 >> 2;
    for (int qb = a0 >> 2; qb < q1; qb += W) {                  // uniform over the W lanes
        if (!NEAREST && (__ballot(best != RC_NONE) & gmask)) break;   // the row has its hit: the lanes of a group leave together
        const int q = qb + lane;
        if (q < q1) {
            const int4 x = quads[q];
            const int h0 = rc_hit<NEAREST>(x.x, v, want, n_rows, dist, nearest), h1 = rc_hit<NEAREST>(x.y, v, want, n_rows, dist, nearest);
            const int h2 = rc_hit<NEAREST>(x.z, v, want, n_rows, dist, nearest), h3 = rc_hit<NEAREST>(x.w, v, want, n_rows, dist, nearest);
            best = min(min(best, min(h0, h1)), min(h2, h3));
        }
    }
    return best;
}

template <int W>
__device__ inline int rc_group_min(int x) {
#pragma unroll
    for (int off = W / 2; off > 0; off >>= 1) x = min(x, __shfl_xor(x, off, WAVE));
    return x;
}

// a workgroup's count, added once: per-wave sums meet in LDS
__device__ inline void rc_block_add(int mine, unsigned long long *counter) {
    __shared__ int block_sum;
    if (threadIdx.x == 0) block_sum = 0;
    __syncthreads();
    const int s = wave_sum_i(mine);
    if ((threadIdx.x & (WAVE - 1)) == 0 && s) atomicAdd(&block_sum, s);
    __syncthreads();
    if (threadIdx.x == 0 && block_sum) atomicAdd(counter, (unsigned long long)(unsigned)block_sum);
}

// level `level`: the rows without a distance that store an entry of distance level - 1 get `level`
template <int G, bool NEAREST>
__global__ __launch_bounds__(RC_THREADS) void hop_level_kernel(RcGraph g, int level, int32_t *dist, int32_t *nearest, unsigned long long *reached) {
    constexpr int PER_BLOCK = RC_THREADS / G, LONG_ROW = 64 * G;
    const int lane = threadIdx.x & (WAVE - 1), gl = threadIdx.x & (G - 1), gid = threadIdx.x / G;
    const unsigned long long gmask = G == WAVE ? ~0ull : ((1ull << G) - 1ull) << (lane & ~(G - 1));
    const int want = level - 1;
    int mine = 0;
    for (int64_t base = (int64_t)blockIdx.x * PER_BLOCK; base < g.n_rows; base += (int64_t)gridDim.x * PER_BLOCK) {
        const int64_t r = base + gid;
        int v = -1, e0 = 0, e1 = 0;
        if (r < g.n_rows && dist[r] < 0) { v = (int)r; e0 = g.indptr[v]; e1 = g.indptr[v + 1]; }
        const bool is_long = G < WAVE && v >= 0 && e1 - e0 > LONG_ROW;
        int best = RC_NONE;
        if (v >= 0 && !is_long) best = rc_walk<G, NEAREST>(g.indices, e0, e1, gl, gmask, v, want, g.n_rows, dist, nearest);
        best = rc_group_min<G>(best);
        if (gl == 0 && best != RC_NONE) {
            dist[v] = level;
            if (NEAREST) nearest[v] = best;
            mine++;
        }
        if (G < WAVE) {                                         // the rows left to the whole wave, one after another
            unsigned long long todo = __ballot(is_long && gl == 0);
            while (todo) {
                const int src = __ffsll((long long)todo) - 1;
                todo &= todo - 1;
                const int wv = __shfl(v, src, WAVE), w0 = __shfl(e0, src, WAVE), w1 = __shfl(e1, src, WAVE);
                const int wb = rc_group_min<WAVE>(rc_walk<WAVE, NEAREST>(g.indices, w0, w1, lane, ~0ull, wv, want, g.n_rows, dist, nearest));
                if (lane == src && wb != RC_NONE) {
                    dist[wv] = level;
                    if (NEAREST) nearest[wv] = wb;
                    mine++;
                }
            }
        }
    }
    rc_block_add(mine, reached);
}

__global__ __launch_bounds__(RC_THREADS) void hop_clear_kernel(int n_rows, int32_t *__restrict__ dist, int32_t *__restrict__ nearest,
                                                               unsigned long long *__restrict__ counters, int n_counters) {
    const int64_t i = (int64_t)blockIdx.x * RC_THREADS + threadIdx.x;
    if (i < n_rows) {
        dist[i] = -1;
        if (nearest) nearest[i] = -1;
    }
    if (i < n_counters) counters[i] = 0;
}

// counters[0] += the rows that became seeds, counters[1] += the seeds outside the graph
__global__ __launch_bounds__(RC_THREADS) void hop_seed_kernel(const int32_t *__restrict__ seeds, int n_seeds, int n_rows, int32_t *dist,
                                                              int32_t *nearest, unsigned long long *counters) {
    const int64_t i = (int64_t)blockIdx.x * RC_THREADS + threadIdx.x;
    if (i >= n_seeds) return;
    const int r = seeds[i];
    if (r < 0 || r >= n_rows) { atomicAdd(&counters[1], 1ull); return; }
    if (atomicExch(&dist[r], 0) != 0) {                        // the first of a repeated seed
        atomicAdd(&counters[0], 1ull);
        if (nearest) nearest[r] = r;
    }
}

// ---- the components --------------------------------------------------------------------------------------------------------

__device__ inline bool rc_hook(int u, int v, int pv, int n_rows, int32_t *parent) {
    if (u == v || (unsigned)u >= (unsigned)n_rows) return false;
    const int pu = parent[u];
    if (pu == pv) return false;
    atomicMin(&parent[max(pu, pv)], min(pu, pv));
    return true;
}

template <int W>
__device__ inline bool rc_hook_walk(const int *__restrict__ indices, int e0, int e1, int lane, int v, int pv, int n_rows, int32_t *parent) {
    bool any = false;
    const int a0 = (e0 + 3) & ~3, a1 = e1 & ~3;
    if (a0 >= a1) {
        for (int e = e0 + lane; e < e1; e += W) any |= rc_hook(indices[e], v, pv, n_rows, parent);
        return any;
    }
    if (lane < a0 - e0) any |= rc_hook(indices[e0 + lane], v, pv, n_rows, parent);
    if (lane < e1 - a1) any |= rc_hook(indices[a1 + lane], v, pv, n_rows, parent);
    const int4 *__restrict__ quads = (const int4 *)indices;
    const int q1 = a1 >> 2;
    for (int q = (a0 >> 2) + lane; q < q1; q += W) {
        const int4 x = quads[q];
        any |= rc_hook(x.x, v, pv, n_rows, parent);
        any |= rc_hook(x.y, v, pv, n_rows, parent);
        any |= rc_hook(x.z, v, pv, n_rows, parent);
        any |= rc_hook(x.w, v, pv, n_rows, parent);
    }
    return any;
}

template <int G>
__global__ __launch_bounds__(RC_THREADS) void comp_hook_kernel(RcGraph g, int32_t *parent, int32_t *changed) {
    constexpr int PER_BLOCK = RC_THREADS / G, LONG_ROW = 64 * G;
    const int lane = threadIdx.x & (WAVE - 1), gl = threadIdx.x & (G - 1), gid = threadIdx.x / G;
    bool any = false;
    for (int64_t base = (int64_t)blockIdx.x * PER_BLOCK; base < g.n_rows; base += (int64_t)gridDim.x * PER_BLOCK) {
        const int64_t r = base + gid;
        int v = -1, e0 = 0, e1 = 0, pv = 0;
        if (r < g.n_rows) { v = (int)r; e0 = g.indptr[v]; e1 = g.indptr[v + 1]; pv = parent[v]; }
        const bool is_long = G < WAVE && v >= 0 && e1 - e0 > LONG_ROW;
        if (v >= 0 && !is_long) any |= rc_hook_walk<G>(g.indices, e0, e1, gl, v, pv, g.n_rows, parent);
        if (G < WAVE) {
            unsigned long long todo = __ballot(is_long && gl == 0);
            while (todo) {
                const int src = __ffsll((long long)todo) - 1;
                todo &= todo - 1;
                const int wv = __shfl(v, src, WAVE), w0 = __shfl(e0, src, WAVE), w1 = __shfl(e1, src, WAVE), wp = __shfl(pv, src, WAVE);
                any |= rc_hook_walk<WAVE>(g.indices, w0, w1, lane, wv, wp, g.n_rows, parent);
            }
        }
    }
    if (__ballot(any) && lane == 0) atomicOr(changed, 1);
}

__global__ __launch_bounds__(RC_THREADS) void comp_init_kernel(int n_rows, int32_t *__restrict__ parent) {
    const int64_t i = (int64_t)blockIdx.x * RC_THREADS + threadIdx.x;
    if (i < n_rows) parent[i] = (int)i;
}

// every row stores its root.  Only thread v writes parent[v], and what another thread reads there is an ancestor before and after.
__global__ __launch_bounds__(RC_THREADS) void comp_jump_kernel(int n_rows, int32_t *parent) {
    const int64_t i = (int64_t)blockIdx.x * RC_THREADS + threadIdx.x;
    if (i >= n_rows) return;
    int p = parent[i];
    for (;;) {                                                  // parent[p] <= p: at most n_rows steps
        const int pp = parent[p];
        if (pp == p) break;
        p = pp;
    }
    parent[i] = p;
}

// ---- counts of the components ------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(RC_THREADS) void comp_zero_kernel(int n_rows, int32_t *__restrict__ size, int32_t *__restrict__ marked,
                                                               unsigned long long *__restrict__ totals) {
    const int64_t i = (int64_t)blockIdx.x * RC_THREADS + threadIdx.x;
    if (i < n_rows) { size[i] = 0; marked[i] = 0; }
    if (i < 6) totals[i] = 0;
}

__global__ __launch_bounds__(RC_THREADS) void comp_size_kernel(int n_rows, const int32_t *__restrict__ comp, const int32_t *__restrict__ mark,
                                                               int32_t *size, int32_t *marked) {
    const int64_t i = (int64_t)blockIdx.x * RC_THREADS + threadIdx.x;
    if (i >= n_rows) return;
    const int r = comp[i];
    if (r < 0 || r >= n_rows) return;
    atomicAdd(&size[r], 1);
    if (mark && mark[i] != 0) atomicAdd(&marked[r], 1);
}

__global__ __launch_bounds__(RC_THREADS) void comp_totals_kernel(int n_rows, const int32_t *__restrict__ comp, const int32_t *__restrict__ size,
                                                                 const int32_t *__restrict__ marked, unsigned long long *__restrict__ totals) {
    __shared__ unsigned long long t[6];
    if (threadIdx.x < 6) t[threadIdx.x] = 0;
    __syncthreads();
    unsigned long long mine[6] = {0, 0, 0, 0, 0, 0};
    for (int64_t i = (int64_t)blockIdx.x * RC_THREADS + threadIdx.x; i < n_rows; i += (int64_t)gridDim.x * RC_THREADS) {
        const int r = comp[i];
        if (r >= 0 && r < n_rows) mine[0]++;
        if (r != (int)i) continue;                              // a root: its component is counted here
        const unsigned long long s = (unsigned)size[i], k = (unsigned)marked[i];
        mine[1]++;
        mine[2] = max(mine[2], s);
        if (k == 0) { mine[3]++; mine[4] += s; }
        mine[5] += k;
    }
#pragma unroll
    for (int k = 0; k < 6; k++) {
        if (!mine[k]) continue;
        if (k == 2) atomicMax(&t[2], mine[2]);
        else atomicAdd(&t[k], mine[k]);
    }
    __syncthreads();
    if (threadIdx.x < 6 && t[threadIdx.x]) {
        if (threadIdx.x == 2) atomicMax(&totals[2], t[2]);
        else atomicAdd(&totals[threadIdx.x], t[threadIdx.x]);
    }
}

// ---- accuracy by distance ----------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(RC_THREADS) void distance_strata_kernel(const int32_t *__restrict__ dist, const int32_t *__restrict__ nearest,
                                                                     const int32_t *__restrict__ pred, const int32_t *__restrict__ truth, int n_rows,
                                                                     const int32_t *__restrict__ d_rows, int n, int C, int hops,
                                                                     unsigned long long *__restrict__ strata, unsigned long long *__restrict__ unlabelled) {
    __shared__ int cell[(RC_MAX_HOPS_BUCKETS + 2) * 4 + 1];     // a workgroup adds at most 2^31 - 1 positions: n is an int
    const int cells = (hops + 2) * 4;
    for (int e = threadIdx.x; e <= cells; e += RC_THREADS) cell[e] = 0;
    __syncthreads();
    for (int64_t i = (int64_t)blockIdx.x * RC_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * RC_THREADS) {
        const int r = d_rows ? d_rows[i] : (int)i;
        if (r < 0 || r >= n_rows) continue;
        const int d = dist[r];
        const int at = (d < 0 ? hops + 1 : min(d, hops)) * 4;
        atomicAdd(&cell[at], 1);
        const int y = truth[r];
        if ((unsigned)y >= (unsigned)C) { atomicAdd(&cell[cells], 1); continue; }
        atomicAdd(&cell[at + 1], 1);
        if (pred && pred[r] == y) atomicAdd(&cell[at + 2], 1);
        if (nearest) {
            const int s = nearest[r];
            if (s >= 0 && s < n_rows && truth[s] == y) atomicAdd(&cell[at + 3], 1);
        }
    }
    __syncthreads();
    for (int e = threadIdx.x; e < cells; e += RC_THREADS)
        if (cell[e]) atomicAdd(&strata[e], (unsigned long long)(unsigned)cell[e]);
    if (threadIdx.x == 0 && cell[cells]) atomicAdd(unlabelled, (unsigned long long)(unsigned)cell[cells]);
}

// ---- entry points ------------------------------------------------------------------------------------------------------------

static int rc_group(const gcnhip_graph *g, int group) {
    if (group) return group;
    const int64_t mean = g->n_rows > 0 ? (int64_t)g->nnz / g->n_rows : 0;
    return mean <= 16 ? 4 : (mean <= 128 ? 16 : 64);
}
static int rc_walk_grid(const gcnhip_ctx *c, int n_rows, int group) {
    return std::max(1, std::min(ceil_div(n_rows, RC_THREADS / group), std::max(c->n_cu, 1) * RC_BLOCKS_PER_CU));
}
static int rc_refuse(const char *name, const char *why) {
    char msg[200];
    snprintf(msg, sizeof msg, "%s: %s", name, why);
    return gcnhip_fail(msg);
}
static bool rc_group_ok(int group) { return group == 0 || group == 4 || group == 16 || group == 64; }

template <bool NEAREST>
static void rc_launch_level(int group, int grid, hipStream_t s, const RcGraph &g, int level, int32_t *dist, int32_t *nearest, unsigned long long *reached) {
    if (group == 4) hop_level_kernel<4, NEAREST><<<grid, RC_THREADS, 0, s>>>(g, level, dist, nearest, reached);
    else if (group == 16) hop_level_kernel<16, NEAREST><<<grid, RC_THREADS, 0, s>>>(g, level, dist, nearest, reached);
    else hop_level_kernel<64, NEAREST><<<grid, RC_THREADS, 0, s>>>(g, level, dist, nearest, reached);
}

extern "C" {

int gcnhip_hop_distance_ex(gcnhip_ctx *c, const gcnhip_graph *g, const int32_t *d_seeds, int n_seeds, int max_hops, int32_t *dist, int32_t *nearest,
                           int64_t *scratch, int *levels, int64_t *level_counts, int capacity, int64_t *skipped, int group, int levels_per_sync) {
    const char *name = "gcnhip_hop_distance";
    if (!c || !g || !dist || !scratch || !levels || !skipped || n_seeds < 0 || max_hops < 0 || capacity < 0 || (n_seeds > 0 && !d_seeds) ||
        (capacity > 0 && !level_counts))
        return rc_refuse(name, "invalid argument");
    if (g->n_rows != g->n_cols) return rc_refuse(name, "a square adjacency object (a row's entries name rows)");
    if (!rc_group_ok(group)) return rc_refuse(name, "the lane group is 0 (by the mean row length), 4, 16 or 64");
    if (levels_per_sync < 1 || levels_per_sync > RC_MAX_SYNC) return rc_refuse(name, "1 <= levels_per_sync <= 64");
    const int n_rows = g->n_rows;
    unsigned long long *counters = (unsigned long long *)scratch;   // [0 .. 63] a batch's levels; after the seeding [0] seeds, [1] skipped
    hop_clear_kernel<<<ceil_div(std::max(n_rows, RC_MAX_SYNC), RC_THREADS), RC_THREADS, 0, c->stream>>>(n_rows, dist, nearest, counters, RC_MAX_SYNC);
    GCNHIP_LAUNCH_CHECK();
    if (n_seeds > 0) {
        hop_seed_kernel<<<ceil_div(n_seeds, RC_THREADS), RC_THREADS, 0, c->stream>>>(d_seeds, n_seeds, n_rows, dist, nearest, counters);
        GCNHIP_LAUNCH_CHECK();
    }
    int64_t h[RC_MAX_SYNC];
    GCNHIP_TRY(hipMemcpyAsync(h, counters, 2 * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
    GCNHIP_TRY(hipStreamSynchronize(c->stream));
    *skipped = h[1];
    *levels = 0;
    if (capacity > 0) level_counts[0] = h[0];
    for (int d = 1; d < capacity; d++) level_counts[d] = 0;
    if (h[0] == 0 || n_rows == 0) return 0;
    group = rc_group(g, group);
    const RcGraph rg = {g->indptr, g->indices, n_rows};
    const int grid = rc_walk_grid(c, n_rows, group);
    const int last = max_hops > 0 ? std::min(max_hops, n_rows - 1) : n_rows - 1;   // no distance passes n_rows - 1
    for (int first = 1; first <= last;) {
        const int k = std::min(levels_per_sync, last - first + 1);
        GCNHIP_TRY(hipMemsetAsync(counters, 0, RC_MAX_SYNC * sizeof(int64_t), c->stream));
        for (int j = 0; j < k; j++) {
            if (nearest) rc_launch_level<true>(group, grid, c->stream, rg, first + j, dist, nearest, counters + j);
            else rc_launch_level<false>(group, grid, c->stream, rg, first + j, dist, nearest, counters + j);
            GCNHIP_LAUNCH_CHECK();
        }
        GCNHIP_TRY(hipMemcpyAsync(h, counters, (size_t)k * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
        GCNHIP_TRY(hipStreamSynchronize(c->stream));
        int j = 0;
        for (; j < k && h[j] > 0; j++) {
            *levels = first + j;
            if (first + j < capacity) level_counts[first + j] = h[j];
        }
        if (j < k) break;                                       // the frontier emptied: the launches behind it changed nothing
        first += k;
    }
    return 0;
}

int gcnhip_hop_distance(gcnhip_ctx *c, const gcnhip_graph *g, const int32_t *d_seeds, int n_seeds, int max_hops, int32_t *dist, int32_t *nearest,
                        int64_t *scratch, int *levels, int64_t *level_counts, int capacity, int64_t *skipped) {
    return gcnhip_hop_distance_ex(c, g, d_seeds, n_seeds, max_hops, dist, nearest, scratch, levels, level_counts, capacity, skipped, 0, 8);
}

int gcnhip_components(gcnhip_ctx *c, const gcnhip_graph *g, int32_t *comp, int64_t *scratch, int *rounds) {
    const char *name = "gcnhip_components";
    if (!c || !g || !comp || !scratch || !rounds) return rc_refuse(name, "invalid argument");
    if (g->n_rows != g->n_cols) return rc_refuse(name, "a square adjacency object (a row's entries name rows)");
    const int n_rows = g->n_rows;
    *rounds = 0;
    if (n_rows == 0) return 0;
    int32_t *changed = (int32_t *)scratch;
    comp_init_kernel<<<ceil_div(n_rows, RC_THREADS), RC_THREADS, 0, c->stream>>>(n_rows, comp);
    GCNHIP_LAUNCH_CHECK();
    const int group = rc_group(g, 0);
    const RcGraph rg = {g->indptr, g->indices, n_rows};
    const int grid = rc_walk_grid(c, n_rows, group);
    for (int round = 1; round <= n_rows + 1; round++) {         // every round but the last lowers a label: the bound is never met
        GCNHIP_TRY(hipMemsetAsync(changed, 0, sizeof(int64_t), c->stream));
        if (group == 4) comp_hook_kernel<4><<<grid, RC_THREADS, 0, c->stream>>>(rg, comp, changed);
        else if (group == 16) comp_hook_kernel<16><<<grid, RC_THREADS, 0, c->stream>>>(rg, comp, changed);
        else comp_hook_kernel<64><<<grid, RC_THREADS, 0, c->stream>>>(rg, comp, changed);
        GCNHIP_LAUNCH_CHECK();
        comp_jump_kernel<<<ceil_div(n_rows, RC_THREADS), RC_THREADS, 0, c->stream>>>(n_rows, comp);
        GCNHIP_LAUNCH_CHECK();
        int32_t h = 0;
        GCNHIP_TRY(hipMemcpyAsync(&h, changed, sizeof h, hipMemcpyDeviceToHost, c->stream));
        GCNHIP_TRY(hipStreamSynchronize(c->stream));
        *rounds = round;
        if (!h) return 0;
    }
    return rc_refuse(name, "the labelling did not settle within n_rows + 1 rounds");
}

int gcnhip_component_counts(gcnhip_ctx *c, const int32_t *comp, const int32_t *mark, int n_rows, int32_t *size, int32_t *marked, int64_t *totals) {
    if (!c || !totals || n_rows < 0 || (n_rows > 0 && (!comp || !size || !marked))) return rc_refuse("gcnhip_component_counts", "invalid argument");
    const int blocks = ceil_div(std::max(n_rows, 6), RC_THREADS);
    comp_zero_kernel<<<blocks, RC_THREADS, 0, c->stream>>>(n_rows, size, marked, (unsigned long long *)totals);
    GCNHIP_LAUNCH_CHECK();
    if (n_rows == 0) return 0;
    comp_size_kernel<<<blocks, RC_THREADS, 0, c->stream>>>(n_rows, comp, mark, size, marked);
    GCNHIP_LAUNCH_CHECK();
    comp_totals_kernel<<<std::min(blocks, 256), RC_THREADS, 0, c->stream>>>(n_rows, comp, size, marked, (unsigned long long *)totals);
    GCNHIP_LAUNCH_CHECK();
    return 0;
}

int gcnhip_distance_strata(gcnhip_ctx *c, const int32_t *dist, const int32_t *nearest, const int32_t *pred, const int32_t *truth, int n_rows,
                           const int32_t *d_rows, int n, int num_classes, int hops, int64_t *strata, int64_t *unlabelled) {
    const char *name = "gcnhip_distance_strata";
    if (!c || !strata || !unlabelled || n < 0 || n_rows < 0 || (n > 0 && n_rows > 0 && (!dist || !truth))) return rc_refuse(name, "invalid argument");
    if (num_classes < 1) return rc_refuse(name, "num_classes >= 1");
    if (hops < 1 || hops > RC_MAX_HOPS_BUCKETS) return rc_refuse(name, "1 <= hops <= 32");
    GCNHIP_TRY(hipMemsetAsync(strata, 0, (size_t)(hops + 2) * 4 * sizeof(int64_t), c->stream));
    GCNHIP_TRY(hipMemsetAsync(unlabelled, 0, sizeof(int64_t), c->stream));
    if (n == 0 || n_rows == 0) return 0;
    distance_strata_kernel<<<std::min(ceil_div(n, RC_THREADS), 256), RC_THREADS, 0, c->stream>>>(
        dist, nearest, pred, truth, n_rows, d_rows, n, num_classes, hops, (unsigned long long *)strata, (unsigned long long *)unlabelled);
    GCNHIP_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
