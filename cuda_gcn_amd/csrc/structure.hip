// structure.hip — where on the graph a labelling agrees with itself: per listed row the number of neighbours that carry its label,
// the class x class mixing counts of the edges, and the accuracy of a prediction by degree and by neighbourhood agreement.
// Beyond the reference, which never looks at its adjacency after building it.  Every number is an integer count formed with integer
// atomics: any grid, any lane grouping, any flush interval and any launch give the same bits.
//
// DEFINITIONS (the contract; tests/structure_ref.py states them again in Python integers)
//   The adjacency object g holds stored rows as the loader made them: the self loop is included, a repeated entry counts as often
//   as it is stored, one-way entries are allowed (gcnhip_graph_arrays names the arrays).  lab is int32, one entry per COLUMN of g.
//   Label x is KNOWN when 0 <= x < C, 1 <= C <= 64.  A query lists n positions; d_rows[i] is the row of position i (NULL: row i);
//   repeats count as often as listed; a position whose row is outside [0, n_rows) counts in `skipped` and nowhere else (its three
//   per-position outputs are 0), as in gcnhip_contingency_rows.
//   For position i with row v, the entries u of row v with u != v are its NON-LOOP entries.
//     deg[i]   = the number of non-loop entries.
//     lab[v] known:   known[i] = the non-loop entries with lab[u] known;  same[i] = those of them with lab[u] == lab[v];
//                     mix[lab[v] * C + lab[u]] += 1 for each of them;  class_rows[lab[v]] += 1.
//     lab[v] unknown: known[i] = same[i] = 0; the position is an unlabelled row (totals[0] - totals[1] counts them).
//   totals [8] int64 = {listed rows in range, labelled rows, rows with known > 0, sum deg, sum known, sum same, self entries seen,
//     ratio_sum}, ratio_sum = the sum over the rows with known > 0 of floor(same . 2^32 / known), formed in 64-bit integers and
//     added as an unsigned 64-bit integer: node homophily = ratio_sum / 2^32 / rows with known > 0, an exact integer sum whatever
//     the launch geometry, within 2^-32 of the float64 mean of same / known.
//   Strata of a query (gcnhip_strata_counts; pred and truth are indexed by ROW, deg / same / known by list position):
//     db(i) = 0 when deg[i] <= 0, else 1 + floor(log2 deg[i])                                  (32 degree buckets)
//     ab(i) = bins when known[i] <= 0 (no labelled neighbour), else min(bins - 1, floor(same[i] . bins / known[i])) in 64-bit
//             integers, same[i] taken inside [0, known[i]]                                      (bins + 1 agreement buckets)
//     strata[(db * (bins + 1) + ab) * 2 + 0] = the positions whose truth is known, [.. + 1] = those of them with pred == truth;
//     a position with an unknown truth counts in *unlabelled; one whose row is outside [0, n_truth) counts nowhere.
//
// gcnhip_nbr_agreement   ONE walk over the index stream of the listed rows: 4 bytes per stored entry, and one label gathered per
//   entry of a labelled row from a table that stays in L2 (932 KB for 233 k nodes).  A lane group of G lanes takes a row, G = 4,
//   16 or 64 by the object's mean stored row length (at most 16 / at most 128 / above), so that short rows fill a wave with 16 or
//   4 rows and hub rows do not serialise on a lane.  A group reads its row as aligned 16-byte vectors (the entries before the
//   first and after the last aligned quad one per lane).  A row of more than 64 G entries (16 vector steps of its group) is left
//   to the whole wave, which takes such rows one after another behind the group step: no block-wide step anywhere in the walk.
//   Counts of a row are reduced over its lanes by shuffles; a thread keeps the eight totals in registers, a wave reduces them by
//   shuffles, the workgroup in LDS, and one 64-bit atomic per total and workgroup reaches global memory at the end (Guideline 12:
//   nothing per entry does).  Atomics on ONE address from many workgroups queue behind each other (measured on reddit-syn: about
//   90 ns each, 0.38 ms of a 0.47 ms launch with 4 096 waves adding their own totals), so the launch is two workgroups of
//   16 waves per CU and no more, and a workgroup starts its walk over the histogram cells at an offset of its own, so that the
//   workgroups that finish together do not meet on one cell.
//   MIXING COUNTS: an LDS histogram of C x C int32 cells per workgroup (at most 16 KB).  The diagonal cell of a row — the hot
//   one on an assortative graph — is added once per row from the row's `same`; only entries with another label are LDS atomics.
//   FLUSH BOUND: a cell is moved to the int64 table by atomicExch(cell, 0) + one 64-bit global atomic, which loses no increment
//   and needs no barrier, so any wave may flush at any time.  A wave counts an upper bound of the entries it walked since its own
//   last flush — 64 . 64 = 4096 per group step (64 / G rows of at most 64 G entries), 8 per whole-wave row for the entries outside
//   its quads and 256 per vector step of it — and flushes the whole histogram when that reaches F = 2^26: at the head of a group
//   step and behind every vector step of a whole-wave row.  The diagonal share of a row arrives when the row is finished, so it
//   may have been counted before the wave's last flush: it goes through LDS only when it is at most 2^16, else straight to the
//   int64 table.  Between two zeroings of a cell each of the 16 waves has therefore added at most F + 4096 + 8 + 256 + 2^16 to
//   it (else it would have zeroed it itself), and no cell passes 16 . (2^26 + 69896) < 2^31.
//   gcnhip_nbr_agreement_ex takes G and F as arguments (0: the defaults), so that a test reaches every path on a small graph.
// gcnhip_strata_counts   a thread per list position, an LDS table of 32 x (bins + 1) x 2 int32 cells (a workgroup adds at most
//   2^31 - 1 positions: n is an int), 64-bit atomics behind it.
// The entry points zero their own outputs (one small launch for the four tables of the agreement call), allocate nothing and
// synchronise nothing.
#include "common.h"
#include <algorithm>
#include <cstdio>

constexpr int ST_MAX_C = 64, ST_MAX_BINS = 32, ST_DEG_BUCKETS = 32;
constexpr int ST_THREADS = 1024;                              // 16 waves share one histogram
constexpr int ST_BLOCKS_PER_CU = 2;
constexpr int ST_STRATA_THREADS = 256;
constexpr unsigned long long ST_FLUSH_DEFAULT = 1ull << 26;   // F of the flush bound above
constexpr unsigned long long ST_FLUSH_MAX = 1ull << 26;       // a larger F would break the bound
constexpr int ST_DIAG_DIRECT = 1 << 16;                       // a row's `same` above this goes to the int64 table directly

struct StGraph {
    const int *__restrict__ indptr;
    const int *__restrict__ indices;
    int n_rows, n_cols;
};

// what a lane has counted of the row it walks
struct StRow {
    int deg, known, same, self;
};

// the label an entry is counted with: -2 for the self entry, -1 without a known label (an unlabelled row gathers nothing)
__device__ inline int st_gather(int u, int v, int lv, int C, int n_cols, const int32_t *__restrict__ lab) {
    if (u == v) return -2;
    if (lv < 0 || (unsigned)u >= (unsigned)n_cols) return -1;
    const int lu = lab[u];
    return (unsigned)lu < (unsigned)C ? lu : -1;
}
__device__ inline void st_tally(int lu, int lv, int C, int *__restrict__ cell, StRow &c) {
    if (lu == -2) { c.self++; return; }
    c.deg++;
    if (lu < 0) return;
    c.known++;
    if (lu == lv) c.same++;
    else if (cell) atomicAdd(&cell[lv * C + lu], 1);
}
__device__ inline void st_visit(int u, int v, int lv, int C, int n_cols, const int32_t *__restrict__ lab, int *__restrict__ cell, StRow &c) {
    st_tally(st_gather(u, v, lv, C, n_cols, lab), lv, C, cell, c);
}

// a wave moves every cell of the workgroup's histogram to the int64 table; no barrier (see FLUSH BOUND)
__device__ inline void st_flush(int *__restrict__ cell, int cells, unsigned long long *__restrict__ mix, int lane) {
    for (int e = lane; e < cells; e += WAVE) {
        const int x = atomicExch(&cell[e], 0);
        if (x) atomicAdd(&mix[e], (unsigned long long)(unsigned)x);
    }
}

// W lanes (lane = 0 .. W - 1) walk the entries [e0, e1) of a row.  W == 64: the whole wave, every control decision wave-uniform,
// the flush bound kept per vector step.
template <int W>
__device__ inline void st_walk(const int *__restrict__ indices, int e0, int e1, int lane, int v, int lv, int C, int n_cols,
                               const int32_t *__restrict__ lab, int *__restrict__ cell, StRow &c, unsigned long long *__restrict__ mix,
                               unsigned long long &walked, unsigned long long flush_every) {
    const int a0 = (e0 + 3) & ~3, a1 = e1 & ~3;                 // the aligned quads are [a0, a1)
    if (W == WAVE) walked += 8;                                 // the entries outside the quads, or a row without a quad
    if (a0 >= a1) {                                             // fewer than 7 entries
        for (int e = e0 + lane; e < e1; e += W) st_visit(indices[e], v, lv, C, n_cols, lab, cell, c);
        return;
    }
    if (lane < a0 - e0) st_visit(indices[e0 + lane], v, lv, C, n_cols, lab, cell, c);
    if (lane < e1 - a1) st_visit(indices[a1 + lane], v, lv, C, n_cols, lab, cell, c);
    const int4 *__restrict__ quads = (const int4 *)indices;     // the index array is a device allocation: 256-byte aligned
    const int q1 = a1 >> 2;
    for (int qb = a0 >> 2; qb < q1; qb += W) {                  // uniform over the W lanes
        const int q = qb + lane;
        if (q < q1) {
            const int4 x = quads[q];                            // the four gathers are in flight before the first count
            const int l0 = st_gather(x.x, v, lv, C, n_cols, lab), l1 = st_gather(x.y, v, lv, C, n_cols, lab);
            const int l2 = st_gather(x.z, v, lv, C, n_cols, lab), l3 = st_gather(x.w, v, lv, C, n_cols, lab);
            st_tally(l0, lv, C, cell, c);
            st_tally(l1, lv, C, cell, c);
            st_tally(l2, lv, C, cell, c);
            st_tally(l3, lv, C, cell, c);
        }
        if (W == WAVE && cell) {
            walked += 4 * WAVE;
            if (walked >= flush_every) { st_flush(cell, C * C, mix, lane); walked = 0; }
        }
    }
}

template <int W>
__device__ inline StRow st_reduce(StRow c) {
#pragma unroll
    for (int off = W / 2; off > 0; off >>= 1) {
        c.deg += __shfl_xor(c.deg, off, WAVE);
        c.known += __shfl_xor(c.known, off, WAVE);
        c.same += __shfl_xor(c.same, off, WAVE);
        c.self += __shfl_xor(c.self, off, WAVE);
    }
    return c;
}

__device__ inline unsigned long long st_wave_sum(unsigned long long x) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned lo = __shfl_xor((unsigned)x, off, WAVE), hi = __shfl_xor((unsigned)(x >> 32), off, WAVE);
        x += ((unsigned long long)hi << 32) | lo;
    }
    return x;
}

// the eight totals and the skipped positions, as one lane holds them
struct StTotals {
    unsigned long long v[9];
};

// one lane finishes a row in range: the per-position outputs, the row's share of the totals, its class and its diagonal cell
__device__ inline void st_finish(int i, int lv, const StRow &c, int C, int32_t *__restrict__ deg, int32_t *__restrict__ same, int32_t *__restrict__ known,
                                 int *__restrict__ cell, int *__restrict__ crow, unsigned long long *__restrict__ mix, StTotals &t) {
    if (deg) deg[i] = c.deg;
    if (same) same[i] = c.same;
    if (known) known[i] = c.known;
    t.v[0] += 1;
    t.v[3] += (unsigned)c.deg;
    t.v[6] += (unsigned)c.self;
    if (lv < 0) return;
    t.v[1] += 1;
    atomicAdd(&crow[lv], 1);
    if (c.known > 0) {
        t.v[2] += 1;
        t.v[4] += (unsigned)c.known;
        t.v[5] += (unsigned)c.same;
        t.v[7] += ((unsigned long long)(unsigned)c.same << 32) / (unsigned long long)(unsigned)c.known;
        if (cell && c.same > ST_DIAG_DIRECT) atomicAdd(&mix[lv * C + lv], (unsigned long long)(unsigned)c.same);
        else if (cell && c.same) atomicAdd(&cell[lv * C + lv], c.same);
    }
}

template <int G>
__global__ __launch_bounds__(ST_THREADS) void nbr_agreement_kernel(StGraph g, const int32_t *__restrict__ lab, int C, const int32_t *__restrict__ d_rows,
                                                                   int n, int32_t *__restrict__ deg, int32_t *__restrict__ same,
                                                                   int32_t *__restrict__ known, unsigned long long *__restrict__ mix,
                                                                   unsigned long long *__restrict__ class_rows, unsigned long long *__restrict__ totals,
                                                                   unsigned long long *__restrict__ skipped, unsigned long long flush_every) {
    extern __shared__ int st_lds[];
    __shared__ unsigned long long block_totals[9];
    int *crow = st_lds;                                         // [C] labelled rows per class
    int *cell = mix ? st_lds + C : nullptr;                     // [C x C] the mixing counts since the last flush
    const int cells = mix ? C * C : 0;
    for (int e = threadIdx.x; e < C + cells; e += ST_THREADS) st_lds[e] = 0;
    if (threadIdx.x < 9) block_totals[threadIdx.x] = 0;
    __syncthreads();

    constexpr int PER_BLOCK = ST_THREADS / G, LONG_ROW = 64 * G;
    const int lane = threadIdx.x & (WAVE - 1), gl = threadIdx.x & (G - 1), gid = threadIdx.x / G;
    StTotals t = {};
    unsigned long long walked = 0;                              // wave-uniform

    for (int64_t base = (int64_t)blockIdx.x * PER_BLOCK; base < n; base += (int64_t)gridDim.x * PER_BLOCK) {
        if (cell) {
            if (walked >= flush_every) { st_flush(cell, cells, mix, lane); walked = 0; }
            if (G < WAVE) walked += WAVE * WAVE;                // 64 / G rows of at most 64 G entries
        }
        const int64_t i64 = base + gid;
        const int i = (int)(i64 < n ? i64 : -1);
        int v = -1, e0 = 0, e1 = 0;
        if (i >= 0) {
            const int r = d_rows ? d_rows[i] : i;
            if (r >= 0 && r < g.n_rows) { v = r; e0 = g.indptr[r]; e1 = g.indptr[r + 1]; }
            else if (gl == 0) {
                t.v[8] += 1;
                if (deg) deg[i] = 0;
                if (same) same[i] = 0;
                if (known) known[i] = 0;
            }
        }
        int lv = v >= 0 && v < g.n_cols ? lab[v] : -1;
        if ((unsigned)lv >= (unsigned)C) lv = -1;
        const bool is_long = G < WAVE && v >= 0 && e1 - e0 > LONG_ROW;
        StRow c = {0, 0, 0, 0};
        if (v >= 0 && !is_long) st_walk<G>(g.indices, e0, e1, gl, v, lv, C, g.n_cols, lab, cell, c, mix, walked, flush_every);
        c = st_reduce<G>(c);
        if (gl == 0 && v >= 0 && !is_long) st_finish(i, lv, c, C, deg, same, known, cell, crow, mix, t);
        if (G < WAVE) {                                         // the rows left to the whole wave, one after another
            unsigned long long todo = __ballot(is_long && gl == 0);
            while (todo) {
                const int src = __ffsll((long long)todo) - 1;
                todo &= todo - 1;
                const int wi = __shfl(i, src, WAVE), wv = __shfl(v, src, WAVE), wlv = __shfl(lv, src, WAVE);
                const int w0 = __shfl(e0, src, WAVE), w1 = __shfl(e1, src, WAVE);
                StRow w = {0, 0, 0, 0};
                st_walk<WAVE>(g.indices, w0, w1, lane, wv, wlv, C, g.n_cols, lab, cell, w, mix, walked, flush_every);
                w = st_reduce<WAVE>(w);
                if (lane == src) st_finish(wi, wlv, w, C, deg, same, known, cell, crow, mix, t);
            }
        }
    }

#pragma unroll
    for (int k = 0; k < 9; k++) {
        const unsigned long long s = st_wave_sum(t.v[k]);
        if (lane == 0 && s) atomicAdd(&block_totals[k], s);
    }
    __syncthreads();                                            // every wave's LDS atomics are done
    if (threadIdx.x < 9 && block_totals[threadIdx.x]) atomicAdd(threadIdx.x < 8 ? &totals[threadIdx.x] : skipped, block_totals[threadIdx.x]);
    const int first = cells ? (int)((blockIdx.x * 192u) % (unsigned)cells) : 0;   // a start of its own: 3 wave-widths further per workgroup
    for (int k = threadIdx.x; k < cells; k += ST_THREADS) {
        const int e = first + k < cells ? first + k : first + k - cells;
        if (cell[e]) atomicAdd(&mix[e], (unsigned long long)(unsigned)cell[e]);
    }
    for (int e = threadIdx.x; e < C; e += ST_THREADS)
        if (crow[e]) atomicAdd(&class_rows[e], (unsigned long long)(unsigned)crow[e]);
}

// the four tables of the agreement call, zeroed by one launch
__global__ __launch_bounds__(256) void st_zero_kernel(unsigned long long *__restrict__ mix, int cells, unsigned long long *__restrict__ class_rows, int C,
                                                      unsigned long long *__restrict__ totals, unsigned long long *__restrict__ skipped) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (mix && i < cells) mix[i] = 0;
    if (i < C) class_rows[i] = 0;
    if (i < 8) totals[i] = 0;
    if (i == 0) *skipped = 0;
}

__global__ __launch_bounds__(ST_STRATA_THREADS) void strata_counts_kernel(const int32_t *__restrict__ deg, const int32_t *__restrict__ same,
                                                                   const int32_t *__restrict__ known, const int32_t *__restrict__ pred,
                                                                   const int32_t *__restrict__ truth, int n_truth, const int32_t *__restrict__ d_rows,
                                                                   int n, int C, int bins, unsigned long long *__restrict__ strata,
                                                                   unsigned long long *__restrict__ unlabelled) {
    extern __shared__ int st_lds[];                             // [32 x (bins + 1) x 2], then the unlabelled count
    const int cells = ST_DEG_BUCKETS * (bins + 1) * 2;
    for (int e = threadIdx.x; e <= cells; e += ST_STRATA_THREADS) st_lds[e] = 0;
    __syncthreads();
    for (int64_t i = (int64_t)blockIdx.x * ST_STRATA_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * ST_STRATA_THREADS) {
        const int r = d_rows ? d_rows[i] : (int)i;
        if (r < 0 || r >= n_truth) continue;
        const int y = truth[r];
        if ((unsigned)y >= (unsigned)C) { atomicAdd(&st_lds[cells], 1); continue; }
        const int d = deg[i], k = known[i];
        const int s = min(max(same[i], 0), max(k, 0));
        const int db = d <= 0 ? 0 : 32 - __clz(d);              // 1 + floor(log2 d), at most 31
        const int ab = k <= 0 ? bins : min(bins - 1, (int)((int64_t)s * bins / k));
        const int at = (db * (bins + 1) + ab) * 2;
        atomicAdd(&st_lds[at], 1);
        if (pred[r] == y) atomicAdd(&st_lds[at + 1], 1);
    }
    __syncthreads();
    for (int e = threadIdx.x; e < cells; e += ST_STRATA_THREADS)
        if (st_lds[e]) atomicAdd(&strata[e], (unsigned long long)(unsigned)st_lds[e]);
    if (threadIdx.x == 0 && st_lds[cells]) atomicAdd(unlabelled, (unsigned long long)(unsigned)st_lds[cells]);
}

extern "C" {

int gcnhip_nbr_agreement_ex(gcnhip_ctx *c, const gcnhip_graph *g, const int32_t *lab, int num_classes, const int32_t *d_rows, int n, int32_t *deg,
                            int32_t *same, int32_t *known, int64_t *mix, int64_t *class_rows, int64_t *totals, int64_t *skipped, int group,
                            int64_t flush_every) {
    const char *name = "gcnhip_nbr_agreement";
    char msg[160];
    const char *why = nullptr;
    if (!c || !g || !lab || !class_rows || !totals || !skipped || n < 0) why = "invalid argument";
    else if (num_classes < 1 || num_classes > ST_MAX_C) why = "1 <= num_classes <= 64";
    else if (group != 0 && group != 4 && group != 16 && group != 64) why = "the lane group is 0 (by the mean row length), 4, 16 or 64";
    else if (flush_every < 0 || (unsigned long long)flush_every > ST_FLUSH_MAX) why = "the flush interval is 0 (the default) .. 2^26 entries";
    if (why) {
        snprintf(msg, sizeof msg, "%s: %s", name, why);
        return gcnhip_fail(msg);
    }
    const int C = num_classes;
    unsigned long long *m64 = (unsigned long long *)mix, *r64 = (unsigned long long *)class_rows, *t64 = (unsigned long long *)totals,
                       *s64 = (unsigned long long *)skipped;
    st_zero_kernel<<<ceil_div(std::max(C * C, 8), 256), 256, 0, c->stream>>>(m64, C * C, r64, C, t64, s64);
    GCNHIP_LAUNCH_CHECK();
    if (n == 0) return 0;
    if (!group) {
        const int64_t mean = g->n_rows > 0 ? (int64_t)g->nnz / g->n_rows : 0;
        group = mean <= 16 ? 4 : (mean <= 128 ? 16 : 64);
    }
    const unsigned long long F = flush_every ? (unsigned long long)flush_every : ST_FLUSH_DEFAULT;
    const StGraph sg = {g->indptr, g->indices, g->n_rows, g->n_cols};
    const size_t lds = ((size_t)C + (mix ? (size_t)C * C : 0)) * sizeof(int);
    const int grid = std::max(1, std::min(ceil_div(n, ST_THREADS / group), std::max(c->n_cu, 1) * ST_BLOCKS_PER_CU));
    if (group == 4) nbr_agreement_kernel<4><<<grid, ST_THREADS, lds, c->stream>>>(sg, lab, C, d_rows, n, deg, same, known, m64, r64, t64, s64, F);
    else if (group == 16) nbr_agreement_kernel<16><<<grid, ST_THREADS, lds, c->stream>>>(sg, lab, C, d_rows, n, deg, same, known, m64, r64, t64, s64, F);
    else nbr_agreement_kernel<64><<<grid, ST_THREADS, lds, c->stream>>>(sg, lab, C, d_rows, n, deg, same, known, m64, r64, t64, s64, F);
    GCNHIP_LAUNCH_CHECK();
    return 0;
}

int gcnhip_nbr_agreement(gcnhip_ctx *c, const gcnhip_graph *g, const int32_t *lab, int num_classes, const int32_t *d_rows, int n, int32_t *deg,
                         int32_t *same, int32_t *known, int64_t *mix, int64_t *class_rows, int64_t *totals, int64_t *skipped) {
    return gcnhip_nbr_agreement_ex(c, g, lab, num_classes, d_rows, n, deg, same, known, mix, class_rows, totals, skipped, 0, 0);
}

int gcnhip_strata_counts(gcnhip_ctx *c, const int32_t *deg, const int32_t *same, const int32_t *known, const int32_t *pred, const int32_t *truth,
                         int n_truth, const int32_t *d_rows, int n, int num_classes, int bins, int64_t *strata, int64_t *unlabelled) {
    if (!c || !strata || !unlabelled || !pred || !truth || n < 0 || n_truth < 0 || (n > 0 && (!deg || !same || !known)))
        return gcnhip_fail("gcnhip_strata_counts: invalid argument");
    if (num_classes < 1 || num_classes > ST_MAX_C) return gcnhip_fail("gcnhip_strata_counts: 1 <= num_classes <= 64");
    if (bins < 1 || bins > ST_MAX_BINS) return gcnhip_fail("gcnhip_strata_counts: 1 <= bins <= 32");
    const int cells = ST_DEG_BUCKETS * (bins + 1) * 2;
    GCNHIP_TRY(hipMemsetAsync(strata, 0, (size_t)cells * sizeof(int64_t), c->stream));
    GCNHIP_TRY(hipMemsetAsync(unlabelled, 0, sizeof(int64_t), c->stream));
    if (n == 0) return 0;
    strata_counts_kernel<<<std::min(ceil_div(n, ST_STRATA_THREADS), 256), ST_STRATA_THREADS, (size_t)(cells + 1) * sizeof(int), c->stream>>>(
        deg, same, known, pred, truth, n_truth, d_rows, n, num_classes, bins, (unsigned long long *)strata, (unsigned long long *)unlabelled);
    GCNHIP_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
