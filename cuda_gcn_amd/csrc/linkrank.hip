// linkrank.hip — how good is a link scorer?  The rank a held-out edge (s, d) takes among every other row c of a table as a candidate
// end, in the filtered setting (the edges the graph already holds do not count against it), matrix-free: the nq x n_table scores
// are formed on the exact-f32 MFMA, compared with the edge's own score and counted; two integers per query leave the GPU.  Beyond
// the reference, which never looks at its hidden matrix.  include/gcnhip_driver.h has the definitions.
//
// The table contract and score(q, c) are embed.hip's.  Every dot product of this file is ONE chain: v_mfma_f32_16x16x4_f32 over the
// columns in 16-column groups c = 0 .. ceil(dim / 16) - 1, inside a group step s = 0..3 with k-slot kg = 0..3 on column
// 16 c + 4 kg + s, columns >= dim as zeros (lr_products).  The bits of an entry depend on the two rows' contents alone — not on the
// lane, wave, tile, chunk or launch that holds them — so equal rows give equal scores, and the threshold t_i = score(s_i, d_i) is
// taken from the same body: the rows d_i of a query tile are gathered into a candidate tile and the diagonal entry is kept.
//
// link_thr_kernel<DP>    grid (query tiles of 64).  Writes t_i (NaN: s_i or d_i outside the table) and, for the whole call, the start
//                        of the counts: 0, or -1 for such a query.
// link_walk_kernel<DP>   grid (query tiles, candidate chunks), 256 threads.  Wave w owns queries 16 w .. 16 w + 15.  Lane (kg, l15)
//                        holds the query row 16 w + l15 as the B operand in REGISTERS and, of every tile of 64 candidates, the entries
//                        of columns 16 g + 4 kg + r (g, r < 4) of that ONE query: t_i, s_i, d_i, both counts and the filter cursor are
//                        that lane's registers.  The chunk's candidate rows stream where they lie in the table, 64 at a time through
//                        double-buffered LDS: the loads of tile t + 1 are in flight across the products of tile t, one barrier per
//                        tile.  No score tile, no list.  What is no candidate is ONE 64-bit mask per query and tile: the columns past
//                        the chunk, d_i, s_i with exclude_self, and the members of the filter set — so each is removed once however
//                        many of these it is.  The filter set of row s_i is sorted; the lane keeps a cursor and the id under it (a
//                        binary search places it at the chunk's first row), and per tile compares that one register with the tile's
//                        end: past it, the common case, nothing else happens; else the ids inside the tile become mask bits and the
//                        cursor moves on.  An id is compared, never used as an index.  At the end the four lanes of a query meet by
//                        two shuffles and the chunk's counts leave by one int32 atomicAdd per query and count.
// DP is 128 or 256 (the register operand and the LDS row); the groups past ceil(dim / 16) are skipped by a uniform test.
// Integer atomics only: any chunking and batching and two launches give the same integers.  Nothing allocates or synchronises.
#include "common.h"
#include <algorithm>
#include <cmath>
#include <cstdio>

using f32x4 = __attribute__((ext_vector_type(4))) float;

constexpr int LR_T = 64;                          // queries per workgroup, candidates per tile
constexpr int LR_MAX_DIM = 256;

struct LrTable {
    const float *data;
    int ld, n, dim;
    const float *inv_norm;
    int vec_ok, nch;                              // rows are 16-byte aligned; 16-column groups that hold a column below dim
};

// columns col .. col + 3 of row r; zeros past dim and for r < 0 (columns [dim, ld) are never read)
__device__ __forceinline__ f32x4 lr_row4(const LrTable &T, int r, int col) {
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (r < 0) return v;
    const float *p = T.data + (size_t)r * T.ld + col;
    if (T.vec_ok && col + 3 < T.dim) return *(const f32x4 *)p;
    if (col < T.dim) v.x = p[0];
    if (col + 1 < T.dim) v.y = p[1];
    if (col + 2 < T.dim) v.z = p[2];
    if (col + 3 < T.dim) v.w = p[3];
    return v;
}

// the query operand of lane (kg, l15): row r, columns 16 c + 4 kg .. + 3
template <int DP>
__device__ __forceinline__ void lr_query_load(const LrTable &T, int r, int kg, f32x4 (&b)[DP / 16]) {
#pragma unroll
    for (int c = 0; c < DP / 16; c++) b[c] = c < T.nch ? lr_row4(T, r, 16 * c + 4 * kg) : f32x4{0.f, 0.f, 0.f, 0.f};
}

template <int DP>
struct LrTile {                                   // what a thread holds of a candidate tile between its loads and its LDS stores
    f32x4 x[DP / 16];
    float inv;
};

// thread e of 256 holds float4 (row, c4) of the tile for idx = e + 256 u: row = idx / (DP / 4), c4 = idx % (DP / 4).  The tile's row
// `row` is table row rows[row] (rows != NULL: a gathered tile, -1: zeros) or min(c0 + row, n - 1): a row that exists, masked later.
template <int DP>
__device__ __forceinline__ void lr_tile_load(LrTile<DP> &L, const LrTable &T, int c0, const int *__restrict__ rows) {
#pragma unroll
    for (int u = 0; u < DP / 16; u++) {
        const int idx = threadIdx.x + 256 * u, row = idx / (DP / 4), col = 4 * (idx % (DP / 4));
        if (col < 16 * T.nch) L.x[u] = lr_row4(T, rows ? rows[row] : min(c0 + row, T.n - 1), col);
    }
    if (threadIdx.x < LR_T) {
        const int r = rows ? rows[threadIdx.x] : min(c0 + (int)threadIdx.x, T.n - 1);
        L.inv = T.inv_norm && r >= 0 ? T.inv_norm[r] : 1.f;
    }
}

template <int DP>
__device__ __forceinline__ void lr_tile_store(const LrTile<DP> &L, const LrTable &T, float *__restrict__ Cs, float *__restrict__ Ns) {
    constexpr int QLD = DP + 4;
#pragma unroll
    for (int u = 0; u < DP / 16; u++) {
        const int idx = threadIdx.x + 256 * u, row = idx / (DP / 4), col = 4 * (idx % (DP / 4));
        if (col < 16 * T.nch) *(f32x4 *)(Cs + row * QLD + col) = L.x[u];
    }
    if (threadIdx.x < LR_T) Ns[threadIdx.x] = L.inv;
}

// THE product body: acc[g][r] = dot(candidate 16 g + 4 kg + r of the tile, this lane's query), one MFMA chain per entry
template <int DP>
__device__ __forceinline__ void lr_products(const float *__restrict__ C, const f32x4 (&b)[DP / 16], f32x4 (&acc)[4], int nch, int kg, int l15) {
    constexpr int QLD = DP + 4;
#pragma unroll
    for (int g = 0; g < 4; g++) acc[g] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int c = 0; c < DP / 16; c++) {
        if (c >= nch) continue;                                 // the same for every thread (no break: b[] keeps static indices)
        f32x4 a[4];
#pragma unroll
        for (int g = 0; g < 4; g++) a[g] = *(const f32x4 *)(C + (16 * g + l15) * QLD + 16 * c + 4 * kg);
#pragma unroll
        for (int s = 0; s < 4; s++)                             // the four accumulators in turn: no MFMA waits for the one before it
#pragma unroll
            for (int g = 0; g < 4; g++) acc[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[g][s], b[c][s], acc[g], 0, 0, 0);
    }
}
__device__ __forceinline__ float lr_score(float dot, float inv_q, float inv_c, bool cosine) { return cosine ? (dot * inv_q) * inv_c : dot; }

__device__ __forceinline__ bool lr_in(int r, int n) { return r >= 0 && r < n; }

// grid (query tiles).  thr [nq]; above / equal [nq] (NULL: the thresholds alone) = 0, or -1 where the query is none
template <int DP>
__global__ __launch_bounds__(256) void link_thr_kernel(LrTable T, const int32_t *__restrict__ src, const int32_t *__restrict__ dst, int nq,
                                                       float *__restrict__ thr, int32_t *__restrict__ above, int32_t *__restrict__ equal) {
    extern __shared__ __align__(16) unsigned char smem[];
    constexpr int QLD = DP + 4;
    float *Cs = (float *)smem;                                  // [64][QLD]
    float *Ns = Cs + LR_T * QLD;                                // [64]
    int *rows = (int *)(Ns + LR_T);                             // [64]: d_i of a valid query, else -1
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, kg = lane >> 4, l15 = lane & 15;
    const int q0 = blockIdx.x * LR_T;
    if (threadIdx.x < LR_T) {
        const int i = q0 + threadIdx.x;
        const int s = i < nq ? src[i] : -1, d = i < nq ? dst[i] : -1;
        const bool ok = lr_in(s, T.n) && lr_in(d, T.n);
        rows[threadIdx.x] = ok ? d : -1;
        if (i < nq && above) { above[i] = ok ? 0 : -1; equal[i] = ok ? 0 : -1; }
    }
    const int i = q0 + 16 * wave + l15;
    const int s = i < nq ? src[i] : -1, d = i < nq ? dst[i] : -1;
    const bool ok = lr_in(s, T.n) && lr_in(d, T.n);
    f32x4 b[DP / 16];
    lr_query_load<DP>(T, ok ? s : -1, kg, b);
    const float inv_q = ok && T.inv_norm ? T.inv_norm[s] : 1.f;
    __syncthreads();
    LrTile<DP> L;
    lr_tile_load<DP>(L, T, 0, rows);
    lr_tile_store<DP>(L, T, Cs, Ns);
    __syncthreads();
    f32x4 acc[4];
    lr_products<DP>(Cs, b, acc, T.nch, kg, l15);
    if (kg == (l15 >> 2) && i < nq) {                           // entry (query 16 w + l15, its own d): g = wave, 4 kg + r = l15
        const f32x4 av = wave == 0 ? acc[0] : wave == 1 ? acc[1] : wave == 2 ? acc[2] : acc[3];
        const int r = l15 & 3;
        const float dot = r == 0 ? av[0] : r == 1 ? av[1] : r == 2 ? av[2] : av[3];
        thr[i] = ok ? lr_score(dot, inv_q, Ns[16 * wave + l15], T.inv_norm != nullptr) : NAN;
    }
}

// grid (query tiles, chunks).  above / equal [nq] += this chunk's counts
template <int DP>
__global__ __launch_bounds__(256) void link_walk_kernel(LrTable T, const int32_t *__restrict__ src, const int32_t *__restrict__ dst, int nq,
                                                        const float *__restrict__ thr, const int32_t *__restrict__ x_ptr,
                                                        const int32_t *__restrict__ x_len, const int32_t *__restrict__ x_ids, int exclude_self,
                                                        int chunk_rows, int32_t *__restrict__ above, int32_t *__restrict__ equal) {
    extern __shared__ __align__(16) unsigned char smem[];
    constexpr int QLD = DP + 4;
    float *Cs = (float *)smem;                                  // [2][64][QLD]
    float *Ns = Cs + 2 * LR_T * QLD;                            // [2][64]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, kg = lane >> 4, l15 = lane & 15;
    const int i = blockIdx.x * LR_T + 16 * wave + l15;
    const int c_begin = blockIdx.y * chunk_rows, c_end = min(T.n, c_begin + chunk_rows);
    const bool cosine = T.inv_norm != nullptr;

    const int s = i < nq ? src[i] : -1, d = i < nq ? dst[i] : -1;
    const bool ok = lr_in(s, T.n) && lr_in(d, T.n);
    f32x4 b[DP / 16];
    lr_query_load<DP>(T, ok ? s : -1, kg, b);
    const float inv_q = ok && cosine ? T.inv_norm[s] : 1.f;
    const float t = ok ? thr[i] : NAN;                          // NaN: above and equal to nothing
    const int self = exclude_self ? s : -1;
    // the filter cursor: [cur, x_end) of x_ids, nxt = the id under it (INT_MAX: none left), placed at the chunk's first row
    int cur = 0, x_end = 0, nxt = 0x7fffffff;
    if (ok && x_ptr) {
        int lo = x_ptr[s];
        x_end = x_len ? lo + x_len[s] : x_ptr[s + 1];
        int hi = x_end;
        while (lo < hi) {
            const int mid = lo + ((hi - lo) >> 1);
            if (x_ids[mid] < c_begin) lo = mid + 1;
            else hi = mid;
        }
        cur = lo;
        if (cur < x_end) nxt = x_ids[cur];
    }
    int n_above = 0, n_equal = 0;

    LrTile<DP> L;
    lr_tile_load<DP>(L, T, c_begin, nullptr);
    lr_tile_store<DP>(L, T, Cs, Ns);
    __syncthreads();
    int buf = 0;
    for (int c0 = c_begin; c0 < c_end; c0 += LR_T, buf ^= 1) {
        const bool more = c0 + LR_T < c_end;
        if (more) lr_tile_load<DP>(L, T, c0 + LR_T, nullptr);   // in flight across the products below
        f32x4 acc[4];
        lr_products<DP>(Cs + buf * LR_T * QLD, b, acc, T.nch, kg, l15);
        // what is no candidate of this query in this tile
        const int left = c_end - c0;
        unsigned long long mask = left < LR_T ? ~0ull << left : 0ull;
        if ((unsigned)(d - c0) < (unsigned)LR_T) mask |= 1ull << (d - c0);
        if ((unsigned)(self - c0) < (unsigned)LR_T) mask |= 1ull << (self - c0);
        if (nxt < c0 + LR_T) {                                  // rare: the set has members in this tile
            do {
                mask |= 1ull << (nxt - c0);                     // nxt >= c0: the cursor never lags behind the tiles
                cur++;
                nxt = cur < x_end ? x_ids[cur] : 0x7fffffff;
            } while (nxt < c0 + LR_T);
        }
        const unsigned long long mine = mask >> (4 * kg);       // bit 16 g + r: column 16 g + 4 kg + r
        const float *Nc = Ns + buf * LR_T;
#pragma unroll
        for (int g = 0; g < 4; g++)
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const float sc = lr_score(acc[g][r], inv_q, cosine ? Nc[16 * g + 4 * kg + r] : 1.f, cosine);
                const int live = 1 - (int)((mine >> (16 * g + r)) & 1ull);
                n_above += sc > t ? live : 0;
                n_equal += sc == t ? live : 0;
            }
        if (more) lr_tile_store<DP>(L, T, Cs + (buf ^ 1) * LR_T * QLD, Ns + (buf ^ 1) * LR_T);
        __syncthreads();                                        // tile c0 is done with, the next is in place
    }
    n_above += __shfl_xor(n_above, 16, WAVE);
    n_above += __shfl_xor(n_above, 32, WAVE);
    n_equal += __shfl_xor(n_equal, 16, WAVE);
    n_equal += __shfl_xor(n_equal, 32, WAVE);
    if (kg == 0 && ok) {
        if (n_above) atomicAdd(&above[i], n_above);
        if (n_equal) atomicAdd(&equal[i], n_equal);
    }
}

// ---- entry points ------------------------------------------------------------------------------------------------------------

static int lr_refuse(const char *name, const char *why) {
    static thread_local char msg[200];
    snprintf(msg, sizeof msg, "%s: %s", name, why);
    return gcnhip_fail(msg);
}
static const char *lr_common(const gcnhip_ctx *c, const void *table, int ld, int n_table, int dim, const void *src, const void *dst, int nq) {
    if (!c || !table) return "invalid argument";
    if (n_table < 0 || nq < 0) return "a negative count";
    if (dim < 1 || dim > LR_MAX_DIM) return "1 <= dim <= 256";
    if (ld < dim) return "the row stride is below dim";
    if (n_table < 1) return "an empty table";
    if (nq > 0 && (!src || !dst)) return "invalid argument (src or dst is NULL)";
    return nullptr;
}
static LrTable lr_table(const float *table, int ld, int n_table, int dim, const float *inv_norm) {
    return LrTable{table, ld, n_table, dim, inv_norm, ld % 4 == 0 && aligned16(table) ? 1 : 0, (dim + 15) / 16};
}
static size_t lr_lds(int dp, int bufs) { return sizeof(float) * (size_t)bufs * LR_T * (dp + 4 + 1) + LR_T * sizeof(int); }

template <int DP>
static int lr_thr_launch(gcnhip_ctx *c, const LrTable &T, const int32_t *src, const int32_t *dst, int nq, float *thr, int32_t *above, int32_t *equal) {
    const size_t lds = lr_lds(DP, 1);
    auto kern = link_thr_kernel<DP>;
    if (lds > 64 * 1024) GCNHIP_TRY(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    kern<<<ceil_div(nq, LR_T), 256, lds, c->stream>>>(T, src, dst, nq, thr, above, equal);
    GCNHIP_LAUNCH_CHECK();
    return 0;
}
template <int DP>
static int lr_walk_launch(gcnhip_ctx *c, const LrTable &T, const int32_t *src, const int32_t *dst, int nq, const float *thr, const int32_t *x_ptr,
                          const int32_t *x_len, const int32_t *x_ids, int exclude_self, int rows, int chunks, int32_t *above, int32_t *equal) {
    const size_t lds = lr_lds(DP, 2);
    auto kern = link_walk_kernel<DP>;
    if (lds > 64 * 1024) GCNHIP_TRY(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    kern<<<dim3(ceil_div(nq, LR_T), chunks), 256, lds, c->stream>>>(T, src, dst, nq, thr, x_ptr, x_len, x_ids, exclude_self, rows, above, equal);
    GCNHIP_LAUNCH_CHECK();
    return 0;
}

extern "C" {

int gcnhip_link_rank_plan(int n_table, int nq, int chunk_rows, int *chunk_rows_used, int *n_chunks, size_t *scratch_bytes) {
    if (n_table < 1 || nq < 0 || chunk_rows < 0) return lr_refuse("gcnhip_link_rank_plan", "invalid argument (n_table >= 1, nq >= 0, chunk_rows >= 0)");
    if (gcnhip_topk_plan(n_table, nq, 1, chunk_rows, chunk_rows_used, n_chunks, nullptr, nullptr) != 0)    // the candidates are cut as similar()'s
        return lr_refuse("gcnhip_link_rank_plan", "more than 65535 chunks: raise chunk_rows");
    if (scratch_bytes) *scratch_bytes = std::max<size_t>((size_t)nq, 1) * sizeof(float);               // the thresholds
    return 0;
}

int gcnhip_link_thresholds(gcnhip_ctx *c, const float *table, int ld, int n_table, int dim, const float *inv_norm, const int32_t *src,
                           const int32_t *dst, int nq, float *thr) {
    if (const char *why = lr_common(c, table, ld, n_table, dim, src, dst, nq)) return lr_refuse("gcnhip_link_thresholds", why);
    if (nq > 0 && !thr) return lr_refuse("gcnhip_link_thresholds", "a NULL output");
    if (nq == 0) return 0;
    const LrTable T = lr_table(table, ld, n_table, dim, inv_norm);
    return dim <= 128 ? lr_thr_launch<128>(c, T, src, dst, nq, thr, nullptr, nullptr) : lr_thr_launch<256>(c, T, src, dst, nq, thr, nullptr, nullptr);
}

int gcnhip_link_ranks(gcnhip_ctx *c, const float *table, int ld, int n_table, int dim, const float *inv_norm, const int32_t *src,
                      const int32_t *dst, int nq, const int32_t *x_ptr, const int32_t *x_len, const int32_t *x_ids, int exclude_self,
                      int chunk_rows, void *scratch, size_t scratch_bytes, int launches, int32_t *above, int32_t *equal) {
    const char *name = "gcnhip_link_ranks";
    if (const char *why = lr_common(c, table, ld, n_table, dim, src, dst, nq)) return lr_refuse(name, why);
    if (nq > 0 && (!above || !equal)) return lr_refuse(name, "a NULL output");
    if (launches < 1 || launches > 3) return lr_refuse(name, "launches is 1 (thresholds), 2 (the walk) or 3 (the answer)");
    if (x_ptr && !x_ids) return lr_refuse(name, "a filter needs x_ids beside x_ptr");
    int rows = 0, chunks = 0;
    size_t need = 0;
    if (chunk_rows < 0) return lr_refuse(name, "a negative count");
    if (gcnhip_link_rank_plan(n_table, nq, chunk_rows, &rows, &chunks, &need) != 0) return -1;
    if (!scratch || scratch_bytes < need) return lr_refuse(name, "the scratch is below what gcnhip_link_rank_plan tells");
    if (nq == 0) return 0;
    const LrTable T = lr_table(table, ld, n_table, dim, inv_norm);
    float *thr = (float *)scratch;
    if (launches & 1) {
        const int rc = dim <= 128 ? lr_thr_launch<128>(c, T, src, dst, nq, thr, above, equal) : lr_thr_launch<256>(c, T, src, dst, nq, thr, above, equal);
        if (rc != 0) return rc;
    }
    if (launches & 2) {
        const int rc = dim <= 128 ? lr_walk_launch<128>(c, T, src, dst, nq, thr, x_ptr, x_len, x_ids, exclude_self, rows, chunks, above, equal)
                                  : lr_walk_launch<256>(c, T, src, dst, nq, thr, x_ptr, x_len, x_ids, exclude_self, rows, chunks, above, equal);
        if (rc != 0) return rc;
    }
    return 0;
}

}  // extern "C"
