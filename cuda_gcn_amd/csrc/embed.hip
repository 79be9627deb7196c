// embed.hip — node embeddings taken out of a trained model: inverse row norms, the k best rows per query by dot product or
// cosine, scores of listed row pairs, and the export gather.  Beyond the reference, which never looks at its hidden matrix.
//
// All kernels read an f32 table [n_table x ld] with 1 <= dim <= 256 and dim <= ld, rows of any stride; columns [dim, ld) are
// never read as values (the tail of a row is loaded element by element behind a column test).
//
// Score of (q, c): the f32 dot product; with inverse norms, (dot . inv_norm[q]) . inv_norm[c].  Candidates are ordered by
// score descending and, on equal scores, by id ascending (id = row_id[c], or c): a TOTAL order, so the k best of a table do
// not depend on how its rows are cut into chunks.  The empty slot is (-inf, INT_MAX), worse than every candidate.
//
// gcnhip_topk_rows is two launches per batch of queries:
//   topk_part_kernel   grid (query tiles of 64, chunks of chunk_rows candidates), 256 threads.  The 64 query rows sit in LDS
//                      (zero-padded to a multiple of 16 columns); the chunk is streamed once in tiles of 64 candidates.  Wave w
//                      multiplies candidates 16w .. 16w + 15 of the tile with all 64 queries on v_mfma_f32_16x16x4_f32 (four
//                      independent accumulators; the exact f32 fma chain in k order, so equal rows give equal bits whichever
//                      lane, wave or chunk holds them) and leaves the 64 x 64 dots in a double-buffered LDS tile: one barrier per
//                      tile.  Wave w then owns queries 16w .. 16w + 15: lane j tests candidate j against the query's current k-th
//                      entry (one broadcast LDS read); only when some lane passes is the query's sorted list (LDS, one entry per
//                      lane) loaded and the passing candidates inserted one by one (ballot, popcount, a one-lane shift).  After
//                      warm-up almost no tile inserts anything.  The chunk's list goes to the caller's scratch.
//   topk_merge_kernel  a wave per query merges its n_chunks sorted lists with the same insertion and writes ids and scores.
// No atomics and no dependence on block order: two launches give the same bits.  Neither allocates nor synchronises.
#include "common.h"
#include <algorithm>
#include <climits>
#include <cstdio>

using f32x4 = __attribute__((ext_vector_type(4))) float;

constexpr int TOPK_QT = 64;                       // queries per workgroup
constexpr int TOPK_CT = 64;                       // candidates per tile
constexpr int TOPK_SLD = TOPK_CT + 1;             // row stride of the score tile
constexpr int TOPK_MAX_K = 64;                    // a list is one entry per lane
constexpr int EMBED_MAX_DIM = 256;
constexpr int TOPK_TARGET_WGS = 1024;             // the automatic split aims at four workgroups per CU ...
constexpr int TOPK_CHUNK_MIN = 1024, TOPK_CHUNK_MAX = 16384;   // ... with chunks inside these row counts
constexpr int TOPK_MAX_CHUNKS = 65535;            // gridDim.y

__device__ inline bool better(float s, int id, float ts, int tid) { return s > ts || (s == ts && id < tid); }

// Insert the passing candidates (bit j of mask: lane j's (s, id)) into the sorted list whose entry p sits in lane p; lanes
// >= k hold the empty slot and never shift anything in that matters: entry k - 1 is the threshold.
__device__ inline void wave_insert(float &ls, int &li, float s, int id, unsigned long long mask, int k, int lane) {
    while (mask) {
        const int j = __ffsll(mask) - 1;
        mask &= mask - 1;
        const float xs = __shfl(s, j, WAVE);
        const int xi = __shfl(id, j, WAVE);
        if (!better(xs, xi, __shfl(ls, k - 1, WAVE), __shfl(li, k - 1, WAVE))) continue;
        const int pos = __popcll(__ballot(better(ls, li, xs, xi)));      // the entries ahead of x: a prefix of the lanes
        const float us = __shfl_up(ls, 1, WAVE);
        const int ui = __shfl_up(li, 1, WAVE);
        if (lane == pos) { ls = xs; li = xi; }
        else if (lane > pos) { ls = us; li = ui; }
    }
}

__global__ __launch_bounds__(256) void topk_part_kernel(const float *__restrict__ table, int ld, int n_table, int dim,
                                                        const float *__restrict__ inv_norm, const int32_t *__restrict__ row_id,
                                                        const int32_t *__restrict__ q_rows, int nqb, int k, int exclude_self,
                                                        int chunk_rows, int n_chunks, int vec_ok, float *__restrict__ part_s,
                                                        int32_t *__restrict__ part_i) {
    extern __shared__ __align__(16) unsigned char smem[];
    const int dpad = (dim + 15) / 16 * 16, qld = dpad + 4;
    float *Qs = (float *)smem;                                  // [64][qld]
    float *S = Qs + TOPK_QT * qld;                              // [2][64][65]
    float *inv_q = S + 2 * TOPK_QT * TOPK_SLD;                  // [64]
    int *qrow = (int *)(inv_q + TOPK_QT);                       // [64]: the query's table row, -1: none
    float *list_s = (float *)(qrow + TOPK_QT);                  // [64][k]
    int *list_i = (int *)(list_s + TOPK_QT * k);                // [64][k]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int qt = blockIdx.x, chunk = blockIdx.y;

    if (threadIdx.x < TOPK_QT) {
        const int b = qt * TOPK_QT + threadIdx.x;
        int r = b < nqb ? q_rows[b] : -1;
        if (r < 0 || r >= n_table) r = -1;
        qrow[threadIdx.x] = r;
        inv_q[threadIdx.x] = r >= 0 && inv_norm ? inv_norm[r] : 1.f;
    }
    for (int i = threadIdx.x; i < TOPK_QT * k; i += 256) { list_s[i] = -INFINITY; list_i[i] = INT_MAX; }
    for (int r = wave; r < TOPK_QT; r += 4) {                   // a wave per query row, lanes along it
        const int b = qt * TOPK_QT + r;
        int row = b < nqb ? q_rows[b] : -1;
        if (row < 0 || row >= n_table) row = -1;
        for (int col = lane; col < dpad; col += WAVE)
            Qs[r * qld + col] = row >= 0 && col < dim ? table[(size_t)row * ld + col] : 0.f;
    }
    __syncthreads();

    const int c_begin = chunk * chunk_rows;
    const int c_end = min(n_table, c_begin + chunk_rows);
    const int kg = lane >> 4, l15 = lane & 15;
    int buf = 0;
    for (int c0 = c_begin; c0 < c_end; c0 += TOPK_CT, buf ^= 1) {
        // ---- the 64 x 16 dots of this wave: A = queries (row l15 of sub-tile t), B = candidate 16w + l15; both take column
        // 16j + 4kg + s for k-slot kg of step s, so a lane loads four consecutive columns of each at once
        const int cr = min(c0 + 16 * wave + l15, n_table - 1);   // past the chunk: a row that exists, dropped by the selection
        const float *crow = table + (size_t)cr * ld;
        f32x4 acc[4] = {};
        for (int j0 = 0; j0 < dpad; j0 += 16) {
            const int col = j0 + 4 * kg;
            f32x4 b;
            if (vec_ok && col + 3 < dim) {
                b = *(const f32x4 *)(crow + col);
            } else {
                b.x = col < dim ? crow[col] : 0.f;
                b.y = col + 1 < dim ? crow[col + 1] : 0.f;
                b.z = col + 2 < dim ? crow[col + 2] : 0.f;
                b.w = col + 3 < dim ? crow[col + 3] : 0.f;
            }
            f32x4 a[4];
#pragma unroll
            for (int t = 0; t < 4; t++) a[t] = *(const f32x4 *)(Qs + (16 * t + l15) * qld + col);
#pragma unroll
            for (int s = 0; s < 4; s++)                         // the four accumulators in turn: no MFMA waits for the one before it
#pragma unroll
                for (int t = 0; t < 4; t++) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[t][s], b[s], acc[t], 0, 0, 0);
        }
        float *Sb = S + buf * TOPK_QT * TOPK_SLD;
#pragma unroll
        for (int t = 0; t < 4; t++)
#pragma unroll
            for (int r = 0; r < 4; r++) Sb[(16 * t + 4 * kg + r) * TOPK_SLD + 16 * wave + l15] = acc[t][r];   // D[row 4kg + r][col l15]
        // every wave has finished selecting from the other buffer before any wave gets here a second time
        __syncthreads();

        // ---- selection: this wave's 16 queries against the tile's 64 candidates, lane j on candidate j
        const int c = c0 + lane;
        const bool cvalid = c < c_end;
        const int cid = cvalid ? (row_id ? row_id[c] : c) : INT_MAX;
        const float cinv = cvalid && inv_norm ? inv_norm[c] : 1.f;
        for (int qi = 0; qi < 16; qi++) {
            const int q = 16 * wave + qi;
            const int qr = qrow[q];
            if (qr < 0) continue;
            float s = Sb[q * TOPK_SLD + lane];
            if (inv_norm) s = (s * inv_q[q]) * cinv;
            const bool pass = cvalid && !(exclude_self && c == qr) && better(s, cid, list_s[q * k + k - 1], list_i[q * k + k - 1]);
            const unsigned long long mask = __ballot(pass);
            if (!mask) continue;
            float ls = lane < k ? list_s[q * k + lane] : -INFINITY;
            int li = lane < k ? list_i[q * k + lane] : INT_MAX;
            wave_insert(ls, li, s, cid, mask, k, lane);
            if (lane < k) { list_s[q * k + lane] = ls; list_i[q * k + lane] = li; }
        }
    }
    // the lists of a wave's queries are its own: nothing to wait for
    for (int qi = 0; qi < 16; qi++) {
        const int q = 16 * wave + qi, b = qt * TOPK_QT + q;
        if (b >= nqb || lane >= k) continue;
        const size_t o = ((size_t)b * n_chunks + chunk) * k + lane;
        part_s[o] = list_s[q * k + lane];
        part_i[o] = list_i[q * k + lane];
    }
}

__global__ __launch_bounds__(256) void topk_merge_kernel(const float *__restrict__ part_s, const int32_t *__restrict__ part_i, int nqb,
                                                         int n_chunks, int k, int32_t *__restrict__ out_id, float *__restrict__ out_score) {
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= nqb) return;
    const int total = n_chunks * k;
    const size_t base = (size_t)b * total;
    float ls = -INFINITY;
    int li = INT_MAX;
    for (int e0 = 0; e0 < total; e0 += WAVE) {
        const int e = e0 + lane;
        const float s = e < total ? part_s[base + e] : -INFINITY;
        const int id = e < total ? part_i[base + e] : INT_MAX;
        const float ts = __shfl(ls, k - 1, WAVE);                 // read by every lane: a shuffle from a lane that a branch has
        const int ti = __shfl(li, k - 1, WAVE);                   // switched off returns 0, not that lane's entry
        const bool pass = e < total && better(s, id, ts, ti);
        wave_insert(ls, li, s, id, __ballot(pass), k, lane);
    }
    if (lane < k) {
        out_score[(size_t)b * k + lane] = ls;
        out_id[(size_t)b * k + lane] = li == INT_MAX ? -1 : li;
    }
}

// a wave per row: lanes along the row, one butterfly
__global__ __launch_bounds__(256) void embed_inv_norms_kernel(const float *__restrict__ table, int ld, int n_table, int dim, float *__restrict__ inv_norm) {
    const int lane = threadIdx.x & 63;
    for (int r = blockIdx.x * 4 + (threadIdx.x >> 6); r < n_table; r += gridDim.x * 4) {
        float s = 0.f;
        for (int col = lane; col < dim; col += WAVE) {
            const float x = table[(size_t)r * ld + col];
            s += x * x;
        }
        s = wave_sum(s);
        if (lane == 0) inv_norm[r] = s > 0.f ? 1.f / sqrtf(s) : 0.f;
    }
}

// 16 lanes per pair
__global__ __launch_bounds__(256) void pair_scores_kernel(const float *__restrict__ table, int ld, int n_table, int dim,
                                                          const float *__restrict__ inv_norm, const int32_t *__restrict__ src,
                                                          const int32_t *__restrict__ dst, int n_pairs, float *__restrict__ out) {
    const int l15 = threadIdx.x & 15;
    const int p = blockIdx.x * 16 + (threadIdx.x >> 4);
    const bool live = p < n_pairs;
    const int a = live ? src[p] : 0, b = live ? dst[p] : 0;
    const bool ok = live && a >= 0 && a < n_table && b >= 0 && b < n_table;   // an id outside the table: NaN, never a read past it
    float s = 0.f;
    if (ok)
        for (int col = l15; col < dim; col += 16) s += table[(size_t)a * ld + col] * table[(size_t)b * ld + col];
#pragma unroll
    for (int off = 8; off > 0; off >>= 1) s += __shfl_xor(s, off, WAVE);
    if (live && l15 == 0) out[p] = !ok ? NAN : (inv_norm ? (s * inv_norm[a]) * inv_norm[b] : s);
}

// out[i, :dim] = table[rows[i], :dim] (. inv_norm[rows[i]]); rows == NULL: row i
__global__ __launch_bounds__(256) void embed_rows_kernel(const float *__restrict__ table, int ld, int n_table, int dim,
                                                         const float *__restrict__ inv_norm, const int32_t *__restrict__ rows, int n,
                                                         float *__restrict__ out, int ld_out) {
    const int lane = threadIdx.x & 63;
    for (int i = blockIdx.x * 4 + (threadIdx.x >> 6); i < n; i += gridDim.x * 4) {
        const int r = rows ? rows[i] : i;
        const bool ok = r >= 0 && r < n_table;
        const float f = ok && inv_norm ? inv_norm[r] : 1.f;
        for (int col = lane; col < dim; col += WAVE) out[(size_t)i * ld_out + col] = ok ? table[(size_t)r * ld + col] * f : NAN;
    }
}

static const char *embed_refusal(const void *table, int ld, int n_table, int dim) {
    if (!table || n_table < 0) return "invalid argument";
    if (dim < 1 || dim > EMBED_MAX_DIM) return "1 <= dim <= 256";
    if (ld < dim) return "the row stride is below dim";
    return nullptr;
}
#define EMBED_REFUSE(NAME, WHY)                                                   \
    do {                                                                          \
        char msg[160];                                                            \
        snprintf(msg, sizeof msg, "%s: %s", NAME, WHY);                           \
        return gcnhip_fail(msg);                                                  \
    } while (0)

static int row_wave_blocks(int n) { return std::min(std::max(ceil_div(n, 4), 1), 4096); }

static int topk_auto_chunk(int n_table, int nq) {
    const int want = ceil_div(TOPK_TARGET_WGS, std::max(ceil_div(nq, TOPK_QT), 1));
    const int rows = ceil_div(ceil_div(n_table, want), TOPK_CT) * TOPK_CT;
    return std::min(std::max(rows, TOPK_CHUNK_MIN), TOPK_CHUNK_MAX);
}

extern "C" {

int gcnhip_embed_inv_norms(gcnhip_ctx *c, const float *table, int ld, int n_table, int dim, float *inv_norm) {
    if (!c || !inv_norm) return gcnhip_fail("gcnhip_embed_inv_norms: invalid argument");
    if (const char *why = embed_refusal(table, ld, n_table, dim)) EMBED_REFUSE("gcnhip_embed_inv_norms", why);
    if (n_table == 0) return 0;
    embed_inv_norms_kernel<<<row_wave_blocks(n_table), 256, 0, c->stream>>>(table, ld, n_table, dim, inv_norm);
    GCNHIP_LAUNCH_CHECK();
    return 0;
}

int gcnhip_topk_plan(int n_table, int nq, int k, int chunk_rows, int *chunk_rows_used, int *n_chunks, size_t *scratch_bytes, size_t *scratch_bytes_min) {
    if (n_table < 1 || nq < 0 || chunk_rows < 0) return gcnhip_fail("gcnhip_topk_plan: invalid argument");
    if (k < 1 || k > TOPK_MAX_K) return gcnhip_fail("gcnhip_topk_plan: 1 <= k <= 64 (a list is one entry per lane)");
    const int rows = chunk_rows > 0 ? chunk_rows : topk_auto_chunk(n_table, nq);
    const int chunks = ceil_div(n_table, rows);
    if (chunks > TOPK_MAX_CHUNKS) return gcnhip_fail("gcnhip_topk_plan: more than 65535 chunks: raise chunk_rows");
    const size_t per_query = (size_t)chunks * k * (sizeof(float) + sizeof(int32_t));
    if (chunk_rows_used) *chunk_rows_used = rows;
    if (n_chunks) *n_chunks = chunks;
    if (scratch_bytes) *scratch_bytes = per_query * (size_t)std::max(ceil_div(nq, TOPK_QT), 1) * TOPK_QT;
    if (scratch_bytes_min) *scratch_bytes_min = per_query * TOPK_QT;
    return 0;
}

int gcnhip_topk_rows(gcnhip_ctx *c, const float *table, int ld, int n_table, int dim, const float *inv_norm, const int32_t *row_id,
                     const int32_t *q_rows, int nq, int k, int exclude_self, int chunk_rows, void *scratch, size_t scratch_bytes,
                     int launches, int32_t *out_id, float *out_score) {
    if (!c || nq < 0 || (nq > 0 && (!q_rows || !out_id || !out_score)) || !scratch || launches < 1 || launches > 3)
        return gcnhip_fail("gcnhip_topk_rows: invalid argument");
    if (const char *why = embed_refusal(table, ld, n_table, dim)) EMBED_REFUSE("gcnhip_topk_rows", why);
    if (n_table < 1) return gcnhip_fail("gcnhip_topk_rows: an empty table");
    int rows = 0, chunks = 0;
    size_t need_min = 0;
    if (gcnhip_topk_plan(n_table, nq, k, chunk_rows, &rows, &chunks, nullptr, &need_min) != 0) return -1;
    if (scratch_bytes < need_min) return gcnhip_fail("gcnhip_topk_rows: the scratch holds no tile of 64 queries (gcnhip_topk_plan tells the bytes)");
    if (nq == 0) return 0;
    const int dpad = (dim + 15) / 16 * 16;
    const size_t lds = sizeof(float) * ((size_t)TOPK_QT * (dpad + 4) + 2 * TOPK_QT * TOPK_SLD + 2 * TOPK_QT + 2 * (size_t)TOPK_QT * k);
    if (lds > 64 * 1024) GCNHIP_TRY(hipFuncSetAttribute((const void *)topk_part_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    const int vec_ok = ld % 4 == 0 && aligned16(table);
    // as many whole query tiles per batch as the scratch holds
    const size_t batch_cap = scratch_bytes / need_min * TOPK_QT;
    const int batch = (int)std::min<size_t>(batch_cap, (size_t)ceil_div(nq, TOPK_QT) * TOPK_QT);
    float *part_s = (float *)scratch;
    int32_t *part_i = (int32_t *)(part_s + (size_t)batch * chunks * k);
    for (int q0 = 0; q0 < nq; q0 += batch) {
        const int nqb = std::min(batch, nq - q0);
        if (launches & 1) {
            topk_part_kernel<<<dim3(ceil_div(nqb, TOPK_QT), chunks), 256, lds, c->stream>>>(table, ld, n_table, dim, inv_norm, row_id, q_rows + q0, nqb, k,
                                                                                          exclude_self, rows, chunks, vec_ok, part_s, part_i);
            GCNHIP_LAUNCH_CHECK();
        }
        if (launches & 2) {
            topk_merge_kernel<<<ceil_div(nqb, 4), 256, 0, c->stream>>>(part_s, part_i, nqb, chunks, k, out_id + (size_t)q0 * k, out_score + (size_t)q0 * k);
            GCNHIP_LAUNCH_CHECK();
        }
    }
    return 0;
}

int gcnhip_pair_scores(gcnhip_ctx *c, const float *table, int ld, int n_table, int dim, const float *inv_norm, const int32_t *src,
                       const int32_t *dst, int n_pairs, float *out) {
    if (!c || n_pairs < 0 || (n_pairs > 0 && (!src || !dst || !out))) return gcnhip_fail("gcnhip_pair_scores: invalid argument");
    if (const char *why = embed_refusal(table, ld, n_table, dim)) EMBED_REFUSE("gcnhip_pair_scores", why);
    if (n_pairs == 0) return 0;
    pair_scores_kernel<<<ceil_div(n_pairs, 16), 256, 0, c->stream>>>(table, ld, n_table, dim, inv_norm, src, dst, n_pairs, out);
    GCNHIP_LAUNCH_CHECK();
    return 0;
}

int gcnhip_embed_rows(gcnhip_ctx *c, const float *table, int ld, int n_table, int dim, const float *inv_norm, const int32_t *d_rows, int n,
                      float *out, int ld_out) {
    if (!c || n < 0 || (n > 0 && !out) || ld_out < dim) return gcnhip_fail("gcnhip_embed_rows: invalid argument");
    if (const char *why = embed_refusal(table, ld, n_table, dim)) EMBED_REFUSE("gcnhip_embed_rows", why);
    if (!d_rows && n > n_table) return gcnhip_fail("gcnhip_embed_rows: without a row list n is at most n_table");
    if (n == 0) return 0;
    embed_rows_kernel<<<row_wave_blocks(n), 256, 0, c->stream>>>(table, ld, n_table, dim, inv_norm, d_rows, n, out, ld_out);
    GCNHIP_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
