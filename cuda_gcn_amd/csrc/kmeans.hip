// kmeans.hip — grouping the rows of a trained model's hidden layer: Lloyd's k-means (assign, update), k-means++ seeding by an
// exponential race, and the cluster x class table of an assignment.  Beyond the reference, which never looks at its hidden matrix.
//
// The table contract is embed.hip's: f32 [n_table x ld], 1 <= dim <= 256, dim <= ld, rows of any stride and alignment; columns
// [dim, ld) are never read as values.  d_rows is a device int32 list of n rows (repeats allowed; NULL: rows 0 .. n - 1); the
// row used is x^ = x . inv_norm[r] (inv_norm == NULL: x itself).  1 <= k <= 256.  No float atomics, no allocation, no
// synchronisation; every output's bits are a function of the arguments' contents alone.
//
// gcnhip_kmeans_assign   d(i, c) = cn[c] - 2 . (dot_f32(T[r], M[c]) . inv_norm[r]); assign[i] = argmin_c d, the lowest c on equal
//   d; dist2[i] = max(0, (sumsq_f32(T[r]) . inv . inv) + d(i, assign[i])).  One launch: a workgroup takes tiles of 64 list
//   positions (grid-stride), stages their rows in LDS once, and walks the centres in tiles of 64 that sit in LDS beside them.
//   Wave w owns positions 16w .. 16w + 15 of the tile: v_mfma_f32_16x16x4_f32 with A = 16 centres, B = its 16 rows, four
//   independent accumulators (the exact f32 fma chain in column order), so that lane (l15, kg) holds the dots of row l15 with
//   centres 16t + 4kg + r.  The running (min, argmin) of a row stays in registers across centre tiles and is folded over the four
//   lane groups at the end.  A centre slot past k has cn = +inf in LDS and is skipped by index as well: it can never win.
//   With one centre tile (k <= 64) the centres are loaded once per workgroup.  *moved is an integer atomic.
// gcnhip_kmeans_update   The order of every float64 sum is fixed by the data: (1) per chunk of KM_CHUNK positions an integer
//   histogram over the centres and the chunk's sum of dist2 (a fixed tree); (2) one scan turns the histograms into offsets,
//   writes sizes and the segment table; (3) a wave per chunk scatters its positions, in order, into the member list: a stable
//   bucketing, so the members of a centre are in ascending position; (4) a wave per (segment of KM_SEG members, slab of 64
//   columns) adds (double)(x . inv) member by member; (5) the segment partials of a centre are added in order into its float64
//   row; (6) M = (float)(sum / count), cn = (float)(the float64 sum of M^2 in column order), inertia.  Steps 4 and 5 run in
//   batches of as many segments as the caller's scratch holds: fewer bytes, more launches, the same sequence of additions.
// gcnhip_kmeans_seed     k-means++ (Arthur & Vassilvitskii, 2007) without a prefix sum: drawing i with probability d2min[i] / sum
//   is taking the smallest of the exponential variates -log(u_i) / d2min[i] — a commutative min over (key, position).
// gcnhip_contingency_rows  integer counts by LDS histogram and integer atomics.
#include "bucket.h"
#include <algorithm>
#include <climits>
#include <cstdio>

using f32x4 = __attribute__((ext_vector_type(4))) float;

constexpr int KM_MAX_DIM = 256, KM_MAX_C = 64;     // KM_MAX_K, KM_CHUNK and the bucketing kernels: bucket.h
constexpr int KM_RT = 64;                         // list positions per tile of the assign kernel
constexpr int KM_CT = 64;                         // centres per LDS tile
constexpr int KM_SEG = 128;                       // members per segment (part of the definition)
constexpr int KM_MIN_SEGS = 64;                   // the smallest batch of segment partials
constexpr int KM_SEED_PARTS = 1024;               // workgroups of a seeding step at most
constexpr int KM_SEED_ROWS = 8;                   // list positions a wave of a seeding step has in flight (a power of two)

// ---- assign ---------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(256) void kmeans_assign_kernel(const float *__restrict__ table, int ld, int n_table, int dim,
                                                            const float *__restrict__ inv_norm, const int32_t *__restrict__ d_rows, int n,
                                                            const float *__restrict__ M, int ldm, const float *__restrict__ cn, int k,
                                                            const int32_t *__restrict__ prev, int32_t *__restrict__ assign,
                                                            float *__restrict__ dist2, int32_t *__restrict__ moved) {
    extern __shared__ __align__(16) unsigned char smem[];
    const int dpad = (dim + 15) / 16 * 16, qld = dpad + 4;
    float *Xs = (float *)smem;                                  // [64][qld] the tile's rows, zero-padded
    float *Ms = Xs + KM_RT * qld;                               // [64][qld] a tile of centres, zero-padded
    float *cns = Ms + KM_CT * qld;                              // [64] their squared norms, +inf past k
    float *rinv = cns + KM_CT;                                  // [64] inverse norm of the row (1 without)
    float *rxn = rinv + KM_RT;                                  // [64] squared norm of the scaled row
    int *rrow = (int *)(rxn + KM_RT);                           // [64] table row, -1: none
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int kg = lane >> 4, l15 = lane & 15;
    const int n_tiles = (n + KM_RT - 1) / KM_RT, n_ct = (k + KM_CT - 1) / KM_CT;
    bool have_m = false;
    int n_moved = 0;

    for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        __syncthreads();                                        // every wave is done with the previous tile's rows and centres
        {                                                       // a wave stages its own 16 rows, lanes along a row
            const int i_mine = tile * KM_RT + 16 * wave + l15;  // lane l15 (of every group) names row l15 of the wave
            const int r_mine = i_mine < n ? list_row(d_rows, i_mine, n_table) : -1;
            const float f_mine = r_mine >= 0 && inv_norm ? inv_norm[r_mine] : 1.f;
            float v[16][4];                                     // every load of the 16 rows is issued before the first sum
#pragma unroll
            for (int rr = 0; rr < 16; rr++) {
                const int r = __shfl(r_mine, rr, WAVE);
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    const int col = lane + WAVE * u;
                    v[rr][u] = r >= 0 && col < dim ? table[(size_t)r * ld + col] : 0.f;
                }
            }
#pragma unroll
            for (int rr = 0; rr < 16; rr++) {
                const int q = 16 * wave + rr;
                float s = 0.f;
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    const int col = lane + WAVE * u;
                    if (col < dpad) Xs[q * qld + col] = v[rr][u];
                    s += v[rr][u] * v[rr][u];                   // columns lane, lane + 64, ..: the order of the one-row loop
                }
                s = wave_sum(s);
                if (lane == rr) {
                    rrow[q] = r_mine;
                    rinv[q] = f_mine;
                    rxn[q] = (s * f_mine) * f_mine;
                }
            }
        }
        float bd = INFINITY;
        int bc = 0;
        for (int ct = 0; ct < n_ct; ct++) {
            if (n_ct > 1 || !have_m) {
                if (ct > 0) __syncthreads();                    // the products with the tile before this one are done
                for (int cc = wave; cc < KM_CT; cc += 4) {
                    const int c = ct * KM_CT + cc;
                    for (int col = lane; col < dpad; col += WAVE) Ms[cc * qld + col] = c < k && col < dim ? M[(size_t)c * ldm + col] : 0.f;
                    if (lane == 0) cns[cc] = c < k ? cn[c] : INFINITY;
                }
                have_m = true;
            }
            __syncthreads();
            f32x4 acc[4] = {};
            const float *xrow = Xs + (16 * wave + l15) * qld;
            for (int j0 = 0; j0 < dpad; j0 += 16) {
                const int col = j0 + 4 * kg;
                const f32x4 b = *(const f32x4 *)(xrow + col);
                f32x4 a[4];
#pragma unroll
                for (int t = 0; t < 4; t++) a[t] = *(const f32x4 *)(Ms + (16 * t + l15) * qld + col);
#pragma unroll
                for (int s = 0; s < 4; s++)
#pragma unroll
                    for (int t = 0; t < 4; t++) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[t][s], b[s], acc[t], 0, 0, 0);
            }
            const float f = rinv[16 * wave + l15];
#pragma unroll
            for (int t = 0; t < 4; t++)
#pragma unroll
                for (int r = 0; r < 4; r++) {                   // D[row 4kg + r][col l15]: centre 16t + 4kg + r, this lane's row
                    const int cc = 16 * t + 4 * kg + r, c = ct * KM_CT + cc;
                    const float d = cns[cc] - 2.f * (acc[t][r] * f);
                    if (c < k && (d < bd || (d == bd && c < bc))) { bd = d; bc = c; }
                }
        }
#pragma unroll
        for (int off = 16; off < 64; off <<= 1) {               // the four lane groups of a row
            const float od = __shfl_xor(bd, off, WAVE);
            const int oc = __shfl_xor(bc, off, WAVE);
            if (od < bd || (od == bd && oc < bc)) { bd = od; bc = oc; }
        }
        const int q = 16 * wave + l15, i = tile * KM_RT + q;
        bool mv = false;
        if (lane < 16 && i < n) {
            const bool ok = rrow[q] >= 0;
            const int a = ok ? bc : -1;
            assign[i] = a;
            dist2[i] = ok ? fmaxf(0.f, rxn[q] + bd) : NAN;
            mv = prev ? prev[i] != a : true;
        }
        n_moved += __popcll(__ballot(mv));
    }
    if (lane == 0 && n_moved) atomicAdd(moved, n_moved);
}

// ---- update ---------------------------------------------------------------------------------------------------------------

// a wave per (segment, slab of 64 columns): the segment's members in order, one float64 chain per column
__global__ __launch_bounds__(256) void kmeans_segsum_kernel(const float *__restrict__ table, int ld, int n_table, int dim,
                                                            const float *__restrict__ inv_norm, const int32_t *__restrict__ d_rows,
                                                            const int32_t *__restrict__ order, const int32_t *__restrict__ cstart,
                                                            const int32_t *__restrict__ segstart, int k, int seg0, int seg1,
                                                            double *__restrict__ partials) {
    const int lane = threadIdx.x & 63;
    const int slabs = (dim + WAVE - 1) / WAVE;
    const int g = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int seg = seg0 + g / slabs, slab = g % slabs;
    if (seg >= seg1 || seg >= segstart[k]) return;              // the same for every lane of the wave
    const int c = segment_key(segstart, k, seg);
    const int first = cstart[c] + (seg - segstart[c]) * KM_SEG;
    const int count = min(KM_SEG, cstart[c + 1] - first);
    const int col = slab * WAVE + lane;
    double sum = 0.0;
    for (int m0 = 0; m0 < count; m0 += WAVE) {
        const int mine = m0 + lane < count ? order[first + m0 + lane] : 0;
        const int r_mine = m0 + lane < count ? list_row(d_rows, mine, n_table) : -1;
        const float f_mine = r_mine >= 0 && inv_norm ? inv_norm[r_mine] : 1.f;
        const int left = min(WAVE, count - m0);
#pragma unroll 8
        for (int m = 0; m < left; m++) {                       // the loads run ahead of the one chain of additions
            const int r = __shfl(r_mine, m, WAVE);
            const float f = __shfl(f_mine, m, WAVE);
            if (r >= 0 && col < dim) sum += (double)(table[(size_t)r * ld + col] * f);
        }
    }
    if (col < dim) partials[(size_t)(seg - seg0) * dim + col] = sum;
}

// block c, thread j: the partials of centre c that lie in this batch, in order
__global__ __launch_bounds__(256) void kmeans_fold_kernel(const double *__restrict__ partials, const int32_t *__restrict__ segstart, int dim,
                                                          int seg0, int seg1, double *__restrict__ acc) {
    const int c = blockIdx.x, j = threadIdx.x;
    if (j >= dim) return;
    const int lo = max(segstart[c], seg0), hi = min(segstart[c + 1], seg1);
    if (lo >= hi) return;
    double a = acc[(size_t)c * dim + j];
    for (int s = lo; s < hi; s++) a += partials[(size_t)(s - seg0) * dim + j];
    acc[(size_t)c * dim + j] = a;
}

// block c: the centre's new row (an empty centre keeps its own) and its squared norm; block 0 also the inertia
__global__ __launch_bounds__(256) void kmeans_finish_kernel(const double *__restrict__ acc, const int32_t *__restrict__ sizes, int dim,
                                                            float *__restrict__ M, int ldm, float *__restrict__ cn,
                                                            const double *__restrict__ dpart, int n_chunks, double *__restrict__ inertia) {
    __shared__ double red[256];
    __shared__ float row[KM_MAX_DIM];
    const int c = blockIdx.x, t = threadIdx.x;
    const int size = sizes[c];
    if (t < dim) {
        float v = M[(size_t)c * ldm + t];
        if (size > 0) {
            v = (float)(acc[(size_t)c * dim + t] / (double)size);
            M[(size_t)c * ldm + t] = v;
        }
        row[t] = v;
    }
    __syncthreads();
    if (t == 0) {
        double s = 0.0;
        for (int j = 0; j < dim; j++) s += (double)row[j] * (double)row[j];
        cn[c] = (float)s;
    }
    if (c == 0 && inertia) {
        double s = 0.0;
        for (int ch = t; ch < n_chunks; ch += 256) s += dpart[ch];
        red[t] = s;
        __syncthreads();
        for (int w = 128; w > 0; w >>= 1) {
            if (t < w) red[t] += red[t + w];
            __syncthreads();
        }
        if (t == 0) *inertia = red[0];
    }
}

// ---- seeding --------------------------------------------------------------------------------------------------------------

constexpr uint32_t KM_PHILOX_TAG = 0x6B6D2B2Bu;

__device__ inline uint32_t seed_word(uint32_t i, uint32_t t, uint64_t s) {
    uint32_t w[4];
    philox4x32_10(i, 0u, t, KM_PHILOX_TAG, (uint32_t)s, (uint32_t)(s >> 32), w);
    return w[0];
}

__device__ inline bool key_before(double ka, int pa, double kb, int pb) { return ka < kb || (ka == kb && pa < pb); }

// d2min = +inf everywhere; block 0: the first centre
__global__ __launch_bounds__(256) void kmeans_seed_init_kernel(const float *__restrict__ table, int ld, int n_table, int dim,
                                                               const float *__restrict__ inv_norm, const int32_t *__restrict__ d_rows, int n,
                                                               uint64_t s, float *__restrict__ M, int ldm, int32_t *__restrict__ seed_pos,
                                                               float *__restrict__ d2min) {
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) d2min[i] = INFINITY;
    if (blockIdx.x == 0) {
        const int p = (int)(((uint64_t)seed_word(0u, 0u, s) * (uint64_t)n) >> 32);
        const int r = list_row(d_rows, p, n_table);
        const float f = r >= 0 && inv_norm ? inv_norm[r] : 1.f;
        if (threadIdx.x == 0) seed_pos[0] = p;
        for (int j = threadIdx.x; j < dim; j += 256) M[j] = r >= 0 ? table[(size_t)r * ld + j] * f : 0.f;
    }
}

// step t: distances to centre t - 1, the race's keys, the workgroup's smallest (key, position)
__global__ __launch_bounds__(256) void kmeans_seed_step_kernel(const float *__restrict__ table, int ld, int n_table, int dim,
                                                               const float *__restrict__ inv_norm, const int32_t *__restrict__ d_rows, int n,
                                                               uint64_t s, int t, const float *__restrict__ M, int ldm,
                                                               float *__restrict__ d2min, double *__restrict__ part_key,
                                                               int32_t *__restrict__ part_pos) {
    __shared__ float centre[KM_MAX_DIM];
    __shared__ double wkey[4];
    __shared__ int wpos[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int j = threadIdx.x; j < dim; j += 256) centre[j] = M[(size_t)(t - 1) * ldm + j];
    __syncthreads();
    double bk = INFINITY;
    int bp = INT_MAX;
    // a wave takes KM_SEED_ROWS positions at a time, lanes along a row: every load is issued before the first sum; lane u then
    // draws the key of position u, so a key is formed once
    for (int i0 = (blockIdx.x * 4 + wave) * KM_SEED_ROWS; i0 < n; i0 += gridDim.x * 4 * KM_SEED_ROWS) {
        const int i_mine = i0 + lane;
        const int r_mine = lane < KM_SEED_ROWS && i_mine < n ? list_row(d_rows, i_mine, n_table) : -1;
        const float f_mine = r_mine >= 0 && inv_norm ? inv_norm[r_mine] : 1.f;
        const float old_mine = r_mine >= 0 ? d2min[i_mine] : 0.f;
        float v[KM_SEED_ROWS][4];
#pragma unroll
        for (int u = 0; u < KM_SEED_ROWS; u++) {
            const int r = __shfl(r_mine, u, WAVE);
#pragma unroll
            for (int w = 0; w < 4; w++) {
                const int col = lane + WAVE * w;
                v[u][w] = r >= 0 && col < dim ? table[(size_t)r * ld + col] : 0.f;
            }
        }
        float d2_mine = 0.f;
#pragma unroll
        for (int u = 0; u < KM_SEED_ROWS; u++) {
            const float f = __shfl(f_mine, u, WAVE);
            float a = 0.f;
#pragma unroll
            for (int w = 0; w < 4; w++) {
                const int col = lane + WAVE * w;
                if (col < dim) {
                    const float d = __fmul_rn(v[u][w], f) - centre[col];   // the rounded product, as the centre holds it: never one fma
                    a = fmaf(d, d, a);
                }
            }
            a = wave_sum(a);
            if (lane == u) d2_mine = a;
        }
        if (r_mine >= 0) {                                      // an invalid row stays (+inf, INT_MAX): behind every row of the table
            const float dm = fminf(old_mine, d2_mine);
            d2min[i_mine] = dm;
            double key = INFINITY;
            if (dm > 0.f) key = -log(((double)seed_word((uint32_t)i_mine, (uint32_t)t, s) + 0.5) * 0x1p-32) / (double)dm;
            if (key_before(key, i_mine, bk, bp)) { bk = key; bp = i_mine; }
        }
    }
#pragma unroll
    for (int off = 1; off < KM_SEED_ROWS; off <<= 1) {          // the lanes that hold keys
        const double ok = __shfl_xor(bk, off, WAVE);
        const int op = __shfl_xor(bp, off, WAVE);
        if (key_before(ok, op, bk, bp)) { bk = ok; bp = op; }
    }
    if (lane == 0) { wkey[wave] = bk; wpos[wave] = bp; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; w++)
            if (key_before(wkey[w], wpos[w], bk, bp)) { bk = wkey[w]; bp = wpos[w]; }
        part_key[blockIdx.x] = bk;
        part_pos[blockIdx.x] = bp;
    }
}

// one block: the smallest of the workgroups' answers; its row, scaled, becomes centre t
__global__ __launch_bounds__(256) void kmeans_seed_pick_kernel(const float *__restrict__ table, int ld, int n_table, int dim,
                                                               const float *__restrict__ inv_norm, const int32_t *__restrict__ d_rows,
                                                               const double *__restrict__ part_key, const int32_t *__restrict__ part_pos,
                                                               int n_parts, int t, float *__restrict__ M, int ldm, int32_t *__restrict__ seed_pos) {
    __shared__ double rk[256];
    __shared__ int rp[256];
    const int th = threadIdx.x;
    double bk = INFINITY;
    int bp = INT_MAX;
    for (int b = th; b < n_parts; b += 256)
        if (key_before(part_key[b], part_pos[b], bk, bp)) { bk = part_key[b]; bp = part_pos[b]; }
    rk[th] = bk;
    rp[th] = bp;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (th < w && key_before(rk[th + w], rp[th + w], rk[th], rp[th])) { rk[th] = rk[th + w]; rp[th] = rp[th + w]; }
        __syncthreads();
    }
    const int p = rp[0];                                        // INT_MAX: the list names no row of the table
    const int r = p != INT_MAX ? list_row(d_rows, p, n_table) : -1;
    const float f = r >= 0 && inv_norm ? inv_norm[r] : 1.f;
    if (th == 0) seed_pos[t] = r >= 0 ? p : -1;
    for (int j = th; j < dim; j += 256) M[(size_t)t * ldm + j] = r >= 0 ? table[(size_t)r * ld + j] * f : 0.f;
}

// ---- the cluster x class table ----------------------------------------------------------------------------------------------

__global__ __launch_bounds__(256) void contingency_rows_kernel(const int32_t *__restrict__ assign, const int32_t *__restrict__ truth, int n_truth,
                                                               const int32_t *__restrict__ d_rows, int n, int k, int C,
                                                               int32_t *__restrict__ counts, int32_t *__restrict__ skipped) {
    extern __shared__ int cell[];                               // [k x C], then the skipped count
    const int cells = k * C;
    for (int e = threadIdx.x; e <= cells; e += 256) cell[e] = 0;
    __syncthreads();
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
        const int a = assign[i];
        const int r = list_row(d_rows, i, n_truth);
        const int y = r >= 0 ? truth[r] : -1;
        if (a >= 0 && a < k && y >= 0 && y < C) atomicAdd(&cell[a * C + y], 1);
        else atomicAdd(&cell[cells], 1);
    }
    __syncthreads();
    for (int e = threadIdx.x; e < cells; e += 256)
        if (cell[e]) atomicAdd(&counts[e], cell[e]);
    if (threadIdx.x == 0 && cell[cells]) atomicAdd(skipped, cell[cells]);
}

// ---- entry points ------------------------------------------------------------------------------------------------------------

static const char *kmeans_refusal(const void *table, int ld, int n_table, int dim, const int32_t *d_rows, int n, int k) {
    if (!table || n_table < 0 || n < 0) return "invalid argument";
    if (dim < 1 || dim > KM_MAX_DIM) return "1 <= dim <= 256";
    if (ld < dim) return "the row stride is below dim";
    if (k < 1 || k > KM_MAX_K) return "1 <= k <= 256";
    if (!d_rows && n > n_table) return "without a row list n is at most n_table";
    return nullptr;
}
#define KM_REFUSE(NAME, WHY)                                                      \
    do {                                                                          \
        char msg[160];                                                            \
        snprintf(msg, sizeof msg, "%s: %s", NAME, WHY);                           \
        return gcnhip_fail(msg);                                                  \
    } while (0)

static size_t up256(size_t b) { return (b + 255) / 256 * 256; }

// the update's scratch: {hist | cstart, segstart | order | dpart | acc | partials}
struct KmLayout {
    int n_chunks, seg_max;
    size_t hist, starts, order, dpart, acc, partials, fixed;
};
static KmLayout km_layout(int n, int k, int dim) {
    KmLayout L;
    L.n_chunks = std::max(ceil_div(n, KM_CHUNK), 1);
    L.seg_max = n / KM_SEG + k;                                 // sum of ceil(size_c / KM_SEG) is at most this
    L.hist = 0;
    L.starts = L.hist + up256((size_t)L.n_chunks * k * sizeof(int32_t));
    L.order = L.starts + up256(2 * (size_t)(k + 1) * sizeof(int32_t));
    L.dpart = L.order + up256((size_t)std::max(n, 1) * sizeof(int32_t));
    L.acc = L.dpart + up256((size_t)L.n_chunks * sizeof(double));
    L.partials = L.acc + up256((size_t)k * dim * sizeof(double));
    L.fixed = L.partials;
    return L;
}

extern "C" {

int gcnhip_kmeans_plan(int n, int k, int dim, size_t *update_bytes, size_t *update_bytes_min, size_t *seed_bytes) {
    if (n < 0 || dim < 1 || dim > KM_MAX_DIM) return gcnhip_fail("gcnhip_kmeans_plan: invalid argument (n >= 0, 1 <= dim <= 256)");
    if (k < 1 || k > KM_MAX_K) return gcnhip_fail("gcnhip_kmeans_plan: 1 <= k <= 256");
    const KmLayout L = km_layout(n, k, dim);
    const size_t per_seg = (size_t)dim * sizeof(double);
    if (update_bytes) *update_bytes = L.fixed + per_seg * (size_t)std::max(L.seg_max, KM_MIN_SEGS);
    if (update_bytes_min) *update_bytes_min = L.fixed + per_seg * KM_MIN_SEGS;
    if (seed_bytes) *seed_bytes = up256((size_t)std::max(n, 1) * sizeof(float)) + up256(KM_SEED_PARTS * sizeof(double)) + up256(KM_SEED_PARTS * sizeof(int32_t));
    return 0;
}

int gcnhip_kmeans_assign(gcnhip_ctx *c, const float *table, int ld, int n_table, int dim, const float *inv_norm, const int32_t *d_rows, int n,
                         const float *centers, int ldm, const float *cn, int k, const int32_t *prev, int32_t *assign, float *dist2,
                         int32_t *moved) {
    if (!c || !centers || !cn || !moved || (n > 0 && (!assign || !dist2))) return gcnhip_fail("gcnhip_kmeans_assign: invalid argument");
    if (const char *why = kmeans_refusal(table, ld, n_table, dim, d_rows, n, k)) KM_REFUSE("gcnhip_kmeans_assign", why);
    if (ldm < dim) return gcnhip_fail("gcnhip_kmeans_assign: the row stride of the centres is below dim");
    GCNHIP_TRY(hipMemsetAsync(moved, 0, sizeof(int32_t), c->stream));
    if (n == 0) return 0;
    const int dpad = (dim + 15) / 16 * 16;
    const size_t lds = sizeof(float) * ((size_t)(KM_RT + KM_CT) * (dpad + 4) + KM_CT + 3 * KM_RT);
    if (lds > 64 * 1024) GCNHIP_TRY(hipFuncSetAttribute((const void *)kmeans_assign_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    const int tiles = ceil_div(n, KM_RT);
    const int blocks = std::min(tiles, 8 * (c->n_cu > 0 ? c->n_cu : 128));
    kmeans_assign_kernel<<<blocks, 256, lds, c->stream>>>(table, ld, n_table, dim, inv_norm, d_rows, n, centers, ldm, cn, k, prev, assign, dist2, moved);
    GCNHIP_LAUNCH_CHECK();
    return 0;
}

int gcnhip_kmeans_update(gcnhip_ctx *c, const float *table, int ld, int n_table, int dim, const float *inv_norm, const int32_t *d_rows, int n,
                         const int32_t *assign, const float *dist2, int k, float *centers, int ldm, int32_t *sizes, float *cn, double *inertia,
                         void *scratch, size_t scratch_bytes) {
    if (!c || !centers || !sizes || !cn || !scratch || (n > 0 && !assign)) return gcnhip_fail("gcnhip_kmeans_update: invalid argument");
    if (const char *why = kmeans_refusal(table, ld, n_table, dim, d_rows, n, k)) KM_REFUSE("gcnhip_kmeans_update", why);
    if (ldm < dim) return gcnhip_fail("gcnhip_kmeans_update: the row stride of the centres is below dim");
    if (!aligned16(scratch)) return gcnhip_fail("gcnhip_kmeans_update: the scratch is not 16-byte aligned");
    size_t need_min = 0;
    if (gcnhip_kmeans_plan(n, k, dim, nullptr, &need_min, nullptr) != 0) return -1;
    if (scratch_bytes < need_min) return gcnhip_fail("gcnhip_kmeans_update: the scratch is below the minimum (gcnhip_kmeans_plan tells the bytes)");
    const KmLayout L = km_layout(n, k, dim);
    unsigned char *base = (unsigned char *)scratch;
    int32_t *hist = (int32_t *)(base + L.hist), *cstart = (int32_t *)(base + L.starts), *segstart = cstart + (k + 1);
    int32_t *order = (int32_t *)(base + L.order);
    double *dpart = (double *)(base + L.dpart), *acc = (double *)(base + L.acc), *partials = (double *)(base + L.partials);
    const int batch = (int)std::min<size_t>((scratch_bytes - L.fixed) / ((size_t)dim * sizeof(double)), (size_t)std::max(L.seg_max, KM_MIN_SEGS));
    GCNHIP_TRY(hipMemsetAsync(acc, 0, (size_t)k * dim * sizeof(double), c->stream));
    kmeans_hist_kernel<<<L.n_chunks, 256, 0, c->stream>>>(assign, d_rows, dist2, n, n_table, k, hist, dpart);
    GCNHIP_LAUNCH_CHECK();
    kmeans_scan_kernel<<<1, 256, 0, c->stream>>>(hist, L.n_chunks, k, KM_SEG, sizes, cstart, segstart);
    GCNHIP_LAUNCH_CHECK();
    if (n > 0) {
        kmeans_scatter_kernel<<<L.n_chunks, 64, 0, c->stream>>>(assign, d_rows, n, n_table, k, hist, cstart, order);
        GCNHIP_LAUNCH_CHECK();
        const int slabs = ceil_div(dim, WAVE);
        for (int s0 = 0; s0 < L.seg_max; s0 += batch) {
            const int s1 = std::min(L.seg_max, s0 + batch);
            kmeans_segsum_kernel<<<ceil_div((int64_t)(s1 - s0) * slabs, 4), 256, 0, c->stream>>>(table, ld, n_table, dim, inv_norm, d_rows, order, cstart,
                                                                                               segstart, k, s0, s1, partials);
            GCNHIP_LAUNCH_CHECK();
            kmeans_fold_kernel<<<k, 256, 0, c->stream>>>(partials, segstart, dim, s0, s1, acc);
            GCNHIP_LAUNCH_CHECK();
        }
    }
    kmeans_finish_kernel<<<k, 256, 0, c->stream>>>(acc, sizes, dim, centers, ldm, cn, dpart, L.n_chunks, inertia);
    GCNHIP_LAUNCH_CHECK();
    return 0;
}

int gcnhip_kmeans_seed(gcnhip_ctx *c, const float *table, int ld, int n_table, int dim, const float *inv_norm, const int32_t *d_rows, int n,
                       int k, uint64_t stream_seed, float *centers, int ldm, int32_t *seed_pos, void *scratch, size_t scratch_bytes) {
    if (!c || !centers || !seed_pos || !scratch) return gcnhip_fail("gcnhip_kmeans_seed: invalid argument");
    if (const char *why = kmeans_refusal(table, ld, n_table, dim, d_rows, n, k)) KM_REFUSE("gcnhip_kmeans_seed", why);
    if (ldm < dim) return gcnhip_fail("gcnhip_kmeans_seed: the row stride of the centres is below dim");
    if (n < 1) return gcnhip_fail("gcnhip_kmeans_seed: an empty list");
    if (!aligned16(scratch)) return gcnhip_fail("gcnhip_kmeans_seed: the scratch is not 16-byte aligned");
    size_t need = 0;
    if (gcnhip_kmeans_plan(n, k, dim, nullptr, nullptr, &need) != 0) return -1;
    if (scratch_bytes < need) return gcnhip_fail("gcnhip_kmeans_seed: the scratch is too small (gcnhip_kmeans_plan tells the bytes)");
    unsigned char *base = (unsigned char *)scratch;
    float *d2min = (float *)base;
    double *part_key = (double *)(base + up256((size_t)n * sizeof(float)));
    int32_t *part_pos = (int32_t *)((unsigned char *)part_key + up256(KM_SEED_PARTS * sizeof(double)));
    const int parts = std::min(KM_SEED_PARTS, ceil_div(n, 4));
    kmeans_seed_init_kernel<<<std::min(ceil_div(n, 256), 1024), 256, 0, c->stream>>>(table, ld, n_table, dim, inv_norm, d_rows, n, stream_seed, centers, ldm,
                                                                                  seed_pos, d2min);
    GCNHIP_LAUNCH_CHECK();
    for (int t = 1; t < k; t++) {
        kmeans_seed_step_kernel<<<parts, 256, 0, c->stream>>>(table, ld, n_table, dim, inv_norm, d_rows, n, stream_seed, t, centers, ldm, d2min, part_key,
                                                            part_pos);
        GCNHIP_LAUNCH_CHECK();
        kmeans_seed_pick_kernel<<<1, 256, 0, c->stream>>>(table, ld, n_table, dim, inv_norm, d_rows, part_key, part_pos, parts, t, centers, ldm, seed_pos);
        GCNHIP_LAUNCH_CHECK();
    }
    return 0;
}

int gcnhip_contingency_rows(gcnhip_ctx *c, const int32_t *assign, const int32_t *truth, int n_truth, const int32_t *d_rows, int n, int k,
                            int num_classes, int32_t *counts, int32_t *skipped) {
    if (!c || !truth || !counts || !skipped || n < 0 || n_truth < 0 || (n > 0 && !assign)) return gcnhip_fail("gcnhip_contingency_rows: invalid argument");
    if (k < 1 || k > KM_MAX_K) return gcnhip_fail("gcnhip_contingency_rows: 1 <= k <= 256");
    if (num_classes < 1 || num_classes > KM_MAX_C) return gcnhip_fail("gcnhip_contingency_rows: 1 <= num_classes <= 64");
    if (!d_rows && n > n_truth) return gcnhip_fail("gcnhip_contingency_rows: without a row list n is at most n_truth");
    GCNHIP_TRY(hipMemsetAsync(counts, 0, (size_t)k * num_classes * sizeof(int32_t), c->stream));
    GCNHIP_TRY(hipMemsetAsync(skipped, 0, sizeof(int32_t), c->stream));
    if (n == 0) return 0;
    const size_t lds = ((size_t)k * num_classes + 1) * sizeof(int);
    if (lds > 64 * 1024) GCNHIP_TRY(hipFuncSetAttribute((const void *)contingency_rows_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    contingency_rows_kernel<<<std::min(ceil_div(n, 256), 256), 256, lds, c->stream>>>(assign, truth, n_truth, d_rows, n, k, num_classes, counts, skipped);
    GCNHIP_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
