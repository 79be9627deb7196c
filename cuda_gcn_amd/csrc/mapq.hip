// mapq.hip — is a map of a table's rows to be believed?  The exact euclidean k nearest neighbours of every listed row among the
// listed rows, the rank a given neighbour holds in a space's distance order, and from both trustworthiness, continuity (Venna &
// Kaski, 2001; scikit-learn's trustworthiness) and the kNN overlap of two spaces, matrix-free: no n x n distance is ever stored,
// every walk recomputes d2 on the exact-f32 MFMA as dbscan.hip does and keeps only integers.  Beyond the reference, which never
// looks at its hidden matrix.  include/gcnhip_driver.h has the definitions.
//
// The rows are the pack gcnhip_tsne_pack makes (tsne_pack.h).  Both walks share the row-tile body of tsne.hip / dbscan.hip: a
// workgroup owns a row tile of 64 positions, four waves of 16 rows, the x^ of the row tile in REGISTERS as the B operand of
// v_mfma_f32_16x16x4_f32, column tiles of 64 positions double-buffered in LDS (the loads of tile t + 1 in flight across the products
// of tile t, one barrier per tile), the 64 x 64 d2 tile in 16 accumulators per lane.  Lane (kg, l15) of wave v holds columns
// 16 g + 4 kg + r (g, r < 4) of ONE row, 16 v + l15: what is per row (a threshold, a count) lives in that lane's registers, the four
// lanes kg = 0..3 of a row agree by ballot or meet by shuffle.  A square walk, every tile: the order of a row's candidates is not
// symmetric.
//
// mapq_knn_kernel<DP, PEND>   the selection walk.  A row's threshold is its current k-th smallest key ((d2 bits) << 32 | position: a
//   total order); an entry enters only below it, which after the first tiles is rare.  Entrants are appended to the row's LDS area
//   (best [32] sorted | pending [PEND]) at the position the ballot of the compare gives; after every 16 columns the rows whose
//   pending part could not hold 16 more, and at the end every row with a pending key, are sorted by their wave: best + pending as a
//   64-key bitonic network across the lanes, the low 32 kept, and the row's lanes take the new threshold.  A wave owns its 16 rows'
//   areas: no barrier beyond the tile's.  PEND is 32; at DP = 256 it is 16 (the two column tiles leave 28 KiB of the 160 KiB), so a
//   row is sorted as soon as it has an entrant.
// mapq_rank_kernel<DP>   the rank walk.  (a) the thresholds: for every t < k the 64 rows x^[targets[r, t]] are gathered into a column
//   tile, the SAME product body runs on it and the diagonal entry (r, r) is kept — the very bits the walk will see at entry (i, j),
//   which VALU arithmetic could not promise — as {d2, position} in LDS.  (b) the walk: cnt[t] += key(entry) < thr[t], a float compare
//   on d2 and the position compare on equality; the counts in 32 registers per lane, the thresholds re-read from LDS in groups of 8
//   per tile; the four lanes of a row meet by shuffle at the end and the rank leaves by a plain store.
// mapq_sums_kernel   a thread per position: the two penalties and the shared neighbours; int64 totals by integer atomics.
#include "common.h"
#include "tsne_pack.h"
#include <cstdio>

using f32x4 = __attribute__((ext_vector_type(4))) float;
typedef unsigned long long mq_key;

constexpr int MQ_T = 64;                          // positions per tile, rows and columns alike
constexpr int MQ_MAX_K = 32;                      // a row's sorted best; with the pending part one wave's bitonic network
constexpr int MQ_THR_LD = MQ_MAX_K + 1;           // the row stride of the rank walk's thresholds in LDS (an odd stride of 8-byte words)
constexpr int MQ_MAX_N = 1 << 26;                 // k . rank <= 32 n stays below 2^31
constexpr mq_key MQ_NONE = ~0ull;                 // above every key: d2 is never NaN and a position is below 2^31

template <int DP>
struct MqTile {                                                 // what a thread holds of a column tile between its loads and its LDS stores
    f32x4 x[DP / 16];
    int2 s;                                                     // {xn bits, a point}
};

template <int DP>
__device__ __forceinline__ void mq_tile_load(MqTile<DP> &T, const float *__restrict__ X, const float4 *__restrict__ S, const int32_t *__restrict__ valid,
                                             int c0) {
    const f32x4 *src = (const f32x4 *)(X + (size_t)c0 * DP);    // the tile is 64 . DP contiguous floats
#pragma unroll
    for (int u = 0; u < DP / 16; u++) T.x[u] = src[threadIdx.x + 256 * u];
    if (threadIdx.x < MQ_T) T.s = make_int2(__float_as_int(S[c0 + threadIdx.x].x), valid[c0 + threadIdx.x]);   // c0 + 63 < n_pad
}

template <int DP>
__device__ __forceinline__ void mq_tile_store(const MqTile<DP> &T, float *__restrict__ Cs, int2 *__restrict__ Is) {
    constexpr int QLD = DP + 4;
#pragma unroll
    for (int u = 0; u < DP / 16; u++) {
        const int idx = threadIdx.x + 256 * u, row = idx / (DP / 4), c4 = idx % (DP / 4);
        *(f32x4 *)(Cs + row * QLD + 4 * c4) = T.x[u];
    }
    if (threadIdx.x < MQ_T) Is[threadIdx.x] = T.s;
}

// the product body of both walks and of the threshold phase: acc[g][r] = dot(x^ of column 16 g + 4 kg + r of the tile, this lane's row),
// one MFMA chain per entry in ascending column order of x^
template <int DP>
__device__ __forceinline__ void mq_products(const float *__restrict__ C, const f32x4 (&b)[DP / 16], f32x4 (&acc)[4], int kg, int l15) {
    constexpr int QLD = DP + 4;
#pragma unroll
    for (int g = 0; g < 4; g++) acc[g] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int c = 0; c < DP / 16; c++) {
        f32x4 a[4];
#pragma unroll
        for (int g = 0; g < 4; g++) a[g] = *(const f32x4 *)(C + (16 * g + l15) * QLD + 16 * c + 4 * kg);
#pragma unroll
        for (int s = 0; s < 4; s++)
#pragma unroll
            for (int g = 0; g < 4; g++) acc[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[g][s], b[c][s], acc[g], 0, 0, 0);
    }
}
__device__ __forceinline__ float mq_d2(float xi, float xj, float dot) { return fmaxf((xi + xj) - 2.f * dot, 0.f); }

// what a wave wrote to LDS is read by other lanes of the same wave
__device__ __forceinline__ void mq_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// the rows of `rows16` (bit r = row r of the wave): best [32] and the pc pending keys sorted together across the 64 lanes, the low 32
// kept; the row's four lanes take key k - 1 as their threshold and an empty pending part.  The whole wave runs it.
template <int PEND>
__device__ __forceinline__ void mq_flush(mq_key *__restrict__ best, mq_key *__restrict__ pend, unsigned rows16, int k, int lane, int l15, mq_key &thr,
                                         int &pc) {
    mq_wave_sync();
    while (rows16) {
        const int row = __ffs(rows16) - 1;
        rows16 &= rows16 - 1;
        const int pcr = __shfl(pc, row, WAVE);                  // lane `row` is lane (kg 0, l15 row)
        mq_key key = MQ_NONE;
        if (lane < MQ_MAX_K) key = best[row * MQ_MAX_K + lane];
        else if (lane - MQ_MAX_K < pcr) key = pend[row * PEND + (lane - MQ_MAX_K)];   // pcr <= PEND
#pragma unroll
        for (int size = 2; size <= WAVE; size <<= 1)
#pragma unroll
            for (int stride = size >> 1; stride > 0; stride >>= 1) {
                const mq_key other = __shfl_xor(key, stride, WAVE);
                const bool keep_min = ((lane & stride) == 0) == ((lane & size) == 0);
                key = (other < key) == keep_min ? other : key;
            }
        if (lane < MQ_MAX_K) best[row * MQ_MAX_K + lane] = key;
        const mq_key kth = __shfl(key, k - 1, WAVE);
        if (l15 == row) { thr = kth; pc = 0; }
    }
    mq_wave_sync();
}

// grid T (row tiles).  pos / d2 [n x k]: the k points l != i of smallest key in ascending key order, -1 / +inf past the candidates
template <int DP, int PEND>
__global__ __launch_bounds__(256) void mapq_knn_kernel(const float *__restrict__ X, const float4 *__restrict__ S, const int32_t *__restrict__ valid,
                                                       int n, int T, int k, int32_t *__restrict__ pos, float *__restrict__ d2out) {
    extern __shared__ __align__(16) unsigned char smem[];
    constexpr int QLD = DP + 4, NCH = DP / 16;
    float *Cs = (float *)smem;                                  // [2][64][QLD]
    int2 *Is = (int2 *)(Cs + 2 * MQ_T * QLD);                   // [2][64]
    mq_key *best_all = (mq_key *)(Is + 2 * MQ_T);               // [64][32]
    mq_key *pend_all = best_all + MQ_T * MQ_MAX_K;              // [64][PEND]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int kg = lane >> 4, l15 = lane & 15;
    mq_key *best = best_all + 16 * wave * MQ_MAX_K, *pend = pend_all + 16 * wave * PEND;   // this wave's 16 rows

    const int I = blockIdx.x, i = I * MQ_T + 16 * wave + l15;
    f32x4 b[NCH];                                               // the row operand: x^_i[16c + 4kg .. + 3]
#pragma unroll
    for (int c = 0; c < NCH; c++) b[c] = *(const f32x4 *)(X + (size_t)i * DP + 16 * c + 4 * kg);
    const float xi = S[i].x;
    const bool vi = valid[i] != 0;
    for (int e = lane; e < 16 * MQ_MAX_K; e += WAVE) best[e] = MQ_NONE;
    mq_key thr = MQ_NONE;
    int pc = 0;                                                 // the row's pending keys; the same in its four lanes

    MqTile<DP> Tl;
    mq_tile_load<DP>(Tl, X, S, valid, 0);
    mq_tile_store<DP>(Tl, Cs, Is);
    __syncthreads();
    for (int t = 0; t < T; t++) {
        const int buf = t & 1, c0 = t * MQ_T;
        if (t + 1 < T) mq_tile_load<DP>(Tl, X, S, valid, c0 + MQ_T);    // in flight across the products below
        const int2 *Ic = Is + buf * MQ_T;
        f32x4 acc[4];
        mq_products<DP>(Cs + buf * MQ_T * QLD, b, acc, kg, l15);
#pragma unroll
        for (int g = 0; g < 4; g++) {
#pragma unroll
            for (int r = 0; r < 4; r++) {                       // D[row 4kg + r][col l15]: column 16g + 4kg + r of the tile, this lane's row
                const int cc = 16 * g + 4 * kg + r, j = c0 + cc;
                const int2 sj = Ic[cc];
                const mq_key key = (mq_key)__float_as_uint(mq_d2(xi, __int_as_float(sj.x), acc[g][r])) << 32 | (unsigned)j;
                const bool enter = vi && sj.y != 0 && j != i && key < thr;
                const unsigned long long m = __ballot(enter);
                if (m) {                                        // the same for the whole wave
                    unsigned mine = 0;                          // bit q: the row's lane kg = q enters
#pragma unroll
                    for (int q = 0; q < 4; q++) mine |= ((unsigned)(m >> (16 * q + l15)) & 1u) << q;
                    if (enter) pend[l15 * PEND + pc + __popc(mine & ((1u << kg) - 1u))] = key;   // pc + 4 <= PEND: see below
                    pc += __popc(mine);
                }
            }
            // a row takes at most 16 entrants from the next 16 columns: the rows that could not hold them are sorted now
            const unsigned full = (unsigned)__ballot(pc > PEND - 16) & 0xffffu;
            if (full) mq_flush<PEND>(best, pend, full, k, lane, l15, thr, pc);
        }
        if (t + 1 < T) mq_tile_store<DP>(Tl, Cs + (buf ^ 1) * MQ_T * QLD, Is + (buf ^ 1) * MQ_T);
        __syncthreads();                                        // tile t is done with, tile t + 1 is in place
    }
    mq_flush<PEND>(best, pend, (unsigned)__ballot(pc > 0) & 0xffffu, k, lane, l15, thr, pc);
    for (int row = 0; row < 16; row++) {
        const int ir = I * MQ_T + 16 * wave + row;
        if (ir < n && lane < k) {
            const mq_key key = best[row * MQ_MAX_K + lane];
            pos[(size_t)ir * k + lane] = key == MQ_NONE ? -1 : (int32_t)(unsigned)key;
            d2out[(size_t)ir * k + lane] = key == MQ_NONE ? __int_as_float(0x7f800000) : __uint_as_float((unsigned)(key >> 32));
        }
    }
}

__device__ __forceinline__ bool vi_of(const int32_t *__restrict__ valid, int i) { return valid[i] != 0; }
// position tj as a target of row i: a point of the list
__device__ __forceinline__ bool mq_target_ok(const int32_t *__restrict__ valid, int tj, int n) { return tj >= 0 && tj < n && valid[tj] != 0; }

// grid T (row tiles).  rank [n x k] = 1 + the points l outside {i, targets[i, t]} whose key in row i is below the target's; 0 where the
// target or the row is no point
// WALK false: phase (a) alone, d2t [n x k] = the threshold distances d2(i, targets[i, t]) as the walk forms them, NaN where there is none
template <int DP, bool WALK>
__global__ __launch_bounds__(256) void mapq_rank_kernel(const float *__restrict__ X, const float4 *__restrict__ S, const int32_t *__restrict__ valid,
                                                        int n, int T, int k, const int32_t *__restrict__ targets, int32_t *__restrict__ rank,
                                                        float *__restrict__ d2t) {
    extern __shared__ __align__(16) unsigned char smem[];
    constexpr int QLD = DP + 4, NCH = DP / 16;
    float *Cs = (float *)smem;                                  // [2][64][QLD]
    int2 *Is = (int2 *)(Cs + 2 * MQ_T * QLD);                   // [2][64]
    int2 *thr = Is + 2 * MQ_T;                                  // [64][MQ_THR_LD]: {d2 bits (NaN: counts nothing), position}
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int kg = lane >> 4, l15 = lane & 15;
    const int lrow = 16 * wave + l15;

    const int I = blockIdx.x, i = I * MQ_T + lrow;
    f32x4 b[NCH];
#pragma unroll
    for (int c = 0; c < NCH; c++) b[c] = *(const f32x4 *)(X + (size_t)i * DP + 16 * c + 4 * kg);
    const float xi = S[i].x;
    const bool vi = valid[i] != 0;
    const int qnan = 0x7fc00000;
    for (int e = threadIdx.x; e < MQ_T * MQ_THR_LD; e += 256) thr[e] = make_int2(qnan, -1);

    // (a) the thresholds: k gathered column tiles, the diagonal entry of each
    for (int t = 0; t < k; t++) {
        __syncthreads();                                        // the last tile's products are done with buffer 0 (and the fill above)
#pragma unroll
        for (int u = 0; u < NCH; u++) {
            const int idx = threadIdx.x + 256 * u, row = idx / (DP / 4), c4 = idx % (DP / 4), ir = I * MQ_T + row;
            const int tj = ir < n ? targets[(size_t)ir * k + t] : -1;
            const int src = mq_target_ok(valid, tj, n) ? tj : 0;   // position 0 is in every pack; the entry is then not kept
            *(f32x4 *)(Cs + row * QLD + 4 * c4) = *(const f32x4 *)(X + (size_t)src * DP + 4 * c4);
        }
        if (threadIdx.x < MQ_T) {
            const int ir = I * MQ_T + threadIdx.x;
            const int tj = ir < n ? targets[(size_t)ir * k + t] : -1;
            const bool ok = mq_target_ok(valid, tj, n);
            Is[threadIdx.x] = make_int2(__float_as_int(S[ok ? tj : 0].x), ok ? tj : -1);
        }
        __syncthreads();
        f32x4 acc[4];
        mq_products<DP>(Cs, b, acc, kg, l15);
        if (kg == (l15 >> 2)) {                                 // entry (lrow, lrow): g = wave, 4 kg + r = l15
            const f32x4 av = wave == 0 ? acc[0] : wave == 1 ? acc[1] : wave == 2 ? acc[2] : acc[3];
            const int r = l15 & 3;
            const float dot = r == 0 ? av[0] : r == 1 ? av[1] : r == 2 ? av[2] : av[3];
            const int2 sj = Is[lrow];
            if (sj.y >= 0) thr[lrow * MQ_THR_LD + t] = make_int2(__float_as_int(mq_d2(xi, __int_as_float(sj.x), dot)), sj.y);
        }
    }
    __syncthreads();
    if (!WALK) {
        for (int e = threadIdx.x; e < MQ_T * k; e += 256) {
            const int row = e / k, t = e % k, ir = I * MQ_T + row;
            if (ir < n) d2t[(size_t)ir * k + t] = vi_of(valid, ir) ? __int_as_float(thr[row * MQ_THR_LD + t].x) : __int_as_float(qnan);
        }
        return;
    }

    // (b) the walk over every column tile
    int cnt[MQ_MAX_K] = {};
    MqTile<DP> Tl;
    mq_tile_load<DP>(Tl, X, S, valid, 0);
    mq_tile_store<DP>(Tl, Cs, Is);
    __syncthreads();
    for (int t = 0; t < T; t++) {
        const int buf = t & 1, c0 = t * MQ_T;
        if (t + 1 < T) mq_tile_load<DP>(Tl, X, S, valid, c0 + MQ_T);
        const int2 *Ic = Is + buf * MQ_T;
        f32x4 acc[4];
        mq_products<DP>(Cs + buf * MQ_T * QLD, b, acc, kg, l15);
        float dv[16];                                           // NaN where the entry is no candidate: below and equal to nothing
#pragma unroll
        for (int g = 0; g < 4; g++)
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int cc = 16 * g + 4 * kg + r;
                const int2 sj = Ic[cc];
                const float d2 = mq_d2(xi, __int_as_float(sj.x), acc[g][r]);
                dv[4 * g + r] = sj.y != 0 && c0 + cc != i ? d2 : __int_as_float(qnan);
            }
#pragma unroll
        for (int q = 0; q < MQ_MAX_K / 8; q++)
            if (8 * q < k) {                                    // the same for every thread
                int2 th[8];
#pragma unroll
                for (int e = 0; e < 8; e++) th[e] = thr[lrow * MQ_THR_LD + 8 * q + e];
#pragma unroll
                for (int g = 0; g < 4; g++)
#pragma unroll
                    for (int r = 0; r < 4; r++) {
                        const float d2 = dv[4 * g + r];
                        const int j = c0 + 16 * g + 4 * kg + r;
#pragma unroll
                        for (int e = 0; e < 8; e++) {
                            const float td = __int_as_float(th[e].x);
                            cnt[8 * q + e] += (d2 < td || (d2 == td && j < th[e].y)) ? 1 : 0;
                        }
                    }
            }
        if (t + 1 < T) mq_tile_store<DP>(Tl, Cs + (buf ^ 1) * MQ_T * QLD, Is + (buf ^ 1) * MQ_T);
        __syncthreads();
    }
#pragma unroll
    for (int t = 0; t < MQ_MAX_K; t++)
        if (t < k) {
            int tot = cnt[t];
            tot += __shfl_xor(tot, 16, WAVE);
            tot += __shfl_xor(tot, 32, WAVE);
            if (kg == (t & 3) && i < n) rank[(size_t)i * k + t] = vi && mq_target_ok(valid, targets[(size_t)i * k + t], n) ? tot + 1 : 0;
        }
}

__global__ __launch_bounds__(64) void mapq_zero_kernel(long long *__restrict__ totals) {
    if (threadIdx.x < 4) totals[threadIdx.x] = 0;
}

// a thread per position.  per [n x 3] = {trust penalty, continuity penalty, shared}; totals [4] += {the three sums, the points}
__global__ __launch_bounds__(256) void mapq_sums_kernel(const int32_t *__restrict__ valid_x, const int32_t *__restrict__ valid_y, int n, int k,
                                                        const int32_t *__restrict__ knn_x, const int32_t *__restrict__ knn_y,
                                                        const int32_t *__restrict__ rank_x, const int32_t *__restrict__ rank_y,
                                                        int32_t *__restrict__ per, long long *__restrict__ totals) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    int v[4] = {0, 0, 0, 0};
    if (i < n && valid_x[i] != 0 && valid_y[i] != 0) {
        v[3] = 1;
        for (int t = 0; t < k; t++) {
            const size_t e = (size_t)i * k + t;
            v[0] += max(rank_x[e] - k, 0);
            v[1] += max(rank_y[e] - k, 0);
            const int a = knn_x[e];
            if (a >= 0)
                for (int u = 0; u < k; u++) v[2] += knn_y[(size_t)i * k + u] == a;
        }
    }
    if (i < n)
        for (int q = 0; q < 3; q++) per[(size_t)i * 3 + q] = v[q];
#pragma unroll
    for (int q = 0; q < 4; q++) {
        long long s = v[q];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, WAVE);
        if ((threadIdx.x & 63) == 0 && s) atomicAdd((unsigned long long *)&totals[q], (unsigned long long)s);
    }
}

// ---- entry points ------------------------------------------------------------------------------------------------------------

static size_t mq_tiles_lds(int dp) { return sizeof(float) * (size_t)(2 * MQ_T * (dp + 4)) + 2 * MQ_T * sizeof(int2); }

template <int DP>
static int mq_knn_launch(gcnhip_ctx *c, const TsPack &P, int n, int k, int32_t *pos, float *d2) {
    constexpr int PEND = DP == 256 ? 16 : 32;
    const size_t lds = mq_tiles_lds(DP) + (size_t)MQ_T * (MQ_MAX_K + PEND) * sizeof(mq_key);
    auto kern = mapq_knn_kernel<DP, PEND>;
    if (lds > 64 * 1024) GCNHIP_TRY(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    const int T = ts_npad(n) / MQ_T;
    kern<<<T, 256, lds, c->stream>>>(P.X, P.S, P.valid, n, T, k, pos, d2);
    GCNHIP_LAUNCH_CHECK();
    return 0;
}
template <int DP, bool WALK>
static int mq_rank_launch_as(gcnhip_ctx *c, const TsPack &P, int n, int k, const int32_t *targets, int32_t *rank, float *d2t) {
    const size_t lds = mq_tiles_lds(DP) + (size_t)MQ_T * MQ_THR_LD * sizeof(int2);
    auto kern = mapq_rank_kernel<DP, WALK>;
    if (lds > 64 * 1024) GCNHIP_TRY(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    const int T = ts_npad(n) / MQ_T;
    kern<<<T, 256, lds, c->stream>>>(P.X, P.S, P.valid, n, T, k, targets, rank, d2t);
    GCNHIP_LAUNCH_CHECK();
    return 0;
}
template <int DP>
static int mq_rank_launch(gcnhip_ctx *c, const TsPack &P, int n, int k, const int32_t *targets, int32_t *rank, float *d2t) {
    return rank ? mq_rank_launch_as<DP, true>(c, P, n, k, targets, rank, nullptr) : mq_rank_launch_as<DP, false>(c, P, n, k, targets, nullptr, d2t);
}
#define MQ_BY_DP(dp, fn, ...)                          \
    switch (dp) {                                      \
    case 16: return fn<16>(__VA_ARGS__);               \
    case 32: return fn<32>(__VA_ARGS__);               \
    case 64: return fn<64>(__VA_ARGS__);               \
    case 128: return fn<128>(__VA_ARGS__);             \
    default: return fn<256>(__VA_ARGS__);              \
    }

static const char *mq_common(const gcnhip_ctx *c, const void *pack, int n, int dim, int k) {
    if (!c || !pack || n < 1) return "invalid argument";
    if (n > MQ_MAX_N) return "at most 2^26 positions (a position's penalty sum is an int32)";
    if (dim < 1 || dim > TS_MAX_DIM) return "1 <= dim <= 256";
    if (k < 1 || k > MQ_MAX_K) return "1 <= k <= 32";
    if (!aligned16(pack)) return "the pack is not 16-byte aligned";
    return nullptr;
}
static int mq_refuse(const char *name, const char *why) {
    static thread_local char msg[160];
    snprintf(msg, sizeof msg, "%s: %s", name, why);
    return gcnhip_fail(msg);
}

extern "C" {

int gcnhip_mapq_plan(int n, int dim, int k, size_t *pack_bytes, size_t *scratch_bytes) {
    if (n < 0 || dim < 1 || dim > TS_MAX_DIM) return mq_refuse("gcnhip_mapq_plan", "invalid argument (n >= 0, 1 <= dim <= 256)");
    if (k < 1 || k > MQ_MAX_K) return mq_refuse("gcnhip_mapq_plan", "1 <= k <= 32");
    if (pack_bytes) *pack_bytes = ts_pack(nullptr, n, dim).bytes;
    if (scratch_bytes) *scratch_bytes = 0;                      // every row tile walks all of its columns: no per-part lists to merge
    return 0;
}

int gcnhip_knn_rows(gcnhip_ctx *c, const void *pack, int n, int dim, int k, int32_t *pos, float *d2) {
    if (const char *why = mq_common(c, pack, n, dim, k)) return mq_refuse("gcnhip_knn_rows", why);
    if (!pos || !d2) return mq_refuse("gcnhip_knn_rows", "invalid argument");
    const TsPack P = ts_pack((void *)pack, n, dim);
    MQ_BY_DP(ts_dp(dim), mq_knn_launch, c, P, n, k, pos, d2)
}

int gcnhip_nbr_ranks(gcnhip_ctx *c, const void *pack, int n, int dim, int k, const int32_t *targets, int32_t *rank) {
    if (const char *why = mq_common(c, pack, n, dim, k)) return mq_refuse("gcnhip_nbr_ranks", why);
    if (!targets || !rank) return mq_refuse("gcnhip_nbr_ranks", "invalid argument");
    const TsPack P = ts_pack((void *)pack, n, dim);
    MQ_BY_DP(ts_dp(dim), mq_rank_launch, c, P, n, k, targets, rank, (float *)nullptr)
}

int gcnhip_nbr_d2(gcnhip_ctx *c, const void *pack, int n, int dim, int k, const int32_t *targets, float *d2) {
    if (const char *why = mq_common(c, pack, n, dim, k)) return mq_refuse("gcnhip_nbr_d2", why);
    if (!targets || !d2) return mq_refuse("gcnhip_nbr_d2", "invalid argument");
    const TsPack P = ts_pack((void *)pack, n, dim);
    MQ_BY_DP(ts_dp(dim), mq_rank_launch, c, P, n, k, targets, (int32_t *)nullptr, d2)
}

int gcnhip_mapq_sums(gcnhip_ctx *c, const void *pack_x, int dim_x, const void *pack_y, int dim_y, int n, int k, const int32_t *knn_x,
                     const int32_t *knn_y, const int32_t *rank_x, const int32_t *rank_y, int32_t *per_position, int64_t *totals) {
    if (const char *why = mq_common(c, pack_x, n, dim_x, k)) return mq_refuse("gcnhip_mapq_sums", why);
    if (const char *why = mq_common(c, pack_y, n, dim_y, k)) return mq_refuse("gcnhip_mapq_sums", why);
    if (!knn_x || !knn_y || !rank_x || !rank_y || !per_position || !totals) return mq_refuse("gcnhip_mapq_sums", "invalid argument");
    mapq_zero_kernel<<<1, 64, 0, c->stream>>>((long long *)totals);
    GCNHIP_LAUNCH_CHECK();
    mapq_sums_kernel<<<ceil_div(n, 256), 256, 0, c->stream>>>(ts_pack((void *)pack_x, n, dim_x).valid, ts_pack((void *)pack_y, n, dim_y).valid, n, k, knn_x,
                                                              knn_y, rank_x, rank_y, per_position, (long long *)totals);
    GCNHIP_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
