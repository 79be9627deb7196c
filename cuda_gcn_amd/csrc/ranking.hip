// ranking.hip — threshold-free ranking metrics (per-class ROC-AUC and average precision) on score rows that stay on the
// device.  Beyond the reference, which stops at accuracy.  Three launches, none of them part of a captured epoch:
//
//   gcnhip_rank_keys          the score table [rows x ld] -> two column-major key tables [class x listed row], one holding the
//                             keys of a class's positives, one of its negatives, every other entry the padding sentinel
//   gcnhip_sort_segments_u32  every segment (a class's column) sorted ascending: a bitonic network per tile of SORT_TILE keys,
//                             then merge-path passes that double the sorted run length, ping-ponging with a scratch table
//   gcnhip_rank_stats         per positive, binary searches in the two sorted columns -> u2 (int64) and ap_sum (float64) per class
//
// Key.  key(s) is the order-preserving u32 image of the f32 s: -0.0 is +0.0 first; then with b = bits(s) the key is ~b when
// the sign bit is set and b | 0x80000000 otherwise.  Two non-NaN floats compare equal exactly when their keys are equal, and
// a < b exactly when key(a) < key(b).  The largest key of a non-NaN score is key(+inf) = 0xFF800000, so the sentinel
// 0xFFFFFFFF is no score's key and sorts behind every one of them.  NaN scores get no key (counted in invalid[c]).
//
// AUC.  U2 = sum over positives i of #{negatives with key < key_i} + #{negatives with key <= key_i}: an exact integer,
// auc = U2 / (2 P N) — the Mann-Whitney statistic with mid-rank ties.
// AP.   ap_sum = sum over positives i of TP_ge(i) / (TP_ge(i) + FP_ge(i)), TP_ge / FP_ge = the positives / negatives with key
// >= key_i: one float64 division of two exact integers per positive; ap = ap_sum / P.
//
// Determinism.  The counts are integer atomics (integer adds commute); the sort has no payload, so every correct sort gives
// the same bits; u2 is an integer sum; ap_sum is added per thread in index order, over the wave and the block in a fixed tree,
// and over the blocks of a class in block order by a fold launch.  Two launches give the same bits.
#include "common.h"
#include <algorithm>
#include <cstdio>
#pragma clang fp contract(off)
#include "score_rules.h"                                       // the key, the sentinel, the searches in a sorted column

constexpr int SORT_TILE = GCNHIP_SORT_TILE;                    // keys a workgroup sorts or merges at a time
constexpr int SORT_THREADS = 256, SORT_PER = SORT_TILE / SORT_THREADS;
constexpr int SORT_N_MAX = 1 << 24;
// LDS image of a tile: key i sits at word i + (i >> 4) — a thread's 16 consecutive keys start 17 words apart, so the lanes of
// a wave reading "their" keys, or the keys of a partner thread, touch 32 different banks; consecutive i stay (almost)
// consecutive for the coalescing copies.  One word past the last key may be read (never used) by the serial merge.
constexpr int SORT_LDS_WORDS = SORT_TILE + SORT_TILE / 16 + 1;
static_assert(SORT_PER == 16, "the register network below is laid out for 16 keys per thread");

namespace {

__device__ __forceinline__ int sort_phys(int i) { return i + (i >> 4); }

// One compare-exchange step of the bitonic network over the 4096 keys of a tile, key i = 16 t + e in register e of thread t:
// partner i ^ J, ascending where (i & K) == 0.  J < 16: both keys are this thread's.  16 <= J < 1024: the partner is lane ^
// (J / 16) of the same wave, one cross-lane move per key.  J >= 1024: another wave's, through the LDS image.
template <int K, int J>
__device__ __forceinline__ void bitonic_step(uint32_t (&v)[SORT_PER], uint32_t *sh, int t) {
    if constexpr (J < SORT_PER) {
#pragma unroll
        for (int e = 0; e < SORT_PER; e++) {
            if ((e & J) == 0) {
                const bool asc = (((t * SORT_PER + e) & K) == 0);
                const uint32_t lo = min(v[e], v[e | J]), hi = max(v[e], v[e | J]);
                v[e] = asc ? lo : hi;
                v[e | J] = asc ? hi : lo;
            }
        }
    } else {
        constexpr int PT = J / SORT_PER;                       // the partner thread is t ^ PT
        const bool keep_min = ((t & PT) == 0) == (((t * SORT_PER) & K) == 0);
        if constexpr (PT < WAVE) {
#pragma unroll
            for (int e = 0; e < SORT_PER; e++) {
                const uint32_t o = (uint32_t)__shfl_xor((int)v[e], PT, WAVE);
                v[e] = keep_min ? min(v[e], o) : max(v[e], o);
            }
        } else {
#pragma unroll
            for (int e = 0; e < SORT_PER; e++) sh[t * (SORT_PER + 1) + e] = v[e];
            __syncthreads();
#pragma unroll
            for (int e = 0; e < SORT_PER; e++) {
                const uint32_t o = sh[(t ^ PT) * (SORT_PER + 1) + e];
                v[e] = keep_min ? min(v[e], o) : max(v[e], o);
            }
            __syncthreads();
        }
    }
}
template <int K, int J>
__device__ __forceinline__ void bitonic_steps(uint32_t (&v)[SORT_PER], uint32_t *sh, int t) {
    bitonic_step<K, J>(v, sh, t);
    if constexpr (J > 1) bitonic_steps<K, J / 2>(v, sh, t);
}
template <int K>
__device__ __forceinline__ void bitonic_stages(uint32_t (&v)[SORT_PER], uint32_t *sh, int t) {
    if constexpr (K > 2) bitonic_stages<K / 2>(v, sh, t);
    bitonic_steps<K, K / 2>(v, sh, t);
}

// the registers' keys (thread t holds keys 16 t .. 16 t + 15 of the tile) -> dst[0 .. valid), coalesced through the LDS image
__device__ __forceinline__ void sort_store_tile(const uint32_t (&v)[SORT_PER], uint32_t *sh, int t, uint32_t *dst, int valid) {
#pragma unroll
    for (int e = 0; e < SORT_PER; e++) sh[t * (SORT_PER + 1) + e] = v[e];
    __syncthreads();
#pragma unroll
    for (int r = 0; r < SORT_PER; r++) {
        const int g = r * SORT_THREADS + t;
        if (g < valid) dst[g] = sh[sort_phys(g)];
    }
}

// Merge path: how many of the first d keys of merge(A, B) come from A, A's key first on a tie
__device__ inline int merge_path_global(const uint32_t *A, int la, const uint32_t *B, int lb, int d) {
    int lo = d > lb ? d - lb : 0, hi = d < la ? d : la;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (A[mid] <= B[d - 1 - mid]) lo = mid + 1; else hi = mid;
    }
    return lo;
}
// the same on the staged image: A = keys [0, na), B = keys [na, na + nb)
__device__ inline int merge_path_lds(const uint32_t *sh, int na, int nb, int d) {
    int lo = d > nb ? d - nb : 0, hi = d < na ? d : na;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (sh[sort_phys(mid)] <= sh[sort_phys(na + d - 1 - mid)]) lo = mid + 1; else hi = mid;
    }
    return lo;
}

}  // namespace

// A workgroup per tile: tile `tile` of segment `seg` (keys [tile . SORT_TILE, ...) of the segment's n) sorted from src to dst
// (which may be the same table: a block reads its tile before it writes it, and no other block touches it).
__global__ __launch_bounds__(SORT_THREADS) void sort_tiles_kernel(const uint32_t *src, uint32_t *dst, int n, int64_t stride, int tiles) {
    __shared__ uint32_t sh[SORT_LDS_WORDS];
    const int t = threadIdx.x;
    const int seg = blockIdx.x / tiles, tile = blockIdx.x - seg * tiles;
    const int64_t base = (int64_t)seg * stride + (int64_t)tile * SORT_TILE;
    const int left = n - tile * SORT_TILE, valid = left < SORT_TILE ? left : SORT_TILE;
    uint32_t v[SORT_PER];
    // which key starts in which register does not matter to a sort: the loads coalesce
#pragma unroll
    for (int e = 0; e < SORT_PER; e++) {
        const int g = e * SORT_THREADS + t;
        v[e] = g < valid ? src[base + g] : RANK_SENTINEL;      // padding sorts to the end, behind (or among equal) real keys
    }
    bitonic_stages<SORT_TILE>(v, sh, t);
    sort_store_tile(v, sh, t, dst + base, valid);
}

// One merge pass: runs of length L (a multiple of SORT_TILE; the last of a segment may be shorter or missing) -> runs of 2 L.
// A workgroup writes output tile `tile` of its segment: the diagonals at its two ends are split by binary search in global
// memory (two threads, one each), the at most SORT_TILE keys between the splits are staged, every thread finds its own split
// in the image and merges 16 keys serially.
__global__ __launch_bounds__(SORT_THREADS) void sort_merge_kernel(const uint32_t *src, uint32_t *dst, int n, int64_t stride, int tiles, int L) {
    __shared__ uint32_t sh[SORT_LDS_WORDS];
    __shared__ int split[2];
    const int t = threadIdx.x;
    const int seg = blockIdx.x / tiles, tile = blockIdx.x - seg * tiles;
    const int o0 = tile * SORT_TILE;                           // < n
    const int pair0 = o0 / (2 * L) * (2 * L);
    const int rest = n - pair0;
    const int la = rest < L ? rest : L, lb = rest - la < L ? rest - la : L;
    const uint32_t *A = src + (int64_t)seg * stride + pair0, *B = A + la;
    const int d0 = o0 - pair0;                                 // < la + lb
    const int d1 = d0 + SORT_TILE < la + lb ? d0 + SORT_TILE : la + lb;
    if (t == 0) split[0] = merge_path_global(A, la, B, lb, d0);
    if (t == WAVE) split[1] = merge_path_global(A, la, B, lb, d1);
    __syncthreads();
    const int a0 = split[0], b0 = d0 - a0;
    const int na = split[1] - a0, total = d1 - d0, nb = total - na;
    for (int g = t; g < total; g += SORT_THREADS) sh[sort_phys(g)] = g < na ? A[a0 + g] : B[b0 + g - na];
    __syncthreads();
    const int diag = t * SORT_PER < total ? t * SORT_PER : total;
    int ai = merge_path_lds(sh, na, nb, diag);
    int bi = na + (diag - ai);                                 // index into the image
    uint32_t ka = sh[sort_phys(ai)], kb = sh[sort_phys(bi < total ? bi : total)];
    uint32_t v[SORT_PER];
#pragma unroll
    for (int e = 0; e < SORT_PER; e++) {
        const bool take_a = bi >= total || (ai < na && ka <= kb);
        v[e] = take_a ? ka : kb;
        ai += take_a;
        bi += !take_a;
        const int nxt = take_a ? ai : bi;
        const uint32_t x = sh[sort_phys(nxt < total ? nxt : total)];     // past the end: read, never taken
        ka = take_a ? x : ka;
        kb = take_a ? kb : x;
    }
    __syncthreads();
    sort_store_tile(v, sh, t, dst + (int64_t)seg * stride + o0, total);
}

// ---- keys ------------------------------------------------------------------------------------------------------------------
// A workgroup walks tiles of 64 listed rows x 64 classes (its column of classes is blockIdx.y).  Per tile: wave 0 fetches the
// rows and their truth; the waves walk the rows, lane j on class cb + j (the table reads coalesce along a row, a wave's 16 rows
// in flight together); then, through the LDS tile, they walk the classes, lane i on listed row i0 + i (the key writes coalesce
// along a column) and count by ballot into the block's LDS counters — a class belongs to one wave, so no LDS atomics.  The
// block adds its counters to global memory once, a class per lane: one contiguous atomic instruction per counter and block
// (a lane-0 atomic per class and tile serialised on the 3 C addresses and cost four times the rest of the kernel).
constexpr int RK_TILE = 64, RK_MAX_BLOCKS = 1024;
enum { RK_NONE = 0, RK_POS = 1, RK_NEG = 2, RK_INVALID = 3 };

__global__ __launch_bounds__(256) void rank_keys_kernel(const float *__restrict__ table, int ld, int n_table, const int32_t *__restrict__ rows, int n,
                                                        int c0, int c1, int num_classes, const int32_t *__restrict__ truth,
                                                        const uint32_t *__restrict__ truth_bits, int wpr, uint32_t *__restrict__ pos_keys,
                                                        uint32_t *__restrict__ neg_keys, int64_t stride, int32_t *pos, int32_t *neg, int32_t *invalid,
                                                        int32_t *unlabelled) {
    __shared__ uint32_t key[RK_TILE][RK_TILE + 1];
    __shared__ uint8_t cat[RK_TILE][RK_TILE + 4];              // a row is 17 words: lanes reading a column touch different banks
    __shared__ int sh_row[RK_TILE], sh_truth[RK_TILE];
    __shared__ int sh_count[3][RK_TILE];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int cb = c0 + blockIdx.y * RK_TILE, c = cb + lane;
    const int tiles = (n + RK_TILE - 1) / RK_TILE;
    if (wave < 3) sh_count[wave][lane] = 0;                    // first touched again behind the tile loop's barriers
    int no_label = 0;
    for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int i0 = tile * RK_TILE;
        if (wave == 0) {
            const int i = i0 + lane;
            int r = -1, tr = -1;
            if (i < n) {
                r = rows ? rows[i] : i;
                if (r < 0 || r >= n_table) r = -1;             // an id outside the table is in no class either
                else if (truth) tr = truth[r];
            }
            const bool labelled = r >= 0 && (!truth || (tr >= 0 && tr < num_classes));
            if (!labelled) r = -1;
            sh_row[lane] = r;
            sh_truth[lane] = tr;
            no_label += (int)__popcll(__ballot(i < n && !labelled));
        }
        __syncthreads();
        uint32_t b[RK_TILE / 4], w[RK_TILE / 4];
#pragma unroll
        for (int q = 0; q < RK_TILE / 4; q++) {
            const int r = sh_row[wave + 4 * q];
            const bool live = r >= 0 && c < c1;
            b[q] = live ? __float_as_uint(table[(size_t)r * ld + c]) : 0u;
            w[q] = live && truth_bits ? truth_bits[(size_t)r * wpr + (c >> 5)] : 0u;
        }
#pragma unroll
        for (int q = 0; q < RK_TILE / 4; q++) {
            const int rr = wave + 4 * q;
            uint32_t k = RANK_SENTINEL;
            int ct = RK_NONE;
            if (sh_row[rr] >= 0 && c < c1) {
                const bool is_pos = truth ? sh_truth[rr] == c : ((w[q] >> (c & 31)) & 1u) != 0u;
                if ((b[q] & 0x7FFFFFFFu) > 0x7F800000u) {
                    ct = RK_INVALID;
                } else {
                    k = rank_key(b[q]);
                    ct = is_pos ? RK_POS : RK_NEG;
                }
            }
            key[rr][lane] = k;
            cat[rr][lane] = (uint8_t)ct;
        }
        __syncthreads();
        for (int cc = wave; cc < RK_TILE && cb + cc < c1; cc += 4) {
            const int i = i0 + lane;
            const uint32_t k = key[lane][cc];
            const int ct = cat[lane][cc];
            const int np = (int)__popcll(__ballot(ct == RK_POS)), nn = (int)__popcll(__ballot(ct == RK_NEG));
            const int ni = (int)__popcll(__ballot(ct == RK_INVALID));
            if (i < n) {
                const size_t at = (size_t)(cb + cc - c0) * (size_t)stride + (size_t)i;
                pos_keys[at] = ct == RK_POS ? k : RANK_SENTINEL;
                neg_keys[at] = ct == RK_NEG ? k : RANK_SENTINEL;
            }
            if (lane == 0) {                                   // class cc is this wave's in every tile
                sh_count[0][cc] += np;
                sh_count[1][cc] += nn;
                sh_count[2][cc] += ni;
            }
        }
        __syncthreads();                                       // the tile is read: the next one may be written
    }
    if (unlabelled && blockIdx.y == 0 && wave == 0 && lane == 0 && no_label) atomicAdd(unlabelled, no_label);
    if (wave < 3 && c < c1) {
        const int v = sh_count[wave][lane];
        int32_t *out = wave == 0 ? pos : (wave == 1 ? neg : invalid);
        if (v) atomicAdd(&out[c - c0], v);
    }
}

// ---- statistics ------------------------------------------------------------------------------------------------------------
// grid (GCNHIP_RANK_STATS_BLOCKS, S): block bx of class c takes the positives bx . 256 + t, + blocks . 256, ...
__global__ __launch_bounds__(256) void rank_stats_kernel(const uint32_t *__restrict__ pos_keys, const uint32_t *__restrict__ neg_keys, int64_t stride,
                                                         int n, const int32_t *__restrict__ pos, const int32_t *__restrict__ neg,
                                                         double *__restrict__ part_ap, long long *__restrict__ part_u2) {
    __shared__ double sh_ap[4];
    __shared__ long long sh_u2[4];
    const int c = blockIdx.y, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    int P = pos[c], N = neg[c];
    P = P < 0 ? 0 : (P > n ? n : P);                           // the valid lengths come from the counts; no count can index past a column
    N = N < 0 ? 0 : (N > n ? n : N);
    const uint32_t *pk = pos_keys + (size_t)c * (size_t)stride, *nk = neg_keys + (size_t)c * (size_t)stride;
    double ap = 0.0;
    long long u2 = 0;
    for (int i = blockIdx.x * 256 + t; i < P; i += gridDim.x * 256) {
        const uint32_t k = pk[i];
        const int lt = rank_lower_bound(nk, N, k), le = rank_upper_bound(nk, N, k);
        const int tp = P - rank_lower_bound(pk, P, k), fp = N - lt;
        u2 += (long long)lt + (long long)le;
        ap += (double)tp / (double)(tp + fp);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        ap += __shfl_xor(ap, off, WAVE);
        u2 += __shfl_xor(u2, off, WAVE);
    }
    if (lane == 0) { sh_ap[wave] = ap; sh_u2[wave] = u2; }
    __syncthreads();
    if (t == 0) {
        part_ap[(size_t)c * gridDim.x + blockIdx.x] = ((sh_ap[0] + sh_ap[1]) + sh_ap[2]) + sh_ap[3];
        part_u2[(size_t)c * gridDim.x + blockIdx.x] = sh_u2[0] + sh_u2[1] + sh_u2[2] + sh_u2[3];
    }
}
// a thread per class: the block partials in block order
__global__ __launch_bounds__(256) void rank_stats_fold_kernel(const double *__restrict__ part_ap, const long long *__restrict__ part_u2, int S, int blocks,
                                                              long long *__restrict__ u2, double *__restrict__ ap_sum) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= S) return;
    double a = 0.0;
    long long u = 0;
    for (int b = 0; b < blocks; b++) {
        a += part_ap[(size_t)c * blocks + b];
        u += part_u2[(size_t)c * blocks + b];
    }
    u2[c] = u;
    ap_sum[c] = a;
}

extern "C" {

int gcnhip_sort_tile(void) { return SORT_TILE; }

int gcnhip_rank_keys(gcnhip_ctx *c, const float *table, int ld, int n_table, const int32_t *d_rows, int n, int c0, int c1, int num_classes,
                     const int32_t *truth, const uint32_t *truth_bits, int words_per_row, uint32_t *pos_keys, uint32_t *neg_keys, int64_t stride,
                     int32_t *d_pos, int32_t *d_neg, int32_t *d_invalid, int32_t *d_unlabelled) {
    if (!c || !table || !pos_keys || !neg_keys || !d_pos || !d_neg || !d_invalid) return gcnhip_fail("gcnhip_rank_keys: invalid argument");
    if (n_table < 0 || n < 0 || n > SORT_N_MAX) return gcnhip_fail("gcnhip_rank_keys: 0 <= n <= 2^24 listed rows");
    if (num_classes < 1 || c0 < 0 || c1 <= c0 || c1 > num_classes) return gcnhip_fail("gcnhip_rank_keys: the class range must be 0 <= c0 < c1 <= num_classes");
    if (ld < num_classes) return gcnhip_fail("gcnhip_rank_keys: the row stride is below num_classes");
    if ((truth != nullptr) == (truth_bits != nullptr)) return gcnhip_fail("gcnhip_rank_keys: give either int32 truth or truth bit rows");
    if (truth_bits && words_per_row < (num_classes + 31) / 32) return gcnhip_fail("gcnhip_rank_keys: words_per_row is below ceil(num_classes / 32)");
    if (stride < n || stride < 1) return gcnhip_fail("gcnhip_rank_keys: the column stride must be at least max(n, 1)");
    if (!d_rows && n > n_table) return gcnhip_fail("gcnhip_rank_keys: without a row list n is at most n_table");
    const size_t cells = (size_t)(c1 - c0) * sizeof(int32_t);
    GCNHIP_TRY(hipMemsetAsync(d_pos, 0, cells, c->stream));
    GCNHIP_TRY(hipMemsetAsync(d_neg, 0, cells, c->stream));
    GCNHIP_TRY(hipMemsetAsync(d_invalid, 0, cells, c->stream));
    if (d_unlabelled) GCNHIP_TRY(hipMemsetAsync(d_unlabelled, 0, sizeof(int32_t), c->stream));
    if (n == 0) return 0;
    const dim3 grid((unsigned)std::min(ceil_div(n, RK_TILE), RK_MAX_BLOCKS), (unsigned)ceil_div(c1 - c0, RK_TILE));
    rank_keys_kernel<<<grid, 256, 0, c->stream>>>(table, ld, n_table, d_rows, n, c0, c1, num_classes, truth, truth_bits, words_per_row, pos_keys, neg_keys,
                                                  stride, d_pos, d_neg, d_invalid, d_unlabelled);
    GCNHIP_LAUNCH_CHECK();
    return 0;
}

int gcnhip_sort_segments_u32(gcnhip_ctx *c, uint32_t *keys, uint32_t *scratch, int n, int segments, int64_t stride) {
    if (!c || !keys) return gcnhip_fail("gcnhip_sort_segments_u32: invalid argument");
    if (n < 0 || n > SORT_N_MAX) return gcnhip_fail("gcnhip_sort_segments_u32: 0 <= n <= 2^24 keys per segment");
    if (segments < 1) return gcnhip_fail("gcnhip_sort_segments_u32: at least one segment");
    if (stride < n) return gcnhip_fail("gcnhip_sort_segments_u32: the segment stride is below n");
    if (n == 0) return 0;
    const int tiles = ceil_div(n, SORT_TILE);
    if ((int64_t)tiles * segments > 0x7FFFFFFF) return gcnhip_fail("gcnhip_sort_segments_u32: more than 2^31 - 1 tiles in one call");
    int passes = 0;
    for (int64_t L = SORT_TILE; L < n; L *= 2) passes++;
    if (passes && (!scratch || scratch == keys)) return gcnhip_fail("gcnhip_sort_segments_u32: more than one tile per segment needs a scratch table");
    const unsigned grid = (unsigned)(tiles * segments);
    // an odd number of passes starts in the scratch, so that the last pass lands in keys
    uint32_t *cur = (passes & 1) ? scratch : keys;
    sort_tiles_kernel<<<grid, SORT_THREADS, 0, c->stream>>>(keys, cur, n, stride, tiles);
    GCNHIP_LAUNCH_CHECK();
    for (int L = SORT_TILE; L < n; L *= 2) {
        uint32_t *other = cur == keys ? scratch : keys;
        sort_merge_kernel<<<grid, SORT_THREADS, 0, c->stream>>>(cur, other, n, stride, tiles, L);
        GCNHIP_LAUNCH_CHECK();
        cur = other;
    }
    return 0;
}

int gcnhip_rank_stats(gcnhip_ctx *c, const uint32_t *pos_keys, const uint32_t *neg_keys, int64_t stride, int n, int segments, const int32_t *d_pos,
                      const int32_t *d_neg, void *d_work, int64_t *d_u2, double *d_ap_sum) {
    if (!c || !pos_keys || !neg_keys || !d_pos || !d_neg || !d_work || !d_u2 || !d_ap_sum) return gcnhip_fail("gcnhip_rank_stats: invalid argument");
    if (n < 0 || n > SORT_N_MAX) return gcnhip_fail("gcnhip_rank_stats: 0 <= n <= 2^24 keys per class");
    if (segments < 1 || segments > 65535) return gcnhip_fail("gcnhip_rank_stats: 1 <= classes <= 65535");
    if (stride < n || stride < 1) return gcnhip_fail("gcnhip_rank_stats: the column stride must be at least max(n, 1)");
    if (((uintptr_t)d_work & 7) != 0) return gcnhip_fail("gcnhip_rank_stats: the work block must be 8-byte aligned");
    double *part_ap = (double *)d_work;
    long long *part_u2 = (long long *)(part_ap + (size_t)segments * GCNHIP_RANK_STATS_BLOCKS);
    rank_stats_kernel<<<dim3(GCNHIP_RANK_STATS_BLOCKS, (unsigned)segments), 256, 0, c->stream>>>(pos_keys, neg_keys, stride, n, d_pos, d_neg, part_ap, part_u2);
    GCNHIP_LAUNCH_CHECK();
    rank_stats_fold_kernel<<<ceil_div(segments, 256), 256, 0, c->stream>>>(part_ap, part_u2, segments, GCNHIP_RANK_STATS_BLOCKS, (long long *)d_u2, d_ap_sum);
    GCNHIP_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
