// dbscan.hip — DBSCAN of a table's rows (Ester, Kriegel, Sander & Xu, 1996; scikit-learn's DBSCAN labels, element for element),
// matrix-free: no n x n distance or adjacency is ever stored, every pass recomputes d2 on the exact-f32 MFMA and keeps only integers.
// Beyond the reference, which never looks at its hidden matrix.  include/gcnhip_driver.h has the definitions.
//
// The rows are the pack gcnhip_tsne_pack makes (tsne_pack.h: contiguous zero-padded x^, xn, which positions are points).  The
// relation d2(i, j) <= eps2 is symmetric, so ONE walk body goes over the tile PAIRS (I <= J) of 64 positions and uses every entry
// for both of its ends: half the products of a square walk.  Integer atomics only; no allocation, no synchronisation.
//
// dbscan_walk_kernel<DP, MODE>   workgroup w of ceil(T / 2) owns row tile w (T - w column tiles) and then row tile T - 1 - w (w + 1
//   column tiles): T + 1 tile pairs each, so the triangle leaves no workgroup idle.  Four waves, wave v owns rows 16v .. 16v + 15.
//   The x^ of the row tile live in REGISTERS (DP / 4 VGPRs per lane: the B operand of lane (l15, kg) of v_mfma_f32_16x16x4_f32), LDS
//   holds TWO column tiles of 64 x (DP + 4) floats with their scalars; the global loads of tile t + 1 are issued into registers
//   before the products of tile t and stored to the other buffer behind them: one barrier per tile.  The 64 x 64 d2 tile lives in
//   accumulators.  In the diagonal tile an entry counts only with column >= row (COUNT) or column > row (LINK).
//     COUNT  E compares per entry.  A row's hits add up in the lane's registers through the whole row of tiles and leave as one
//            atomicAdd per row and radius.  A column's hits are the mirrored half: the compare's wave mask IS the ballot, a popcount
//            of its 16-bit field gives the column's hits among the wave's 16 rows, four radii packed to a word; the four waves' words
//            meet in LDS and leave as one atomicAdd per column, radius and tile pair.
//     LINK   one round of hooking plus the border rule.  Two neighbouring core points whose roots differ: atomicMin of the smaller
//            root into the larger root's hook slot, and the round's flag.  A core and a non-core neighbour: the core's root into the
//            other's border slot (the row side keeps its minimum in a register until the row tile ends).  Reads comp, writes hook:
//            what a round computes does not depend on the order in which workgroups run.  A tile pair without a core point on
//            either side is skipped.
// dbscan_prep_kernel  the start of a round: a core point follows the hooks from its root to the root that has none (hooks only ever
//   point to a smaller position), border slots are reset.  dbscan_core_kernel: the core flags, a tile's core count, comp = hook = i.
// dbscan_rank_kernel  one workgroup: an exclusive scan of the roots over positions.  dbscan_label_kernel: labels, sizes, totals.
#include "bucket.h"
#include "tsne_pack.h"
#include <climits>
#include <cmath>
#include <cstdio>

using f32x4 = __attribute__((ext_vector_type(4))) float;

constexpr int DB_MAX_E = 8;
constexpr int DB_T = 64;                          // positions per tile, rows and columns alike
enum { DB_COUNT = 0, DB_LINK = 1 };

struct DbEps {
    float e2[DB_MAX_E];
    int n;
};
struct DbState {                                  // int32 [n_pad] each, then ncore [tiles]
    int32_t *comp, *hook, *border, *core, *rank, *ncore;
    size_t bytes;
};
static DbState db_state(void *state, int n) {
    const size_t n_pad = (size_t)ts_npad(n);
    int32_t *b = (int32_t *)state;
    DbState s;
    s.comp = b; s.hook = b + n_pad; s.border = b + 2 * n_pad; s.core = b + 3 * n_pad; s.rank = b + 4 * n_pad; s.ncore = b + 5 * n_pad;
    s.bytes = (5 * n_pad + n_pad / DB_T) * sizeof(int32_t);
    return s;
}

template <int DP>
struct DbTile {                                                 // what a thread holds of a column tile between its loads and its LDS stores
    f32x4 x[DP / 16];
    int4 s;                                                     // {xn bits, a point, a core point, comp}
};

template <int DP, int MODE>
__device__ __forceinline__ void db_tile_load(DbTile<DP> &T, const float *__restrict__ X, const float4 *__restrict__ S, const int32_t *__restrict__ valid,
                                             const DbState &st, int c0) {
    const f32x4 *src = (const f32x4 *)(X + (size_t)c0 * DP);    // the tile is 64 . DP contiguous floats
#pragma unroll
    for (int u = 0; u < DP / 16; u++) T.x[u] = src[threadIdx.x + 256 * u];
    if (threadIdx.x < DB_T) {
        const int col = c0 + threadIdx.x;                       // col < n_pad; a padding position is no point
        T.s = make_int4(__float_as_int(S[col].x), valid[col], MODE == DB_LINK ? st.core[col] : 0, MODE == DB_LINK ? st.comp[col] : 0);
    }
}

template <int DP>
__device__ __forceinline__ void db_tile_store(const DbTile<DP> &T, float *__restrict__ Cs, int4 *__restrict__ Is) {
    constexpr int QLD = DP + 4;
#pragma unroll
    for (int u = 0; u < DP / 16; u++) {
        const int idx = threadIdx.x + 256 * u, row = idx / (DP / 4), c4 = idx % (DP / 4);
        *(f32x4 *)(Cs + row * QLD + 4 * c4) = T.x[u];
    }
    if (threadIdx.x < DB_T) Is[threadIdx.x] = T.s;
}

// grid ceil(T / 2).  COUNT: count [E x n], zeroed before the launch.  LINK: st and *changed.
template <int DP, int MODE>
__global__ __launch_bounds__(256) void dbscan_walk_kernel(const float *__restrict__ X, const float4 *__restrict__ S, const int32_t *__restrict__ valid,
                                                          int n, int T, DbEps eps, int32_t *__restrict__ count, DbState st,
                                                          int32_t *__restrict__ changed) {
    extern __shared__ __align__(16) unsigned char smem[];
    constexpr int QLD = DP + 4, NCH = DP / 16;
    float *Cs = (float *)smem;                                  // [2][64][QLD]
    int4 *Is = (int4 *)(Cs + 2 * DB_T * QLD);                   // [2][64]
    int32_t *colred = (int32_t *)(Is + 2 * DB_T);               // [2][2 words][4 waves][64]: a column's hits per wave, a byte per radius
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int kg = lane >> 4, l15 = lane & 15;
    int flag = 0;

    for (int pass = 0; pass < 2; pass++) {
        const int I = pass ? T - 1 - (int)blockIdx.x : (int)blockIdx.x;
        if (pass && I == (int)blockIdx.x) break;                // an odd T: the middle tile has no partner
        const int i = I * DB_T + 16 * wave + l15;
        f32x4 b[NCH];                                           // the row operand: x^_i[16c + 4kg .. + 3]
#pragma unroll
        for (int c = 0; c < NCH; c++) b[c] = *(const f32x4 *)(X + (size_t)i * DP + 16 * c + 4 * kg);
        const float xi = S[i].x;
        const bool vi = valid[i] != 0;
        const bool ci = MODE == DB_LINK && st.core[i] != 0;
        const int pi = MODE == DB_LINK ? st.comp[i] : 0;
        const int cores_i = MODE == DB_LINK ? st.ncore[I] : 1;
        int rowcnt[DB_MAX_E] = {};
        int bmin = INT_MAX;
        const int n_tiles = T - I;

        DbTile<DP> Tl;
        db_tile_load<DP, MODE>(Tl, X, S, valid, st, I * DB_T);
        db_tile_store<DP>(Tl, Cs, Is);
        __syncthreads();
        for (int t = 0; t < n_tiles; t++) {
            const int buf = t & 1, J = I + t, c0 = J * DB_T;
            const bool diag = t == 0;
            if (t + 1 < n_tiles) db_tile_load<DP, MODE>(Tl, X, S, valid, st, c0 + DB_T);      // in flight across the products below
            const float *C = Cs + buf * DB_T * QLD;
            const int4 *Ic = Is + buf * DB_T;
            if (MODE == DB_COUNT || cores_i + st.ncore[J] > 0) {                            // the same for every thread of the workgroup
                f32x4 acc[4] = {};
#pragma unroll
                for (int c = 0; c < NCH; c++) {
                    f32x4 a[4];
#pragma unroll
                    for (int g = 0; g < 4; g++) a[g] = *(const f32x4 *)(C + (16 * g + l15) * QLD + 16 * c + 4 * kg);
#pragma unroll
                    for (int s = 0; s < 4; s++)
#pragma unroll
                        for (int g = 0; g < 4; g++) acc[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[g][s], b[c][s], acc[g], 0, 0, 0);
                }
                unsigned mine[2] = {0u, 0u};
#pragma unroll
                for (int g = 0; g < 4; g++)
#pragma unroll
                    for (int r = 0; r < 4; r++) {               // D[row 4kg + r][col l15]: column 16g + 4kg + r of the tile, this lane's row
                        const int cc = 16 * g + 4 * kg + r, j = c0 + cc;
                        const int4 sj = Ic[cc];
                        const float d2 = fmaxf((xi + __int_as_float(sj.x)) - 2.f * acc[g][r], 0.f);
                        if (MODE == DB_COUNT) {
                            const bool ok = vi && sj.y != 0 && (!diag || j >= i);
                            unsigned word[2] = {0u, 0u};
#pragma unroll
                            for (int e = 0; e < DB_MAX_E; e++)
                                if (e < eps.n) {
                                    const bool hit = ok && d2 <= eps.e2[e];
                                    rowcnt[e] += hit ? 1 : 0;   // the self pair counts once, here
                                    const unsigned long long m = __ballot(hit && j != i);
                                    const unsigned half = kg & 2 ? (unsigned)(m >> 32) : (unsigned)m;
                                    word[e >> 2] |= (unsigned)__popc((half >> (16 * (kg & 1))) & 0xffffu) << (8 * (e & 3));
                                }
                            if (l15 == 4 * g + r) { mine[0] = word[0]; mine[1] = word[1]; }
                        } else {
                            const bool near = vi && sj.y != 0 && (!diag || j > i) && d2 <= eps.e2[0];
                            if (near) {
                                const bool cj = sj.z != 0;
                                const int pj = sj.w;
                                if (ci && cj) {
                                    if (pi != pj) {
                                        atomicMin(&st.hook[max(pi, pj)], min(pi, pj));
                                        flag = 1;
                                    }
                                } else if (ci) {
                                    atomicMin(&st.border[j], pi);
                                } else if (cj) {
                                    bmin = min(bmin, pj);
                                }
                            }
                        }
                    }
                if (MODE == DB_COUNT) {                         // lane (kg, l15) keeps column 16 (l15 / 4) + 4 kg + l15 % 4 of its wave's 16 rows
                    const int cc = 16 * (l15 >> 2) + 4 * kg + (l15 & 3);
                    colred[((buf * 2 + 0) * 4 + wave) * DB_T + cc] = (int32_t)mine[0];
                    colred[((buf * 2 + 1) * 4 + wave) * DB_T + cc] = (int32_t)mine[1];
                }
            }
            if (t + 1 < n_tiles) db_tile_store<DP>(Tl, Cs + (buf ^ 1) * DB_T * QLD, Is + (buf ^ 1) * DB_T);
            __syncthreads();                                    // tile t is done with, tile t + 1 and the column words of t are in place
            if (MODE == DB_COUNT && threadIdx.x < 2 * DB_T) {   // read before the next barrier; tile t + 1 writes the other half
                const int wsel = threadIdx.x >> 6, cc = threadIdx.x & 63, j = c0 + cc;
                unsigned v = 0;                                 // a byte holds at most 4 x 16 hits
#pragma unroll
                for (int w = 0; w < 4; w++) v += (unsigned)colred[((buf * 2 + wsel) * 4 + w) * DB_T + cc];
                if (v && j < n)
#pragma unroll
                    for (int q = 0; q < 4; q++) {
                        const int e = 4 * wsel + q, hits = (int)((v >> (8 * q)) & 0xffu);
                        if (e < eps.n && hits) atomicAdd(&count[(size_t)e * n + j], hits);
                    }
            }
        }
        if (MODE == DB_COUNT) {
#pragma unroll
            for (int e = 0; e < DB_MAX_E; e++)
                if (e < eps.n) {
                    int tot = rowcnt[e];
                    tot += __shfl_xor(tot, 16, WAVE);
                    tot += __shfl_xor(tot, 32, WAVE);
                    if (kg == 0 && i < n && tot) atomicAdd(&count[(size_t)e * n + i], tot);
                }
        } else {
            bmin = min(bmin, __shfl_xor(bmin, 16, WAVE));
            bmin = min(bmin, __shfl_xor(bmin, 32, WAVE));
            if (kg == 0 && bmin != INT_MAX) atomicMin(&st.border[i], bmin);
        }
    }
    if (MODE == DB_LINK && flag) atomicOr(changed, 1);
}

__global__ __launch_bounds__(256) void dbscan_zero_kernel(int32_t *__restrict__ p, size_t total) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e < total) p[e] = 0;
}

// a wave per tile: core flags, the tile's core count, every position its own root
__global__ __launch_bounds__(64) void dbscan_core_kernel(const int32_t *__restrict__ valid, const int32_t *__restrict__ count, int n, int min_samples,
                                                         DbState st) {
    const int i = blockIdx.x * DB_T + threadIdx.x;
    const bool c = i < n && valid[i] != 0 && count[i] >= min_samples;
    st.core[i] = c;
    st.comp[i] = i;
    st.hook[i] = i;
    st.border[i] = INT_MAX;
    const unsigned long long m = __ballot(c);
    if (threadIdx.x == 0) st.ncore[blockIdx.x] = __popcll(m);
}

// the start of a round: comp follows last round's hooks to the root that has none; the border slots and the flag are reset
__global__ __launch_bounds__(256) void dbscan_prep_kernel(int n_pad, DbState st, int32_t *__restrict__ changed) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i == 0) *changed = 0;
    if (i >= n_pad) return;
    if (st.core[i]) {
        int r = st.comp[i];
        for (int h = st.hook[r]; h != r; h = st.hook[r]) r = h; // strictly descending: it ends
        st.comp[i] = r;
    }
    st.border[i] = INT_MAX;
}

// one workgroup: rank[i] = the roots at positions below i; sizes zeroed; counts = {points, core, 0, 0, clusters}
__global__ __launch_bounds__(1024) void dbscan_rank_kernel(const int32_t *__restrict__ valid, int n, DbState st, int32_t *__restrict__ sizes,
                                                           int32_t *__restrict__ counts) {
    __shared__ int scan[1024], tot[2][1024];
    const int t = threadIdx.x, chunk = (n + 1023) / 1024, lo = min(t * chunk, n), hi = min(lo + chunk, n);
    int roots = 0, cores = 0, points = 0;
    for (int i = lo; i < hi; i++) {
        const bool c = st.core[i] != 0;
        roots += c && st.comp[i] == i;
        cores += c;
        points += valid[i] != 0;
        sizes[i] = 0;
    }
    scan[t] = roots; tot[0][t] = cores; tot[1][t] = points;
    __syncthreads();
    for (int w = 1; w < 1024; w <<= 1) {                        // inclusive scan of the roots; plain sums of the other two
        const int v = t >= w ? scan[t - w] : 0;
        __syncthreads();
        scan[t] += v;
        __syncthreads();
    }
    for (int w = 512; w > 0; w >>= 1) {
        if (t < w) { tot[0][t] += tot[0][t + w]; tot[1][t] += tot[1][t + w]; }
        __syncthreads();
    }
    int run = scan[t] - roots;
    for (int i = lo; i < hi; i++) {
        st.rank[i] = run;
        run += st.core[i] != 0 && st.comp[i] == i;
    }
    if (t == 0) { counts[0] = tot[1][0]; counts[1] = tot[0][0]; counts[2] = 0; counts[3] = 0; counts[4] = scan[1023]; }
}

__global__ __launch_bounds__(256) void dbscan_label_kernel(const int32_t *__restrict__ valid, int n, DbState st, int32_t *__restrict__ labels,
                                                           uint8_t *__restrict__ core, int32_t *__restrict__ sizes, int32_t *__restrict__ counts) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    int lab = -1;
    bool is_core = false, is_border = false, is_noise = false;
    if (i < n && valid[i] != 0) {
        is_core = st.core[i] != 0;
        const int root = is_core ? st.comp[i] : st.border[i];
        is_border = !is_core && root != INT_MAX;
        is_noise = !is_core && !is_border;
        if (!is_noise) lab = st.rank[root];
    }
    if (i < n) {
        labels[i] = lab;
        core[i] = is_core;
        if (lab >= 0) atomicAdd(&sizes[lab], 1);
    }
    const int nb = __popcll(__ballot(is_border)), nn = __popcll(__ballot(is_noise));
    if ((threadIdx.x & 63) == 0) {
        if (nb) atomicAdd(&counts[2], nb);
        if (nn) atomicAdd(&counts[3], nn);
    }
}

// ---- entry points ------------------------------------------------------------------------------------------------------------

template <int DP, int MODE>
static int db_walk_launch(gcnhip_ctx *c, const TsPack &P, int n, const DbEps &eps, int32_t *count, const DbState &st, int32_t *changed) {
    const size_t lds = sizeof(float) * (size_t)(2 * DB_T * (DP + 4)) + 2 * DB_T * sizeof(int4) + 2 * 2 * 4 * DB_T * sizeof(int32_t);
    auto kern = dbscan_walk_kernel<DP, MODE>;
    if (lds > 64 * 1024) GCNHIP_TRY(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    const int T = ts_npad(n) / DB_T;
    kern<<<(T + 1) / 2, 256, lds, c->stream>>>(P.X, P.S, P.valid, n, T, eps, count, st, changed);
    GCNHIP_LAUNCH_CHECK();
    return 0;
}
template <int MODE, typename... A>
static int db_walk(int dp, A... a) {
    switch (dp) {
    case 16: return db_walk_launch<16, MODE>(a...);
    case 32: return db_walk_launch<32, MODE>(a...);
    case 64: return db_walk_launch<64, MODE>(a...);
    case 128: return db_walk_launch<128, MODE>(a...);
    default: return db_walk_launch<256, MODE>(a...);
    }
}

static bool db_eps(const double *eps, int n_eps, DbEps &out) {
    out.n = n_eps;
    for (int e = 0; e < DB_MAX_E; e++) out.e2[e] = -1.f;
    for (int e = 0; e < n_eps; e++) {
        if (!(eps[e] > 0.0) || !std::isfinite(eps[e]) || !std::isfinite((float)(eps[e] * eps[e]))) return false;
        out.e2[e] = (float)(eps[e] * eps[e]);                   // the product in double, rounded once
    }
    return true;
}

static const char *db_common(const gcnhip_ctx *c, const void *pack, int n, int dim) {
    if (!c || !pack || n < 1) return "invalid argument";
    if (dim < 1 || dim > TS_MAX_DIM) return "1 <= dim <= 256";
    if (!aligned16(pack)) return "the pack is not 16-byte aligned";
    return nullptr;
}
#define DB_REFUSE(name, why) return gcnhip_fail(name ": " why)
#define DB_COMMON(name)                                                          \
    if (const char *why = db_common(c, pack, n, dim)) {                          \
        static thread_local char msg[160];                                       \
        snprintf(msg, sizeof msg, "%s: %s", name, why);                          \
        return gcnhip_fail(msg);                                                 \
    }

extern "C" {

int gcnhip_dbscan_plan(int n, int dim, size_t *pack_bytes, size_t *state_bytes) {
    if (n < 0 || dim < 1 || dim > TS_MAX_DIM) DB_REFUSE("gcnhip_dbscan_plan", "invalid argument (n >= 0, 1 <= dim <= 256)");
    if (pack_bytes) *pack_bytes = ts_pack(nullptr, n, dim).bytes;
    if (state_bytes) *state_bytes = db_state(nullptr, n).bytes;
    return 0;
}

int gcnhip_dbscan_counts(gcnhip_ctx *c, const void *pack, int n, int dim, const double *eps, int n_eps, int32_t *count) {
    DB_COMMON("gcnhip_dbscan_counts")
    if (!eps || !count) DB_REFUSE("gcnhip_dbscan_counts", "invalid argument");
    if (n_eps < 1 || n_eps > DB_MAX_E) DB_REFUSE("gcnhip_dbscan_counts", "1 <= E <= 8 radii");
    DbEps e;
    if (!db_eps(eps, n_eps, e)) DB_REFUSE("gcnhip_dbscan_counts", "eps must be finite and above 0");
    const size_t total = (size_t)n_eps * (size_t)n;
    dbscan_zero_kernel<<<ceil_div((int64_t)total, 256), 256, 0, c->stream>>>(count, total);
    GCNHIP_LAUNCH_CHECK();
    return db_walk<DB_COUNT>(ts_dp(dim), c, ts_pack((void *)pack, n, dim), n, e, count, DbState{}, (int32_t *)nullptr);
}

int gcnhip_dbscan_cores(gcnhip_ctx *c, const void *pack, int n, int dim, const int32_t *count, int min_samples, void *state, size_t state_bytes) {
    DB_COMMON("gcnhip_dbscan_cores")
    if (!count || !state) DB_REFUSE("gcnhip_dbscan_cores", "invalid argument");
    if (min_samples < 1) DB_REFUSE("gcnhip_dbscan_cores", "min_samples must be at least 1");
    const DbState st = db_state(state, n);
    if (state_bytes < st.bytes) DB_REFUSE("gcnhip_dbscan_cores", "the state is too small (gcnhip_dbscan_plan tells the bytes)");
    dbscan_core_kernel<<<ts_npad(n) / DB_T, DB_T, 0, c->stream>>>(ts_pack((void *)pack, n, dim).valid, count, n, min_samples, st);
    GCNHIP_LAUNCH_CHECK();
    return 0;
}

int gcnhip_dbscan_link(gcnhip_ctx *c, const void *pack, int n, int dim, double eps, void *state, size_t state_bytes, int32_t *changed) {
    DB_COMMON("gcnhip_dbscan_link")
    if (!state || !changed) DB_REFUSE("gcnhip_dbscan_link", "invalid argument");
    DbEps e;
    if (!db_eps(&eps, 1, e)) DB_REFUSE("gcnhip_dbscan_link", "eps must be finite and above 0");
    const DbState st = db_state(state, n);
    if (state_bytes < st.bytes) DB_REFUSE("gcnhip_dbscan_link", "the state is too small (gcnhip_dbscan_plan tells the bytes)");
    const int n_pad = ts_npad(n);
    dbscan_prep_kernel<<<ceil_div(n_pad, 256), 256, 0, c->stream>>>(n_pad, st, changed);
    GCNHIP_LAUNCH_CHECK();
    return db_walk<DB_LINK>(ts_dp(dim), c, ts_pack((void *)pack, n, dim), n, e, (int32_t *)nullptr, st, changed);
}

int gcnhip_dbscan_labels(gcnhip_ctx *c, const void *pack, int n, int dim, const void *state, size_t state_bytes, int32_t *labels, uint8_t *core,
                         int32_t *sizes, int32_t *counts) {
    DB_COMMON("gcnhip_dbscan_labels")
    if (!state || !labels || !core || !sizes || !counts) DB_REFUSE("gcnhip_dbscan_labels", "invalid argument");
    const DbState st = db_state((void *)state, n);
    if (state_bytes < st.bytes) DB_REFUSE("gcnhip_dbscan_labels", "the state is too small (gcnhip_dbscan_plan tells the bytes)");
    const int32_t *valid = ts_pack((void *)pack, n, dim).valid;
    dbscan_rank_kernel<<<1, 1024, 0, c->stream>>>(valid, n, st, sizes, counts);
    GCNHIP_LAUNCH_CHECK();
    dbscan_label_kernel<<<ceil_div(n, 256), 256, 0, c->stream>>>(valid, n, st, labels, core, sizes, counts);
    GCNHIP_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
