// hdbscan.hip — the minimum spanning tree of a table's rows under HDBSCAN's mutual-reachability distance (Campello, Moulavi & Sander,
// 2013; scikit-learn's HDBSCAN), by Boruvka rounds and matrix-free: the n (n - 1) / 2 edge weights of the complete graph are never
// stored, every round recomputes d2 on the exact-f32 MFMA and keeps only integer keys.  Beyond the reference, which has no such
// query.  include/gcnhip_driver.h has the definitions; host/hdbscan.cpp derives the clusters from the tree without a GPU.
//
// The rows are the pack gcnhip_tsne_pack makes (tsne_pack.h).  w(i, j) = max(d2(i, j), core2[i], core2[j]) with d2 formed as
// dbscan.hip forms it; an edge's key is (bits of w, lo, hi) on list positions, a strict total order that looks the same from both
// ends because each unordered pair is evaluated ONCE, with the larger position as the column.
//
// hdbscan_nearest_kernel<DP>   one launch is one Boruvka round's search.  DBSCAN's triangle geometry: workgroup w of ceil(T / 2) owns
//   row tile w and then row tile T - 1 - w, four waves own 16 rows each with the row operand in registers, column tiles of 64 x
//   (DP + 4) floats alternate in LDS with their scalars {xn, a point, core2 bits, comp}; the loads of tile t + 1 are in flight
//   across the products of tile t, one barrier per tile.  An entry (i, j) whose ends are points of different components (j > i in
//   the diagonal tile) is a candidate for BOTH ends:
//     row side     the lane's running best key (w bits << 32 | j) stays in registers through the whole row of tiles, is reduced over
//                  the four kg lane groups by two shuffles per word and leaves as ONE u64 atomicMin per row and row tile.
//     column side  a per-column best (w bits << 32 | i) in LDS, [2][64] u64, reset when its tile is stored.  An entry first READS
//                  the column's best (the 16 lanes of a kg group read one address) and issues the LDS atomicMin only when it beats
//                  it; a stale read costs one atomic more, never a wrong minimum.  After the tile's barrier a column that improved
//                  sends one global atomicMin.
//   A tile pair whose two tiles lie in one and the same component, or one of which holds no point, is skipped: the per-tile
//   {min comp, max comp} is refreshed by the merge.  That is what makes the last rounds cheap.
//   Reads comp, writes best: integer atomicMin only, what a round computes does not depend on the order the workgroups run in.
// hdbscan_pick_kernel    every point sends its best edge, as (w bits << 32 | lo << 16 | hi), to its root's slot with a u64 atomicMin:
//   positions are below 65 536.  For a fixed end the order by (w, other end) IS the order by (w, lo, hi), so the root's minimum is the
//   component's lightest outgoing edge under the full order.
// hdbscan_hook_kernel    a root with a chosen edge finds the root at the other end.  Two roots that chose each other chose the same
//   key: the smaller root emits the edge and stays, the larger hangs under it.  Every other root emits its edge and hangs under the
//   other.  Under a strict order the hooks form trees with exactly that one pair at the top, so following them ends.
// hdbscan_jump_kernel    a wave per tile: comp follows the hooks to their end; best and root slots are reset; the tile's {min, max}
//   comp; the round's counts {components, edges}.
#include "bucket.h"
#include "tsne_pack.h"
#include <climits>
#include <cstdio>

using f32x4 = __attribute__((ext_vector_type(4))) float;
using u64 = unsigned long long;

constexpr int HD_T = 64;                          // positions per tile, rows and columns alike
constexpr int HD_MAX_N = 65536;                   // lo and hi take 16 bits each of a root's key
constexpr u64 HD_NONE = ~0ull;

struct HdState {                                  // u64 best, pick [n_pad]; int32 comp, hook, core2 [n_pad]; tile [2 x tiles]; edges [8]
    u64 *best, *pick;
    int32_t *comp, *hook, *core2, *tile, *edges;
    size_t bytes;
};
static HdState hd_state(void *state, int n) {
    const size_t n_pad = (size_t)ts_npad(n), T = n_pad / HD_T;
    HdState s;
    s.best = (u64 *)state; s.pick = s.best + n_pad;
    s.comp = (int32_t *)(s.pick + n_pad); s.hook = s.comp + n_pad; s.core2 = s.hook + n_pad; s.tile = s.core2 + n_pad; s.edges = s.tile + 2 * T;
    s.bytes = 2 * n_pad * sizeof(u64) + (3 * n_pad + 2 * T + 8) * sizeof(int32_t);
    return s;
}

template <int DP>
struct HdTile {                                                 // what a thread holds of a column tile between its loads and its LDS stores
    f32x4 x[DP / 16];
    int4 s;                                                     // {xn bits, a point, core2 bits, comp}
};

template <int DP>
__device__ __forceinline__ void hd_tile_load(HdTile<DP> &T, const float *__restrict__ X, const float4 *__restrict__ S, const int32_t *__restrict__ valid,
                                             const HdState &st, int c0) {
    const f32x4 *src = (const f32x4 *)(X + (size_t)c0 * DP);    // the tile is 64 . DP contiguous floats
#pragma unroll
    for (int u = 0; u < DP / 16; u++) T.x[u] = src[threadIdx.x + 256 * u];
    if (threadIdx.x < HD_T) {
        const int col = c0 + threadIdx.x;                       // col < n_pad; a padding position is no point
        T.s = make_int4(__float_as_int(S[col].x), valid[col], st.core2[col], st.comp[col]);
    }
}

template <int DP>
__device__ __forceinline__ void hd_tile_store(const HdTile<DP> &T, float *__restrict__ Cs, int4 *__restrict__ Is, u64 *__restrict__ Bs) {
    constexpr int QLD = DP + 4;
#pragma unroll
    for (int u = 0; u < DP / 16; u++) {
        const int idx = threadIdx.x + 256 * u, row = idx / (DP / 4), c4 = idx % (DP / 4);
        *(f32x4 *)(Cs + row * QLD + 4 * c4) = T.x[u];
    }
    if (threadIdx.x < HD_T) {
        Is[threadIdx.x] = T.s;
        Bs[threadIdx.x] = HD_NONE;
    }
}

// grid ceil(T / 2).  st.best is HD_NONE everywhere before the launch.
template <int DP>
__global__ __launch_bounds__(256) void hdbscan_nearest_kernel(const float *__restrict__ X, const float4 *__restrict__ S, const int32_t *__restrict__ valid,
                                                              int T, HdState st) {
    extern __shared__ __align__(16) unsigned char smem[];
    constexpr int QLD = DP + 4, NCH = DP / 16;
    float *Cs = (float *)smem;                                  // [2][64][QLD]
    int4 *Is = (int4 *)(Cs + 2 * HD_T * QLD);                   // [2][64]
    u64 *Bs = (u64 *)(Is + 2 * HD_T);                           // [2][64]: a column's best key among the row tile's 64 rows
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int kg = lane >> 4, l15 = lane & 15;

    for (int pass = 0; pass < 2; pass++) {
        const int I = pass ? T - 1 - (int)blockIdx.x : (int)blockIdx.x;
        if (pass && I == (int)blockIdx.x) break;                // an odd T: the middle tile has no partner
        const int i = I * HD_T + 16 * wave + l15;
        f32x4 b[NCH];                                           // the row operand: x^_i[16c + 4kg .. + 3]
#pragma unroll
        for (int c = 0; c < NCH; c++) b[c] = *(const f32x4 *)(X + (size_t)i * DP + 16 * c + 4 * kg);
        const float xi = S[i].x;
        const bool vi = valid[i] != 0;
        const unsigned ci = (unsigned)st.core2[i];
        const int pi = st.comp[i];
        const int lo_i = st.tile[2 * I], hi_i = st.tile[2 * I + 1];
        u64 rbest = HD_NONE;
        const int n_tiles = T - I;

        HdTile<DP> Tl;
        hd_tile_load<DP>(Tl, X, S, valid, st, I * HD_T);
        hd_tile_store<DP>(Tl, Cs, Is, Bs);
        __syncthreads();
        for (int t = 0; t < n_tiles; t++) {
            const int buf = t & 1, J = I + t, c0 = J * HD_T;
            const bool diag = t == 0;
            if (t + 1 < n_tiles) hd_tile_load<DP>(Tl, X, S, valid, st, c0 + HD_T);            // in flight across the products below
            const float *C = Cs + buf * HD_T * QLD;
            const int4 *Ic = Is + buf * HD_T;
            u64 *Bc = Bs + buf * HD_T;
            const int lo_j = st.tile[2 * J], hi_j = st.tile[2 * J + 1];
            // the same for every thread of the workgroup: both tiles hold points, and not all of them in one component
            if (hi_i >= 0 && hi_j >= 0 && !(lo_i == hi_i && lo_j == hi_j && lo_i == lo_j)) {
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
#pragma unroll
                for (int g = 0; g < 4; g++)
#pragma unroll
                    for (int r = 0; r < 4; r++) {               // D[row 4kg + r][col l15]: column 16g + 4kg + r of the tile, this lane's row
                        const int cc = 16 * g + 4 * kg + r, j = c0 + cc;
                        const int4 sj = Ic[cc];
                        const float d2 = fmaxf((xi + __int_as_float(sj.x)) - 2.f * acc[g][r], 0.f);
                        // a non-negative float's bits keep its order: the maximum of three is an integer maximum
                        const unsigned wb = max(max((unsigned)__float_as_int(d2) & 0x7fffffffu, ci), (unsigned)sj.z);
                        if (vi && sj.y != 0 && pi != sj.w && (!diag || j > i)) {
                            const u64 krow = ((u64)wb << 32) | (unsigned)j, kcol = ((u64)wb << 32) | (unsigned)i;
                            rbest = min(rbest, krow);
                            if (kcol < Bc[cc]) atomicMin(&Bc[cc], kcol);
                        }
                    }
            }
            if (t + 1 < n_tiles) hd_tile_store<DP>(Tl, Cs + (buf ^ 1) * HD_T * QLD, Is + (buf ^ 1) * HD_T, Bs + (buf ^ 1) * HD_T);
            __syncthreads();                                    // tile t is done with, tile t + 1 and the column keys of t are in place
            if (threadIdx.x < HD_T) {                           // read before the next barrier; tile t + 2 resets this half behind it
                const u64 k = Bc[threadIdx.x];
                if (k != HD_NONE) atomicMin(&st.best[c0 + threadIdx.x], k);
            }
        }
        rbest = min(rbest, (u64)__shfl_xor(rbest, 16, WAVE));
        rbest = min(rbest, (u64)__shfl_xor(rbest, 32, WAVE));
        if (kg == 0 && rbest != HD_NONE) atomicMin(&st.best[i], rbest);
    }
}

// a wave per tile: every position its own root, core2 = the k-th neighbour's d2 (0 without a list, or where the position is no point)
__global__ __launch_bounds__(64) void hdbscan_start_kernel(const int32_t *__restrict__ valid, const float *__restrict__ knn_d2, int k, int n, HdState st) {
    const int i = blockIdx.x * HD_T + threadIdx.x;
    const bool v = valid[i] != 0;
    st.best[i] = HD_NONE;
    st.pick[i] = HD_NONE;
    st.comp[i] = i;
    st.hook[i] = i;
    st.core2[i] = v && knn_d2 && i < n ? __float_as_int(fmaxf(knn_d2[(size_t)i * k + (k - 1)], 0.f)) & 0x7fffffff : 0;
    const u64 m = __ballot(v);
    if (threadIdx.x == 0) {
        st.tile[2 * blockIdx.x] = m ? i + (int)__ffsll((long long)m) - 1 : INT_MAX;
        st.tile[2 * blockIdx.x + 1] = m ? i + 63 - (int)__clzll((long long)m) : -1;
        if (blockIdx.x == 0) st.edges[0] = 0;
    }
}

__global__ __launch_bounds__(256) void hdbscan_pick_kernel(const int32_t *__restrict__ valid, int n_pad, HdState st) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_pad || valid[i] == 0) return;
    const u64 k = st.best[i];
    if (k == HD_NONE) return;
    const unsigned j = (unsigned)k, lo = min((unsigned)i, j), hi = max((unsigned)i, j);
    atomicMin(&st.pick[st.comp[i]], (k & 0xffffffff00000000ull) | (u64)(lo << 16) | hi);
}

// reads comp and pick, writes hook and the edge list [3 x cap] = {lo | hi | w bits}
__global__ __launch_bounds__(256) void hdbscan_hook_kernel(const int32_t *__restrict__ valid, int n_pad, HdState st, int32_t *__restrict__ edges, int cap) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_pad) return;
    int to = i;
    const u64 k = valid[i] != 0 && st.comp[i] == i ? st.pick[i] : HD_NONE;
    if (k != HD_NONE) {
        const int lo = (int)((k >> 16) & 0xffffu), hi = (int)(k & 0xffffu);
        const int a = st.comp[lo], other = a == i ? st.comp[hi] : a;
        const bool mutual = st.pick[other] == k;
        if (!mutual || i > other) to = other;
        if (!mutual || i < other) {
            const int e = atomicAdd(&st.edges[0], 1);
            if (e < cap) {
                edges[e] = lo;
                edges[cap + e] = hi;
                edges[2 * (size_t)cap + e] = (int32_t)(k >> 32);
            }
        }
    }
    st.hook[i] = to;
}

// a wave per tile: reads hook, writes comp, the tile's {min, max} comp, the reset slots and counts = {components, edges}
__global__ __launch_bounds__(64) void hdbscan_jump_kernel(const int32_t *__restrict__ hdr, const int32_t *__restrict__ valid, int n_pad, HdState st,
                                                          int32_t *__restrict__ counts) {
    const int i = blockIdx.x * HD_T + threadIdx.x;
    const bool v = valid[i] != 0;
    int r = st.comp[i];
    for (int h = st.hook[r], step = 0; h != r && step < n_pad; h = st.hook[r], step++) r = h;   // the hooks are trees: it ends
    st.comp[i] = r;
    st.best[i] = HD_NONE;
    st.pick[i] = HD_NONE;
    int lo = v ? r : INT_MAX, hi = v ? r : -1;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        lo = min(lo, __shfl_xor(lo, o, WAVE));
        hi = max(hi, __shfl_xor(hi, o, WAVE));
    }
    if (threadIdx.x == 0) {
        st.tile[2 * blockIdx.x] = lo;
        st.tile[2 * blockIdx.x + 1] = hi;
        if (blockIdx.x == 0 && counts) {
            const int e = st.edges[0];
            counts[0] = hdr[0] - e;
            counts[1] = e;
        }
    }
}

// ---- entry points ------------------------------------------------------------------------------------------------------------

template <int DP>
static int hd_nearest_launch(gcnhip_ctx *c, const TsPack &P, int n, const HdState &st) {
    const size_t lds = sizeof(float) * (size_t)(2 * HD_T * (DP + 4)) + 2 * HD_T * sizeof(int4) + 2 * HD_T * sizeof(u64);
    auto kern = hdbscan_nearest_kernel<DP>;
    if (lds > 64 * 1024) GCNHIP_TRY(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    const int T = ts_npad(n) / HD_T;
    kern<<<(T + 1) / 2, 256, lds, c->stream>>>(P.X, P.S, P.valid, T, st);
    GCNHIP_LAUNCH_CHECK();
    return 0;
}

static int hd_refuse(const char *name, const char *why) {
    static thread_local char msg[200];
    snprintf(msg, sizeof msg, "%s: %s", name, why);
    return gcnhip_fail(msg);
}
static const char *hd_common(const gcnhip_ctx *c, const void *pack, int n, int dim, const void *state, size_t state_bytes) {
    if (!c || !pack || !state || n < 1) return "invalid argument";
    if (n > HD_MAX_N) return "at most 65536 positions (an edge's two ends share a 64-bit key with its weight)";
    if (dim < 1 || dim > TS_MAX_DIM) return "1 <= dim <= 256";
    if (!aligned16(pack) || !aligned16(state)) return "the pack and the state must be 16-byte aligned";
    if (state_bytes < hd_state(nullptr, n).bytes) return "the state is too small (gcnhip_hdbscan_plan tells the bytes)";
    return nullptr;
}

extern "C" {

int gcnhip_hdbscan_plan(int n, int dim, size_t *pack_bytes, size_t *state_bytes) {
    if (n < 0 || dim < 1 || dim > TS_MAX_DIM) return hd_refuse("gcnhip_hdbscan_plan", "invalid argument (n >= 0, 1 <= dim <= 256)");
    if (n > HD_MAX_N) return hd_refuse("gcnhip_hdbscan_plan", "at most 65536 positions (an edge's two ends share a 64-bit key with its weight)");
    if (pack_bytes) *pack_bytes = ts_pack(nullptr, n, dim).bytes;
    if (state_bytes) *state_bytes = hd_state(nullptr, n).bytes;
    return 0;
}

int gcnhip_hdbscan_start(gcnhip_ctx *c, const void *pack, int n, int dim, const float *knn_d2, int k, void *state, size_t state_bytes) {
    if (const char *why = hd_common(c, pack, n, dim, state, state_bytes)) return hd_refuse("gcnhip_hdbscan_start", why);
    if (knn_d2 && (k < 1 || k > 32)) return hd_refuse("gcnhip_hdbscan_start", "1 <= k <= 32 with a neighbour list");
    hdbscan_start_kernel<<<ts_npad(n) / HD_T, HD_T, 0, c->stream>>>(ts_pack((void *)pack, n, dim).valid, knn_d2, k, n, hd_state(state, n));
    GCNHIP_LAUNCH_CHECK();
    return 0;
}

int gcnhip_hdbscan_nearest(gcnhip_ctx *c, const void *pack, int n, int dim, void *state, size_t state_bytes) {
    if (const char *why = hd_common(c, pack, n, dim, state, state_bytes)) return hd_refuse("gcnhip_hdbscan_nearest", why);
    const TsPack P = ts_pack((void *)pack, n, dim);
    const HdState st = hd_state(state, n);
    switch (ts_dp(dim)) {
    case 16: return hd_nearest_launch<16>(c, P, n, st);
    case 32: return hd_nearest_launch<32>(c, P, n, st);
    case 64: return hd_nearest_launch<64>(c, P, n, st);
    case 128: return hd_nearest_launch<128>(c, P, n, st);
    default: return hd_nearest_launch<256>(c, P, n, st);
    }
}

int gcnhip_hdbscan_merge(gcnhip_ctx *c, const void *pack, int n, int dim, void *state, size_t state_bytes, int32_t *edges, int32_t *counts) {
    if (const char *why = hd_common(c, pack, n, dim, state, state_bytes)) return hd_refuse("gcnhip_hdbscan_merge", why);
    if (!edges || !counts) return hd_refuse("gcnhip_hdbscan_merge", "invalid argument");
    const TsPack P = ts_pack((void *)pack, n, dim);
    const HdState st = hd_state(state, n);
    const int n_pad = ts_npad(n);
    hdbscan_pick_kernel<<<ceil_div(n_pad, 256), 256, 0, c->stream>>>(P.valid, n_pad, st);
    GCNHIP_LAUNCH_CHECK();
    hdbscan_hook_kernel<<<ceil_div(n_pad, 256), 256, 0, c->stream>>>(P.valid, n_pad, st, edges, n);
    GCNHIP_LAUNCH_CHECK();
    hdbscan_jump_kernel<<<n_pad / HD_T, HD_T, 0, c->stream>>>(P.hdr, P.valid, n_pad, st, counts);
    GCNHIP_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
