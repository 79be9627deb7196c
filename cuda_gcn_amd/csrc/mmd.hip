// mmd.hip — do two groups of rows of a table come from one distribution?  The kernel two-sample statistic (MMD^2; Gretton et al.,
// 2012) with the RBF kernel and a permutation test, matrix-free: per column b of a 0/1 membership matrix S [n x Bp] (column 0 all
// ones, column 1 the observed group A, columns 2.. permuted groups, made by the caller) the three sums AA_b, AB_b, BB_b of
// k(q, r) over the pairs inside A_b, across, and outside it.  The n x n kernel matrix is never stored: a tile of it is formed on the
// exact-f32 MFMA and is, in the registers it lands in, the operand of a second MFMA product with the tile's slice of S.  Beyond the
// reference, which never looks at its hidden matrix.  include/gcnhip_driver.h has the call contracts.
//
// Rows.  silhouette.hip's contract: f32 [n_table x ld], 1 <= dim <= 256, dim <= ld, rows of any stride and alignment, columns
// [dim, ld) never read; d_rows a device int32 list of n positions (two positions that name one row are two points; NULL: rows
// 0 .. n - 1); a position whose row is outside [0, n_table) is no point.  Operand x'[j] = (T[r][j] . inv_norm[r]) - shift[j]: one
// rounded f32 multiply (none with inv_norm == NULL) and one rounded f32 subtract, never one fma; zeros past dim.  The RBF kernel is
// translation invariant, so shift (the caller's: the f32-rounded mean of the rows) changes no exact value; it removes the
// cancellation of xn_i + xn_j - 2 x_i . x_j on unit ReLU rows, which sit far from the origin.
//
// mmd_pack_kernel   block = 64 positions, wave w its rows 16 w .. 16 w + 15 one after the other: X [n_pad x ldx] = x' (ldx = dim
//   rounded up to 16, n_pad = n rounded up to 64, zeros elsewhere); xn = sum x'^2: lane l the fma chain over columns l, l + 64,
//   l + 128, l + 192 in this order, then the butterfly over the lanes (xor 32, 16, .., 1).  vmask [tile]: bit p = position
//   64 tile + p is a point.  St [tile][b]: bit p = S[64 tile + p][b] of a point (0 of what is no point): S transposed, one 64-bit
//   word per tile and column, by ballot.
// mmd_walk_kernel<DP>   grid (row tiles of 64 positions, parts of MM_PART = 1024 positions: part of the definition of the bits).
//   Wave w owns rows 16 w .. 16 w + 15; lane (kg, l15) holds x' of row 16 w + l15, columns 16 c + 4 kg .. + 3, as the B operand in
//   REGISTERS.  The part's rows stream from X in tiles of 64 through double-buffered LDS with their xn and the tile's Bp words of
//   St: the loads of tile t + 1 are in flight across the math of tile t, one barrier per tile.
//   First product: dot(q, m) ONE chain of v_mfma_f32_16x16x4_f32 over the 16-column groups c = 0 .. ldx / 16 - 1, inside a group
//   step s = 0..3 with k-slot kg = 0..3 on column 16 c + 4 kg + s.  Lane (l15, kg) then holds the dots of its row with members
//   16 t + 4 kg + r (t, r = 0..3) of the tile.  d2 = max((xn_q + xn_m) - 2 dot, 0); k = expf(fl(-gamma . d2)); the entry whose
//   member is the row's own list position is exactly 1.
//   Second product, fused: T^T[b][q] += sum_m S^T[b][m] . k[m][q] on the same instruction, one f32x4 accumulator per 16 columns of
//   S (at most 16).  The lane's k are the B operand as they lie: step (t, r) takes the four members 16 t + 4 kg + r, kg = 0..3;
//   the A operand is bit 16 t + 4 kg + r of the LDS word of column 16 a + l15, expanded to 0.f / 1.f.  So T_b[q] is ONE chain over
//   the part's tiles in ascending order, inside a tile (t, r) = (0, 0), (0, 1), .., (3, 3), four members per step: 1024 products.
//   End of the part: T -> float64 (0 for a row that is no point), R = T_0; per column b: aa = q in A_b ? T : 0, ab = q in A_b ? 0 : T,
//   bb = q in A_b ? 0 : R - T (float64); over the wave's 16 rows the butterfly xor 8, 4, 2, 1, over the waves (w0 + w1) + (w2 + w3):
//   one partial per (part, row tile, quantity, column).  With want_witness T_0 and T_1 per (part, row), float64.
// mmd_foldsum_kernel   block = (column, quantity): the batch's parts in ascending order; per part thread t adds the row tiles
//   t, t + 256, .. in order, a tree over the 256 threads (t += t + w, w = 128 .. 1), and the part's sum goes onto the running sum.
//   mmd_foldwit_kernel adds a row's T_0 and T_1 in part order.  A call walks as many parts per launch as its scratch holds: less
//   scratch, more launches, the same sequence of additions.
// mmd_final_kernel   sums [3 x Bp] = {AA | AB | BB}; counts = {points, m = points of column 1}; witness f[q] = T_1 / m - (R - T_1) /
//   (points - m), ONE float64 expression rounded to f32 (NaN for what is no point).
// No random numbers, no float atomics, no allocation, no synchronisation: every output's bits are a function of the arguments'
// contents alone.  Error of a sum against exact arithmetic on the f32 operands, u = 2^-24, gamma_(m) = m u / (1 - m u):
// |d2 - d2_exact| <= gamma_(ldx + 3) (xn_q + xn_m + 2 sum |x_q x_m|); k through e^(+-gamma . that), the rounding of the argument and
// the 1 ulp of expf; T adds gamma_(1024) of the part's sum; the float64 folds n 2^-53.  DESIGN 4.31 has the derivation.
// -Rpass-analysis=kernel-resource-usage for gfx950: DESIGN 4.31 has the table.
#include "common.h"
#include <algorithm>
#include <cmath>
#include <cstdio>

using f32x4 = __attribute__((ext_vector_type(4))) float;
using u64 = unsigned long long;

constexpr int MM_T = 64;                          // list positions per row tile, members per LDS tile
constexpr int MM_PART = 1024;                     // positions per part (part of the definition of the bits)
constexpr int MM_MAX_DIM = 256, MM_MAX_B = 256;

struct MmPack {                                   // the packed image of a call, in its scratch
    float *X, *xn;                                // [n_pad x ldx], [n_pad]
    u64 *vmask, *St;                              // [n_tiles], [n_tiles x Bp]
    int ldx, n_pad, n_tiles;
};

__device__ __forceinline__ float mm_shifted(float x, float inv, float shift) {
#pragma clang fp contract(off)
    const float p = x * inv;
    return p - shift;
}
__device__ __forceinline__ int mm_list_row(const int32_t *__restrict__ d_rows, int pos, int n, int n_table) {
    if (pos >= n) return -1;
    const int r = d_rows ? d_rows[pos] : pos;
    return r >= 0 && r < n_table ? r : -1;
}

// block = tile of 64 positions
__global__ __launch_bounds__(256) void mmd_pack_kernel(const float *__restrict__ table, int ld, int n_table, int dim,
                                                       const float *__restrict__ inv_norm, const int32_t *__restrict__ d_rows, int n,
                                                       const float *__restrict__ shift, const uint8_t *__restrict__ bits, int Bp, MmPack P) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, tile = blockIdx.x;
    float sh[4];
#pragma unroll
    for (int u = 0; u < 4; u++) sh[u] = lane + WAVE * u < dim ? shift[lane + WAVE * u] : 0.f;
    for (int rr = 0; rr < 16; rr++) {
        const int pos = tile * MM_T + 16 * wave + rr;
        const int r = mm_list_row(d_rows, pos, n, n_table);
        const float inv = r >= 0 && inv_norm ? inv_norm[r] : 1.f;
        float s = 0.f;
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int col = lane + WAVE * u;
            if (col < P.ldx) {
                const float v = r >= 0 && col < dim ? mm_shifted(table[(size_t)r * ld + col], inv, sh[u]) : 0.f;
                P.X[(size_t)pos * P.ldx + col] = v;
                s = __fmaf_rn(v, v, s);
            }
        }
        s = wave_sum(s);
        if (lane == 0) P.xn[pos] = s;
    }
    const int pos = tile * MM_T + lane;
    const bool ok = mm_list_row(d_rows, pos, n, n_table) >= 0;
    const u64 vm = __ballot(ok);
    if (wave == 0 && lane == 0) P.vmask[tile] = vm;
    const uint8_t *mine = bits + (size_t)pos * (Bp / 8);       // read only where ok
    for (int c = wave; c < Bp; c += 4) {
        const bool bit = ok && ((mine[c >> 3] >> (c & 7)) & 1);
        const u64 w = __ballot(bit);
        if (lane == 0) P.St[(size_t)tile * Bp + c] = w;
    }
}

template <int DP>
struct MmTile {                                   // what a thread holds of a member tile between its loads and its LDS stores
    f32x4 x[DP / 16];
    float xn;
    u64 s;
};

// thread e of 256 holds float4 (row, c4) of the tile for idx = e + 256 u: row = idx / (DP / 4), c4 = idx % (DP / 4)
template <int DP>
__device__ __forceinline__ void mm_tile_load(MmTile<DP> &L, const MmPack &P, int tile, int Bp) {
#pragma unroll
    for (int u = 0; u < DP / 16; u++) {
        const int idx = threadIdx.x + 256 * u, row = idx / (DP / 4), col = 4 * (idx % (DP / 4));
        if (col < P.ldx) L.x[u] = *(const f32x4 *)(P.X + (size_t)(tile * MM_T + row) * P.ldx + col);
    }
    if (threadIdx.x < MM_T) L.xn = P.xn[tile * MM_T + threadIdx.x];
    if ((int)threadIdx.x < Bp) L.s = P.St[(size_t)tile * Bp + threadIdx.x];
}
template <int DP>
__device__ __forceinline__ void mm_tile_store(const MmTile<DP> &L, const MmPack &P, int Bp, float *__restrict__ Cs, float *__restrict__ Ns,
                                              u64 *__restrict__ Ss) {
    constexpr int QLD = DP + 4;
#pragma unroll
    for (int u = 0; u < DP / 16; u++) {
        const int idx = threadIdx.x + 256 * u, row = idx / (DP / 4), col = 4 * (idx % (DP / 4));
        if (col < P.ldx) *(f32x4 *)(Cs + row * QLD + col) = L.x[u];
    }
    if (threadIdx.x < MM_T) Ns[threadIdx.x] = L.xn;
    if ((int)threadIdx.x < Bp) Ss[threadIdx.x] = L.s;
}

// the first product: acc[t][r] = dot(member 16 t + 4 kg + r of the tile, this lane's row), one MFMA chain per entry
template <int DP>
__device__ __forceinline__ void mm_products(const float *__restrict__ C, const f32x4 (&b)[DP / 16], f32x4 (&acc)[4], int nch, int kg, int l15) {
    constexpr int QLD = DP + 4;
#pragma unroll
    for (int t = 0; t < 4; t++) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int c = 0; c < DP / 16; c++) {
        if (c >= nch) continue;                                 // the same for every thread (no break: b[] keeps static indices)
        f32x4 a[4];
#pragma unroll
        for (int t = 0; t < 4; t++) a[t] = *(const f32x4 *)(C + (16 * t + l15) * QLD + 16 * c + 4 * kg);
#pragma unroll
        for (int s = 0; s < 4; s++)                             // the four accumulators in turn: no MFMA waits for the one before it
#pragma unroll
            for (int t = 0; t < 4; t++) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[t][s], b[c][s], acc[t], 0, 0, 0);
    }
}

// grid (row tiles, parts of the batch).  partials [part of the batch][row tile][quantity][Bp]; wit [part of the batch][n_pad][2]
template <int DP>
__global__ __launch_bounds__(256) void mmd_walk_kernel(MmPack P, int Bp, float neg_gamma, int part0, double *__restrict__ partials,
                                                       double *__restrict__ wit) {
    extern __shared__ __align__(16) unsigned char smem[];
    constexpr int QLD = DP + 4;
    float *Cs = (float *)smem;                                  // [2][64][QLD]
    float *Ns = Cs + 2 * MM_T * QLD;                            // [2][64]
    u64 *Ss = (u64 *)(Ns + 2 * MM_T);                           // [2][256]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, kg = lane >> 4, l15 = lane & 15;
    const int nch = P.ldx / 16, nb = Bp / 16;
    const int rt = blockIdx.x, part = part0 + blockIdx.y;
    const int t_begin = part * (MM_PART / MM_T), t_end = min(P.n_tiles, t_begin + MM_PART / MM_T);
    const int mine = 16 * wave + l15, q = rt * MM_T + mine;

    f32x4 b[DP / 16];
#pragma unroll
    for (int c = 0; c < DP / 16; c++) b[c] = c < nch ? *(const f32x4 *)(P.X + (size_t)q * P.ldx + 16 * c + 4 * kg) : f32x4{0.f, 0.f, 0.f, 0.f};
    const float xnq = P.xn[q];
    f32x4 T[MM_MAX_B / 16];
#pragma unroll
    for (int a = 0; a < MM_MAX_B / 16; a++) T[a] = f32x4{0.f, 0.f, 0.f, 0.f};

    MmTile<DP> L;
    mm_tile_load<DP>(L, P, t_begin, Bp);
    mm_tile_store<DP>(L, P, Bp, Cs, Ns, Ss);
    __syncthreads();
    int buf = 0;
    for (int tile = t_begin; tile < t_end; tile++, buf ^= 1) {
        const bool more = tile + 1 < t_end;
        if (more) mm_tile_load<DP>(L, P, tile + 1, Bp);         // in flight across the math below
        f32x4 acc[4];
        mm_products<DP>(Cs + buf * MM_T * QLD, b, acc, nch, kg, l15);
        const float *Nc = Ns + buf * MM_T;
        const int self = tile == rt ? mine : -1;                // the member of this tile that is the row's own position
#pragma unroll
        for (int t = 0; t < 4; t++)
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int cc = 16 * t + 4 * kg + r;
                const float d2 = fmaxf((xnq + Nc[cc]) - 2.f * acc[t][r], 0.f);
                const float k = expf(__fmul_rn(neg_gamma, d2));
                acc[t][r] = cc == self ? 1.f : k;
            }
        const u64 *Sc = Ss + buf * MM_MAX_B;
#pragma unroll
        for (int a0 = 0; a0 < MM_MAX_B / 16; a0 += 4) {
            if (a0 >= nb) continue;                             // the same for every thread
            unsigned lo[4], hi[4];                              // bit 16 (t & 1) + r of lo (t < 2) or hi: member 16 t + 4 kg + r
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const u64 w = a0 + j < nb ? Sc[16 * (a0 + j) + l15] >> (4 * kg) : 0ull;
                lo[j] = (unsigned)w;
                hi[j] = (unsigned)(w >> 32);
            }
#pragma unroll
            for (int t = 0; t < 4; t++)
#pragma unroll
                for (int r = 0; r < 4; r++)
#pragma unroll
                    for (int j = 0; j < 4; j++) {               // up to four accumulators in turn
                        if (a0 + j >= nb) continue;
                        const float av = (float)(((t < 2 ? lo[j] : hi[j]) >> (16 * (t & 1) + r)) & 1u);
                        T[a0 + j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, acc[t][r], T[a0 + j], 0, 0, 0);
                    }
        }
        if (more) mm_tile_store<DP>(L, P, Bp, Cs + (buf ^ 1) * MM_T * QLD, Ns + (buf ^ 1) * MM_T, Ss + (buf ^ 1) * MM_MAX_B);
        __syncthreads();                                        // this tile is done with, the next is in place
    }

    // the end of the part: lane (l15, kg) holds T_b[q] of its row for b = 16 a + 4 kg + rr.  The tile buffers are free.
    const bool point = (P.vmask[rt] >> mine) & 1ull;
    const float t0 = __shfl(T[0][0], l15, WAVE), t1 = __shfl(T[0][1], l15, WAVE);   // lane (l15, 0): columns 0 and 1
    const double R = point ? (double)t0 : 0.0;
    if (wit && kg == 0) {
        double *out = wit + ((size_t)blockIdx.y * P.n_pad + q) * 2;
        out[0] = R;
        out[1] = point ? (double)t1 : 0.0;
    }
    double *red = (double *)smem;                               // [4 waves][3][Bp]
#pragma unroll
    for (int a = 0; a < MM_MAX_B / 16; a++) {
        if (a >= nb) continue;
#pragma unroll
        for (int rr = 0; rr < 4; rr++) {
            const int col = 16 * a + 4 * kg + rr;
            const bool in = (P.St[(size_t)rt * Bp + col] >> mine) & 1ull;   // a point, or the bit is 0
            const double t = point ? (double)T[a][rr] : 0.0;
            double aa = in ? t : 0.0, ab = in ? 0.0 : t, bb = in ? 0.0 : R - t;
#pragma unroll
            for (int off = 8; off > 0; off >>= 1) {
                aa += __shfl_xor(aa, off, WAVE);
                ab += __shfl_xor(ab, off, WAVE);
                bb += __shfl_xor(bb, off, WAVE);
            }
            if (l15 == 0) {
                red[(wave * 3 + 0) * Bp + col] = aa;
                red[(wave * 3 + 1) * Bp + col] = ab;
                red[(wave * 3 + 2) * Bp + col] = bb;
            }
        }
    }
    __syncthreads();
    double *out = partials + ((size_t)blockIdx.y * P.n_tiles + rt) * 3 * Bp;
    for (int e = threadIdx.x; e < 3 * Bp; e += 256) out[e] = (red[e] + red[3 * Bp + e]) + (red[6 * Bp + e] + red[9 * Bp + e]);
}

// grid (Bp, 3): run [quantity][Bp] (+)= the batch's parts in order, each part's row tiles by a strided sum and a tree
__global__ __launch_bounds__(256) void mmd_foldsum_kernel(const double *__restrict__ partials, int n_tiles, int parts, int Bp, int from_zero,
                                                          double *__restrict__ run) {
    __shared__ double red[256];
    const int t = threadIdx.x, col = blockIdx.x, qty = blockIdx.y;
    double total = from_zero ? 0.0 : run[qty * Bp + col];
    for (int p = 0; p < parts; p++) {
        double s = 0.0;
        for (int tile = t; tile < n_tiles; tile += 256) s += partials[(((size_t)p * n_tiles + tile) * 3 + qty) * Bp + col];
        red[t] = s;
        __syncthreads();
        for (int w = 128; w > 0; w >>= 1) {
            if (t < w) red[t] += red[t + w];
            __syncthreads();
        }
        total += red[0];
        __syncthreads();
    }
    if (t == 0) run[qty * Bp + col] = total;
}
// thread = (row, 0 | 1): run [n_pad][2] (+)= T_0, T_1 of the batch's parts in order
__global__ __launch_bounds__(256) void mmd_foldwit_kernel(const double *__restrict__ wit, int n_pad, int parts, int from_zero, double *__restrict__ run) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x, len = 2 * (size_t)n_pad;
    if (e >= len) return;
    double s = from_zero ? 0.0 : run[e];
    for (int p = 0; p < parts; p++) s += wit[(size_t)p * len + e];
    run[e] = s;
}

// grid (n_pad / 256): every block counts, block 0 hands the sums and the counts, each its 256 rows of the witness
__global__ __launch_bounds__(256) void mmd_final_kernel(MmPack P, int n, int Bp, const double *__restrict__ run, const double *__restrict__ wrun,
                                                        double *__restrict__ sums, int32_t *__restrict__ counts, float *__restrict__ witness) {
    __shared__ int pts[256], obs[256];
    const int t = threadIdx.x;
    int np = 0, nm = 0;
    for (int tile = t; tile < P.n_tiles; tile += 256) {
        np += __popcll(P.vmask[tile]);
        nm += __popcll(P.St[(size_t)tile * Bp + 1]);
    }
    pts[t] = np;
    obs[t] = nm;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (t < w) { pts[t] += pts[t + w]; obs[t] += obs[t + w]; }
        __syncthreads();
    }
    if (blockIdx.x == 0) {
        for (int e = t; e < 3 * Bp; e += 256) sums[e] = run[e];
        if (t == 0) { counts[0] = pts[0]; counts[1] = obs[0]; }
    }
    const int i = blockIdx.x * 256 + t;
    if (witness && i < n) {
        const bool point = (P.vmask[i / MM_T] >> (i % MM_T)) & 1ull;
        const double m = (double)obs[0], rest = (double)(pts[0] - obs[0]), R = wrun[2 * (size_t)i], t1 = wrun[2 * (size_t)i + 1];
        witness[i] = point ? (float)(t1 / m - (R - t1) / rest) : NAN;
    }
}

// ---- entry points ------------------------------------------------------------------------------------------------------------

static int mm_refuse(const char *name, const char *why) {
    static thread_local char msg[200];
    snprintf(msg, sizeof msg, "%s: %s", name, why);
    return gcnhip_fail(msg);
}
static size_t mm_up256(size_t b) { return (b + 255) / 256 * 256; }

// the scratch of a call: {run [3 x Bp] | wrun [n_pad x 2] | X | xn | vmask | St | per part: partials [n_tiles x 3 x Bp], wit [n_pad x 2]}
struct MmLayout {
    int n_pad, n_tiles, parts, ldx;
    size_t run, wrun, X, xn, vmask, St, part0, psum, per_part;
};
static MmLayout mm_layout(int n, int dim, int Bp, int want_witness) {
    MmLayout L;
    L.n_tiles = std::max(ceil_div(n, MM_T), 1);
    L.n_pad = L.n_tiles * MM_T;
    L.parts = ceil_div(L.n_pad, MM_PART);
    L.ldx = (dim + 15) / 16 * 16;
    L.run = 0;
    L.wrun = L.run + mm_up256(3 * (size_t)Bp * sizeof(double));
    L.X = L.wrun + (want_witness ? mm_up256(2 * (size_t)L.n_pad * sizeof(double)) : 0);
    L.xn = L.X + mm_up256((size_t)L.n_pad * L.ldx * sizeof(float));
    L.vmask = L.xn + mm_up256((size_t)L.n_pad * sizeof(float));
    L.St = L.vmask + mm_up256((size_t)L.n_tiles * sizeof(u64));
    L.part0 = L.St + mm_up256((size_t)L.n_tiles * Bp * sizeof(u64));
    L.psum = mm_up256((size_t)L.n_tiles * 3 * Bp * sizeof(double));
    L.per_part = L.psum + (want_witness ? mm_up256(2 * (size_t)L.n_pad * sizeof(double)) : 0);
    return L;
}
static MmPack mm_pack(const MmLayout &L, void *scratch) {
    unsigned char *b = (unsigned char *)scratch;
    return MmPack{(float *)(b + L.X), (float *)(b + L.xn), (u64 *)(b + L.vmask), (u64 *)(b + L.St), L.ldx, L.n_pad, L.n_tiles};
}
static const char *mm_shape(int n, int dim, int Bp) {
    if (n < 0) return "invalid argument (n >= 0)";
    if (dim < 1 || dim > MM_MAX_DIM) return "1 <= dim <= 256";
    if (Bp < 16 || Bp > MM_MAX_B || Bp % 16 != 0) return "the columns of S are a multiple of 16 in 16..256 (more permutations: more calls)";
    return nullptr;
}

template <int DP>
static int mm_walk_launch(gcnhip_ctx *c, const MmPack &P, int Bp, float gamma, int part0, int parts, double *partials, double *wit) {
    const size_t lds = sizeof(float) * (2 * (size_t)MM_T * (DP + 4) + 2 * MM_T) + 2 * MM_MAX_B * sizeof(u64);
    auto kern = mmd_walk_kernel<DP>;
    if (lds > 64 * 1024) GCNHIP_TRY(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    kern<<<dim3(P.n_tiles, parts), 256, lds, c->stream>>>(P, Bp, -gamma, part0, partials, wit);
    GCNHIP_LAUNCH_CHECK();
    return 0;
}

extern "C" {

int gcnhip_mmd_plan(int n, int dim, int Bp, int want_witness, size_t *bytes, size_t *bytes_min) {
    if (const char *why = mm_shape(n, dim, Bp)) return mm_refuse("gcnhip_mmd_plan", why);
    const MmLayout L = mm_layout(n, dim, Bp, want_witness);
    if (bytes) *bytes = L.part0 + (size_t)L.parts * L.per_part;
    if (bytes_min) *bytes_min = L.part0 + L.per_part;
    return 0;
}

int gcnhip_mmd_walk(gcnhip_ctx *c, const float *table, int ld, int n_table, int dim, const float *inv_norm, const int32_t *d_rows, int n,
                    const float *shift, float gamma, const uint8_t *bits, int Bp, int want_witness, void *scratch, size_t scratch_bytes) {
    const char *name = "gcnhip_mmd_walk";
    if (!c || !table || !shift || !scratch || n_table < 0 || (n > 0 && !bits)) return mm_refuse(name, "invalid argument");
    if (const char *why = mm_shape(n, dim, Bp)) return mm_refuse(name, why);
    if (ld < dim) return mm_refuse(name, "the row stride is below dim");
    if (!d_rows && n > n_table) return mm_refuse(name, "without a row list n is at most n_table");
    if (!(gamma >= 0.f) || !std::isfinite(gamma)) return mm_refuse(name, "gamma must be finite and at least 0");
    if (!aligned16(scratch)) return mm_refuse(name, "the scratch is not 16-byte aligned");
    const MmLayout L = mm_layout(n, dim, Bp, want_witness);
    if (scratch_bytes < L.part0 + L.per_part) return mm_refuse(name, "the scratch is below the minimum (gcnhip_mmd_plan tells the bytes)");
    const MmPack P = mm_pack(L, scratch);
    unsigned char *base = (unsigned char *)scratch;
    double *run = (double *)(base + L.run), *wrun = want_witness ? (double *)(base + L.wrun) : nullptr;
    double *partials = (double *)(base + L.part0);

    mmd_pack_kernel<<<L.n_tiles, 256, 0, c->stream>>>(table, ld, n_table, dim, inv_norm, d_rows, n, shift, bits, Bp, P);
    GCNHIP_LAUNCH_CHECK();
    const int batch = (int)std::min<size_t>(std::min<size_t>((scratch_bytes - L.part0) / L.per_part, (size_t)L.parts), 65535);
    for (int p0 = 0; p0 < L.parts; p0 += batch) {
        const int parts = std::min(batch, L.parts - p0);
        double *wit = want_witness ? (double *)(base + L.part0 + (size_t)batch * L.psum) : nullptr;
        const int rc = dim <= 128 ? mm_walk_launch<128>(c, P, Bp, gamma, p0, parts, partials, wit)
                                  : mm_walk_launch<256>(c, P, Bp, gamma, p0, parts, partials, wit);
        if (rc != 0) return rc;
        mmd_foldsum_kernel<<<dim3(Bp, 3), 256, 0, c->stream>>>(partials, L.n_tiles, parts, Bp, p0 == 0 ? 1 : 0, run);
        GCNHIP_LAUNCH_CHECK();
        if (want_witness) {
            mmd_foldwit_kernel<<<ceil_div(2 * (int64_t)L.n_pad, 256), 256, 0, c->stream>>>(wit, L.n_pad, parts, p0 == 0 ? 1 : 0, wrun);
            GCNHIP_LAUNCH_CHECK();
        }
    }
    return 0;
}

int gcnhip_mmd_fold(gcnhip_ctx *c, int n, int dim, int Bp, int want_witness, const void *scratch, size_t scratch_bytes, double *sums,
                    int32_t *counts, float *witness) {
    const char *name = "gcnhip_mmd_fold";
    if (!c || !scratch || !sums || !counts || (want_witness && n > 0 && !witness)) return mm_refuse(name, "invalid argument");
    if (const char *why = mm_shape(n, dim, Bp)) return mm_refuse(name, why);
    if (!aligned16(scratch)) return mm_refuse(name, "the scratch is not 16-byte aligned");
    const MmLayout L = mm_layout(n, dim, Bp, want_witness);
    if (scratch_bytes < L.part0 + L.per_part) return mm_refuse(name, "the scratch is below the minimum (gcnhip_mmd_plan tells the bytes)");
    const MmPack P = mm_pack(L, const_cast<void *>(scratch));
    const unsigned char *base = (const unsigned char *)scratch;
    mmd_final_kernel<<<L.n_pad / 256 + 1, 256, 0, c->stream>>>(P, n, Bp, (const double *)(base + L.run), (const double *)(base + L.wrun), sums, counts,
                                                               want_witness ? witness : nullptr);
    GCNHIP_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
