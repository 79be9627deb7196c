// bucket.h — the stable bucketing of a list by a small integer key (a centre, a label), shared by kmeans.hip and silhouette.hip:
// an integer histogram per chunk of positions, one scan, and a scatter in position order, so that the members of a key are in
// ascending position.  Integers only; the float64 sums built on the member list take their order from it.
#pragma once
#include "common.h"

constexpr int KM_MAX_K = 256;
constexpr int KM_CHUNK = 1024;                    // positions per histogram chunk (part of the definition of the sums' order)

__device__ inline int list_row(const int32_t *__restrict__ d_rows, int i, int n_table) {
    const int r = d_rows ? d_rows[i] : i;
    return r >= 0 && r < n_table ? r : -1;
}

// a member: a position whose centre is in [0, k) and whose row is in the table
__device__ inline int member_centre(const int32_t *__restrict__ assign, const int32_t *__restrict__ d_rows, int i, int n, int n_table, int k) {
    if (i >= n) return -1;
    const int c = assign[i];
    return c >= 0 && c < k && list_row(d_rows, i, n_table) >= 0 ? c : -1;
}

// block = chunk: hist[chunk][c] = members of centre c in the chunk; dpart[chunk] = the chunk's sum of dist2 over members
static __global__ __launch_bounds__(256) void kmeans_hist_kernel(const int32_t *__restrict__ assign, const int32_t *__restrict__ d_rows,
                                                                 const float *__restrict__ dist2, int n, int n_table, int k,
                                                                 int32_t *__restrict__ hist, double *__restrict__ dpart) {
    __shared__ int cnt[KM_MAX_K];
    __shared__ double red[256];
    const int chunk = blockIdx.x, t = threadIdx.x;
    cnt[t] = 0;
    __syncthreads();
    double s = 0.0;
    for (int b = 0; b < KM_CHUNK / 256; b++) {
        const int i = chunk * KM_CHUNK + b * 256 + t;
        const int c = member_centre(assign, d_rows, i, n, n_table, k);
        if (c >= 0) {
            atomicAdd(&cnt[c], 1);
            if (dist2) s += (double)dist2[i];
        }
    }
    red[t] = s;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (t < w) red[t] += red[t + w];
        __syncthreads();
    }
    if (t < k) hist[(size_t)chunk * k + t] = cnt[t];
    if (t == 0) dpart[chunk] = red[0];
}

// one block: hist -> the chunk's offset inside its centre; sizes, cstart [k + 1] (first slot of a centre in the member list),
// segstart [k + 1] (first segment of a centre, in segments of `seg` members)
static __global__ __launch_bounds__(256) void kmeans_scan_kernel(int32_t *__restrict__ hist, int n_chunks, int k, int seg, int32_t *__restrict__ sizes,
                                                                 int32_t *__restrict__ cstart, int32_t *__restrict__ segstart) {
    __shared__ int tot[KM_MAX_K];
    const int c = threadIdx.x;
    if (c < k) {
        int run = 0;
#pragma unroll 8
        for (int ch = 0; ch < n_chunks; ch++) {
            const int v = hist[(size_t)ch * k + c];
            hist[(size_t)ch * k + c] = run;
            run += v;
        }
        tot[c] = run;
        sizes[c] = run;
    }
    __syncthreads();
    if (c == 0) {
        int a = 0, s = 0;
        for (int j = 0; j < k; j++) {
            cstart[j] = a;
            segstart[j] = s;
            a += tot[j];
            s += (tot[j] + seg - 1) / seg;
        }
        cstart[k] = a;
        segstart[k] = s;
    }
}

// a wave per chunk: its positions go, in order, to the next free slots of their centres
static __global__ __launch_bounds__(64) void kmeans_scatter_kernel(const int32_t *__restrict__ assign, const int32_t *__restrict__ d_rows, int n,
                                                                   int n_table, int k, const int32_t *__restrict__ hist,
                                                                   const int32_t *__restrict__ cstart, int32_t *__restrict__ order) {
    __shared__ int next[KM_MAX_K];
    const int chunk = blockIdx.x, lane = threadIdx.x;
    for (int c = lane; c < k; c += WAVE) next[c] = cstart[c] + hist[(size_t)chunk * k + c];
    __syncthreads();
    const unsigned long long below = lane ? (~0ull >> (64 - lane)) : 0ull;
    for (int b = 0; b < KM_CHUNK / WAVE; b++) {
        const int i = chunk * KM_CHUNK + b * WAVE + lane;
        const int c = member_centre(assign, d_rows, i, n, n_table, k);
        unsigned long long left = __ballot(c >= 0), mine = 0;
        while (left) {                                          // one round per distinct centre among the 64 positions
            const int lead = __ffsll(left) - 1;
            const int cl = __shfl(c, lead, WAVE);
            const unsigned long long same = __ballot(c == cl);
            if (c == cl) mine = same;
            left &= ~same;
        }
        int base = 0;
        if (c >= 0) base = next[c];
        __syncthreads();
        if (c >= 0) {
            order[base + __popcll(mine & below)] = i;
            if ((mine >> lane) >> 1 == 0) next[c] = base + __popcll(mine);    // the group's last lane
        }
        __syncthreads();
    }
}

// the last key whose first segment is <= seg and that has one (seg < segstart[k])
__device__ inline int segment_key(const int32_t *__restrict__ segstart, int k, int seg) {
    int lo = 0, hi = k - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (segstart[mid] <= seg) lo = mid; else hi = mid - 1;
    }
    return lo;
}
