// explain.hip — why a trained model gives a node a logit: the logit of query (v, c) split by the neighbour a term came through,
// by hidden unit and by input feature column.  Beyond the reference, which only prints accuracy.
//
// The network is Z = A^ . (ReLU(A^ . X . W1) . W2) without bias.  With the ReLU gates of a forward fixed (g_i[k] = H1[u_i, k] > 0,
// read from the very table the forward wrote), a logit is a plain sum over the stored edges e_1 .. e_d of row v (u_i = col(e_i),
// a_i = A^[v, u_i]) and S = A^ . X:
//   z      = sum_i a_i sum_k H1[u_i, k] W2[k, c]
//   nbr_i  = a_i sum_k H1[u_i, k] W2[k, c]
//   hid_k  = W2[k, c] sum_i a_i H1[u_i, k]
//   feat_f = sum_i a_i sum_k g_i[k] W2[k, c] W1[f, k] S[u_i, f]
// scaling (gcnhip_graphsum_ex's meaning): 0 = plain tables, a_i = coef[e_i]; 1 = the factored form, table row r carries dinv[r],
// so a_i . H1[u_i] = dinv_row[v] . H1'[u_i], a_i . S[u_i] = dinv_row[v] . S'[u_i], and the two-hop term a_i . A^[u_i, w] . x(w) =
// dinv_row[v] . dinv2_row[u_i] . X'[w]: the kernels then use a_i := dinv_row[v] on the scaled tables.
//
//   explain_hops_kernel       a workgroup per query.  Waves take the stored edges in turn, lanes along k, one butterfly per edge:
//                             nbr_i.  Thread k then walks the edges in stored order for hid_k; wave 0 adds the hid_k (four per lane in
//                             fixed order, one butterfly): the logit.
//   explain_feat_agg_kernel   grid (query, tiles of 64 feature columns), 256 threads = 64 columns x 4 parts.  The W1 tile sits in LDS
//                             transposed ([k][65]: lanes on consecutive columns, no bank conflict), the neighbours are consumed in
//                             chunks of 16 in stored order: the chunk's gated rows r_j[k] = a_j g_j[k] W2[k, c] go to LDS, part p
//                             folds neighbours 4p .. 4p + 3 of the chunk (t_j = sum_k r_j[k] W1[f, k], one W1 read per four FMAs,
//                             the r reads are broadcasts) and adds S[u_j, f] . t_j — a thread owns a column, so S row loads coalesce.
//                             The four partial sums are added as (p0 + p1) + (p2 + p3).
//   explain_feat_walk_kernel  a wave per query, for a feature object in CSR (sparse, or dense with indices == NULL): i -> w in
//                             row(u_i) -> non-zeros (f, x); lanes along k hold r_i in registers, one butterfly per non-zero, and lane 0
//                             alone adds into the neighbour's LDS row, which the wave adds to feat[q, :] when the neighbour is done:
//                             a fixed order.  Clarity before speed: sparse rows are short.
//   explain_abs_colsum_kernel 64 columns per workgroup; a thread owns a column, keeps its [C] double sums in LDS (its own slots: no
//                             barrier) and walks the batch's rows in order.
// No atomics, no allocation, no dependence on block order or on the other queries of a launch: two launches give the same bits.
// The entry points copy the query lists to the host and check them (this synchronises the stream): a row or class outside its
// range is an argument error before any launch.
#include "common.h"
#include <algorithm>
#include <cstdio>
#include <vector>

constexpr int XP_MAX_H = 256;                     // hidden width: thread k of a workgroup owns unit k
constexpr int XP_MAX_C = 256;                     // abs_colsum: classes whose sums a thread keeps in LDS
constexpr int XP_FT = 64;                         // feature columns per workgroup of the _agg kernel
constexpr int XP_NC = 16;                         // first-hop neighbours per chunk: four per part
constexpr int XP_WLD = XP_FT + 1;                 // row stride of the transposed W1 tile

struct XpGraph {
    const int *indptr, *indices;
    const float *coef, *dinv_row, *dinv2_row;
};
struct XpQuery {
    const int32_t *row, *cls;
    const float *h1; int ld_h1, h;
    const float *w2; int ld_w2;
    int scaling;
};

__global__ __launch_bounds__(256) void explain_hops_kernel(XpGraph g, XpQuery q, float *__restrict__ logit, float *__restrict__ hidden, int ld_out,
                                                           const int32_t *__restrict__ nbr_ptr, int32_t *__restrict__ nbr_row,
                                                           float *__restrict__ nbr_val) {
    __shared__ float w2c[XP_MAX_H], hid[XP_MAX_H];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int v = q.row[b], c = q.cls[b];
    const int e0 = g.indptr[v], d = g.indptr[v + 1] - e0;
    const float post = q.scaling ? g.dinv_row[v] : 1.f;
    w2c[tid] = tid < q.h ? q.w2[(size_t)tid * q.ld_w2 + c] : 0.f;
    __syncthreads();
    const size_t p0 = (size_t)nbr_ptr[b];
    for (int i = wave; i < d; i += 4) {
        const int u = g.indices[e0 + i];
        const float *row = q.h1 + (size_t)u * q.ld_h1;
        float s = 0.f;
        for (int k = lane; k < q.h; k += WAVE) s += row[k] * w2c[k];
        s = wave_sum(s);
        if (lane == 0) {
            nbr_val[p0 + i] = (q.scaling ? post : g.coef[e0 + i]) * s;
            nbr_row[p0 + i] = u;
        }
    }
    float hv = 0.f;
    if (tid < q.h) {
        float acc = 0.f;
        if (q.scaling) {
            for (int i = 0; i < d; i++) acc += q.h1[(size_t)g.indices[e0 + i] * q.ld_h1 + tid];
            acc *= post;
        } else {
            for (int i = 0; i < d; i++) acc += g.coef[e0 + i] * q.h1[(size_t)g.indices[e0 + i] * q.ld_h1 + tid];
        }
        hv = w2c[tid] * acc;
        hidden[(size_t)b * ld_out + tid] = hv;
    }
    hid[tid] = hv;
    __syncthreads();
    if (wave == 0) {
        const float s = wave_sum((hid[lane] + hid[lane + 64]) + (hid[lane + 128] + hid[lane + 192]));
        if (lane == 0) logit[b] = s;
    }
}

__global__ __launch_bounds__(256) void explain_feat_agg_kernel(XpGraph g, XpQuery q, const float *__restrict__ w1, int ld_w1, int F,
                                                               const float *__restrict__ S, int ld_s, float *__restrict__ feat, int ld_f) {
    extern __shared__ __align__(16) unsigned char smem[];
    const int h = q.h;
    float *W1s = (float *)smem;                                // [h][65]: W1[f0 + ff, k] at k * 65 + ff
    float *rs = W1s + (size_t)h * XP_WLD;                      // [16][h]: the chunk's gated rows
    float *w2c = rs + XP_NC * h;                               // [h]
    float *part = w2c + h;                                     // [4][64]
    int *us = (int *)(part + 4 * XP_FT);                       // [16]: the chunk's rows of S
    const int b = blockIdx.x, f0 = blockIdx.y * XP_FT, tid = threadIdx.x, fl = tid & 63, p = tid >> 6, f = f0 + fl;
    const int v = q.row[b], c = q.cls[b];
    const int e0 = g.indptr[v], d = g.indptr[v + 1] - e0;
    const float post = q.scaling ? g.dinv_row[v] : 1.f;
    for (int idx = tid; idx < XP_FT * h; idx += 256) {
        const int ff = idx / h, k = idx - ff * h;
        W1s[k * XP_WLD + ff] = f0 + ff < F ? w1[(size_t)(f0 + ff) * ld_w1 + k] : 0.f;
    }
    for (int k = tid; k < h; k += 256) w2c[k] = q.w2[(size_t)k * q.ld_w2 + c];
    float acc = 0.f;
    for (int i0 = 0; i0 < d; i0 += XP_NC) {
        __syncthreads();                                       // the chunk before this one is consumed (first pass: W1s, w2c are there)
        const int nv = min(XP_NC, d - i0);
        if (tid < XP_NC) us[tid] = tid < nv ? g.indices[e0 + i0 + tid] : -1;
        for (int idx = tid; idx < XP_NC * h; idx += 256) {
            const int j = idx / h, k = idx - j * h;
            float r = 0.f;
            if (j < nv) {
                const int e = e0 + i0 + j;
                const float a = q.scaling ? post : g.coef[e];
                if (q.h1[(size_t)g.indices[e] * q.ld_h1 + k] > 0.f) r = a * w2c[k];
            }
            rs[idx] = r;
        }
        __syncthreads();
        float t0 = 0.f, t1 = 0.f, t2 = 0.f, t3 = 0.f;
        const float *r0 = rs + (size_t)(4 * p) * h;
        for (int k = 0; k < h; k++) {
            const float w = W1s[k * XP_WLD + fl];
            t0 += r0[k] * w;
            t1 += r0[h + k] * w;
            t2 += r0[2 * h + k] * w;
            t3 += r0[3 * h + k] * w;
        }
        if (f < F) {
            const int j = 4 * p;
            if (j < nv) acc += S[(size_t)us[j] * ld_s + f] * t0;
            if (j + 1 < nv) acc += S[(size_t)us[j + 1] * ld_s + f] * t1;
            if (j + 2 < nv) acc += S[(size_t)us[j + 2] * ld_s + f] * t2;
            if (j + 3 < nv) acc += S[(size_t)us[j + 3] * ld_s + f] * t3;
        }
    }
    part[p * XP_FT + fl] = acc;
    __syncthreads();
    if (p == 0 && f < F) feat[(size_t)b * ld_f + f] = (part[fl] + part[XP_FT + fl]) + (part[2 * XP_FT + fl] + part[3 * XP_FT + fl]);
}

// One wave per workgroup, so the barriers below only order this wave's LDS traffic.  tmp [F] in LDS holds the inner sum of one
// first-hop neighbour (over w and the non-zeros of X[w]); it is added to feat[q, :] when the neighbour is done: the nested order
// sum_i (sum_w ...) of the definition, d + D additions deep, not d . D.
__global__ __launch_bounds__(64) void explain_feat_walk_kernel(XpGraph g, XpQuery q, const float *__restrict__ w1, int ld_w1, int F,
                                                               const int *__restrict__ x_indptr, const int *__restrict__ x_indices,
                                                               const float *__restrict__ x_values, float *__restrict__ feat, int ld_f) {
    extern __shared__ __align__(16) unsigned char smem[];
    float *tmp = (float *)smem;                                // [F]
    const int lane = threadIdx.x, b = blockIdx.x;
    const int v = q.row[b], c = q.cls[b];
    const int e0 = g.indptr[v], d = g.indptr[v + 1] - e0;
    const float post = q.scaling ? g.dinv_row[v] : 1.f;
    float *out = feat + (size_t)b * ld_f;
    for (int f = lane; f < F; f += WAVE) { out[f] = 0.f; tmp[f] = 0.f; }
    float w2r[4];                                              // lane's units k = lane + 64 m
#pragma unroll
    for (int m = 0; m < 4; m++) {
        const int k = lane + 64 * m;
        w2r[m] = k < q.h ? q.w2[(size_t)k * q.ld_w2 + c] : 0.f;
    }
    __syncthreads();
    for (int i = 0; i < d; i++) {
        const int u = g.indices[e0 + i];
        const float a = q.scaling ? post : g.coef[e0 + i];
        float r[4];
#pragma unroll
        for (int m = 0; m < 4; m++) {
            const int k = lane + 64 * m;
            r[m] = k < q.h && q.h1[(size_t)u * q.ld_h1 + k] > 0.f ? a * w2r[m] : 0.f;
        }
        const int u0 = g.indptr[u], u1 = g.indptr[u + 1];
        for (int e = u0; e < u1; e++) {
            const int w = g.indices[e];
            const float hop = q.scaling ? g.dinv2_row[u] : g.coef[e];
            const int x0 = x_indptr[w], x1 = x_indptr[w + 1];
            for (int z = x0; z < x1; z++) {
                const int f = x_indices ? x_indices[z] : z - x0;
                const float *wrow = w1 + (size_t)f * ld_w1;
                float s = 0.f;
#pragma unroll
                for (int m = 0; m < 4; m++) {
                    const int k = lane + 64 * m;
                    if (k < q.h) s += wrow[k] * r[m];
                }
                s = wave_sum(s);
                if (lane == 0) tmp[f] += (hop * x_values[z]) * s;
            }
        }
        __syncthreads();
        for (int f = lane; f < F; f += WAVE) { out[f] += tmp[f]; tmp[f] = 0.f; }
        __syncthreads();
    }
}

__global__ __launch_bounds__(64) void explain_abs_colsum_kernel(const float *__restrict__ feat, int ld_f, const int32_t *__restrict__ q_class,
                                                                int nq, int F, int C, double *__restrict__ acc, int32_t *__restrict__ count) {
    extern __shared__ __align__(16) unsigned char smem[];
    double *a = (double *)smem;                                // [C][64]: column `lane` is this thread's alone
    const int lane = threadIdx.x, f = blockIdx.x * 64 + lane;
    if (f < F) {
        for (int cls = 0; cls < C; cls++) a[cls * 64 + lane] = acc[(size_t)cls * F + f];
        for (int i = 0; i < nq; i++) a[q_class[i] * 64 + lane] += fabs((double)feat[(size_t)i * ld_f + f]);
        for (int cls = 0; cls < C; cls++) acc[(size_t)cls * F + f] = a[cls * 64 + lane];
    }
    if (blockIdx.x == 0)
        for (int cls = lane; cls < C; cls += 64) {
            int n = 0;
            for (int i = 0; i < nq; i++) n += q_class[i] == cls;
            count[cls] += n;
        }
}

#define XP_REFUSE(NAME, WHY)                                                      \
    do {                                                                          \
        char msg[200];                                                            \
        snprintf(msg, sizeof msg, "%s: %s", NAME, WHY);                           \
        return gcnhip_fail(msg);                                                  \
    } while (0)

// a device int32 list on the host (synchronises the stream)
static int xp_download(gcnhip_ctx *c, const int32_t *d, int n, std::vector<int32_t> &h) {
    h.resize((size_t)n);
    if (n) GCNHIP_TRY(hipMemcpyAsync(h.data(), d, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    GCNHIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

// what every entry point checks of its queries and tables; rows: the host copy of q_row
static int xp_check(gcnhip_ctx *c, const char *name, const gcnhip_graph *g, const int32_t *q_row, const int32_t *q_class, int nq,
                    const float *h1, int ld_h1, int h, const float *w2, int ld_w2, int C, int scaling, std::vector<int32_t> &rows) {
    if (!c || !g || nq < 0 || (nq > 0 && (!q_row || !q_class)) || !h1 || !w2) XP_REFUSE(name, "invalid argument");
    if (h < 1 || h > XP_MAX_H) XP_REFUSE(name, "1 <= h <= 256");
    if (ld_h1 < h) XP_REFUSE(name, "the row stride of H1 is below h");
    if (C < 1 || ld_w2 < C) XP_REFUSE(name, "the row stride of W2 is below the number of classes");
    if (scaling != 0 && scaling != 1) XP_REFUSE(name, "scaling is 0 (per-edge coefficients) or 1 (the factored form)");
    if ((int)g->h_indptr.size() != g->n_rows + 1) XP_REFUSE(name, "the adjacency object has no host row pointers");
    std::vector<int32_t> cls;
    int rc = xp_download(c, q_row, nq, rows);
    if (rc == 0) rc = xp_download(c, q_class, nq, cls);
    if (rc != 0) return rc;
    for (int i = 0; i < nq; i++) {
        if (rows[i] < 0 || rows[i] >= g->n_rows) XP_REFUSE(name, "a query row outside the adjacency object");
        if (cls[i] < 0 || cls[i] >= C) XP_REFUSE(name, "a query class outside 0 .. C - 1");
    }
    return 0;
}

static XpGraph xp_graph(const gcnhip_graph *g) { return {g->indptr, g->indices, g->coef, g->dinv_row, g->dinv2_row}; }

extern "C" {

int gcnhip_explain_hops(gcnhip_ctx *c, const gcnhip_graph *g, const int32_t *q_row, const int32_t *q_class, int nq, const float *h1,
                        int ld_h1, int h, const float *w2, int ld_w2, int num_classes, int scaling, float *logit, float *hidden,
                        int ld_out, const int32_t *nbr_ptr, int32_t *nbr_row, float *nbr_val, int64_t nbr_capacity) {
    const char *name = "gcnhip_explain_hops";
    std::vector<int32_t> rows, ptr;
    if (int rc = xp_check(c, name, g, q_row, q_class, nq, h1, ld_h1, h, w2, ld_w2, num_classes, scaling, rows)) return rc;
    if (nq == 0) return 0;
    if (!logit || !hidden || !nbr_ptr || !nbr_row || !nbr_val || ld_out < h) XP_REFUSE(name, "invalid argument");
    if (int rc = xp_download(c, nbr_ptr, nq, ptr)) return rc;
    int64_t at = 0;
    for (int i = 0; i < nq; i++) {                             // a wrong scan would write past the lists
        if (ptr[i] != at) XP_REFUSE(name, "nbr_ptr is not the exclusive scan of the queried rows' lengths");
        at += g->h_indptr[rows[i] + 1] - g->h_indptr[rows[i]];
        if (at > INT32_MAX) XP_REFUSE(name, "more than 2^31 - 1 neighbour entries in one launch");
    }
    if (at > nbr_capacity) XP_REFUSE(name, "the neighbour lists are shorter than the queried rows");
    const XpQuery q{q_row, q_class, h1, ld_h1, h, w2, ld_w2, scaling};
    explain_hops_kernel<<<nq, 256, 0, c->stream>>>(xp_graph(g), q, logit, hidden, ld_out, nbr_ptr, nbr_row, nbr_val);
    GCNHIP_LAUNCH_CHECK();
    return 0;
}

int gcnhip_explain_features_agg(gcnhip_ctx *c, const gcnhip_graph *g, const int32_t *q_row, const int32_t *q_class, int nq, const float *h1,
                                int ld_h1, int h, const float *w2, int ld_w2, int num_classes, const float *w1, int ld_w1, int n_features,
                                const float *s, int ld_s, int scaling, float *feat, int ld_f) {
    const char *name = "gcnhip_explain_features_agg";
    std::vector<int32_t> rows;
    if (int rc = xp_check(c, name, g, q_row, q_class, nq, h1, ld_h1, h, w2, ld_w2, num_classes, scaling, rows)) return rc;
    if (!w1 || !s || n_features < 1 || ld_w1 < h || ld_s < n_features || ld_f < n_features || (nq > 0 && !feat)) XP_REFUSE(name, "invalid argument");
    if (nq == 0) return 0;
    const int tiles = ceil_div(n_features, XP_FT);
    if (tiles > 65535) XP_REFUSE(name, "more than 65535 tiles of 64 feature columns");
    const size_t lds = sizeof(float) * ((size_t)h * XP_WLD + (size_t)XP_NC * h + h + 4 * XP_FT) + sizeof(int) * XP_NC;
    if (lds > 64 * 1024) GCNHIP_TRY(hipFuncSetAttribute((const void *)explain_feat_agg_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    const XpQuery q{q_row, q_class, h1, ld_h1, h, w2, ld_w2, scaling};
    explain_feat_agg_kernel<<<dim3(nq, tiles), 256, lds, c->stream>>>(xp_graph(g), q, w1, ld_w1, n_features, s, ld_s, feat, ld_f);
    GCNHIP_LAUNCH_CHECK();
    return 0;
}

int gcnhip_explain_features_walk(gcnhip_ctx *c, const gcnhip_graph *g, const gcnhip_feat *x, const int32_t *q_row, const int32_t *q_class, int nq,
                                 const float *h1, int ld_h1, int h, const float *w2, int ld_w2, int num_classes, const float *w1, int ld_w1,
                                 int scaling, float *feat, int ld_f) {
    const char *name = "gcnhip_explain_features_walk";
    std::vector<int32_t> rows;
    if (int rc = xp_check(c, name, g, q_row, q_class, nq, h1, ld_h1, h, w2, ld_w2, num_classes, scaling, rows)) return rc;
    if (!x || !w1 || ld_w1 < h || (nq > 0 && !feat)) XP_REFUSE(name, "invalid argument");
    if (g->n_cols != g->n_rows) XP_REFUSE(name, "the second hop needs a square adjacency object (every column is a row)");
    if (x->n_rows != g->n_cols) XP_REFUSE(name, "the feature object has another number of rows than the adjacency object");
    if (x->n_cols < 1 || ld_f < x->n_cols) XP_REFUSE(name, "the row stride of feat is below the number of feature columns");
    if (nq == 0) return 0;
    const size_t lds = (size_t)x->n_cols * sizeof(float);
    if (lds > 160 * 1024 - 256) XP_REFUSE(name, "more feature columns than one workgroup's LDS holds (40 896)");
    if (lds > 64 * 1024) GCNHIP_TRY(hipFuncSetAttribute((const void *)explain_feat_walk_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    const XpQuery q{q_row, q_class, h1, ld_h1, h, w2, ld_w2, scaling};
    explain_feat_walk_kernel<<<nq, 64, lds, c->stream>>>(xp_graph(g), q, w1, ld_w1, x->n_cols, x->indptr, x->dense ? nullptr : (const int *)x->indices, x->values,
                                                         feat, ld_f);
    GCNHIP_LAUNCH_CHECK();
    return 0;
}

int gcnhip_explain_abs_colsum(gcnhip_ctx *c, const float *feat, int ld_f, const int32_t *q_class, int nq, int n_features, int num_classes,
                              double *acc, int32_t *count) {
    const char *name = "gcnhip_explain_abs_colsum";
    if (!c || nq < 0 || (nq > 0 && (!feat || !q_class)) || !acc || !count || n_features < 1 || ld_f < n_features) XP_REFUSE(name, "invalid argument");
    if (num_classes < 1 || num_classes > XP_MAX_C) XP_REFUSE(name, "1 <= C <= 256 (a thread keeps its column's sums of every class in LDS)");
    std::vector<int32_t> cls;
    if (int rc = xp_download(c, q_class, nq, cls)) return rc;
    for (int i = 0; i < nq; i++)
        if (cls[i] < 0 || cls[i] >= num_classes) XP_REFUSE(name, "a query class outside 0 .. C - 1");
    if (nq == 0) return 0;
    const size_t lds = (size_t)num_classes * 64 * sizeof(double);
    if (lds > 64 * 1024) GCNHIP_TRY(hipFuncSetAttribute((const void *)explain_abs_colsum_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    explain_abs_colsum_kernel<<<ceil_div(n_features, 64), 64, lds, c->stream>>>(feat, ld_f, q_class, nq, n_features, num_classes, acc, count);
    GCNHIP_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
