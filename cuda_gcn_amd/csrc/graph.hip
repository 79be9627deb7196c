// graph.hip — the prepared adjacency object: edges, coefficients, row schedule, row subsets.
// Host-side preparation happens ONCE per dataset (the reference re-derives
// degrees per edge per call); its rules are plan.h.
#include "common.h"
#include "plan.h"
#include <math.h>

// coef(e) for every edge, computed once.  One thread per row walks its edges
// (one-time cost; the per-call kernels then stream coef[] coalesced).
__global__ void edge_coef_kernel(const int *__restrict__ indptr, const int *__restrict__ indices,
                                 const int *__restrict__ col_deg, float *__restrict__ coef, int n_rows) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_rows) return;
    const int e0 = indptr[r], e1 = indptr[r + 1];
    const int64_t ds = e1 - e0;
    for (int e = e0; e < e1; e++) {
        const int d = indices[e];
        const int64_t dd = col_deg ? col_deg[d] : (indptr[d + 1] - indptr[d]);
        // module.cpp:91-93: float sqrtf of the integer product, divide in double, narrow
        coef[e] = (float)(1.0 / (double)sqrtf((float)(ds * dd)));
    }
}

// the tasks of the full schedule whose row is in the subset, same order, same segment slots
static int build_rowset(gcnhip_rowset *rs, const gcnhip_graph *g) {
    const plan::Schedule s = plan::filter_rows(g->h_tasks, g->h_srows, rs->bits);
    rs->n_tasks = (int)s.tasks.size();
    rs->n_split_rows = (int)s.split.size();
    plan::xcd_bounds(s.tasks, rs->bounds);
    return upload_lists(s.tasks, s.split, rs->tasks, rs->split_rows);
}

// (Re)build the row schedule: the task list of a given row order; a row
// above SPLIT_EDGES becomes consecutive segments whose partial sums a second kernel adds in order.
static int build_tasks(gcnhip_graph *g, const std::vector<int> &order) {
    const int SPLIT_EDGES = plan::split_length(g->nnz, g->split_edges_opt);
    plan::Schedule s = plan::cut_segments(g->h_indptr.data(), order.data(), g->n_rows, SPLIT_EDGES);
    g->n_tasks = (int)s.tasks.size();
    g->n_split_rows = (int)s.split.size();
    g->n_slots = s.n_slots;
    GCNHIP_TRY((hipError_t)upload_lists(s.tasks, s.split, g->tasks, g->split_rows));
    // segment scratch for the widest aggregation this object will serve: sized HERE (and by
    // gcnhip_graph_reserve_width), never inside a launch path
    g->partials.reset();
    if (g->part_ld < 256) g->part_ld = 256;
    if (g->n_slots) GCNHIP_TRY(g->partials.alloc((size_t)g->n_slots * g->part_ld));
    plan::xcd_bounds(s.tasks, g->bounds);
    g->h_tasks = std::move(s.tasks);
    g->h_srows = std::move(s.split);
    for (auto &rs : g->rowsets) {
        const int rc = build_rowset(rs.get(), g);
        if (rc != 0) return rc;
    }
    return 0;
}

extern "C" {

int gcnhip_graph_create(gcnhip_ctx *c, gcnhip_graph **out, const int *h_indptr, const int *h_indices,
                        int n_rows, int n_cols, const int *h_col_deg) {
    return gcnhip_graph_create_grouped(c, out, h_indptr, h_indices, n_rows, n_cols, h_col_deg, nullptr);
}

int gcnhip_graph_create_grouped(gcnhip_ctx *c, gcnhip_graph **out, const int *h_indptr, const int *h_indices,
                                int n_rows, int n_cols, const int *h_col_deg, const int *h_row_group) {
    if (!c || !out || !h_indptr || n_rows < 0) return -1;
    if (!h_col_deg && n_cols != n_rows) return -1;
    if (!plan::valid_csr(h_indptr, h_indices, n_rows, n_cols)) return -1;
    GCNHIP_TRY(hipSetDevice(c->device));
    std::unique_ptr<gcnhip_graph> g(new gcnhip_graph());
    const int nnz = h_indptr[n_rows];
    g->n_rows = n_rows; g->n_cols = n_cols; g->nnz = nnz;
    g->split_edges_opt = c->opt.split_edges;
    GCNHIP_TRY(g->indptr.upload(h_indptr, (size_t)n_rows + 1));
    std::vector<int> sorted_idx(h_indices, h_indices + nnz);      // every row's neighbours in gather order
    plan::sort_neighbours(h_indptr, n_rows, h_col_deg, sorted_idx, plan::sort_threads(nnz));
    GCNHIP_TRY(g->indices.upload(sorted_idx.data(), (size_t)nnz));
    GCNHIP_TRY(g->coef.alloc((size_t)std::max(nnz, 1)));
    DevBuf<int> d_col_deg;
    if (h_col_deg) GCNHIP_TRY(d_col_deg.upload(h_col_deg, (size_t)n_cols));
    if (n_rows) {
        edge_coef_kernel<<<ceil_div(n_rows, 256), 256, 0, c->stream>>>(g->indptr, g->indices, d_col_deg, g->coef, n_rows);
        GCNHIP_LAUNCH_CHECK();
    }
    GCNHIP_TRY(hipStreamSynchronize(c->stream));
    d_col_deg.reset();

    g->h_indptr.assign(h_indptr, h_indptr + n_rows + 1);
    {   // the factored form of the coefficients: per-row and per-column 1/sqrt(deg) and 1/deg
        std::vector<float> dr((size_t)std::max(n_rows, 1)), dr2(dr.size()), dc((size_t)std::max(n_cols, 1)), dc2(dc.size());
        for (int r = 0; r < n_rows; r++) {
            const double d = (double)std::max(1, h_indptr[r + 1] - h_indptr[r]);
            dr[r] = (float)(1.0 / sqrt(d)); dr2[r] = (float)(1.0 / d);
        }
        for (int j = 0; j < n_cols; j++) {
            const double d = (double)std::max(1, h_col_deg ? h_col_deg[j] : h_indptr[j + 1] - h_indptr[j]);
            dc[j] = (float)(1.0 / sqrt(d)); dc2[j] = (float)(1.0 / d);
        }
        GCNHIP_TRY(g->dinv_row.upload(dr.data(), dr.size()));
        GCNHIP_TRY(g->dinv2_row.upload(dr2.data(), dr.size()));
        GCNHIP_TRY(g->dinv_col.upload(dc.data(), dc.size()));
        GCNHIP_TRY(g->dinv2_col.upload(dc2.data(), dc.size()));
    }
    GCNHIP_TRY((hipError_t)build_tasks(g.get(), plan::row_order(h_indptr, n_rows, h_row_group)));
    *out = g.release();
    return 0;
}

// A second object from a parent: its row count, factors (degrees of the FULL graph), scratch width, split option and current
// row order, and its OWN task lists and split-row scratch (two streams may aggregate at the same time only through different
// objects).  h_col_bits == nullptr: every edge, by device-to-device copies —
// none of the host preparation of gcnhip_graph_create (validation, per-row neighbour sort, coefficient kernel) is repeated.
// Otherwise the edges whose column has its bit set, filtered on the host from the parent's edges as it stores them
// (neighbours by descending degree) with ITS coefficients.
static int graph_from_parent(gcnhip_ctx *c, gcnhip_graph **out, const gcnhip_graph *parent, const uint32_t *h_col_bits) {
    GCNHIP_TRY(hipSetDevice(c->device));
    GCNHIP_TRY(hipStreamSynchronize(c->stream));
    const int n_rows = parent->n_rows, n_cols = parent->n_cols, nnz = parent->nnz;
    std::unique_ptr<gcnhip_graph> g(new gcnhip_graph());
    g->n_rows = n_rows; g->n_cols = n_cols; g->nnz = nnz;
    g->part_ld = parent->part_ld;
    g->split_edges_opt = parent->split_edges_opt;
    g->h_indptr = parent->h_indptr;
    if (!h_col_bits) {
        GCNHIP_TRY(g->indptr.copy_from(parent->indptr, (size_t)n_rows + 1));
        GCNHIP_TRY(g->indices.copy_from(parent->indices, (size_t)nnz));
        GCNHIP_TRY(g->coef.copy_from(parent->coef, (size_t)nnz));
    } else {
        std::vector<int> idx((size_t)std::max(nnz, 1));
        std::vector<float> cf((size_t)std::max(nnz, 1));
        if (nnz) {
            GCNHIP_TRY(hipMemcpy(idx.data(), parent->indices, (size_t)nnz * sizeof(int), hipMemcpyDeviceToHost));
            GCNHIP_TRY(hipMemcpy(cf.data(), parent->coef, (size_t)nnz * sizeof(float), hipMemcpyDeviceToHost));
        }
        g->h_indptr = plan::restrict_edges(parent->h_indptr.data(), n_rows, h_col_bits, idx.data(), cf.data());
        g->nnz = g->h_indptr[n_rows];
        GCNHIP_TRY(g->indptr.upload(g->h_indptr.data(), (size_t)n_rows + 1));
        GCNHIP_TRY(g->indices.upload(idx.data(), (size_t)g->nnz));
        GCNHIP_TRY(g->coef.upload(cf.data(), (size_t)g->nnz));
    }
    GCNHIP_TRY(g->dinv_row.copy_from(parent->dinv_row, (size_t)std::max(n_rows, 1)));
    GCNHIP_TRY(g->dinv2_row.copy_from(parent->dinv2_row, (size_t)std::max(n_rows, 1)));
    GCNHIP_TRY(g->dinv_col.copy_from(parent->dinv_col, (size_t)std::max(n_cols, 1)));
    GCNHIP_TRY(g->dinv2_col.copy_from(parent->dinv2_col, (size_t)std::max(n_cols, 1)));
    const std::vector<int> order = plan::order_of(parent->h_tasks, n_rows);
    if ((int)order.size() != n_rows) return -1;
    GCNHIP_TRY((hipError_t)build_tasks(g.get(), order));
    *out = g.release();
    return 0;
}

int gcnhip_graph_create_restricted(gcnhip_ctx *c, gcnhip_graph **out, const gcnhip_graph *parent, const uint32_t *h_col_bits) {
    if (!c || !out || !parent || !h_col_bits || parent->h_indptr.empty()) return -1;
    return graph_from_parent(c, out, parent, h_col_bits);
}
int gcnhip_graph_clone(gcnhip_ctx *c, gcnhip_graph **out, const gcnhip_graph *parent) {
    if (!c || !out || !parent || parent->h_indptr.empty()) return -1;
    return graph_from_parent(c, out, parent, nullptr);
}

int gcnhip_graph_destroy(gcnhip_ctx *c, gcnhip_graph *g) {
    if (!g) return 0;
    hipSetDevice(c->device);
    delete g;
    return 0;
}

int gcnhip_graph_set_schedule(gcnhip_ctx *c, gcnhip_graph *g, int mode, const int *h_row_group, int n_groups) {
    if (!c || !g || g->h_indptr.empty() || mode < 0 || mode > 2) return -1;
    if (mode == 1 && !h_row_group) return -1;
    if (mode == 2 && n_groups < 1) return -1;
    GCNHIP_TRY(hipSetDevice(c->device));
    GCNHIP_TRY(hipStreamSynchronize(c->stream));       // no aggregation may still be reading the old task list
    return build_tasks(g, plan::schedule_order(g->h_indptr.data(), g->n_rows, mode, h_row_group, n_groups));
}

int gcnhip_graph_add_rowset(gcnhip_ctx *c, gcnhip_graph *g, const uint32_t *h_row_bits, gcnhip_rowset **out) {
    if (!c || !g || !h_row_bits || !out || g->h_indptr.empty()) return -1;
    GCNHIP_TRY(hipSetDevice(c->device));
    std::unique_ptr<gcnhip_rowset> rs(new gcnhip_rowset());
    rs->owner = g;
    rs->bits.assign(h_row_bits, h_row_bits + ((size_t)g->n_rows + 31) / 32);   // exactly the n_rows bits the header documents
    rs->bits.push_back(0u);                                                       // (+ a zero word: row ids index it as r >> 5 with r < n_rows)
    GCNHIP_TRY((hipError_t)build_rowset(rs.get(), g));
    *out = rs.get();
    g->rowsets.push_back(std::move(rs));
    return 0;
}
int gcnhip_graph_remove_rowset(gcnhip_ctx *c, gcnhip_graph *g, gcnhip_rowset *rs) {
    if (!c || !g || !rs) return -1;
    if (rs->owner != g) return gcnhip_fail("gcnhip_graph_remove_rowset: the row subset was registered on another adjacency object");
    auto it = std::find_if(g->rowsets.begin(), g->rowsets.end(), [&](const std::unique_ptr<gcnhip_rowset> &p) { return p.get() == rs; });
    if (it == g->rowsets.end()) return -1;
    GCNHIP_TRY(hipSetDevice(c->device));
    GCNHIP_TRY(hipStreamSynchronize(c->stream));       // no aggregation of this context may still be reading its task list
    g->rowsets.erase(it);
    return 0;
}
int gcnhip_rowset_size(const gcnhip_rowset *rs, int *n_rows_tasks) {
    if (!rs || !n_rows_tasks) return -1;
    *n_rows_tasks = rs->n_tasks;
    return 0;
}

int gcnhip_graph_reserve_width(gcnhip_ctx *c, gcnhip_graph *g, int max_dim) {
    if (!c || !g || max_dim <= 0) return -1;
    const int want = (max_dim + 7) / 8 * 8;
    if (want <= g->part_ld) return 0;
    GCNHIP_TRY(hipSetDevice(c->device));
    GCNHIP_TRY(hipStreamSynchronize(c->stream));       // no aggregation may still be writing the old scratch
    g->partials.reset();
    g->part_ld = want;
    if (g->n_slots) GCNHIP_TRY(g->partials.alloc((size_t)g->n_slots * g->part_ld));
    return 0;
}

int gcnhip_graph_scales(const gcnhip_graph *g, const float **dinv_row, const float **dinv2_row, const float **dinv_col, const float **dinv2_col) {
    if (!g) return -1;
    if (dinv_row) *dinv_row = g->dinv_row;
    if (dinv2_row) *dinv2_row = g->dinv2_row;
    if (dinv_col) *dinv_col = g->dinv_col;
    if (dinv2_col) *dinv2_col = g->dinv2_col;
    return 0;
}

int gcnhip_graph_arrays(const gcnhip_graph *g, const int **d_indptr, const int **d_indices,
                        const float **d_coef, int *n_rows, int *nnz) {
    if (!g) return -1;
    if (d_indptr) *d_indptr = g->indptr;
    if (d_indices) *d_indices = g->indices;
    if (d_coef) *d_coef = g->coef;
    if (n_rows) *n_rows = g->n_rows;
    if (nnz) *nnz = g->nnz;
    return 0;
}

}  // extern "C"
