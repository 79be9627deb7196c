// feat.hip — the prepared feature object: X on the device once per dataset (the reference re-uploads it
// every epoch), its CSC view and the task list of the weight gradient; the host rules are plan.h.
#include "common.h"
#include "plan.h"

extern "C" {

// values[e] *= scale[row of e]: the feature matrix of the factored first layer, (D^-1/2 X) — see gcnhip_graphsum_ex
__global__ void feat_scale_rows_kernel(float *vals, float *vals_pad, int ld_pad, const int *indptr, const float *scale, int n_rows, int n_cols, int dense) {
    const int r = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (r >= n_rows) return;
    const float s = scale[r];
    const int lane = threadIdx.x & 63;
    for (int e = indptr[r] + lane; e < indptr[r + 1]; e += 64) vals[e] *= s;
    if (vals_pad && dense)
        for (int k = lane; k < n_cols; k += 64) vals_pad[(size_t)r * ld_pad + k] *= s;
}
__global__ void feat_scale_csc_kernel(float *csc_val, const int *csc_row, const float *scale, int64_t nnz) {
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q < nnz) csc_val[q] *= scale[csc_row[q]];
}
int gcnhip_feat_scale_rows(gcnhip_ctx *c, gcnhip_feat *f, const float *d_row_scale) {
    if (!c || !f || !d_row_scale) return -1;
    if (f->n_rows == 0) return 0;
    feat_scale_rows_kernel<<<ceil_div(f->n_rows, 4), 256, 0, c->stream>>>(f->values, f->values_pad, f->ld_pad, f->indptr, d_row_scale, f->n_rows, f->n_cols, f->dense ? 1 : 0);
    GCNHIP_LAUNCH_CHECK();
    if (f->csc_val && f->nnz) {
        feat_scale_csc_kernel<<<ceil_div(f->nnz, 256), 256, 0, c->stream>>>(f->csc_val, f->csc_row, d_row_scale, f->nnz);
        GCNHIP_LAUNCH_CHECK();
    }
    GCNHIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

int gcnhip_feat_create(gcnhip_ctx *c, gcnhip_feat **out, const int *h_indptr, const int *h_indices,
                       const float *h_values, int n_rows, int n_cols) {
    if (!c || !out || !h_indptr || !h_values || n_rows < 0 || n_cols <= 0) return -1;
    GCNHIP_TRY(hipSetDevice(c->device));
    std::unique_ptr<gcnhip_feat> f(new gcnhip_feat());
    f->n_rows = n_rows; f->n_cols = n_cols;
    const int64_t nnz = h_indptr[n_rows];
    f->nnz = nnz;
    const bool dense = plan::dense_layout(h_indptr, h_indices, n_rows, n_cols);
    if (!h_indices && !dense) return -1;
    f->dense = dense;
    GCNHIP_TRY(f->indptr.upload(h_indptr, (size_t)n_rows + 1));
    GCNHIP_TRY(f->values.alloc((size_t)std::max<int64_t>(nnz, 4)));
    if (nnz) GCNHIP_TRY(hipMemcpy(f->values, h_values, (size_t)nnz * sizeof(float), hipMemcpyHostToDevice));
    {   // flat: a bit per stored element; chunk-major (dense X, dense_bf16x3.h): a word per row and 32 columns.  Slack: tiles read bits of pad columns
        const size_t words_cm = dense ? (size_t)n_rows * ((n_cols + 31) / 32) : 0;
        GCNHIP_TRY(f->keep_bits.alloc(std::max((size_t)(nnz / 32), words_cm) + 32));
    }
    if (dense && n_cols % 128 != 0 && n_cols >= 64) {
        // the MFMA tiles stage X with unconditional 16-byte lane loads when every row starts on a 16-byte
        // boundary and its stride covers whole 128-column tiles (zero padded); HBM has room for the second copy
        f->ld_pad = (n_cols + 127) / 128 * 128;
        GCNHIP_TRY(f->values_pad.alloc((size_t)n_rows * f->ld_pad));
        GCNHIP_TRY(hipMemset(f->values_pad, 0, (size_t)n_rows * f->ld_pad * sizeof(float)));
        GCNHIP_TRY(hipMemcpy2D(f->values_pad, (size_t)f->ld_pad * sizeof(float), f->values, (size_t)n_cols * sizeof(float),
                               (size_t)n_cols * sizeof(float), (size_t)n_rows, hipMemcpyDeviceToDevice));
        // a device memset and a device-to-device copy return before they have run, on the null stream, which the context's
        // non-blocking stream does not wait for: a product launched straight after the object is made (predict_new) must
        // find the padded image complete
        GCNHIP_TRY(hipStreamSynchronize(nullptr));
    }
    if (!dense) {
        if (!plan::indices_in_range(h_indices, nnz, n_cols)) return -1;
        GCNHIP_TRY(f->indices.upload(h_indices, (size_t)nnz));
        const plan::Csc csc = plan::csc_sort(h_indptr, h_indices, n_rows, n_cols);
        GCNHIP_TRY(f->csc_ptr.upload(csc.ptr.data(), csc.ptr.size()));
        GCNHIP_TRY(f->csc_row.upload(csc.row.data(), (size_t)nnz));
        GCNHIP_TRY(f->csc_pos.upload(csc.pos.data(), (size_t)nnz));
        if (nnz) {
            std::vector<float> cv((size_t)nnz);
            for (int64_t q = 0; q < nnz; q++) cv[q] = h_values[csc.pos[q]];
            GCNHIP_TRY(f->csc_val.upload(cv.data(), (size_t)nnz));
        }
        f->bwd_nw = plan::column_waves(nnz, n_cols, c->opt.spmm_nw);
        const plan::Schedule s = plan::cut_segments(csc.ptr.data(), nullptr, n_cols, plan::column_segment(f->bwd_nw));
        f->n_bwd_tasks = (int)s.tasks.size(); f->n_bwd_split = (int)s.split.size(); f->n_bwd_slots = s.n_slots;
        GCNHIP_TRY((hipError_t)upload_lists(s.tasks, s.split, f->bwd_tasks, f->bwd_split));
    }
    *out = f.release();
    return 0;
}

// A^.X for a dense X, computed once: the feature object of an evaluation forward that aggregates first.
int gcnhip_feat_create_aggregated(gcnhip_ctx *c, gcnhip_feat **out, gcnhip_graph *g, const gcnhip_feat *x) {
    if (!c || !out || !g || !x || !x->dense || x->n_rows != g->n_cols) return -1;
    GCNHIP_TRY(hipSetDevice(c->device));
    std::unique_ptr<gcnhip_feat> f(new gcnhip_feat());
    const int F = x->n_cols, n = g->n_rows;
    f->n_rows = n; f->n_cols = F; f->nnz = (int64_t)n * F; f->dense = true;
    std::vector<int> ip((size_t)n + 1);
    for (int r = 0; r <= n; r++) ip[r] = (int)((int64_t)r * F);
    GCNHIP_TRY(f->indptr.upload(ip.data(), (size_t)n + 1));
    GCNHIP_TRY(f->values.alloc((size_t)std::max<int64_t>(f->nnz, 4)));
    // no keep-bit array: an aggregated feature object serves evaluation forwards only (no dropout); a dropout call on it
    // is refused in spmm.hip
    int rc = gcnhip_graph_reserve_width(c, g, F);
    if (rc != 0) return rc;
    const float *src = x->values_pad ? x->values_pad : x->values;
    const int ld_src = x->values_pad ? x->ld_pad : F;
    if (x->values_pad) {                          // keep the padded, 16-byte aligned layout the MFMA tiles read
        f->ld_pad = x->ld_pad;
        GCNHIP_TRY(f->values_pad.alloc((size_t)n * f->ld_pad));
        GCNHIP_TRY(hipMemsetAsync(f->values_pad, 0, (size_t)n * f->ld_pad * sizeof(float), c->stream));
        rc = gcnhip_graphsum(c, g, src, ld_src, f->values_pad, f->ld_pad, F);
        if (rc != 0) return rc;
        GCNHIP_TRY(hipMemcpy2DAsync(f->values, (size_t)F * sizeof(float), f->values_pad, (size_t)f->ld_pad * sizeof(float),
                                    (size_t)F * sizeof(float), (size_t)n, hipMemcpyDeviceToDevice, c->stream));
    } else {
        rc = gcnhip_graphsum(c, g, src, ld_src, f->values, F, F);
        if (rc != 0) return rc;
    }
    GCNHIP_TRY(hipStreamSynchronize(c->stream));
    *out = f.release();
    return 0;
}

int gcnhip_feat_destroy(gcnhip_ctx *c, gcnhip_feat *f) {
    if (!f) return 0;
    hipSetDevice(c->device);
    delete f;
    return 0;
}
int gcnhip_feat_is_dense(const gcnhip_feat *f) { return f && f->dense ? 1 : 0; }
const float *gcnhip_feat_values(const gcnhip_feat *f) { return f ? f->values : nullptr; }
int64_t gcnhip_feat_nnz(const gcnhip_feat *f) { return f ? f->nnz : 0; }

}  // extern "C"
