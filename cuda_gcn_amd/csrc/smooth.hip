// smooth.hip — the row-local steps of Correct & Smooth (Huang et al., 2020) around the blend aggregation
// (gcnhip_graphsum_blend, graphsum.hip).  Beyond the reference, which stops at the accuracy of the raw forward.
//
// Layout: bce.hip's — one wave64 per row, lane j on class j (C <= 64: a row is one register), so rows of any stride are
// read coalesced and nothing but |e| is reduced across a row.  The residual norm sum |E| is deterministic: per-lane in row
// order, a fixed shuffle tree, block partials added in block order by a one-block finalize launch; the grid depends on
// the row count alone, so two launches give the same bits.
#include "common.h"
#pragma clang fp contract(off)

constexpr int CS_MAX_BLOCKS = 1024;      // the partials sit where bce.hip's do: red_f[2048, 3072), red_i[0, 1024)

// E[r, j] = [j == truth[r]] - exp(logp[r, j]) for the listed rows whose truth is a class; E was zeroed before
__global__ __launch_bounds__(256) void cs_error_kernel(const float *logp, int ld_logp, const int32_t *truth, const int32_t *rows, int n_listed,
                                                       int n_table, int C, float *E, int ld_e, float *part_f, int32_t *part_i) {
    __shared__ float sh_f[4];
    __shared__ int sh_i[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int waves_total = gridDim.x * 4;
    float sum = 0.f;
    int cnt = 0;
    for (int q = blockIdx.x * 4 + wave; q < n_listed; q += waves_total) {
        const int r = rows ? rows[q] : q;
        if (r < 0 || r >= n_table) continue;              // wave-uniform: no row id can index past the tables
        const int t = truth[r];
        if (t < 0 || t >= C) continue;
        if (lane < C) {
            const float e = (lane == t ? 1.f : 0.f) - expf(logp[(size_t)r * ld_logp + lane]);
            E[(size_t)r * ld_e + lane] = e;
            sum += fabsf(e);
        }
        cnt += lane == 0;
    }
    sum = wave_sum(sum);
    cnt = wave_sum_i(cnt);
    if (lane == 0) { sh_f[wave] = sum; sh_i[wave] = cnt; }
    __syncthreads();
    if (threadIdx.x == 0) {
        part_f[blockIdx.x] = (sh_f[0] + sh_f[1]) + (sh_f[2] + sh_f[3]);
        part_i[blockIdx.x] = sh_i[0] + sh_i[1] + sh_i[2] + sh_i[3];
    }
}

// block partials in block order (thread 0 alone: at most 1024 adds) -> sigma = {sum |E|, rows}
__global__ void cs_error_finalize_kernel(const float *part_f, const int32_t *part_i, int n, float *sigma) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    float s = 0.f;
    int k = 0;
    for (int i = 0; i < n; i++) { s += part_f[i]; k += part_i[i]; }
    sigma[0] = s;
    sigma[1] = (float)k;
}

// G0[r, :] = onehot(truth[r]) where truth[r] is a class, else exp(logp[r, :]) + s . Ehat[r, :], s = sigma / sum_j |Ehat[r, j]|
// (1 unless s <= 1000: a zero row, inf and NaN included), sigma = d_sigma[0] / d_sigma[1]
__global__ __launch_bounds__(256) void cs_correct_kernel(const float *logp, int ld_logp, const float *eh, int ld_e, const int32_t *truth, int n_table,
                                                         int C, const float *d_sigma, float *G0, int ld_g) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= n_table) return;                             // whole waves leave together
    const int t = truth[r];
    float out;
    if (t >= 0 && t < C) {
        out = lane == t ? 1.f : 0.f;
    } else {
        const float e = lane < C ? eh[(size_t)r * ld_e + lane] : 0.f;
        const float norm = wave_sum(fabsf(e));
        float s = (d_sigma[0] / d_sigma[1]) / norm;
        if (!(s <= 1000.f)) s = 1.f;
        out = lane < C ? expf(logp[(size_t)r * ld_logp + lane]) + s * e : 0.f;
    }
    if (lane < C) G0[(size_t)r * ld_g + lane] = out;
}

extern "C" {

int gcnhip_cs_error_rows(gcnhip_ctx *c, const float *logp, int ld_logp, const int32_t *truth, int n_table, const int32_t *d_rows, int n_listed,
                         int num_classes, float *e, int ld_e, float *d_sigma) {
    if (!c || !logp || !truth || !e || !d_sigma || n_table < 0 || n_listed < 0) return gcnhip_fail("gcnhip_cs_error_rows: invalid argument");
    if (num_classes < 1 || num_classes > WAVE) return gcnhip_fail("gcnhip_cs_error_rows: 1 <= num_classes <= 64 (lane j holds class j)");
    if (ld_logp < num_classes || ld_e < num_classes) return gcnhip_fail("gcnhip_cs_error_rows: a row stride is below num_classes");
    if (!d_rows && n_listed > n_table) return gcnhip_fail("gcnhip_cs_error_rows: without a row list n_listed is at most n_table");
    if (n_table) GCNHIP_TRY(hipMemsetAsync(e, 0, (size_t)n_table * ld_e * sizeof(float), c->stream));
    int blocks = ceil_div(n_listed, 4 * 4);
    if (blocks > CS_MAX_BLOCKS) blocks = CS_MAX_BLOCKS;
    if (blocks < 1) blocks = 1;
    float *part_f = c->red_f + 2048;
    int32_t *part_i = c->red_i;
    cs_error_kernel<<<blocks, 256, 0, c->stream>>>(logp, ld_logp, truth, d_rows, n_listed, n_table, num_classes, e, ld_e, part_f, part_i);
    GCNHIP_LAUNCH_CHECK();
    cs_error_finalize_kernel<<<1, 64, 0, c->stream>>>(part_f, part_i, blocks, d_sigma);
    GCNHIP_LAUNCH_CHECK();
    return 0;
}

int gcnhip_cs_correct_rows(gcnhip_ctx *c, const float *logp, int ld_logp, const float *e_hat, int ld_e, const int32_t *truth, int n_table,
                           int num_classes, const float *d_sigma, float *g0, int ld_g) {
    if (!c || !logp || !e_hat || !truth || !d_sigma || !g0 || n_table < 0) return gcnhip_fail("gcnhip_cs_correct_rows: invalid argument");
    if (num_classes < 1 || num_classes > WAVE) return gcnhip_fail("gcnhip_cs_correct_rows: 1 <= num_classes <= 64 (lane j holds class j)");
    if (ld_logp < num_classes || ld_e < num_classes || ld_g < num_classes) return gcnhip_fail("gcnhip_cs_correct_rows: a row stride is below num_classes");
    if (g0 == e_hat) return gcnhip_fail("gcnhip_cs_correct_rows: g0 must not be e_hat");
    if (n_table == 0) return 0;
    cs_correct_kernel<<<ceil_div(n_table, 4), 256, 0, c->stream>>>(logp, ld_logp, e_hat, ld_e, truth, n_table, num_classes, d_sigma, g0, ld_g);
    GCNHIP_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
