// tsne_pack.h — the layout of the packed image gcnhip_tsne_pack makes of a table's listed rows, shared by the code objects that walk
// it (tsne.hip, which owns the pack kernel, and dbscan.hip): {header | X [n_pad x DP] | S [n_pad] | valid [n_pad]}, n_pad = n
// rounded up to 64, DP = dim rounded up to 16, 32, 64, 128 or 256 (zero padded), S = {xn, beta, m, 1 / Z} in f32, header int32 [0] =
// the points.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <hip/hip_runtime.h>

constexpr int TS_MAX_DIM = 256;
constexpr int TS_RT = 64;                         // list positions per row tile
constexpr int TS_HDR = 256;                       // bytes of the pack's header: int32 [0] = the points

static inline int ts_dp(int dim) { return dim <= 16 ? 16 : dim <= 32 ? 32 : dim <= 64 ? 64 : dim <= 128 ? 128 : 256; }
static inline int ts_npad(int n) { return std::max((n + TS_RT - 1) / TS_RT, 1) * TS_RT; }

struct TsPack {
    int32_t *hdr;
    float *X;
    float4 *S;
    int32_t *valid;
    size_t bytes;
};
static inline TsPack ts_pack(void *pack, int n, int dim) {
    const size_t n_pad = (size_t)ts_npad(n), dp = (size_t)ts_dp(dim);
    unsigned char *b = (unsigned char *)pack;
    TsPack P;
    P.hdr = (int32_t *)b;
    P.X = (float *)(b + TS_HDR);
    P.S = (float4 *)(b + TS_HDR + n_pad * dp * sizeof(float));
    P.valid = (int32_t *)(b + TS_HDR + n_pad * dp * sizeof(float) + n_pad * sizeof(float4));
    P.bytes = TS_HDR + n_pad * dp * sizeof(float) + n_pad * sizeof(float4) + n_pad * sizeof(int32_t);
    return P;
}
