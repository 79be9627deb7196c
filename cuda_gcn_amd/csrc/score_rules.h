// score_rules.h — the rules that more than one file scores a logit by, each defined once: the order-preserving key of an f32
// and the searches in a sorted key column (ranking.hip, thresholds.hip), the sigmoid of a multi-label probability (bce.hip,
// thresholds.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

constexpr uint32_t RANK_SENTINEL = 0xFFFFFFFFu;                // no score's key: the padding of the key tables

// key(s) from the bits of s (not a NaN): -0.0 is +0.0 first; then ~b when the sign bit is set and b | 0x80000000 otherwise
__device__ __forceinline__ uint32_t rank_key(uint32_t b) {
    if (b == 0x80000000u) b = 0u;                              // -0.0 == +0.0
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
// the bits of the float a key came from (+0.0 for the key of either zero)
__device__ __forceinline__ uint32_t rank_key_bits(uint32_t k) { return (k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k; }

__device__ inline int rank_lower_bound(const uint32_t *a, int n, uint32_t k) {    // #{a < k}
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (a[mid] < k) lo = mid + 1; else hi = mid;
    }
    return lo;
}
__device__ inline int rank_upper_bound(const uint32_t *a, int n, uint32_t k) {    // #{a <= k}
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (a[mid] <= k) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__device__ inline float bce_sigmoid(float z) {
    if (z >= 0.f) return 1.f / (1.f + expf(-z));
    const float e = expf(z);
    return e / (1.f + e);
}
