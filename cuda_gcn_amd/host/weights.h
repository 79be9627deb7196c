// weights.h — the file of a trained model's weights (beyond the reference, whose program keeps nothing).  Host only: no GPU.
//
// Layout, little-endian:
//   "GCNW" | uint32 version (1) | int32 input_dim F | int32 hidden_dim h | int32 output_dim C
//   | W1 [F x h] f32 row-major | W2 [h x C] f32 row-major | uint32 CRC-32 (IEEE, of every byte before it)
// The size is implied by the widths, so a truncated or padded file is refused, and the CRC catches damaged bytes.
// Adam's moments and step count are not part of the file.
#pragma once
#include <cstdint>
#include <string>

constexpr uint32_t GCN_WEIGHTS_VERSION = 1;

// 0, or -1 with the reason in *err
int gcn_weights_write(const char *path, int F, int h, int C, const float *w1, const float *w2, std::string *err);
// w1 == NULL and w2 == NULL: read and check the file, report its widths in *F, *h, *C.  Otherwise *F, *h, *C are the widths
// of the caller's buffers and must equal the file's (a mismatch is an error: nothing is reshaped); the weights are copied in.
int gcn_weights_read(const char *path, int *F, int *h, int *C, float *w1, float *w2, std::string *err);
uint32_t gcn_crc32(const unsigned char *p, size_t n, uint32_t crc = 0);
