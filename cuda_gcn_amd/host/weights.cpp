// weights.cpp — the weights file (weights.h)
#include "weights.h"
#include <cstdio>
#include <cstring>
#include <vector>

uint32_t gcn_crc32(const unsigned char *p, size_t n, uint32_t crc) {
    static uint32_t table[256];
    static bool ready = false;
    if (!ready) {                                            // (benign race: every thread writes the same values)
        for (uint32_t i = 0; i < 256; i++) {
            uint32_t c = i;
            for (int k = 0; k < 8; k++) c = (c & 1) ? 0xEDB88320u ^ (c >> 1) : c >> 1;
            table[i] = c;
        }
        ready = true;
    }
    crc = ~crc;
    for (size_t i = 0; i < n; i++) crc = table[(crc ^ p[i]) & 0xFF] ^ (crc >> 8);
    return ~crc;
}

static void put_u32(std::vector<unsigned char> &b, uint32_t v) {
    for (int k = 0; k < 4; k++) b.push_back((unsigned char)(v >> (8 * k)));
}
static uint32_t get_u32(const unsigned char *p) {
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}
static void put_f32s(std::vector<unsigned char> &b, const float *v, size_t n) {
    for (size_t i = 0; i < n; i++) {
        uint32_t u;
        memcpy(&u, &v[i], 4);
        put_u32(b, u);
    }
}
static void get_f32s(const unsigned char *p, float *v, size_t n) {
    for (size_t i = 0; i < n; i++) {
        const uint32_t u = get_u32(p + 4 * i);
        memcpy(&v[i], &u, 4);
    }
}

static constexpr size_t HEADER_BYTES = 20;                  // magic, version, three widths

static int fail(std::string *err, const std::string &msg) {
    if (err) *err = msg;
    return -1;
}

int gcn_weights_write(const char *path, int F, int h, int C, const float *w1, const float *w2, std::string *err) {
    if (!path || F <= 0 || h <= 0 || C <= 0 || !w1 || !w2) return fail(err, "gcn_weights_write: invalid argument");
    const size_t n1 = (size_t)F * h, n2 = (size_t)h * C;
    std::vector<unsigned char> b;
    b.reserve(HEADER_BYTES + 4 * (n1 + n2) + 4);
    b.insert(b.end(), {'G', 'C', 'N', 'W'});
    put_u32(b, GCN_WEIGHTS_VERSION);
    put_u32(b, (uint32_t)F); put_u32(b, (uint32_t)h); put_u32(b, (uint32_t)C);
    put_f32s(b, w1, n1);
    put_f32s(b, w2, n2);
    put_u32(b, gcn_crc32(b.data(), b.size()));
    FILE *f = fopen(path, "wb");
    if (!f) return fail(err, std::string("gcn_weights_write: cannot open ") + path + " for writing");
    const bool ok = fwrite(b.data(), 1, b.size(), f) == b.size();
    if (fclose(f) != 0 || !ok) return fail(err, std::string("gcn_weights_write: could not write ") + path);
    return 0;
}

int gcn_weights_read(const char *path, int *F, int *h, int *C, float *w1, float *w2, std::string *err) {
    if (!path || !F || !h || !C || (!w1) != (!w2)) return fail(err, "gcn_weights_read: invalid argument");
    FILE *f = fopen(path, "rb");
    if (!f) return fail(err, std::string("gcn_weights_read: cannot open ") + path);
    std::vector<unsigned char> b;
    unsigned char buf[1 << 16];
    size_t got;
    while ((got = fread(buf, 1, sizeof buf, f)) > 0) b.insert(b.end(), buf, buf + got);
    fclose(f);
    const std::string where = std::string(" (") + path + ")";
    if (b.size() < HEADER_BYTES + 4 || memcmp(b.data(), "GCNW", 4) != 0)
        return fail(err, "gcn_weights_read: not a weights file: no GCNW header" + where);
    const uint32_t version = get_u32(&b[4]);
    if (version != GCN_WEIGHTS_VERSION)
        return fail(err, "gcn_weights_read: format version " + std::to_string(version) + ", this build reads version " +
                             std::to_string(GCN_WEIGHTS_VERSION) + where);
    const int32_t fF = (int32_t)get_u32(&b[8]), fh = (int32_t)get_u32(&b[12]), fC = (int32_t)get_u32(&b[16]);
    if (fF <= 0 || fh <= 0 || fC <= 0) return fail(err, "gcn_weights_read: widths in the header are not positive" + where);
    const size_t n1 = (size_t)fF * fh, n2 = (size_t)fh * fC;
    const size_t want = HEADER_BYTES + 4 * (n1 + n2) + 4;  // (n1, n2 < 2^62: no overflow; absurd widths fail the size test)
    if (n1 > b.size() || n2 > b.size() || b.size() != want)
        return fail(err, "gcn_weights_read: the file has " + std::to_string(b.size()) + " bytes, its widths " + std::to_string(fF) + " x " +
                             std::to_string(fh) + " x " + std::to_string(fC) + " need " + std::to_string(want) + " (truncated or damaged)" + where);
    if (gcn_crc32(b.data(), want - 4) != get_u32(&b[want - 4])) return fail(err, "gcn_weights_read: CRC-32 mismatch (damaged file)" + where);
    if (!w1) {
        *F = fF; *h = fh; *C = fC;
        return 0;
    }
    if (*F != fF || *h != fh || *C != fC)
        return fail(err, "gcn_weights_read: the file holds widths input_dim=" + std::to_string(fF) + " hidden_dim=" + std::to_string(fh) +
                             " output_dim=" + std::to_string(fC) + ", the model has " + std::to_string(*F) + ", " + std::to_string(*h) + ", " +
                             std::to_string(*C) + where);
    get_f32s(&b[HEADER_BYTES], w1, n1);
    get_f32s(&b[HEADER_BYTES + 4 * n1], w2, n2);
    return 0;
}
