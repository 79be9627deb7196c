// labels.cpp — the multi-label truth file (labels.h)
#include "labels.h"
#include <algorithm>
#include <cerrno>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>

static int fail(std::string *err, const std::string &msg) {
    if (err) *err = msg;
    return -1;
}

int gcn_labels_read(const char *path, int *num_nodes, int *num_classes, std::vector<uint32_t> &bits, std::string *err) {
    if (!path || !num_nodes || !num_classes) return fail(err, "labels: invalid argument");
    std::ifstream f(path, std::ios::binary);
    if (!f) return fail(err, std::string("labels: cannot open ") + path);
    std::stringstream ss;
    ss << f.rdbuf();
    const std::string text = ss.str();
    // lines: pieces between '\n'; a final newline ends the last line rather than starting an empty one
    std::vector<std::vector<int>> rows;
    const std::string where = std::string("labels: ") + path + ":";
    int max_id = -1;
    size_t pos = 0;
    while (pos < text.size()) {
        size_t end = text.find('\n', pos);
        if (end == std::string::npos) end = text.size();
        std::string line = text.substr(pos, end - pos);
        pos = end + 1;
        if (!line.empty() && line.back() == '\r') line.pop_back();
        const int lineno = (int)rows.size() + 1;
        rows.emplace_back();
        std::vector<int> &ids = rows.back();
        bool blank = line.find_first_not_of(" \t") == std::string::npos;
        if (blank) continue;
        size_t p = 0;
        while (true) {
            size_t q = line.find(',', p);
            if (q == std::string::npos) q = line.size();
            std::string tok = line.substr(p, q - p);
            const size_t a = tok.find_first_not_of(" \t"), b = tok.find_last_not_of(" \t");
            tok = a == std::string::npos ? std::string() : tok.substr(a, b - a + 1);
            if (!tok.empty() && tok[0] == '-' && tok.size() > 1 && tok.find_first_not_of("0123456789", 1) == std::string::npos)
                return fail(err, where + std::to_string(lineno) + ": negative class id '" + tok + "'");
            if (tok.empty() || tok.find_first_not_of("0123456789") != std::string::npos)
                return fail(err, where + std::to_string(lineno) + ": bad token '" + tok + "' (expected class ids separated by commas)");
            errno = 0;
            const long v = strtol(tok.c_str(), nullptr, 10);
            if (errno || v > GCN_LABELS_MAX_CLASS)
                return fail(err, where + std::to_string(lineno) + ": class id '" + tok + "' is too large");
            if (*num_classes > 0 && v >= *num_classes)
                return fail(err, where + std::to_string(lineno) + ": class id " + tok + " is not below the number of classes " + std::to_string(*num_classes));
            ids.push_back((int)v);
            if ((int)v > max_id) max_id = (int)v;
            if (q == line.size()) break;
            p = q + 1;
        }
    }
    const int n = (int)rows.size();
    if (*num_nodes > 0 && n != *num_nodes)
        return fail(err, where + " " + std::to_string(n) + " lines, but the dataset has " + std::to_string(*num_nodes) + " nodes (one line per node)");
    if (n == 0) return fail(err, where + " no lines");
    const int C = *num_classes > 0 ? *num_classes : std::max(max_id + 1, 1);
    const int wpr = gcn_label_words(C);
    bits.assign((size_t)n * wpr, 0u);
    for (int i = 0; i < n; i++)
        for (int c : rows[i]) bits[(size_t)i * wpr + (c >> 5)] |= 1u << (c & 31);
    *num_nodes = n;
    *num_classes = C;
    return 0;
}

int gcn_labels_write(const char *path, int num_nodes, int num_classes, const uint32_t *bits, std::string *err) {
    if (!path || num_nodes < 1 || num_classes < 1 || !bits) return fail(err, "labels: invalid argument");
    FILE *f = fopen(path, "w");
    if (!f) return fail(err, std::string("labels: cannot write ") + path);
    const int wpr = gcn_label_words(num_classes);
    bool ok = true;
    for (int i = 0; ok && i < num_nodes; i++) {
        bool first = true;
        for (int c = 0; ok && c < num_classes; c++)
            if ((bits[(size_t)i * wpr + (c >> 5)] >> (c & 31)) & 1u) {
                ok = fprintf(f, first ? "%d" : ",%d", c) > 0;
                first = false;
            }
        ok = ok && fputc('\n', f) != EOF;
    }
    if (fclose(f) != 0) ok = false;
    return ok ? 0 : fail(err, std::string("labels: could not write ") + path);
}
