// plan_check.cpp — runs the host planning of csrc/plan.h on arrays from a file and writes the plans back, so that
// tests/test_plan_cpu.py can compare them with numpy.  A program of its own (no HIP runtime, no Python): the test builds
// it with g++ and -fsanitize=address,undefined.
//     plan_check graph <in> <out>      plan_check feat <in> <out>
// A file is a sequence of arrays, each an int32 count followed by that many 32-bit words.
#include "../cuda_gcn_amd/csrc/plan.h"
#include <stdio.h>
#include <string.h>

typedef std::vector<int> Arr;

static std::vector<Arr> read_arrays(const char *path) {
    std::vector<Arr> out;
    FILE *fp = fopen(path, "rb");
    int n;
    while (fp && fread(&n, 4, 1, fp) == 1) {
        Arr a((size_t)n);
        if (n && fread(a.data(), 4, (size_t)n, fp) != (size_t)n) { out.clear(); break; }
        out.push_back(std::move(a));
    }
    if (fp) fclose(fp);
    return out;
}
static FILE *g_out;
static void put(const int *p, size_t n) {
    const int cnt = (int)n;
    fwrite(&cnt, 4, 1, g_out);
    if (n) fwrite(p, 4, n, g_out);
}
static void put(const Arr &a) { put(a.data(), a.size()); }
static void put(const std::vector<int4> &a) { put((const int *)a.data(), a.size() * 4); }
static void put(const plan::Schedule &s) { put(s.tasks); put(s.split); put(Arr{s.n_slots}); }
static const int *ptr_or_null(const Arr &a) { return a.empty() ? nullptr : a.data(); }

// in: {n_rows, n_cols, forced split length, schedule mode, n_groups, threads}, indptr, indices, col_deg (or empty),
//     row_group (or empty), row bits of a subset, column bits of a restriction, coefficients (f32 words)
static int graph(const std::vector<Arr> &in) {
    if (in.size() != 8 || in[0].size() != 6) return 2;
    const int n_rows = in[0][0], n_cols = in[0][1], forced = in[0][2], mode = in[0][3], n_groups = in[0][4], n_thr = in[0][5];
    const Arr &indptr = in[1], &indices = in[2];
    const bool valid = plan::valid_csr(indptr.data(), ptr_or_null(indices), n_rows, n_cols);
    put(Arr{valid ? 1 : 0});
    if (!valid) return 0;
    const int nnz = indptr[n_rows];
    Arr one = indices, many = indices;                           // the neighbour sort, with one thread and with several
    plan::sort_neighbours(indptr.data(), n_rows, ptr_or_null(in[3]), one, 1);
    plan::sort_neighbours(indptr.data(), n_rows, ptr_or_null(in[3]), many, n_thr);
    put(one); put(many);
    const int seg = plan::split_length(nnz, forced);
    Arr lengths{seg, plan::split_length((int64_t)1 << 40, forced), plan::sort_threads(nnz), plan::sort_threads((int64_t)1 << 20)};
    for (int64_t n : {0, 128 * 8192 - 1, 256 * 8192 - 1, 256 * 8192, 512 * 8192, 1024 * 8192}) lengths.push_back(plan::split_length(n, 0));
    put(lengths);
    const Arr order = plan::schedule_order(indptr.data(), n_rows, mode, ptr_or_null(in[4]), n_groups);
    put(order);
    const plan::Schedule s = plan::cut_segments(indptr.data(), order.data(), n_rows, seg);
    put(s);
    int bounds[4][9];
    plan::xcd_bounds(s.tasks, bounds);
    put(&bounds[0][0], 36);
    std::vector<uint32_t> bits(in[5].begin(), in[5].end());
    const plan::Schedule sub = plan::filter_rows(s.tasks, s.split, bits);
    put(sub);
    plan::xcd_bounds(sub.tasks, bounds);
    put(&bounds[0][0], 36);
    put(plan::order_of(s.tasks, n_rows));
    Arr idx = one;                                               // the restriction of the sorted edges
    std::vector<float> cf(in[7].size());
    std::vector<uint32_t> col_bits(in[6].begin(), in[6].end());
    memcpy(cf.data(), in[7].data(), cf.size() * 4);
    const Arr ip = plan::restrict_edges(indptr.data(), n_rows, col_bits.data(), idx.data(), cf.data());
    Arr cf_words((size_t)ip[n_rows]);
    memcpy(cf_words.data(), cf.data(), cf_words.size() * 4);
    idx.resize(cf_words.size());
    put(ip); put(idx); put(cf_words);
    return 0;
}

// in: {n_rows, n_cols, forced waves per column task}, indptr, indices (empty: none given)
static int feat(const std::vector<Arr> &in) {
    if (in.size() != 3 || in[0].size() != 3) return 2;
    const int n_rows = in[0][0], n_cols = in[0][1], forced = in[0][2];
    const Arr &indptr = in[1], &indices = in[2];
    const int64_t nnz = indptr[n_rows];
    const bool dense = plan::dense_layout(indptr.data(), ptr_or_null(indices), n_rows, n_cols);
    const bool in_range = plan::indices_in_range(indices.data(), (int64_t)indices.size(), n_cols);
    put(Arr{dense ? 1 : 0, in_range ? 1 : 0});
    if (dense || !in_range || (int64_t)indices.size() != nnz) return 0;
    const plan::Csc csc = plan::csc_sort(indptr.data(), indices.data(), n_rows, n_cols);
    put(csc.ptr); put(csc.row); put(csc.pos);
    const int nw = plan::column_waves(nnz, n_cols, forced), seg = plan::column_segment(nw);
    put(Arr{nw, seg});
    put(plan::cut_segments(csc.ptr.data(), nullptr, n_cols, seg));
    return 0;
}

int main(int argc, char **argv) {
    if (argc != 4) return 2;
    const std::vector<Arr> in = read_arrays(argv[2]);
    g_out = fopen(argv[3], "wb");
    if (in.empty() || !g_out) return 2;
    const int rc = !strcmp(argv[1], "graph") ? graph(in) : (!strcmp(argv[1], "feat") ? feat(in) : 2);
    return fclose(g_out) == 0 ? rc : 2;
}
