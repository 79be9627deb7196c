// plan.h — the host planning of the prepared adjacency and feature objects (graph.hip, feat.hip): everything here fixes
// the summation order of an aggregation or a weight gradient, and none of it calls the HIP runtime, so a plain C++
// program can run it (tests/plan_check.cpp).  int4 is only the record type of a task.
#pragma once
#include <hip/hip_vector_types.h>
#include <stdint.h>
#include <algorithm>
#include <thread>
#include <utility>
#include <vector>

namespace plan {

// the stored arrays of a CSR matrix are usable: row pointers ascend from a non-negative count, every index is a column
inline bool indices_in_range(const int *indices, int64_t nnz, int n_cols) {
    for (int64_t e = 0; e < nnz; e++)
        if (indices[e] < 0 || indices[e] >= n_cols) return false;    // a bad column would fault the gather
    return true;
}
inline bool valid_csr(const int *indptr, const int *indices, int n_rows, int n_cols) {
    const int nnz = indptr[n_rows];
    if (nnz < 0 || (nnz > 0 && !indices)) return false;
    for (int r = 0; r < n_rows; r++)
        if (indptr[r + 1] < indptr[r]) return false;
    return indices_in_range(indices, nnz, n_cols);
}

// Rows longer than the split length are cut into segments (one wave each).  A segment is a serial walk, so it
// must stay short against the work one wave slot gets: nnz / (256 CUs x 32 waves), clamped to [128, 1024]
// (a full Reddit graph keeps 1024; a 1/8 row block of it gets 256, which removed a 50 us critical path
// from a 130 us launch).
inline int split_length(int64_t nnz, int forced) {
    if (forced >= 16) return forced;                 // the split_edges option of the creating context (experiments)
    int s = 1024;      // round 3 sweep: 512 is 1 % better on reddit-syn's hidden width (0.766 -> 0.756 ms, epoch +0.4 %) and 5 % worse on
                       // the R-MAT scale-22 model (24.5 vs 25.8 epochs/s: ten times the segments, all through the partial scratch); 256 and
                       // 2048+ lose on both.  1024 stays.
    while (s > 128 && (int64_t)s * 8192 > nnz) s >>= 1;
    return s;
}

// a task list {id, begin, end, partial slot or -1}, the ids that were cut {id, first slot, segments, 0}, and the slot count
struct Schedule {
    std::vector<int4> tasks, split;
    int n_slots = 0;
};

// One task per range ptr[id] .. ptr[id + 1] in the given order (order == nullptr: 0 .. n - 1); a range longer than `seg`
// becomes consecutive segments of at most `seg` whose partial sums (slots numbered in task order) a second launch adds in
// order.  The rows of an adjacency and the columns of a CSC view are both cut here.
inline Schedule cut_segments(const int *ptr, const int *order, int n, int seg) {
    Schedule s;
    s.tasks.reserve((size_t)n + 64);
    for (int i = 0; i < n; i++) {
        const int id = order ? order[i] : i, e0 = ptr[id], e1 = ptr[id + 1];
        if (e1 - e0 <= seg) { s.tasks.push_back(make_int4(id, e0, e1, -1)); continue; }
        const int ns = (e1 - e0 + seg - 1) / seg;
        s.split.push_back(make_int4(id, s.n_slots, ns, 0));
        for (int q = 0; q < ns; q++)
            s.tasks.push_back(make_int4(id, e0 + q * seg, std::min(e1, e0 + (q + 1) * seg), s.n_slots + q));
        s.n_slots += ns;
    }
    return s;
}

// the tasks of the full schedule whose row is in the subset (bit r of `bits`), same order, same segment slots
inline Schedule filter_rows(const std::vector<int4> &tasks, const std::vector<int4> &split, const std::vector<uint32_t> &bits) {
    auto in = [&](int r) { return (bits[r >> 5] >> (r & 31)) & 1u; };
    Schedule s;
    for (const int4 &t : tasks) if (in(t.x)) s.tasks.push_back(t);
    for (const int4 &sr : split) if (in(sr.x)) s.split.push_back(sr);
    return s;
}

// the row order a task list was built from (a split row appears once per segment, consecutively)
inline std::vector<int> order_of(const std::vector<int4> &tasks, int n_rows) {
    std::vector<int> order;
    order.reserve((size_t)n_rows);
    for (const int4 &t : tasks)
        if (order.empty() || order.back() != t.x) order.push_back(t.x);
    return order;
}

// equal-work task ranges for G XCD groups, each starting on a multiple of 4 tasks (one workgroup); prefix[t] = work before task t
inline void xcd_group_bounds(const std::vector<int64_t> &prefix, int G, int out[9]) {
    const int n_units = (int)prefix.size() - 1;
    out[0] = 0;
    for (int k = 1; k < G; k++) {
        const int64_t target = prefix[n_units] * k / G;
        int t = (int)(std::lower_bound(prefix.begin(), prefix.end(), target) - prefix.begin());
        t = (t + 3) / 4 * 4;
        if (t > n_units) t = n_units;
        if (t < out[k - 1]) t = out[k - 1];
        out[k] = t;
    }
    for (int k = G; k <= 8; k++) out[k] = n_units;
}
// ... for 1/2/4/8 groups
inline void xcd_bounds(const std::vector<int4> &tasks, int bounds[4][9]) {
    const int n_units = (int)tasks.size();
    std::vector<int64_t> prefix((size_t)n_units + 1);   // work before task t: edges + a per-task constant
    prefix[0] = 0;
    for (int t = 0; t < n_units; t++) prefix[t + 1] = prefix[t] + (tasks[t].z - tasks[t].y) + 8;
    for (int lg = 0; lg < 4; lg++) xcd_group_bounds(prefix, 1 << lg, bounds[lg]);
}

// Row order of the schedule: rows in descending degree order (heavy work first, similar rows together), group-major
// when the caller names communities — (key[row] ascending, degree descending), stable; key == nullptr: degree only.
inline std::vector<int> row_order(const int *indptr, int n_rows, const int *key) {
    std::vector<int> order(n_rows);
    for (int r = 0; r < n_rows; r++) order[r] = r;
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) {
        if (key && key[a] != key[b]) return key[a] < key[b];
        return indptr[a + 1] - indptr[a] > indptr[b + 1] - indptr[b];
    });
    return order;
}
// ... of a schedule mode (gcnhip_graph_set_schedule): 0 by degree, 1 by the caller's groups, 2 dealt —
// rows ranked by descending degree, rank r goes to group r % n_groups: every group has the
// same degree mix, so hub rows and the long tail of short rows are in flight together
inline std::vector<int> schedule_order(const int *indptr, int n_rows, int mode, const int *row_group, int n_groups) {
    if (mode != 2) return row_order(indptr, n_rows, mode == 1 ? row_group : nullptr);
    const std::vector<int> rank = row_order(indptr, n_rows, nullptr);
    std::vector<int> key(n_rows);
    for (int k = 0; k < n_rows; k++) key[rank[k]] = k % n_groups;
    return row_order(indptr, n_rows, key.data());
}

// Gather order inside a row: neighbours by descending degree.  Every wave then asks for the
// popular rows (which are the ones that stay in L2) at the same point of its walk; measured on
// reddit-syn this and the degree-ordered task list are worth 6 % (d = 128) and 13 % (d = 41).
// Only the order of the floating-point sum changes.  std::sort of (-degree, id) pairs: ties go by ascending id.
// (host threads over row ranges of equal edge count: at Reddit scale this sort was 0.4 s of a 0.67 s object build, at
//  R-MAT scale 22 most of 4.8 s; rows are independent, so the result does not depend on the thread count)
inline int sort_threads(int64_t nnz) {
    return nnz < (1 << 20) ? 1 : (int)std::min<unsigned>(16u, std::max(1u, std::thread::hardware_concurrency()));
}
inline void sort_neighbours(const int *indptr, int n_rows, const int *col_deg, std::vector<int> &idx, int n_thr) {
    const int nnz = indptr[n_rows];
    auto deg_of = [&](int j) { return col_deg ? col_deg[j] : indptr[j + 1] - indptr[j]; };
    auto sort_rows = [&](int r_lo, int r_hi) {
        std::vector<std::pair<int, int>> tmp;
        for (int r = r_lo; r < r_hi; r++) {
            const int e0 = indptr[r], e1 = indptr[r + 1];
            if (e1 - e0 < 2) continue;
            tmp.resize(e1 - e0);
            for (int e = e0; e < e1; e++) tmp[e - e0] = {-deg_of(idx[e]), idx[e]};
            std::sort(tmp.begin(), tmp.end());
            for (int e = e0; e < e1; e++) idx[e] = tmp[e - e0].second;
        }
    };
    if (n_thr <= 1) return sort_rows(0, n_rows);
    std::vector<std::thread> pool;
    int r_lo = 0;
    for (int t = 0; t < n_thr; t++) {
        const int64_t target = (int64_t)nnz * (t + 1) / n_thr;
        int r_hi = t == n_thr - 1 ? n_rows : (int)(std::upper_bound(indptr, indptr + n_rows + 1, (int)target) - indptr);
        r_hi = std::max(r_lo, std::min(n_rows, r_hi));
        pool.emplace_back(sort_rows, r_lo, r_hi);
        r_lo = r_hi;
    }
    for (auto &th : pool) th.join();
}

// Keep the edges whose column has its bit set, in their stored order and with their coefficients: idx and cf are
// compacted in place, the new row pointers are returned (their last entry is the number of edges left).
inline std::vector<int> restrict_edges(const int *indptr, int n_rows, const uint32_t *col_bits, int *idx, float *cf) {
    std::vector<int> ip((size_t)n_rows + 1);
    size_t w = 0;
    for (int r = 0; r < n_rows; r++) {
        ip[r] = (int)w;
        for (int e = indptr[r]; e < indptr[r + 1]; e++) {
            const int j = idx[e];
            if ((col_bits[j >> 5] >> (j & 31)) & 1u) { idx[w] = j; cf[w] = cf[e]; w++; }   // w <= e: in place
        }
    }
    ip[n_rows] = (int)w;
    return ip;
}

// dense <=> every row is exactly 0..n_cols-1 in order (indices == NULL asserts it)
inline bool dense_layout(const int *indptr, const int *indices, int n_rows, int n_cols) {
    if ((int64_t)indptr[n_rows] != (int64_t)n_rows * n_cols || n_rows <= 0) return false;
    if (!indices) return true;
    for (int r = 0; r < n_rows; r++) {
        if (indptr[r + 1] - indptr[r] != n_cols) return false;
        const int *row = indices + (size_t)r * n_cols;
        for (int k = 0; k < n_cols; k++)
            if (row[k] != k) return false;
    }
    return true;
}

// CSC by counting sort; entries of a column stay in row order, so the
// gather-form weight gradient adds them in the reference's order
// (src/seq/module.cpp:68-74 visits rows ascending).
struct Csc {
    std::vector<int> ptr, row, pos;     // [n_cols + 1]; source row of each entry; its position in CSR order
};
inline Csc csc_sort(const int *indptr, const int *indices, int n_rows, int n_cols) {
    const int64_t nnz = indptr[n_rows];
    Csc c{std::vector<int>((size_t)n_cols + 1, 0), std::vector<int>((size_t)nnz), std::vector<int>((size_t)nnz)};
    for (int64_t e = 0; e < nnz; e++) c.ptr[indices[e] + 1]++;
    for (int k = 0; k < n_cols; k++) c.ptr[k + 1] += c.ptr[k];
    std::vector<int> fill(c.ptr.begin(), c.ptr.end() - 1);
    for (int r = 0; r < n_rows; r++)
        for (int e = indptr[r]; e < indptr[r + 1]; e++) {
            const int q = fill[indices[e]]++;
            c.row[q] = r;
            c.pos[q] = e;
        }
    return c;
}

// Task list of the weight gradient (spmm_sparse.h).  Waves per task by the mean column length: a short column is
// one wave's walk, a long one is shared by 4 or 16 waves of one workgroup (Pubmed: ~2 000 entries per column);
// anything beyond the segment length is cut into several tasks with partial rows (skewed bag-of-words columns).
inline int column_waves(int64_t nnz, int n_cols, int forced) {
    if (forced == 1 || forced == 4 || forced == 16) return forced;      // the spmm_nw option (experiments)
    const double mean = n_cols ? (double)nnz / n_cols : 0.0;
    return mean <= 128.0 ? 1 : (mean <= 1024.0 ? 4 : 16);
}
inline int column_segment(int waves) { return std::max(1024, waves * 256); }

}  // namespace plan
