// hdbscan.cpp — the host half of HDBSCAN: from the sorted minimum spanning tree to labels (hdbscan.h has the definitions).  No GPU.
#include "hdbscan.h"
#include <algorithm>
#include <cmath>
#include <limits>
#include <map>
#include <vector>

namespace {

struct HdRow { int64_t left, right; double dist; int64_t size; };      // a dendrogram row: cluster p + e
struct HdCond { int64_t parent, child; double lambda; int64_t size; }; // a condensed-tree row

int64_t hd_find(std::vector<int64_t> &up, int64_t x) {
    while (up[x] != x) {
        up[x] = up[up[x]];
        x = up[x];
    }
    return x;
}

// the points (ascending positions) and the dendrogram rows; an empty string when the rows are a sorted tree
std::string hd_linkage(const int32_t *lo, const int32_t *hi, const double *d2, int64_t edges, int64_t n, std::vector<int64_t> &pts, std::vector<HdRow> &rows) {
    if (n < 0 || edges < 0 || (edges > 0 && (!lo || !hi || !d2))) return "invalid argument";
    if (edges >= std::max<int64_t>(n, 1)) return "a tree over " + std::to_string(n) + " positions has fewer than " + std::to_string(edges) + " edges";
    std::vector<int64_t> id((size_t)n, -1);
    for (int64_t e = 0; e < edges; e++) {
        if (lo[e] < 0 || lo[e] >= n || hi[e] < 0 || hi[e] >= n || lo[e] == hi[e]) return "edge " + std::to_string(e) + " has an end outside the list";
        if (!(d2[e] >= 0.0) || (e > 0 && d2[e] < d2[e - 1])) return "the weights must be non-negative and ascending (edge " + std::to_string(e) + ")";
        id[lo[e]] = id[hi[e]] = 0;
    }
    pts.clear();
    for (int64_t i = 0; i < n; i++)
        if (id[i] == 0) {
            id[i] = (int64_t)pts.size();
            pts.push_back(i);
        }
    const int64_t p = (int64_t)pts.size();
    rows.clear();
    if (edges == 0) return "";
    if (p != edges + 1) return "the edges do not form one tree";
    std::vector<int64_t> start((size_t)p + 1, 0), nbr((size_t)(2 * edges)), depth((size_t)p, -1), queue;
    for (int64_t e = 0; e < edges; e++) { start[id[lo[e]] + 1]++; start[id[hi[e]] + 1]++; }
    for (int64_t i = 0; i < p; i++) start[i + 1] += start[i];
    std::vector<int64_t> fill(start.begin(), start.end() - 1);
    for (int64_t e = 0; e < edges; e++) { nbr[fill[id[lo[e]]]++] = id[hi[e]]; nbr[fill[id[hi[e]]]++] = id[lo[e]]; }
    depth[0] = 0;
    queue.push_back(0);
    for (size_t q = 0; q < queue.size(); q++)
        for (int64_t s = start[queue[q]]; s < start[queue[q] + 1]; s++)
            if (depth[nbr[s]] < 0) {
                depth[nbr[s]] = depth[queue[q]] + 1;
                queue.push_back(nbr[s]);
            }
    if ((int64_t)queue.size() != p) return "the edges do not form one tree";
    std::vector<int64_t> up((size_t)p), clus((size_t)p), size((size_t)(2 * p - 1), 1);
    for (int64_t i = 0; i < p; i++) up[i] = clus[i] = i;
    for (int64_t e = 0; e < edges; e++) {
        int64_t a = id[lo[e]], b = id[hi[e]];
        if (depth[a] > depth[b]) std::swap(a, b);                  // a: the end nearer to point 0
        const int64_t ra = hd_find(up, a), rb = hd_find(up, b);
        const int64_t l = clus[ra], r = clus[rb];
        size[p + e] = size[l] + size[r];
        rows.push_back(HdRow{l, r, std::sqrt(d2[e]), size[p + e]});
        up[rb] = ra;
        clus[ra] = p + e;
    }
    return "";
}

// the nodes below `node` breadth first, left before right, `node` first
void hd_bfs(const std::vector<HdRow> &rows, int64_t p, int64_t node, std::vector<int64_t> &out) {
    out.assign(1, node);
    for (size_t q = 0; q < out.size(); q++)
        if (out[q] >= p) {
            out.push_back(rows[out[q] - p].left);
            out.push_back(rows[out[q] - p].right);
        }
}

int hd_fail(std::string *err, const char *what, const std::string &why) {
    if (err) *err = std::string(what) + ": " + why;
    return -1;
}

}  // namespace

int gcn_hdbscan_tree(const int32_t *lo, const int32_t *hi, const double *d2, int64_t edges, int64_t n, int min_cluster_size, bool leaf,
                     bool allow_single_cluster, int32_t *labels, double *probabilities, double *linkage, int64_t *info, std::string *err) {
    if (!labels || !probabilities) return hd_fail(err, "hdbscan_tree", "invalid argument");
    if (min_cluster_size < 2) return hd_fail(err, "hdbscan_tree", "min_cluster_size must be at least 2, got " + std::to_string(min_cluster_size));
    std::vector<int64_t> pts;
    std::vector<HdRow> rows;
    const std::string why = hd_linkage(lo, hi, d2, edges, n, pts, rows);
    if (!why.empty()) return hd_fail(err, "hdbscan_tree", why);
    const int64_t p = (int64_t)pts.size(), mcs = min_cluster_size;
    for (int64_t i = 0; i < n; i++) { labels[i] = -1; probabilities[i] = 0.0; }
    if (info) { info[0] = p; info[1] = 0; info[2] = p; }
    if (p < 2) return 0;
    if (linkage)
        for (int64_t e = 0; e < edges; e++) {
            linkage[4 * e] = (double)std::min(rows[e].left, rows[e].right);
            linkage[4 * e + 1] = (double)std::max(rows[e].left, rows[e].right);
            linkage[4 * e + 2] = rows[e].dist;
            linkage[4 * e + 3] = (double)rows[e].size;
        }

    // the condensed tree, in scikit-learn's row order
    const int64_t root = 2 * (p - 1);
    std::vector<int64_t> order, sub, relabel((size_t)root + 1, -1);
    std::vector<char> ignore((size_t)root + 1, 0);
    std::vector<HdCond> cond;
    int64_t next = p + 1;
    relabel[root] = p;
    hd_bfs(rows, p, root, order);
    for (const int64_t node : order) {
        if (node < p || ignore[node]) continue;
        const HdRow &row = rows[node - p];
        const double lambda = row.dist > 0.0 ? 1.0 / row.dist : std::numeric_limits<double>::infinity();
        const int64_t side[2] = {row.left, row.right};
        const int64_t count[2] = {row.left >= p ? rows[row.left - p].size : 1, row.right >= p ? rows[row.right - p].size : 1};
        for (int s = 0; s < 2; s++) {
            if (count[s] >= mcs && count[1 - s] >= mcs) {
                relabel[side[s]] = next++;
                cond.push_back(HdCond{relabel[node], relabel[side[s]], lambda, count[s]});
            } else if (count[s] >= mcs) {
                relabel[side[s]] = relabel[node];
            } else {
                hd_bfs(rows, p, side[s], sub);
                for (const int64_t x : sub) {
                    if (x < p) cond.push_back(HdCond{relabel[node], x, lambda, 1});
                    ignore[x] = 1;
                }
            }
        }
    }

    // stabilities and the selection; cluster c is number p + c
    const int64_t n_cl = next - p;
    const double nan = std::numeric_limits<double>::quiet_NaN();
    std::vector<double> birth((size_t)n_cl, nan), stab((size_t)n_cl, 0.0), death((size_t)n_cl, 0.0);
    std::vector<int64_t> par((size_t)n_cl, -1), top((size_t)n_cl, 0), number((size_t)n_cl, -1);
    std::vector<std::vector<int64_t>> kids((size_t)n_cl);
    birth[0] = 0.0;
    for (const HdCond &c : cond)
        if (c.child >= p) {
            birth[c.child - p] = c.lambda;
            par[c.child - p] = c.parent - p;
            kids[c.parent - p].push_back(c.child - p);
        }
    for (const HdCond &c : cond) stab[c.parent - p] += (c.lambda - birth[c.parent - p]) * (double)c.size;
    std::vector<char> keep((size_t)n_cl, 1);
    keep[0] = allow_single_cluster && !leaf;
    if (leaf) {
        for (int64_t c = 1; c < n_cl; c++) keep[c] = kids[c].empty();
    } else {
        for (int64_t c = n_cl - 1; c >= (allow_single_cluster ? 0 : 1); c--) {
            double below = 0.0;
            for (const int64_t k : kids[c]) below += stab[k];
            if (below > stab[c]) {
                keep[c] = 0;
                stab[c] = below;
            } else {
                sub.assign(kids[c].begin(), kids[c].end());
                for (size_t q = 0; q < sub.size(); q++) {
                    keep[sub[q]] = 0;
                    sub.insert(sub.end(), kids[sub[q]].begin(), kids[sub[q]].end());
                }
            }
        }
    }
    int64_t k = 0;
    for (int64_t c = 0; c < n_cl; c++) {
        if (keep[c]) number[c] = k++;
        top[c] = c == 0 || keep[c] ? c : top[par[c]];              // a parent's number is below its children's
    }
    int64_t cur = cond[0].parent - p;                              // max_lambdas: the last run of a parent's rows wins
    double best = cond[0].lambda, root_max = 0.0;
    for (size_t r = 1; r < cond.size(); r++) {
        if (cond[r].parent - p == cur) {
            best = std::max(best, cond[r].lambda);
        } else {
            death[cur] = best;
            cur = cond[r].parent - p;
            best = cond[r].lambda;
        }
    }
    death[cur] = best;
    for (const HdCond &c : cond)
        if (c.parent == p) root_max = std::max(root_max, c.lambda);
    int64_t noise = p;
    for (const HdCond &c : cond) {
        if (c.child >= p) continue;
        const int64_t t = top[c.parent - p];
        if (!keep[t] || (t == 0 && !(c.lambda >= root_max))) continue;
        labels[pts[c.child]] = (int32_t)number[t];
        probabilities[pts[c.child]] = death[t] == 0.0 || std::isinf(c.lambda) ? 1.0 : std::min(c.lambda, death[t]) / death[t];
        noise--;
    }
    if (info) { info[1] = k; info[2] = noise; }
    return 0;
}

int gcn_hdbscan_cut(const int32_t *lo, const int32_t *hi, const double *d2, int64_t edges, int64_t n, double distance, int min_cluster_size,
                    int32_t *labels, int64_t *info, std::string *err) {
    if (!labels || std::isnan(distance)) return hd_fail(err, "hdbscan_cut", "invalid argument");
    if (min_cluster_size < 1) return hd_fail(err, "hdbscan_cut", "min_cluster_size must be at least 1, got " + std::to_string(min_cluster_size));
    std::vector<int64_t> pts;
    std::vector<HdRow> rows;
    const std::string why = hd_linkage(lo, hi, d2, edges, n, pts, rows);
    if (!why.empty()) return hd_fail(err, "hdbscan_cut", why);
    const int64_t p = (int64_t)pts.size(), total = std::max<int64_t>(2 * p - 1, 0);
    for (int64_t i = 0; i < n; i++) labels[i] = -1;
    std::vector<int64_t> up((size_t)total), rank((size_t)total, 0);
    for (int64_t i = 0; i < total; i++) up[i] = i;
    const auto join = [&](int64_t x, int64_t y) {                  // scikit-learn's TreeUnionFind: by rank, x's root on a tie
        const int64_t a = hd_find(up, x), b = hd_find(up, y);
        if (rank[a] < rank[b]) {
            up[a] = b;
        } else {
            up[b] = a;
            rank[a] += rank[a] == rank[b];
        }
    };
    for (int64_t e = 0; e < edges; e++)
        if (rows[e].dist < distance) {
            join(rows[e].left, p + e);
            join(rows[e].right, p + e);
        }
    std::map<int64_t, int64_t> size;                               // by ascending representative
    for (int64_t i = 0; i < p; i++) size[hd_find(up, i)]++;
    int64_t k = 0, noise = p;
    for (auto &s : size) {
        noise -= s.second >= min_cluster_size ? s.second : 0;
        s.second = s.second >= min_cluster_size ? k++ : -1;
    }
    for (int64_t i = 0; i < p; i++) labels[pts[i]] = (int32_t)size[hd_find(up, i)];
    if (info) { info[0] = p; info[1] = k; info[2] = noise; }
    return 0;
}
