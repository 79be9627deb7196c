// hdbscan.h — what HDBSCAN derives from the sorted minimum spanning tree of the mutual-reachability graph, on the host and without
// a GPU (Campello, Moulavi & Sander, 2013; scikit-learn's HDBSCAN, whose labels, numbering and probabilities these are):
// the single-linkage dendrogram, the condensed tree for min_cluster_size, the clusters selected by stability (excess of mass) or
// the leaves, the labels and membership probabilities, and the DBSCAN* labels at any cut.  The tree comes from csrc/hdbscan.hip
// (include/gcnhip_driver.h has its definitions); ModelQueries::hdbscan and the C entry points call these.
//
// The tree: `edges` rows (lo[e], hi[e], d2[e]) on list positions 0 .. n - 1, sorted by ascending d2 (squared distances in float64; the
// square roots are taken here), acyclic and connected over the positions it touches.  Those positions are the POINTS,
// numbered 0 .. p - 1 in ascending position; every other position is no point: label -1, probability 0.
// Dendrogram: union-find over the edges in order.  Row e joins the two current clusters of its ends into cluster p + e; `left` is
//   the cluster of the end NEARER TO POINT 0 IN THE TREE — how scikit-learn's Prim walk from point 0 orients its edges, which
//   decides the numbering below.  linkage [edges x 4] = {min(left, right), max(left, right), sqrt(d2), size}: scipy's format.
// Condensed tree: scikit-learn's _condense_tree, breadth first from the root, left before right, lambda = 1 / distance (+inf at 0):
//   a split whose sides both hold min_cluster_size points makes two new clusters, numbered in that order from p + 1 (the root is p);
//   otherwise the smaller side's points fall out of the parent at that lambda.
// Selection: stability(c) = sum over c's rows of (lambda - birth(c)) . size.  "eom": from the highest number down, a cluster whose
//   children's stabilities sum to more than its own passes the sum up, else it is kept and its descendants dropped; the root only
//   with allow_single_cluster.  "leaf": the clusters without cluster children.  Labels number the kept clusters 0 .. k - 1 in
//   ascending cluster number; a point belongs to the first kept cluster above it.  With the root alone kept, a point belongs to it
//   when its lambda reaches the largest lambda of the root's own rows.
// probability = min(lambda(point), death(c)) / death(c), 1 where death(c) is 0 or lambda is +inf; death(c) is scikit-learn's
//   max_lambdas: the largest lambda in the LAST contiguous run of c's rows.
// cut(distance): the clusters of the edges with sqrt(d2) < distance; those below min_cluster_size are noise; numbered as
//   scikit-learn's dbscan_clustering numbers them (ascending representative of its union-find).
#pragma once
#include <cstdint>
#include <string>

// labels int32 [n], probabilities float64 [n]; linkage float64 [edges x 4] or NULL; info [3] = {points, clusters, noise points}.
// min_cluster_size >= 2.  -1 with *err set when the rows are no sorted tree.
int gcn_hdbscan_tree(const int32_t *lo, const int32_t *hi, const double *d2, int64_t edges, int64_t n, int min_cluster_size, bool leaf,
                     bool allow_single_cluster, int32_t *labels, double *probabilities, double *linkage, int64_t *info, std::string *err);
// labels int32 [n]; info [3] as above
int gcn_hdbscan_cut(const int32_t *lo, const int32_t *hi, const double *d2, int64_t edges, int64_t n, double distance, int min_cluster_size,
                    int32_t *labels, int64_t *info, std::string *err);
