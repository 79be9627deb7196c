// attach.h — the stored rows of NEW nodes attached to a dataset's graph, and their coefficients: host only, no GPU.
// (ModelQueries::predict_new and gcnhip_attach_gather consume them; DESIGN §4.17 has the definition.)
//
// The dataset has N nodes; a call brings m new ones, new node i has id N + i.  Its stored row is
//     [N + i, nbr_ids[nbr_ptr[i] : nbr_ptr[i + 1]] ...]
// — the self loop first, then the listed ids in listed order — under the loader's rule (tests/irregular_inputs.py): degree =
// stored row length, a repeated entry counts twice, one-way entries are legal.  A listed id below N is a dataset node, N + k
// is new node k of the same call (also k == i again, also a later one); no existing row changes and existing nodes do not list
// the new ones back.  len(v) = the stored row length: 1 + the listed ids for a new node, the existing row for a dataset node.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

enum AttachCoef {
    ATTACH_COEF_EDGE = 0,      // coef[e] = a(v, j) = (float)(1 / sqrtf((float)(len(v) . len(j)))), the product in 64 bits: what
                               // gcnhip_graph_create stores per edge (HIPGCN_EDGE_COEF models: raw tables)
    ATTACH_COEF_FACTORED = 1,  // coef[e] = dinv(v) = (float)(1 / sqrt(len(v))) on every entry of row v: the factored model, whose
                               // gathered tables already carry dinv of their own row (gcnhip_graph_scales' dinv)
};

struct AttachRows {
    std::vector<int32_t> ptr;      // [m + 1]
    std::vector<int32_t> col;      // [ptr[m]]: table rows — a dataset id mapped through row_of_id, N + k kept
    std::vector<float> coef;       // [ptr[m]]
    std::vector<int32_t> len;      // [m] stored row lengths
};

// row_len [N]: the stored row length of every dataset node, indexed by TABLE ROW; row_of_id (may be NULL: identity) [N] maps a
// dataset id to its table row (a model that renumbered its nodes).  Refused with a message (returns -1, *err set): m < 0, a
// missing array, nbr_ptr[0] != 0 or a decreasing nbr_ptr, an id outside [0, N + m), more than 2^31 - 1 stored entries.
int gcn_attach_rows(int num_nodes, const int *row_len, const int *row_of_id, int m, const int64_t *nbr_ptr, const int *nbr_ids, int mode,
                    AttachRows *out, std::string *err);
