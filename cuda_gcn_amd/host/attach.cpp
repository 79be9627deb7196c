// attach.cpp — gcn_attach_rows (attach.h): validation, the stored rows and the coefficients of new nodes.
#include "attach.h"
#include <climits>
#include <cmath>

static int attach_fail(std::string *err, const std::string &why) {
    if (err) *err = "new_node_rows: " + why;
    return -1;
}

int gcn_attach_rows(int N, const int *row_len, const int *row_of_id, int m, const int64_t *nbr_ptr, const int *nbr_ids, int mode, AttachRows *out,
                    std::string *err) {
    if (m < 0) return attach_fail(err, "m = " + std::to_string(m) + " is negative");
    if (N < 0 || !out || !nbr_ptr || (N > 0 && !row_len)) return attach_fail(err, "invalid argument");
    if (mode != ATTACH_COEF_EDGE && mode != ATTACH_COEF_FACTORED) return attach_fail(err, "the coefficient form is 0 (per edge) or 1 (factored)");
    if (nbr_ptr[0] != 0) return attach_fail(err, "nbr_ptr[0] = " + std::to_string(nbr_ptr[0]) + ", not 0");
    for (int i = 0; i < m; i++)
        if (nbr_ptr[i + 1] < nbr_ptr[i]) return attach_fail(err, "nbr_ptr decreases at new node " + std::to_string(i));
    const int64_t listed = nbr_ptr[m], total = listed + m;
    if (total > INT32_MAX) return attach_fail(err, std::to_string(total) + " stored entries: more than 2^31 - 1");
    if (listed > 0 && !nbr_ids) return attach_fail(err, "invalid argument");
    const int64_t limit = (int64_t)N + m;
    for (int64_t e = 0; e < listed; e++)
        if (nbr_ids[e] < 0 || nbr_ids[e] >= limit)
            return attach_fail(err, "id " + std::to_string(nbr_ids[e]) + " is outside [0, " + std::to_string(limit) + ") (the dataset's nodes, then this call's new ones)");
    out->ptr.assign((size_t)m + 1, 0);
    out->len.assign((size_t)m, 0);
    out->col.resize((size_t)total);
    out->coef.resize((size_t)total);
    for (int i = 0; i < m; i++) {
        out->len[i] = (int32_t)(1 + nbr_ptr[i + 1] - nbr_ptr[i]);
        out->ptr[i + 1] = out->ptr[i] + out->len[i];
    }
    auto len_of = [&](int64_t id) -> int64_t { return id < N ? row_len[row_of_id ? row_of_id[id] : id] : out->len[id - N]; };
    for (int i = 0; i < m; i++) {
        const int64_t lv = out->len[i];
        const float dinv = (float)(1.0 / std::sqrt((double)lv));
        int64_t e = out->ptr[i];
        for (int64_t k = -1; k < nbr_ptr[i + 1] - nbr_ptr[i]; k++, e++) {
            const int64_t id = k < 0 ? (int64_t)N + i : nbr_ids[nbr_ptr[i] + k];
            out->col[e] = (int32_t)(id < N && row_of_id ? row_of_id[id] : id);
            // the per-edge form as gcnhip_graph_create forms it: float sqrtf of the 64-bit product, divide in double, narrow
            out->coef[e] = mode == ATTACH_COEF_FACTORED ? dinv : (float)(1.0 / (double)sqrtf((float)(lv * len_of(id))));
        }
    }
    return 0;
}
