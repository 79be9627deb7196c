// labels.h — the multi-label truth file (beyond the reference, whose svmlight parser reads one class per node).  Host only.
//
// Format: one line per node, in node order.  A line holds the node's class ids separated by commas ("3,17,40"), or is
// empty for a node with no class; spaces around an id are allowed.  A final newline is optional.  The number of classes C
// is the largest id + 1 unless the caller fixes it.  A wrong number of lines, a token that is not a class id, a negative
// id or an id >= a fixed C is refused with a message naming the line; nothing is mended.
// The matrix is returned as multi-hot bit rows: bit (c & 31) of word [node * ceil(C / 32) + (c >> 5)] = class c of node.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

constexpr int GCN_LABELS_MAX_CLASS = 1 << 20;            // an id above this is refused (a typo, not a class)

inline int gcn_label_words(int num_classes) { return (num_classes + 31) / 32; }

// *num_nodes > 0: the file must have that many lines (else the count is taken from the file); *num_classes > 0: every id
// must be below it (else C = largest id + 1, at least 1).  Both receive the values used.  0, or -1 with the reason in *err.
int gcn_labels_read(const char *path, int *num_nodes, int *num_classes, std::vector<uint32_t> &bits, std::string *err);
// the inverse (tests, tools): one line per node of the class ids in ascending order
int gcn_labels_write(const char *path, int num_nodes, int num_classes, const uint32_t *bits, std::string *err);
