// reach.h — how far the listed nodes are from the labels a model learns from, from integer counts (beyond the reference).  Host
// only: no GPU.  The ONE place where what gcnhip_distance_strata counted (csrc/reach.hip has the definitions) becomes a report:
// ModelQueries::reach's callers (the Python binding, gcn-hip's GCN_REACH) hand it the tables.
//
// strata [(hops + 2) x 4]: per distance bucket {rows listed, rows with a known truth, of those predicted right, of those whose
// nearest source carries their label}; bucket b < hops holds distance b, bucket hops every distance >= hops, bucket hops + 1 the
// rows no source reaches.  1 <= hops <= 32.  `layers` is the depth of the model: a row is INSIDE the receptive field when
// 0 <= dist <= layers — the buckets 0 .. layers, which are exact distances only for layers < hops, so 0 <= layers < hops is
// required — and OUTSIDE it otherwise (further away or unreachable).
//   accuracy = correct / labelled, nearest_accuracy = nearest_correct / labelled, per bucket, inside, outside and over all rows;
//   unreachable = the rows of bucket hops + 1, unreachable_share = unreachable / rows listed.
// Everything is float64 arithmetic on the integers; a zero denominator gives 0, never NaN; a negative count, or a count above
// the one it is part of, is an error.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

constexpr int REACH_MAX_HOPS = 32, REACH_DEFAULT_LAYERS = 2;

struct ReachRow {
    int64_t rows = 0, labelled = 0, correct = 0, nearest_correct = 0;
    double accuracy = 0, nearest_accuracy = 0;
};
struct ReachMetrics {
    int hops = 0, layers = 0;
    std::vector<ReachRow> by_distance;                         // [hops + 2]
    ReachRow inside, outside, all;
    int64_t unreachable = 0;
    double unreachable_share = 0;
};
// the integers of one report, as gcn-hip writes them and reads them back
struct ReachCounts {
    int hops = 0, layers = 0;
    int64_t sources = 0, unlabelled = 0, rounds = 0;           // rows that became sources; listed rows without a label; components' rounds
    int64_t totals[6] = {};                                    // gcnhip_component_counts' totals
    std::vector<int64_t> level_counts;                         // [levels + 1]
    std::vector<int64_t> strata;                               // [(hops + 2) x 4]
};

// the depth used for a report of `hops` buckets: the model's two layers, or hops - 1 when the table is shorter than that
inline int gcn_reach_layers(int hops) { return hops > REACH_DEFAULT_LAYERS ? REACH_DEFAULT_LAYERS : hops - 1; }
// each: 0, or -1 with the reason in *err
int gcn_reach_metrics(const int64_t *strata, int hops, int layers, ReachMetrics *out, std::string *err);
// The text report: a header line, the integers by name (info, totals, level_counts, the strata rows) and, derived from them, the
// per-distance table and the inside / outside lines; the derived lines start with '#', and the reader, which takes the integers
// alone, passes over them.
int gcn_reach_write(const char *path, const ReachCounts &c, std::string *err);
int gcn_reach_read(const char *path, ReachCounts *out, std::string *err);
