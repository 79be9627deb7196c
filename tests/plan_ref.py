"""The schedule rules of csrc/plan.h stated in numpy: what test_plan_cpu.py compares the C++ against, and what
tools/gather_peak.py builds the product's own index stream from.  Host-side only."""
import numpy as np


def split_length(nnz, forced=0):
    """segment length of split rows: the forced value from 16 up, else 1024 halved while 8192 segments exceed nnz, 128 at least"""
    if forced >= 16:
        return int(forced)
    s = 1024
    while s > 128 and s * 8192 > nnz:
        s >>= 1
    return s


def neighbour_order(indptr, indices, col_deg=None):
    """the index array with every row's neighbours sorted by (-degree, id) — std::sort of pairs (-deg, id) in plan.h"""
    gp, gi = np.asarray(indptr, np.int64), np.asarray(indices, np.int64)
    deg = np.diff(gp) if col_deg is None else np.asarray(col_deg, np.int64)
    row_of = np.repeat(np.arange(gp.size - 1), np.diff(gp))
    return gi[np.lexsort((gi, -deg[gi], row_of))].astype(np.int32)


def row_order(indptr, key=None):
    """rows by (key ascending, degree descending), stable; key None: degree only"""
    deg = np.diff(np.asarray(indptr, np.int64))
    n = deg.size
    return np.lexsort((np.arange(n), -deg, np.zeros(n, np.int64) if key is None else np.asarray(key, np.int64)))


def dealt_key(indptr, n_groups):
    """degree rank dealt into n_groups groups (schedule mode 2)"""
    n = np.asarray(indptr).size - 1
    key = np.empty(n, np.int64)
    key[row_order(indptr)] = np.arange(n) % n_groups
    return key


def cut_segments(ptr, order, seg):
    """(tasks [T, 4] = {id, begin, end, slot or -1}, split [S, 4] = {id, first slot, segments, 0}, n_slots): one task per range
    in the given order, a range longer than seg in consecutive seg-long segments with consecutive slots"""
    ptr = np.asarray(ptr, np.int64)
    tasks, split, n_slots = [], [], 0
    for r in np.asarray(order).tolist():
        a, b = int(ptr[r]), int(ptr[r + 1])
        if b - a <= seg:
            tasks.append((r, a, b, -1))
            continue
        starts = range(a, b, seg)
        split.append((r, n_slots, len(starts), 0))
        tasks.extend((r, s, min(b, s + seg), n_slots + q) for q, s in enumerate(starts))
        n_slots += len(starts)
    return np.array(tasks, np.int32).reshape(-1, 4), np.array(split, np.int32).reshape(-1, 4), n_slots


def xcd_bounds(tasks):
    """[4, 9]: equal-work task ranges for 1/2/4/8 groups (work of a task: its edges + 8), each starting on a multiple of 4"""
    t = np.asarray(tasks, np.int64).reshape(-1, 4)
    prefix = np.concatenate([[0], np.cumsum(t[:, 2] - t[:, 1] + 8)])
    n = t.shape[0]
    out = np.full((4, 9), n, np.int32)
    for lg in range(4):
        G = 1 << lg
        out[lg, 0] = 0
        for k in range(1, G):
            b = int(np.searchsorted(prefix, int(prefix[-1]) * k // G, side="left"))
            out[lg, k] = max(min((b + 3) // 4 * 4, n), out[lg, k - 1])
    return out


def schedule_key(ds, schedule):
    """the row-group key the task list is sorted by (gcnhip_graph_set_schedule): labels, nothing, or degree rank dealt
    into G groups"""
    n = ds["num_nodes"]
    if schedule == "label-major":
        return ds["label"].astype(np.int64)
    if schedule.startswith("dealt-"):
        return dealt_key(ds["g_indptr"], int(schedule.split("-")[1]))
    return np.zeros(n, np.int64)


def product_order(ds, group_major=True, key=None, split=None):
    """the task list and index array as csrc/graph.hip builds them: neighbours of a row by descending degree (stable),
    rows by (group key, descending degree) — key = label when group_major, else none; rows above the split length
    (default: by the graph's size) in segments of that length -> (e0, e1, row of the task, indices)"""
    gp = ds["g_indptr"].astype(np.int64)
    if key is None:
        key = ds["label"].astype(np.int64) if group_major else None
    seg = split_length(int(gp[-1])) if split is None else split
    tasks, _, _ = cut_segments(gp, row_order(gp, key), seg)
    return tasks[:, 1].copy(), tasks[:, 2].copy(), tasks[:, 0].copy(), neighbour_order(gp, ds["g_indices"])
