"""The yardstick of flx_summary (include/filtlong_hip.h): a plain numpy restatement of its definitions — a stable descending
sort, a cumulative sum and np.searchsorted against the edges the library exports.  Shared by the summary tests."""
import numpy as np

from filtlong_amd import api

FIELDS = api.SUMMARY_FIELDS
POW2 = 2 ** np.arange(1, 32, dtype=np.int64)  # bin b holds 2^b <= L < 2^(b+1); bin 0 holds 0 and 1


def q_hist(q, ln, edges):
    count, bases = np.zeros(52, np.int64), np.zeros(52, np.int64)
    if q is not None:
        q = np.asarray(q, dtype=np.float64)
        with np.errstate(invalid="ignore"):
            k = np.searchsorted(edges, q, side="right") - 1  # edges[k] <= q < edges[k+1]; 50: q >= edges[50]
            k[np.isnan(q) | (q < 0)] = 51
        np.add.at(count, k, 1)
        np.add.at(bases, k, ln)
    return [int(x) for x in count], [int(x) for x in bases]


def reference(lengths, mean_q=None, window_q=None, mask=None, edges=None):
    edges = api.summary_q_edges() if edges is None else edges
    ln = np.asarray(lengths, dtype=np.int64)
    keep = np.ones(len(ln), bool) if mask is None else np.asarray(mask) != 0
    ln = ln[keep]
    n, bases = len(ln), int(ln.sum())
    desc = ln[np.argsort(-ln, kind="stable")]
    cum = np.cumsum(desc)
    out = {"n": n, "bases": bases, "min_length": int(ln.min()) if n else 0, "max_length": int(ln.max()) if n else 0,
           "median_length": int(np.sort(ln, kind="stable")[(n - 1) // 2]) if n else 0, "nx": []}
    for x in range(10, 100, 10):  # the first entry at which 100 * cum >= x * bases, i.e. cum >= ceil(x * bases / 100)
        out["nx"].append(int(desc[np.searchsorted(cum, -(-x * bases // 100), side="left")]) if bases else 0)
    b = np.searchsorted(POW2, ln, side="right")
    lc, lb = np.zeros(32, np.int64), np.zeros(32, np.int64)
    np.add.at(lc, b, 1)
    np.add.at(lb, b, ln)
    out["len_count"], out["len_bases"] = [int(x) for x in lc], [int(x) for x in lb]
    out["mean_q_count"], out["mean_q_bases"] = q_hist(None if mean_q is None else np.asarray(mean_q)[keep], ln, edges)
    out["window_q_count"], out["window_q_bases"] = q_hist(None if window_q is None else np.asarray(window_q)[keep], ln, edges)
    return out


def diff(got, want):
    """The fields that differ (empty: equal in every field)."""
    return {k: (got[k], want[k]) for k in FIELDS if got[k] != want[k]}


def grid_constants():
    """(threads per workgroup, most workgroups) of the summary kernels, read from the header they are launched from."""
    import os
    import re
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "filtlong_amd", "csrc", "summary_select.h")).read()
    return tuple(int(re.search(r"constexpr int %s = (\d+);" % name, src).group(1)) for name in ("kThreads", "kMaxBlocks"))
