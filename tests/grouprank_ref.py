"""The group ranking table (prb_grouprank, `ris -t -G FILE -R N`) restated in a few lines: the yardstick of
test_gpu_grouprank_kernel.py, test_gpu_grouprank.py and test_grouprank_cli.py."""
import numpy as np


def with_ids(recs, ids):
    """the records of GroupSet.finish(0) of one batch under the caller's identifiers: `query` becomes ids[query]"""
    out = recs.copy()
    out["query"] = np.asarray(ids, np.int32)[recs["query"]]
    return out


def rank(batches, n):
    """batches = GROUP_DTYPE arrays whose `query` is the identifier -> per group (ascending) the n records of lowest e_min -
    compared as floats, so -0.0 == +0.0; ties by identifier -, `rank` counted from 0 within the group"""
    batches = [b for b in batches if len(b)]
    if not batches:
        return None
    allr = np.concatenate(batches)
    out = []
    for g in sorted(set(int(x) for x in allr["group"])):
        rs = sorted((r for r in allr if int(r["group"]) == g), key=lambda r: (float(r["e_min"]), int(r["query"])))
        for k, r in enumerate(rs[:n]):
            r = r.copy()
            r["rank"] = k
            out.append(r)
    return np.array(out, allr.dtype)


def rank_bytes(batches, n):
    r = rank(batches, n)
    return b"" if r is None else r.tobytes()
