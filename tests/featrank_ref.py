"""The feature ranking table (prb_featrank, `ris -t -A FILE -B N`) restated in a few lines: the yardstick of
test_gpu_featrank_kernel.py, test_gpu_featrank.py and test_featrank_cli.py.  No *_ref.py module here restates the
library's energy key; like grouprank_ref.py this fold compares e_min as floats, which is the key's order: -0.0 == +0.0,
and no energy is a NaN."""
import numpy as np


def with_ids(recs, ids):
    """the FEATURE_DTYPE records of FeatSet.finish() of one batch as FEATRANK_DTYPE records under the caller's identifiers:
    `query` becomes ids[query], rank and reserved are 0"""
    from priblast_amd import capi
    out = np.zeros(len(recs), capi.FEATRANK_DTYPE)
    for name in capi.FEATURE_DTYPE.names:
        out[name] = recs[name]
    out["query"] = np.asarray(ids, np.int32)[recs["query"]]
    return out


def rank(batches, n):
    """batches = FEATRANK_DTYPE arrays whose `query` is the identifier -> per feature (ascending) the n records of lowest
    e_min, ties by identifier, `rank` counted from 0 within the feature and `reserved` 0; None without records"""
    batches = [b for b in batches if len(b)]
    if not batches:
        return None
    allr = np.concatenate(batches)
    by_feature = {}
    for i in range(len(allr)):  # 1. grouped by feature
        by_feature.setdefault(int(allr["feature"][i]), []).append(i)
    out = []
    for f in sorted(by_feature):
        order = sorted(by_feature[f], key=lambda i: (float(allr["e_min"][i]), int(allr["query"][i])))  # 2. ordered
        for k, i in enumerate(order[:n]):  # 3. cut, ranked
            r = allr[i].copy()
            r["rank"], r["reserved"] = k, 0
            out.append(r)
    return np.array(out, allr.dtype)


def rank_bytes(batches, n):
    r = rank(batches, n)
    return b"" if r is None else r.tobytes()
