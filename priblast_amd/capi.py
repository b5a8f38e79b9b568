"""ctypes binding of priblast_amd/lib/libpriblast_hip.so (include/priblast_hip.h).

This is plumbing for tests and bench.py; the product is the shared library and the
`pRIblast-hip` command line.  There is no CPU fallback: if the library is missing it raises,
and on a machine without a GPU `Context()` raises with the library's error text.
"""
import contextlib
import ctypes
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PRB_LIB_PATH") or os.path.join(ROOT, "lib", "libpriblast_hip.so")  # (PRB_LIB_PATH: developer builds)
BIN_PATH = os.path.join(ROOT, "bin", "pRIblast-hip")
PARAMS = os.path.join(ROOT, "params", "rna_andronescu2007.par")

c_i32, c_i64, c_dbl = ctypes.c_int32, ctypes.c_int64, ctypes.c_double
P = ctypes.POINTER


class RisOpts(ctypes.Structure):
    _fields_ = [("max_seed_length", c_i32), ("hybrid_threshold", c_dbl), ("interaction_threshold", c_dbl),
                ("final_threshold", c_dbl), ("drop_out_wo_gap", c_i32), ("drop_out_w_gap", c_i32),
                ("min_helix_length", c_i32), ("output_style", c_i32), ("distinct_sites", c_i32), ("chain_sites", c_i32),
                ("allowed_pairs", ctypes.c_void_p)]  # a prb_pairmask (PairMask.h), or None: every pair


class Hit(ctypes.Structure):
    _fields_ = [("q_sp", c_i32), ("db_sp", c_i32), ("q_len", c_i32), ("db_len", c_i32), ("db_id", c_i32),
                ("db_id_start", c_i32), ("e_acc", c_dbl), ("e_hyb", c_dbl), ("e_tot", c_dbl), ("query", c_i32),
                ("bp_count", c_i32), ("bp_offset", c_i64)]


class PageHits(ctypes.Structure):
    _fields_ = [("hits", ctypes.c_void_p), ("nhits", c_i64), ("basepairs", ctypes.c_void_p), ("npairs", c_i64)]


HIT_DTYPE = np.dtype([("q_sp", "<i4"), ("db_sp", "<i4"), ("q_len", "<i4"), ("db_len", "<i4"), ("db_id", "<i4"),
                      ("db_id_start", "<i4"), ("e_acc", "<f8"), ("e_hyb", "<f8"), ("e_tot", "<f8"),
                      ("query", "<i4"), ("bp_count", "<i4"), ("bp_offset", "<i8")])
assert HIT_DTYPE.itemsize == ctypes.sizeof(Hit)

# prb_pair_summary: one (query, database sequence) pair of prb_search_page_summary
PAIR_DTYPE = np.dtype([("query", "<i4"), ("db_id", "<i4"), ("hits", "<i8"), ("e_min", "<f8"), ("e_sum", "<f8"),
                       ("e_acc", "<f8"), ("e_hyb", "<f8"), ("bp_first", "<i4", (2,)), ("bp_last", "<i4", (2,))])
assert PAIR_DTYPE.itemsize == 64

# prb_top_pair: the embedded prb_pair_summary's fields, then the page it was found in and its rank within its query
TOP_DTYPE = np.dtype(PAIR_DTYPE.descr + [("page", "<i4"), ("rank", "<i4")])
assert TOP_DTYPE.itemsize == 72

# prb_top_hit: the embedded prb_hit's fields, then the page it was found in and its rank within its query
TOPHIT_DTYPE = np.dtype(HIT_DTYPE.descr + [("page", "<i4"), ("rank", "<i4")])
assert TOPHIT_DTYPE.itemsize == 72

# prb_target_pair: the embedded prb_pair_summary's fields (`query` = the query's identifier), then the target's page and the
# pair's rank within its target
TARGET_DTYPE = np.dtype(PAIR_DTYPE.descr + [("page", "<i4"), ("rank", "<i4")])
assert TARGET_DTYPE.itemsize == 72

# prb_profile_pos: one covered query position of the per-position profile (`ris -q`)
PROFILE_DTYPE = np.dtype([("query", "<i4"), ("pos", "<i4"), ("hits", "<i8"), ("targets", "<i4"), ("page", "<i4"),
                          ("db_id", "<i4"), ("reserved", "<i4"), ("e_min", "<f8"), ("bp_first", "<i4", (2,)),
                          ("bp_last", "<i4", (2,))])
assert PROFILE_DTYPE.itemsize == 56

# prb_target_region: one region of a target covered by at least D queries (`ris -c D`)
REGION_DTYPE = np.dtype([("page", "<i4"), ("db_id", "<i4"), ("start", "<i4"), ("end", "<i4"), ("hits", "<i8"),
                         ("max_hits", "<i8"), ("max_queries", "<i4"), ("peak", "<i4"), ("e_min", "<f8"), ("query", "<i4"),
                         ("reserved", "<i4"), ("bp_first", "<i4", (2,)), ("bp_last", "<i4", (2,))])
assert REGION_DTYPE.itemsize == 72

# prb_null_pair: the embedded prb_pair_summary's fields (the observed pair), then its page, the decoys per query and the
# null counters (`ris -t -z N`)
NULL_DTYPE = np.dtype(PAIR_DTYPE.descr + [("page", "<i4"), ("decoys", "<i4"), ("null_hits", "<i8"), ("null_le", "<i8"),
                                          ("null_min", "<f8")])
assert NULL_DTYPE.itemsize == 96
# prb_null_fdr (priblast_hip.h): the Benjamini-Hochberg figures of one record of NULL_DTYPE
FDR_DTYPE = np.dtype([("tests", "<i8"), ("rank", "<u4"), ("q_rank", "<u4"), ("q_num", "<u4"), ("q_den", "<u4")])
assert FDR_DTYPE.itemsize == 24

# prb_group_pair: the embedded prb_pair_summary's fields (the group's best member pair), then that pair's page, the group,
# the members with a hit, the rank within the query and the members' hits (`ris -t -G FILE`)
GROUP_DTYPE = np.dtype(PAIR_DTYPE.descr + [("page", "<i4"), ("group", "<i4"), ("members", "<i4"), ("rank", "<i4"), ("group_hits", "<i8")])
assert GROUP_DTYPE.itemsize == 88

# prb_gnull_pair: the embedded prb_group_pair's fields (the kept record), then the decoys per query and the null counters of
# the group (`ris -t -G FILE -P N`)
GNULL_DTYPE = np.dtype(GROUP_DTYPE.descr + [("decoys", "<i4"), ("pad", "<i4"), ("null_hits", "<i8"), ("null_le", "<i8"),
                                            ("null_min", "<f8")])
assert GNULL_DTYPE.itemsize == 120

# prb_feature_pair: the embedded prb_pair_summary's fields (over the feature's hits), then the target's page, the feature's
# index in the annotation and the hits wholly inside the feature (`ris -t -A FILE`)
FEATURE_DTYPE = np.dtype(PAIR_DTYPE.descr + [("page", "<i4"), ("feature", "<i4"), ("inside", "<i8")])
assert FEATURE_DTYPE.itemsize == 80

# prb_fnull_pair: the embedded prb_feature_pair's fields (the kept record), then the decoys per query and the null counters
# of the feature (`ris -t -A FILE -F N`)
FNULL_DTYPE = np.dtype(FEATURE_DTYPE.descr + [("decoys", "<i4"), ("pad", "<i4"), ("null_hits", "<i8"), ("null_le", "<i8"),
                                              ("null_min", "<f8")])
assert FNULL_DTYPE.itemsize == 112

# prb_featrank_pair: the embedded prb_feature_pair's fields with `query` = the query's identifier, then the rank within the
# feature (`ris -t -A FILE -B N`)
FEATRANK_DTYPE = np.dtype(FEATURE_DTYPE.descr + [("rank", "<i4"), ("reserved", "<i4")])
assert FEATRANK_DTYPE.itemsize == 88

# prb_eval_score: a real hit's place among its query's real hits and among the pooled hits of its decoys (`ris -k N -E M`)
EVAL_DTYPE = np.dtype([("decoys", "<i4"), ("reserved", "<i4"), ("null_le", "<i8"), ("rank", "<i8"), ("q_num", "<u4"), ("q_den", "<u4")])
assert EVAL_DTYPE.itemsize == 32


class PagePairs(ctypes.Structure):
    _fields_ = [("pairs", ctypes.c_void_p), ("npairs", c_i64)]

# every symbol include/priblast_hip.h declares: (restype, argtypes)
SYMBOLS = {
    "prb_last_error": (ctypes.c_char_p, []),
    "prb_version": (ctypes.c_char_p, []),
    "prb_cpu_budget": (ctypes.c_int, []),
    "prb_host_threads_default": (ctypes.c_int, []),
    "prb_seed_pair_layout": (ctypes.c_int, [c_i64, c_i64, c_i32, c_i32, c_i32, c_i32, P(c_i32)]),
    "prb_ris_opts_default": (None, [P(RisOpts)]),
    "prb_ctx_create": (ctypes.c_int, [ctypes.c_int, ctypes.c_char_p, P(ctypes.c_void_p)]),
    "prb_ctx_destroy": (None, [ctypes.c_void_p]),
    "prb_ctx_synchronize": (ctypes.c_int, [ctypes.c_void_p]),
    "prb_ctx_stage_ms": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_char_p, P(c_dbl), P(c_i64)]),
    "prb_ctx_reset_timers": (None, [ctypes.c_void_p]),
    "prb_accessibility": (ctypes.c_int, [ctypes.c_void_p, c_i32, ctypes.c_char_p, ctypes.c_void_p, c_i32, c_i32,
                                         ctypes.c_void_p, ctypes.c_void_p]),
    "prb_accessibility_tables": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_char_p, c_i32, c_i32, c_i32,
                                                ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                                ctypes.c_void_p]),
    "prb_encode_query": (ctypes.c_int, [ctypes.c_char_p, c_i32, c_i32, ctypes.c_void_p]),
    "prb_suffix_array": (ctypes.c_int, [ctypes.c_void_p, c_i32, ctypes.c_void_p]),
    "prb_db_open": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_char_p, P(ctypes.c_void_p)]),
    "prb_db_open_streaming": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_char_p, c_i32, P(ctypes.c_void_p)]),
    "prb_db_page_uploads": (c_i64, [ctypes.c_void_p]),
    "prb_db_close": (None, [ctypes.c_void_p]),
    "prb_db_info": (ctypes.c_int, [ctypes.c_void_p, P(c_i32), P(c_i32), P(c_i32), P(c_i32), P(c_i32)]),
    "prb_db_page_info": (ctypes.c_int, [ctypes.c_void_p, c_i32, P(c_i32), P(c_i64)]),
    "prb_db_seq_name": (ctypes.c_char_p, [ctypes.c_void_p, c_i32, c_i32]),
    "prb_db_seq_lengths": (ctypes.c_int, [ctypes.c_void_p, c_i32, c_i32, P(c_i32), P(c_i32), P(c_i32)]),
    "prb_db_build": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_char_p, c_i32, P(ctypes.c_char_p), ctypes.c_char_p,
                                    ctypes.c_void_p, c_i32, c_i32, c_i32, c_i32, c_i32]),
    "prb_qbatch_create": (ctypes.c_int, [ctypes.c_void_p, c_i32, ctypes.c_char_p, ctypes.c_void_p, c_i32,
                                         P(ctypes.c_void_p)]),
    "prb_qbatch_destroy": (None, [ctypes.c_void_p]),
    "prb_qbatch_accessibility": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, c_i32, c_i32]),
    "prb_qbatch_get": (ctypes.c_int, [ctypes.c_void_p, c_i32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                      ctypes.c_void_p]),
    "prb_qbatch_length_unmasked": (c_i32, [ctypes.c_void_p, c_i32]),
    "prb_qbatch_seed_search_begin": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, c_i32, P(RisOpts)]),
    "prb_search_page": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, c_i32, P(RisOpts), c_i32,
                                       P(ctypes.c_void_p)]),
    "prb_pairmask_create": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, P(ctypes.c_void_p)]),
    "prb_pairmask_allow": (ctypes.c_int, [ctypes.c_void_p, c_i64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "prb_pairmask_count": (c_i64, [ctypes.c_void_p]),
    "prb_pairmask_row_words": (c_i64, [ctypes.c_void_p]),
    "prb_pairmask_words": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, c_i64]),
    "prb_pairmask_create_live": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, c_i32, P(ctypes.c_void_p)]),
    "prb_pairmask_free": (None, [ctypes.c_void_p]),
    "prb_hitset_size": (c_i64, [ctypes.c_void_p]),
    "prb_hitset_hits": (ctypes.c_void_p, [ctypes.c_void_p]),
    "prb_hitset_basepairs": (ctypes.c_void_p, [ctypes.c_void_p, P(c_i64)]),
    "prb_hitset_counts": (None, [ctypes.c_void_p, P(c_i64)]),
    "prb_hitset_free": (None, [ctypes.c_void_p]),
    "prb_distinct_sites": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, c_i64, ctypes.c_void_p]),
    "prb_chain_sites": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, c_i64, ctypes.c_void_p]),
    "prb_sort_filter": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, c_i64, c_dbl, ctypes.c_void_p, ctypes.c_void_p,
                                       ctypes.c_void_p]),
    "prb_search_page_summary": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, c_i32, P(RisOpts),
                                               P(ctypes.c_void_p)]),
    "prb_pairset_size": (c_i64, [ctypes.c_void_p]),
    "prb_pairset_pairs": (ctypes.c_void_p, [ctypes.c_void_p]),
    "prb_pairset_counts": (None, [ctypes.c_void_p, P(c_i64)]),
    "prb_pairset_free": (None, [ctypes.c_void_p]),
    "prb_topset_create": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, c_i32, P(ctypes.c_void_p)]),
    "prb_search_page_top": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, c_i32, P(RisOpts), ctypes.c_void_p]),
    "prb_topset_merge": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "prb_topset_finish": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p]),
    "prb_topset_size": (c_i64, [ctypes.c_void_p]),
    "prb_topset_pairs": (ctypes.c_void_p, [ctypes.c_void_p]),
    "prb_topset_counts": (None, [ctypes.c_void_p, P(c_i64)]),
    "prb_topset_free": (None, [ctypes.c_void_p]),
    "prb_tophits_create": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, c_i32, P(ctypes.c_void_p)]),
    "prb_search_page_tophits": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, c_i32, P(RisOpts), ctypes.c_void_p]),
    "prb_tophits_merge": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "prb_tophits_finish": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p]),
    "prb_tophits_size": (c_i64, [ctypes.c_void_p]),
    "prb_tophits_hits": (ctypes.c_void_p, [ctypes.c_void_p]),
    "prb_tophits_basepairs": (ctypes.c_void_p, [ctypes.c_void_p, P(c_i64)]),
    "prb_tophits_counts": (None, [ctypes.c_void_p, P(c_i64)]),
    "prb_tophits_free": (None, [ctypes.c_void_p]),
    "prb_profset_create": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, P(ctypes.c_void_p)]),
    "prb_search_page_profile": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, c_i32, P(RisOpts), ctypes.c_void_p]),
    "prb_profset_merge": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "prb_profset_finish": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p]),
    "prb_profset_size": (c_i64, [ctypes.c_void_p]),
    "prb_profset_rows": (ctypes.c_void_p, [ctypes.c_void_p]),
    "prb_profset_counts": (None, [ctypes.c_void_p, P(c_i64)]),
    "prb_profset_free": (None, [ctypes.c_void_p]),
    "prb_targetset_create": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, c_i32, P(ctypes.c_void_p)]),
    "prb_search_page_targets": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, c_i32, P(RisOpts), ctypes.c_void_p,
                                               ctypes.c_void_p]),
    "prb_targetset_merge": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "prb_targetset_finish": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p]),
    "prb_targetset_size": (c_i64, [ctypes.c_void_p]),
    "prb_targetset_pairs": (ctypes.c_void_p, [ctypes.c_void_p]),
    "prb_targetset_counts": (None, [ctypes.c_void_p, P(c_i64)]),
    "prb_targetset_free": (None, [ctypes.c_void_p]),
    "prb_covset_create": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, P(ctypes.c_void_p)]),
    "prb_search_page_coverage": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, c_i32, P(RisOpts), ctypes.c_void_p,
                                                ctypes.c_void_p]),
    "prb_covset_add_hits": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, c_i32, ctypes.c_void_p, c_i32, ctypes.c_void_p, c_i64,
                                           ctypes.c_void_p, c_i64]),
    "prb_covset_merge": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "prb_covset_finish": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, c_i32]),
    "prb_covset_size": (c_i64, [ctypes.c_void_p]),
    "prb_covset_regions": (ctypes.c_void_p, [ctypes.c_void_p]),
    "prb_covset_counts": (None, [ctypes.c_void_p, P(c_i64)]),
    "prb_covset_free": (None, [ctypes.c_void_p]),
    "prb_nullset_create": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, c_i32, P(ctypes.c_void_p)]),
    "prb_search_page_observed": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, c_i32, P(RisOpts), ctypes.c_void_p]),
    "prb_search_page_decoys": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, c_i32, P(RisOpts), ctypes.c_void_p,
                                              ctypes.c_void_p, ctypes.c_void_p]),
    "prb_nullset_observe": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, c_i32, ctypes.c_void_p, c_i64]),
    "prb_nullset_add_pairs": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, c_i32, ctypes.c_void_p, ctypes.c_void_p, c_i32,
                                             ctypes.c_void_p, c_i64]),
    "prb_nullset_retire": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, c_i64, c_i32, ctypes.c_void_p]),
    "prb_nullset_finish": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p]),
    "prb_nullset_finish_fdr": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "prb_nullset_fdr": (ctypes.c_void_p, [ctypes.c_void_p]),
    "prb_fdr_chunk": (c_i32, []),
    "prb_nullset_size": (c_i64, [ctypes.c_void_p]),
    "prb_nullset_pairs": (ctypes.c_void_p, [ctypes.c_void_p]),
    "prb_nullset_counts": (None, [ctypes.c_void_p, P(c_i64)]),
    "prb_nullset_decoy_counts": (None, [ctypes.c_void_p, P(c_i64)]),
    "prb_nullset_free": (None, [ctypes.c_void_p]),
    "prb_write_null_lines": (ctypes.c_int, [ctypes.c_void_p, c_i32, P(ctypes.c_char_p), ctypes.c_void_p, ctypes.c_void_p, c_i64,
                                            c_i64, ctypes.c_int, P(c_i64), P(c_i64)]),
    "prb_write_null_fdr_lines": (ctypes.c_int, [ctypes.c_void_p, c_i32, P(ctypes.c_char_p), ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                                c_i64, c_i64, ctypes.c_int, P(c_i64), P(c_i64)]),
    "prb_groupset_create": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, P(ctypes.c_void_p), c_i32, P(ctypes.c_void_p)]),
    "prb_search_page_groups": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, c_i32, P(RisOpts), ctypes.c_void_p]),
    "prb_groupset_add_pairs": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, c_i32, ctypes.c_void_p, c_i64]),
    "prb_groupset_merge": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "prb_groupset_finish": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, c_i32]),
    "prb_groupset_size": (c_i64, [ctypes.c_void_p]),
    "prb_groupset_pairs": (ctypes.c_void_p, [ctypes.c_void_p]),
    "prb_groupset_counts": (None, [ctypes.c_void_p, P(c_i64)]),
    "prb_groupset_free": (None, [ctypes.c_void_p]),
    "prb_write_group_lines": (ctypes.c_int, [ctypes.c_void_p, c_i32, P(ctypes.c_char_p), ctypes.c_void_p, ctypes.c_void_p, c_i64,
                                             P(ctypes.c_char_p), ctypes.c_void_p, c_i32, c_i64, ctypes.c_int, P(c_i64), P(c_i64)]),
    "prb_grouprank_create": (ctypes.c_int, [ctypes.c_void_p, c_i32, c_i32, P(ctypes.c_void_p)]),
    "prb_grouprank_add_groupset": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "prb_grouprank_add_records": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, c_i64]),
    "prb_grouprank_merge": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "prb_grouprank_finish": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p]),
    "prb_grouprank_size": (c_i64, [ctypes.c_void_p]),
    "prb_grouprank_pairs": (ctypes.c_void_p, [ctypes.c_void_p]),
    "prb_grouprank_counts": (None, [ctypes.c_void_p, P(c_i64)]),
    "prb_grouprank_free": (None, [ctypes.c_void_p]),
    "prb_write_grouprank_lines": (ctypes.c_int, [ctypes.c_void_p, c_i32, P(ctypes.c_char_p), ctypes.c_void_p, ctypes.c_void_p, c_i64,
                                                 P(ctypes.c_char_p), ctypes.c_void_p, c_i32, c_i64, ctypes.c_int, P(c_i64), P(c_i64)]),
    "prb_gnullset_create": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, c_i32, c_i32, P(ctypes.c_void_p)]),
    "prb_gnullset_begin": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, c_i32]),
    "prb_search_page_gnull": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, c_i32, P(RisOpts), ctypes.c_void_p]),
    "prb_gnullset_add_pairs": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, c_i32, ctypes.c_void_p, c_i64]),
    "prb_gnullset_end": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p]),
    "prb_gnullset_finish": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p]),
    "prb_gnullset_size": (c_i64, [ctypes.c_void_p]),
    "prb_gnullset_pairs": (ctypes.c_void_p, [ctypes.c_void_p]),
    "prb_gnullset_decoy_counts": (None, [ctypes.c_void_p, P(c_i64)]),
    "prb_gnullset_free": (None, [ctypes.c_void_p]),
    "prb_write_gnull_lines": (ctypes.c_int, [ctypes.c_void_p, c_i32, P(ctypes.c_char_p), ctypes.c_void_p, ctypes.c_void_p, c_i64,
                                             P(ctypes.c_char_p), ctypes.c_void_p, c_i32, c_i64, ctypes.c_int, P(c_i64), P(c_i64)]),
    "prb_evalset_create": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, c_i32, P(ctypes.c_void_p)]),
    "prb_search_page_scored": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, c_i32, P(RisOpts), ctypes.c_void_p,
                                              ctypes.c_void_p]),
    "prb_search_page_null_hits": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, c_i32, P(RisOpts), ctypes.c_void_p,
                                                 ctypes.c_void_p, ctypes.c_void_p]),
    "prb_evalset_add_keys": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, c_i32, ctypes.c_void_p, ctypes.c_void_p, c_i64]),
    "prb_evalset_close": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p]),
    "prb_evalset_score": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, c_i64, ctypes.c_void_p]),
    "prb_evalset_sizes": (None, [ctypes.c_void_p, P(c_i64), P(c_i64)]),
    "prb_evalset_counts": (None, [ctypes.c_void_p, P(c_i64)]),
    "prb_evalset_decoy_counts": (None, [ctypes.c_void_p, P(c_i64)]),
    "prb_evalset_free": (None, [ctypes.c_void_p]),
    "prb_annot_create": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, c_i64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                        ctypes.c_void_p, P(ctypes.c_void_p)]),
    "prb_annot_count": (c_i64, [ctypes.c_void_p]),
    "prb_annot_free": (None, [ctypes.c_void_p]),
    "prb_featset_create": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, P(ctypes.c_void_p)]),
    "prb_search_page_features": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, c_i32, P(RisOpts), ctypes.c_void_p]),
    "prb_featset_add_hits": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, c_i32, ctypes.c_void_p, c_i64, ctypes.c_void_p, c_i64]),
    "prb_featset_merge": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "prb_featset_finish": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p]),
    "prb_featset_finish_top": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, c_i32]),
    "prb_featset_size": (c_i64, [ctypes.c_void_p]),
    "prb_featset_records": (ctypes.c_void_p, [ctypes.c_void_p]),
    "prb_featset_counts": (None, [ctypes.c_void_p, P(c_i64)]),
    "prb_featset_unassigned": (c_i64, [ctypes.c_void_p]),
    "prb_featset_free": (None, [ctypes.c_void_p]),
    "prb_fnullset_create": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, c_i32, P(ctypes.c_void_p)]),
    "prb_fnullset_create_top": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, c_i32, c_i32, P(ctypes.c_void_p)]),
    "prb_fnullset_begin": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, c_i32]),
    "prb_search_page_fnull": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, c_i32, P(RisOpts), ctypes.c_void_p]),
    "prb_fnullset_add_hits": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, c_i32, ctypes.c_void_p, c_i64, ctypes.c_void_p, c_i64]),
    "prb_fnullset_end": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p]),
    "prb_fnullset_finish": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p]),
    "prb_fnullset_size": (c_i64, [ctypes.c_void_p]),
    "prb_fnullset_records": (ctypes.c_void_p, [ctypes.c_void_p]),
    "prb_fnullset_decoy_counts": (None, [ctypes.c_void_p, P(c_i64)]),
    "prb_fnullset_free": (None, [ctypes.c_void_p]),
    "prb_write_fnull_lines": (ctypes.c_int, [ctypes.c_void_p, c_i32, P(ctypes.c_char_p), ctypes.c_void_p, ctypes.c_void_p, c_i64,
                                             P(ctypes.c_char_p), ctypes.c_void_p, ctypes.c_void_p, c_i64, c_i64, ctypes.c_int, P(c_i64),
                                             P(c_i64)]),
    "prb_write_feature_lines": (ctypes.c_int, [ctypes.c_void_p, c_i32, P(ctypes.c_char_p), ctypes.c_void_p, ctypes.c_void_p, c_i64,
                                               P(ctypes.c_char_p), ctypes.c_void_p, ctypes.c_void_p, c_i64, c_i64, ctypes.c_int, P(c_i64),
                                               P(c_i64)]),
    "prb_featrank_create": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, c_i32, P(ctypes.c_void_p)]),
    "prb_featrank_add_featset": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "prb_featrank_add_records": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, c_i64]),
    "prb_featrank_merge": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "prb_featrank_finish": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p]),
    "prb_featrank_size": (c_i64, [ctypes.c_void_p]),
    "prb_featrank_records": (ctypes.c_void_p, [ctypes.c_void_p]),
    "prb_featrank_counts": (None, [ctypes.c_void_p, P(c_i64)]),
    "prb_featrank_unassigned": (c_i64, [ctypes.c_void_p]),
    "prb_featrank_free": (None, [ctypes.c_void_p]),
    "prb_write_featrank_lines": (ctypes.c_int, [ctypes.c_void_p, c_i32, P(ctypes.c_char_p), ctypes.c_void_p, ctypes.c_void_p, c_i64,
                                                P(ctypes.c_char_p), ctypes.c_void_p, ctypes.c_void_p, c_i64, c_i64, ctypes.c_int, P(c_i64),
                                                P(c_i64)]),
    "prb_comm_unique_id": (ctypes.c_int, [ctypes.c_char_p]),
    "prb_comm_create": (ctypes.c_int, [ctypes.c_void_p, c_i32, c_i32, ctypes.c_char_p, P(ctypes.c_void_p)]),
    "prb_comm_destroy": (None, [ctypes.c_void_p]),
    "prb_gather_hits": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, c_i32, ctypes.c_void_p, c_i32, P(ctypes.c_void_p)]),
    "prb_hitset_gathered_queries": (ctypes.c_int, [ctypes.c_void_p, P(c_i32), P(P(c_i32)), P(P(c_i32))]),
    "prb_gather_plan": (ctypes.c_int, [c_i32, ctypes.c_void_p, ctypes.c_void_p]),
    "prb_ctx_keep_device_records": (None, [ctypes.c_void_p, c_i32]),
    "prb_write_lines": (ctypes.c_int, [ctypes.c_void_p, c_i32, P(ctypes.c_char_p), ctypes.c_void_p, ctypes.c_void_p, c_i32,
                                       c_i32, c_i64, ctypes.c_int, P(c_i64), P(c_i64)]),
    "prb_write_summary_lines": (ctypes.c_int, [ctypes.c_void_p, c_i32, P(ctypes.c_char_p), ctypes.c_void_p, ctypes.c_void_p,
                                               c_i32, c_i64, ctypes.c_int, P(c_i64), P(c_i64)]),
    "prb_write_top_lines": (ctypes.c_int, [ctypes.c_void_p, c_i32, P(ctypes.c_char_p), ctypes.c_void_p, ctypes.c_void_p, c_i64,
                                           c_i64, ctypes.c_int, P(c_i64), P(c_i64)]),
    "prb_shuffle_sequence": (ctypes.c_int, [ctypes.c_char_p, c_i32, ctypes.c_uint64, c_i64, c_i32, ctypes.c_char_p]),
    "prb_write_target_lines": (ctypes.c_int, [ctypes.c_void_p, c_i32, P(ctypes.c_char_p), ctypes.c_void_p, ctypes.c_void_p, c_i64,
                                              c_i64, ctypes.c_int, P(c_i64), P(c_i64)]),
    "prb_write_profile_lines": (ctypes.c_int, [ctypes.c_void_p, c_i32, P(ctypes.c_char_p), ctypes.c_void_p, ctypes.c_void_p, c_i64,
                                               c_i64, ctypes.c_int, P(c_i64), P(c_i64)]),
    "prb_write_region_lines": (ctypes.c_int, [ctypes.c_void_p, c_i32, P(ctypes.c_char_p), ctypes.c_void_p, ctypes.c_void_p, c_i64,
                                              c_i64, ctypes.c_int, P(c_i64), P(c_i64)]),
}

_lib = None


def build():
    """Compile the HIP library (and the ris driver) in-tree for gfx950."""
    subprocess.run(["make", "-s", "-j8", "-C", os.path.join(ROOT, "csrc")], check=True)


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                               "(there is no CPU fallback)")
        L = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SYMBOLS.items():
            if not hasattr(L, name):  # reported by tests/test_host.py, not here
                continue
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


class PrbError(RuntimeError):
    pass


def _check(rc):
    if rc != 0:
        raise PrbError(f"libpriblast_hip error {rc}: {lib().prb_last_error().decode()}")


def _concat(seqs):
    offs = np.zeros(len(seqs) + 1, np.int64)
    for i, s in enumerate(seqs):
        offs[i + 1] = offs[i] + len(s)
    return "".join(seqs).encode(), offs


def encode_query(seq, repeat_flag=0):
    enc = np.zeros(len(seq) + 1, np.uint8)
    _check(lib().prb_encode_query(seq.encode(), len(seq), repeat_flag, enc.ctypes.data))
    return enc


def suffix_array(text):
    text = np.ascontiguousarray(text, np.uint8)
    sa = np.zeros(len(text), np.int32)
    _check(lib().prb_suffix_array(text.ctypes.data, len(text), sa.ctypes.data))
    return sa


def shuffle_sequence(seq, seed=1, file_pos=0, decoy=0):
    """prb_shuffle_sequence: the dinucleotide-preserving decoy of seq (str or bytes) -> the same type"""
    raw = seq.encode("latin-1") if isinstance(seq, str) else bytes(seq)
    out = ctypes.create_string_buffer(max(len(raw), 1))
    _check(lib().prb_shuffle_sequence(raw, len(raw), seed, file_pos, decoy, out))
    res = out.raw[:len(raw)]
    return res.decode("latin-1") if isinstance(seq, str) else res


def seed_pair_layout(nchars, query_span, row_shift=7, sort_bits=16, local_order=True, pair_wide=False):
    """prb_seed_pair_layout -> dict(narrow, pbits, kbits, begin, local_bits, wide_key)"""
    out = (c_i32 * 6)()
    _check(lib().prb_seed_pair_layout(nchars, query_span, row_shift, sort_bits, int(local_order), int(pair_wide), out))
    return dict(narrow=bool(out[0]), pbits=out[1], kbits=out[2], begin=out[3], local_bits=out[4], wide_key=bool(out[5]))


def default_opts(**kw):
    o = RisOpts()
    lib().prb_ris_opts_default(ctypes.byref(o))
    for k, v in kw.items():
        setattr(o, k, v)
    return o


class Context:
    def __init__(self, device=0, param_file=None):
        h = ctypes.c_void_p()
        _check(lib().prb_ctx_create(device, param_file.encode() if param_file else PARAMS.encode(), ctypes.byref(h)))
        self.h = h

    def close(self):
        if self.h:
            lib().prb_ctx_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def accessibility(self, seqs, W=70, delta=5):
        """Raccess for a list of sequences -> list of (acc, cond) float32 arrays."""
        buf, offs = _concat(seqs)
        total = int(offs[-1])
        acc = np.zeros(max(total, 1), np.float32)
        cond = np.zeros(max(total, 1), np.float32)
        _check(lib().prb_accessibility(self.h, len(seqs), buf, offs.ctypes.data, W, delta, acc.ctypes.data,
                                       cond.ctypes.data))
        return [(acc[offs[i]:offs[i + 1]], cond[offs[i]:offs[i + 1]]) for i in range(len(seqs))]

    def accessibility_tables(self, seq, W=70, delta=5):
        L = len(seq)
        acc = np.zeros(max(L, 1), np.float32)
        cond = np.zeros(max(L, 1), np.float32)
        out = {"alpha_outer": np.zeros(L + 1), "beta_outer": np.zeros(L + 1)}
        names = ["stem", "stemend", "multi", "multibif", "multi1", "multi2"]
        ptrs = (ctypes.c_void_p * 12)()
        k = 0
        for side in ("alpha", "beta"):
            for nm in names:
                t = np.zeros((L + 1, W + 2))
                out[f"{side}_{nm}"] = t
                ptrs[k] = t.ctypes.data
                k += 1
        _check(lib().prb_accessibility_tables(self.h, seq.encode(), L, W, delta, acc.ctypes.data, cond.ctypes.data,
                                              out["alpha_outer"].ctypes.data, out["beta_outer"].ctypes.data, ptrs))
        return acc[:L], cond[:L], out

    def stage_ms(self, stage):
        ms, n = c_dbl(), c_i64()
        _check(lib().prb_ctx_stage_ms(self.h, stage.encode(), ctypes.byref(ms), ctypes.byref(n)))
        return ms.value, n.value

    def reset_timers(self):
        lib().prb_ctx_reset_timers(self.h)

    def synchronize(self):
        _check(lib().prb_ctx_synchronize(self.h))


class Db:
    """Database pages resident in HBM (prb_db_open)."""

    def __init__(self, ctx, prefix, max_resident_pages=None):
        h = ctypes.c_void_p()
        if max_resident_pages is None:
            _check(lib().prb_db_open(ctx.h, prefix.encode(), ctypes.byref(h)))
        else:
            _check(lib().prb_db_open_streaming(ctx.h, prefix.encode(), max_resident_pages, ctypes.byref(h)))
        self.h, self.ctx = h, ctx
        v = [c_i32() for _ in range(5)]
        _check(lib().prb_db_info(self.h, *[ctypes.byref(x) for x in v]))
        self.hash_size, self.repeat_flag, self.W, self.delta, self.npages = (x.value for x in v)

    def close(self):
        if self.h:
            lib().prb_db_close(self.h)
            self.h = None

    @property
    def page_uploads(self):
        return lib().prb_db_page_uploads(self.h)

    def page_info(self, page):
        n, c = c_i32(), c_i64()
        _check(lib().prb_db_page_info(self.h, page, ctypes.byref(n), ctypes.byref(c)))
        return n.value, c.value

    def seq_name(self, page, i):
        return lib().prb_db_seq_name(self.h, page, i).decode()

    def seq_lengths(self, page, i):
        a, b, c = c_i32(), c_i32(), c_i32()
        _check(lib().prb_db_seq_lengths(self.h, page, i, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)))
        return a.value, b.value, c.value


def db_build(ctx, prefix, names, seqs, repeat_flag=0, hash_size=8, W=70, delta=5, page_size=2 ** 31 - 1):
    buf, offs = _concat(seqs)
    arr = (ctypes.c_char_p * len(names))(*[n.encode() for n in names])
    _check(lib().prb_db_build(ctx.h, prefix.encode(), len(seqs), arr, buf, offs.ctypes.data, repeat_flag, hash_size, W,
                              delta, page_size))


class QBatch:
    """A batch of queries: encoded + suffix arrays (host), accessibilities (GPU)."""

    def __init__(self, ctx, seqs, repeat_flag=0):
        buf, offs = _concat(seqs)
        h = ctypes.c_void_p()
        _check(lib().prb_qbatch_create(ctx.h, len(seqs), buf, offs.ctypes.data, repeat_flag, ctypes.byref(h)))
        self.h, self.ctx, self.lens = h, ctx, [len(s) for s in seqs]

    def close(self):
        if self.h:
            lib().prb_qbatch_destroy(self.h)
            self.h = None

    def accessibility(self, W, delta):
        _check(lib().prb_qbatch_accessibility(self.ctx.h, self.h, W, delta))

    def get(self, q):
        L = self.lens[q]
        enc = np.zeros(L + 1, np.uint8)
        sa = np.zeros(L + 1, np.int32)
        acc = np.zeros(max(L, 1), np.float32)
        cond = np.zeros(max(L, 1), np.float32)
        _check(lib().prb_qbatch_get(self.h, q, enc.ctypes.data, sa.ctypes.data, acc.ctypes.data, cond.ctypes.data))
        return enc, sa, acc[:L], cond[:L]

    def length_unmasked(self, q):
        return lib().prb_qbatch_length_unmasked(self.h, q)

    def seed_search_begin(self, db, page, opts=None):
        """starts the seed DFS against `page` in the background; a later search_page with the same options uses it"""
        o = opts or default_opts()
        _check(lib().prb_qbatch_seed_search_begin(self.ctx.h, self.h, db.h, page, ctypes.byref(o)))


class PairMask:
    """A prb_pairmask: the (query, target) pairs a search of `qb` against `db` is restricted to.  Give it to a search as
    default_opts(allowed_pairs=mask.h); it must outlive the searches that use it."""

    def __init__(self, ctx, qb, db):
        h = ctypes.c_void_p()
        _check(lib().prb_pairmask_create(ctx.h, qb.h, db.h, ctypes.byref(h)))
        self.h = h

    @classmethod
    def live(cls, ctx, ns, dqb, owner):
        """prb_pairmask_create_live: the mask of the decoy batch dqb from the live pairs of the NullSet ns, made on the
        device; row k = the live pairs of query owner[k]"""
        owner = np.ascontiguousarray(owner, np.int32)
        self = cls.__new__(cls)
        self.h = None
        h = ctypes.c_void_p()
        _check(lib().prb_pairmask_create_live(ctx.h, ns.h, dqb.h, owner.ctypes.data if len(owner) else None, len(owner), ctypes.byref(h)))
        self.h = h
        return self

    def allow(self, query, page, db_id):
        """arrays of equal length; query -1 = every query of the batch"""
        q, p, d = (np.ascontiguousarray(np.atleast_1d(x), np.int32) for x in (query, page, db_id))
        assert len(q) == len(p) == len(d)
        _check(lib().prb_pairmask_allow(self.h, len(q), q.ctypes.data, p.ctypes.data, d.ctypes.data))
        return self

    @property
    def count(self):
        return lib().prb_pairmask_count(self.h)

    def words(self, nrows):
        """prb_pairmask_words -> uint32 [nrows, row_words]: the rows as a search reads them"""
        rw = lib().prb_pairmask_row_words(self.h)
        out = np.zeros((nrows, rw), np.uint32)
        _check(lib().prb_pairmask_words(self.h, out.ctypes.data if out.size else None, out.size))
        return out

    def close(self):
        if self.h:
            lib().prb_pairmask_free(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


class _HitSetOwner:
    """Frees the prb_hitset when the last numpy view of it goes away."""

    def __init__(self, handle):
        self.h = handle

    def __del__(self):
        lib().prb_hitset_free(self.h)


class _HitSetView:
    """Array-interface window on memory of a hit set: numpy arrays made from it alias the
    library's memory (no copy) and keep the owner alive through their .base chain."""

    def __init__(self, owner, ptr, nbytes):
        self._owner = owner
        self.__array_interface__ = {"shape": (nbytes,), "typestr": "|u1", "data": (ptr, False), "version": 3}


class HitSet:
    """A prb_hitset: .hits (structured array HIT_DTYPE) and .bp (int32 [n, 2]) are views of the library's
    memory (no copy); they keep the hit set alive, which is freed when the last of them goes away."""

    def __init__(self, handle):
        self._owner = _HitSetOwner(handle)
        self.h = handle
        counts = (c_i64 * 3)()
        lib().prb_hitset_counts(handle, counts)
        self.counts = tuple(counts)
        n = lib().prb_hitset_size(handle)
        cnt = c_i64()
        p = lib().prb_hitset_basepairs(handle, ctypes.byref(cnt))
        if n:
            self.hits = np.asarray(_HitSetView(self._owner, lib().prb_hitset_hits(handle), n * HIT_DTYPE.itemsize)).view(HIT_DTYPE)
        else:
            self.hits = np.zeros(0, HIT_DTYPE)
        if cnt.value:
            self.bp = np.asarray(_HitSetView(self._owner, p, cnt.value * 8)).view(np.int32).reshape(-1, 2)
        else:
            self.bp = np.zeros((0, 2), np.int32)


def search_page_hs(ctx, qb, db, page, opts=None, last_stage=3):
    """prb_search_page -> HitSet"""
    o = opts or default_opts()
    h = ctypes.c_void_p()
    _check(lib().prb_search_page(ctx.h, qb.h, db.h, page, ctypes.byref(o), last_stage, ctypes.byref(h)))
    return HitSet(h)


def search_page(ctx, qb, db, page, opts=None, last_stage=3):
    """-> (hits: structured array HIT_DTYPE, bp: int32 [n,2], counts (seed, ungapped, final)).
    The arrays are views of the hit set (freed when the last of them goes away)."""
    hs = search_page_hs(ctx, qb, db, page, opts, last_stage)
    return hs.hits, hs.bp, hs.counts


def distinct_sites(ctx, hits):
    """prb_distinct_sites: hits = structured array HIT_DTYPE (a caller's list of final hits) -> uint8 [n], 1 for the hits
    that the selection of opts.distinct_sites keeps within their run of equal (query, db_id)"""
    hits = np.ascontiguousarray(hits, HIT_DTYPE)
    keep = np.zeros(len(hits), np.uint8)
    _check(lib().prb_distinct_sites(ctx.h, hits.ctypes.data if len(hits) else None, len(hits),
                                    keep.ctypes.data if len(hits) else None))
    return keep


def chain_sites(ctx, hits):
    """prb_chain_sites: hits = structured array HIT_DTYPE (a caller's list of final hits, db_sp not decreasing inside a run
    of equal (query, db_id)) -> uint8 [n], 1 for the hits of their run's best co-linear chain (opts.chain_sites)"""
    hits = np.ascontiguousarray(hits, HIT_DTYPE)
    keep = np.zeros(len(hits), np.uint8)
    _check(lib().prb_chain_sites(ctx.h, hits.ctypes.data if len(hits) else None, len(hits),
                                 keep.ctypes.data if len(hits) else None))
    return keep


# prb_sort_filter's *form (include/priblast_hip.h)
SORT_PACKED_TWO_LENGTHS, SORT_PACKED_ONE_LENGTH, SORT_GENERAL_WIDTH, SORT_GENERAL_TIE_RUN, SORT_GENERAL_FORCED = range(5)


def sort_filter(ctx, hits, threshold):
    """prb_sort_filter: hits = structured array HIT_DTYPE in any order -> (the records in the stages' sorted order, uint8
    [n] keep flags of the redundancy filter by sorted position, the SORT_* form of the sort that ran; None for no hits)"""
    hits = np.ascontiguousarray(hits, HIT_DTYPE)
    n = len(hits)
    out = np.zeros(n, HIT_DTYPE)
    keep = np.zeros(n, np.uint8)
    form = np.full(1, -1, np.int32)
    _check(lib().prb_sort_filter(ctx.h, hits.ctypes.data if n else None, n, float(threshold), out.ctypes.data if n else None,
                                 keep.ctypes.data if n else None, form.ctypes.data))
    return out, keep, int(form[0]) if n else None


def search_page_summary(ctx, qb, db, page, opts=None, with_counts=False):
    """prb_search_page_summary -> structured array PAIR_DTYPE (a copy): one record per (query, database sequence) pair
    with final hits, in output order.  with_counts: -> (records, (seed, ungapped, final) counts)."""
    o = opts or default_opts()
    h = ctypes.c_void_p()
    _check(lib().prb_search_page_summary(ctx.h, qb.h, db.h, page, ctypes.byref(o), ctypes.byref(h)))
    try:
        pairs = _records(lib().prb_pairset_pairs(h), lib().prb_pairset_size(h), PAIR_DTYPE)
        counts = (c_i64 * 3)()
        lib().prb_pairset_counts(h, counts)
    finally:
        lib().prb_pairset_free(h)
    return (pairs, tuple(counts)) if with_counts else pairs


def _records(ptr, n, dtype):
    """n records of `dtype` at `ptr` in the library's memory -> structured array (a copy)"""
    if not n:
        return np.zeros(0, dtype)
    return np.frombuffer((ctypes.c_char * (n * dtype.itemsize)).from_address(ptr), dtype).copy()


class _Table:
    """A result table on the device, whichever it is made for: prb_<PREFIX>_merge / _finish / _counts / _free."""
    PREFIX = None

    def _fn(self, name):
        return getattr(lib(), f"prb_{self.PREFIX}_{name}")

    def absorb(self, other):
        """prb_<PREFIX>_merge: the unfinished table `other` (over other pages - or other (identifier, page) sets - of the
        same queries or database; of any context) merged into this one on the device; `other` is left empty"""
        _check(self._fn("merge")(self.ctx.h, self.h, other.h))

    def _finish(self, records, dtype, *finish_args):
        """prb_<PREFIX>_finish -> the records that prb_<PREFIX>_<records> points to (a copy)"""
        _check(self._fn("finish")(self.ctx.h, self.h, *finish_args))
        return _records(self._fn(records)(self.h), self._fn("size")(self.h), dtype)

    def counts(self):
        c = (c_i64 * 3)()
        self._fn("counts")(self.h, c)
        return tuple(c)

    def close(self):
        if self.h:
            self._fn("free")(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class _MergeTable(_Table):
    """A table on the device that the pages of one batch are merged into: prb_<PREFIX>_create and
    prb_search_page_<MERGE>."""
    MERGE = None

    def __init__(self, ctx, qb, *create_args):
        h = ctypes.c_void_p()
        _check(self._fn("create")(ctx.h, qb.h, *create_args, ctypes.byref(h)))
        self.h, self.ctx, self.qb = h, ctx, qb

    def merge(self, db, page, opts=None):
        """prb_search_page_<MERGE>: searches the batch against `page` and merges the result into the table"""
        o = opts or default_opts()
        _check(getattr(lib(), "prb_search_page_" + self.MERGE)(self.ctx.h, self.qb.h, db.h, page, ctypes.byref(o), self.h))

    def search(self, db, opts, pages):
        """every page (all of them, in this order, by default) merged, then finish() -> (what finish returns, counts)"""
        for p in range(db.npages) if pages is None else pages:
            self.merge(db, p, opts)
        return self.finish(), self.counts()


class TopSet(_MergeTable):
    """prb_topset: the N best pairs per query of one batch, in a table on the device that pages are merged into."""
    PREFIX, MERGE = "topset", "top"

    def __init__(self, ctx, qb, n):
        super().__init__(ctx, qb, n)

    def finish(self):
        """prb_topset_finish -> structured array TOP_DTYPE (a copy), by query, then rank"""
        return self._finish("pairs", TOP_DTYPE)


def search_top(ctx, qb, db, n, opts=None, pages=None, with_counts=False):
    """The n pairs of lowest e_min per query over the pages (all of them, in this order, by default) -> structured array
    TOP_DTYPE, by query, then rank.  with_counts: -> (records, (seed, ungapped, final) counts summed over the pages)."""
    with TopSet(ctx, qb, n) as ts:
        recs, counts = ts.search(db, opts, pages)
    return (recs, counts) if with_counts else recs


class TopHits(_MergeTable):
    """prb_tophits: the N best final hits per query of one batch, with their base pairs, in a table on the device that
    pages are merged into."""
    PREFIX, MERGE = "tophits", "tophits"

    def __init__(self, ctx, qb, n):
        super().__init__(ctx, qb, n)

    def finish(self):
        """prb_tophits_finish -> (structured array TOPHIT_DTYPE by query, then rank; int32 [npairs, 2] that the records'
        bp_offset / bp_count index), both copies"""
        recs = self._finish("hits", TOPHIT_DTYPE)
        cnt = c_i64()
        p = lib().prb_tophits_basepairs(self.h, ctypes.byref(cnt))
        return recs, _records(p, cnt.value * 2, np.dtype(np.int32)).reshape(-1, 2)


def search_tophits(ctx, qb, db, n, opts=None, pages=None, with_counts=False):
    """The n final hits of lowest e_tot per query over the pages (all of them, in this order, by default) ->
    (records TOPHIT_DTYPE by query, then rank; base pairs int32 [npairs, 2]).  with_counts: -> (records, base pairs,
    (seed, ungapped, final) counts summed over the pages)."""
    with TopHits(ctx, qb, n) as th:
        (recs, bp), counts = th.search(db, opts, pages)
    return (recs, bp, counts) if with_counts else (recs, bp)


class ProfSet(_MergeTable):
    """prb_profset: the per-position profile of one batch, in a table on the device that pages are merged into."""
    PREFIX, MERGE = "profset", "profile"

    def finish(self):
        """prb_profset_finish -> structured array PROFILE_DTYPE (a copy), by query, then position"""
        return self._finish("rows", PROFILE_DTYPE)


def search_profile(ctx, qb, db, opts=None, pages=None, with_counts=False):
    """The per-position profile over the pages (all of them, in this order, by default) -> structured array
    PROFILE_DTYPE, by query, then position.  with_counts: -> (rows, (seed, ungapped, final) counts summed over the pages)."""
    with ProfSet(ctx, qb) as ps:
        rows, counts = ps.search(db, opts, pages)
    return (rows, counts) if with_counts else rows


class _RunTable(_Table):
    """A table on the device, made for one database, that any number of batches is merged into, page by page; every
    batch names its queries by identifiers of the caller's: prb_<PREFIX>_create and prb_search_page_<MERGE>."""
    MERGE = None

    def __init__(self, ctx, db, *create_args):
        h = ctypes.c_void_p()
        _check(self._fn("create")(ctx.h, db.h, *create_args, ctypes.byref(h)))
        self.h, self.ctx, self.db = h, ctx, db

    def merge(self, qb, page, ids, opts=None, db=None):
        """prb_search_page_<MERGE>: searches the batch against `page` and merges the result into the table;
        ids[q] = the identifier of query q of the batch"""
        o = opts or default_opts()
        ids = np.ascontiguousarray(ids, np.int32)
        assert len(ids) == len(qb.lens)
        _check(getattr(lib(), "prb_search_page_" + self.MERGE)(self.ctx.h, qb.h, (db or self.db).h, page, ctypes.byref(o), ids.ctypes.data, self.h))


class TargetSet(_RunTable):
    """prb_targetset: the N best queries per target (page, db_id) of one database, in a table on the device that any
    number of batches is merged into, page by page; every batch names its queries by identifiers of the caller's."""
    PREFIX, MERGE = "targetset", "targets"

    def __init__(self, ctx, db, n):
        super().__init__(ctx, db, n)

    def finish(self):
        """prb_targetset_finish -> structured array TARGET_DTYPE (a copy), by page, then db_id, then rank"""
        return self._finish("pairs", TARGET_DTYPE)


def search_targets(ctx, db, n, batches, opts=None, pages=None, with_counts=False):
    """The n pairs of lowest e_min per target over batches = [(QBatch, ids)], every batch against the pages (all of them,
    in this order, by default) -> structured array TARGET_DTYPE, by page, db_id and rank.  with_counts: -> (records,
    (seed, ungapped, final) counts summed over the calls)."""
    with TargetSet(ctx, db, n) as ts:
        for qb, ids in batches:
            for p in range(db.npages) if pages is None else pages:
                ts.merge(qb, p, ids, opts)
        recs, counts = ts.finish(), ts.counts()
    return (recs, counts) if with_counts else recs


class CovSet(_RunTable):
    """prb_covset: the per-position coverage of every target (page, db_id) of one database, in a table on the device that
    any number of batches - or of hit lists - is merged into, page by page; every batch names its queries by identifiers
    of the caller's."""
    PREFIX, MERGE = "covset", "coverage"

    def __init__(self, ctx, db):
        super().__init__(ctx, db)

    def add_hits(self, page, ids, hits, bp):
        """prb_covset_add_hits: a list of final hits of `page` (HIT_DTYPE records ascending by `query`, with the int32 [n, 2]
        pairs their bp_offset / bp_count index) merged into the table; ids[q] = the identifier of the list's query q"""
        ids = np.ascontiguousarray(ids, np.int32)
        hits = np.ascontiguousarray(hits, HIT_DTYPE)
        bp = np.ascontiguousarray(bp, np.int32)
        _check(lib().prb_covset_add_hits(self.ctx.h, self.h, page, ids.ctypes.data if len(ids) else None, len(ids),
                                         hits.ctypes.data if len(hits) else None, len(hits), bp.ctypes.data if bp.size else None,
                                         bp.size // 2))

    def finish(self, d):
        """prb_covset_finish -> structured array REGION_DTYPE (a copy): the regions of depth d by page, db_id and start"""
        return self._finish("regions", REGION_DTYPE, d)


def search_coverage(ctx, db, d, batches, opts=None, pages=None, with_counts=False):
    """The regions of every target that at least d queries bind, over batches = [(QBatch, ids)], every batch against the
    pages (all of them, in this order, by default) -> structured array REGION_DTYPE, by page, db_id and start.
    with_counts: -> (records, (seed, ungapped, final) counts summed over the calls)."""
    with CovSet(ctx, db) as cs:
        for qb, ids in batches:
            for p in range(db.npages) if pages is None else pages:
                cs.merge(qb, p, ids, opts)
        recs, counts = cs.finish(d), cs.counts()
    return (recs, counts) if with_counts else recs


class NullSet(_Table):
    """prb_nullset: per observed (query, target) pair of one batch, how the query's decoys fare against the target, in a
    table on the device: the real batch is observed page by page, then its decoys are merged batch by batch.  Close it
    before its context."""
    PREFIX = "nullset"

    def __init__(self, ctx, qb, db, ndecoys):
        h = ctypes.c_void_p()
        _check(lib().prb_nullset_create(ctx.h, qb.h, db.h, ndecoys, ctypes.byref(h)))
        self.h, self.ctx, self.qb, self.db = h, ctx, qb, db

    def observed(self, page, opts=None):
        """prb_search_page_observed: the real batch against `page`"""
        o = opts or default_opts()
        _check(lib().prb_search_page_observed(self.ctx.h, self.qb.h, self.db.h, page, ctypes.byref(o), self.h))

    def decoys(self, dqb, page, owner, decoy, opts=None):
        """prb_search_page_decoys: the batch dqb of decoys against `page`; owner[q] / decoy[q] = the real query and the decoy
        number of its query q"""
        o = opts or default_opts()
        owner, decoy = np.ascontiguousarray(owner, np.int32), np.ascontiguousarray(decoy, np.int32)
        assert len(owner) == len(decoy) == len(dqb.lens)
        _check(lib().prb_search_page_decoys(self.ctx.h, dqb.h, self.db.h, page, ctypes.byref(o), owner.ctypes.data, decoy.ctypes.data,
                                            self.h))

    def observe(self, page, pairs):
        """prb_nullset_observe: a caller's PAIR_DTYPE records of the real batch against `page`"""
        pairs = np.ascontiguousarray(pairs, PAIR_DTYPE)
        _check(lib().prb_nullset_observe(self.ctx.h, self.h, page, pairs.ctypes.data if len(pairs) else None, len(pairs)))

    def add_pairs(self, page, owner, decoy, pairs):
        """prb_nullset_add_pairs: a caller's PAIR_DTYPE records of a batch of decoys against `page`; their `query` indexes
        owner / decoy"""
        owner, decoy = np.ascontiguousarray(owner, np.int32), np.ascontiguousarray(decoy, np.int32)
        assert len(owner) == len(decoy)
        pairs = np.ascontiguousarray(pairs, PAIR_DTYPE)
        _check(lib().prb_nullset_add_pairs(self.ctx.h, self.h, page, owner.ctypes.data if len(owner) else None,
                                           decoy.ctypes.data if len(owner) else None, len(owner),
                                           pairs.ctypes.data if len(pairs) else None, len(pairs)))

    def retire(self, min_le, upto):
        """prb_nullset_retire: the live pairs with null_le >= min_le retire with decoys = upto -> the live pairs left per
        query (int64 array)"""
        left = np.zeros(len(self.qb.lens), np.int64)
        _check(lib().prb_nullset_retire(self.ctx.h, self.h, min_le, upto, left.ctypes.data if len(left) else None))
        return left

    def finish(self):
        """prb_nullset_finish -> structured array NULL_DTYPE (a copy), by query, then page, then db_id"""
        return self._finish("pairs", NULL_DTYPE)

    def finish_fdr(self, tests=None):
        """prb_nullset_finish_fdr -> (NULL_DTYPE records as finish() returns them, FDR_DTYPE figures parallel to them); tests =
        the hypotheses per query (None: every target of the database)"""
        t = None if tests is None else np.ascontiguousarray(tests, np.int64)
        assert t is None or len(t) == len(self.qb.lens)
        _check(lib().prb_nullset_finish_fdr(self.ctx.h, self.h, None if t is None or not len(t) else t.ctypes.data))
        n = lib().prb_nullset_size(self.h)
        figs = lib().prb_nullset_fdr(self.h)  # (NULL: the table was finished without them)
        return _records(lib().prb_nullset_pairs(self.h), n, NULL_DTYPE), _records(figs, n if figs else 0, FDR_DTYPE)

    def decoy_counts(self):
        c = (c_i64 * 3)()
        lib().prb_nullset_decoy_counts(self.h, c)
        return tuple(c)


class GroupSet(_Table):
    """prb_groupset: per (query, group of database sequences) of one batch, the group's best member pair and the integer
    sums over its members, in a dense table on the device that pages are folded into.  group_of_page[p][db_id] = the group
    of sequence db_id of page p, in [0, ngroups).  Close it before its context."""
    PREFIX = "groupset"

    def __init__(self, ctx, qb, db, group_of_page, ngroups):
        maps = [np.ascontiguousarray(m, np.int32) for m in group_of_page]
        ptrs = (ctypes.c_void_p * max(len(maps), 1))(*[m.ctypes.data if len(m) else None for m in maps])
        h = ctypes.c_void_p()
        _check(lib().prb_groupset_create(ctx.h, qb.h, db.h, ptrs, ngroups, ctypes.byref(h)))
        self.h, self.ctx, self.qb, self.db = h, ctx, qb, db

    def merge(self, page, opts=None):
        """prb_search_page_groups: searches the batch against `page` and folds the pairs' records into the table"""
        o = opts or default_opts()
        _check(lib().prb_search_page_groups(self.ctx.h, self.qb.h, self.db.h, page, ctypes.byref(o), self.h))

    def add_pairs(self, page, pairs):
        """prb_groupset_add_pairs: a caller's PAIR_DTYPE records of the batch against `page`"""
        pairs = np.ascontiguousarray(pairs, PAIR_DTYPE)
        _check(lib().prb_groupset_add_pairs(self.ctx.h, self.h, page, pairs.ctypes.data if len(pairs) else None, len(pairs)))

    def finish(self, n=0):
        """prb_groupset_finish -> structured array GROUP_DTYPE (a copy): by query, then group (n = 0), or each query's n
        best groups by query, then rank"""
        return self._finish("pairs", GROUP_DTYPE, n)


def search_groups(ctx, qb, db, group_of_page, ngroups, n=0, opts=None, pages=None, with_counts=False):
    """The group table of the batch over the pages (all of them, in this order, by default) -> structured array
    GROUP_DTYPE.  with_counts: -> (records, (seed, ungapped, final) counts summed over the pages)."""
    with GroupSet(ctx, qb, db, group_of_page, ngroups) as gs:
        for p in range(db.npages) if pages is None else pages:
            gs.merge(p, opts)
        recs, counts = gs.finish(n), gs.counts()
    return (recs, counts) if with_counts else recs


class Annotation:
    """prb_annot: the annotated features of one database on the device.  features = [(page, db_id, start, end)], start <= end
    inclusive, in the target's forward coordinates (what the result lines print).  Close it after every FeatSet made with
    it, and before its database."""

    def __init__(self, ctx, db, features):
        f = np.ascontiguousarray(np.asarray(features, np.int32).reshape(-1, 4).T)
        h = ctypes.c_void_p()
        n = f.shape[1]
        _check(lib().prb_annot_create(ctx.h, db.h, n, *[f[k].ctypes.data if n else None for k in range(4)], ctypes.byref(h)))
        self.h, self.ctx, self.db = h, ctx, db

    def count(self):
        return lib().prb_annot_count(self.h)

    def close(self):
        if self.h:
            lib().prb_annot_free(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


class FeatSet(_Table):
    """prb_featset: per (query, annotated feature of a target) of one batch, the `-t` summary over the final hits whose span
    meets the feature, in a table on the device that pages are folded into.  Close it before its annotation."""
    PREFIX = "featset"

    def __init__(self, ctx, qb, annot):
        h = ctypes.c_void_p()
        _check(lib().prb_featset_create(ctx.h, qb.h, annot.h, ctypes.byref(h)))
        self.h, self.ctx, self.qb, self.annot = h, ctx, qb, annot

    def merge(self, db, page, opts=None, qb=None):
        """prb_search_page_features: searches the batch against `page` and folds its final hits into the table"""
        o = opts or default_opts()
        _check(lib().prb_search_page_features(self.ctx.h, (qb or self.qb).h, db.h, page, ctypes.byref(o), self.h))

    def add_hits(self, page, hits, bp):
        """prb_featset_add_hits: a list of final hits of `page` (HIT_DTYPE records ascending by `query`, with the int32 [n, 2]
        pairs their bp_offset / bp_count index) folded into the table"""
        hits = np.ascontiguousarray(hits, HIT_DTYPE)
        bp = np.ascontiguousarray(bp, np.int32)
        _check(lib().prb_featset_add_hits(self.ctx.h, self.h, page, hits.ctypes.data if len(hits) else None, len(hits),
                                          bp.ctypes.data if bp.size else None, bp.size // 2))

    def finish(self):
        """prb_featset_finish -> structured array FEATURE_DTYPE (a copy): by query, page, target and feature"""
        return self._finish("records", FEATURE_DTYPE)

    def finish_top(self, n):
        """prb_featset_finish_top -> structured array FEATURE_DTYPE (a copy): each query's n best records, ranked on the
        device by (e_min, place in the order of finish()); by query, then rank"""
        _check(lib().prb_featset_finish_top(self.ctx.h, self.h, n))
        return feature_records(self)

    def unassigned(self):
        return lib().prb_featset_unassigned(self.h)


def search_features(ctx, qb, db, annot, opts=None, pages=None, with_counts=False):
    """The feature table of the batch over the pages (all of them, in this order, by default) -> (structured array
    FEATURE_DTYPE, unassigned hits).  with_counts: -> (records, unassigned, (seed, ungapped, final) counts)."""
    with FeatSet(ctx, qb, annot) as fs:
        for p in range(db.npages) if pages is None else pages:
            fs.merge(db, p, opts)
        recs, un, counts = fs.finish(), fs.unassigned(), fs.counts()
    return (recs, un, counts) if with_counts else (recs, un)


class _RankTable(_Table):
    """A ranking table of a run on the device: records of DTYPE, which prb_<PREFIX>_<RECORDS> points to once it is finished."""
    DTYPE = RECORDS = None

    def add_records(self, recs):
        """prb_<PREFIX>_add_records: a caller's DTYPE records whose `query` is the identifier already"""
        recs = np.ascontiguousarray(recs, self.DTYPE)
        _check(self._fn("add_records")(self.ctx.h, self.h, recs.ctypes.data if len(recs) else None, len(recs)))

    def merge(self, other):
        """prb_<PREFIX>_merge: the unfinished table `other` (over other identifiers; of any context) merged into this
        one on the device; `other` is left empty"""
        self.absorb(other)

    def finish(self):
        """prb_<PREFIX>_finish -> structured array DTYPE (a copy), by list - group, feature -, then rank"""
        return self._finish(self.RECORDS, self.DTYPE)


class GroupRank(_RankTable):
    """prb_grouprank: the N best queries per group of database sequences, in a table on the device that any number of
    batches is merged into - each as its complete, unfinished GroupSet, or as GROUP_DTYPE records -; every batch names its
    queries by identifiers of the caller's.  Close it before its context."""
    PREFIX, DTYPE, RECORDS = "grouprank", GROUP_DTYPE, "pairs"

    def __init__(self, ctx, ngroups, n):
        h = ctypes.c_void_p()
        _check(lib().prb_grouprank_create(ctx.h, ngroups, n, ctypes.byref(h)))
        self.h, self.ctx = h, ctx

    def add_groupset(self, gs, ids):
        """prb_grouprank_add_groupset: every occupied slot of the unfinished GroupSet `gs` (every page merged), on the
        device; ids[q] = the identifier of query q of its batch.  gs is left as it was"""
        ids = np.ascontiguousarray(ids, np.int32)
        assert len(ids) == len(gs.qb.lens)
        _check(lib().prb_grouprank_add_groupset(self.ctx.h, self.h, gs.h, ids.ctypes.data))


def search_grouprank(ctx, db, group_of_page, ngroups, n, batches, opts=None, pages=None, with_counts=False):
    """The n (query, group) records of lowest e_min per group over batches = [(QBatch, ids)], every batch against every
    page (in this order, if given) into a group table of its own, which is merged into the ranking on the device and
    dropped -> structured array GROUP_DTYPE, by group and rank.  with_counts: -> (records, (seed, ungapped, final) counts
    summed over the batches)."""
    with GroupRank(ctx, ngroups, n) as gr:
        for qb, ids in batches:
            with GroupSet(ctx, qb, db, group_of_page, ngroups) as gs:
                for p in range(db.npages) if pages is None else pages:
                    gs.merge(p, opts)
                gr.add_groupset(gs, ids)
        recs, counts = gr.finish(), gr.counts()
    return (recs, counts) if with_counts else recs


class FeatRank(_RankTable):
    """prb_featrank: the N best queries per feature of an Annotation, in a table on the device that any number of batches
    is merged into - each as its complete, unfinished FeatSet, or as FEATRANK_DTYPE records -; every batch names its queries
    by identifiers of the caller's.  Close it before its annotation and its context."""
    PREFIX, DTYPE, RECORDS = "featrank", FEATRANK_DTYPE, "records"

    def __init__(self, ctx, annot, n):
        h = ctypes.c_void_p()
        _check(lib().prb_featrank_create(ctx.h, annot.h, n, ctypes.byref(h)))
        self.h, self.ctx, self.annot = h, ctx, annot

    def add_featset(self, fs, ids):
        """prb_featrank_add_featset: every record of the unfinished FeatSet `fs` (every page merged), on the device;
        ids[q] = the identifier of query q of its batch.  fs is left as it was"""
        ids = np.ascontiguousarray(ids, np.int32)
        assert len(ids) == len(fs.qb.lens)
        _check(lib().prb_featrank_add_featset(self.ctx.h, self.h, fs.h, ids.ctypes.data))

    def unassigned(self):
        return lib().prb_featrank_unassigned(self.h)


def search_featrank(ctx, db, annot, n, batches, opts=None, pages=None, with_counts=False):
    """The n (query, feature) records of lowest e_min per feature over batches = [(QBatch, ids)], every batch against
    every page (in this order, if given) into a feature table of its own, which is merged into the ranking on the device
    and dropped -> (structured array FEATRANK_DTYPE, by feature and rank; unassigned hits).  with_counts: -> (records,
    unassigned, (seed, ungapped, final) counts summed over the batches)."""
    with FeatRank(ctx, annot, n) as fr:
        for qb, ids in batches:
            with FeatSet(ctx, qb, annot) as fs:
                for p in range(db.npages) if pages is None else pages:
                    fs.merge(db, p, opts)
                fr.add_featset(fs, ids)
        recs, un, counts = fr.finish(), fr.unassigned(), fr.counts()
    return (recs, un, counts) if with_counts else (recs, un)


class GNullSet(_Table):
    """prb_gnullset: per kept (query, group) record of a group table, how the query's decoys fare against the group's
    members.  Made from a GroupSet with every page merged, which it finishes (gs.records() are then its records); the decoys
    come in batches between begin() and end().  Close it before its context."""
    PREFIX = "gnullset"

    def __init__(self, ctx, gs, n, ndecoys):
        h = ctypes.c_void_p()
        _check(lib().prb_gnullset_create(ctx.h, gs.h, n, ndecoys, ctypes.byref(h)))
        self.h, self.ctx, self.db = h, ctx, gs.db

    def begin(self, owner, decoy):
        """prb_gnullset_begin: opens the batch of the decoys decoy[k] of the real queries owner[k]"""
        owner, decoy = np.ascontiguousarray(owner, np.int32), np.ascontiguousarray(decoy, np.int32)
        assert len(owner) == len(decoy)
        _check(lib().prb_gnullset_begin(self.ctx.h, self.h, owner.ctypes.data if len(owner) else None,
                                        decoy.ctypes.data if len(owner) else None, len(owner)))

    def merge(self, dqb, page, opts=None):
        """prb_search_page_gnull: the open batch's decoys dqb against `page`"""
        o = opts or default_opts()
        _check(lib().prb_search_page_gnull(self.ctx.h, dqb.h, self.db.h, page, ctypes.byref(o), self.h))

    def add_pairs(self, page, pairs):
        """prb_gnullset_add_pairs: a caller's PAIR_DTYPE records of the open batch against `page`; their `query` indexes
        the batch"""
        pairs = np.ascontiguousarray(pairs, PAIR_DTYPE)
        _check(lib().prb_gnullset_add_pairs(self.ctx.h, self.h, page, pairs.ctypes.data if len(pairs) else None, len(pairs)))

    def end(self):
        """prb_gnullset_end: the open batch counted and closed"""
        _check(lib().prb_gnullset_end(self.ctx.h, self.h))

    def finish(self):
        """prb_gnullset_finish -> structured array GNULL_DTYPE (a copy), in the group table's order"""
        return self._finish("pairs", GNULL_DTYPE)

    def counts(self):
        """the stage counts of the decoy searches"""
        c = (c_i64 * 3)()
        lib().prb_gnullset_decoy_counts(self.h, c)
        return tuple(c)


class FNullSet(_Table):
    """prb_fnullset: per kept (query, feature) record of a feature table, how the query's decoys fare against the feature.
    Made from a FeatSet with every page merged, which it finishes (feature_records(fs) are then its records); the decoys come
    in batches between begin() and end().  top: over each query's `top` best records only, as FeatSet.finish_top(top) ranks
    them (prb_fnullset_create_top).  Close it before its annotation."""
    PREFIX = "fnullset"

    def __init__(self, ctx, fs, ndecoys, top=None):
        h = ctypes.c_void_p()
        if top is None:
            _check(lib().prb_fnullset_create(ctx.h, fs.h, ndecoys, ctypes.byref(h)))
        else:
            _check(lib().prb_fnullset_create_top(ctx.h, fs.h, ndecoys, top, ctypes.byref(h)))
        self.h, self.ctx, self.db = h, ctx, fs.annot.db

    def begin(self, owner, decoy):
        """prb_fnullset_begin: opens the batch of the decoys decoy[k] of the real queries owner[k]"""
        owner, decoy = np.ascontiguousarray(owner, np.int32), np.ascontiguousarray(decoy, np.int32)
        assert len(owner) == len(decoy)
        _check(lib().prb_fnullset_begin(self.ctx.h, self.h, owner.ctypes.data if len(owner) else None,
                                        decoy.ctypes.data if len(owner) else None, len(owner)))

    def merge(self, dqb, page, opts=None):
        """prb_search_page_fnull: the open batch's decoys dqb against `page`"""
        o = opts or default_opts()
        _check(lib().prb_search_page_fnull(self.ctx.h, dqb.h, self.db.h, page, ctypes.byref(o), self.h))

    def add_hits(self, page, hits, bp):
        """prb_fnullset_add_hits: a list of final hits of the open batch's decoys against `page` (HIT_DTYPE records ascending
        by `query`, their place in the batch, with the int32 [n, 2] pairs their bp_offset / bp_count index)"""
        hits = np.ascontiguousarray(hits, HIT_DTYPE)
        bp = np.ascontiguousarray(bp, np.int32)
        _check(lib().prb_fnullset_add_hits(self.ctx.h, self.h, page, hits.ctypes.data if len(hits) else None, len(hits),
                                           bp.ctypes.data if bp.size else None, bp.size // 2))

    def end(self):
        """prb_fnullset_end: the open batch counted and closed"""
        _check(lib().prb_fnullset_end(self.ctx.h, self.h))

    def finish(self):
        """prb_fnullset_finish -> structured array FNULL_DTYPE (a copy), in the feature table's order"""
        return self._finish("records", FNULL_DTYPE)

    def counts(self):
        """the stage counts of the decoy searches"""
        c = (c_i64 * 3)()
        lib().prb_fnullset_decoy_counts(self.h, c)
        return tuple(c)


def feature_records(fs):
    """prb_featset_records of a finished feature table (an FNullSet finishes the one it is made from) -> FEATURE_DTYPE (a copy)"""
    return _records(lib().prb_featset_records(fs.h), lib().prb_featset_size(fs.h), FEATURE_DTYPE)


def search_fnull(ctx, qb, seqs, db, annot, ndecoys, seed=1, file_pos0=0, opts=None, mask=True, decoy_batch=None, pages=None, top=None, with_counts=False):
    """The feature null table of the batch qb (of the sequences seqs, the first of which stands at place file_pos0 of its
    file) against db under the annotation -> structured array FNULL_DTYPE, in the order of FeatSet.finish().  mask: every
    decoy batch is searched under a pair mask that allows each decoy the targets of its owner's kept records only (the same
    records either way).  decoy_batch: decoys per batch (all at once by default); pages: their order.  top: over each
    query's `top` best records only, in the order of FeatSet.finish_top(top).  with_counts: -> (records, the (seed, ungapped,
    final) counts of the decoy searches)."""
    o = opts or default_opts()
    pages = list(range(db.npages)) if pages is None else list(pages)
    with FeatSet(ctx, qb, annot) as fs:
        for p in pages:
            fs.merge(db, p, o)
        with FNullSet(ctx, fs, ndecoys, top) as fn:
            kept = feature_records(fs)

            def targets(q):
                mine = kept[kept["query"] == q]
                return mine["page"].astype(np.int32), mine["db_id"].astype(np.int32)

            with contextlib.closing(_decoy_batches(ctx, seqs, db, ndecoys, seed, file_pos0, o, decoy_batch, targets if mask else None)) as batches:
                for dqb, own, dec, od in batches:
                    fn.begin(own, dec)
                    for p in pages:
                        fn.merge(dqb, p, od)
                    fn.end()
            recs = fn.finish()
            return (recs, fn.counts()) if with_counts else recs


class EvalSet(_Table):
    """prb_evalset: the energy keys of one batch's final hits and of its decoys', pooled per query over the whole database,
    and per real hit its rank, the decoy hits at or below it and the pair of its FDR q-value.  The real batch is searched
    page by page (with a TopHits table beside it, if wanted), then its decoys batch by batch; close(); then score().  Close
    it before its context."""
    PREFIX = "evalset"

    def __init__(self, ctx, qb, db, ndecoys):
        h = ctypes.c_void_p()
        _check(lib().prb_evalset_create(ctx.h, qb.h, db.h, ndecoys, ctypes.byref(h)))
        self.h, self.ctx, self.qb, self.db = h, ctx, qb, db

    def scored(self, page, opts=None, tophits=None):
        """prb_search_page_scored: the real batch against `page`, once; tophits: a TopHits table that takes the same hits"""
        o = opts or default_opts()
        _check(lib().prb_search_page_scored(self.ctx.h, self.qb.h, self.db.h, page, ctypes.byref(o), tophits.h if tophits else None, self.h))

    def null_hits(self, dqb, page, owner, decoy, opts=None):
        """prb_search_page_null_hits: the batch dqb of decoys against `page`; owner[q] / decoy[q] = the real query and the
        decoy number of its query q"""
        o = opts or default_opts()
        owner, decoy = np.ascontiguousarray(owner, np.int32), np.ascontiguousarray(decoy, np.int32)
        assert len(owner) == len(decoy) == len(dqb.lens)
        _check(lib().prb_search_page_null_hits(self.ctx.h, dqb.h, self.db.h, page, ctypes.byref(o), owner.ctypes.data, decoy.ctypes.data,
                                               self.h))

    def add_keys(self, is_decoy, query_or_owner, energy):
        """prb_evalset_add_keys: a caller's energies under their queries (real list) or owners (decoy list)"""
        ids, energy = np.ascontiguousarray(query_or_owner, np.int32), np.ascontiguousarray(energy, np.float64)
        assert len(ids) == len(energy)
        _check(lib().prb_evalset_add_keys(self.ctx.h, self.h, int(bool(is_decoy)), ids.ctypes.data if len(ids) else None,
                                          energy.ctypes.data if len(ids) else None, len(ids)))

    def finish(self):
        """prb_evalset_close: the lists sorted, every real hit's figures computed; nothing is merged after it"""
        _check(lib().prb_evalset_close(self.ctx.h, self.h))

    def score(self, query, energy):
        """prb_evalset_score -> structured array EVAL_DTYPE, one record per (query[i], energy[i])"""
        query, energy = np.ascontiguousarray(query, np.int32), np.ascontiguousarray(energy, np.float64)
        assert len(query) == len(energy)
        out = np.zeros(len(query), EVAL_DTYPE)
        _check(lib().prb_evalset_score(self.ctx.h, self.h, query.ctypes.data if len(query) else None, energy.ctypes.data if len(query) else None,
                                       len(query), out.ctypes.data if len(query) else None))
        return out

    def sizes(self):
        a, b = c_i64(), c_i64()
        lib().prb_evalset_sizes(self.h, ctypes.byref(a), ctypes.byref(b))
        return a.value, b.value

    def decoy_counts(self):
        c = (c_i64 * 3)()
        lib().prb_evalset_decoy_counts(self.h, c)
        return tuple(c)


def group_records(gs):
    """prb_groupset_pairs of a finished group table (a GNullSet finishes the one it is made from) -> GROUP_DTYPE (a copy)"""
    return _records(lib().prb_groupset_pairs(gs.h), lib().prb_groupset_size(gs.h), GROUP_DTYPE)


def search_gnull(ctx, qb, seqs, db, group_of_page, ngroups, ndecoys, n=0, seed=1, file_pos0=0, opts=None, mask=True, decoy_batch=None,
                 pages=None):
    """The group null table of the batch qb (of the sequences seqs, the first of which stands at place file_pos0 of its
    file) against db -> structured array GNULL_DTYPE, in the order of GroupSet.finish(n).  mask: every decoy batch is
    searched under a pair mask that allows each decoy the members of its owner's kept groups only (the same records either
    way).  decoy_batch: decoys per batch (all at once by default); pages: their order."""
    o = opts or default_opts()
    pages = list(range(db.npages)) if pages is None else list(pages)
    with GroupSet(ctx, qb, db, group_of_page, ngroups) as gs:
        for p in pages:
            gs.merge(p, o)
        with GNullSet(ctx, gs, n, ndecoys) as gn:
            kept = group_records(gs)
            members = {}  # group -> [(page, db_id)]
            for p, m in enumerate(group_of_page):
                for i, g in enumerate(m):
                    members.setdefault(int(g), []).append((p, i))

            def targets(q):
                tgt = [t for g in kept["group"][kept["query"] == q] for t in members[int(g)]]
                return np.array([t[0] for t in tgt], np.int32), np.array([t[1] for t in tgt], np.int32)

            with contextlib.closing(_decoy_batches(ctx, seqs, db, ndecoys, seed, file_pos0, o, decoy_batch, targets if mask else None)) as batches:
                for dqb, own, dec, od in batches:
                    gn.begin(own, dec)
                    for p in pages:
                        gn.merge(dqb, p, od)
                    gn.end()
            return gn.finish()


def null_decoys(seqs, ndecoys, seed=1, file_pos0=0):
    """the decoys of a batch as search_null searches them -> (sequences, owner, decoy), query by query, decoy by decoy"""
    dseqs, owner, decoy = [], [], []
    for q, s in enumerate(seqs):
        for d in range(ndecoys):
            dseqs.append(shuffle_sequence(s, seed, file_pos0 + q, d))
            owner.append(q)
            decoy.append(d)
    return dseqs, np.array(owner, np.int32), np.array(decoy, np.int32)


def _decoy_batches(ctx, seqs, db, ndecoys, seed, file_pos0, opts, decoy_batch, targets):
    """The decoys of a batch in batches of decoy_batch (all at once by default): for each, yields the decoy QBatch with its
    accessibilities computed, its owner and decoy slices, and the options for its searches - opts without the caller's
    mask, which is for the real batch, and, with targets(q) -> (pages, db_ids), under a PairMask that allows every decoy
    of query q those targets.  What was made for a batch is closed when the caller comes back for the next one, or closes
    the generator."""
    dseqs, owner, decoy = null_decoys(seqs, ndecoys, seed, file_pos0)
    step = decoy_batch or len(dseqs)
    for i0 in range(0, len(dseqs), step):
        own, dec = owner[i0:i0 + step], decoy[i0:i0 + step]
        dqb = QBatch(ctx, dseqs[i0:i0 + step], db.repeat_flag)
        pm = None
        try:
            dqb.accessibility(db.W, db.delta)
            od = RisOpts.from_buffer_copy(opts)
            od.allowed_pairs = None
            if targets is not None:
                pm = PairMask(ctx, dqb, db)
                for k in range(len(own)):
                    tp, td = targets(own[k])
                    if len(td):
                        pm.allow(np.full(len(td), k, np.int32), tp, td)
                od.allowed_pairs = pm.h.value
            yield dqb, own, dec, od
        finally:
            if pm is not None:
                pm.close()
            dqb.close()


def search_null(ctx, qb, seqs, db, ndecoys, seed=1, file_pos0=0, opts=None, mask=True, decoy_batch=None, pages=None,
                with_counts=False, fdr=False):
    """The null table of the batch qb (of the sequences seqs, the first of which stands at place file_pos0 of its file)
    against db with ndecoys decoys per query -> structured array NULL_DTYPE, by query, then page, then db_id.  mask: every
    decoy batch is searched under a pair mask that allows its owners' observed targets only (the same records either way).
    decoy_batch: decoys per batch (all at once by default); pages: their order.  with_counts: -> (records, counts of the
    real batch's searches, counts of the decoys').  fdr: the records are (records, FDR_DTYPE figures), finished with the
    q-values over every target of the database (NullSet.finish_fdr)."""
    o = opts or default_opts()
    pages = list(range(db.npages)) if pages is None else list(pages)
    with NullSet(ctx, qb, db, ndecoys) as ns:
        observed, counts = [], np.zeros(3, np.int64)
        for p in pages:
            if mask:  # (as the command line: the mask needs the observed triples on the host, the table takes them from there)
                recs, c = search_page_summary(ctx, qb, db, p, o, with_counts=True)
                observed.append((recs["query"].copy(), np.full(len(recs), p, np.int32), recs["db_id"].copy()))
                counts += np.array(c, np.int64)
                ns.observe(p, recs)
            else:
                ns.observed(p, o)

        obs_q, obs_p, obs_d = (np.concatenate([np.zeros(0, np.int32)] + [x[i] for x in observed]) for i in range(3))

        def targets(q):  # (what the real batch's mask allows is all that is observed)
            return obs_p[obs_q == q], obs_d[obs_q == q]

        with contextlib.closing(_decoy_batches(ctx, seqs, db, ndecoys, seed, file_pos0, o, decoy_batch, targets if mask else None)) as batches:
            for dqb, own, dec, od in batches:
                for p in pages:
                    ns.decoys(dqb, p, own, dec, od)
        recs = ns.finish_fdr() if fdr else ns.finish()
        counts = tuple(int(x) for x in counts) if mask else ns.counts()
        dcounts = ns.decoy_counts()
    return (recs, counts, dcounts) if with_counts else recs


def search_seqnull(ctx, qb, seqs, db, ndecoys, min_le, per_round, seed=1, file_pos0=0, opts=None, mask=True, decoy_batch=None,
                   with_counts=False):
    """The null table of search_null with sequential p-values (`ris -t -z ndecoys -H min_le -D per_round`): the decoys in
    rounds of per_round, each round for the queries that still have live pairs and - with mask - under the mask of the live
    pairs made on the device; at every round's end the pairs with null_le >= min_le retire.  -> NULL_DTYPE records, whose
    `decoys` is per pair.  with_counts: -> (records, counts of the real batch, counts of the decoys, [(boundary, live pairs
    per query)])."""
    o = opts or default_opts()
    rounds = []
    with NullSet(ctx, qb, db, ndecoys) as ns:
        for p in range(db.npages):
            ns.observed(p, o)
        od = RisOpts.from_buffer_copy(o)
        queries = list(range(len(seqs)))
        for lo in range(0, ndecoys, per_round):
            if not queries:
                break
            hi = min(ndecoys, lo + per_round)
            todo = [(q, d) for q in queries for d in range(lo, hi)]
            step = decoy_batch or len(todo)
            for i0 in range(0, len(todo), step):
                part = todo[i0:i0 + step]
                own, dec = np.array([q for q, _ in part], np.int32), np.array([d for _, d in part], np.int32)
                dqb = QBatch(ctx, [shuffle_sequence(seqs[q], seed, file_pos0 + q, d) for q, d in part], db.repeat_flag)
                pm = None
                try:
                    dqb.accessibility(db.W, db.delta)
                    od.allowed_pairs = None
                    if mask:
                        pm = PairMask.live(ctx, ns, dqb, own)
                        od.allowed_pairs = pm.h.value
                    for p in range(db.npages):
                        ns.decoys(dqb, p, own, dec, od)
                finally:
                    if pm is not None:
                        pm.close()
                    dqb.close()
            left = ns.retire(min_le, hi)
            rounds.append((hi, left))
            queries = [q for q in queries if left[q] > 0]
        recs = ns.finish()
        counts, dcounts = ns.counts(), ns.decoy_counts()
    return (recs, counts, dcounts, rounds) if with_counts else recs


class Comm:
    """prb_comm: the RCCL communicator of the final hit gather (one process per GPU)."""

    ID_BYTES = 128

    @staticmethod
    def unique_id():
        buf = ctypes.create_string_buffer(Comm.ID_BYTES)
        _check(lib().prb_comm_unique_id(buf))
        return buf.raw

    def __init__(self, ctx, nranks, rank, uid):
        h = ctypes.c_void_p()
        _check(lib().prb_comm_create(ctx.h, nranks, rank, uid, ctypes.byref(h)))
        self.h, self.nranks, self.rank = h, nranks, rank

    def close(self):
        if self.h:
            lib().prb_comm_destroy(self.h)
            self.h = None

    def gather(self, hitset, qlen_unmasked, root=0):
        """collective; on root -> (HitSet of all ranks, nq per rank, unmasked lengths of all queries), else None"""
        ql = np.ascontiguousarray(qlen_unmasked, np.int32)
        out = ctypes.c_void_p()
        _check(lib().prb_gather_hits(self.h, hitset.h if hitset is not None else None, len(ql), ql.ctypes.data if len(ql) else None,
                                     root, ctypes.byref(out)))
        if self.rank != root:
            return None
        n, pn, pq = c_i32(), P(c_i32)(), P(c_i32)()
        _check(lib().prb_hitset_gathered_queries(out, ctypes.byref(n), ctypes.byref(pn), ctypes.byref(pq)))
        nq_of = np.ctypeslib.as_array(pn, (n.value,)).copy()
        total = int(nq_of.sum())
        qall = np.ctypeslib.as_array(pq, (total,)).copy() if total else np.zeros(0, np.int32)
        g = HitSet(out)
        g._owner.comm = self  # (not needed by the library - the pinned buffer is shared with the hit set - but it keeps the
        return g, nq_of, qall  #  order of destruction the plain one: hit sets first)


def _write(fn, db, qnames, qlen_unmasked, *args):
    """One of the prb_write_*lines: the queries' names and lengths marshalled, `args` between them and the output
    counters -> (lines, bytes)"""
    names = (ctypes.c_char_p * len(qnames))(*[n.encode() for n in qnames])
    ql = np.ascontiguousarray(qlen_unmasked, np.int32)
    lines, nbytes = c_i64(), c_i64()
    _check(fn(db.h, len(qnames), names, ql.ctypes.data, *args, ctypes.byref(lines), ctypes.byref(nbytes)))
    return lines.value, nbytes.value


def write_lines(db, qnames, qlen_unmasked, pages, output_style=0, id0=0, fd=-1):
    """Result lines (SaveMyResults) of one batch: pages = [(hits, bp)] per database page as search_page returns
    them.  -> (lines, bytes) written to the descriptor fd (-1: formatted and counted only)."""
    arr = (PageHits * len(pages))()
    keep = []
    for k, (hits, bp) in enumerate(pages):
        hits = np.ascontiguousarray(hits)
        bp = np.ascontiguousarray(bp, np.int32)
        keep += [hits, bp]
        arr[k] = PageHits(hits.ctypes.data if len(hits) else None, len(hits), bp.ctypes.data if bp.size else None, bp.size // 2)
    return _write(lib().prb_write_lines, db, qnames, qlen_unmasked, arr, len(pages), output_style, id0, fd)


def write_summary_lines(db, qnames, qlen_unmasked, pages, id0=0, fd=-1):
    """Summary lines (`ris -t`) of one batch: pages = [records] per database page as search_page_summary returns
    them.  -> (lines, bytes) written to the descriptor fd (-1: formatted and counted only)."""
    arr = (PagePairs * len(pages))()
    keep = []
    for k, recs in enumerate(pages):
        recs = np.ascontiguousarray(recs, PAIR_DTYPE)
        keep.append(recs)
        arr[k] = PagePairs(recs.ctypes.data if len(recs) else None, len(recs))
    return _write(lib().prb_write_summary_lines, db, qnames, qlen_unmasked, arr, len(pages), id0, fd)


def write_top_lines(db, qnames, qlen_unmasked, recs, id0=0, fd=-1):
    """Lines of `ris -t -n N` for one batch: recs as search_top returns them.  -> (lines, bytes) written to fd
    (-1: formatted and counted only)."""
    recs = np.ascontiguousarray(recs, TOP_DTYPE)
    return _write(lib().prb_write_top_lines, db, qnames, qlen_unmasked, recs.ctypes.data if len(recs) else None, len(recs), id0, fd)


def write_null_lines(db, qnames, qlen_unmasked, recs, id0=0, fd=-1):
    """Lines of `ris -t -z N` for one batch: recs as search_null returns them.  -> (lines, bytes) written to fd
    (-1: formatted and counted only)."""
    recs = np.ascontiguousarray(recs, NULL_DTYPE)
    return _write(lib().prb_write_null_lines, db, qnames, qlen_unmasked, recs.ctypes.data if len(recs) else None, len(recs), id0, fd)


def write_group_lines(db, qnames, qlen_unmasked, recs, group_names, group_sizes, id0=0, fd=-1):
    """Lines of `ris -t -G FILE` for one batch: recs as GroupSet.finish returns them; group_names / group_sizes indexed by
    group.  -> (lines, bytes) written to fd (-1: formatted and counted only)."""
    recs = np.ascontiguousarray(recs, GROUP_DTYPE)
    gn = (ctypes.c_char_p * max(len(group_names), 1))(*[g.encode() for g in group_names])
    gsz = np.ascontiguousarray(group_sizes, np.int32)
    return _write(lib().prb_write_group_lines, db, qnames, qlen_unmasked, recs.ctypes.data if len(recs) else None, len(recs), gn,
                  gsz.ctypes.data if len(gsz) else None, len(group_names), id0, fd)


def write_feature_lines(db, qnames, qlen_unmasked, recs, feat_names, feat_start, feat_end, id0=0, fd=-1):
    """prb_write_feature_lines over FEATURE_DTYPE records; feat_names / feat_start / feat_end are indexed by their `feature`"""
    recs = np.ascontiguousarray(recs, FEATURE_DTYPE)
    names = (ctypes.c_char_p * max(len(feat_names), 1))(*[n.encode() for n in feat_names])
    fs, fe = np.ascontiguousarray(feat_start, np.int32), np.ascontiguousarray(feat_end, np.int32)
    return _write(lib().prb_write_feature_lines, db, qnames, qlen_unmasked, recs.ctypes.data if len(recs) else None, len(recs), names,
                  fs.ctypes.data, fe.ctypes.data, len(feat_names), id0, fd)


def write_grouprank_lines(db, qnames, qlen_unmasked, recs, group_names, group_sizes, id0=0, fd=-1):
    """Lines of `ris -t -G FILE -R N`: recs as GroupRank.finish returns them; qnames / qlen_unmasked indexed by query
    identifier, group_names / group_sizes by group.  -> (lines, bytes) written to fd (-1: formatted and counted only)."""
    recs = np.ascontiguousarray(recs, GROUP_DTYPE)
    gn = (ctypes.c_char_p * max(len(group_names), 1))(*[g.encode() for g in group_names])
    gsz = np.ascontiguousarray(group_sizes, np.int32)
    return _write(lib().prb_write_grouprank_lines, db, qnames, qlen_unmasked, recs.ctypes.data if len(recs) else None, len(recs), gn,
                  gsz.ctypes.data if len(gsz) else None, len(group_names), id0, fd)


def write_featrank_lines(db, qnames, qlen_unmasked, recs, feat_names, feat_start, feat_end, id0=0, fd=-1):
    """Lines of `ris -t -A FILE -B N`: recs as FeatRank.finish returns them; qnames / qlen_unmasked indexed by query
    identifier, feat_names / feat_start / feat_end by feature.  -> (lines, bytes) written to fd (-1: formatted and counted only)."""
    recs = np.ascontiguousarray(recs, FEATRANK_DTYPE)
    names = (ctypes.c_char_p * max(len(feat_names), 1))(*[n.encode() for n in feat_names])
    fs, fe = np.ascontiguousarray(feat_start, np.int32), np.ascontiguousarray(feat_end, np.int32)
    return _write(lib().prb_write_featrank_lines, db, qnames, qlen_unmasked, recs.ctypes.data if len(recs) else None, len(recs), names,
                  fs.ctypes.data, fe.ctypes.data, len(feat_names), id0, fd)


def write_null_fdr_lines(db, qnames, qlen_unmasked, recs, fdr, id0=0, fd=-1):
    """Lines of `ris -t -z N -Q` for one batch: recs and fdr as NullSet.finish_fdr returns them -> (lines, bytes)"""
    recs, fdr = np.ascontiguousarray(recs, NULL_DTYPE), np.ascontiguousarray(fdr, FDR_DTYPE)
    assert len(recs) == len(fdr)
    return _write(lib().prb_write_null_fdr_lines, db, qnames, qlen_unmasked, recs.ctypes.data if len(recs) else None,
                  fdr.ctypes.data if len(recs) else None, len(recs), id0, fd)


def write_fnull_lines(db, qnames, qlen_unmasked, recs, feat_names, feat_start, feat_end, id0=0, fd=-1):
    """Lines of `ris -t -A FILE -F N` for one batch: recs as FNullSet.finish returns them; feat_names / feat_start / feat_end
    indexed by their `feature`"""
    recs = np.ascontiguousarray(recs, FNULL_DTYPE)
    names = (ctypes.c_char_p * max(len(feat_names), 1))(*[n.encode() for n in feat_names])
    fs, fe = np.ascontiguousarray(feat_start, np.int32), np.ascontiguousarray(feat_end, np.int32)
    return _write(lib().prb_write_fnull_lines, db, qnames, qlen_unmasked, recs.ctypes.data if len(recs) else None, len(recs), names,
                  fs.ctypes.data, fe.ctypes.data, len(feat_names), id0, fd)


def write_gnull_lines(db, qnames, qlen_unmasked, recs, group_names, group_sizes, id0=0, fd=-1):
    """Lines of `ris -t -G FILE -P N` for one batch: recs as GNullSet.finish returns them; group_names / group_sizes indexed
    by group.  -> (lines, bytes) written to fd (-1: formatted and counted only)."""
    recs = np.ascontiguousarray(recs, GNULL_DTYPE)
    gn = (ctypes.c_char_p * max(len(group_names), 1))(*[g.encode() for g in group_names])
    gsz = np.ascontiguousarray(group_sizes, np.int32)
    return _write(lib().prb_write_gnull_lines, db, qnames, qlen_unmasked, recs.ctypes.data if len(recs) else None, len(recs), gn,
                  gsz.ctypes.data if len(gsz) else None, len(group_names), id0, fd)


def write_target_lines(db, qnames, qlen_unmasked, recs, id0=0, fd=-1):
    """Lines of `ris -r N`: recs as search_targets returns them; qnames / qlen_unmasked indexed by query identifier.
    -> (lines, bytes) written to fd (-1: formatted and counted only)."""
    recs = np.ascontiguousarray(recs, TARGET_DTYPE)
    return _write(lib().prb_write_target_lines, db, qnames, qlen_unmasked, recs.ctypes.data if len(recs) else None, len(recs), id0, fd)


def write_profile_lines(db, qnames, qlen_unmasked, rows, id0=0, fd=-1):
    """Lines of `ris -q` for one batch: rows as search_profile returns them.  -> (lines, bytes) written to fd
    (-1: formatted and counted only)."""
    rows = np.ascontiguousarray(rows, PROFILE_DTYPE)
    return _write(lib().prb_write_profile_lines, db, qnames, qlen_unmasked, rows.ctypes.data if len(rows) else None, len(rows), id0, fd)


def write_region_lines(db, qnames, qlen_unmasked, recs, id0=0, fd=-1):
    """Lines of `ris -c D`: recs as search_coverage returns them; qnames / qlen_unmasked indexed by query identifier.
    -> (lines, bytes) written to fd (-1: formatted and counted only)."""
    recs = np.ascontiguousarray(recs, REGION_DTYPE)
    return _write(lib().prb_write_region_lines, db, qnames, qlen_unmasked, recs.ctypes.data if len(recs) else None, len(recs), id0, fd)
