"""The non-default `ris` option sets of the option sweeps, once: tests/golden/make_golden.py (`mixopt`) writes the
reference's stage dumps for them on the `mix` case (tests/golden/mix_opt<k>.stg.gz, k = index in OPTION_SETS), and
tests/test_oracle_options.py (the restatement) and tests/test_gpu_options.py (the HIP path) are pinned to those.

No imports beyond the standard library: the generator runs where neither numpy nor the package need be present."""
import gzip
import os

OPTION_SETS = [
    dict(max_seed_length=8, hybrid_threshold=-4.0),
    dict(interaction_threshold=-2.0, final_threshold=-5.0),
    dict(drop_out_w_gap=4, drop_out_wo_gap=2),
    dict(drop_out_w_gap=30, drop_out_wo_gap=12, min_helix_length=1),
    dict(min_helix_length=5, final_threshold=-6.0),
    dict(min_helix_length=2),
    dict(min_helix_length=9, interaction_threshold=-2.0, final_threshold=-4.0, drop_out_w_gap=24),
    # odd and tiny -x: tier 0 takes two anti-diagonals per step, a direction without improvement (x + 1) / 2 steps
    dict(drop_out_w_gap=5, final_threshold=-6.0),
    dict(drop_out_w_gap=7, min_helix_length=4, final_threshold=-5.0),
    dict(drop_out_w_gap=1, final_threshold=-5.0),
    dict(drop_out_w_gap=19, drop_out_wo_gap=7),
]
# capi.default_opts keyword -> field of the restatement's orc_ris_opts / switch of `ris` and of `ref_harness stages`
ORACLE_NAMES = dict(max_seed_length="max_seed_length", hybrid_threshold="hybrid_thr", interaction_threshold="interaction_thr",
                    final_threshold="final_thr", drop_out_w_gap="drop_w_gap", drop_out_wo_gap="drop_wo_gap",
                    min_helix_length="min_helix")
SWITCHES = dict(max_seed_length="-l", hybrid_threshold="-e", interaction_threshold="-f", final_threshold="-g",
                drop_out_w_gap="-x", drop_out_wo_gap="-y", min_helix_length="-m")
# the seed list depends on these two alone; a fixture of a set that changes neither is stored with empty seed lists
# (make_golden.py checks them equal to mix.stg's, record for record, before it drops them)
SEED_OPTIONS = ("max_seed_length", "hybrid_threshold")
# the three sets whose ungapped lists (and, for the first, seed lists) the HIP path is compared on as well
STAGE_SETS = (0, 2, 3)

# The hits at which the reference's output differs from ours because of a tie of its comparator (deviation
# 1), as found when the fixtures were generated: (set index, query, page, q_sp, db_sp, q_len, db_len, db_id,
# db_id_start).  Each is proven a tie by the tests (two extended hits with these coordinates and bit-identical e_tot and
# e_acc, one the reference's, one ours) - a new one is a failure to look at, not an entry to add.
EXCUSED = {
    # {-f -2, -g -5}, query mq0, page 0: e_tot -5.133396243825555, e_acc 5.706603756174445 on both twins; the reference
    # keeps e_hyb -10.84 with the 1-nt bulge at database position 888 (pairs ... (80,887) (81,889) ...), we keep
    # e_hyb -10.840000000000002 with the bulge at 887 (... (80,888) (81,889) ...)
    (1, 0, 0, 75, 882, 12, 13, 3, 41),
}
MAX_EXCUSED_PER_LIST = 1
MAX_EXCUSED = 2


def holds_seeds(k):
    return any(o in OPTION_SETS[k] for o in SEED_OPTIONS)


def switches(kw):
    """The option set as command-line words: ["-l", "8", "-e", "-4", ...]."""
    out = []
    for name, v in kw.items():
        out += [SWITCHES[name], "%g" % v]
    return out


def fixture(k):
    return "mix_opt%d.stg.gz" % k


def unpack(golden, k, dst):
    """Unpacks one set's stage dump into the directory dst; returns its path."""
    path = os.path.join(dst, "mix_opt%d.stg" % k)
    with gzip.open(os.path.join(golden, fixture(k)), "rb") as f, open(path, "wb") as g:
        g.write(f.read())
    return path
