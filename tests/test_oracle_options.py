"""Pins the CPU restatement (oracle/*.c) to the UNMODIFIED reference under the non-default `ris` options of
tests/option_sets.py: the reference's stage dumps of the `mix` case (tests/golden/mix_opt<k>.stg.gz, written by
make_golden.py mixopt).  CPU only.  test_gpu_options.py pins the HIP path to the same files."""
import os

import pytest

import option_sets
import refdump
import tiecheck
from option_sets import OPTION_SETS
from test_oracle import _key, _same_hit

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# (seed, ungapped, gapped) hits of the reference over the 7 queries x 3 pages, per set
COUNTS = [
    (38330, 2156, 35),
    (13357, 5785, 1158),
    (13357, 1732, 19),
    (13357, 1803, 42),
    (13357, 1787, 332),
    (13357, 1787, 33),
    (13357, 5785, 2586),
    (13357, 1787, 299),
    (13357, 1787, 984),
    (13357, 1787, 981),
    (13357, 1800, 35),
]


@pytest.fixture(scope="module")
def excused_log():
    """The excused hits of every set this session ran, for the cap over the whole sweep."""
    return {}


@pytest.mark.parametrize("k", range(len(OPTION_SETS)))
def test_option_stage_dumps(oracle, golden_dir, tmp_path, excused_log, k):
    """test_oracle.py::test_stage_dumps per option set: seed hits in the reference's emission order (where the fixture
    holds them), the ungapped list as a multiset with the split to 1e-12, the final list as a multiset, exact - but
    for proven ties (tiecheck.py), which must be exactly the ones recorded in option_sets.EXCUSED."""
    kw = OPTION_SETS[k]
    names, seqs = refdump.read_fasta(os.path.join(GOLDEN, "mix_q.fa"))
    stg = refdump.read_stages(option_sets.unpack(GOLDEN, k, str(tmp_path)))
    db = oracle.Db(os.path.join(golden_dir, "mixdb"))
    opts = oracle.default_opts(**{option_sets.ORACLE_NAMES[o]: v for o, v in kw.items()})
    n = [0, 0, 0]
    excused = set()
    try:
        for rec in stg:
            where = (k, rec["q"], rec["page"])
            seed, ung, gap, ext = db.stages(seqs[rec["q"]], rec["page"], opts, extended=True)
            if option_sets.holds_seeds(k):
                assert len(seed) == len(rec["seed"]), where
                for a, b in zip(seed, rec["seed"]):
                    assert _same_hit(a, b), (where, a, b)
            else:
                assert rec["seed"] == []
            assert len(ung) == len(rec["ungapped"]), where
            for a, b in zip(sorted(ung, key=_key), sorted(rec["ungapped"], key=_key)):
                assert _same_hit(a, b, 1e-12), (where, a, b)
            assert len(gap) == len(rec["gapped"]), where
            pairs = tiecheck.pair_twins(*tiecheck.unmatched(gap, rec["gapped"]))
            assert len(pairs) <= option_sets.MAX_EXCUSED_PER_LIST, (where, pairs)
            for ours, theirs in pairs:
                tiecheck.prove_tie(ours, theirs, ext)
                assert ours["e_hyb"] < theirs["e_hyb"], (where, ours, theirs)  # the total order: the lower e_hyb stays
                excused.add(where + tiecheck.coords(ours))
            n[0] += len(seed)
            n[1] += len(ung)
            n[2] += len(gap)
    finally:
        db.close()
    assert tuple(n) == COUNTS[k]
    assert excused == {e for e in option_sets.EXCUSED if e[0] == k}
    excused_log[k] = excused
    assert sum(len(v) for v in excused_log.values()) <= option_sets.MAX_EXCUSED


def test_excused_hits_are_within_the_cap():
    """At most two excused hits over the whole sweep, at most one per (query, page) list - on the recorded set, which
    every parameter above is asserted equal to."""
    assert len(option_sets.EXCUSED) <= option_sets.MAX_EXCUSED
    lists = [e[:3] for e in option_sets.EXCUSED]
    assert all(lists.count(l) <= option_sets.MAX_EXCUSED_PER_LIST for l in lists)


def test_fixtures_drop_only_the_seed_lists_that_mix_stg_holds():
    """Which fixtures hold seeds follows from the options alone: -l and -e decide the seed list."""
    assert [k for k in range(len(OPTION_SETS)) if option_sets.holds_seeds(k)] == [0]
    assert set(option_sets.STAGE_SETS) == {OPTION_SETS.index(s) for s in (
        dict(drop_out_w_gap=4, drop_out_wo_gap=2), dict(drop_out_w_gap=30, drop_out_wo_gap=12, min_helix_length=1),
        dict(max_seed_length=8, hybrid_threshold=-4.0))}
