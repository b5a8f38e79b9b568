"""The decoys of a query (prb_shuffle_sequence, priblast_amd/host/shuffle.cpp) against the rule restated in
tests/shuffle_ref.py, and the properties that make a decoy a null for its query: length, both ends and every count of
adjacent bytes kept.  No GPU."""
import os
import random

import numpy as np
import pytest

import refdump
import shuffle_ref
from priblast_amd import capi

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

HAND = [
    "", "A", "AC", "ACG",                      # len 0 - 3 (below 3: a copy)
    "AAAAAAAAAAAA",                            # a homopolymer
    "ACACAC",                                  # one Eulerian walk only
    "ACGUACGGCAUUAGCAUCGACUAGCAUUCGAUCGAN",    # the last symbol occurs once
    "acguACGUacgGCAUuagcAUCGacuagCAUUcgaucga",  # mixed case: soft-masked letters are symbols of their own
    "GGGGGCCCCCGGGGGCCCCC",
]


def _cases():
    _, seqs = refdump.read_fasta(os.path.join(GOLDEN, "mix_q.fa"))
    return HAND + list(seqs)


def _pair_counts(b):
    m = np.zeros((256, 256), np.int64)
    a = np.frombuffer(b, np.uint8)
    if len(a) > 1:
        np.add.at(m, (a[:-1], a[1:]), 1)
    return m


@pytest.mark.parametrize("seed,file_pos,decoy", [(1, 0, 0), (1, 3, 2), (2 ** 64 - 1, 2 ** 40, 999), (12345, 7, 1)])
def test_equals_the_restatement(seed, file_pos, decoy):
    for s in _cases():
        got = capi.shuffle_sequence(s.encode(), seed, file_pos, decoy)
        assert got == shuffle_ref.shuffle(s.encode(), seed, file_pos, decoy), (s, seed, file_pos, decoy)


def test_keeps_length_ends_and_pair_counts():
    moved = 0
    for k, s in enumerate(_cases()):
        raw = s.encode()
        for d in range(3):
            got = capi.shuffle_sequence(raw, 1, k, d)
            assert len(got) == len(raw)
            if raw:
                assert got[0] == raw[0] and got[-1] == raw[-1]
            assert np.array_equal(_pair_counts(got), _pair_counts(raw)), (s, d)
            moved += got != raw
    assert moved > 0  # (the shuffle is not the identity)


def test_short_sequences_are_copied():
    for s in HAND[:3]:
        assert capi.shuffle_sequence(s, 5, 1, 1) == s


def test_mixed_case_stays_masked():
    s = HAND[7]
    got = capi.shuffle_sequence(s, 1, 0, 0)
    assert sorted(got) == sorted(s)  # every letter keeps its case


def test_same_arguments_same_bytes():
    for s in _cases():
        assert capi.shuffle_sequence(s, 9, 4, 2) == capi.shuffle_sequence(s, 9, 4, 2)


def test_decoys_seeds_and_places_differ():
    rnd = random.Random(5)
    s = "".join(rnd.choice("ACGU") for _ in range(200))
    decoys = [capi.shuffle_sequence(s, 1, 0, d) for d in range(8)]
    assert len(set(decoys)) == 8 and s not in decoys
    assert capi.shuffle_sequence(s, 2, 0, 0) != decoys[0]  # another seed, other decoys
    assert capi.shuffle_sequence(s, 1, 1, 0) != decoys[0]  # and so does the query's place in its file


def test_bad_arguments():
    L = capi.lib()
    assert L.prb_shuffle_sequence(b"ACGU", -1, 1, 0, 0, None) != 0
    assert L.prb_shuffle_sequence(b"ACGU", 4, 1, -1, 0, None) != 0
    assert L.prb_shuffle_sequence(None, 4, 1, 0, 0, None) != 0
