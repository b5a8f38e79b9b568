"""Final hit lists against the reference's, with the one difference DESIGN.md 2 (deviation 1) allows - and only on proof.

Two gapped extensions can end on the same six coordinates with bit-identical total and accessibility energy and yet
hold different base pairs (and a hybridization sum that differs in its last bit).  They are a tie of the reference's
comparator: its std::sort leaves their order open and CheckRedundancy keeps whichever comes first; our total order
keeps the one with the lower e_hyb.  A (reference hit, our hit) pair that differs is excused only if the list of
extended hits before the final sort and filter (oraclelib.Db.stages(..., extended=True)) holds both twins."""
import numpy as np

COORDS = ("q_sp", "db_sp", "q_len", "db_len", "db_id", "db_id_start")


def b64(x):
    return int(np.asarray(x, np.float64).view(np.uint64))


def coords(h):
    return tuple(int(h[k]) for k in COORDS)


def tie_key(h):
    """What two twins share: the coordinates and the bits of e_tot and e_acc."""
    return coords(h) + (b64(h["e_tot"]), b64(h["e_acc"]))


def identity(h):
    """Everything the comparison is exact on after the gapped stage."""
    return tie_key(h) + (b64(h["e_hyb"]), np.ascontiguousarray(h["bp"], np.int32).tobytes())


def unmatched(mine, ref):
    """The two lists as multisets of identity(): (our hits the reference does not have, its hits we do not have)."""
    left = {}
    for h in ref:
        left.setdefault(identity(h), []).append(h)
    only_mine = []
    for h in mine:
        same = left.get(identity(h))
        if same:
            same.pop()
        else:
            only_mine.append(h)
    return only_mine, [h for l in left.values() for h in l]


def pair_twins(only_mine, only_ref):
    """Pairs the leftovers of unmatched() by tie_key; anything that finds no partner is a plain difference."""
    assert len(only_mine) == len(only_ref), (only_mine, only_ref)
    rest = list(only_ref)
    pairs = []
    for a in only_mine:
        partner = [b for b in rest if tie_key(b) == tie_key(a)]
        assert len(partner) == 1, ("no tie: a hit the reference does not have", a, only_ref)
        rest.remove(partner[0])
        pairs.append((a, partner[0]))
    return pairs


def prove_tie(ours, theirs, extended):
    """The proof: two DIFFERENT entries of `extended` that agree with the pair on tie_key, one equal to ours, the other
    to the reference's, e_hyb and base pairs included."""
    assert tie_key(ours) == tie_key(theirs) and identity(ours) != identity(theirs)
    twins = [h for h in extended if tie_key(h) == tie_key(ours)]
    ids = [identity(h) for h in twins]
    assert identity(ours) in ids and identity(theirs) in ids, ("not a tie of two extended hits", ours, theirs, twins)
