// Decoys for an empirical null of interaction energies: shuffles of a query that keep its dinucleotide counts (Altschul & Erikson 1985), so that a
// decoy has the composition and the nearest-neighbour make-up of its query and none of its biology.  The rule - the
// lists, the order of the draws, the generator and its seeding - is in include/priblast_hip.h (prb_shuffle_sequence);
// tests/shuffle_ref.py restates it.  Behind prb_shuffle_sequence.
#pragma once
#include <cstdint>

namespace prb {

// the generator's first state for decoy `decoy` of the sequence at place file_pos of its file
uint64_t shuffle_state(uint64_t seed, int64_t file_pos, int32_t decoy);
// out[0, len) = the decoy of seq[0, len) over its bytes as read: first byte, last byte and every count of adjacent bytes
// kept; len < 3 copies.  `out` must not overlap `seq`.
void shuffle_sequence(const char *seq, int32_t len, uint64_t seed, int64_t file_pos, int32_t decoy, char *out);

} // namespace prb
