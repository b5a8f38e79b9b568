#include "shuffle.hpp"

#include <algorithm>
#include <cstring>
#include <utility>
#include <vector>

namespace prb {

namespace {
constexpr uint64_t kGolden = 0x9E3779B97F4A7C15ull;

// the splitmix64 output for state x + kGolden
uint64_t mix(uint64_t x) {
  uint64_t z = x + kGolden;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
struct SplitMix {
  uint64_t state;
  uint64_t next() {
    const uint64_t z = mix(state);
    state += kGolden;
    return z;
  }
  size_t draw(size_t k) { return (size_t)(next() % (uint64_t)k); }
};
} // namespace

uint64_t shuffle_state(uint64_t seed, int64_t file_pos, int32_t decoy) {
  return mix(mix(mix(seed) ^ (uint64_t)file_pos) ^ (uint64_t)decoy);
}

void shuffle_sequence(const char *seq, int32_t len, uint64_t seed, int64_t file_pos, int32_t decoy, char *out) {
  if (len < 3) {
    if (len > 0) std::memcpy(out, seq, (size_t)len);
    return;
  }
  const uint8_t *s = reinterpret_cast<const uint8_t *>(seq);
  SplitMix rng{shuffle_state(seed, file_pos, decoy)};
  // 1. every symbol's successors, in order of occurrence
  std::vector<uint8_t> succ[256];
  for (int32_t i = 0; i + 1 < len; i++) succ[s[i]].push_back(s[i + 1]);
  const int last = s[len - 1];
  std::vector<int> inner; // the symbols that need a last edge, ascending
  for (int c = 0; c < 256; c++)
    if (c != last && !succ[c].empty()) inner.push_back(c);
  // 2. last edges, drawn until they form a tree into the last byte's symbol
  int edge[256];
  for (bool tree = false; !tree;) {
    for (int c : inner) edge[c] = succ[c][rng.draw(succ[c].size())];
    tree = true;
    for (int c : inner) {
      int t = c;
      for (size_t step = 0; t != last && step <= inner.size(); step++) t = edge[t];
      if (t != last) {
        tree = false;
        break;
      }
    }
  }
  // 3. the lists shuffled, the last edge at the end
  for (int c = 0; c < 256; c++) {
    std::vector<uint8_t> &l = succ[c];
    if (l.empty()) continue;
    if (c != last) {
      size_t at = l.size();
      while (l[--at] != (uint8_t)edge[c]) {
      }
      l.erase(l.begin() + (std::ptrdiff_t)at);
    }
    for (size_t i = l.size(); i-- > 1;) std::swap(l[i], l[rng.draw(i + 1)]);
    if (c != last) l.push_back((uint8_t)edge[c]);
  }
  // 4. the walk
  size_t used[256] = {0};
  int cur = s[0];
  out[0] = seq[0];
  for (int32_t i = 1; i < len; i++) {
    cur = succ[cur][used[cur]++];
    out[i] = (char)cur;
  }
}

} // namespace prb
