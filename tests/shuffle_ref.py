"""The decoy shuffle restated in Python (include/priblast_hip.h, prb_shuffle_sequence): the tests'
yardstick for priblast_amd/host/shuffle.cpp, written from the rule, not from the C++."""

MASK = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15


def mix(x):
    """the splitmix64 output for state x (the increment included)"""
    z = (x + GOLDEN) & MASK
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
    return z ^ (z >> 31)


class SplitMix:
    def __init__(self, state):
        self.state = state & MASK

    def next(self):
        self.state = (self.state + GOLDEN) & MASK
        z = self.state
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
        return z ^ (z >> 31)

    def draw(self, k):
        return self.next() % k


def first_state(seed, file_pos, decoy):
    return mix(mix(mix(seed & MASK) ^ (file_pos & MASK)) ^ (decoy & MASK))


def shuffle(seq, seed, file_pos, decoy):
    """seq: bytes; returns the decoy as bytes"""
    seq = bytes(seq)
    n = len(seq)
    if n < 3:
        return seq
    rng = SplitMix(first_state(seed, file_pos, decoy))
    succ = {}
    for a, b in zip(seq, seq[1:]):
        succ.setdefault(a, []).append(b)
    last = seq[-1]
    inner = sorted(c for c in succ if c != last)
    while True:
        edge = {c: succ[c][rng.draw(len(succ[c]))] for c in inner}
        ok = True
        for c in inner:
            t, steps = c, 0
            while t != last and steps <= len(inner):
                t = edge[t]
                steps += 1
            if t != last:
                ok = False
                break
        if ok:
            break
    for c in sorted(succ):
        l = succ[c]
        if c != last:
            at = len(l) - 1 - l[::-1].index(edge[c])
            del l[at]
        for i in range(len(l) - 1, 0, -1):
            j = rng.draw(i + 1)
            l[i], l[j] = l[j], l[i]
        if c != last:
            l.append(edge[c])
    used = {c: 0 for c in succ}
    out = bytearray([seq[0]])
    cur = seq[0]
    for _ in range(1, n):
        nxt = succ[cur][used[cur]]
        used[cur] += 1
        out.append(nxt)
        cur = nxt
    return bytes(out)
