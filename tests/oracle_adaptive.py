"""The adaptive accumulation's stopping rule and round semantics in Python integers (include/vrt.h vrt_accum_begin_adaptive)
-- TEST INFRASTRUCTURE ONLY.

active() is the rule, exact. accumulate() applies it to per-sample frames from any of the checkers (oracle_samples,
oracle_jitter, oracle_lens): in round r every pixel active at the start of the round adds sample first + r. resolve() divides
each pixel's sums by its own count."""
import numpy as np


def active(n, s, q, min_samples, max_samples, tolerance):
    """the rule for one pixel: n samples, s = sum of L, q = sum of L^2 (L = R + G + B of one sample's bytes)"""
    n, s, q = int(n), int(s), int(q)
    if n < min_samples:
        return True
    if n >= max_samples:
        return False
    return 256 * (n * q - s * s) > tolerance * tolerance * n * n * (n - 1)


def active_map(n, s, q, min_samples, max_samples, tolerance):
    """the rule for every pixel -> bool array; object arrays of Python integers are exact at any size, int64 ones while
    tolerance^2 * n^3 and 256 * n * Q stay below 2^63 (a few hundred samples)"""
    lhs = 256 * (n * q - s * s)
    rhs = tolerance * tolerance * n * n * (n - 1)
    return np.asarray((n < min_samples) | ((n < max_samples) & (lhs > rhs)), dtype=bool)


class State:
    """Per-pixel sums (R, G, B), counts, S and Q of an adaptive accumulation, as Python integers (dtype=np.int64: faster, for
    large frames and few rounds)"""

    def __init__(self, height, width, dtype=object):
        self.dtype = dtype
        self.sums = np.zeros((height, width, 3), dtype=dtype)
        self.n = np.zeros((height, width), dtype=dtype)
        self.s = np.zeros((height, width), dtype=dtype)
        self.q = np.zeros((height, width), dtype=dtype)
        self.rounds = 0

    def active(self, rule):
        return active_map(self.n, self.s, self.q, *rule)

    def add_round(self, rgba, rule):
        """one round: the pixels active now add this sample's bytes (rgba8[H, W, 4])"""
        act = self.active(rule)
        b = rgba[..., :3].astype(np.int64).astype(self.dtype)
        L = b[..., 0] + b[..., 1] + b[..., 2]
        self.sums[act] += b[act]
        self.n[act] += 1
        self.s[act] += L[act]
        self.q[act] += L[act] * L[act]
        self.rounds += 1

    def counts(self):
        return self.n.astype(np.uint32)

    def resolve(self):
        """rgba8[H, W, 4]: (sum + n / 2) / n with each pixel's own n, alpha 255"""
        n = np.maximum(self.n, 1)
        out = np.full(self.sums.shape[:2] + (4,), 255, np.uint8)
        for c in range(3):
            out[..., c] = ((self.sums[..., c] + n // 2) // n).astype(np.int64).astype(np.uint8)
        return out


def accumulate(sample, height, width, first, rounds, rule, dtype=object):
    """sample(k) -> rgba8[H, W, 4] of sample index k (modulo 2^32); `rounds` rounds from sample `first` -> State"""
    st = State(height, width, dtype)
    for r in range(rounds):
        if not st.active(rule).any():
            st.rounds += 1
            continue
        st.add_round(sample((first + r) & 0xFFFFFFFF), rule)
    return st
