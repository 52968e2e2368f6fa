"""NumPy model of the device's Philox draws (rng="philox") -- TEST INFRASTRUCTURE ONLY.

Written from the definition of Philox2x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random
numbers: as easy as 1, 2, 3", SC'11) and the stream contract in include/spgg_abi.h
(SPGG_RNG_PHILOX), not from anything the device computes:

  key      (uint32) seed ^ (uint32)(seed >> 32) * 0x85EBCA6B ^ (uint32) stream_id * 0xC2B2AE35
           (products modulo 2^32; `*` binds tighter than `^`)
  counter  word 0 = g >> 1 for the agent of raster index g = y * L + x,
           word 1 = t + (k << 26): iteration t = 1, 2, .. and select k (0: the action select;
           SARSA 1, 2: its second and third selects; Double-Q 1: the table choice)
  bits     output word g & 1 of that block
  u        (bits >> 1) / 2^31, exact in float64;   b = bits & 1

With these u the oracle's own `u < eps` and `u_upd < 0.5` decide what the device decides with
its integer compares (thr31 below; tests/test_philox_oracle_cpu.py proves the equivalence), so
`spgg_oracle.run(..., draws=...)` fed from draws() is the device's Philox trajectory.
"""
from __future__ import annotations

import math

import numpy as np

from .spgg_oracle import canonical_algorithm

PHILOX_M2X32 = 0xD256D193   # the 2x32 round multiplier
PHILOX_W32 = 0x9E3779B9     # key bump (golden ratio)
KEY_MUL_SEED_HI = 0x85EBCA6B
KEY_MUL_STREAM = 0xC2B2AE35
SELECT_SHIFT = 26           # counter word 1 = t + (k << 26): iterations < 2^26
MASK32 = 0xFFFFFFFF


def philox2x32_10(c0, c1, key, rounds: int = 10):
    """Philox2x32-10 of counter (c0, c1) under `key`, vectorised over uint32 arrays.

    A round maps (L, R) = (c0, c1) to (mulhi(M, L) ^ key ^ R, mullo(M, L)); the key grows by
    PHILOX_W32 before every round but the first.  Returns the two output words (uint32)."""
    c0 = np.asarray(c0, dtype=np.uint32).astype(np.uint64)
    c1 = np.asarray(c1, dtype=np.uint32).astype(np.uint64)
    c0, c1 = np.broadcast_arrays(c0, c1)
    k = int(key) & MASK32
    for r in range(rounds):
        if r:
            k = (k + PHILOX_W32) & MASK32
        p = np.uint64(PHILOX_M2X32) * c0            # 32 x 32 -> 64: no overflow in uint64
        hi, lo = p >> np.uint64(32), p & np.uint64(MASK32)
        c0, c1 = hi ^ np.uint64(k) ^ c1, lo
    return c0.astype(np.uint32), c1.astype(np.uint32)


def philox_key(seed: int, stream_id: int) -> int:
    """The replica's 32-bit key: the 64-bit seed folded with the low 32 bits of the stream id."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    lo, hi = seed & MASK32, seed >> 32
    return lo ^ ((hi * KEY_MUL_SEED_HI) & MASK32) ^ (((int(stream_id) & MASK32) * KEY_MUL_STREAM) & MASK32)


def select_bits(key: int, L: int, t: int, k: int = 0) -> np.ndarray:
    """(L, L) uint32: every agent's 32 bits of select k at iteration t."""
    g = np.arange(L * L, dtype=np.uint32)
    w1 = np.uint32((int(t) + (int(k) << SELECT_SHIFT)) & MASK32)
    x, y = philox2x32_10(g >> np.uint32(1), w1, key)
    return np.where((g & np.uint32(1)) == 1, y, x).reshape(L, L)


def _u_b(bits):
    return (bits >> np.uint32(1)).astype(np.float64) / 2.0 ** 31, (bits & np.uint32(1)).astype(np.int64)


def draws(key: int, L: int, t: int, algorithm: str = "qlearning") -> dict:
    """The draws of iteration t, with the keys and shapes of spgg_oracle.draw_step."""
    if not 0 < int(t) < (1 << SELECT_SHIFT):
        raise ValueError(f"iteration {t} outside 1 .. 2^{SELECT_SHIFT} - 1")
    d = {}
    d["u"], d["b"] = _u_b(select_bits(key, L, t, 0))
    alg = canonical_algorithm(algorithm)
    if alg == "sarsa":
        d["u2"], d["b2"] = _u_b(select_bits(key, L, t, 1))
        d["u3"], d["b3"] = _u_b(select_bits(key, L, t, 2))
    elif alg == "double_qlearning":
        d["u_upd"], _ = _u_b(select_bits(key, L, t, 1))
    return d


# ---- the device's integer compares, in Python integers ---------------------------------------

def u53_threshold(thr: float) -> int:
    """ceil(thr * 2^53) for thr in [0, 1]: the product by 2^53 is exact in float64."""
    return math.ceil(float(thr) * 9007199254740992.0)


def thr31(thr53: int) -> int:
    """ceil(thr53 / 2^22): explore <=> (bits >> 1) < thr31."""
    return (int(thr53) + ((1 << 22) - 1)) >> 22


DOUBLE_Q_THR53 = 1 << 52    # the table choice rand < 0.5
