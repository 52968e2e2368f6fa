"""oracle/philox.py, the NumPy model of the device's Philox draws, on its own (no GPU): the
generator against Random123's known answers, the integer threshold compares against the
oracle's float compares, the counter layout, and draw injection into the oracle's run."""
import itertools
import math

import numpy as np
import pytest

from oracle import philox as PH
from oracle import spgg_oracle as O


# Random123 kat_vectors, philox2x32 10 rounds: (counter word 0, word 1), key, output
KAT = [((0x00000000, 0x00000000), 0x00000000, (0xff1dae59, 0x6cd10df2)),
       ((0xffffffff, 0xffffffff), 0xffffffff, (0x2c3f628b, 0xab4fd7ad)),
       ((0x243f6a88, 0x85a308d3), 0x13198a2e, (0xdd7ce038, 0xf62a4c12))]


def _philox_scalar(c0, c1, key, rounds=10):
    """The definition once more in Python integers (one block)."""
    for r in range(rounds):
        if r:
            key = (key + 0x9E3779B9) % 2**32
        p = 0xD256D193 * c0
        c0, c1 = (p >> 32) ^ key ^ c1, p % 2**32
    return c0, c1


@pytest.mark.parametrize("ctr,key,want", KAT)
def test_known_answers(ctr, key, want):
    x, y = PH.philox2x32_10(np.uint32(ctr[0]), np.uint32(ctr[1]), key)
    assert (int(x), int(y)) == want
    assert _philox_scalar(ctr[0], ctr[1], key) == want


def test_known_answers_vectorised_and_round_count():
    c0 = np.array([k[0][0] for k in KAT], dtype=np.uint32)
    c1 = np.array([k[0][1] for k in KAT], dtype=np.uint32)
    for i, (_, key, want) in enumerate(KAT):     # the key is a scalar: one call per vector, all counters
        x, y = PH.philox2x32_10(c0, c1, key)
        assert x.dtype == np.uint32 and x.shape == (3,)
        assert (int(x[i]), int(y[i])) == want
        x9, y9 = PH.philox2x32_10(c0, c1, key, rounds=9)
        assert (int(x9[i]), int(y9[i])) != want
    rs = np.random.RandomState(0)
    a, b = rs.randint(0, 2**32, size=(2, 64), dtype=np.uint64).astype(np.uint32)
    x, y = PH.philox2x32_10(a, b, 0xDEADBEEF)
    for i in range(64):
        assert (int(x[i]), int(y[i])) == _philox_scalar(int(a[i]), int(b[i]), 0xDEADBEEF)


EPS = ([0.0, 1.0, 0.5, 0.01] + [0.5 * 0.99 ** j for j in (1, 2, 3, 7, 19, 50, 123, 300, 389, 390, 1000)]
       + [2.0 ** -31, np.nextafter(2.0 ** -31, 0.0), np.nextafter(2.0 ** -31, 1.0), 2.0 ** -40,
          1.0 - 2.0 ** -53])


@pytest.mark.parametrize("eps", EPS)
def test_integer_threshold_is_the_float_compare(eps):
    """(bits >> 1) < thr31 on the device <=> u < eps in the oracle, u = (bits >> 1) / 2^31."""
    eps = float(eps)
    t53 = PH.u53_threshold(eps)
    assert t53 == math.ceil(eps * 2**53) and 0 <= t53 <= 2**53
    t31 = PH.thr31(t53)
    assert t31 == -(-t53 // 2**22) and 0 <= t31 <= 2**31
    ks = {0, 1, 2**31 - 1} | {t31 + d for d in (-2, -1, 0, 1)}
    for k in sorted(k for k in ks if 0 <= k < 2**31):
        u = np.float64(k) / 2.0 ** 31
        assert u * 2.0 ** 31 == k                   # exact in float64
        assert (k < t31) == bool(u < eps), (eps, k, t31)
    if eps == 0.0:
        assert t31 == 0
    if eps == 1.0:
        assert t31 == 2**31
    if 0.0 < eps <= 2.0 ** -31:
        assert t31 == 1                             # tiny eps rounds up: only k = 0 explores


def test_double_q_threshold():
    assert PH.DOUBLE_Q_THR53 == PH.u53_threshold(0.5) == 1 << 52
    t31 = PH.thr31(PH.DOUBLE_Q_THR53)
    assert t31 == 1 << 30
    for k in (0, 1, t31 - 2, t31 - 1, t31, t31 + 1, 2**31 - 1):
        assert (k < t31) == bool(np.float64(k) / 2.0 ** 31 < 0.5)


def test_u_and_b_are_the_bit_fields():
    key, L, t = PH.philox_key(5, 2), 13, 9
    bits = PH.select_bits(key, L, t, 0)
    d = PH.draws(key, L, t, "qlearning")
    assert set(d) == {"u", "b"} and d["u"].shape == d["b"].shape == (L, L)
    assert d["u"].dtype == np.float64
    assert np.array_equal(d["u"] * 2.0 ** 31, (bits >> np.uint32(1)).astype(np.float64))
    assert np.array_equal(d["b"], bits & np.uint32(1))
    assert d["u"].min() >= 0.0 and d["u"].max() < 1.0 and set(np.unique(d["b"])) == {0, 1}


@pytest.mark.parametrize("L", [13, 37])
def test_counter_layout(L):
    seed, t = 11, 7
    key = PH.philox_key(seed, 0)
    bits = PH.select_bits(key, L, t, 0).reshape(-1)
    # agents 2m and 2m+1 share block m, across the row end where L is odd
    for m in (0, 1, (L - 1) // 2, L // 2 + 3, (L * L - 3) // 2):
        w = _philox_scalar(m, t, key)
        assert (int(bits[2 * m]), int(bits[2 * m + 1])) == w
    m = (L - 1) // 2                        # pair (L - 1, L): the last cell of row 0, the first of row 1
    assert (2 * m) // L == 0 and (2 * m + 1) // L == 1
    # the lattice's last agent (even index L*L - 1) takes word 0 of a block of its own
    assert int(bits[-1]) == _philox_scalar((L * L - 1) >> 1, t, key)[0]
    # each select draws from a counter of its own: t + (k << 26)
    for k in (1, 2):
        bk = PH.select_bits(key, L, t, k).reshape(-1)
        assert (int(bk[2]), int(bk[3])) == _philox_scalar(1, t + (k << 26), key)
    sa, dq = PH.draws(key, L, t, "sarsa"), PH.draws(key, L, t, "double_qlearning")
    assert set(sa) == {"u", "b", "u2", "b2", "u3", "b3"} and set(dq) == {"u", "b", "u_upd"}
    nxt = PH.draws(key, L, t + 1, "sarsa")
    planes = [sa["u"], sa["u2"], sa["u3"], nxt["u"], nxt["u2"], nxt["u3"]]
    for a, b in itertools.combinations(planes, 2):
        assert np.mean(a == b) < 0.01
    bplanes = [sa["b"], sa["b2"], sa["b3"]]
    for a, b in itertools.combinations(bplanes, 2):
        assert 0.3 < np.mean(a == b) < 0.7
    assert np.array_equal(dq["u"], sa["u"]) and np.array_equal(dq["b"], sa["b"])
    assert np.array_equal(dq["u_upd"], sa["u2"])      # Double-Q's table choice is select 1
    # stream ids under one seed, and the high half of the seed, reach the key
    k1 = PH.philox_key(seed, 1)
    assert k1 != key and np.mean(PH.draws(k1, L, t)["u"] == sa["u"]) < 0.01
    assert PH.philox_key(seed + (1 << 32), 0) != key
    assert PH.philox_key(seed, 1 << 32) == key        # stream ids equal modulo 2^32 share a stream


def test_key_fold_wraps():
    assert PH.philox_key(0, 0) == 0
    assert PH.philox_key(0x7F4A7C15, 0) == 0x7F4A7C15
    assert PH.philox_key(1 << 32, 0) == 0x85EBCA6B
    assert PH.philox_key(0, 1) == 0xC2B2AE35
    seed, sid = 0x9E3779B97F4A7C15, 3
    want = 0x7F4A7C15 ^ ((0x9E3779B9 * 0x85EBCA6B) % 2**32) ^ ((3 * 0xC2B2AE35) % 2**32)
    assert PH.philox_key(seed, sid) == want and 0 <= want < 2**32
    assert PH.philox_key(seed, sid) != PH.philox_key(0x7F4A7C15, sid)


@pytest.mark.parametrize("alg", O.ALGORITHMS)
def test_injected_draws_reproduce_the_run(alg):
    L = 8
    p = O.Params(L=L, iterations=30, r=3.0, c=1, cost=1, alpha=0.8, gamma=0.9, epsilon=0.5, epsilon_decay=0.99,
                 epsilon_min=0.01, use_second_order=True, reward_weight_payoff=0.95, rep_gain_C=1.0,
                 algorithm=alg)
    ds0, f0 = O.run(p, np.random.RandomState(3))
    rs = np.random.RandomState(3)
    calls = []

    def inject(i):
        calls.append(i)
        return O.draw_step(rs, L, alg)

    ds1, f1 = O.run(p, rs, draws=inject)
    assert calls == list(range(1, len(calls) + 1)) and len(calls) == len(ds0["epsilon_history_final"])
    assert set(ds0) == set(ds1)
    for k in ds0:
        assert np.array_equal(ds0[k], ds1[k], equal_nan=ds0[k].dtype.kind == "f"), k
    for k in ("S", "R", "Q", "P"):
        assert np.array_equal(f0[k], f1[k]), k
    assert f0["stop_iter"] == f1["stop_iter"] and f0["epsilon"] == f1["epsilon"]
    if alg == "double_qlearning":
        assert np.array_equal(f0["tables"][0], f1["tables"][0]) and np.array_equal(f0["tables"][1], f1["tables"][1])


def test_run_without_a_generator():
    """rs may be None when the initial state and the draws are given."""
    L = 8
    p = O.Params(L=L, iterations=12, r=3.0, algorithm="sarsa")
    rs = np.random.RandomState(1)
    Q, _ = O.init_tables(p, rs)
    S = rs.randint(0, 2, size=(L, L))
    key = PH.philox_key(1, 0)
    a = O.run(p, None, S_init=S, Q_init=Q, draws=lambda i: PH.draws(key, L, i, "sarsa"))
    b = O.run(p, None, S_init=S, Q_init=Q, draws=lambda i: PH.draws(key, L, i, "sarsa"))
    assert np.array_equal(a[1]["S"], b[1]["S"]) and np.array_equal(a[1]["Q"], b[1]["Q"])
    c = O.run(p, None, S_init=S, Q_init=Q, draws=lambda i: PH.draws(PH.philox_key(1, 1), L, i, "sarsa"))
    assert not np.array_equal(a[1]["S"], c[1]["S"])


def test_absorption_case_of_the_gpu_test_absorbs():
    """The eps-edge GPU case (L=16, T=80, eps 1 -> 0.5 -> .. -> 0): at least one of its two
    replicas must absorb before T for the stop iteration and history lengths to be exercised."""
    from tests._philox import EDGE_CASE, philox_oracle_kw
    L, T, kws = EDGE_CASE["L"], EDGE_CASE["T"], EDGE_CASE["replicas"]
    stops = [philox_oracle_kw(L, T, {k: v for k, v in kw.items() if k != "seed"}, kw["seed"], i, False,
                              "reputation")[1]["stop_iter"] for i, kw in enumerate(kws)]
    assert any(0 < s < T for s in stops), stops
