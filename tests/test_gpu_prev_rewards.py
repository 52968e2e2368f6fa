"""The step kernel's previous rewards per agent slot and its unit-weight reward path
(profiles/prev_rewards/README.txt) against the oracle: S, R, Q and the stop iteration bit for bit,
every slot of the history record inside tests/_record.bounds.

Both changes sit in the per-launch large-batch Philox instances of compile-time width (the slot
word by region index): the rewards of iteration t-1 are evaluated by the thread that owns the
agent, and by one pass over the ring cells, instead of a loop over the region (Q-learning and
Expected SARSA, replicas with kappa != 0); and a replica with w_P == 1 (w_rep == 0) takes rew = P
at every reward site (SARSA too).  Which thread evaluates which cell changes, and which
instructions run; no floating-point operation on the way to a result does.  So the cases are that
instance at the smallest lattice that reaches it (L = 120: 3 x 5 tiles of 40 x 24, so a tile has
interior and wrapped neighbours and the ring crosses the periodic edge), kappa in {0, 0.5, 1} at
w_P = 1, w_P in {0.95, 0} beside it (w_P = 0: the product w_P * P is a zero), the bench's own
tile at L = 200, one launch whose workgroups take different branches, the other two operators,
and two instances the change must leave alone (M = 2 at a run-time width, MT19937).  T <= 30.
"""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import _record as R  # noqa: E402
from tests import test_gpu_issue_cuts as C  # noqa: E402  (its helpers)

L_CTW, T = 120, 30


def _rep(i, kappa, w_p, seed0):
    return C._params(influence_factor=kappa, reward_weight_payoff=w_p, seed=seed0 + i, r=3.0 + 0.4 * i)


@functools.lru_cache(maxsize=None)      # one oracle run per case: read only
def _record(rng, alg, L, T, M2, i, kappa, w_p, seed0):
    p = _rep(i, kappa, w_p, seed0)
    if rng == "philox":
        return R.philox_record(L, T, C._kw(p), p.seed, i, M2, "reputation", alg)
    return R.exact_record(C._kw(p), L, T, M2, "reputation", alg, rs=np.random.RandomState(p.seed))


def _check(L, T, kappa_wp, seed0, want_tile, rng="philox", alg="qlearning", M2=False):
    """Run one replica per (kappa, w_P) in one launch group and hold each to its oracle record."""
    from spgg_amd.engine import BatchEngine
    from tests._philox import check_final
    reps = [_rep(i, k, w, seed0) for i, (k, w) in enumerate(kappa_wp)]
    recs = [_record(rng, alg, L, T, M2, i, k, w, seed0) for i, (k, w) in enumerate(kappa_wp)]
    eng = BatchEngine(L, T, reps, use_second_order=M2, state_representation="reputation", rng=rng, algorithm=alg)
    try:
        want_tile(eng)
        assert eng.rep_int8         # the bench's int8 reputation path
        eng.run(snapshots=False)
        st = eng.stats_folded().cpu().numpy()
        eng.all_stopped()
        assert st.shape == (len(recs), T + 2, R.NSTAT)
        for k, rec in enumerate(recs):
            bad = R.mismatches(st[k], rec, R.bounds(rec, apt_max=4, rep_int8=eng.rep_int8))
            assert not bad, "replica %d: (t, slot, got, want, bound) %s (%d in all)" % (k, bad[:12], len(bad))
            assert int(eng.stopped[k]) == rec.stop_iter, (k, int(eng.stopped[k]), rec.stop_iter)
            check_final(eng.final_state(k), rec.final, k)
    finally:
        eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kappa", [0.0, 0.5, 1.0])
def test_unit_weights_match_oracle(kappa, monkeypatch):
    """w_P = 1: rew = P at every site; kappa != 0 adds the per-slot previous rewards."""
    C._force(monkeypatch, SPGG_APT="max")
    _check(L_CTW, T, [(kappa, 1.0)], 300, C._tile_ctw)


@pytest.mark.gpu
@pytest.mark.parametrize("w_p", [0.95, 0.0])
def test_general_weights_match_oracle(w_p, monkeypatch):
    """The general path beside the new one; w_P = 0 makes w_P * P a zero product (w_rep = 1)."""
    C._force(monkeypatch, SPGG_APT="max")
    _check(L_CTW, T, [(0.5, w_p)], 310, C._tile_ctw)


@pytest.mark.gpu
def test_bench_tile_matches_oracle(monkeypatch):
    """One replica at L = 200: 5 x 8 tiles of 40 x 25, the last agent slot partly shadow."""
    C._force(monkeypatch, SPGG_APT="max")

    def tile(eng):
        assert eng.tile == (40, 25), eng.tile

    _check(200, 20, [(0.5, 1.0)], 320, tile)


@pytest.mark.gpu
def test_second_order_run_time_width_matches_oracle(monkeypatch):
    """L = 80, M = 2: a run-time width and the second order, neither path reaches it."""
    C._force(monkeypatch, SPGG_APT="max")

    def tile(eng):
        assert not C._compile_time_width_40(eng), eng.tile

    _check(80, T, [(0.5, 1.0)], 330, tile, M2=True)


@pytest.mark.gpu
def test_mt19937_matches_oracle(monkeypatch):
    """MT19937 at the same tiles keeps the (row, column) word, the region loop and the general path."""
    C._force(monkeypatch, SPGG_APT="max")
    _check(L_CTW, T, [(0.5, 1.0)], 340, C._tile_ctw, rng="mt19937")


@pytest.mark.gpu
def test_workgroups_of_one_launch_take_different_branches(monkeypatch):
    """Four replicas in one launch, w_P = 1 and 0.95 alternating."""
    C._force(monkeypatch, SPGG_APT="max", SPGG_STREAMS="1")
    _check(L_CTW, T, [(0.5, 1.0), (0.5, 0.95), (0.5, 1.0), (0.5, 0.95)], 350, C._tile_ctw)


@pytest.mark.gpu
@pytest.mark.parametrize("alg", ["expected_sarsa", "sarsa"])
def test_other_operators_match_oracle(alg, monkeypatch):
    """Expected SARSA recomputes the record too (its eps_{t-1} target); SARSA keeps the stored record
    and takes the unit-weight path alone."""
    C._force(monkeypatch, SPGG_APT="max")
    _check(L_CTW, T, [(0.5, 1.0)], 360, C._tile_ctw, alg=alg)
