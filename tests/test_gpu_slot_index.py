"""The step kernel's slot word by region index (profiles/slot_index/README.txt) against the oracle:
S, R, Q and the stop iteration bit for bit, every slot of the history record inside
tests/_record.bounds.

The change is integer index arithmetic and register selects in the per-launch large-batch Philox
instance of compile-time width: the slot word holds the agent's index at the planes' common pitch
(the plus-count planes took that pitch) and the agent's global index is held per slot.  So the
cases are that instance at
the smallest lattice that reaches it (L = 120: 3 x 5 tiles of 40 x 24, 64 shadow slots in the last
agent slot), kappa in {0, 0.5, 1} x w_P in {1.0, 0.95} under both draw streams (MT19937 takes the
instance that keeps the (row, column) word on the new plus-count pitch); the bench's own tile
(L = 200: 40 x 25, the last slot partly shadow); the persistent form and an absorbing stop's
flush against the per-launch path; and the paths the change must leave alone (M = 2, a run-time
width).  T <= 30; an oracle record takes about a second.
"""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import _record as R  # noqa: E402
from tests import test_gpu_issue_cuts as C  # noqa: E402  (its helpers and its absorbing replica)

L_CTW, T_CTW = 120, 30
KAPPA_WP = [(k, w) for k in (0.0, 0.5, 1.0) for w in (1.0, 0.95)]


def _replicas(seed0, kappa_wp=KAPPA_WP):
    return [C._params(influence_factor=k, reward_weight_payoff=w, seed=seed0 + i, r=3.0 + 0.4 * i)
            for i, (k, w) in enumerate(kappa_wp)]


@functools.lru_cache(maxsize=None)      # one oracle run per (stream, shape, replica): read only
def _record(rng, L, T, seed0, i, M2=False):
    p = _replicas(seed0)[i]
    if rng == "philox":
        return R.philox_record(L, T, C._kw(p), p.seed, i, M2, "reputation", "qlearning")
    return R.exact_record(C._kw(p), L, T, M2, "reputation", "qlearning", rs=np.random.RandomState(p.seed))


def _check(L, T, reps, rng, recs, want_tile, M2=False, **engine_kw):
    """Run `reps` and hold every replica to its oracle record: test_gpu_issue_cuts._run with the
    neighbourhood as an argument and without its `L in R.GPU_LATTICES` guard, which would keep
    the bench's own lattice out -- L = 200 is not in that table, but tests/test_record_bounds_cpu.py
    holds the bounds there too (its VARIANTS), and its tile kind (40 x 25, four per thread) is the
    table's L = 1000 entry."""
    from spgg_amd.engine import BatchEngine
    from tests._philox import check_final
    eng = BatchEngine(L, T, reps, use_second_order=M2, state_representation="reputation", rng=rng,
                      algorithm="qlearning", **engine_kw)
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
@pytest.mark.parametrize("rng", ["philox", "mt19937"])
def test_slot_index_instance_matches_oracle(rng, monkeypatch):
    """kappa in {0, 0.5, 1} x w_P in {1, 0.95} (w_rep = 0 and 0.05), 30 iterations."""
    C._force(monkeypatch, SPGG_APT="max")
    reps = _replicas(160)
    recs = [_record(rng, L_CTW, T_CTW, 160, i) for i in range(len(reps))]
    _check(L_CTW, T_CTW, reps, rng, recs, C._tile_ctw)


@pytest.mark.gpu
def test_bench_tile_with_partly_shadow_last_slot_matches_oracle(monkeypatch):
    """L = 200, four agents per thread as in the bench's large batch: 5 x 8 tiles of 40 x 25 = 1000
    agents, 24 shadow slots in the last agent slot."""
    C._force(monkeypatch, SPGG_APT="max")
    L, T = 200, 5
    reps = _replicas(170)[3:5]          # kappa = 0.5 at w_P = 0.95, kappa = 1 at w_P = 1

    def tile(eng):
        assert eng.tile == (40, 25), eng.tile

    recs = [R.philox_record(L, T, C._kw(p), p.seed, k, False, "reputation", "qlearning")
            for k, p in enumerate(reps)]
    _check(L, T, reps, "philox", recs, tile)


def _final(monkeypatch, persist, L, T, reps, **engine_kw):
    from spgg_amd.engine import BatchEngine
    C._force(monkeypatch, SPGG_APT="max", SPGG_PERSIST="1" if persist else "0")
    eng = BatchEngine(L, T, reps, use_second_order=False, state_representation="reputation", rng="philox",
                      algorithm="qlearning", **engine_kw)
    try:
        C._tile_ctw(eng)
        assert eng.persistent == persist, (eng.persistent, eng.persist_capacity)
        eng.run(snapshots=False)
        return [eng.final_state(k) for k in range(len(reps))], [int(s) for s in eng.stop_iter.cpu().numpy()]
    finally:
        eng.close()


@pytest.mark.gpu
def test_persistent_form_stores_the_same_q_planes(monkeypatch):
    """The persistent form keeps the (row, column) slot word and stores both Q rows by state after
    its last iteration; the per-launch form stores the rows each launch changed.  Same planes."""
    reps = _replicas(180)[2:4]
    fa, sa = _final(monkeypatch, True, L_CTW, T_CTW, reps)
    fb, sb = _final(monkeypatch, False, L_CTW, T_CTW, reps)
    assert sa == sb == [0, 0]
    for k, (x, y) in enumerate(zip(fa, fb)):
        for name, u, v in zip("QRS", x, y):
            assert np.array_equal(u, v), (k, name)


@pytest.mark.gpu
def test_flush_after_an_absorbing_stop_stores_the_same_q_planes(monkeypatch):
    """The replica of test_gpu_issue_cuts that absorbs at all-D inside the run: the absorbing
    iteration stores the finalised table (both rows, after the pending NI term) in the per-launch
    and in the persistent form; both equal the oracle's."""
    from tests._philox import check_final
    rec = C._absorb_record()
    assert 2 < rec.stop_iter < C.ABSORB_T
    p = C._params(seed=C.ABSORB_SEED, **C.ABSORB)
    fa, sa = _final(monkeypatch, True, L_CTW, C.ABSORB_T, [p], init=[C._absorb_init()])
    fb, sb = _final(monkeypatch, False, L_CTW, C.ABSORB_T, [p], init=[C._absorb_init()])
    assert sa == sb == [rec.stop_iter]
    for name, u, v in zip("QRS", fa[0], fb[0]):
        assert np.array_equal(u, v), name
    check_final(fb[0], rec.final, 0)


@pytest.mark.gpu
def test_second_order_neighbourhood_matches_oracle(monkeypatch):
    """M = 2 at the same tiles, the compile-time-width instance of four agents per thread: it keeps
    the (row, column) word (the gate excludes the second order); its plus-count planes take the
    common pitch (a row of region + 1 ring is 48 bytes of 52)."""
    C._force(monkeypatch, SPGG_APT="max")
    T = 10
    reps = _replicas(190)[3:4]

    def tile(eng):
        assert eng.tile == (40, 24), eng.tile
        assert C._compile_time_width_40(eng)

    recs = [R.philox_record(L_CTW, T, C._kw(p), p.seed, k, True, "reputation", "qlearning")
            for k, p in enumerate(reps)]
    _check(L_CTW, T, reps, "philox", recs, tile, M2=True)


@pytest.mark.gpu
def test_run_time_width_matches_oracle(monkeypatch):
    """L = 80: 27 x 27 tiles, a run-time width (plus-count pitch 64, the (row, column) word)."""
    C._force(monkeypatch, SPGG_APT="max")
    L, T = 80, 20
    reps = _replicas(200)[4:6]          # kappa = 1 at both w_P

    def tile(eng):
        assert L % eng.tile[0] and not C._compile_time_width_40(eng), eng.tile

    recs = [R.philox_record(L, T, C._kw(p), p.seed, k, False, "reputation", "qlearning")
            for k, p in enumerate(reps)]
    _check(L, T, reps, "philox", recs, tile)
