"""The step kernel's issue cuts (profiles/valu_diet/README.txt) against the oracle: S, R, Q and
the stop iteration bit for bit, every slot of the history record inside tests/_record.bounds.

The cuts change how the compile-time-width instance of four agents per thread computes, not
what: the agent slots that always hold an owned agent carry no ownership mask, one pass over the
S window builds the plus-count planes of S_t and S_{t-1}, the deferred NI term is added to the
entry the diagnostic selected, and the Philox explore bound is made in 31 bits.  So the cases are
that instance at the smallest lattice with two tiles each way (L = 120: 3 x 5 tiles of 40 x 24,
64 shadow slots in the last agent slot), kappa in {0, 0.5} x w_P in {1.0, 0.95} under both draw
streams; a run-time-width lattice whose tiles do not divide it (every slot masked: the path the
cuts must leave alone); and a replica that absorbs at all-D inside the run (the flush of the
finalised table after a recomputed NI record).  T <= 40; an oracle record takes about a second.
"""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import _record as R  # noqa: E402

L_CTW, T_CTW = 120, 40
KAPPA_WP = [(0.0, 1.0), (0.0, 0.95), (0.5, 1.0), (0.5, 0.95)]

# the absorbing replica: D favoured by one unit in every agent's table, exploration gone after a
# few iterations (eps = 0.1 * 0.1^t, no floor), r = 0.5
ABSORB = dict(R.BASE, influence_factor=0.5, reward_weight_payoff=0.95, r=0.5, epsilon=0.1, epsilon_decay=0.1,
              epsilon_min=0.0)
ABSORB_SEED, ABSORB_T = 7, 20


def _absorb_init():
    from spgg_amd.engine import reference_init
    init = reference_init(L_CTW, np.random.RandomState(ABSORB_SEED))
    init.Q[..., 0] -= 1.0
    init.Q[..., 1] += 1.0
    return init


@functools.lru_cache(maxsize=None)      # shared by the CPU check and the GPU case; read only
def _absorb_record():
    return R.philox_record(L_CTW, ABSORB_T, ABSORB, ABSORB_SEED, 0, False, "reputation", "qlearning",
                           init=_absorb_init())


def test_oracle_alone_absorbs_at_all_defect_within_the_run():
    """On the CPU: the oracle, with the chosen seed, absorbs at all-D after some iterations with
    cooperators (so the pending NI term was live) and before T."""
    rec = _absorb_record()
    assert 2 < rec.stop_iter < ABSORB_T, rec.stop_iter
    assert rec.value[rec.stop_iter, R.NCOOP] == 0.0                 # all-D, not all-C
    assert (rec.value[1:rec.stop_iter, R.NCOOP] > 0).all()


def _params(**kw):
    from spgg_amd.engine import ReplicaParams
    return ReplicaParams(**dict(R.BASE, **kw))


def _kw(p):
    return {k: getattr(p, k) for k in R.PARAM_KEYS}


def _record(rng, L, T, p, stream_id):
    if rng == "philox":
        return R.philox_record(L, T, _kw(p), p.seed, stream_id, False, "reputation", "qlearning")
    return R.exact_record(_kw(p), L, T, False, "reputation", "qlearning", rs=np.random.RandomState(p.seed))


def _force(monkeypatch, **env):
    for v in ("SPGG_APT", "SPGG_TILE", "SPGG_PERSIST", "SPGG_CACHE_MB", "SPGG_CHUNK", "SPGG_STREAMS",
              "SPGG_MT_CHUNK", "SPGG_MT_CHAINS", "SPGG_MT_PER_CHAIN", "SPGG_TILES_PER_STRIPE"):
        monkeypatch.delenv(v, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _compile_time_width_40(eng):
    """The library's instance rule (csrc/spgg_kernels.hip, twc_of) restated: four agents per thread,
    40-wide tiles of a lattice that is a multiple of 40 and at least 120, at most 25 rows, the
    shortest tile still past three full agent slots."""
    tw, th = eng.tile
    short = eng.L % th or th
    return tw == 40 and eng.L % 40 == 0 and eng.L >= 120 and th <= 25 and short * 40 > 3 * 256


def _run(L, T, reps, rng, recs, want_tile, **engine_kw):
    from spgg_amd.engine import BatchEngine
    from tests._philox import check_final
    assert L in R.GPU_LATTICES      # (test_record_bounds_cpu.py holds the bounds at these lattices)
    eng = BatchEngine(L, T, reps, use_second_order=False, state_representation="reputation", rng=rng,
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


def _tile_ctw(eng):
    assert eng.tile == (40, 24), eng.tile
    assert (eng.L // 40, eng.L // 24) == (3, 5)         # at least two tiles each way
    assert _compile_time_width_40(eng)


@pytest.mark.gpu
@pytest.mark.parametrize("rng", ["philox", "mt19937"])
def test_compile_time_width_instance_matches_oracle(rng, monkeypatch):
    _force(monkeypatch, SPGG_APT="max")
    reps = [_params(influence_factor=k, reward_weight_payoff=w, seed=60 + i, r=3.0 + 0.5 * i)
            for i, (k, w) in enumerate(KAPPA_WP)]
    recs = [_record(rng, L_CTW, T_CTW, p, k) for k, p in enumerate(reps)]
    _run(L_CTW, T_CTW, reps, rng, recs, _tile_ctw)


@pytest.mark.gpu
def test_run_time_width_tiles_not_dividing_the_lattice_match_oracle(monkeypatch):
    """L = 80, four agents per thread: 27 x 27 tiles (729 agents: the third slot partly, the fourth
    wholly shadow slots), the last tile row and column past the edge, so every agent slot keeps
    its ownership mask."""
    _force(monkeypatch, SPGG_APT="max")
    L, T = 80, 30
    reps = [_params(influence_factor=k, reward_weight_payoff=w, seed=70 + i, r=3.0 + 1.2 * i)
            for i, (k, w) in enumerate([(0.5, 0.95), (0.0, 1.0)])]

    def tile(eng):
        assert 512 < eng.tile[0] * eng.tile[1] <= 1024 and L % eng.tile[0] and L % eng.tile[1], eng.tile
        assert not _compile_time_width_40(eng)

    _run(L, T, reps, "philox", [_record("philox", L, T, p, k) for k, p in enumerate(reps)], tile)


@pytest.mark.gpu
def test_absorption_at_all_defect_inside_the_run_matches_oracle(monkeypatch):
    _force(monkeypatch, SPGG_APT="max")
    rec = _absorb_record()
    assert 2 < rec.stop_iter < ABSORB_T     # (the CPU test above says why)
    p = _params(seed=ABSORB_SEED, **ABSORB)
    _run(L_CTW, ABSORB_T, [p], "philox", [rec], _tile_ctw, init=[_absorb_init()])
