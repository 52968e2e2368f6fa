"""The seven in-run device records (clusters, correlations, reputation, dwell, policy, payoff, pair_map),
armed together, under every launch layout of BatchEngine.step: one group, a run that starts late, resident
groups through spgg_step_groups and through one spgg_step call per group (SPGG_INTERLEAVE=0), cache-blocked
waves on shared streams, groups retired mid-run (SPGG_SKIP_DEAD), persistent launches (the five kinds that
are allowed there), and the tiled cluster kernel beside the other six.

Every expectation comes from one oracle run per replica (tests/_observers.py): the existing host models
on the oracle's S_t / R_t and tables, which the device had no part in.  Each case also holds the run
itself to the oracle -- S, R, Q, the stop iteration and the MT19937 key bit for bit -- which is "the
records do not disturb the run" for all seven at once.  tests/test_records_layouts_cpu.py holds, on the
oracle alone, that the batches are not absorbed away, that a record of the planes of iteration t - 1
would differ, and that the periods interleave.  Integers and bit patterns, exact; no tolerance."""
import time

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import spgg_amd  # noqa: E402
from spgg_amd import dwell as DW, pairmap as PM, payoff as PF, policy as PL, spgg as SP  # noqa: E402
from spgg_amd.engine import BatchEngine  # noqa: E402
from spgg_amd.h5io import read_datasets  # noqa: E402
from tests import _observers as OB  # noqa: E402
from tests import _params as P  # noqa: E402
from tests.test_gpu_parity import APPROX  # noqa: E402
from tests.test_gpu_record import _force  # noqa: E402

# the engine's own knobs that tests/test_gpu_record._force leaves alone
ENGINE_KNOBS = ("SPGG_INTERLEAVE", "SPGG_ENQ_CHUNK", "SPGG_SKIP_DEAD", "SPGG_REP_F64", "SPGG_OWN_STREAMS",
                "SPGG_SHARED_DRAW_STREAM")


def _engine(b, **kw):
    reps = [P.replica_params(row, s) for row, s in zip(b.rows, b.seeds)]
    return BatchEngine(b.L, b.T, reps, use_second_order=b.M2, state_representation=b.state, rng=b.rng, algorithm=b.alg, **kw)


def _force_layout(monkeypatch, lay, b, **more):
    """The layout's environment and nothing else: a stray override of the caller's cannot change it."""
    monkeypatch.setenv("SPGG_TUNING", "1")
    for v in ENGINE_KNOBS:
        monkeypatch.delenv(v, raising=False)
    env = dict(lay.env, **more)
    if env.get("SPGG_CACHE_MB") == "budget":      # four replicas' state, by the engine's own per-replica figure
        _force(monkeypatch)
        probe = _engine(b, streams=lay.streams)
        per_replica = probe.state_bytes_per_replica()
        probe.close()
        env["SPGG_CACHE_MB"] = repr(4 * per_replica / 2**20)
    _force(monkeypatch, **env)


def _assert_layout(name, eng, skip_dead=None):
    got = dict(waves=eng.waves, G=eng.G, resident=eng.resident, persistent=eng.persistent, interleave=eng.interleave)
    print("layout", name, eng.rng, got, "rep_int8", eng.rep_int8, "tile", eng.tile)
    if name in ("one_group", "one_group_f64", "late_start", "tiled_clusters"):
        assert eng.G == 1 and not eng.persistent, got
    elif name == "groups":
        assert eng.G == eng.resident == 3 and eng.interleave and eng.double_q, got
    elif name == "no_interleave":
        assert eng.G == eng.resident == 3 and not eng.interleave and eng.enqueue_chunk == 8, got
    elif name == "waves":
        assert eng.waves == 3 and eng.G == 6 and eng.resident == 2 and eng.chunk == 7, got
    elif name == "retired":
        assert eng.G == eng.resident == 3 and eng.interleave and eng.skip_dead == (skip_dead == "1"), got
    elif name == "persistent":
        assert eng.persistent and eng.G == 1, got
    else:
        raise ValueError(name)
    assert eng.rep_int8 == (name != "one_group_f64")


CASES = [pytest.param(name, rng, skip, id=f"{name}{'[SPGG_SKIP_DEAD=%s]' % skip if skip else ''}-{rng}")
         for name, rng in OB.CASES for skip in (("1", "0") if name == "retired" else (None,))]


@pytest.mark.parametrize("name,rng,skip_dead", CASES)
def test_records_under_layout(name, rng, skip_dead, monkeypatch):
    lay = OB.LAYOUTS[name]
    b = lay.batch(rng)
    s = lay.settings
    t_oracle = time.perf_counter()
    exp = lay.expected(rng)
    t_oracle = time.perf_counter() - t_oracle
    _force_layout(monkeypatch, lay, b, **({"SPGG_SKIP_DEAD": skip_dead} if skip_dead else {}))
    t_dev = time.perf_counter()
    eng = _engine(b, streams=lay.streams)
    try:
        _assert_layout(name, eng, skip_dead)
        if name == "one_group_f64":      # the pair sums are the int8 path's: refused before anything is enqueued
            with pytest.raises(ValueError, match="f64"):
                eng.run(snapshots=False, **OB.run_kwargs(OB.settings()))
            assert eng.t == 1 and not eng.records and eng.dwell_t_ref is None
        if lay.first:
            eng.step(lay.first)
        assert eng.t == s["t0"]
        eng.run(chunk=lay.chunk, snapshots=False, **OB.run_kwargs(s))
        if name == "retired":
            live = [g["live"] for g in eng.groups]
            assert live == ([False, True, True] if skip_dead == "1" else [True] * 3), (live, eng.stopped)
            if skip_dead == "1":      # retired mid-run, not at the end: its context stayed behind the engine's t
                assert eng.groups[0]["t_retired"] < b.T - lay.chunk, eng.groups[0]["t_retired"]
        OB.assert_all(eng, exp, s)
        OB.assert_run(eng, exp)
    finally:
        eng.close()
    print("seconds", name, rng, skip_dead, "oracle %.2f" % t_oracle, "device and checks %.2f" % (time.perf_counter() - t_dev))


# ---- the drop-in, every option at once ------------------------------------------------------------------------------------
DROPIN_SEED = 4242
DROPIN = dict(L=16, iterations=14, r=3.0, use_second_order=True)


def _dropin_batch():
    """The drop-in's constructor defaults (spgg.py:50-56) as a one-replica batch."""
    row = dict(r=3.0, c=1, cost=0.5, alpha=0.1, gamma=0.9, epsilon=0.5, epsilon_decay=0.995, epsilon_min=0.01,
               influence_factor=1.0, lambda_epsilon=0.01, delta_R_D=1, R_min=-10, R_max=10, reward_weight_payoff=1.0,
               rep_gain_C=0.5, alg_alpha=None, alg_gamma=None)
    return P.Batch("dropin", "mt19937", DROPIN["L"], DROPIN["iterations"], True, "reputation", "qlearning", [row], (DROPIN_SEED,))


def test_dropin_writes_every_record_at_once(tmp_path):
    s = OB.settings(clusters=dict(periodic=True))
    exp = OB.expected(_dropin_batch(), s["policy"]["bins"], s["policy"]["gap_range"])
    e = exp[0]
    assert e.stop_iter == 0
    orig = np.random.seed
    np.random.seed = lambda seed=None: orig(DROPIN_SEED if seed is None else seed)      # SPGG.__init__ reseeds from entropy
    try:
        m = spgg_amd.SPGG(**DROPIN)
    finally:
        np.random.seed = orig
    m.save_png = False
    m.cluster_history_every, m.cluster_history_periodic = s["clusters"]["every"], True
    m.correlation_history_every, m.correlation_max_distance = s["correlations"]["every"], s["correlations"]["max_d"]
    m.reputation_history_every, m.reputation_history_bins = s["reputation"]["every"], s["reputation"]["bins"]
    m.reputation_max_distance = s["reputation"]["max_d"]
    m.dwell_history_every, m.dwell_fields = s["dwell"]["every"], True
    m.policy_history_every, m.policy_history_bins = s["policy"]["every"], s["policy"]["bins"]
    m.policy_history_gap_range, m.policy_map_final = s["policy"]["gap_range"], True
    m.payoff_history_every, m.payoff_max_distance, m.payoff_map_final = s["payoff"]["every"], s["payoff"]["max_d"], True
    m.pair_map_history_every, m.pair_map_max_distance = s["pair_map"]["every"], s["pair_map"]["max_d"]
    m.pair_map_fields = [list(p) for p in s["pair_map"]["fields"]]
    m.folder = str(tmp_path)
    fn = str(tmp_path / "experiment_data.h5")
    m.run(fn)
    ds = read_datasets(fn)

    # every dataset of the seven records, once, and no name shared between two kinds
    want = {kind: OB.datasets(e, kind, s[kind]) for kind in OB.KINDS}
    maps = tuple(PM.dataset_name(a, b) for a, b in s["pair_map"]["fields"])
    names = dict(clusters=SP.CLUSTER_DATASETS, correlations=SP.CORRELATION_DATASETS, reputation=SP.REPUTATION_DATASETS,
                 dwell=DW.DWELL_DATASETS, policy=PL.POLICY_DATASETS, payoff=PF.PAYOFF_DATASETS + (PF.PAYOFF_PAIRS_DATASET,),
                 pair_map=(PM.PAIR_MAP_ITERS_DATASET, PM.PAIR_MAP_DISTANCE_DATASET) + maps)
    every = ([n for kind in OB.KINDS for n in names[kind]] + list(DW.DWELL_FIELD_DATASETS)
             + [PL.POLICY_MAP_DATASET, PF.PAYOFF_MAP_DATASET])
    assert len(set(every)) == len(every) and set(every) <= set(ds), sorted(set(every) - set(ds))
    assert not set(every) & set(e.datasets)
    for kind in OB.KINDS:
        assert tuple(want[kind]) == tuple(names[kind]), kind
        for name, w in want[kind].items():
            g, w = ds[name], np.asarray(w)
            if w.ndim == 0:
                assert g.size == 1 and g.dtype == w.dtype and g.ravel()[0] == w, (kind, name, g, w)
            else:
                assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), (kind, name, g.tolist(), w.tolist())
    row, f, freq = OB.final_dwell(e)
    L = DROPIN["L"]
    for name, w in zip(DW.DWELL_FIELD_DATASETS, (f[0], f[1], freq)):
        assert ds[name].dtype == w.dtype and np.array_equal(ds[name], w.reshape(L, L)), name
    assert ds[PL.POLICY_MAP_DATASET].dtype == np.uint8
    assert np.array_equal(ds[PL.POLICY_MAP_DATASET], e.policy.planes[e.t_final])
    assert ds[PF.PAYOFF_MAP_DATASET].dtype == np.uint8
    assert np.array_equal(ds[PF.PAYOFF_MAP_DATASET], PF.host_payoff_census(e.S[e.t_final])[1])

    # the reference's own datasets: the oracle's.  The sums the step kernels reduce in another order than np.mean
    # (tests/test_gpu_parity.APPROX) are held by test_spgg_dropin_matches_reference, not here
    for name, w in e.datasets.items():
        assert ds[name].shape == np.shape(w), (name, ds[name].shape, np.shape(w))
        if name not in APPROX:
            assert np.array_equal(ds[name], w, equal_nan=np.asarray(w).dtype.kind == "f"), name
    for i in (1, 10):
        assert np.array_equal(ds[f"Sn_snapshot_{i}"], e.S[i]) and np.array_equal(ds[f"R_snapshot_{i}"], e.R[i]), i
    assert set(ds) - set(every) - set(e.datasets) == {f"{n}_{i}" for n in ("Sn_snapshot", "R_snapshot", "rep_hist", "rep_bins")
                                                     for i in (1, 10)}
    assert np.array_equal(m._Sn, e.final["S"]) and np.array_equal(m.R, e.final["R"]) and np.array_equal(m.q_table, e.final["Q"])
    st = np.random.get_state()
    assert st[2] == e.mt[1] and np.array_equal(np.asarray(st[1], dtype=np.uint32), e.mt[0])
