"""The pair maps on the device (spgg_pair_map; BatchEngine.pair_map, run(pair_map_every=)) against the host
model (spgg_amd.pairmap: np.roll) on synthetic byte planes and on the oracle's S_{t-1}, S_t.  Integers, exact;
no expectation comes from the device.  The shapes are the smallest at which each part can go wrong: sides the
map wraps onto itself at, an odd side, exactly one word and a second word of one bit, three and four dx
blocks, the thresholds between the count instances, a side above every LDS instance."""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import spgg_amd  # noqa: E402
from spgg_amd import _lib, pairmap as PM, sweep as SW  # noqa: E402
from spgg_amd.engine import BatchEngine  # noqa: E402
from spgg_amd.h5io import h5native, read_datasets  # noqa: E402
from tests import _observers as OB  # noqa: E402
from tests import _pairmap as K  # noqa: E402
from tests import _params as P  # noqa: E402
from tests import _record as R  # noqa: E402
from tests.test_gpu_payoff import _plane_engine, _set_planes  # noqa: E402
from tests.test_gpu_record import _force  # noqa: E402

NAMES = ("random", "checkerboard", "all_c", "all_d", "one_cell")


def _check_planes(L, distances, groups=((0, 1, 2), (3, 4)), axis_rows=True):
    """Replicas with different lattices per engine; every pair of fields at every distance; t = 2 (plane 1)."""
    pats = K.patterns(L)
    engines = {}
    try:
        for group in groups:
            names = [NAMES[i] for i in group]
            eng = engines.setdefault(len(names), _plane_engine(L, len(names)))
            planes = [K.byte_plane(*pats[name], seed=100 * L + i) for i, name in zip(group, names)]
            assert all(np.any(p & ~np.uint8(K.KEEP)) for p in planes) or L == 1
            _set_planes(eng, planes, buf=1)
            eng.t = 2                                   # the state of iteration 2 lies in plane 1
            for k, (name, plane) in enumerate(zip(names, planes)):
                f = PM.host_fields(plane, 2)
                for D in distances:
                    for a, b in K.ALL_PAIRS:
                        want = PM.host_pair_map(f[a], f[b], D)
                        got = eng.pair_map(k, a, b, D)
                        assert got.dtype == np.int64 and got.shape == PM.map_shape(D)
                        assert np.array_equal(got, want), (L, name, a, b, D, np.argwhere(got != want)[:6].tolist())
                    if axis_rows and L <= eng.correlations_max_side:
                        pc, cc = eng.pair_counts(k, D), eng.pair_map(k, "coop", "coop", D)
                        assert np.array_equal(cc[0, D:], pc[0]) and np.array_equal(cc[0, D::-1], pc[0]), (L, name, D)
                        assert np.array_equal(cc[:, D], pc[1]), (L, name, D)
    finally:
        for e in engines.values():
            e.close()


# ---- synthetic planes -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [1, 2, 3, 5, 13, 32, 33, 70, 100])
def test_synthetic_planes(L):
    """1, 2, 3, 5: the map wraps onto itself, aliased columns; 13: odd, replica planes at odd byte offsets; 32 and
    33: exactly one word, a second word of one bit; 70: three words and three dx blocks at D = 35; 100: four
    blocks.  D = L // 2 and one smaller value."""
    D = L // 2
    assert {70: 3, 100: 4}.get(L, K.dx_blocks(D)) == K.dx_blocks(D)
    assert K.instance(L, D) == "small"
    _check_planes(L, sorted({D, K.smaller(L)}))


EDGES = K.instance_edges(3)


@pytest.mark.parametrize("L", [side for edge in EDGES for side in edge] + [1000])
def test_instance_thresholds(L):
    """The last side of each count instance and the first of the next (16 KiB of LDS, 160 KiB, the workspace in
    L2) at D = 3; L = 1000 at D = 2."""
    assert [K.instance(a, 3) + ">" + K.instance(b, 3) for a, b in EDGES] == ["small>full", "full>global"]
    D = 2 if L == 1000 else 3
    assert L != 1000 or K.instance(L, D) == "global"
    _check_planes(L, [D], groups=((0, 4),), axis_rows=False)


def test_full_lds_instance_at_full_distance():
    """L = 200 at D = 100: the 160 KiB instance, seven blocks, the last one cut at 2 D."""
    assert K.instance(200, 100) == "full" and K.dx_blocks(100) == 7
    _check_planes(200, [100], groups=((0, 1),), axis_rows=False)


# ---- the plane rule ---------------------------------------------------------------------------------------------------
STOPS = (0, 3, 4, 6, 1)     # live; absorbed at an odd, at an even iteration; at the first observed one; at t = 1
TIMES = (6, 7)


def test_absorbed_replicas_read_the_plane_of_their_absorbing_iteration():
    """tests/test_gpu_observed_plane.py's rule for this observer: every replica holds two different lattices; the
    map of t is that of plane (tt - 1) & 1, tt = s for a replica absorbed at s < t.  The flip field of a state
    of iteration 1 is zero whatever bit 3 holds."""
    L, Rn = 5, len(STOPS)
    rs = np.random.RandomState(43)
    S = rs.randint(0, 256, (2, Rn, L, L)).astype(np.uint8)
    eng = _plane_engine(L, Rn, T=8)
    try:
        torch.cuda.synchronize()
        eng.S.copy_(torch.from_numpy(S.reshape(2, Rn, L * L)).to(eng.dev))
        eng.stop_iter.copy_(torch.tensor(STOPS, dtype=torch.int32).to(eng.dev))
        torch.cuda.synchronize()
        D = L // 2
        ws = eng._pair_map_work(D)
        width = (D + 1) * (2 * D + 1)
        for t in TIMES + (1,):
            for a, b in K.ALL_PAIRS:
                out = torch.full((Rn, width), -7, dtype=torch.int32, device=eng.dev)
                eng._observe(eng.lib.spgg_pair_map, t, (PM.FIELDS[a], PM.FIELDS[b], D, ws), out)
                torch.cuda.synchronize()
                for k, stop in enumerate(STOPS):
                    tt = stop if stop != 0 and stop < t else t
                    p = (tt - 1) & 1
                    f, other = PM.host_fields(S[p, k], tt), PM.host_fields(S[1 - p, k], tt)
                    want = PM.host_pair_map(f[a], f[b], D)
                    if tt > 1:
                        assert not np.array_equal(want, PM.host_pair_map(other[a], other[b], D)), k   # the planes tell apart
                    else:
                        assert np.any((S[p, k] ^ (S[p, k] >> 3)) & 1) and (want.any() == ((a, b) == ("coop", "coop")))
                    assert np.array_equal(out[k].cpu().numpy().reshape(D + 1, 2 * D + 1), want), (t, k, tt, a, b)
    finally:
        eng.close()


# ---- bit 3 on real runs: the in-run record --------------------------------------------------------------------------------
ABSORBING = dict(R.BASE, alg_alpha=None, alg_gamma=None, epsilon=0.0, epsilon_min=0.0)
EVERY, MAX_D = 3, 4
FIELDS = K.PAIRS


def _batch(rng, alg="qlearning"):
    """L = 18, four replicas: one with kappa != 0 and one with kappa = 0 that run on, one that absorbs at t = 6
    (between two recorded iterations), one that absorbs at t = 16 (a recorded one; under Double-Q it runs on)."""
    rows = [P.B_ROWS["dyadic"][0], dict(ABSORBING, reward_weight_payoff=0.0, influence_factor=0.0),
            dict(ABSORBING, reward_weight_payoff=0.0), dict(ABSORBING, reward_weight_payoff=1.0, r=2.0, cost=4)]
    return P.Batch("pair_map", rng, 18, 20, True, "reputation", alg, rows, (900, 902, 902, 901))


def _engine(b, **kw):
    reps = [P.replica_params(row, s) for row, s in zip(b.rows, b.seeds)]
    return BatchEngine(b.L, b.T, reps, use_second_order=b.M2, state_representation=b.state, rng=b.rng, algorithm=b.alg, **kw)


def _check_final(eng, exp):
    for k, e in enumerate(exp):
        t = e.t_final
        f = PM.host_fields(K.oracle_bytes(e, t), t)
        for a, b in K.ALL_PAIRS:
            assert np.array_equal(eng.pair_map(k, a, b, MAX_D), PM.host_pair_map(f[a], f[b], MAX_D)), (k, a, b)


def _check_flips_against_the_history(eng, hist):
    """map_FF[0][D] of a recorded t > 1 is SW_CD + SW_DC of iteration t - 1."""
    own = eng.histories()
    seen = 0
    for k, h in enumerate(hist):
        sw = np.asarray(own[k]["switch_C_to_D"]) + np.asarray(own[k]["switch_D_to_C"])
        for row, t in enumerate(h["pair_map_history_iters"]):
            got = int(h["pair_map_flip_flip_history"][row, 0, MAX_D])
            assert got == (int(sw[t - 2]) if t > 1 else 0), (k, t, got)
            seen += got
    assert seen > 0


def _run_and_check(b, monkeypatch, streams=1, **env):
    _force(monkeypatch, **env)
    exp = OB.expected(b)
    assert [e.stop_iter for e in exp] == [0, 0, 6, 0 if b.alg == "double_qlearning" else 16]
    assert float(b.rows[0]["influence_factor"]) != 0.0 and float(b.rows[1]["influence_factor"]) == 0.0
    want = [K.datasets(e, EVERY, MAX_D, FIELDS) for e in exp]
    assert any(w["pair_map_flip_flip_history"][1:].any() for w in want)
    eng = _engine(b, streams=streams)
    try:
        assert eng.G == streams and not eng.persistent
        eng.run(snapshots=False, pair_map_every=EVERY, pair_map_max_d=MAX_D, pair_map_fields=FIELDS)
        hist = eng.pair_map_histories()
        for k in range(len(exp)):
            K.compare(hist[k], want[k], k)
        OB.assert_run(eng, exp)                   # the run itself is the oracle's: the record does not disturb it
        _check_flips_against_the_history(eng, hist)
        _check_final(eng, exp)
        return eng.tile
    finally:
        eng.close()


@pytest.mark.parametrize("streams", [1, 3])
@pytest.mark.parametrize("rng", ["mt19937", "philox"])
def test_in_run_record(rng, streams, monkeypatch):
    b = _batch(rng)
    _run_and_check(b, monkeypatch, streams=streams)


@pytest.mark.parametrize("apt", ["1", "max"])
@pytest.mark.parametrize("alg", P.ALGS)
def test_every_operator_holds_the_previous_strategy_in_bit_3(alg, apt, monkeypatch):
    """All four operators at one and at their most agents per thread."""
    tw, th = _run_and_check(_batch("philox", alg), monkeypatch, SPGG_APT=apt)
    assert (tw * th <= 256) == (apt == "1"), (tw, th)         # 256 threads per tile: more agents than that share threads


def test_continued_with_the_same_and_with_other_settings(monkeypatch):
    _force(monkeypatch)
    b = _batch("philox")
    exp = OB.expected(b)
    T0 = 5
    eng = _engine(b)
    try:
        eng.step(T0 - 1)
        eng.run(snapshots=False, pair_map_every=EVERY, pair_map_max_d=MAX_D, pair_map_fields=FIELDS)       # recorded from t0 = 5 on
        rec, outs = eng.records["pair_map"], list(eng.records["pair_map"].out)
        assert rec.t0 == T0 and rec.key == (EVERY, MAX_D, FIELDS)
        shape = (4, (b.T - T0) // EVERY + 1, (MAX_D + 1) * (2 * MAX_D + 1))
        assert [tuple(o.shape) for o in outs] == [shape] * 3 and all(o.dtype == torch.int32 for o in outs)
        first = eng.pair_map_histories()
        for k, e in enumerate(exp):
            K.compare(first[k], K.datasets(e, EVERY, MAX_D, FIELDS, t0=T0), k)
        eng.run(snapshots=False, pair_map_every=EVERY, pair_map_max_d=MAX_D, pair_map_fields=FIELDS)       # the same record
        assert eng.records["pair_map"] is rec and all(x is y for x, y in zip(rec.out, outs))
        for x, y in zip(first, eng.pair_map_histories()):
            assert all(np.array_equal(x[key], y[key]) for key in x)
        OB.assert_run(eng, exp)
        _check_final(eng, exp)
        eng.run(snapshots=False, pair_map_every=2)                                # other settings: afresh at the current t
        other = eng.records["pair_map"]
        assert other is not rec and other.t0 == eng.t == b.T + 1 and other.key == (2, 9, (("coop", "coop"),)) and len(other.out) == 1
        for h in eng.pair_map_histories():
            assert len(h["pair_map_history_iters"]) == 0 and list(h) == ["pair_map_history_iters", "pair_map_max_distance",
                                                                         "pair_map_coop_coop_history"]
        eng.run(snapshots=False)                                                  # nothing asked: the record stays readable
        assert eng.records["pair_map"] is other
    finally:
        eng.close()


def test_persistent_context(monkeypatch):
    """A function of S_t alone: allowed on a context that steps in persistent launches, at its launch boundaries."""
    monkeypatch.setenv("SPGG_TUNING", "1")
    _force(monkeypatch, SPGG_PERSIST="1", SPGG_APT="2")
    b = P.batch_f(60)
    b = b._replace(rows=b.rows[:3], seeds=b.seeds[:3])
    exp = OB.expected(b)
    eng = _engine(b)
    try:
        assert eng.persistent
        eng.run(chunk=5, snapshots=False, pair_map_every=EVERY, pair_map_max_d=MAX_D, pair_map_fields=FIELDS)
        hist = eng.pair_map_histories()
        for k, e in enumerate(exp):
            K.compare(hist[k], K.datasets(e, EVERY, MAX_D, FIELDS), k)
        OB.assert_run(eng, exp)
        _check_final(eng, exp)
    finally:
        eng.close()


# ---- the drop-in and the sweep --------------------------------------------------------------------------------------------
def _check_file(ds, L, every, D, pairs):
    its = np.arange(1, len(ds["coop_rate_history"]) + 1, every)
    assert np.array_equal(ds["pair_map_history_iters"], its) and ds["pair_map_history_iters"].dtype == np.int64
    assert ds["pair_map_max_distance"].size == 1 and int(ds["pair_map_max_distance"].ravel()[0]) == D and ds["pair_map_max_distance"].dtype == np.int64
    names = {PM.dataset_name(a, b) for a, b in pairs}
    assert {n for n in ds if n.startswith("pair_map_")} == names | {"pair_map_history_iters", "pair_map_max_distance"}
    for n in names:
        assert ds[n].shape == (len(its),) + PM.map_shape(D) and ds[n].dtype == np.int64, n
    assert its[0] == 1 and its[3] == 10           # the rows of the reference's snapshot iterations 1 and 10
    cc = ds["pair_map_coop_coop_history"]
    for row, i in ((0, 1), (3, 10)):
        c = ds[f"Sn_snapshot_{i}"] == 0
        assert np.array_equal(cc[row], PM.host_pair_map(c, c, D)), i
    nc = np.rint(ds["coop_rate_history"] * L * L).astype(np.int64)
    assert np.array_equal(cc[:, 0, D], nc[its - 1])
    if "pair_map_flip_flip_history" in ds:
        sw = np.rint(ds["switch_C_to_D"] + ds["switch_D_to_C"]).astype(np.int64)
        ff = ds["pair_map_flip_flip_history"][:, 0, D]
        assert ff[0] == 0 and np.array_equal(ff[1:], sw[its[1:] - 2]) and ff.any()


SINKS = ("npz",) + (("native",) if h5native.available() else ())
try:
    import h5py  # noqa: F401
    SINKS += ("h5py",)
except ImportError:
    pass


@pytest.mark.parametrize("sink", SINKS)
def test_dropin_writes_the_datasets(sink, tmp_path, monkeypatch):
    monkeypatch.setenv("SPGG_H5_SINK", sink)
    L, T = 16, 20
    m = spgg_amd.SPGG(L=L, iterations=T, r=3.0, use_second_order=True)
    m.save_png = False
    m.pair_map_history_every, m.pair_map_max_distance, m.pair_map_fields = 3, 5, K.PAIRS
    m.folder = str(tmp_path)
    fn = str(tmp_path / "experiment_data.h5")
    m.run(fn)
    ds = read_datasets(fn)
    assert len(ds["coop_rate_history"]) == T
    _check_file(ds, L, 3, 5, K.PAIRS)

    m2 = spgg_amd.SPGG(L=L, iterations=T, r=3.0, use_second_order=True)      # the defaults: the file of before
    m2.save_png = False
    m2.folder = str(tmp_path / "plain")
    fn2 = str(tmp_path / "plain.h5")
    m2.run(fn2)
    plain = read_datasets(fn2)
    extra = {n for n in ds if n.startswith("pair_map_")}
    assert len(extra) == 5 and not extra & set(plain) and set(ds) - set(plain) == extra and set(plain) <= set(ds)


@pytest.mark.parametrize("sink", SINKS)
def test_sweep_carries_the_options(sink, tmp_path, monkeypatch):
    monkeypatch.setenv("SPGG_H5_SINK", sink)
    monkeypatch.chdir(tmp_path)
    combos = [(3.0, 1.0, False, 0.8, 1.0, 1.0, "reputation", "qlearning"), (4.0, 0.5, False, 0.8, 0.9, 1.0, "reputation", "qlearning")]
    SW.run_batch(combos, seeds=[1, 2], save_png=False, verbose=False, L=16, iterations=14, pair_map_history_every=3,
                 pair_map_fields=(("coop", "coop"), ("flip", "flip")))
    for p in combos:
        got = read_datasets(str(tmp_path / SW.get_folder_name(*SW.unpack(p)) / "data" / "experiment_data.h5"))
        _check_file(got, 16, 3, 8, (("coop", "coop"), ("flip", "flip")))      # the default distance: min(L // 2, 32)


# ---- refusals -----------------------------------------------------------------------------------------------------------
def test_errors(monkeypatch):
    _force(monkeypatch)
    L = 10
    eng = _plane_engine(L, 2)
    try:
        lib, ctx = eng.lib, eng.ctx
        D = L // 2
        width = (D + 1) * (2 * D + 1)
        words = ctypes.c_int64()
        assert lib.spgg_pair_map_workspace(ctx, D, ctypes.byref(words)) == _lib.OK and words.value == K.plane_words(L, D)
        assert lib.spgg_pair_map_workspace(ctx, D + 1, ctypes.byref(words)) == _lib.E_ARG
        assert lib.spgg_pair_map_workspace(ctx, 0, ctypes.byref(words)) == _lib.OK and words.value == K.plane_words(L, 0)
        out = torch.full((2, width), -7, dtype=torch.int32, device=eng.dev)
        ws = torch.full((2, K.plane_words(L, D)), -7, dtype=torch.int32, device=eng.dev)
        call = lambda t=1, a=0, b=0, d=D, w=ws.data_ptr(), o=out.data_ptr(), stride=width: lib.spgg_pair_map(  # noqa: E731
            ctx, t, a, b, d, w, o, stride, eng.stream)
        assert call(t=0) == _lib.E_ARG and b"spgg_pair_map" in lib.spgg_last_error(ctx)
        for bad in (dict(a=-1), dict(a=2), dict(b=2), dict(b=-1)):
            assert call(**bad) == _lib.E_ARG and b"table" in lib.spgg_last_error(ctx), bad
        assert call(d=-1) == _lib.E_ARG and call(d=D + 1) == _lib.E_ARG and b"L / 2" in lib.spgg_last_error(ctx)
        assert call(w=None) == _lib.E_ARG and call(o=None) == _lib.E_ARG
        assert call(stride=width - 1) == _lib.E_ARG and b"out_stride" in lib.spgg_last_error(ctx)
        torch.cuda.synchronize()
        assert np.all(out.cpu().numpy() == -7) and np.all(ws.cpu().numpy() == -7)        # nothing was enqueued
        for kw in (dict(pair_map_every=-1), dict(pair_map_every=2, pair_map_max_d=D + 1), dict(pair_map_every=2, pair_map_max_d=-1),
                   dict(pair_map_every=2, pair_map_fields=(("coop", "state"),)), dict(pair_map_every=2, pair_map_fields=())):
            with pytest.raises(ValueError):
                eng.run(snapshots=False, **kw)
            assert eng.t == 1
        assert eng._pair_map_ws is None and "pair_map" not in eng.records
        with pytest.raises(ValueError):
            eng.pair_map_histories()
        for bad in (dict(max_d=D + 1), dict(a="state"), dict(b="rep")):
            with pytest.raises(ValueError):
                eng.pair_map(0, **bad)
        assert call() == _lib.OK
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy(), np.full((2, width), L * L))             # all-C planes: every count is n
    finally:
        eng.close()
    lib = _lib.load()
    cfg = _lib.Config(device=0, n_rep=1, L=8, second_order=0, state_mode=0, rng_mode=_lib.RNG_PHILOX, iterations=4,
                      rep_int8=0, algorithm=0, batch_reps=1)
    ctx = ctypes.c_void_p()      # before bind
    _lib.check(lib.spgg_create(ctypes.byref(ctx), cfg), None, "spgg_create")
    try:
        assert lib.spgg_pair_map(ctx, 1, 0, 0, 0, 8, 8, 1, None) == _lib.E_STATE
    finally:
        lib.spgg_destroy(ctx)


def test_work_above_the_cap_is_refused_and_enqueues_nothing(monkeypatch):
    """One replica of the smallest side (in hundreds) whose whole half-plane lies above the cap by pairmap.work: a fault
    of the refusal shows only at that size.  D = 3 on the same context is served."""
    _force(monkeypatch)
    L = next(s for s in range(100, 32768, 100) if PM.work(s, 1, s // 2) > PM.WORK_CAP)
    D = L // 2
    assert PM.work(L, 1, D) > PM.WORK_CAP >= PM.work(L, 1, 3) and L <= 6000
    eng = _plane_engine(L, 1, T=2)
    try:
        lib, ctx = eng.lib, eng.ctx
        out = torch.full((1, 8), -7, dtype=torch.int32, device=eng.dev)
        ws = torch.full((1, 8), -7, dtype=torch.int32, device=eng.dev)
        rc = lib.spgg_pair_map(ctx, 1, 0, 0, D, ws.data_ptr(), out.data_ptr(), (D + 1) * (2 * D + 1), eng.stream)
        assert rc == _lib.E_ARG and b"cap" in lib.spgg_last_error(ctx)
        torch.cuda.synchronize()
        assert np.all(out.cpu().numpy() == -7) and np.all(ws.cpu().numpy() == -7)
        with pytest.raises(ValueError, match="cap"):
            eng.run(snapshots=False, pair_map_every=1, pair_map_max_d=D)
        with pytest.raises(ValueError, match="cap"):
            eng.pair_map(0, max_d=D)
        assert eng.t == 1 and eng._pair_map_ws is None and "pair_map" not in eng.records
        m = eng.pair_map(0, max_d=3)
        assert np.array_equal(m, np.full((4, 7), L * L))
    finally:
        eng.close()
