"""bench.py --dump-outputs on the GPU: the files hold the state a caller of the timed path receives
(every replica's S, R, Q after warmup + steps iterations, flushed), equal to what BatchEngine.run
of the same replicas returns, identical from run to run, float32 / float64, within the size limit."""
import json
import os

import numpy as np
import pytest

import bench  # noqa: E402  (repository root)
from spgg_amd.engine import BatchEngine

pytestmark = pytest.mark.gpu
NAMES = {"S", "R", "Q", "coop_trace", "coop_final", "stop_iter"}


def _dump(tmp_path, name, argv, capsys):
    d = tmp_path / name
    bench.main(["--gpus", "1", *argv, "--dump-outputs", str(d)])
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert {f[:-4] for f in os.listdir(d)} == NAMES
    arrays = {n: np.load(d / f"{n}.npy") for n in NAMES}
    assert all(a.dtype in (np.float32, np.float64) for a in arrays.values())
    assert sum(a.nbytes for a in arrays.values()) <= 64 * 10 ** 6
    return line, arrays


def test_dump_is_the_engines_final_state_and_repeats(tmp_path, capsys):
    argv = ["--config", "cfg4", "--steps", "4", "--warmup", "3"]
    line, a = _dump(tmp_path, "a", argv, capsys)
    _, b = _dump(tmp_path, "b", argv, capsys)
    for n in NAMES:
        assert np.array_equal(a[n], b[n]), n
    _, L, M2, state, reps = bench.workload("cfg4", 0)
    eng = BatchEngine(L, 7, reps, use_second_order=M2, state_representation=state, rng="philox")
    try:
        eng.run(snapshots=False)
        fin = [eng.final_state(k) for k in range(len(reps))]
        ncoop = eng.stats_folded()[:, :, 0].cpu().numpy()
    finally:
        eng.close()
    assert a["S"].shape == (8, L, L) and a["Q"].shape == (8, L, L, 2, 2)
    assert np.array_equal(a["S"], np.stack([f[2] for f in fin]))
    assert np.array_equal(a["R"], np.stack([f[1] for f in fin]))
    assert np.array_equal(a["Q"], np.stack([f[0] for f in fin]))
    assert np.array_equal(a["stop_iter"], np.zeros(8))
    assert np.array_equal(a["coop_trace"], ncoop[:, 4:8] / (L * L))     # iterations 4-7
    assert abs(a["coop_final"].mean() - line["gather"]["mean_final_coop"]) < 1e-15
    # and the dump is the oracle's state under the same Philox draws (oracle/philox.py)
    from tests._philox import check_final, philox_oracle
    for k in (0, 7):
        _, want = philox_oracle(L, 7, reps[k], k, M2, state)
        check_final((a["Q"][k], a["R"][k], a["S"][k]), want, k)


def test_large_outputs_are_a_fixed_sample(tmp_path, capsys):
    """cfg3's R and Q (105 x 200 x 200 agents) exceed the per-array limit: a seeded sample of the
    flattened array, the same elements in every run."""
    _, a = _dump(tmp_path, "c", ["--steps", "2", "--warmup", "1"], capsys)
    n = bench.DUMP_ARRAY_BYTES // 8
    assert a["S"].shape == (105, 200, 200) and a["R"].shape == (n,) and a["Q"].shape == (n,)
    idx = np.sort(np.random.RandomState(bench.DUMP_SAMPLE_SEED).choice(105 * 200 * 200, n, replace=False))
    _, L, M2, state, reps = bench.workload("cfg3", 0)
    eng = BatchEngine(L, 3, reps, use_second_order=M2, state_representation=state, rng="philox")
    try:
        eng.run(snapshots=False)
        fin = {k: eng.final_state(k) for k in (0, 52, 104)}
    finally:
        eng.close()
    for k, (Q, R, S) in fin.items():
        sel = (idx >= k * L * L) & (idx < (k + 1) * L * L)      # the sample's elements of replica k
        assert sel.sum() > 0.9 * n / 105
        assert np.array_equal(a["R"][sel], R.reshape(-1)[idx[sel] - k * L * L])
        assert np.array_equal(a["S"][k], S)
