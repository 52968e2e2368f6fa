"""bench.py's run shapes on CPU, with BatchEngine and the device clock stubbed: a plain run makes
one engine, times --steps iterations after --warmup and prints the headline line alone; --full
adds the legs that take runs of their own (here the MT19937 and the steady window)."""
import json
import time

import pytest
import torch


class _Event:
    def __init__(self, enable_timing=False):
        self.t = None

    def record(self, stream=None):
        self.t = time.perf_counter()

    def elapsed_time(self, other):
        return (other.t - self.t) * 1e3


@pytest.fixture
def fake_bench(monkeypatch):
    import bench
    from spgg_amd import _lib as C
    from spgg_amd import engine as E
    made, steps = [], []

    class FakeEngine:
        """BatchEngine's surface as bench.window uses it."""

        def __init__(self, L, iterations, replicas, rng="mt19937", **kw):
            self.R = len(replicas)
            self.resident = self.G = self.waves = 1
            self.persistent = False
            self.mt_layout = (1, 1)
            self.stop_iter = torch.zeros(self.R, dtype=torch.int32)
            self.st = torch.zeros((self.R, iterations + 2, C.NSTAT), dtype=torch.float64)
            made.append((rng, iterations))

        def launch_streams(self):
            return [None]

        def step(self, n, ordered=True):
            time.sleep(1e-3)
            steps.append(n)

        def stats_folded(self):
            return self.st

        def check_status(self):
            pass

        def close(self):
            pass

    monkeypatch.setattr(torch.cuda, "set_device", lambda d: None)
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: None)
    monkeypatch.setattr(torch.cuda, "Event", _Event)
    monkeypatch.setattr(E, "BatchEngine", FakeEngine)
    monkeypatch.setenv("SPGG_DIST_BACKEND", "gloo")   # the line's sums on host tensors
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    return bench, made, steps


MOVED = ("steady_window", "mt19937", "full_run", "cpu_baseline")


def test_plain_run_is_the_timed_window_alone(fake_bench, capsys):
    bench, made, steps = fake_bench
    bench.main(["--gpus", "1", "--config", "cfg2", "--steps", "7", "--warmup", "3"])
    out = capsys.readouterr().out.strip().splitlines()
    assert len(out) == 1
    line = json.loads(out[0])
    assert made == [("philox", 10)] and steps == [3, 7]     # one engine: W untimed, K timed
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in line, k
    assert line["steps"] == 7 and line["warmup"] == 3 and line["higher_is_better"] is True
    assert line["unit"] == "agent-steps/s" and line["dtype"] == "f64"
    # value = the K steps' agent-steps over their wall time; ms_per_step = that time per step
    assert abs(line["value"] - 7 * 200 * 200 / (line["ms_per_step"] * 7 / 1e3)) <= 1e-9 * line["value"]
    assert line["ms_per_step"] * 7 >= 1.0
    assert not [k for k in MOVED if k in line]


def test_full_adds_the_other_legs(fake_bench, capsys):
    bench, made, steps = fake_bench
    bench.main(["--gpus", "1", "--config", "cfg2", "--steps", "7", "--warmup", "3", "--full",
                "--no-cpu-baseline", "--full-run", "0"])
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert made == [("philox", 10), ("mt19937", 10), ("philox", 600)]
    assert steps == [3, 7, 3, 7, 400, 200]
    assert line["steps"] == 7 and line["steady_window"]["window"] == "iterations 401-600"
    assert line["mt19937"]["ms_per_step"] > 0
    assert "full_run" not in line and "cpu_baseline" not in line   # switched off above
