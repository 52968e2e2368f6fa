"""What the device reputation record costs (profiles/reputation/README.txt).

    python tools/reputation_cost.py [--repeats 5] [--iters 10000] [--legs hist,pairs,host,run]

Every variant runs in a fresh process (this driver never touches the GPU) and reports the
median of its repeats:
  hist   device time of one spgg_reputation_hist round (20 bins, the reference's edges) over every
         replica (HIP events over 100 rounds) at cfg3's, cfg4's and cfg5's shapes
  pairs  the same for spgg_reputation_pairs, max_d = 100 at L = 200 and 500 at L = 1000
  host   both by the host path: copies of the S and R planes, np.histogram per strategy and
         engine.host_reputation_pair_sums (np.roll)
  run    the whole cfg3 run (BatchEngine.run, MT19937, as bench.full_run times it) with
         reputation_every in {0, 16, 1}, 20 bins, max_d = 100
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MAX_D = {"cfg3": 100, "cfg4": 100, "cfg5": 500}
BINS = 20


def _engine_at(config, t, T, rng="philox"):
    import torch
    import bench
    from spgg_amd.engine import BatchEngine
    _desc, L, M2, state, reps = bench.workload(config, 0)
    eng = BatchEngine(L, T, reps, use_second_order=M2, state_representation=state, rng=rng)
    eng.step(t)
    eng.flush()
    torch.cuda.synchronize()
    eng.all_stopped()
    return eng


def _timed_rounds(eng, a, call):
    import torch
    cur = torch.cuda.current_stream(eng.dev)
    rounds, out = 100, []
    for _ in range(a.repeats + 1):   # (the first repeat warms up)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(cur)
        for _ in range(rounds):
            for g in eng.groups:   # every group on one stream: the kernels' own time
                rc = call(g, cur.cuda_stream)
                assert rc == 0, rc
        e1.record(cur)
        e1.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3 / rounds)
    return out[1:]


def leg_hist(a):
    import torch
    eng = _engine_at(a.variant, 200, 300)
    try:
        edges = eng._reputation_edges(BINS)
        out_buf = torch.zeros((eng.R, 2 * BINS), dtype=torch.int32, device=eng.dev)
        us = _timed_rounds(eng, a, lambda g, s: eng.lib.spgg_reputation_hist(
            g["ctx"], eng.t, BINS, edges[g["r0"]].data_ptr(), out_buf[g["r0"]].data_ptr(), 2 * BINS, s))
        assert (out_buf.cpu().numpy().sum(axis=1) == eng.L * eng.L).all()   # every cell lies within R_min .. R_max
        return {"leg": "hist", "variant": a.variant, "L": eng.L, "bins": BINS, "replicas": eng.R, "groups": eng.G,
                "int8": bool(eng.rep_int8), "us_per_round": us}
    finally:
        eng.close()


def leg_pairs(a):
    import torch
    D = MAX_D[a.variant]
    eng = _engine_at(a.variant, 200, 300)
    try:
        width = 2 * (D + 1) + 1
        out_buf = torch.zeros((eng.R, width), dtype=torch.int64, device=eng.dev)
        us = _timed_rounds(eng, a, lambda g, s: eng.lib.spgg_reputation_pairs(
            g["ctx"], eng.t, D, out_buf[g["r0"]].data_ptr(), width, s))
        got = out_buf.cpu().numpy()
        assert (got[:, 1] == got[:, D + 2]).all()   # rows[0] == cols[0]
        return {"leg": "pairs", "variant": a.variant, "L": eng.L, "max_d": D, "replicas": eng.R, "groups": eng.G,
                "us_per_round": us}
    finally:
        eng.close()


def leg_host(a):
    import numpy as np
    from spgg_amd.engine import host_reputation_pair_sums
    D = MAX_D[a.variant]
    eng = _engine_at(a.variant, 200, 300)
    try:
        dev_hist = [eng.reputation_histogram(k, BINS) for k in range(eng.R)]
        dev_pairs = [eng.reputation_pair_sums(k, D) for k in range(eng.R)]
        t_hist, t_pairs = [], []
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            S = [eng.S[b].cpu().numpy().reshape(eng.R, eng.L, eng.L) for b in (0, 1)]
            Rp = [eng.Rep[b].cpu().numpy().reshape(eng.R, eng.L, eng.L) for b in (0, 1)]
            t1 = time.perf_counter()
            hists, pairs = [], []
            for k in range(eng.R):
                s = int(eng.stopped[k])   # the plane final_state reads
                b = (s - 1) & 1 if s else (eng.t - 1) & 1
                p = eng.reps[k]
                x, coop = Rp[b][k] * eng.rep_units[k], (S[b][k] & 1) == 0
                hists.append(np.stack([np.histogram(x[coop], bins=BINS, range=(p.R_min, p.R_max))[0],
                                       np.histogram(x[~coop], bins=BINS, range=(p.R_min, p.R_max))[0]]))
            t2 = time.perf_counter()
            for k in range(eng.R):
                s = int(eng.stopped[k])
                pairs.append(host_reputation_pair_sums(Rp[(s - 1) & 1 if s else (eng.t - 1) & 1][k], D))
            t3 = time.perf_counter()
            t_hist.append((t1 - t0) + (t2 - t1))
            t_pairs.append((t1 - t0) + (t3 - t2))
        same = all((h == d).all() for h, d in zip(hists, dev_hist)) and all(
            int(h[0]) == d[0] and (h[1] == d[1]).all() and (h[2] == d[2]).all() for h, d in zip(pairs, dev_pairs))
        return {"leg": "host", "variant": a.variant, "L": eng.L, "max_d": D, "replicas": eng.R,
                "equals_device": bool(same), "hist_seconds": t_hist, "seconds": t_pairs}
    finally:
        eng.close()


def leg_run(a):
    import torch
    import bench
    from spgg_amd.engine import BatchEngine
    every = int(a.variant)
    _desc, L, M2, state, reps = bench.workload("cfg3", 0)
    out = []
    for _ in range(a.repeats + 1):
        eng = BatchEngine(L, a.iters, reps, use_second_order=M2, state_representation=state, rng="mt19937")
        try:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            eng.run(snapshots=False, reputation_every=every, reputation_bins=BINS,
                    reputation_max_d=MAX_D["cfg3"] if every else None)
            torch.cuda.synchronize()
            out.append(time.perf_counter() - t0)
        finally:
            eng.close()
    return {"leg": "run", "variant": a.variant, "iterations": a.iters, "max_d": MAX_D["cfg3"], "seconds": out[1:]}


LEGS = {"hist": (leg_hist, ["cfg3", "cfg4", "cfg5"]),
        "pairs": (leg_pairs, ["cfg3", "cfg4", "cfg5"]),
        "host": (leg_host, ["cfg3", "cfg4", "cfg5"]),
        "run": (leg_run, ["0", "16", "1"])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10000)
    ap.add_argument("--legs", default="hist,pairs,host,run")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--variant", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        print("RESULT " + json.dumps(LEGS[a.child][0](a)), flush=True)
        return 0
    for leg in a.legs.split(","):
        for variant in LEGS[leg][1]:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", leg, "--variant", variant,
                                "--repeats", str(a.repeats), "--iters", str(a.iters)],
                               capture_output=True, text=True, timeout=600)
            line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
            if r.returncode or not line:
                print(f"{leg} {variant}: failed rc={r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}", flush=True)
                return 1   # nothing more is started after a failed leg
            d = json.loads(line[0][7:])
            for key, unit in (("us_per_round", "us"), ("hist_seconds", "s (hist)"), ("seconds", "s")):
                vals = d.get(key)
                if not vals:
                    continue
                print(f"{leg:5s} {variant:6s} median {statistics.median(vals):.6g} {unit}  "
                      f"min {min(vals):.6g} max {max(vals):.6g}  n={len(vals)}  "
                      + " ".join(f"{k}={v}" for k, v in d.items()
                                 if k not in ("seconds", "hist_seconds", "us_per_round", "leg", "variant")),
                      flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
