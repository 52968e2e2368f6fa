"""What the device pair counts cost (profiles/correlations/README.txt).

    python tools/correlation_cost.py [--repeats 5] [--iters 10000] [--legs call,host,run]

Every variant runs in a fresh process (this driver never touches the GPU) and reports the
median of its repeats:
  call   device time of one spgg_correlations round over every replica (HIP events over 100
         rounds) at cfg3's, cfg4's (max_d = 100) and cfg5's (max_d = 500) shapes
  host   the same counts by engine.host_pair_counts on host copies of the planes (np.roll)
  run    the whole cfg3 run (BatchEngine.run, MT19937, as bench.full_run times it) with
         correlations_every in {0, 16, 1}, max_d = 100
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


def leg_call(a):
    import torch
    D = MAX_D[a.variant]
    eng = _engine_at(a.variant, 200, 300)
    try:
        out_buf = torch.zeros((eng.R, 2 * (D + 1)), dtype=torch.int32, device=eng.dev)
        cur = torch.cuda.current_stream(eng.dev)
        rounds, out = 100, []
        for _ in range(a.repeats + 1):   # (the first repeat warms up)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(cur)
            for _ in range(rounds):
                for g in eng.groups:   # every group on one stream: the kernels' own time
                    rc = eng.lib.spgg_correlations(g["ctx"], eng.t, D, out_buf[g["r0"]].data_ptr(), 2 * (D + 1),
                                                   cur.cuda_stream)
                    assert rc == 0, rc
            e1.record(cur)
            e1.synchronize()
            out.append(e0.elapsed_time(e1) * 1e3 / rounds)
        got = out_buf.cpu().numpy()
        assert (got[:, 0] == got[:, D + 1]).all()   # rows[0] == cols[0]
        return {"leg": "call", "variant": a.variant, "L": eng.L, "max_d": D, "replicas": eng.R, "groups": eng.G,
                "us_per_round": out[1:]}
    finally:
        eng.close()


def leg_host(a):
    from spgg_amd.engine import host_pair_counts
    D = MAX_D[a.variant]
    eng = _engine_at(a.variant, 200, 300)
    try:
        device = [eng.pair_counts(k, D) for k in range(eng.R)]
        out = []
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            S = [eng.S[b].cpu().numpy().reshape(eng.R, eng.L, eng.L) for b in (0, 1)]
            host = []
            for k in range(eng.R):
                s = int(eng.stopped[k])   # the plane final_state reads
                host.append(host_pair_counts(S[(s - 1) & 1 if s else (eng.t - 1) & 1][k], D))
            out.append(time.perf_counter() - t0)
        same = all((h == d).all() for h, d in zip(host, device))
        return {"leg": "host", "variant": a.variant, "L": eng.L, "max_d": D, "replicas": eng.R,
                "equals_device": bool(same), "seconds": out}
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
            eng.run(snapshots=False, correlations_every=every, correlations_max_d=MAX_D["cfg3"])
            torch.cuda.synchronize()
            out.append(time.perf_counter() - t0)
        finally:
            eng.close()
    return {"leg": "run", "variant": a.variant, "iterations": a.iters, "max_d": MAX_D["cfg3"], "seconds": out[1:]}


LEGS = {"call": (leg_call, ["cfg3", "cfg4", "cfg5"]),
        "host": (leg_host, ["cfg3", "cfg4", "cfg5"]),
        "run": (leg_run, ["0", "16", "1"])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10000)
    ap.add_argument("--legs", default="call,host,run")
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
            vals = d.get("seconds") or d.get("us_per_round")
            unit = "s" if "seconds" in d else "us"
            print(f"{leg:5s} {variant:6s} median {statistics.median(vals):.6g} {unit}  "
                  f"min {min(vals):.6g} max {max(vals):.6g}  n={len(vals)}  "
                  + " ".join(f"{k}={v}" for k, v in d.items() if k not in ("seconds", "us_per_round", "leg", "variant")),
                  flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
