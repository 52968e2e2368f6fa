"""What the device cluster labelling costs (profiles/clusters/README.txt).

    python tools/cluster_cost.py [--repeats 5] [--iters 10000] [--legs final,call,run]

Every variant runs in a fresh process (this driver never touches the GPU) and reports the
median of its repeats:
  final  the final cluster sizes of the cfg3 batch (105 x L=200) at t ~ 500: the device path
         (spgg_clusters + compaction of the size planes on the device + copy) against the host
         path it replaces (copy of each replica's S + scipy.ndimage.label)
  call   device time of one spgg_clusters round over every replica (HIP events over 100 rounds)
         at cfg3's and cfg4's shapes: record only / with the size planes, walls / periodic
  run    the whole cfg3 run (BatchEngine.run, MT19937, as bench.full_run times it) with
         clusters_every in {0, 1, 16}
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


def leg_final(a):
    import torch
    from spgg_amd import spgg
    eng = _engine_at("cfg3", 500, 600)
    try:
        out = []
        for _ in range(a.repeats + 1):   # (the first repeat warms up: allocation, scipy import)
            eng._cl_cache = {}
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if a.variant == "device":
                n = sum(len(eng.cluster_sizes(k)) for k in range(eng.R))
            else:
                n = 0
                for k in range(eng.R):
                    s = int(eng.stopped[k])   # the plane final_state reads
                    S = (eng.S[(s - 1) & 1 if s else (eng.t - 1) & 1, k].cpu().numpy() & 1).reshape(eng.L, eng.L)
                    n += len(spgg.cluster_sizes(S))
            out.append(time.perf_counter() - t0)
        return {"leg": "final", "variant": a.variant, "replicas": eng.R, "clusters": n, "seconds": out[1:]}
    finally:
        eng.close()


def leg_call(a):
    import torch
    config, sizes, periodic = a.variant.split(":")
    eng = _engine_at(config, 500, 600)
    try:
        eng.cluster_sizes(0)   # allocates the size planes and the record
        cur = torch.cuda.current_stream(eng.dev)
        rounds, out = 100, []
        for _ in range(a.repeats + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(cur)
            for _ in range(rounds):
                for g in eng.groups:   # every group on one stream: the kernels' own time
                    r0 = g["r0"]
                    rc = eng.lib.spgg_clusters(g["ctx"], eng.t, int(periodic),
                                               eng._cl_sizes[r0].data_ptr() if sizes == "sizes" else None,
                                               eng._cl_final[r0].data_ptr(), 3, cur.cuda_stream)
                    assert rc == 0, rc
            e1.record(cur)
            e1.synchronize()
            out.append(e0.elapsed_time(e1) * 1e3 / rounds)
        return {"leg": "call", "variant": a.variant, "replicas": eng.R, "groups": eng.G,
                "us_per_round": out[1:]}
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
            eng.run(snapshots=False, clusters_every=every)
            torch.cuda.synchronize()
            out.append(time.perf_counter() - t0)
            if every:
                eng.cluster_histories()   # (raises on a capped labelling)
        finally:
            eng.close()
    return {"leg": "run", "variant": a.variant, "iterations": a.iters, "seconds": out[1:]}


LEGS = {"final": (leg_final, ["device", "host"]),
        "call": (leg_call, [f"{c}:{s}:{p}" for c in ("cfg3", "cfg4") for s in ("record", "sizes") for p in (0, 1)]),
        "run": (leg_run, ["0", "1", "16"])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10000)
    ap.add_argument("--legs", default="final,call,run")
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
            print(f"{leg:5s} {variant:16s} median {statistics.median(vals):.6g} {unit}  "
                  f"min {min(vals):.6g} max {max(vals):.6g}  n={len(vals)}  "
                  + " ".join(f"{k}={v}" for k, v in d.items() if k not in ("seconds", "us_per_round", "leg", "variant")),
                  flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
