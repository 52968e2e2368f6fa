"""What the device records cost (profiles/{clusters,correlations,reputation,dwell,policy,payoff,pair_map}/README.txt).

    python tools/record_cost.py --record clusters|correlations|reputation|dwell|policy|payoff|pair_map [--repeats 5] [--iters 10000]
                                [--legs LEG,LEG,...]

Every variant runs in a fresh process (this driver never touches the GPU) and reports the median of
its repeats.  Legs (default: all of the record's, in this order):
  clusters      final  the final cluster sizes of the cfg3 batch (105 x L=200) at t ~ 500: the device
                       path (spgg_clusters + compaction of the size planes on the device + copy)
                       against the host path it replaces (copy of each replica's S + scipy label)
                call   device time of one spgg_clusters round over every replica (HIP events over 100
                       rounds) at cfg3's and cfg4's shapes: record only / with the size planes,
                       walls / periodic
                tiled  the same for one spgg_clusters_tiled round (five launches): variant
                       CONFIG:TILE:record|sizes, TILE a tile side, 0 for the library's or "lds" for the
                       one-workgroup spgg_clusters in the same session (cfg3 / cfg4 only); cfg5 sweeps the
                       tile sides that settle the library's
                host5  the host path cfg5 (1 x L=1000) had before: copy of S + scipy label + bincount
                run5   the whole cfg5 run (BatchEngine.run, MT19937) with clusters_every 0 / 256 / 16,
                       clusters_tiled=True
  correlations  call   the same for spgg_correlations at cfg3's, cfg4's (max_d = 100) and cfg5's
                       (max_d = 500) shapes
                host   the same counts by engine.host_pair_counts on host copies of the planes
  reputation    hist   the same for spgg_reputation_hist (20 bins, the reference's edges)
                pairs  the same for spgg_reputation_pairs, max_d as for correlations
                host   both by the host path: copies of the S and R planes, np.histogram per strategy
                       and engine.host_reputation_pair_sums (np.roll)
  dwell         run    the whole run (BatchEngine.run, MT19937) of cfg3, cfg4 and cfg5 with dwell_every
                       0 / 256 / 16, and the first 400 iterations alone (large eps: about half the agents
                       flip per iteration); variant CONFIG:EVERY:ITERATIONS
                launch device time per iteration of step(100) (HIP events on the current stream) without
                       and with the dwell launch armed, in one process, after 20 and after 400
                       iterations: the difference is the dwell launch's own cost; variant CONFIG:T
                record device time of one spgg_dwell_record round / one spgg_dwell_fields round
  policy        call   device time of one spgg_policy round (three launches: zero, policy, bonds; 32 bins)
                       at cfg3's, cfg4's and cfg5's shapes after 200 iterations, the table in place still
                       without its pending term (the in-run case: the term is rebuilt) and flushed; the
                       fraction of the byte floor at 8 TB/s; variant CONFIG:pending|flushed
                run    the whole run (BatchEngine.run, MT19937) of cfg3, cfg4 and cfg5 with policy_every
                       0 / 100 / 10 / 1; variant CONFIG:EVERY:ITERATIONS
  payoff        census device time of one spgg_payoff_census round (two launches: zero, census with the plane)
                       at cfg3's, cfg4's and cfg5's shapes after 200 iterations; the fraction of the byte floor
                       (1 B read, 1 B written per agent) at 8 TB/s
                pairs  the same for one spgg_payoff_pairs round on the plane that census wrote, max_d as for
                       correlations
                run    the whole run (BatchEngine.run, MT19937) of cfg3, cfg4 and cfg5 with payoff_every
                       0 / 100 / 10 / 1 (max_d as above where armed); variant CONFIG:EVERY:ITERATIONS
  pair_map      call   device time of one spgg_pair_map round (two launches: pack, count) at cfg3's, cfg4's and
                       cfg5's shapes after 200 iterations, at D = 32 and D = L // 2, for the cooperator auto-map
                       alone (cc) and for cc + ff + cf; the work in word blocks and the rate; variant
                       CONFIG:D:cc|all
                run    the whole cfg3 run (BatchEngine.run, MT19937) with pair_map_every 0 / 100 / 10 at D = 32;
                       variant cfg3:EVERY:ITERATIONS
                host   the same maps by pairmap.host_pair_map (np.roll) on host copies of the planes, the copy
                       included, at D = 32, and by pairmap.host_pair_map_fft at D = L // 2; variant CONFIG:D:roll|fft
  every other   run    the whole cfg3 run (BatchEngine.run, MT19937, as bench.full_run times it) with
                       the record every {0, 16, 1} iterations (max_d = 100, 20 bins)
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
SHAPES = ["cfg3", "cfg4", "cfg5"]


def _engine_at(config, t, T, rng="philox", flush=True):
    import torch
    import bench
    from spgg_amd.engine import BatchEngine
    _desc, L, M2, state, reps = bench.workload(config, 0)
    eng = BatchEngine(L, T, reps, use_second_order=M2, state_representation=state, rng=rng)
    eng.step(t)
    if flush:
        eng.flush()
    torch.cuda.synchronize()
    eng.all_stopped()
    return eng


def _timed_rounds(eng, a, call):
    """us per round of call(group, stream) over every group on one stream: the kernels' own time."""
    import torch
    cur = torch.cuda.current_stream(eng.dev)
    rounds, out = 100, []
    for _ in range(a.repeats + 1):   # (the first repeat warms up)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(cur)
        for _ in range(rounds):
            for g in eng.groups:
                rc = call(g, cur.cuda_stream)
                assert rc == 0, rc
        e1.record(cur)
        e1.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3 / rounds)
    return out[1:]


def _final_planes(eng, buf):
    """(R, L, L) host copies of the plane of `buf` (eng.S / eng.Rep) that final_state reads, per replica."""
    planes = [buf[b].cpu().numpy().reshape(eng.R, eng.L, eng.L) for b in (0, 1)]
    stop = [int(s) for s in eng.stopped]
    return [planes[(s - 1) & 1 if s else (eng.t - 1) & 1][k] for k, s in enumerate(stop)]


def leg_final(a):
    import torch
    from spgg_amd import spgg
    eng = _engine_at("cfg3", 500, 600)
    try:
        out = []
        for _ in range(a.repeats + 1):   # (the first repeat warms up: allocation, scipy import)
            eng.step(1)                  # one more iteration: the engine forgets its cached sizes
            torch.cuda.synchronize()
            eng.all_stopped()
            t0 = time.perf_counter()
            if a.variant == "device":
                n = sum(len(eng.cluster_sizes(k)) for k in range(eng.R))
            else:
                n = sum(len(spgg.cluster_sizes(S & 1)) for S in _final_planes(eng, eng.S))
            out.append(time.perf_counter() - t0)
        return {"leg": "final", "variant": a.variant, "replicas": eng.R, "clusters": n, "seconds": out[1:]}
    finally:
        eng.close()


def leg_call(a):
    import numpy as np
    import torch
    if a.record == "clusters":
        config, sizes, periodic = a.variant.split(":")
    else:
        config = a.variant
    D = MAX_D[config]
    eng = _engine_at(config, *((500, 600) if a.record == "clusters" else (200, 300)))
    try:
        def buf(width, dtype=torch.int32):
            return torch.zeros((eng.R, width), dtype=dtype, device=eng.dev)
        info = {} if a.record == "clusters" else {"L": eng.L}
        if a.record == "clusters":
            out_buf, planes = buf(3), buf(eng.n) if sizes == "sizes" else None
            us = _timed_rounds(eng, a, lambda g, s: eng.lib.spgg_clusters(
                g["ctx"], eng.t, int(periodic), planes[g["r0"]].data_ptr() if planes is not None else None,
                out_buf[g["r0"]].data_ptr(), 3, s))
        elif a.record == "correlations":
            out_buf = buf(2 * (D + 1))
            us = _timed_rounds(eng, a, lambda g, s: eng.lib.spgg_correlations(
                g["ctx"], eng.t, D, out_buf[g["r0"]].data_ptr(), 2 * (D + 1), s))
            got = out_buf.cpu().numpy()
            assert (got[:, 0] == got[:, D + 1]).all()   # rows[0] == cols[0]
            info["max_d"] = D
        elif a.child == "hist":
            from spgg_amd.engine import reputation_bin_edges
            edges = torch.from_numpy(np.stack([reputation_bin_edges(p.R_min, p.R_max, BINS) for p in eng.reps])).to(eng.dev)
            out_buf = buf(2 * BINS)
            us = _timed_rounds(eng, a, lambda g, s: eng.lib.spgg_reputation_hist(
                g["ctx"], eng.t, BINS, edges[g["r0"]].data_ptr(), out_buf[g["r0"]].data_ptr(), 2 * BINS, s))
            assert (out_buf.cpu().numpy().sum(axis=1) == eng.L * eng.L).all()   # every cell lies within R_min .. R_max
            info.update(bins=BINS, int8=bool(eng.rep_int8))
        else:
            width = 2 * (D + 1) + 1
            out_buf = buf(width, torch.int64)
            us = _timed_rounds(eng, a, lambda g, s: eng.lib.spgg_reputation_pairs(
                g["ctx"], eng.t, D, out_buf[g["r0"]].data_ptr(), width, s))
            got = out_buf.cpu().numpy()
            assert (got[:, 1] == got[:, D + 2]).all()   # rows[0] == cols[0]
            info["max_d"] = D
        return {"leg": a.child, "variant": a.variant, **info, "replicas": eng.R, "groups": eng.G, "us_per_round": us}
    finally:
        eng.close()


def leg_tiled(a):
    import ctypes
    import torch
    config, tile, sizes = a.variant.split(":")
    eng = _engine_at(config, 500, 600)
    try:
        out_buf = torch.zeros((eng.R, 3), dtype=torch.int32, device=eng.dev)
        planes = torch.zeros((eng.R, eng.n), dtype=torch.int32, device=eng.dev) if sizes == "sizes" else None

        def plane_ptr(g):
            return planes[g["r0"]].data_ptr() if planes is not None else None
        if tile == "lds":
            us = _timed_rounds(eng, a, lambda g, s: eng.lib.spgg_clusters(
                g["ctx"], eng.t, 0, plane_ptr(g), out_buf[g["r0"]].data_ptr(), 3, s))
        else:
            words = ctypes.c_int64(0)
            assert eng.lib.spgg_clusters_tiled_workspace(eng.ctx, ctypes.byref(words)) == 0
            work = torch.empty((eng.R, words.value), dtype=torch.int32, device=eng.dev)
            us = _timed_rounds(eng, a, lambda g, s: eng.lib.spgg_clusters_tiled(
                g["ctx"], eng.t, 0, int(tile), work[g["r0"]].data_ptr(), plane_ptr(g), out_buf[g["r0"]].data_ptr(), 3, s))
        rec = out_buf.cpu().numpy()
        assert (rec[:, 0] >= 0).all(), rec   # no cap
        return {"leg": "tiled", "variant": a.variant, "L": eng.L, "replicas": eng.R, "groups": eng.G,
                "clusters": int(rec[:, 0].sum()), "largest": int(rec[:, 1].max()), "us_per_round": us}
    finally:
        eng.close()


def leg_host5(a):
    import torch
    from spgg_amd import spgg
    eng = _engine_at(a.variant, 500, 600)
    try:
        device = sum(len(eng.cluster_sizes(k)) for k in range(eng.R))   # (above side 200: the tiled path)
        out = []
        for _ in range(a.repeats + 1):   # (the first repeat warms up: the scipy import)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            n = sum(len(spgg.cluster_sizes(S & 1)) for S in _final_planes(eng, eng.S))
            out.append(time.perf_counter() - t0)
        return {"leg": "host5", "variant": a.variant, "L": eng.L, "replicas": eng.R, "clusters": n,
                "equals_device": n == device, "seconds": out[1:]}
    finally:
        eng.close()


def leg_run5(a):
    import torch
    import bench
    from spgg_amd.engine import BatchEngine
    every = int(a.variant)
    _desc, L, M2, state, reps = bench.workload("cfg5", 0)
    out = []
    for _ in range(a.repeats + 1):
        eng = BatchEngine(L, a.iters, reps, use_second_order=M2, state_representation=state, rng="mt19937")
        try:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            eng.run(snapshots=False, clusters_every=every, clusters_tiled=bool(every))
            torch.cuda.synchronize()
            out.append(time.perf_counter() - t0)
            executed = eng.t - 1
            if every:
                eng.cluster_histories()   # (raises on a capped labelling)
        finally:
            eng.close()
    return {"leg": "run5", "variant": a.variant, "iterations": executed, "L": L, "seconds": out[1:]}


def leg_host(a):
    import numpy as np
    from spgg_amd.engine import host_pair_counts, host_reputation_pair_sums
    D = MAX_D[a.variant]
    eng = _engine_at(a.variant, 200, 300)
    try:
        res = {"leg": "host", "variant": a.variant, "L": eng.L, "max_d": D, "replicas": eng.R}
        if a.record == "correlations":
            device = [eng.pair_counts(k, D) for k in range(eng.R)]
            out = []
            for _ in range(a.repeats):
                t0 = time.perf_counter()
                host = [host_pair_counts(S, D) for S in _final_planes(eng, eng.S)]
                out.append(time.perf_counter() - t0)
            same = all((h == d).all() for h, d in zip(host, device))
            return {**res, "equals_device": bool(same), "seconds": out}
        dev_hist = [eng.reputation_histogram(k, BINS) for k in range(eng.R)]
        dev_pairs = [eng.reputation_pair_sums(k, D) for k in range(eng.R)]
        t_hist, t_pairs = [], []
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            S, Rp = _final_planes(eng, eng.S), _final_planes(eng, eng.Rep)
            t1 = time.perf_counter()
            hists = []
            for k, p in enumerate(eng.reps):
                x, coop = Rp[k] * eng.rep_units[k], (S[k] & 1) == 0
                hists.append(np.stack([np.histogram(x[coop], bins=BINS, range=(p.R_min, p.R_max))[0],
                                       np.histogram(x[~coop], bins=BINS, range=(p.R_min, p.R_max))[0]]))
            t2 = time.perf_counter()
            pairs = [host_reputation_pair_sums(Rp[k], D) for k in range(eng.R)]
            t3 = time.perf_counter()
            t_hist.append(t2 - t0)
            t_pairs.append((t1 - t0) + (t3 - t2))
        same = all((h == d).all() for h, d in zip(hists, dev_hist)) and all(
            int(h[0]) == d[0] and (h[1] == d[1]).all() and (h[2] == d[2]).all() for h, d in zip(pairs, dev_pairs))
        return {**res, "equals_device": bool(same), "hist_seconds": t_hist, "seconds": t_pairs}
    finally:
        eng.close()


def leg_run(a):
    import torch
    import bench
    from spgg_amd.engine import BatchEngine
    every = int(a.variant)
    run_kw = {"clusters": dict(clusters_every=every),
              "correlations": dict(correlations_every=every, correlations_max_d=MAX_D["cfg3"]),
              "reputation": dict(reputation_every=every, reputation_bins=BINS,
                                 reputation_max_d=MAX_D["cfg3"] if every else None)}[a.record]
    _desc, L, M2, state, reps = bench.workload("cfg3", 0)
    out = []
    for _ in range(a.repeats + 1):
        eng = BatchEngine(L, a.iters, reps, use_second_order=M2, state_representation=state, rng="mt19937")
        try:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            eng.run(snapshots=False, **run_kw)
            torch.cuda.synchronize()
            out.append(time.perf_counter() - t0)
            if every and a.record == "clusters":
                eng.cluster_histories()   # (raises on a capped labelling)
        finally:
            eng.close()
    info = {} if a.record == "clusters" else {"max_d": MAX_D["cfg3"]}
    return {"leg": "run", "variant": a.variant, "iterations": a.iters, **info, "seconds": out[1:]}


def leg_dwell_run(a):
    import torch
    import bench
    from spgg_amd.engine import BatchEngine
    config, every, iters = a.variant.split(":")
    _desc, L, M2, state, reps = bench.workload(config, 0)
    out = []
    for _ in range(a.repeats + 1):
        eng = BatchEngine(L, int(iters), reps, use_second_order=M2, state_representation=state, rng="mt19937")
        try:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            eng.run(snapshots=False, dwell_every=int(every))
            torch.cuda.synchronize()
            out.append(time.perf_counter() - t0)
            executed = eng.t - 1
        finally:
            eng.close()
    return {"leg": "run", "variant": a.variant, "iterations": executed, "replicas": len(reps), "L": L,
            "us_per_iter": [s / executed * 1e6 for s in out[1:]], "seconds": out[1:]}


def leg_dwell_launch(a):
    import torch
    config, t = a.variant.split(":")
    n_steps = 100
    eng = _engine_at(config, int(t), int(t) + 2 * (a.repeats + 1) * n_steps + 1)
    try:
        cur = torch.cuda.current_stream(eng.dev)

        def timed():
            out = []
            for _ in range(a.repeats + 1):   # (the first repeat warms up)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(cur)
                eng.step(n_steps)   # (ordered: the groups' streams start after e0 and e1 waits for them)
                e1.record(cur)
                e1.synchronize()
                out.append(e0.elapsed_time(e1) * 1e3 / n_steps)
            return out[1:]
        off = timed()
        eng.dwell_start()
        on = timed()
        flips = eng.dwell_record()[:, 5].sum() / (eng.R * eng.n * (a.repeats + 1) * n_steps)
        return {"leg": "launch", "variant": a.variant, "replicas": eng.R, "L": eng.L, "groups": eng.G,
                "flip_share": float(flips), "us_per_iter_off": off, "us_per_iter_on": on}
    finally:
        eng.close()


def leg_dwell_record(a):
    import torch
    config, what = a.variant.split(":")
    eng = _engine_at(config, 200, 300)
    try:
        eng.dwell_start()
        eng.step(20)
        torch.cuda.synchronize()
        fn, width, dtype = ((eng.lib.spgg_dwell_record, 61, torch.int64) if what == "record" else
                            (eng.lib.spgg_dwell_fields, 3 * eng.n, torch.int32))
        out_buf = torch.zeros((eng.R, width), dtype=dtype, device=eng.dev)
        us = _timed_rounds(eng, a, lambda g, s: fn(g["ctx"], eng.t, out_buf[g["r0"]].data_ptr(), width, s))
        return {"leg": "record", "variant": a.variant, "replicas": eng.R, "L": eng.L, "us_per_round": us}
    finally:
        eng.close()


POLICY_BINS = 32
FLOOR_BYTES_PER_SECOND = 8e12   # cache-resident reads as this project has measured them (7.4-8.6 TB/s)


def leg_policy_call(a):
    import torch
    from spgg_amd.policy import policy_width
    config, table = a.variant.split(":")
    eng = _engine_at(config, 200, 300, flush=table == "flushed")
    try:
        width = policy_width(POLICY_BINS)
        out_buf = torch.zeros((eng.R, width), dtype=torch.int32, device=eng.dev)
        edges, plane = eng._policy_edges(POLICY_BINS, (-2.0, 2.0)), eng._policy_plane()
        us = _timed_rounds(eng, a, lambda g, s: eng.lib.spgg_policy(
            g["ctx"], eng.t, POLICY_BINS, edges[g["r0"]].data_ptr(), plane[g["r0"]].data_ptr(),
            out_buf[g["r0"]].data_ptr(), width, s))
        got = out_buf.cpu().numpy()
        assert (got[:, :16].sum(axis=1) == eng.n).all() and (got[:, 16:21].sum(axis=1) == 2 * eng.n).all()
        live = int((eng.stopped == 0).sum())
        bytes_ = eng.R * eng.n * (eng.QW * 8 + 3)     # Q, the S byte, the plane byte written and read back
        floor_us = bytes_ / FLOOR_BYTES_PER_SECOND * 1e6
        return {"leg": "call", "variant": a.variant, "replicas": eng.R, "L": eng.L, "groups": eng.G, "live": live,
                "MB": round(bytes_ / 1e6, 1), "floor_us": round(floor_us, 2),
                "floor_fraction": [round(floor_us / u, 3) for u in us], "us_per_round": us}
    finally:
        eng.close()


def leg_policy_run(a):
    import torch
    import bench
    from spgg_amd.engine import BatchEngine
    config, every, iters = a.variant.split(":")
    _desc, L, M2, state, reps = bench.workload(config, 0)
    out = []
    for _ in range(a.repeats + 1):
        eng = BatchEngine(L, int(iters), reps, use_second_order=M2, state_representation=state, rng="mt19937")
        try:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            eng.run(snapshots=False, policy_every=int(every), policy_bins=POLICY_BINS)
            torch.cuda.synchronize()
            out.append(time.perf_counter() - t0)
            executed = eng.t - 1
        finally:
            eng.close()
    return {"leg": "run", "variant": a.variant, "iterations": executed, "replicas": len(reps), "L": L,
            "us_per_iter": [s / executed * 1e6 for s in out[1:]], "seconds": out[1:]}


def leg_payoff_call(a):
    import torch
    from spgg_amd.payoff import PAYOFF_SLOTS, pairs_width
    config = a.variant
    D = MAX_D[config]
    eng = _engine_at(config, 200, 300)
    try:
        plane = eng._payoff_plane()
        census = torch.zeros((eng.R, PAYOFF_SLOTS), dtype=torch.int32, device=eng.dev)

        def census_call(g, s):
            return eng.lib.spgg_payoff_census(g["ctx"], eng.t, plane[g["r0"]].data_ptr(), census[g["r0"]].data_ptr(),
                                              PAYOFF_SLOTS, s)
        info = {"L": eng.L, "replicas": eng.R, "groups": eng.G}
        if a.child == "census":
            us = _timed_rounds(eng, a, census_call)
            bytes_ = 2 * eng.R * eng.n
        else:
            for g in eng.groups:
                assert census_call(g, torch.cuda.current_stream(eng.dev).cuda_stream) == 0
            width = pairs_width(D)
            out_buf = torch.zeros((eng.R, width), dtype=torch.int64, device=eng.dev)
            us = _timed_rounds(eng, a, lambda g, s: eng.lib.spgg_payoff_pairs(
                g["ctx"], eng.t, D, plane[g["r0"]].data_ptr(), out_buf[g["r0"]].data_ptr(), width, s))
            got = out_buf.cpu().numpy()[:, 2:].reshape(eng.R, 2, D + 1, 3)
            assert (got[:, 0, 0] == got[:, 1, 0]).all()   # rows[0] == cols[0]
            bytes_ = eng.R * eng.n * 2 * (D + 1)           # the plane once per (direction, distance)
            info["max_d"] = D
        got = census.cpu().numpy()
        assert (got[:, :260].sum(axis=1) == eng.n).all() and (got[:, 260:].sum(axis=1) == 2 * eng.n).all()
        floor_us = bytes_ / FLOOR_BYTES_PER_SECOND * 1e6
        return {"leg": a.child, "variant": a.variant, **info, "MB": round(bytes_ / 1e6, 1), "floor_us": round(floor_us, 2),
                "floor_fraction": [round(floor_us / u, 3) for u in us], "us_per_round": us}
    finally:
        eng.close()


def leg_payoff_run(a):
    import torch
    import bench
    from spgg_amd.engine import BatchEngine
    config, every, iters = a.variant.split(":")
    _desc, L, M2, state, reps = bench.workload(config, 0)
    out = []
    for _ in range(a.repeats + 1):
        eng = BatchEngine(L, int(iters), reps, use_second_order=M2, state_representation=state, rng="mt19937")
        try:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            eng.run(snapshots=False, payoff_every=int(every), payoff_max_d=MAX_D[config] if int(every) else None)
            torch.cuda.synchronize()
            out.append(time.perf_counter() - t0)
            executed = eng.t - 1
        finally:
            eng.close()
    return {"leg": "run", "variant": a.variant, "iterations": executed, "replicas": len(reps), "L": L,
            "us_per_iter": [s / executed * 1e6 for s in out[1:]], "seconds": out[1:]}


PAIR_MAP_FIELDS = {"cc": (("coop", "coop"),), "all": (("coop", "coop"), ("flip", "flip"), ("coop", "flip"))}


def leg_pair_map_call(a):
    import torch
    from spgg_amd import pairmap
    config, D, which = a.variant.split(":")
    eng = _engine_at(config, 200, 300, flush=False)
    try:
        D = eng.L // 2 if D == "half" else int(D)
        pairs = [(pairmap.FIELDS[x], pairmap.FIELDS[y]) for x, y in PAIR_MAP_FIELDS[which]]
        shape = pairmap.map_shape(D)
        width = shape[0] * shape[1]
        ws = eng._pair_map_work(D)
        outs = [torch.zeros((eng.R, width), dtype=torch.int32, device=eng.dev) for _ in pairs]

        def call(g, s):
            rc = 0
            for (fa, fb), o in zip(pairs, outs):
                rc = rc or eng.lib.spgg_pair_map(g["ctx"], eng.t, fa, fb, D, ws[g["r0"]].data_ptr(), o[g["r0"]].data_ptr(), width, s)
            return rc
        us = _timed_rounds(eng, a, call)
        cc = outs[0].cpu().numpy().reshape((eng.R,) + shape)
        assert (cc[:, 0, D + 1:] == cc[:, 0, D - 1::-1][:, :D]).all() if D else True      # the axis row is symmetric
        work = sum(pairmap.work(eng.L, g["r1"] - g["r0"], D) for g in eng.groups) * len(pairs)
        return {"leg": "call", "variant": a.variant, "L": eng.L, "replicas": eng.R, "groups": eng.G, "max_d": D,
                "maps": len(pairs), "word_blocks": work, "word_blocks_per_second": [round(work / (u * 1e-6)) for u in us],
                "us_per_round": us}
    finally:
        eng.close()


def leg_pair_map_run(a):
    import torch
    import bench
    from spgg_amd.engine import BatchEngine
    config, every, iters = a.variant.split(":")
    _desc, L, M2, state, reps = bench.workload(config, 0)
    out = []
    for _ in range(a.repeats + 1):
        eng = BatchEngine(L, int(iters), reps, use_second_order=M2, state_representation=state, rng="mt19937")
        try:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            eng.run(snapshots=False, pair_map_every=int(every), pair_map_max_d=32 if int(every) else None)
            torch.cuda.synchronize()
            out.append(time.perf_counter() - t0)
            executed = eng.t - 1
        finally:
            eng.close()
    return {"leg": "run", "variant": a.variant, "iterations": executed, "replicas": len(reps), "L": L,
            "us_per_iter": [s / executed * 1e6 for s in out[1:]], "seconds": out[1:]}


def leg_pair_map_host(a):
    from spgg_amd import pairmap
    config, D, how = a.variant.split(":")
    eng = _engine_at(config, 200, 300)
    try:
        D = eng.L // 2 if D == "half" else int(D)
        fn = pairmap.host_pair_map if how == "roll" else pairmap.host_pair_map_fft
        device = [eng.pair_map(k, "coop", "coop", D) for k in range(eng.R)]
        out = []
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            host = []
            for S in _final_planes(eng, eng.S):          # (the copy is part of the host path)
                c = (S & 1) == 0
                host.append(fn(c, c, D))
            out.append(time.perf_counter() - t0)
        same = all((h == d).all() for h, d in zip(host, device))
        return {"leg": "host", "variant": a.variant, "L": eng.L, "max_d": D, "replicas": eng.R, "equals_device": bool(same),
                "seconds": out}
    finally:
        eng.close()


RUN = (leg_run, ["0", "16", "1"])
LEGS = {"clusters": {"final": (leg_final, ["device", "host"]),
                     "call": (leg_call, [f"{c}:{s}:{p}" for c in ("cfg3", "cfg4") for s in ("record", "sizes")
                                         for p in (0, 1)]),
                     "run": (leg_run, ["0", "1", "16"]),
                     "tiled": (leg_tiled, [f"cfg5:{t}:{s}" for t in (32, 64, 128, 200) for s in ("record", "sizes")]
                               + [f"{c}:{t}:record" for c in ("cfg4", "cfg3") for t in ("lds", 0, 32, 128)]),
                     "host5": (leg_host5, ["cfg5"]),
                     "run5": (leg_run5, ["0", "256", "16"])},
        "correlations": {"call": (leg_call, SHAPES), "host": (leg_host, SHAPES), "run": RUN},
        "reputation": {"hist": (leg_call, SHAPES), "pairs": (leg_call, SHAPES), "host": (leg_host, SHAPES), "run": RUN},
        "dwell": {"run": (leg_dwell_run, [f"{c}:{e}:{i}" for c in SHAPES for i in ("iters", "400") for e in (0, 256, 16)]),
                  "launch": (leg_dwell_launch, [f"{c}:{t}" for c in SHAPES for t in (20, 400)]),
                  "record": (leg_dwell_record, [f"{c}:{w}" for c in SHAPES for w in ("record", "fields")])},
        "policy": {"call": (leg_policy_call, [f"{c}:{w}" for c in SHAPES for w in ("pending", "flushed")]),
                   "run": (leg_policy_run, [f"{c}:{e}:iters" for c in SHAPES for e in (0, 100, 10, 1)])},
        "payoff": {"census": (leg_payoff_call, SHAPES), "pairs": (leg_payoff_call, SHAPES),
                   "run": (leg_payoff_run, [f"{c}:{e}:iters" for c in SHAPES for e in (0, 100, 10, 1)])},
        "pair_map": {"call": (leg_pair_map_call, [f"{c}:{d}:{w}" for c in SHAPES for d in (32, "half") for w in ("cc", "all")]),
                     "run": (leg_pair_map_run, [f"cfg3:{e}:iters" for e in (0, 100, 10)]),
                     "host": (leg_pair_map_host, ["cfg3:32:roll", "cfg4:32:roll", "cfg5:32:roll", "cfg3:half:fft", "cfg4:half:fft",
                                                  "cfg5:half:fft"])}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--record", required=True, choices=sorted(LEGS))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10000)
    ap.add_argument("--legs", default=None)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--variant", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    legs = LEGS[a.record]
    if a.child:
        print("RESULT " + json.dumps(legs[a.child][0](a)), flush=True)
        return 0
    width = 16 if a.record in ("clusters", "dwell", "policy", "payoff", "pair_map") else 6
    for leg in (a.legs.split(",") if a.legs else legs):
        for variant in legs[leg][1]:
            variant = variant.replace(":iters", f":{a.iters}")
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--record", a.record, "--child", leg,
                                "--variant", variant, "--repeats", str(a.repeats), "--iters", str(a.iters)],
                               capture_output=True, text=True, timeout=600)
            line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
            if r.returncode or not line:
                print(f"{leg} {variant}: failed rc={r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}", flush=True)
                return 1   # nothing more is started after a failed leg
            d = json.loads(line[0][7:])
            for key, unit in (("us_per_round", "us"), ("us_per_iter", "us/iter"), ("us_per_iter_off", "us/iter (off)"),
                              ("us_per_iter_on", "us/iter (armed)"), ("hist_seconds", "s (hist)"), ("seconds", "s")):
                vals = d.get(key)
                if not vals:
                    continue
                print(f"{leg:5s} {variant:{width}s} median {statistics.median(vals):.6g} {unit}  "
                      f"min {min(vals):.6g} max {max(vals):.6g}  n={len(vals)}  "
                      + " ".join(f"{k}={v}" for k, v in d.items()
                                 if k not in ("seconds", "hist_seconds", "us_per_round", "us_per_iter", "us_per_iter_off",
                                              "us_per_iter_on", "leg", "variant")),
                      flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
