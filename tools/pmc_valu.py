"""VALU issue of the step kernel from one rocprofv3 --pmc pass (no tracing beside it) over a
fresh run of tools/window_probe.py: per iteration window, the dynamic VALU / SALU instructions
per wave, the VALU-busy share and, where the pass recorded dispatch times, the effective clock.

    python tools/pmc_valu.py <dir> --groups G [--windows 6-25,401-600]

<dir> holds the pass's counter_collection.csv (counters SQ_WAVES SQ_INSTS_VALU
SQ_ACTIVE_INST_VALU SQ_INSTS_SALU SQ_WAVE_CYCLES SQ_BUSY_CYCLES GRBM_GUI_ACTIVE).  The run
launches G replica groups per iteration, so iteration t is dispatches (t-1)*G .. t*G-1 of the
step kernel in dispatch order.

  valu/wave      SQ_INSTS_VALU / SQ_WAVES
  salu/wave      SQ_INSTS_SALU / SQ_WAVES
  valu_busy      the share of SIMD time with a VALU instruction in flight.  rocprofv3 reports
                 SQ_ACTIVE_INST_VALU summed over every SIMD in quad-cycles and SQ_BUSY_CYCLES
                 summed over the 32 shader engines (8 XCDs x 4), so the share is
                 (4 x SQ_ACTIVE_INST_VALU / 1024 SIMDs) / (SQ_BUSY_CYCLES / 32) = raw / 8.
                 Cross-checks: SQ_BUSY_CYCLES / 32 comes out at 0.8 x GRBM_GUI_ACTIVE / 8, and
                 SQ_ACTIVE_INST_VALU at 1.02 x SQ_INSTS_VALU (one quad-cycle per instruction,
                 whatever its width: DESIGN.md section 4).  The raw ratio is printed beside it.
  wave_cyc/wave  SQ_WAVE_CYCLES x4 / SQ_WAVES (a wave's residency in clocks)
  MHz            GRBM_GUI_ACTIVE / 8 XCDs / dispatch duration, if the csv carries timestamps.  The
                 counter's window is wider than the timestamps' (it comes out above the 2400 MHz
                 peak), so this is an upper bound of the clock, good for comparing runs only.
"""
import argparse
import collections
import csv
import glob
import gzip
import os


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("dir")
    ap.add_argument("--groups", type=int, default=1)
    ap.add_argument("--windows", default="6-25,401-600")
    ap.add_argument("--kernel", default="spgg_step_kernel")
    a = ap.parse_args()
    per = collections.defaultdict(dict)
    dur = {}
    for f in glob.glob(os.path.join(a.dir, "**", "*counter_collection.csv*"), recursive=True):
        fh = gzip.open(f, "rt") if f.endswith(".gz") else open(f)
        rows = [r for r in csv.DictReader(fh) if a.kernel in r["Kernel_Name"]]
        ids = sorted({int(r["Dispatch_Id"]) for r in rows})
        order = {d: i for i, d in enumerate(ids)}
        for r in rows:
            i = order[int(r["Dispatch_Id"])]
            per[r["Counter_Name"]][i] = per[r["Counter_Name"]].get(i, 0.0) + float(r["Counter_Value"])
            if r.get("Start_Timestamp") and r.get("End_Timestamp"):
                dur[i] = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
    n = max((max(v) + 1 for v in per.values()), default=0)
    print(f"{os.path.basename(os.path.normpath(a.dir))}: {n} step-kernel dispatches, {a.groups} per iteration; counters {sorted(per)}")
    print("iters      valu/wave salu/wave  valu_busy   (raw)  wave_cyc/wave  busy_cyc/disp  gui_active/disp  dur_us    MHz")
    for w in a.windows.split(","):
        lo, hi = (int(x) for x in w.split("-"))
        idx = [i for i in range((lo - 1) * a.groups, hi * a.groups) if i < n]

        def tot(k):
            return sum(per[k].get(i, 0.0) for i in idx)
        waves = max(tot("SQ_WAVES"), 1.0)
        busy = max(tot("SQ_BUSY_CYCLES"), 1.0)
        share = tot("SQ_ACTIVE_INST_VALU") / busy
        d = [dur[i] for i in idx if i in dur]
        gui = tot("GRBM_GUI_ACTIVE")
        mhz = f"{gui / 8 / sum(d):7.0f}" if d and sum(d) > 0 else "    n/a"
        du = f"{sum(d) / len(d):7.2f}" if d else "    n/a"
        print(f"{lo:4d}-{hi:<4d} {tot('SQ_INSTS_VALU') / waves:10.1f} {tot('SQ_INSTS_SALU') / waves:9.1f} "
              f"{share / 8:10.3f} {share:7.4f} {4 * tot('SQ_WAVE_CYCLES') / waves:13.0f} "
              f"{busy / max(len(idx), 1):14.0f} {gui / max(len(idx), 1):16.0f} {du} {mhz}")


if __name__ == "__main__":
    main()
