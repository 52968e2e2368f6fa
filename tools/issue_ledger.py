"""Static issue ledger of one step-kernel instance: VALU count and weighted issue cycles per
barrier segment and per source function.

    python tools/issue_ledger.py [--tu 0] [--instance false,false,true,2,4,40,0] [--top 25]
                                 [--asm file.s] [--keep file.s] [--trips SEG=N[,SEG=N...]]

Rebuilds one translation unit of csrc/spgg_kernels.hip to gfx950 assembly with the build's own
compiler and flags (spgg_amd.build: HIPCC, FLAGS, the defines of that unit in UNITS) plus -gline-tables-only (line
directives only: the code is the build's), or reads --asm.  The instance is
spgg_step_kernel<M2, AS, RQ, RNG, APT, TWC, ALG>; the default is the one bench.py's cfg3 runs.

Weights (MI355X: a wave64 op issues over a 32-lane SIMD datapath): 2 cycles for a 32-bit VALU
op, 4 for f64 / 64-bit ops, 8 for the quarter-rate 32-bit multiplies and v_mad_u64_u32 and for
v_rcp_f64.  Counts are static: a loop body counts once, whatever its trip count.
Instructions are counted by class (the v_ / s_ / ds_ / global_ prefixes) alone.

--trips SEG=N weights the loop bodies of barrier segment SEG by the stated trip count N (a
fraction is a mean over the waves: 1134 cells / 256 threads = 4.43): the instructions between a
label and the last branch back to it count N times, the rest of the segment once.  The weighted
totals are printed beside the static ones; a segment without a backward branch is unchanged.

A line belongs to the function whose definition encloses it in its source file (the innermost
inlined callee the line tables name), and to the segment between the s_barriers around it.
"""
import argparse
import collections
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HEAVY = {"v_mad_u64_u32": 8, "v_mul_lo_u32": 8, "v_mul_hi_u32": 8, "v_rcp_f64": 8,
         "v_rcp_f32_e32": 4}
WIDE = ("f64", "b64", "u64", "i64")


def weight(op):
    return HEAVY.get(op, 4 if any(w in op for w in WIDE) else 2)


def mangled(instance):
    out = "spgg_step_kernelI"
    for f in instance.split(","):
        f = f.strip()
        out += {"false": "Lb0E", "true": "Lb1E"}.get(f) or f"Li{int(f)}E"
    return out + "E"


def assemble(tu, keep):
    import spgg_amd.build as B
    out = keep or os.path.join(tempfile.mkdtemp(prefix="ledger"), f"tu{tu}.s")
    src, defs, _ = next(u for u in B.UNITS if f"SPGG_TU={tu}" in u[1])  # the unit of the build table
    cmd = [B.HIPCC, *B.FLAGS, '-DSPGG_BUILD_ID="ledger"', *(f"-D{d}" for d in defs), f"-I{B.INC}", "-gline-tables-only",
           "--cuda-device-only", "-S", src, "-o", out]
    subprocess.run(cmd, check=True)
    return out


_FN = re.compile(r"^\s{0,2}(?:template\s*<[^>]*>\s*)?(?:static\s+|inline\s+|constexpr\s+|__host__\s+|__device__\s+|"
                 r"__global__\s+|__forceinline__\s+|__launch_bounds__\([^)]*\)\s+|\([^)]*\)\s*)*"
                 r"[\w:<>,\s\*&]*?\b(\w+)\s*\([^;]*$")


def function_map(path):
    """line -> name of the enclosing function definition (brace depth <= 1: namespace or struct level)."""
    try:
        src = open(path, errors="replace").read().split("\n")
    except OSError:
        return {}
    owner, cur, depth, fdepth, pending = {}, None, 0, None, None
    for i, l in enumerate(src, 1):
        code = l.split("//")[0]
        if cur is None and ("__device__" in code or "__global__" in code) and "(" in code:
            m = _FN.match(code)
            if m and m.group(1) not in ("if", "for", "while", "switch", "return", "sizeof"):
                pending = m.group(1)
        if pending and cur is None and "{" in code:
            cur, fdepth, pending = pending, depth, None
        elif pending and ";" in code and "{" not in code:
            pending = None
        if cur:
            owner[i] = cur
        depth += code.count("{") - code.count("}")
        if cur and depth <= fdepth:
            cur = None
    return owner


def parse_trips(text):
    """'2=4.43,5=3' -> {2: 4.43, 5: 3.0}"""
    out = {}
    for item in filter(None, (text or "").split(",")):
        k, _, v = item.partition("=")
        out[int(k)] = float(v)
    return out


_LABEL = re.compile(r"^([\w$.]+):")
_BRANCH = re.compile(r"^\s*s_c?branch\w*\s+([\w$.]+)")


def loop_lines(lines):
    """Indices of `lines` inside a loop body: from a label to the last branch that names it from
    below (a backward branch), both ends included."""
    label_at, inside = {}, set()
    for i, l in enumerate(lines):
        m = _LABEL.match(l)
        if m:
            label_at[m.group(1)] = i
            continue
        b = _BRANCH.match(l)
        if b and b.group(1) in label_at:
            inside.update(range(label_at[b.group(1)], i + 1))
    return inside


def weighted_segments(body, trips):
    """(valu, cycles) per barrier segment of a kernel body (its lines after the symbol, up to the
    function's end), loop bodies of segment SEG counted trips[SEG] times."""
    loops = loop_lines(body)
    seg = [[0.0, 0.0]]
    for i, l in enumerate(body):
        t = l.strip()
        if not l.startswith("\t") or not t or t.startswith((".", ";")):
            continue
        op = t.split()[0]
        if op == "s_barrier":
            seg.append([0.0, 0.0])
        elif op.startswith("v_"):
            n = trips.get(len(seg) - 1, 1.0) if i in loops else 1.0
            seg[-1][0] += n
            seg[-1][1] += n * weight(op)
    return seg


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tu", type=int, default=0)
    ap.add_argument("--instance", default="false,false,true,2,4,40,0")
    ap.add_argument("--top", type=int, default=25, help="source lines listed")
    ap.add_argument("--asm", default=None)
    ap.add_argument("--keep", default=None)
    ap.add_argument("--trips", default="", help="SEG=N[,SEG=N...]: trip count of segment SEG's loop bodies")
    a = ap.parse_args()
    path = a.asm or assemble(a.tu, a.keep)
    s = open(path).read().split("\n")
    key = mangled(a.instance)
    try:
        st = next(i for i, l in enumerate(s) if key in l and re.match(r"^[\w$.]+:", l))
    except StopIteration:
        sys.exit(f"no kernel symbol containing {key} in {path}")
    files = {}
    for l in s:
        if l.startswith("\t.file"):
            m = re.match(r'\t\.file\s+(\d+)\s+"([^"]*)"(?:\s+"([^"]*)")?', l)
            if m:
                d, f = (m.group(2), m.group(3)) if m.group(3) else ("", m.group(2))
                files[m.group(1)] = f if os.path.isabs(f) else os.path.join(d, f)
    end = next((i for i in range(st + 1, len(s)) if s[i].startswith(".Lfunc_end")), len(s))
    trips = parse_trips(a.trips)
    wseg = weighted_segments(s[st + 1:end], trips) if trips else None
    fmaps = {}
    seg = [collections.Counter()]
    fn = collections.defaultdict(collections.Counter)
    ln = collections.defaultdict(collections.Counter)
    cur = (None, 0)
    for l in s[st + 1:]:
        if l.startswith(".Lfunc_end"):
            break
        if l.startswith("\t.loc"):
            p = l.split()
            cur = (files.get(p[1], p[1]), int(p[2]))
            continue
        t = l.strip()
        if not l.startswith("\t") or not t or t.startswith((".", ";")):
            continue
        op = t.split()[0]
        c = seg[-1]
        if op == "s_barrier":
            c["salu"] += 1
            seg.append(collections.Counter())
        elif op.startswith("v_"):
            f = cur[0]
            if f not in fmaps:
                fmaps[f] = function_map(f) if f else {}
            name = fmaps[f].get(cur[1], "?")
            w = weight(op)
            for k in (c, fn[name], ln[(os.path.basename(f or "?"), cur[1], name)]):
                k["valu"] += 1
                k["cyc"] += w
            fn[name][f"seg{len(seg) - 1}"] += w
        elif op.startswith("s_"):
            c["salu"] += 1
        elif op.startswith("ds_"):
            c["lds"] += 1
        elif op.startswith(("global_", "buffer_", "flat_", "scratch_")):
            c["vmem"] += 1
    meta = {}
    for l in s[st:]:
        m = re.match(r"\s*[;.]\s*(?:\.?)(NumVgprs|ScratchSize|Occupancy|NumSgprs|LDSByteSize)\s*:\s*(\d+)", l)
        if m and m.group(1) not in meta:
            meta[m.group(1)] = int(m.group(2))
        if len(meta) == 5 or l.startswith("\t.end_amdhsa_kernel"):
            if len(meta) >= 3:
                break
    tot = sum(c["cyc"] for c in seg)
    nv = sum(c["valu"] for c in seg)
    print(f"instance spgg_step_kernel<{a.instance}>  (TU {a.tu})")
    print(f"static VALU {nv}  weighted VALU cycles {tot}  SALU {sum(c['salu'] for c in seg)}  "
          f"LDS {sum(c['lds'] for c in seg)}  VMEM {sum(c['vmem'] for c in seg)}  " +
          "  ".join(f"{k} {v}" for k, v in sorted(meta.items())))
    if wseg:
        print(f"with --trips {a.trips}: VALU {sum(w[0] for w in wseg):.0f}  weighted VALU cycles "
              f"{sum(w[1] for w in wseg):.0f}  (loop bodies of those segments at their trip counts)")
    print("\nper barrier segment")
    for i, c in enumerate(seg):
        more = f"  at {trips[i]:g} trips: valu {wseg[i][0]:7.1f}  cyc {wseg[i][1]:7.1f}" if wseg and i in trips else ""
        print(f"  seg {i:2d}: valu {c['valu']:5d}  cyc {c['cyc']:5d} ({100 * c['cyc'] / max(tot, 1):4.1f}%)  "
              f"salu {c['salu']:4d}  lds {c['lds']:4d}  vmem {c['vmem']:3d}{more}")
    print("\nper source function (weighted cycles by segment)")
    for name, c in sorted(fn.items(), key=lambda kv: -kv[1]["cyc"]):
        segs = " ".join(f"s{i}:{c[f'seg{i}']}" for i in range(len(seg)) if c[f"seg{i}"])
        print(f"  {name:28s} valu {c['valu']:5d}  cyc {c['cyc']:5d} ({100 * c['cyc'] / max(tot, 1):4.1f}%)  {segs}")
    print(f"\ntop {a.top} source lines")
    for (f, line, name), c in sorted(ln.items(), key=lambda kv: -kv[1]["cyc"])[:a.top]:
        print(f"  {c['cyc']:5d} {100 * c['cyc'] / max(tot, 1):4.1f}%  n={c['valu']:4d}  {f}:{line}  ({name})")


if __name__ == "__main__":
    main()
