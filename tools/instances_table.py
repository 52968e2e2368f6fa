"""VGPRs, scratch bytes and occupancy of every step and persistent kernel of the four operator
units of csrc/spgg_kernels.hip, one source tree against another (profiles/*/instances.txt).

    python tools/instances_table.py PARENT_TREE [HEAD_TREE] [--jobs 4] [--keep DIR] > instances.txt

Each tree's units are compiled to gfx950 assembly with that tree's own build table
(the package's build.py: HIPCC, FLAGS, UNITS), and NumVgprs / ScratchSize / Occupancy are read
from each kernel's trailer.  '*' marks the instances with the slot word by region index (SLOT:
first order, Philox, compile-time width 40, four agents per thread, not Double-Q; step_rth is such
an instance at the run-time tile height, step the one at the compile-time height).  The lines that
differ are listed again at the end.
"""
import argparse
import glob
import importlib.util
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {0: "Q-learning", 1: "SARSA", 2: "Expected SARSA", 3: "Double Q-learning"}


def build_table(tree):
    (path,) = glob.glob(os.path.join(tree, "*_amd", "build.py"))  # the package directory (spgg_amd.py names it)
    spec = importlib.util.spec_from_file_location("spgg_build_" + re.sub(r"\W", "_", os.path.abspath(tree)), path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def assemble(B, tu, out):
    src, defs, _ = next(u for u in B.UNITS if f"SPGG_TU={tu}" in u[1])
    cmd = [B.HIPCC, *B.FLAGS, '-DSPGG_BUILD_ID="table"', *(f"-D{d}" for d in defs), f"-I{B.INC}",
           "--cuda-device-only", "-S", src, "-o", out]
    subprocess.run(cmd, check=True, stderr=subprocess.DEVNULL)
    return out


_SYM = re.compile(r"^(_Z\w*?\d+spgg_(step|persist)_kernel(_rth)?I((?:L[bi]\d+E)+)E\w*):")
_ARG = re.compile(r"L([bi])(\d+)E")


def kernels(path):
    """{'step<0,0,1,2,4,40,0>': (vgprs, scratch, occupancy)} of one assembly file."""
    out, cur, meta = {}, None, {}
    for l in open(path):
        m = _SYM.match(l)
        if m:
            cur, meta = f"{m.group(2)}{m.group(3) or ''}<{','.join(a[1] for a in _ARG.findall(m.group(4)))}>", {}
            continue
        if cur:
            m = re.match(r"\s*;\s*(NumVgprs|ScratchSize|Occupancy)\s*:\s*(\d+)", l)
            if m:
                meta.setdefault(m.group(1), int(m.group(2)))
                if len(meta) == 3:
                    out[cur] = (meta["NumVgprs"], meta["ScratchSize"], meta["Occupancy"])
                    cur = None
    return out


def is_slot(name):
    kind, args = name.split("<")
    a = [int(x) for x in args.rstrip(">").split(",")]
    return kind in ("step", "step_rth") and a[0] == 0 and a[3] == 2 and a[4] == 4 and a[5] == 40 and a[6] != 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parent")
    ap.add_argument("head", nargs="?", default=ROOT)
    ap.add_argument("--jobs", type=int, default=4)
    ap.add_argument("--keep", default=None, help="directory for the assembly files")
    a = ap.parse_args()
    keep = a.keep or tempfile.mkdtemp(prefix="instances")
    os.makedirs(keep, exist_ok=True)
    trees = {"parent": build_table(a.parent), "head": build_table(a.head)}
    jobs = [(tag, tu) for tu in range(4) for tag in trees]
    with ThreadPoolExecutor(a.jobs) as ex:
        paths = dict(zip(jobs, ex.map(lambda j: assemble(trees[j[0]], j[1], os.path.join(keep, f"{j[0]}_tu{j[1]}.s")), jobs)))
    diff = []
    print(__doc__.split("\n\n")[0].replace("\n", " ") + "  Template arguments: M2, AS, RQ, RNG (1 MT19937, 2 Philox), "
          "APT, TWC, ALG.\n'*' marks the instances with the slot word by region index (SLOT).")
    for tu in range(4):
        p, h = kernels(paths[("parent", tu)]), kernels(paths[("head", tu)])
        print(f"\nunit {tu} ({NAMES[tu]}): {len(h)} kernels")
        print("instance                          parent (vgpr scratch occ)   head (vgpr scratch occ)")
        for k in sorted(set(p) | set(h)):
            x, y = p.get(k), h.get(k)
            f = lambda v: "   -    -   -" if v is None else f"{v[0]:4d} {v[1]:4d} {v[2]:3d}"
            print(f"{k:30s} {'*' if is_slot(k) else ' '}  {f(x)}             {f(y)}")
            if x != y:
                why = []
                if x and y:
                    if y[2] != x[2]:
                        why.append("occupancy " + ("LOWER" if y[2] < x[2] else "higher"))
                    if y[1] != x[1]:
                        why.append(("more" if y[1] > x[1] else "less") + " scratch")
                    if y[0] != x[0] and not why:
                        why.append("vgprs")
                diff.append(f"  {k}  {x} -> {y}  {', '.join(why)}")
    print(f"\n{len(diff)} instances differ:")
    print("\n".join(diff))


if __name__ == "__main__":
    sys.exit(main())
