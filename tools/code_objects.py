#!/usr/bin/env python3
"""Compare the gfx950 code objects of two builds of libspgg_hip.so (no GPU).

    python tools/code_objects.py A/libspgg_hip.so B/libspgg_hip.so [--isa-diff]

The code objects are cut out of the library's offload bundles as tests/test_kernel_resources_cpu.py
does (one per translation unit).  Printed, A -> B:
  1. per code object (named by its first kernel; matched by its set of kernel names): SHA-256 (12
     digits) of .text and .rodata, and whether both are equal;
  2. the kernel symbols only one library has;
  3. per kernel whose metadata differs (VGPRs, SGPRs, LDS bytes, scratch bytes, spills): both sets;
  4. per kernel of a code object that is not byte-identical: whether its disassembly is the same
     instruction text (addresses and encodings stripped; --isa-diff prints the unified diff otherwise).
Kernels are matched by demangled name without the parameter list, so a kernel whose parameter types
moved to another namespace still finds its partner (its symbol shows up under 2).
Exit status 1 if a code object, a symbol, a metadata field or an instruction differs."""
import argparse
import difflib
import hashlib
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from test_kernel_resources_cpu import _code_objects  # noqa: E402

LLVM = "/opt/rocm/lib/llvm/bin"
FIELDS = ("vgpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size",
          "vgpr_spill_count", "sgpr_spill_count")


def run(*cmd):
    return subprocess.run(cmd, capture_output=True, text=True, check=True).stdout


def base_name(demangled):
    """The demangled name without its parameter list (and without a leading return type)."""
    depth = 0
    for i in range(len(demangled) - 1, -1, -1):
        c = demangled[i]
        depth += (c == ")") - (c == "(")
        if depth == 0 and c == "(":
            demangled = demangled[:i]
            break
    return re.sub(r"^void ", "", demangled)


def section_hash(path, section, tmp):
    out = os.path.join(tmp, "section.bin")
    run(f"{LLVM}/llvm-objcopy", "-O", "binary", f"--only-section={section}", path, out)
    return hashlib.sha256(open(out, "rb").read()).hexdigest()[:12]


def disassembly(path):
    """{symbol: [instruction text]} of the object's functions, addresses stripped."""
    text = run(f"{LLVM}/llvm-objdump", "-d", "--no-show-raw-insn", "--no-leading-addr", path)
    fns, cur = {}, None
    for line in text.splitlines():
        m = re.match(r"^[0-9a-f]* ?<(\S+)>:$", line)
        if m:
            cur = fns.setdefault(m.group(1), [])
        elif cur is not None and line.strip():
            ins = re.sub(r"\s*//.*$", "", line).strip()
            if ins and ins != "..." and not ins.startswith(("s_nop", "s_code_end")):  # (...: elided padding)
                cur.append(ins)
    return fns


def load(lib, tmp):
    """The library's code objects: [{kernels: {base name: (symbol, metadata)}, text, rodata, isa}]."""
    objs = []
    for i, co in enumerate(_code_objects(lib)):
        f = os.path.join(tmp, f"co{i}.o")
        open(f, "wb").write(co)
        notes = run(f"{LLVM}/llvm-readelf", "--notes", f)
        syms = [(re.search(r"\.name:\s+(\S+)", blk).group(1),
                 {k: int(re.search(rf"\.{k}:\s+(\d+)", blk).group(1)) for k in FIELDS})
                for blk in notes.split("- .agpr_count:")[1:]]
        names = run(shutil.which("c++filt") or f"{LLVM}/llvm-cxxfilt", *[s for s, _ in syms]).splitlines() if syms else []
        objs.append({"kernels": {base_name(n): sm for n, sm in zip(names, syms)},
                     "first": base_name(names[0]) if names else "(no kernel)",
                     "text": section_hash(f, ".text", tmp), "rodata": section_hash(f, ".rodata", tmp),
                     "isa": disassembly(f)})
    return objs


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("a")
    ap.add_argument("b")
    ap.add_argument("--isa-diff", action="store_true", help="print the diff of a kernel whose instructions differ")
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        A, B = load(args.a, tmp), load(args.b, tmp)
    bad = 0
    print(f"A = {args.a}\nB = {args.b}\n")
    print("1. code objects: first kernel, kernels, .text .rodata  ->  .text .rodata")
    by_set = {frozenset(o["kernels"]): o for o in B}
    moved = []  # objects of A without a B object of the same kernels
    for o in A:
        p = by_set.pop(frozenset(o["kernels"]), None)
        if p is None:
            moved.append(o)
            print(f"  {o['first']:<60} n={len(o['kernels']):3d} {o['text']} {o['rodata']}  ->  (kernels regrouped)")
            continue
        same = (o["text"], o["rodata"]) == (p["text"], p["rodata"])
        bad += not same
        print(f"  {o['first']:<60} n={len(o['kernels']):3d} {o['text']} {o['rodata']}  ->  {p['text']} {p['rodata']}"
              f"  {'IDENTICAL' if same else 'differs'}")
        if not same:
            moved.append(o)
    for p in by_set.values():
        print(f"  {'(kernels regrouped)':<60}  ->  {p['first']} n={len(p['kernels'])} {p['text']} {p['rodata']}")

    ka = {k: (o, *sm) for o in A for k, sm in o["kernels"].items()}
    kb = {k: (o, *sm) for o in B for k, sm in o["kernels"].items()}
    sa, sb = {v[1] for v in ka.values()}, {v[1] for v in kb.values()}
    print(f"\n2. kernel symbols: {len(sa)} -> {len(sb)}; only in A: {len(sa - sb)}, only in B: {len(sb - sa)}")
    for s in sorted(sa - sb):
        print(f"  A only: {s}")
    for s in sorted(sb - sa):
        print(f"  B only: {s}")
    for k in sorted(set(ka) ^ set(kb)):
        print(f"  kernel without a partner: {k}")
    bad += len(sa ^ sb) + len(set(ka) ^ set(kb))

    print("\n3. kernels whose metadata differs (" + ", ".join(FIELDS) + ")")
    n = 0
    for k in sorted(set(ka) & set(kb)):
        if ka[k][2] != kb[k][2]:
            n += 1
            print(f"  {k}: {list(ka[k][2].values())} -> {list(kb[k][2].values())}")
    print(f"  {n} of {len(set(ka) & set(kb))}")
    bad += n

    print("\n4. kernels of the code objects that are not byte-identical: instruction text")
    for o in moved:
        for k, (sym, _) in sorted(o["kernels"].items()):
            if k not in kb:
                continue
            ia, ib = o["isa"].get(sym, []), kb[k][0]["isa"].get(kb[k][1], [])
            same = ia == ib and bool(ia)
            bad += not same
            print(f"  {k:<60} {len(ia):6d} -> {len(ib):6d} instructions  {'ISA identical' if same else 'DIFFERS'}")
            if not same and args.isa_diff:
                print("\n".join(difflib.unified_diff(ia, ib, "A", "B", lineterm="", n=2)))
    print(f"\n{'no difference' if not bad else f'{bad} difference(s)'}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
