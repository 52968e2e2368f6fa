"""Static VALU instruction count of the bench's step-kernel instance (CPU: disassembles the gfx950
code object of libspgg_hip.so, no GPU).

The instance runs close to its VALU issue limit (profiles/valu_diet/README.txt), and an
edit that adds vector instructions changes no result, so no parity test sees it.  Instructions
are counted by class alone (the v_ prefix of the disassembly), as tools/issue_ledger.py counts
them from the compiler's assembly.

The ceiling is what the issue cuts reached, not what they aimed at: 1864 -> 1768 static VALU,
4836 -> 4576 weighted issue cycles (-5.4 %; the goal was -10 %)."""
import os
import subprocess
import tempfile

import pytest

from tests.test_kernel_resources_cpu import BENCH_KERNEL, LIB, _code_objects

OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"
# tools/issue_ledger.py on this kernel's sources (profiles/valu_diet/ledger_head.txt: "static VALU
# 1768", down from the 1864 of profiles/valu_diet/ledger_parent.txt), plus 2 % for compiler drift
BENCH_STATIC_VALU = 1768
BENCH_MAX_STATIC_VALU = BENCH_STATIC_VALU * 102 // 100


def _static_valu(path, kernel):
    with tempfile.TemporaryDirectory() as tmp:
        for i, co in enumerate(_code_objects(path)):
            f = os.path.join(tmp, f"co{i}.o")
            open(f, "wb").write(co)
            syms = subprocess.run([OBJDUMP, "-t", f], capture_output=True, text=True, check=True).stdout
            names = [ln.split()[-1] for ln in syms.splitlines() if kernel in ln and "F .text" in ln]
            if not names:
                continue
            assert len(names) == 1, names
            dis = subprocess.run([OBJDUMP, "-d", f"--disassemble-symbols={names[0]}", f], capture_output=True,
                                 text=True, check=True).stdout
            ops = [ln.split()[0] for ln in dis.splitlines() if ln.startswith("\t") and ln.split()]
            return sum(op.startswith("v_") for op in ops), len(ops)
    return None


def test_bench_kernel_static_valu_count():
    if not os.path.exists(LIB):
        pytest.skip("libspgg_hip.so not built")
    if not os.path.exists(OBJDUMP):
        pytest.skip("llvm-objdump not available")
    got = _static_valu(LIB, BENCH_KERNEL)
    assert got is not None, "bench instance not found in libspgg_hip.so"
    valu, total = got
    print(f"bench instance: {valu} VALU of {total} instructions (ceiling {BENCH_MAX_STATIC_VALU})")
    assert total > valu > 1000, got        # a whole kernel was disassembled
    assert valu <= BENCH_MAX_STATIC_VALU, (valu, BENCH_MAX_STATIC_VALU)
