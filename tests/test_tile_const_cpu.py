"""Static VALU count of the bench's step-kernel instance after the compile-time tile height and the
twin plus-count planes (CPU: disassembles the gfx950 code object of libspgg_hip.so, no GPU), and
the register budget of the run-time-height forms those instances gained.

The cut changes no result -- only which instruction forms an address -- so no parity test sees an
edit that gives it back (profiles/tile_const/README.txt).  The ceiling is this cut's own ledger
figure (profiles/tile_const/ledger_head.txt, tools/issue_ledger.py: "static VALU 1718") plus 2 %
for compiler drift; the figure itself is below the 1788 of the parent
(profiles/tile_const/ledger_parent.txt).
"""
import os

import pytest

from tests.test_kernel_issue_cpu import OBJDUMP, _static_valu
from tests.test_kernel_resources_cpu import BENCH_KERNEL, BENCH_MAX_VGPR, LIB, READELF, _kernels

PARENT_STATIC_VALU = 1788
HEAD_STATIC_VALU = 1718
HEAD_MAX_STATIC_VALU = HEAD_STATIC_VALU * 102 // 100
# the run-time-height form of a slot-word instance: first order, Philox (2), four agents per
# thread, width 40; action / reputation state, f64 / int8 reputation, three one-table operators
RTH_KERNEL = "spgg_step_kernel_rthILb0E"
RTH_INSTANCES = 12


def test_ledger_figure_is_below_the_parents():
    assert HEAD_STATIC_VALU < PARENT_STATIC_VALU
    assert HEAD_MAX_STATIC_VALU < PARENT_STATIC_VALU    # the ceiling itself keeps part of the cut


def test_bench_kernel_static_valu_after_the_cut():
    if not os.path.exists(LIB):
        pytest.skip("libspgg_hip.so not built")
    if not os.path.exists(OBJDUMP):
        pytest.skip("llvm-objdump not available")
    got = _static_valu(LIB, BENCH_KERNEL)
    assert got is not None, "bench instance not found in libspgg_hip.so"
    valu, total = got
    print(f"bench instance: {valu} VALU of {total} instructions (ceiling {HEAD_MAX_STATIC_VALU})")
    assert total > valu > 1000, got        # a whole kernel was disassembled
    assert valu <= HEAD_MAX_STATIC_VALU, (valu, HEAD_MAX_STATIC_VALU)


def test_run_time_height_forms_keep_the_register_budget():
    """Twelve of them, none named like the bench's instance, each within five waves and no scratch."""
    if not os.path.exists(LIB):
        pytest.skip("libspgg_hip.so not built")
    if not os.path.exists(READELF):
        pytest.skip("llvm-readelf not available")
    ks = _kernels(LIB)
    rth = {k: v for k, v in ks.items() if RTH_KERNEL in k}
    assert len(rth) == RTH_INSTANCES, sorted(rth)
    assert not [k for k in rth if BENCH_KERNEL in k]
    bad = {k: v for k, v in rth.items()
           if v["private_segment_fixed_size"] or v["vgpr_spill_count"] or v["vgpr_count"] > BENCH_MAX_VGPR}
    assert not bad, bad
