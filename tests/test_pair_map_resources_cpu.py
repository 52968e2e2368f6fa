"""Register / scratch budget of the built pair-map kernels (CPU: reads the gfx950 code objects of
libspgg_hip.so as tests/test_kernel_resources_cpu.py does for the step kernels, no GPU).

A lane of the count launch holds 32 accumulators, one per displacement of its block, and adds to each
with a constant funnel shift; were the accumulators indexed at run time they would live in scratch memory
and the count would run several times slower with the same results, which no parity test can see."""
import os

import pytest

from tests import test_kernel_resources_cpu as KR

INSTANCES = (("spgg_pair_map_pack_kernel", 1), ("spgg_pair_map_count_kernel", 3))      # count: 16 KiB, 160 KiB, global
MAX_VGPR = 128           # four 512-thread workgroups per CU: 16 waves per SIMD-quad, 512 / 4


@pytest.fixture(scope="module")
def kernels():
    if not os.path.exists(KR.LIB):
        pytest.skip("libspgg_hip.so not built")
    if not os.path.exists(KR.READELF):
        pytest.skip("llvm-readelf not available")
    return {k: v for k, v in KR._kernels(KR.LIB).items() if "spgg_pm" in k}


def test_every_instance_is_built(kernels):
    for part, count in INSTANCES:
        assert len([k for k in kernels if part in k]) == count, (part, sorted(kernels))
    assert len(kernels) == sum(count for _part, count in INSTANCES), sorted(kernels)


def test_pair_map_kernels_use_no_scratch_and_spill_nothing(kernels):
    bad = {k: v for k, v in kernels.items() if v["private_segment_fixed_size"] or v["vgpr_spill_count"] or v["sgpr_spill_count"]}
    assert not bad, bad


def test_count_kernels_hold_their_accumulators_in_registers(kernels):
    for k, v in kernels.items():
        if "count_kernel" in k:
            assert 32 < v["vgpr_count"] <= MAX_VGPR, (k, v)
