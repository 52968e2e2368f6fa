"""The slot-word step kernels' compile-time tile height and twin plus-count planes
(profiles/tile_const/README.txt) against the oracle: S, R, Q and the stop iteration bit for bit,
every slot of the history record inside tests/_record.bounds.

Both changes sit in the per-launch large-batch Philox instances of compile-time width 40.  Where
every tile of the lattice is 40 x 25 (25 divides L: L = 200, 1000) the instance with the height as
a constant runs: the LDS layout, the ring and the loop bounds are then constants.  Every other
height (L = 120: 40 x 24) keeps the run-time-height form of the same kernel.  In both forms a
payoff evaluation reads the plus-count plane or its twin (every byte + 48) by the cell's own
strategy and takes the table entries from one base.  Which instruction forms an address changes;
no floating-point operation, operand or order does.  So the cases are the fixed-height instance at
the smallest lattice that reaches it (L = 200: 5 x 8 tiles, interior and wrapped neighbours both
ways), kappa in {0, 0.5, 1} at w_P = 1 (kappa != 0 adds the S_{t-1} planes, the twin of which
shares the ring records' space), the general reward path at w_P = 0.95, one launch whose workgroups
take different branches, the other two operators (SARSA builds its one plane from the defector
bits), and the run-time-height form at L = 120.  T <= 30.
"""
import pytest

torch = pytest.importorskip("torch")

from tests import test_gpu_issue_cuts as C  # noqa: E402  (its helpers)
from tests import test_gpu_prev_rewards as P  # noqa: E402  (its oracle records, shared and read only)

L_FIXED, T_FIXED = 200, 20
L_RTH, T_RTH = 120, 30
TILE_H = 25     # csrc/spgg_kernels.hip, kTileH


def _fixed_height(eng):
    """The library's rule restated (csrc/spgg_kernels.hip, launch_cfg and launch_t): a slot-word
    instance (first order, Philox, four agents per thread at the compile-time width 40) takes the
    fixed-height form where the tile is 25 rows high and 25 divides the lattice side."""
    return C._compile_time_width_40(eng) and eng.tile[1] == TILE_H and eng.L % TILE_H == 0


def _tile_fixed(eng):
    assert eng.tile == (40, TILE_H), eng.tile
    assert (eng.L // 40, eng.L // TILE_H) == (5, 8)     # at least two tiles each way
    assert _fixed_height(eng)


def _tile_rth(eng):
    C._tile_ctw(eng)                                    # 40 x 24: the compile-time width ...
    assert not _fixed_height(eng)                       # ... at the run-time height


@pytest.mark.gpu
@pytest.mark.parametrize("kappa", [0.0, 0.5, 1.0])
def test_fixed_height_unit_weights_match_oracle(kappa, monkeypatch):
    """w_P = 1; kappa != 0 evaluates the rewards of t-1 from the S_{t-1} plane and its twin."""
    C._force(monkeypatch, SPGG_APT="max")
    _seed0 = 320 if kappa == 0.5 else 400               # (kappa = 0.5: the record test_gpu_prev_rewards made)
    P._check(L_FIXED, T_FIXED, [(kappa, 1.0)], _seed0, _tile_fixed)


@pytest.mark.gpu
def test_fixed_height_general_weights_match_oracle(monkeypatch):
    C._force(monkeypatch, SPGG_APT="max")
    P._check(L_FIXED, T_FIXED, [(0.5, 0.95)], 410, _tile_fixed)


@pytest.mark.gpu
def test_fixed_height_mixed_replicas_in_one_launch(monkeypatch):
    """Four replicas of mixed w_P and kappa in one launch: workgroups with and without the S_{t-1}
    planes, on the unit and the general reward path, side by side."""
    C._force(monkeypatch, SPGG_APT="max", SPGG_STREAMS="1")
    P._check(L_FIXED, T_FIXED, [(0.5, 1.0), (0.0, 0.95), (1.0, 1.0), (0.5, 0.95)], 420, _tile_fixed)


@pytest.mark.gpu
@pytest.mark.parametrize("alg", ["expected_sarsa", "sarsa"])
def test_fixed_height_other_operators_match_oracle(alg, monkeypatch):
    C._force(monkeypatch, SPGG_APT="max")
    P._check(L_FIXED, T_FIXED, [(0.5, 1.0)], 430, _tile_fixed, alg=alg)


@pytest.mark.gpu
def test_run_time_height_matches_oracle(monkeypatch):
    """L = 120: 24-row tiles, the run-time-height form of the same instance (twin planes included)."""
    C._force(monkeypatch, SPGG_APT="max")
    P._check(L_RTH, T_RTH, [(0.5, 1.0)], 300, _tile_rth)   # (the record test_gpu_prev_rewards made)
