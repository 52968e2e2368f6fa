"""tools/issue_ledger.py --trips: loop bodies of a barrier segment weighted by a stated trip count.

A toy kernel body of three barrier segments: the second holds a loop (a label and a backward branch
to it) with straight-line code before and after, the third a forward branch only.  The weighted
totals equal the hand count.
"""
import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("issue_ledger", os.path.join(ROOT, "tools", "issue_ledger.py"))
L = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(L)

TOY = """\
\tv_mov_b32_e32 v0, 0
\tv_add_f64 v[2:3], v[2:3], v[4:5]
\ts_barrier
\tv_mov_b32_e32 v1, 0
.LBB0_1:
\tv_add_u32_e32 v1, 1, v1
\tv_mul_f64 v[2:3], v[2:3], v[2:3]
\tv_mul_lo_u32 v6, v1, v1
\ts_cmp_lt_i32 s0, 5
\ts_cbranch_scc1 .LBB0_1
\tv_mov_b32_e32 v7, 0
\ts_barrier
\ts_cbranch_scc0 .LBB0_3
\tv_add_f64 v[2:3], v[2:3], v[4:5]
.LBB0_3:
\tv_mov_b32_e32 v0, 0
\ts_endpgm
""".split("\n")


def test_parse_trips():
    assert L.parse_trips("") == {}
    assert L.parse_trips("2=4.43,5=3") == {2: 4.43, 5: 3.0}


def test_loop_lines_are_label_to_backward_branch():
    inside = L.loop_lines(TOY)
    assert inside == set(range(4, 10))          # .LBB0_1 .. s_cbranch_scc1; the forward branch makes no loop


def test_weighted_total_equals_hand_count():
    # weights: 32-bit op 2, f64 op 4, v_mul_lo_u32 8
    static = L.weighted_segments(TOY, {})
    assert static == [[2.0, 6.0], [5.0, 18.0], [2.0, 6.0]]
    w = L.weighted_segments(TOY, {1: 4.5})
    # segment 1: v_mov (2) + 4.5 x (v_add_u32 2 + v_mul_f64 4 + v_mul_lo_u32 8) + v_mov (2)
    assert w[1] == [2 + 4.5 * 3, 4 + 4.5 * 14]
    assert w[0] == static[0] and w[2] == static[2]
    assert sum(x[0] for x in w) == 2 + 15.5 + 2
    assert sum(x[1] for x in w) == 6 + 67 + 6
    # a trip count for a segment without a loop changes nothing
    assert L.weighted_segments(TOY, {0: 9, 2: 9}) == static
