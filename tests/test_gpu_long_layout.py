"""GPU parity of k_long at the limits of its layout (k_long.hip), the way test_gpu_short_triplet_layout.py and
test_gpu_value_limits.py pin k_short's: the quality flush every 255 rows and the counter spill every 15 rows of a wave and mate,
the spill at a read-group change at every fill level around 15, reads that end, carry an N, a quality threshold or a CIGAR segment
boundary within 17 cycles of a row seam (992 cycles), and chunks of fewer reads than a workgroup has waves, of exactly one, two
and three rounds of them, and of 128 reads and one more.

Every case is compared bit for bit with the oracle AND with closed forms computed from the input columns (tests/long_layout.py;
tests/test_long_layout_cpu.py holds the two against each other and proves the premises for other CU counts).  Cases 1 and 2 first
prove from the restated work assignment, for this card's CU count, that they reach what they claim."""
import functools

import numpy as np
import pytest

from tests import long_layout as ll
from tests.parity import assert_parity
from tests.test_gpu_value_limits import n_cu

pytestmark = pytest.mark.gpu


def _check(cols_list, ref, n_lanes=1, triplets=None):
    if isinstance(cols_list, dict):
        cols_list = [cols_list]
    co, cg, _, _ = assert_parity(cols_list, [ref], n_lanes=n_lanes, **ll.OPTS)
    d = ll.diff_closed_forms(ll.closed_forms(cols_list, n_lanes), cg)
    assert not d, "\n".join(d[:20])
    if triplets is not None:
        for lane, want in enumerate(triplets):
            assert np.array_equal(cg[lane]["triplet"], want), "lane %d triplet" % lane
    return cg


# ---------------------------------------------------------------------------------------------------------------------------
# 1. flush cadences
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["A", "B"])
def test_quality_flush_and_counter_spill_cadences(variant, monkeypatch):
    """Every wave of the workgroups of row 0 adds at least 2 * 296 rows of Phred 222 of each mate (296 * 222 does not fit 16 bits)
    in ONE read group: it passes the 255-row quality flush twice and the 15-row spill some forty times.  Every short read's first
    cycle is an A, so the 4-bit counter of A at cycle 0 is full at every spill.  A: first mates only.  B: mates 1, 1, 2 by read
    index — the two mates' counters of a wave reach 15 and 255 in different reads.  With 60 chunks per workgroup (A) a wave adds
    600 rows; B needs 180 chunks for 600 rows of the second mate (92 161 reads, 5.4 MB of columns on a card of 256 CUs)."""
    monkeypatch.setenv("BQC_NO_FAST", "1")
    cu = n_cu()
    factor = ll.case1_factor(cu, variant)
    gx, rows, fewest = ll.case1_rows(cu, variant, factor)
    print("case 1 %s: n_cu %d, grid %d x %d, %d chunks per workgroup, every wave adds >= %d rows of a mate" % (variant, cu, gx, rows, factor, fewest))
    assert gx == max(1, cu // ll.long_rows(cu)) and fewest >= 2 * ll.WRAP_ROWS
    cols, ref = ll.case1(cu, variant)
    g = _check(cols, ref, triplets=[ll.triplets_all_m(ref, cols)])[0]  # (Phred 222: no triplet counts)
    L = cols["l_seq"].astype(np.int64)
    for m, bit in (("r1", ll.FIRST), ("r2", ll.LAST)):
        Lm = L[(cols["flag"] & bit) != 0]
        want = 222 * (Lm[None, :] > np.arange(Lm.max() if len(Lm) else 0)[:, None]).sum(1)
        assert np.array_equal(g[m + ".qualcount"].astype(np.int64), want), m
        assert (int(g[m + ".averageQual"][222]) if len(Lm) else 0) == len(Lm) == int(g[m + ".averageQual"].sum()), m


# ---------------------------------------------------------------------------------------------------------------------------
# 2. fill level at a read-group change
# ---------------------------------------------------------------------------------------------------------------------------
def test_read_group_change_at_every_fill_level(monkeypatch):
    """24 read groups in order; at a change a wave of row 0 holds 0 to 19 rows of a mate — 14, 15 (spilled by the row itself: the
    change spills zeros) and 16 (one row after a spill) among them; a workgroup meets 24 read groups, more than it has 8-mer
    scratch rows (BQC_T8_SPW = 8), so the 8-mer table leaves by atomics too."""
    monkeypatch.setenv("BQC_NO_FAST", "1")
    cu = n_cu()
    cols, ref = ll.case2(cu)
    gx, levels, changes = ll.case2_levels(cu, cols)
    print("case 2: n_cu %d, gx %d, fill levels %s" % (cu, gx, sorted(levels)))
    assert {ll.SPILL_ROWS - 1, ll.SPILL_ROWS, ll.SPILL_ROWS + 1} <= levels and min(levels - {0}) >= 1
    assert changes == ll.CASE2_GROUPS > ll.T8_SPW
    _check(cols, ref, n_lanes=ll.CASE2_GROUPS, triplets=[ll.triplets_all_m(ref, cols, g) for g in range(ll.CASE2_GROUPS)])


# ---------------------------------------------------------------------------------------------------------------------------
# 3. row seams
# ---------------------------------------------------------------------------------------------------------------------------
_case3 = functools.lru_cache(maxsize=None)(ll.case3)  # (built once; never changed)


@pytest.mark.parametrize("sub", ["a", "b", "c"])
def test_row_seams(sub):
    """Lengths 992 r + d (r = 1, 2; d = -17..17) and 256..258, forward / reverse x first / second mate.  a: N-free all-M (triplet
    closed form); b: an N within 9 cycles of the seam, qualities 19 / 20 / 94 / 95 on the four cycles around it; c: a deletion,
    an insertion or a skip whose segment boundary lies within 2 bases of the seam (triplets against the oracle)."""
    cols, ref = _case3(sub)
    g = _check(cols, ref, triplets=[ll.triplets_all_m(ref, cols)] if sub == "a" else None)[0]
    assert int(g["triplet"].sum()) > 0


def test_row_seams_all_in_two_batches():
    parts = [_case3(s) for s in "abc"]
    _check(ll.case3_two_batches(parts), parts[0][1])


# ---------------------------------------------------------------------------------------------------------------------------
# 4. chunk sizes
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", ll.CHUNK_NS)
def test_chunk_sizes(n):
    """n reads of 300 / 1100 bases in turn: fewer reads than the workgroup has waves (a wave's pipeline starts empty), exactly
    12, 24 and 36 (the prologue's reads k, k + 12, k + 24 and nothing behind them), one more and one fewer, a full chunk and a
    second one of 1 or 129 reads; row 1 skips every other read."""
    cols, ref = ll.case4(n)
    chunks, _, _ = ll.chunk_plan(cols)
    assert sum(len(r) for _, r in chunks) == n and len(chunks) == -(-n // ll.CHUNK_READS)
    _check(cols, ref)
