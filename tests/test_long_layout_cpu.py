"""CPU: the two statements that tests/test_gpu_long_layout.py holds against k_long agree with each other, and its cases reach
what they claim to reach.  For every batch builder of tests/long_layout.py the closed forms (written from the column definitions)
equal the oracle's counts; the restated work assignment gives, for cards of 64, 256 and 304 CUs, the rows per wave of case 1 and
the fill levels of case 2; and the constants of that restatement are read out of the kernel sources, so that a changed constant
fails here and not silently on the card."""
import os
import re

import numpy as np
import pytest

from tests import long_layout as ll
from tests.parity import run_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bamqc_amd", "csrc")
N_CUS = (64, 256, 304)


def _oracle_agrees(cols_list, ref, n_lanes=1, triplets=None):
    if isinstance(cols_list, dict):
        cols_list = [cols_list]
    rc, co, _ = run_oracle(cols_list, [ref], n_lanes=n_lanes, n_refs=1, **ll.OPTS)
    assert rc == 0
    d = ll.diff_closed_forms(ll.closed_forms(cols_list, n_lanes), co)
    assert not d, "\n".join(d[:20])
    if triplets is not None:
        for lane, want in enumerate(triplets):
            assert np.array_equal(co[lane]["triplet"], want), lane
    return co


# ---------------------------------------------------------------------------------------------------------------------------
# the constants of the restatement
# ---------------------------------------------------------------------------------------------------------------------------
def _source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _one(pattern, text):
    found = re.findall(pattern, text)
    assert len(found) == 1, (pattern, found)
    return int(found[0])


def test_constants_are_the_kernels():
    kl, dt = _source("k_long.hip"), _source("device_types.h")
    assert _one(r"#define KL_ROW\s+(\d+)", kl) == ll.KL_ROW
    assert _one(r"#define KL_WAVES\s+(\d+)", kl) == ll.KL_WAVES
    assert _one(r"\+\+n1\[mate\] == (\d+)u", kl) == ll.SPILL_ROWS
    assert _one(r"\+\+n2\[mate\] == (\d+)u", kl) == ll.QFLUSH_ROWS
    assert _one(r"#define BQC_CHUNK_READS\s+(\d+)", dt) == ll.CHUNK_READS
    assert _one(r"#define BQC_FAST_MAXLEN\s+(\d+)", dt) == ll.FAST_MAXLEN
    assert _one(r"#define BQC_T8_SPW\s+(\d+)", dt) == ll.T8_SPW
    # a lane of a row holds 16 cycles, 62 lanes count: the 4-bit counters take 15 rows, the 16-bit sums 255 rows of Phred <= 255
    assert ll.KL_ROW == 62 * 16 and ll.SPILL_ROWS == 2 ** 4 - 1 and ll.QFLUSH_ROWS * 255 < 2 ** 16
    assert (ll.WRAP_ROWS - 1) * 222 < 2 ** 16 <= ll.WRAP_ROWS * 222
    # wave w takes the reads w, w + KL_WAVES, ...; a workgroup the chunks x, x + gridDim.x, ...
    assert re.search(r"for \(uint32_t k = wave; k < ch\.count; k \+= KL_WAVES\)", kl)
    assert re.search(r"for \(uint32_t ci = blockIdx\.x;; ci \+= gridDim\.x\)", kl)


def test_grid_restatement_equals_the_librarys():
    import ctypes
    from bamqc_amd import _lib
    slots = _lib.load().bqc_long_slots
    slots.argtypes = [ctypes.c_uint32] * 4
    slots.restype = ctypes.c_uint32
    for n_cu in N_CUS + (80,):
        for longest in (1, 256, 992, 993, ll.long_len(n_cu), 64 * 992 + 1, 65536, 300_000):
            for n_chunks in (1, 3, 7, 1000):
                gx, rows = ll.kl_grid(longest, 65536, n_chunks, n_cu)
                assert gx * rows == slots(longest, 65536, n_chunks, n_cu), (n_cu, longest, n_chunks)


def test_chunk_plan_cuts_per_read_group_and_every_128():
    L = np.array([300] * 130 + [100] * 5 + [300] * 3)
    lane = np.array([1] * 130 + [0] * 5 + [0] * 3)
    chunks, ub, longest = ll.chunk_plan(dict(l_seq=L, lane=lane), n_lanes=2)
    assert [(l, len(r)) for l, r in chunks] == [(0, 3), (1, 128), (1, 2)] and longest == 300  # read group 0 first; the 100s are k_short's
    assert list(chunks[0][1]) == [135, 136, 137] and ub == 133 // 128 + 2 + 4
    chunks, _, _ = ll.chunk_plan(dict(l_seq=L, lane=lane), n_lanes=2, no_fast=True)
    assert [(l, len(r)) for l, r in chunks] == [(0, 8), (1, 128), (1, 2)]
    chunks, ub, _ = ll.chunk_plan(dict(l_seq=L, lane=np.zeros(138, int)), n_lanes=1)
    assert [(l, len(r)) for l, r in chunks] == [(0, 128), (0, 5)] and ub == 1 + 1 + 4


# ---------------------------------------------------------------------------------------------------------------------------
# the premises of cases 1 and 2
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_cu", N_CUS)
def test_long_read_shapes_a_small_grid(n_cu):
    rows = ll.long_rows(n_cu)
    gx = max(1, n_cu // rows)
    assert 60 <= rows <= 65 and ll.long_len(n_cu) <= ll.OPTS["max_read_len"]
    assert 1 <= gx <= 5 and gx % 3 != 0


@pytest.mark.parametrize("variant", ["A", "B"])
@pytest.mark.parametrize("n_cu", N_CUS)
def test_case1_every_wave_passes_the_quality_flush_twice(n_cu, variant):
    factor = ll.case1_factor(n_cu, variant)
    gx, rows, fewest = ll.case1_rows(n_cu, variant, factor)
    assert rows == ll.long_rows(n_cu) and gx == max(1, n_cu // rows)
    assert fewest >= 2 * ll.WRAP_ROWS > 2 * ll.QFLUSH_ROWS > 2 * ll.SPILL_ROWS
    if variant == "B":  # the two mates' counters reach 15 and 255 in different reads: some wave holds different row counts of them
        _, _, runs = ll.row0_runs(ll.case1_layout(n_cu, variant, factor)[2], n_cu, no_fast=True)
        by = {(x, w, m): n for x, w, m, _, n in runs}
        assert all(by[x, w, 0] != by[x, w, 1] for x in range(gx) for w in range(ll.KL_WAVES))


@pytest.mark.parametrize("n_cu", N_CUS)
def test_case2_fill_levels_around_the_spill(n_cu):
    cols, _ = ll.case2(n_cu)
    gx, levels, changes = ll.case2_levels(n_cu, cols)
    assert {ll.SPILL_ROWS - 1, ll.SPILL_ROWS, ll.SPILL_ROWS + 1} <= levels, sorted(levels)
    assert min(levels - {0}) >= 1 and max(levels) < 2 * ll.SPILL_ROWS
    assert changes == ll.CASE2_GROUPS > ll.T8_SPW  # every workgroup meets every read group: more than it has 8-mer scratch rows


def test_case4_chunk_counts():
    for n in ll.CHUNK_NS:
        cols, _ = ll.case4(n)
        chunks, _, longest = ll.chunk_plan(cols)
        assert [len(r) for _, r in chunks] == [128] * (n // 128) + ([n % 128] if n % 128 else []) and longest == (1100 if n > 1 else 300)
    assert {1, 2, 11, 12, 13, 24, 36, 128, 129} <= set(ll.CHUNK_NS)  # fewer reads than waves, whole rounds of them, a second chunk


# ---------------------------------------------------------------------------------------------------------------------------
# closed forms == oracle, for every builder
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["A", "B"])
def test_case1_closed_forms_equal_the_oracle(variant):
    cols, ref = ll.case1(256, variant)
    co = _oracle_agrees(cols, ref, triplets=[ll.triplets_all_m(ref, cols)])
    L = cols["l_seq"].astype(np.int64)
    for m, bit in (("r1", ll.FIRST), ("r2", ll.LAST)):
        Lm = L[(cols["flag"] & bit) != 0]
        want = 222 * (Lm[None, :] > np.arange(Lm.max() if len(Lm) else 0)[:, None]).sum(1)
        assert np.array_equal(co[0][m + ".qualcount"].astype(np.int64), want)
        assert (int(co[0][m + ".averageQual"][222]) if len(Lm) else 0) == len(Lm) == int(co[0][m + ".averageQual"].sum())
    assert int(co[0]["r1.dnacount0"][0]) == int(((cols["flag"] & ll.FIRST) != 0).sum()) - 1 + int(ref[0] == 0)  # first cycle: A


def test_case2_closed_forms_equal_the_oracle():
    cols, ref = ll.case2(256)
    _oracle_agrees(cols, ref, n_lanes=ll.CASE2_GROUPS, triplets=[ll.triplets_all_m(ref, cols, g) for g in range(ll.CASE2_GROUPS)])


@pytest.mark.parametrize("sub", ["a", "b", "c"])
def test_case3_closed_forms_equal_the_oracle(sub):
    cols, ref = ll.case3(sub)
    assert sorted(set(cols["l_seq"].tolist())) == sorted(ll.SEAM_LENGTHS) and len(cols["flag"]) == 4 * len(ll.SEAM_LENGTHS)
    co = _oracle_agrees(cols, ref, triplets=[ll.triplets_all_m(ref, cols)] if sub == "a" else None)
    if sub == "b":
        assert int(co[0]["r1.Ncount"][1] + co[0]["r2.Ncount"][1]) == len(cols["flag"])  # one N per read
    assert int(co[0]["triplet"].sum()) > 0


def test_case3_all_in_two_batches():
    parts = [ll.case3(s) for s in "abc"]
    _oracle_agrees(ll.case3_two_batches(parts), parts[0][1])


def test_case4_closed_forms_equal_the_oracle():
    for n in ll.CHUNK_NS:
        cols, ref = ll.case4(n)
        _oracle_agrees(cols, ref)
