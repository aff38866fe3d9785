"""GPU: k_qcyc and k_mbc past one step per workgroup (bamqc_amd/csrc/k_qcyc.hip, k_mbc.hip).

Both kernels use about one workgroup per CU and walk a workgroup's share of the batch in steps of 960 / 768 reads, so a workgroup
makes a second step only when the batch has more than STEP * n_cu reads — 245 760 / 196 608 on 256 CUs, which every production batch
has and no older test.  The step batch (tests/cycle_steps.py) gives every workgroup of both kernels three steps: k_qcyc's prefetch of
the next step while this one is counted, the tile carried from step to step, k_mbc's fetch at a base that is not the share's begin and
its list overflowing in every step, the exit after the last step, and a read-group change exactly on a step seam of each kernel and
one inside a step.  The variant "long" adds 300 reads of 300 bases: two rows, and a row-1 workgroup that steps through the whole batch
(g1 = 1; half of it with g1 = 2), hundreds of steps, most of them without a read of its row.

The layout is asserted from the restated launch arithmetic for this card's CU count before anything runs; both modules' whole blocks
of the state vector are compared with the vectorised restatements (tests/test_cycle_steps_cpu.py proves those equal to the loop
restatements), and the views with the checks of the two older test files."""
import numpy as np
import pytest

from bamqc_amd import Aggregator
from tests import cycle_steps as cs
from tests import mbc_ref, qbc_ref
from tests import test_gpu_mismatch_by_cycle as tm
from tests import test_gpu_qual_by_cycle as tq
from tests.parity import split
from tests.test_gpu_value_limits import n_cu

pytestmark = pytest.mark.gpu
LANES = 4


_built = {}  # (a batch is built once per layout and never changed; N enters through n and the changes alone)


def _case(cu, variant, N):
    lay = cs.step_layout(cu, variant, N)
    key = (cu, variant, lay["n"], lay["changes"])
    if key not in _built:
        _built[key] = cs.step_batch(lay)
    cols, ref = _built[key]
    return lay, cols, ref, qbc_ref.table_fast(cols, LANES, N), mbc_ref.table_fast(cols, [ref], LANES, N)


def context(ref, N):
    a = Aggregator(n_lanes=LANES, qual_by_cycle=N, mismatch_by_cycle=N, **tq.OPTS)
    a.set_reference(0, ref)
    return a


def blocks(a, N):
    """(k_qcyc's words, k_mbc's words) of the state vector: the .qbc block is the vector's last, the .mbc block lies in front of it."""
    return tq.module_words(a, LANES, N), tm.module_words(a, LANES, N, behind=LANES * 2 * N * 224)


@pytest.mark.parametrize("N", [64, 300])  # below and above the longest read
@pytest.mark.parametrize("variant", ["short", "long"])
def test_three_steps_per_workgroup(variant, N):
    cu = n_cu()
    lay, cols, ref, H, T = _case(cu, variant, N)
    fewest = cs.assert_step_layout(lay, cols, len(ref))
    print("steps %s N %d: n_cu %d, %s; fewest runs of a full k_mbc step %d" % (variant, N, cu, cs.describe(lay), fewest))
    assert all(H[l, m].any() and T[l, m, t].any() for l in range(LANES) for m in range(2) for t in range(2))
    a = context(ref, N)
    a.submit(cols)
    counts = a.finalize()
    got_q, got_m = blocks(a, N)
    assert np.array_equal(got_q, H), "k_qcyc: %d words differ, first at (lane, mate, cycle, q) %s" % (
        (got_q != H).sum(), np.argwhere(got_q != H)[0].tolist())
    assert np.array_equal(got_m, T), "k_mbc: %d words differ, first at (lane, mate, table, cycle, q) %s" % (
        (got_m != T).sum(), np.argwhere(got_m != T)[0].tolist())
    tq.check_tables(a, counts, H)  # (the identity sum_q q * H == qualcount included)
    tm.check_tables(a, counts, T)
    a.close()
    # the same reads in two batches, cut where no workgroup of the whole batch had a seam: other shares, other seams, the same sums
    cut = lay["n"] // 2 + 11
    assert cut not in lay["mbc_seams"] and cut not in lay["qcyc_seams"] and cut not in lay["changes"]
    b = context(ref, N)
    for part in split(cols, [cut]):
        b.submit(part)
    b.finalize()
    again_q, again_m = blocks(b, N)
    assert np.array_equal(again_q, got_q) and np.array_equal(again_m, got_m)
    b.close()
