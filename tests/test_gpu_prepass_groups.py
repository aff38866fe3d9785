"""GPU parity at the edges of the pre-pass's groups (k_prep.hip): k_prep_sizes sums the payload sizes of PR_GROUP blocks of 1024 reads
per workgroup, and k_prep_reads adds the totals of the groups before its own — batch sizes one read short of a group, exactly one
group, one read more, and two groups and a block and a read; reads of differing lengths and CIGARs across every group edge, so that
the three sums (ceil(L/2), L, n_cigar) differ from block to block; one read group and three (the `order` path); and a resident
batch of the largest size replayed over its own scratch."""
import ctypes
import functools

import numpy as np
import pytest

from bamqc_amd import Aggregator, _abi, _lib
from bamqc_amd import synth as csynth
from tests import synth
from tests.parity import assert_parity, run_oracle

pytestmark = pytest.mark.gpu

REF_LEN = 3_000_000
ACROSS = 3000  # reads of mixed lengths and CIGARs across every group edge


def _group_reads():
    fn = _lib.load().bqc_prep_group
    fn.argtypes, fn.restype = [], ctypes.c_uint32
    return fn() * 1024


def _sizes():
    g = _group_reads()
    return [g - 1, g, g + 1, 2 * g + 1025]


@functools.lru_cache(maxsize=None)
def _reference():
    return csynth.reference(811, 0, REF_LEN)


@functools.lru_cache(maxsize=None)
def _batch(which, n_lanes):
    """bulk reads of one length, and ACROSS mixed reads over every group edge the batch has or ends at (one contig: the FASTA scan
    never goes back, whatever the order of positions)"""
    n = _sizes()[which]
    g = _group_reads()
    ref = _reference()
    cols = csynth.batch(820 + which, n, [REF_LEN], [ref], n_lanes=n_lanes)
    for e, edge in enumerate(range(g, n + g, g)):
        lo, hi = edge - ACROSS // 2, min(n, edge + ACROSS // 2)
        if lo >= n:
            break
        mixed, _ = synth.synth(seed=830 + 10 * which + e, n_reads=hi - lo, L=150, refs=[ref], n_lanes=n_lanes, var_len=True, long_cigar=True,
                               p_indel=0.3)
        cols = synth.concat([synth.slice_batch(cols, 0, lo), mixed, synth.slice_batch(cols, hi, n)])
    assert len(cols["flag"]) == n
    # the three sums differ from block to block around the edges
    blocks = [(b * 1024, min(n, (b + 1) * 1024)) for b in (g // 1024 - 2, g // 1024 - 1, g // 1024) if b * 1024 < n]
    sums = {(int(cols["l_seq"][a:z].sum()), int(cols["n_cigar"][a:z].sum())) for a, z in blocks if z - a == 1024}
    assert len(sums) == len([1 for a, z in blocks if z - a == 1024])
    return cols


@pytest.mark.parametrize("n_lanes", [1, 3])
@pytest.mark.parametrize("which", range(4))
def test_parity_at_group_edges(which, n_lanes):
    co, cg, _, _ = assert_parity(_batch(which, n_lanes), [_reference()], n_refs=1, n_lanes=n_lanes)
    assert cg is not None  # (no error: the counts were compared)


def test_resident_batch_of_the_largest_size_five_times():
    # every replay rewrites blk_sizes and grp_sizes in full: after a reset each pass leaves exactly the state of the first
    cols = _batch(3, 3)
    ref = _reference()
    rc, co, _ = run_oracle([cols], [ref], n_refs=1, n_lanes=3)
    assert rc == 0
    a = Aggregator(n_refs=1, n_lanes=3)
    a.set_reference(0, ref)
    db = a.upload(cols)
    first = None
    for k in range(5):
        a.reset()
        a.process(db)
        st = a.state_export_host()
        if first is None:
            first = st.copy()
        assert np.array_equal(st, first), "pass %d differs from the first" % k
    cg = a.finalize()
    db.free()
    a.close()
    d = _abi.diff_counts(co, cg)
    assert not d, "\n".join(d[:10])
