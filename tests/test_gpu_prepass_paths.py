"""GPU parity of k_prep_reads' two paths (k_prep.hip): a read with at most one CIGAR operation is done in the thread's unrolled body
from CIGAR word 0, every other read — several operations, or set aside by a shard — by the kernel's one copy of the CIGAR walks,
called in a loop, which stores its entries behind the thread's own.  Batch sizes around a thread's four reads, a block and a
super-window; all 16 patterns of the two paths over a thread's four reads; the reads that end the run, with reads of the other path
around them; the generic kernels, three read groups, a shard's set-aside reads and replays of a resident batch.

The oracle reports an exit code and no text: where the run ends, the code is compared with the oracle's and the message with the read
the test put there (the message names the read whose key won)."""
import ctypes as C
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from bamqc_amd import Aggregator, _abi, _lib
from tests import prepass_paths as pp
from tests import synth
from tests.parity import assert_parity, run_oracle

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_AS_TAG, ERR_FASTA, ERR_RANGE = 4, 5, 6


# ---------------------------------------------------------------------------------------------------------------------------------
# batch sizes
# ---------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _mixed():
    """4097 reads of differing lengths, read i from a batch whose mapped reads all have 8 and more operations when i % 3 == 1, else
    from one with one operation, or two to five (indels, clips)"""
    ref = pp.reference()
    many, _ = synth.synth(seed=9101, n_reads=4097, L=150, refs=[ref], var_len=True, long_cigar=True, p_indel=0.3)
    few, _ = synth.synth(seed=9102, n_reads=4097, L=150, refs=[ref], var_len=True, p_indel=0.3, p_clip=0.2)
    pick = np.arange(4097) % 3 == 1
    both = synth.concat([few, many])
    cols = pp.take(both, np.where(pick, np.arange(4097) + 4097, np.arange(4097)))
    nc = cols["n_cigar"]
    assert (nc <= 1).sum() > 1000 and ((nc > 1) & (nc <= 4)).sum() > 300 and (nc > 4).sum() > 1000
    return cols


@pytest.mark.parametrize("n", [1, 3, 4, 5, 1023, 1024, 1025, 4097])
def test_batch_sizes(n):
    co, cg, _, _ = assert_parity(synth.slice_batch(_mixed(), 0, n), [pp.reference()], n_refs=1)
    assert cg is not None


# ---------------------------------------------------------------------------------------------------------------------------------
# the 16 patterns
# ---------------------------------------------------------------------------------------------------------------------------------
def test_all_patterns_of_the_two_paths_in_a_quad():
    cols = pp.pattern_batch()
    co, cg, _, _ = assert_parity(cols, [pp.reference()], n_refs=1)
    assert cg is not None
    assert int(cg[0]["triplet"].sum()) > 0


def test_three_read_groups():
    co, cg, _, _ = assert_parity(pp.pattern_batch(n_lanes=3), [pp.reference()], n_refs=1, n_lanes=3)
    assert cg is not None


_NO_FAST = r"""
import json, sys
sys.path.insert(0, sys.argv[1])
from bamqc_amd import _abi
from tests import prepass_paths as pp
from tests.parity import run_gpu, run_oracle
cols, ref = pp.pattern_batch(), pp.reference()
rc_o, co, _ = run_oracle([cols], [ref], n_refs=1)
rc_g, cg, a = run_gpu([cols], [ref], n_refs=1)
print(json.dumps({"rc": [rc_o, rc_g], "diffs": _abi.diff_counts(co, cg)[:10] if rc_o == 0 and rc_g == 0 else None}))
"""


def test_generic_kernels():
    # BQC_NO_FAST is read once per process: a child for the setting
    out = subprocess.run([sys.executable, "-c", _NO_FAST, ROOT], env=dict(os.environ, BQC_NO_FAST="1"), capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    r = json.loads(out.stdout.strip().splitlines()[-1])
    assert r["rc"] == [0, 0] and r["diffs"] == [], r


def test_resident_batch_three_times():
    cols, ref = pp.pattern_batch(), pp.reference()
    rc, co, _ = run_oracle([cols], [ref], n_refs=1)
    assert rc == 0
    a = Aggregator(n_refs=1)
    a.set_reference(0, ref)
    db = a.upload(cols)
    first = None
    for k in range(3):
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


# ---------------------------------------------------------------------------------------------------------------------------------
# reads that end the run
# ---------------------------------------------------------------------------------------------------------------------------------
def _quiet(i, pos, d, **kw):
    """a read no check looks at twice: mapping quality 0, so not eligible for triplets"""
    return (pp.deferred if d else pp.common)(i, pos, **dict(dict(mapq=0), **kw))


def _fails_at(cols, refs, read, **opts):
    co, cg, o, a = assert_parity(cols, refs, **opts)  # (the same code as the oracle's)
    assert cg is None
    msg = (a.lib.bqc_last_error(a.h) or b"").decode()
    a.close()
    assert "read %d " % read in msg.replace("(", " ").replace(")", " ").replace(":", " ") + " ", (read, msg)


@pytest.mark.parametrize("as_", [synth.BQC_AS_ABSENT, -3])
@pytest.mark.parametrize("on_deferred", [True, False])
def test_as_tag_on_one_path_between_reads_of_the_other(as_, on_deferred):
    # quad 1 of the batch: reads 4 .. 7, the failing read is number 5; eligible reads of the other path before and behind it
    recs = [(pp.deferred(i, 100 + 10 * i, kind=pp.UNCLIPPED[i % 5], as_=as_ if i == 5 else 90) if (i == 5) == on_deferred else
             pp.common(i, 100 + 10 * i, as_=as_ if i == 5 else 90)) for i in range(12)]
    cols = synth.concat(recs)
    rc, _, _ = run_oracle([cols], [pp.reference()], n_refs=1)
    assert rc == ERR_AS_TAG
    _fails_at(cols, [pp.reference()], 5, n_refs=1)


@pytest.mark.parametrize("early_deferred", [True, False])
@pytest.mark.parametrize("early,late", [(8, 10), (5, 700), (100, 1500)], ids=["thread", "block", "blocks"])
def test_fasta_order_across_the_two_paths(early, late, early_deferred):
    # two eligible reads in 1600: `early` on the second contig, `late` back on the first, one on each path
    ref = pp.reference()
    recs = []
    for i in range(1600):
        if i == early:
            recs.append(pp.deferred(i, 100 + i, kind=pp.UNCLIPPED[i % 5], rid=1) if early_deferred else pp.common(i, 100 + i, rid=1))
        elif i == late:
            recs.append(pp.common(i, 100 + i, rid=0) if early_deferred else pp.deferred(i, 100 + i, kind=pp.UNCLIPPED[i % 5], rid=0))
        else:
            recs.append(_quiet(i, 100 + i, i % 5 == 0, rid=0 if i < early else 1))
    cols = synth.concat(recs)
    for i in (early, late):  # both eligible by their CIGARs: no clipped base
        w = cols["cigar"][int(cols["n_cigar"][:i].sum()):int(cols["n_cigar"][:i + 1].sum())]
        assert not np.isin(w & 15, (4, 5)).any()
    assert (cols["n_cigar"][early] > 1) == early_deferred and (cols["n_cigar"][late] > 1) != early_deferred
    rc, _, _ = run_oracle([cols], [ref, ref], n_refs=2)
    assert rc == ERR_FASTA
    _fails_at(cols, [ref, ref], late, n_refs=2)


@pytest.mark.parametrize("on_deferred", [True, False])
def test_read_longer_than_max_read_len(on_deferred):
    long_ops = [(600, "M"), (2, "D"), (500, "M")] if on_deferred else [(1100, "M")]
    recs = [pp.read(i, 100 + 10 * i, long_ops, length=1100) if i == 6 else (pp.common if on_deferred else pp.deferred)(i, 100 + 10 * i) for i in range(12)]
    cols = synth.concat(recs)
    rc, _, _ = run_oracle([cols], [pp.reference()], n_refs=1, max_read_len=1024)
    assert rc == ERR_RANGE
    _fails_at(cols, [pp.reference()], 6, n_refs=1, max_read_len=1024)


# ---------------------------------------------------------------------------------------------------------------------------------
# a shard
# ---------------------------------------------------------------------------------------------------------------------------------
def test_shard_whose_first_reads_are_set_aside():
    """Two workers on one card: the stream's head through a plain context, its tail through a shard_tail context.  The reads are
    dense on one contig, so nothing resets the windows: every read of the tail is set aside (BQC_COV_PENDING), one in eight of them
    and the quads of the 16 patterns with several operations.  Resolved from the head's state, the two state vectors add up to the
    single worker's, word for word."""
    lib = _lib.load()
    cols, ref = pp.pattern_batch(), pp.reference()
    n = len(cols["flag"])
    head, tail = synth.slice_batch(cols, 0, 5 * 1024 + 2), synth.slice_batch(cols, 5 * 1024 + 2, n)
    assert (tail["n_cigar"][:64] > 1).any()

    def ctx(**opts):
        a = Aggregator(n_refs=1, **opts)
        a.set_reference(0, ref)
        return a

    single, pred, succ = ctx(), ctx(), ctx(shard_tail=1)
    try:
        single.submit(cols)
        pred.submit(head)
        succ.submit(tail)
        buf = np.zeros(int(lib.bqc_shard_state_bytes(pred.h)), np.uint8)
        assert lib.bqc_shard_export(pred.h, buf.ctypes.data_as(C.c_void_p)) == 0, (lib.bqc_last_error(pred.h) or b"").decode()
        assert lib.bqc_shard_resolve(succ.h, buf.ctypes.data_as(C.c_void_p)) == 0, (lib.bqc_last_error(succ.h) or b"").decode()
        want, got = single.state_export_host(), pred.state_export_host() + succ.state_export_host()
        assert np.array_equal(want, got), np.flatnonzero(want != got)[:10]
        rc, co, _ = run_oracle([cols], [ref], n_refs=1)
        assert rc == 0
        d = _abi.diff_counts(co, single.finalize())
        assert not d, "\n".join(d[:10])
    finally:
        for a in (single, pred, succ):
            a.close()
