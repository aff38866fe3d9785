"""GPU: the per-read statistics (bamqc_amd/csrc/read_stats.h: the flag cascade, read length, mapping quality, mismatch, deletion and
insertion counts, soft clips by cycle, insert size) at the ends of their LDS tables and at their caps, through the C ABI, against the
oracle over every key AND against the restatement of tests/rs_ref.py over the keys it models.  Every comparison is integer equality.

Every batch of tests/rs_steps.py (tests/test_read_stats_cpu.py asserts that each reaches its seam and that oracle and restatement
agree on it) runs twice: in this process, where reads of at most 255 bases take k_short<15> (phase A, a lane per read) and longer ones
k_reads, and in one child process with BQC_NO_FAST=1 (read once per process), where every read takes k_reads (a thread per read).
A batch that must end the run is compared by its error code; the same context then takes a clean batch after reset().

Which batch catches which mutation of read_stats.h (by the LDS map: per mate [readnr][readlen 305][mapq 256][mm 64][del 64][ins 64]
[sc5 305][sc3 305], then [insert 1024]; every mutated kernel still ends cleanly, the word behind a table lies inside RS_WORDS):
  `bin < cap` -> `bin <= cap` in rs_hist       bins: a count of 64 lands in word 0 of the next table (mismatch 64 in deletions 0, deletion
                                               64 in insertions 0, insertion 64 in the 5' clip histogram) and is missing from its own bin
                                               (lengths likewise: a read of 305 bases lands in word 0 of the mapping qualities)
  the sign extension in rs_flush dropped       clip_cancel, through the state vector alone: word 100 of the second mates' difference array
                                               nets -140 and would be added as 2^32 - 140.  NO count shows that: the finalize takes the
                                               prefix sums mod 2^32 (the reference's `unsigned`), and so does everything else that reads
                                               these words.  The exported state vector does: each clipped read adds +1 and -1, so the
                                               words of the difference array sum to 0 mod 2^64, and the vector's sum equals that of the
                                               same reads with an insertion where the clip is (test_clip_words_sum_to_zero)
  `lds[i] = 0` removed from rs_flush           flush_reuse: read group 1 receives the even bins of group 0, group 2 the odd bins of group 1
A build with the three mutations fails bins, lengths, clips (a read of 305 bases), the three flush_reuse runs and
test_clip_words_sum_to_zero with wrong counts, and passes the rest.

What these batches do not reach:
  - read_stats_counted's path `gl = live && !use_lds` ("other lane inside a mixed wave"): both callers pass use_lds == live and chunks
    hold one read group, so no batch can reach it.
  - the carry of totalbps' low LDS word (word 14 into word 15): it needs more than 2^32 summed bases in one workgroup between two
    flushes.
  - a workgroup that RETURNS to a read group within a launch: the processing order is grouped by read group, so a workgroup meets read
    groups in rising order only (tests/rs_steps.py, flush_reuse); the second part of a group comes with the next submit."""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

from bamqc_amd import Aggregator, BamQCError, _abi
from tests import rs_ref, rs_steps
from tests.parity import run_oracle, split
from tests.test_gpu_value_limits import n_cu

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_batches(cols_list, refs, opts):
    """(code, counts or None, code and counts of the clean batch through the same context after reset())."""
    a = Aggregator(**opts)
    try:
        for cols in cols_list:
            a.submit(cols)
        rc, counts = 0, a.finalize()
    except BamQCError as e:
        rc, counts = e.code, None
    a.reset()
    try:
        a.submit(rs_steps.clean()[0])
        after = (0, a.finalize())
    except BamQCError as e:
        after = (e.code, None)
    a.close()
    return rc, counts, after


def runs(cu):
    """Every run of this file by name: (list of column dicts, refs, opts)."""
    out = {}
    for name in rs_steps.BATCHES:
        cols, refs, opts = rs_steps.made(name)
        out[name] = ([cols], refs, opts)
    for name in rs_steps.SPLIT:
        cols, refs, opts = rs_steps.made(name)
        out[name + "/split"] = (split(cols, [(len(cols["flag"]) // 2) | 1]), refs, opts)
    cols, refs, opts = rs_steps.made_flush(cu)
    shuffled = rs_steps.made_flush(cu, True)[0]
    out["flush_reuse"] = ([cols], refs, opts)
    out["flush_reuse/shuffled"] = ([shuffled], refs, opts)
    out["flush_reuse/twice"] = ([cols, shuffled], refs, opts)
    return out


RUNS = list(rs_steps.BATCHES) + [n + "/split" for n in rs_steps.SPLIT] + ["flush_reuse", "flush_reuse/shuffled", "flush_reuse/twice"]

_CHILD = r"""
import pickle, sys
sys.path.insert(0, sys.argv[1])
from tests import test_gpu_read_stats as t
out = {name: t.run_batches(*run) for name, run in t.runs(t.n_cu()).items()}
pickle.dump(out, open(sys.argv[2], "wb"))
"""


@pytest.fixture(scope="module")
def cu():
    return n_cu()


@pytest.fixture(scope="module")
def all_runs(cu):
    return runs(cu)


@pytest.fixture(scope="module")
def no_fast_results(tmp_path_factory):
    """Every run with every read on k_reads: one child process with BQC_NO_FAST=1."""
    path = str(tmp_path_factory.mktemp("read_stats") / "child.pkl")
    env = dict(os.environ, BQC_NO_FAST="1")
    out = subprocess.run([sys.executable, "-c", _CHILD, ROOT, path], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    return pickle.load(open(path, "rb"))


_expected, _restated = {}, {}


def expected(name, run):
    """(code, the oracle's counts, the restatement's counts) of a run, computed once; the clean batch's likewise under "clean"."""
    if name not in _expected:
        cols_list, refs, opts = run
        rc_o, want, _ = run_oracle(cols_list, refs, **opts)
        if name.startswith("flush_reuse"):  # the batch, the same reads in another order, and both: the same counts, and twice the counts
            if "flush_reuse" not in _restated:
                _restated["flush_reuse"] = rs_ref.counts(cols_list[:1], **opts)
            rc_r, once = _restated["flush_reuse"]
            ref = [{key: v if key.endswith("n_cycles") else len(cols_list) * v for key, v in c.items()} for c in once]
        else:
            rc_r, ref = rs_ref.counts(cols_list, **opts)
        assert rc_r == rc_o
        if rc_o == 0:
            d = rs_ref.diff(ref, want)
            assert not d, "restatement against the oracle:\n" + "\n".join(d[:20])
        _expected[name] = (rc_o, want, ref)
    return _expected[name]


def check(what, name, run, got):
    rc_o, want, ref = expected(name, run)
    rc_g, counts, after = got
    assert rc_g == rc_o, "%s: error code %d, the oracle's is %d" % (what, rc_g, rc_o)
    assert rc_o == (rs_steps.BATCHES[name][1] if name in rs_steps.BATCHES else 0)
    if rc_o == 0:
        d = _abi.diff_counts(want, counts)
        assert not d, "%s against the oracle:\n" % what + "\n".join(d[:20])
        d = rs_ref.diff(ref, counts)
        assert not d, "%s against the restatement:\n" % what + "\n".join(d[:20])
    # the same context after reset(): neither the error word nor anything counted before outlives it
    cols, refs, opts = rs_steps.clean()
    rc_c, want_c, ref_c = expected("clean/%r" % sorted(run[2].items()), ([cols], refs, run[2]))  # (once per set of options)
    assert (rc_c, after[0]) == (0, 0), "%s: the clean batch after reset() ends with %d" % (what, after[0])
    d = _abi.diff_counts(want_c, after[1]) + rs_ref.diff(ref_c, after[1])
    assert not d, "%s, the clean batch after reset():\n" % what + "\n".join(d[:20])


@pytest.mark.parametrize("name", RUNS)
def test_read_stats(name, all_runs, no_fast_results):
    assert "BQC_NO_FAST" not in os.environ and "BQC_SHORT_PARTS" not in os.environ  # this process runs k_short<15>
    run = all_runs[name]
    check("k_short / k_reads", name, run, run_batches(*run))
    check("k_reads alone (BQC_NO_FAST=1)", name, run, no_fast_results[name])


def test_clip_words_sum_to_zero():
    """A 3' clip adds +1 and -1 to the difference array, in LDS as wrapping 32-bit words that rs_flush must sign-extend: the array's
    64-bit words then sum to 0 mod 2^64, and the whole state vector sums to what the same reads give with an insertion in the clip's
    place (the same bases, positions and covered intervals; a read moves between two bins of the insertion histogram).  Without the
    sign extension every word with a negative net adds 2^32 to the sum, which no count shows (they are taken mod 2^32)."""
    sums = []
    for op in "SI":
        cols, refs, opts = rs_steps.clip_cancel(op)
        a = Aggregator(**opts)
        a.submit(cols)
        v = a.state_export_host()
        sums.append(int(v.sum(dtype=np.uint64)))
        a.close()
    assert sums[0] == sums[1]


def test_flush_reuse_crosses_read_groups(cu, all_runs):
    """By the launch rules restated in tests/rs_steps.py, for the card's CU count: a workgroup of k_short and a workgroup of k_reads
    (in the child) walk a chunk of read group 0, then one of group 1, then one of group 2 in one launch, in either order of the batch."""
    for name in ("flush_reuse", "flush_reuse/shuffled"):
        short, reads = rs_steps.flush_crossings(all_runs[name][0][0], cu)
        assert short and reads, (name, cu)
    want = expected("flush_reuse", all_runs["flush_reuse"])[2]
    for g, c in enumerate(want):  # read groups 0 and 2 fill even bins only, read group 1 odd bins only
        for key in ("r1.readLength", "r2.mapQ", "r1.mismatch", "r2.delhist", "r1.inshist", "r1.insertSize"):
            assert c[key][g & 1::2].sum() > 0 and not c[key][1 - (g & 1)::2].any(), (g, key)
