"""GPU: the window state machine of OverallNumbers::coverage (OverallNumbers.hpp:84-110) on the card for contexts with SEVERAL read
groups (csrc/k_anchor.hip: one state per read group, candidates compacted by read group; include/bamqc.h: bqc_anchor_*), against a
restatement of the recurrence with one state per read group, read by read, and — through bqc_submit_anchored — against the host's pass
(bqc_submit) and the oracle on the same batches; then the program with the reader on the card on files with several read groups."""
import ctypes as C
import filecmp
import os
import re
import subprocess

import numpy as np
import pytest

from bamqc_amd import Aggregator, BamQCError, _abi, _lib, hostio, synth
from tests import synth as tsynth
from tests.anchor_recurrence import NO_WIN, per_group_anchors
from tests.cli_oracle import oracle_bamqualcheck
from tests.hipmem import Hip
from tests.parity import run_oracle
from tests.test_gpu_anchor import device_batch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "bin", "bamqualcheck")


def enqueue(lib, agg, hip, cols):
    """bqc_anchor_enqueue + bqc_anchor_complete: (enqueue's rc, complete's rc, device batch, handle, anchors)"""
    b, d_cov = device_batch(hip, cols)
    h = C.c_void_p()
    rc = lib.bqc_anchor_enqueue(agg.h, C.byref(b), d_cov, None, C.byref(h))
    if rc:
        return rc, None, b, None, None
    assert hip.rt.hipDeviceSynchronize() == 0
    rc2 = lib.bqc_anchor_complete(agg.h, h, None)
    cov = hip.get(d_cov, 8 * len(cols["flag"]), np.uint32).reshape(-1, 2) if rc2 == 0 else None
    return 0, rc2, b, h, cov


def finalize(agg):
    try:
        return agg.finalize()
    except BamQCError as e:
        return e.code


def contexts(refs, n_lanes, **opts):
    out = []
    for _ in range(2):
        a = Aggregator(n_refs=len(refs), n_lanes=n_lanes, max_read_len=1024, **opts)
        for i, r in enumerate(refs):
            a.set_reference(i, r)
        out.append(a)
    return out


def run_stream(batches, refs, n_lanes, may_fail=False, state_words=False, **opts):
    """every batch anchored on the card (checked read by read) and submitted anchored; a second context gets the same batches through
    bqc_submit; both against each other and against the oracle (state_words: the two contexts' exported state vectors are compared
    word by word as well, before they are finalised)"""
    lib = _lib.load()
    hip = Hip()
    n_refs = len(refs)
    try:
        dev, host = contexts(refs, n_lanes, **opts)
        states = [(True, 0, 0, 0)] * n_lanes
        for cols in batches:
            rc, rc2, b, h, cov = enqueue(lib, dev, hip, cols)
            assert rc == 0, (rc, (lib.bqc_anchor_error(dev.h) or b"").decode())
            assert rc2 == 0, (rc2, (lib.bqc_anchor_error(dev.h) or b"").decode())
            win, off, states = per_group_anchors(cols, states, n_lanes, n_refs)
            got = cov[:, 0].astype(np.uint64)
            assert np.array_equal(got, win), np.flatnonzero(got != win)[:10]
            cand = win != NO_WIN
            assert np.array_equal(cov[cand, 1], off[cand]), np.flatnonzero(cov[cand, 1] != off[cand])[:10]
            rc = lib.bqc_submit_anchored(dev.h, C.byref(b), h, None)
            assert rc == 0 or may_fail, (lib.bqc_last_error(dev.h) or b"").decode()
            try:
                dev.sync()  # (the columns' device buffers are released after the test: the batch must be through)
                host.submit(cols)
            except BamQCError:
                assert may_fail
        if state_words:
            v_dev, v_host = dev.state_export_host(), host.state_export_host()
            assert np.array_equal(v_dev, v_host), np.flatnonzero(v_dev != v_host)[:10]
        res = [finalize(dev), finalize(host)]
        if isinstance(res[0], int) or isinstance(res[1], int):
            assert res[0] == res[1] and may_fail, res
        else:
            diffs = _abi.diff_counts(res[1], res[0])
            assert not diffs, diffs[:10]
            rc, want, _ = run_oracle(batches, refs, n_refs=n_refs, n_lanes=n_lanes, max_read_len=1024, **opts)
            assert rc == 0
            diffs = _abi.diff_counts(want, res[0])
            assert not diffs, diffs[:10]
        dev.close()
        host.close()
    finally:
        hip.free()


def with_lanes_positions(cols, lane=None, pos=None, rid=None, flag_or=0):
    c = dict(cols)
    for k in ("flag", "lane", "pos", "rid"):
        c[k] = np.array(cols[k], copy=True)
    if lane is not None:
        c["lane"] = np.asarray(lane, np.uint8)
    if pos is not None:
        c["pos"] = np.asarray(pos, np.int64).astype(np.int32)
    if rid is not None:
        c["rid"] = np.asarray(rid, np.int32)
    c["flag"] = (c["flag"] | flag_or).astype(np.uint16)
    return c


def split(cols, k):
    n = len(cols["flag"])
    cuts = [n * j // k for j in range(k + 1)]
    return [tsynth.slice_batch(cols, cuts[j], cuts[j + 1]) for j in range(k)]


LENS = [3_000_000, 2_000_000]


def refs_for(seed, lens=LENS):
    return [synth.reference(seed, i, ln) for i, ln in enumerate(lens)]


def case_batches(kind, rng):
    refs = refs_for(5)
    if kind == "dense":  # interleaved read groups, sorted positions, over both contigs
        return split(synth.batch(5, 90_000, LENS, refs, n_lanes=4), 3), refs, 4
    if kind == "sparse_one_group":  # group 3 with gaps around 1000 and 2000 beside dense groups: breaks in one group only
        base = synth.batch(6, 40_000, LENS[:1], refs[:1], n_lanes=1)
        n = len(base["flag"])
        i = np.arange(n)
        lane = np.where(i % 20 == 3, 3, i % 3)
        pos = np.sort(rng.integers(0, 2_900_000, size=n))
        k3 = np.flatnonzero(lane == 3)
        gaps = rng.choice([3, 400, 999, 1000, 1001, 1500, 1999, 2000, 2001, 2600], size=len(k3))
        pos[k3] = np.minimum(np.cumsum(gaps), 2_900_000)
        c = with_lanes_positions(base, lane=lane, pos=pos)
        return split(c, 2), refs[:1], 4
    if kind == "late_and_absent":  # group 3 first appears in the third batch; group 1 is absent from the second and carried unchanged
        base = synth.batch(7, 48_000, LENS, refs, n_lanes=3)
        b = split(base, 4)
        b[1] = with_lanes_positions(b[1], lane=np.where(b[1]["lane"] == 1, 0, b[1]["lane"]))
        b[2] = with_lanes_positions(b[2], lane=np.where(np.arange(len(b[2]["flag"])) % 5 == 0, 3, b[2]["lane"]))
        n2 = len(b[2]["flag"])  # a batch without one candidate (every record secondary), from the tail of the one before
        b.insert(3, with_lanes_positions(tsynth.slice_batch(b[2], n2 - 200, n2), flag_or=0x100))
        return b, refs, 4
    if kind == "stuck":  # group 1 stuck at offset 2000 across a batch end; group 0 dense beside it
        base = synth.batch(8, 30, LENS[:1], refs[:1], n_lanes=1)
        p1 = [[100, 2100, 2100, 2100, 2100], [2100, 2100, 2101, 4101, 4101], [4101, 4500, 6000]]
        out, at = [], 0
        for k, ps in enumerate(p1):
            n = 2 * len(ps)
            lane = np.array([0, 1] * len(ps), np.uint8)
            pos = np.empty(n, np.int64)
            pos[1::2] = ps
            pos[0::2] = at + np.arange(len(ps)) * 7
            at += 50
            if k == 0:
                pos[2 * 3] = 300  # (a group-0 read further back: a break of group 0 only)
            c = with_lanes_positions(tsynth.slice_batch(base, 0, n), lane=lane, pos=pos)
            c["flag"] = ((c["flag"] & ~np.uint16(0xD04)) | np.uint16(0x40)).astype(np.uint16)  # (every read a candidate)
            out.append(c)
        return out, refs[:1], 2
    if kind == "wild":  # unsorted and wild records, 40 groups
        from tests.test_gpu_fuzz import wild_batch
        cols, wrefs = wild_batch(93, 16_000, n_lanes=40)
        cols = {k: v for k, v in cols.items() if not k.startswith("nm_extra")}
        return split(cols, 2), wrefs, 40
    if kind == "many_groups":  # the n_lanes maximum, a few reads each
        base = synth.batch(9, 3_000, LENS, refs, n_lanes=1)
        lane = rng.integers(0, 256, size=len(base["flag"]))
        return split(with_lanes_positions(base, lane=lane), 2), refs, 256
    raise ValueError(kind)


@pytest.mark.parametrize("kind", ["dense", "sparse_one_group", "late_and_absent", "stuck", "wild", "many_groups"])
def test_per_group_anchors_equal_the_recurrence_the_host_pass_and_the_oracle(kind):
    batches, refs, n_lanes = case_batches(kind, np.random.default_rng(11))
    run_stream(batches, refs, n_lanes, may_fail=kind == "wild")


def test_sketch_and_8mers_of_every_group():
    """k-mer sketch (k = 5, 31) and the quality 8-mers of every read group: lane_count, lane_bits and the folds of each group"""
    refs = refs_for(12)
    batches = split(synth.batch(12, 60_000, LENS, refs, n_lanes=5), 3)
    run_stream(batches, refs, 5, klist=[5, 31], qlist=[17])


def test_lane_out_of_range_is_the_same_error():
    """a read whose lane is >= n_lanes: the same error code and message through bqc_submit_anchored as through bqc_submit"""
    lib = _lib.load()
    refs = refs_for(13)
    cols = synth.batch(13, 20_000, LENS, refs, n_lanes=4)
    lane = np.array(cols["lane"], copy=True)
    lane[[700, 9_000]] = [4, 200]
    cols = with_lanes_positions(cols, lane=lane)
    hip = Hip()
    try:
        dev, host = contexts(refs, 4)
        rc, rc2, b, h, cov = enqueue(lib, dev, hip, cols)
        assert (rc, rc2) == (0, 0), (lib.bqc_anchor_error(dev.h) or b"").decode()
        got = []
        for agg, submit in ((dev, lambda: lib.bqc_submit_anchored(dev.h, C.byref(b), h, None)), (host, None)):
            try:
                if submit:
                    rc = submit()
                    if rc:
                        raise BamQCError(rc, (lib.bqc_last_error(dev.h) or b"").decode())
                else:
                    agg.submit(cols)
                agg.finalize()
                got.append(None)
            except BamQCError as e:
                got.append((e.code, str(e)))
        assert got[0] is not None and got[0] == got[1], got
        assert "lane" in got[0][1]
        dev.close()
        host.close()
    finally:
        hip.free()


def test_too_many_breaks_in_one_group_leave_every_group_to_the_host():
    """more breaks than the card's chain takes (AN_MAX_BREAKS = 16 384, over the batch), all in one read group: bqc_anchor_complete says 1,
    no group's state moves, the next enqueue says 1, and the rest through bqc_submit equals a host-only stream"""
    lib = _lib.load()
    lens = [30_000_000]
    refs = refs_for(14, lens)
    rng = np.random.default_rng(4)
    dense_at = lambda cols, lo: with_lanes_positions(cols, pos=np.sort(rng.integers(lo, lo + 2_000_000, size=len(cols["flag"]))))
    first = dense_at(synth.batch(14, 40_000, lens, refs, n_lanes=3), 0)
    base = synth.batch(15, 60_000, lens, refs, n_lanes=1)
    n = len(base["flag"])
    lane = np.where(np.arange(n) % 3 == 2, 2, np.arange(n) % 2).astype(np.uint8)
    pos = np.sort(rng.integers(2_000_000, 4_000_000, size=n))
    k2 = np.flatnonzero(lane == 2)  # 20 000 reads 1200 apart: every one a break
    pos[k2] = np.arange(len(k2)) * 1200 + 2_000_007
    sparse = with_lanes_positions(base, lane=lane, pos=pos)
    after = dense_at(synth.batch(16, 30_000, lens, refs, n_lanes=3), 27_000_000)
    hip = Hip()
    try:
        dev, host = contexts(refs, 3)
        rc, rc2, b, h, cov = enqueue(lib, dev, hip, first)
        assert (rc, rc2) == (0, 0)
        assert lib.bqc_submit_anchored(dev.h, C.byref(b), h, None) == 0
        rc, rc2, _, _, _ = enqueue(lib, dev, hip, sparse)
        assert (rc, rc2) == (0, 1)
        dev.submit(sparse)
        rc, _, _, _, _ = enqueue(lib, dev, hip, after)
        assert rc == 1
        dev.submit(after)
        for cols in (first, sparse, after):
            host.submit(cols)
        diffs = _abi.diff_counts(host.finalize(), dev.finalize())
        assert not diffs, diffs[:10]
        dev.close()
        host.close()
    finally:
        hip.free()


def test_reset_starts_every_read_group_over_on_the_card():
    """three read groups: an anchored batch that leaves every group on the second contig, bqc_reset, then a second anchored stream that
    starts on the first contig — every group's first read is a FIRST read again (not a reset out of the windows of the stream before:
    two windows flushed too many), so anchors and final counts equal those of a fresh context given only the second stream"""
    lib = _lib.load()
    refs = refs_for(17)
    before = synth.batch(17, 30_000, LENS, refs, n_lanes=3)
    stream = split(synth.batch(18, 40_000, LENS, refs, n_lanes=3), 2)
    hip = Hip()
    try:
        used, fresh = contexts(refs, 3)
        rc, rc2, b, h, _ = enqueue(lib, used, hip, before)
        assert (rc, rc2) == (0, 0), (lib.bqc_anchor_error(used.h) or b"").decode()
        assert lib.bqc_submit_anchored(used.h, C.byref(b), h, None) == 0
        used.sync()
        used.reset()
        for agg in (used, fresh):
            states = [(True, 0, 0, 0)] * 3
            for cols in stream:
                rc, rc2, b, h, cov = enqueue(lib, agg, hip, cols)
                assert (rc, rc2) == (0, 0), (lib.bqc_anchor_error(agg.h) or b"").decode()
                win, off, states = per_group_anchors(cols, states, 3, len(refs))
                got = cov[:, 0].astype(np.uint64)
                assert np.array_equal(got, win), (agg is used, np.flatnonzero(got != win)[:10])
                cand = win != NO_WIN
                assert np.array_equal(cov[cand, 1], off[cand])
                assert lib.bqc_submit_anchored(agg.h, C.byref(b), h, None) == 0, (lib.bqc_last_error(agg.h) or b"").decode()
                agg.sync()
        diffs = _abi.diff_counts(fresh.finalize(), used.finalize())
        assert not diffs, diffs[:10]
        used.close()
        fresh.close()
    finally:
        hip.free()


def run_program(args, **env):
    r = subprocess.run([EXE] + list(args), capture_output=True, text=True, env=dict(os.environ, **env), timeout=600)
    assert r.returncode == 0, r.stderr
    return r


def anchored_batches(stderr):
    m = re.findall(r"\[timing\] (\d+) batches anchored on the card \(fixed columns never on the host\) of (\d+) batches", stderr)
    assert m, stderr
    return [(int(a), int(b)) for a, b in m]


def test_program_keeps_a_three_read_group_file_on_the_card(tmp_path):
    """three read groups over two contigs, small batches, the reader on the card: every batch anchored there; the same bytes as the
    host's pass (BQC_DEVICE_ANCHORS=0), the host reader and the oracle program"""
    bam, fa = str(tmp_path / "rg3.bam"), str(tmp_path / "rg3.fa")
    hostio.synth_write(bam, fa, seed=41, n_reads=60_000, ref_names=["chr1", "chr2"], ref_lens=[2_000_000, 1_000_000], n_lanes=3)
    common = ["-r", fa, "-c", "chr1,chr2", "--batch-reads", "9000", bam]
    outs = {}
    for name, env in (("card", {"BQC_GPU_DECODE": "1", "BQC_TIMING": "1"}), ("host_pass", {"BQC_GPU_DECODE": "1", "BQC_TIMING": "1", "BQC_DEVICE_ANCHORS": "0"}),
                      ("host_reader", {"BQC_GPU_DECODE": "0"})):
        outs[name] = str(tmp_path / (name + ".bamqc"))
        r = run_program(["-o", outs[name]] + common, **env)
        if name == "card":
            [(k, total)] = anchored_batches(r.stderr)
            assert total >= 5 and k == total, r.stderr
        if name == "host_pass":
            assert anchored_batches(r.stderr)[0][0] == 0
    want = str(tmp_path / "oracle.bamqc")
    assert oracle_bamqualcheck(bam, fa, want, chroms="chr1,chr2", batch_reads=9000) == 0
    for name, got in outs.items():
        assert filecmp.cmp(got, want, shallow=False), name


def test_program_two_workers_two_read_groups(tmp_path):
    """--gpus 2 on one card with two read groups: the same bytes as the single-process run; worker 0 (the head of the stream) anchors
    on the card, the worker that starts inside the stream keeps its anchors on the host (out of scope there)"""
    bam, fa = str(tmp_path / "rg2.bam"), str(tmp_path / "rg2.fa")
    hostio.synth_write(bam, fa, seed=42, n_reads=200_000, ref_names=["chr1", "chr2", "chrM"], ref_lens=[2_000_000, 400_000, 20_000], n_lanes=2)
    single = str(tmp_path / "single.bamqc")
    run_program(["-r", fa, "-o", single, "-c", "chr1,chr2", bam], BQC_GPU_DECODE="1")
    out = str(tmp_path / "two.bamqc")
    r = run_program(["--gpus", "2", "-r", fa, "-o", out, "-c", "chr1,chr2", "--batch-reads", "20011", bam],
                    BQC_GPUS_SHARE_DEVICE="1", BQC_GPU_DECODE="1", BQC_TIMING="1")
    assert filecmp.cmp(single, out, shallow=False)
    counts = anchored_batches(r.stdout + r.stderr)
    assert len(counts) == 2 and max(k for k, _ in counts) > 0, counts
