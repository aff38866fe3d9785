"""GPU: the k-mer sketch at error rates other than the default 0.01 (-e / --error-rate), against the oracle.

The reference sizes its StreamCounter from e (StreamCounter.hpp:25-46): an F2 table of roundUpPowerOfTwo(2/e^2 + 1) entries and
roundUpPowerOfTwo(max(8192, 48/e^2 + 1) / 16) * 16 counters per level.  k_sketch keeps F2 tables of up to 32768 entries in LDS
(e >= ~0.0079) and adds to the global table otherwise; the cases below cover the 8192-counter floor (0.2), small LDS tables,
the last sizes on both sides of 32768 entries (0.0079: 32768, 0.0078: 65536) and the global path (0.005, 0.002).

The oracle's F0 / f1 (as the reference's) rescan every level for each of up to ~40 limits while no level is 20 % full, so a
sketch with few distinct k-mers (k = 5 has at most 1024) costs seconds per million counters on the host: e = 0.002 (16 M
counters per level) runs k = 32 only, on enough distinct k-mers to stop after a few limits."""
import os
import subprocess

import numpy as np
import pytest

from bamqc_amd import BamQCError, synth as csynth
from tests.parity import assert_parity, run_gpu, split

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "bin", "bamqualcheck")


def _input(seed, n_reads=40_000, lens=(1_500_000, 500_000)):
    """two read groups, qualities raised to >= 35 except for one base in fifty (restarts for q = 30, some for q = 17)"""
    refs = [csynth.reference(seed, i, n) for i, n in enumerate(lens)]
    cols = csynth.batch(seed, n_reads, lens, refs, n_lanes=2)
    rng = np.random.default_rng(seed)
    q = np.maximum(cols["qual"], 35).astype(np.uint8)
    low = rng.random(q.size) < 0.02
    q[low] = cols["qual"][low]
    cols["qual"] = np.where(cols["qual"] == 0xFF, 0xFF, q).astype(np.uint8)
    return cols, refs


def _cuts(cols):
    n = len(cols["flag"])
    return [n // 5, n // 2, (4 * n) // 5]


@pytest.mark.parametrize("e", [0.2, 0.05, 0.02, 0.0111, 0.0079, 0.0078, 0.005])
def test_sketch_parity_at_error_rate(e):
    cols, refs = _input(41)
    co, cg, _, _ = assert_parity(split(cols, _cuts(cols)), refs, n_lanes=2, klist=[5, 32], qlist=[17, 30], e=e)
    for lane in cg:
        assert len(lane["sketch"]) == 4 and all(s[2] > 0 for s in lane["sketch"])


def test_sketch_parity_at_error_rate_0_002_global_f2():
    cols, refs = _input(42, n_reads=150_000, lens=(5_000_000, 3_000_000))
    assert_parity(split(cols, _cuts(cols)), refs, n_lanes=2, klist=[32], qlist=[17, 30], e=0.002)


def test_error_rate_changes_f2():
    cols, refs = _input(43, n_reads=10_000)
    rc1, c1, _ = run_gpu([cols], refs, n_refs=2, n_lanes=2, klist=[32], qlist=[17])
    rc2, c2, _ = run_gpu([cols], refs, n_refs=2, n_lanes=2, klist=[32], qlist=[17], e=0.05)
    assert rc1 == 0 and rc2 == 0
    for a, b in zip(c1, c2):
        (q, k, n, F0, f1, F2), (q2, k2, n2, F0b, f1b, F2b) = a["sketch"][0], b["sketch"][0]
        assert (q, k, n) == (q2, k2, n2) and n > 0  # same k-mers ...
        assert F2 != F2b  # ... counted into a 1024-entry F2 table instead of 32768 entries


@pytest.mark.parametrize("e", [0.05, 0.005])
def test_state_vectors_add_at_error_rate(e):
    """the state vector's sketch part at a non-default size: two contexts each take part of the reads (two batches each, cut where
    the chromosome changes), export; a fresh context imports the sum and finalises: the single context's result (and the oracle's)"""
    from bamqc_amd import Aggregator, _abi
    cols, refs = _input(44, n_reads=20_000)
    cut = int(np.argmax(cols["rid"] == 1))  # (reads in coordinate order, unmapped ones, rid -1, among them)
    parts = split(cols, [cut // 2, cut, (cut + len(cols["flag"])) // 2])
    opts = dict(n_refs=2, n_lanes=2, klist=[32], qlist=[17], e=e)
    co, cg, _, _ = assert_parity(parts, refs, **opts)
    total = None
    for half in (parts[:2], parts[2:]):
        a = Aggregator(**opts)
        for i, r in enumerate(refs):
            a.set_reference(i, r)
        for p in half:
            a.submit(p)
        v = a.state_export_host()
        a.close()
        total = v if total is None else total + v
    m = Aggregator(**opts)
    assert m.state_words == len(total)
    m.state_import_host(total)
    d = _abi.diff_counts(cg, m.finalize())
    m.close()
    assert not d, d[:5]


def _free_bytes():
    import ctypes as C
    from tests.hipmem import Hip
    rt = Hip().rt
    free_b, total_b = C.c_size_t(), C.c_size_t()
    assert rt.hipMemGetInfo(C.byref(free_b), C.byref(total_b)) == 0
    return free_b.value


def test_arena_larger_than_the_card_is_refused_before_allocating():
    from bamqc_amd import Aggregator
    before = _free_bytes()
    # e = 0.0007: 2^27 counters per level (the largest supported), 16 GiB per (read group, k/q pair); 64 read groups: 1 TiB
    with pytest.raises(BamQCError) as ei:
        Aggregator(n_refs=1, n_lanes=64, klist=[32], qlist=[17], e=0.0007)
    msg = str(ei.value)
    assert "error rate 0.0007 needs" in msg and "bytes of sketch tables" in msg and "free" in msg, msg
    assert _free_bytes() >= before - (64 << 20)  # nothing of the arena was allocated (or left behind)
    with pytest.raises(BamQCError) as ei:  # 2^31 counters per level: beyond the 32-bit counter index
        Aggregator(n_refs=1, klist=[32], qlist=[17], e=1e-4)
    assert "below the smallest supported" in str(ei.value)
    with pytest.raises(BamQCError) as ei:
        Aggregator(n_refs=1, klist=[32], qlist=[17], e=0.0)
    assert "error rate must be > 0" in str(ei.value)
    cols, refs = _input(45, n_reads=2000)  # the card is fine afterwards
    assert_parity(cols, refs, n_lanes=2, klist=[32], qlist=[17], e=0.05)


# ---- the program: bamqualcheck -e

def _oracle_bamqc(bam, fasta, out, chroms, e):
    """tests/cli_oracle.py's oracle_bamqualcheck with the error rate passed on (that helper has no e)"""
    from bamqc_amd import hostio
    from tests.oracle_lib import Oracle
    f = hostio.BamFile(bam)
    main = np.array([1 if n in chroms.split(",") else 0 for n in f.ref_names], np.uint8)
    f.set_main_chrom(main)
    fa = hostio.load_fasta(fasta)
    fidx = np.full(max(1, len(f.ref_names)), -1, np.int32)
    for r, name in enumerate(f.ref_names):
        for i, (n, _) in enumerate(fa):
            if n == name:
                fidx[r] = i
                break
    o = Oracle(n_lanes=f.lane_count, n_refs=len(f.ref_names), isize=1000, main_chrom=main, fasta_index=fidx, max_read_len=65536,
               hist_cap=65536, klist=(32,), qlist=(17,), e=e)
    for r in range(len(f.ref_names)):
        if fidx[r] >= 0:
            o.reference(r, fa[fidx[r]][1])
    for cols in f.batches(max_reads=1 << 20):
        assert o.process(cols) == 0
    lanes = f.lanes()
    o.finalize()
    o.write_bamqc(out, sample_id=f.sample_id, lane_names=[n for n, _ in lanes], lane_index=[i for _, i in lanes])


def _split_sketch(path):
    lines = open(path).read().splitlines()
    sk = [l for l in lines if "_after_qual_clipping_" in l]  # count, distinct, unique, F2 of each (k, q)
    return sk, [l for l in lines if "_after_qual_clipping_" not in l]


@pytest.fixture(scope="module")
def cli_input(tmp_path_factory):
    from bamqc_amd import hostio
    d = tmp_path_factory.mktemp("cli_e")
    bam, fa = str(d / "e.bam"), str(d / "e.fa")
    hostio.synth_write(bam, fa, seed=1003, n_reads=20_000, ref_names=["chr1", "chr2"], ref_lens=[600_000, 400_000], n_lanes=2)
    default = str(d / "default.bamqc")
    r = subprocess.run([EXE, "-r", fa, "-o", default, "-c", "chr1,chr2", bam], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return d, bam, fa, default


@pytest.mark.parametrize("e", ["0.05", "0.005"])
def test_cli_error_rate_sketch_lines_match_the_oracle(cli_input, e):
    d, bam, fa, default = cli_input
    got, want = str(d / ("gpu_%s.bamqc" % e)), str(d / ("oracle_%s.bamqc" % e))
    r = subprocess.run([EXE, "-r", fa, "-o", got, "-c", "chr1,chr2", "-e", e, bam], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    _oracle_bamqc(bam, fa, want, "chr1,chr2", float(e))
    assert open(got).read() == open(want).read()
    sk, rest = _split_sketch(got)
    sk_default, rest_default = _split_sketch(default)
    assert len(sk) == len(sk_default) == 8 and sk != sk_default  # four sketch lines per read group; F2 sized from e
    assert rest == rest_default  # every other line as in the default run


@pytest.mark.parametrize("e,msg", [("0", "error rate must be > 0"), ("-1", "is smaller than the minimum value of 0")])
def test_cli_error_rate_refusals_unchanged(cli_input, e, msg):
    d, bam, fa, _ = cli_input
    r = subprocess.run([EXE, "-r", fa, "-o", str(d / "x.bamqc"), "-e", e, bam], capture_output=True, text=True)
    assert r.returncode == 1 and msg in r.stderr, (r.returncode, r.stderr)
