"""GPU: SAM text decoded on the card (csrc/gpu_sam.hip) against the host reader (SamReader) and the independent BAM decoder of
tests/pybam.py — identical columns whatever the batch and chunk sizes; lines of forms the card has no rule for go, a batch at a time,
through the host's line parser, which is also the one that words every error."""
import filecmp
import os
import re
import subprocess

import numpy as np
import pytest

from bamqc_amd import hostio
from tests import pybam, sam_sweeps
from tests.cli_oracle import oracle_bamqualcheck
from tests.test_gpu_reader import all_columns, same

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "bin", "bamqualcheck")


def read_all(path, batch_reads, **kw):
    """Columns of the whole file (further NM values with the index of their read in the FILE), batches, batches handed over, lanes."""
    b = hostio.BamFile(path, **kw)
    cols, n_batches, base, err = {}, 0, 0, None
    try:
        for batch in b.batches(batch_reads):
            n_batches += 1
            for k, v in batch.items():
                cols.setdefault(k, []).append(np.array(v, copy=True) + (base if k == "nm_extra_read" else 0))
            base += len(batch["flag"])
    except IOError as e:
        err = str(e)
    handed, lanes = b.batches_handed_over, b.lanes()
    b.close()
    return {k: np.concatenate(v) for k, v in cols.items()}, n_batches, handed, lanes, err


@pytest.fixture(scope="module")
def shapes(tmp_path_factory):
    """[(sam path, columns of the BAM file the text was written from)] for short reads on three contigs in two lanes, and long reads."""
    d = tmp_path_factory.mktemp("sam_shapes")
    out = {}
    for name, kw in (("short", dict(seed=31, n_reads=30_000, ref_names=["chr1", "chr2", "chrM"], ref_lens=[400_000, 250_000, 16_000], n_lanes=2)),
                     ("long", dict(seed=32, n_reads=300, ref_names=["chr1", "chr2"], ref_lens=[3_000_000, 2_000_000], read_len=9000, long_reads=True))):
        bam, sam = str(d / (name + ".bam")), str(d / (name + ".sam"))
        hostio.synth_stream(bam, None, **kw)
        cols, _ = all_columns(bam, 1 << 20)
        hostio.write_sam(sam, cols, kw["ref_names"], kw["ref_lens"], n_lanes=kw.get("n_lanes", 1))
        want = pybam.columns(bam, main_chrom=[0] * len(kw["ref_names"]))[0]
        host, _ = all_columns(sam, 1 << 20)
        same(want, host)  # (the host reader of SAM text against the independent decoder of the BAM file)
        out[name] = (sam, host)
    return out


@pytest.mark.parametrize("chunk_kb", [None, 64])
@pytest.mark.parametrize("shape", ["short", "long"])
def test_columns_equal_the_host_readers(shapes, monkeypatch, shape, chunk_kb):
    sam, host = shapes[shape]
    if shape == "long":
        assert host["n_cigar"].astype(int).mean() > 30
    if chunk_kb:
        monkeypatch.setenv("BQC_GS_CHUNK_KB", str(chunk_kb))
    for batch_reads in (777, 10_000, 1 << 20):
        got, nb, handed, _, err = read_all(sam, batch_reads, gpu=0)
        assert err is None and handed == 0 and nb >= 1
        same(host, got)


def test_every_offset_around_segment_and_chunk_boundaries(tmp_path, monkeypatch):
    path = str(tmp_path / "boundary.sam")
    n_probe = sam_sweeps.boundary(path)
    raw = open(path, "rb").read()
    starts = [m.start() for m in re.finditer(re.escape(sam_sweeps.PROBE.encode()), raw)]
    assert len(starts) == n_probe and raw[16384 - 1:16384 + 3] == b"\nf0\t"
    assert [s - (sam_sweeps.BOUNDARY_FIRST + i) * 65536 for i, s in enumerate(starts)] == [40 - i for i in range(n_probe)]
    host, _, _, _, err = read_all(path, 1 << 20)
    assert err is None and host["l_seq"].max() == 100_000 and host["n_cigar"].max() == 121
    for chunk_kb in (64, 16, None):
        if chunk_kb:
            monkeypatch.setenv("BQC_GS_CHUNK_KB", str(chunk_kb))
        else:
            monkeypatch.delenv("BQC_GS_CHUNK_KB")
        for batch_reads in (1 << 20, 5000):
            got, nb, handed, _, err = read_all(path, batch_reads, gpu=0)
            assert err is None and handed == 0
            same(host, got)


def test_wild_lines_stay_on_the_card_and_odd_ones_are_handed_over(tmp_path):
    path = str(tmp_path / "wild.sam")
    want = sam_sweeps.wild(path)
    host, _, _, _, _ = read_all(path, 777)
    for batch_reads in (777, 1 << 20):
        got, nb, handed, _, err = read_all(path, batch_reads, gpu=0)
        assert err is None and handed == 0
        same(host, got)
    for k in ("lane", "rid", "pos", "tlen", "nm", "as_", "seq", "qual", "cigar"):
        assert np.array_equal(got[k], want[k]), k
    # the odd lines, far enough apart to lie in batches of their own
    rng = np.random.default_rng(8)
    odd = sam_sweeps.odd_lines(rng)
    text = open(path, newline="").read() + "\n"
    k = 0
    for _, line in odd + [odd[2]]:  # (the read group learnt from the first line that names it is one of the table's the next time)
        text += "".join(sam_sweeps.plain_line(rng, "g%d" % (k + i)) + "\n" for i in range(3000)) + line + "\n"
        k += 3000
    text += "".join(sam_sweeps.plain_line(rng, "z%d" % i) + "\n" for i in range(3000))
    path2 = str(tmp_path / "odd.sam")
    open(path2, "w", newline="").write(text)
    host, _, _, host_lanes, err = read_all(path2, 777)
    assert err is None and len(host["nm_extra_read"]) == 1 and ("newcomer", 0) in host_lanes
    got, nb, handed, lanes, err = read_all(path2, 777, gpu=0)
    assert err is None and lanes == host_lanes
    same(host, got)
    assert handed == len(odd) and nb > 3 * handed  # (one batch per odd line; the repeated read group is decoded on the card)


@pytest.mark.parametrize("which", range(8))
def test_errors_are_the_host_readers(tmp_path, which):
    rng = np.random.default_rng(4)
    what, line, code, msg = sam_sweeps.bad_lines(rng)[which]
    good = [sam_sweeps.plain_line(rng, "g%d" % i) for i in range(5000)]
    path = str(tmp_path / "bad.sam")
    open(path, "w").write(sam_sweeps.header() + "\n".join(good[:2500] + [line] + good[2500:]) + "\n")
    host, _, _, _, host_err = read_all(path, 777)
    got, _, _, _, err = read_all(path, 777, gpu=0)
    assert host_err is not None and host_err.startswith("bam read error %d: %s" % (code, msg)), what
    assert err == host_err
    assert len(got["flag"]) == 2500 and 0 < len(host["flag"]) <= 2500  # the reads in front of it are delivered (all of them by the card)
    for k in host:
        assert np.array_equal(host[k], got[k][:len(host[k])]), k


def _program(sam_text, fa, out, decode, *args):
    return subprocess.run([EXE, "-r", fa, "-o", out] + list(args) + ["-"], input=sam_text, capture_output=True,
                          env=dict(os.environ, BQC_GPU_DECODE=decode, BQC_TIMING="1"))


def test_program_reads_a_stream_on_the_card(tmp_path):
    bam, fa = str(tmp_path / "m.bam"), str(tmp_path / "m.fa")
    names, lens = ["chr1", "chr2", "chrX", "chrUn_1"], [400_000, 300_000, 200_000, 50_000]
    hostio.synth_write(bam, fa, seed=7, n_reads=30_000, ref_names=names, ref_lens=lens, n_lanes=3)
    cols, _ = all_columns(bam, 1 << 20)
    sam = str(tmp_path / "m.sam")
    hostio.write_sam(sam, cols, names, lens, n_lanes=3)
    text = open(sam, "rb").read()
    args = ["-i", "500", "--batch-reads", "7001", "-k", "21,32", "-q", "10"]
    out_b, out_1, out_0, want = (str(tmp_path / x) for x in ("b.bamqc", "s1.bamqc", "s0.bamqc", "oracle.bamqc"))
    r = subprocess.run([EXE, "-r", fa, "-o", out_b] + args + [bam], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert oracle_bamqualcheck(bam, fa, want, isize=500, klist=(21, 32), qlist=(10,), batch_reads=4000) == 0
    q = _program(text, fa, out_1, "1", *args)
    assert q.returncode == 0, q.stderr
    m = re.search(rb"\[sam reader\] (\d+) batches on the card, (\d+) handed over, (\d+) anchored", q.stderr)
    assert m, q.stderr
    on_card, handed, anchored = (int(x) for x in m.groups())
    assert on_card >= 1 and handed == 0 and anchored == on_card
    assert filecmp.cmp(out_1, out_b, shallow=False) and filecmp.cmp(out_1, want, shallow=False)
    q = _program(text, fa, out_0, "0", *args)
    assert q.returncode == 0, q.stderr
    assert b"[sam reader]" not in q.stderr and filecmp.cmp(out_0, want, shallow=False)


def test_program_on_wild_text_hands_batches_over(tmp_path):
    """Records no aligner would write (tests/test_host_io.py: _wild_bam — junk tags of every type, further NM tags), as SAM text on
    stdin: the oracle's bytes, with batches that went through the host's line parser."""
    from tests.test_host_io import _wild_bam
    from tests.test_gpu_fuzz import wild_batch
    bam, fa = str(tmp_path / "w.bam"), str(tmp_path / "w.fa")
    _wild_bam(bam, 34, 1500)
    _, refs = wild_batch(34, 1)
    hostio.write_fasta(fa, ["chr%d" % (i + 1) for i in range(len(refs))], refs)
    text = pybam.bam_to_sam_text(bam).encode("latin-1")  # (qualities over the whole byte range: one byte each)
    sam = str(tmp_path / "w.sam")
    open(sam, "wb").write(text)
    same(all_columns(bam, 1 << 20)[0], all_columns(sam, 1 << 20)[0])  # (the text says what the BAM file says: no one-base read of Phred 9, whose QUAL would be "*")
    got, want = str(tmp_path / "gpu.bamqc"), str(tmp_path / "oracle.bamqc")
    args = ["-i", "2000", "--batch-reads", "300", "-k", "8,32", "-q", "17"]
    q = _program(text, fa, got, "1", *args)
    assert q.returncode == 0, q.stderr
    assert oracle_bamqualcheck(bam, fa, want, isize=2000, klist=(8, 32), qlist=(17,), batch_reads=999) == 0
    assert filecmp.cmp(got, want, shallow=False)
    m = re.search(rb"\[sam reader\] (\d+) batches on the card, (\d+) handed over", q.stderr)
    assert m and 0 < int(m.group(2)) <= int(m.group(1)), q.stderr
