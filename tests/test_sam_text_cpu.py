"""SAM text on the host: the writer (bqc_sam_write) against the independent converter of tests/pybam.py, and the line parser behind
SamReader (host/bam_io.cpp: SamLineParser — also what a batch handed over by the reader on the card goes through) against the
columns the generator of tests/sam_sweeps.py knows by construction."""
import numpy as np
import pytest

from bamqc_amd import hostio
from tests import pybam, sam_sweeps


def _read_all(path, batch_reads):
    b = hostio.BamFile(path)
    b.set_main_chrom(np.ones(len(b.ref_names), np.uint8))
    got = list(b.batches(batch_reads))
    lanes = b.lanes()
    b.close()
    return {k: np.concatenate([x[k] for x in got]) for k in got[0]}, lanes


def test_sam_writer_equals_the_independent_converter(tmp_path):
    names, lens = ["chr1", "chr2"], [300_000, 200_000]
    bam0, bam, sam = str(tmp_path / "a.bam"), str(tmp_path / "b.bam"), str(tmp_path / "b.sam")
    hostio.synth_write(bam0, None, seed=12, n_reads=2000, ref_names=names, ref_lens=lens, n_lanes=2)
    f = hostio.BamFile(bam0)
    cols = next(f.batches())
    f.close()
    qo = np.concatenate([[0], np.cumsum(cols["l_seq"].astype(np.int64))])
    for i in range(0, 2000, 17):  # reads without qualities
        cols["qual"][qo[i]:qo[i + 1]] = 0xFF
    cols["rid"][5] = -1  # an unplaced read
    hostio.write_bam(bam, cols, names, lens, n_lanes=2, first_read_index=100)
    hostio.write_sam(sam, cols, names, lens, n_lanes=2, first_read_index=100)
    want = pybam.bam_to_sam_text(bam)
    assert want.count("\t*\tRG:Z:") == len(range(0, 2000, 17))
    assert open(sam, newline="").read() == want


@pytest.mark.parametrize("batch_reads", [1 << 20, 777])
def test_host_reader_gives_the_columns_the_generator_wrote(tmp_path, batch_reads):
    path = str(tmp_path / "wild.sam")
    want = sam_sweeps.wild(path)
    raw = open(path, "rb").read()
    assert not raw.endswith(b"\n") and b"\r\n" in raw and b"\n\n" in raw and b"\n@CO" in raw.split(b"\nw0\t")[1]
    got, lanes = _read_all(path, batch_reads)
    assert len(want["flag"]) == 3000
    assert set(got) == set(want)  # (no further NM values: every line of this file is one the card decodes too)
    for k in want:
        assert np.array_equal(got[k], want[k]), k
    assert lanes == [("L1", 0), ("L2", 1)]


def test_host_reader_takes_the_odd_lines_and_ends_at_the_bad_ones(tmp_path):
    rng = np.random.default_rng(3)
    good = [sam_sweeps.plain_line(rng, "g%d" % i) for i in range(50)]
    odd = sam_sweeps.odd_lines(rng)
    path = str(tmp_path / "odd.sam")
    open(path, "w").write(sam_sweeps.header() + "\n".join(good[:25] + [l for _, l in odd] + good[25:]) + "\n")
    got, lanes = _read_all(path, 1 << 20)
    assert len(got["flag"]) == 56
    assert got["nm_extra_read"].tolist() == [25] and got["nm_extra_val"].tolist() == [9]
    assert got["as_"][26] == 41 and got["lane"][27] == 0 and ("newcomer", 0) in lanes
    assert got["pos"][28] == 4 and got["mapq"][29] == 5 and got["flag"][30] == (12345678999 & 0xFFF) | 0x1000
    for what, line, code, msg in sam_sweeps.bad_lines(rng):
        open(path, "w").write(sam_sweeps.header() + "\n".join(good[:25] + [line] + good[25:]) + "\n")
        b = hostio.BamFile(path)
        with pytest.raises(IOError) as e:
            list(b.batches(10))
        b.close()
        assert str(e.value).startswith("bam read error %d: %s" % (code, msg)), what
        if what == "no RG":
            assert "(record 25)" in str(e.value)
