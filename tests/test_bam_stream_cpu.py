"""CPU: the host reader over a BAM STREAM — {a prefix in memory, then the descriptor} (host/bgzf.h: BgzfStream):
"-" with BGZF magic and a FIFO path give the columns of the same bytes read as a file, wherever the prefix is cut; what is no BAM
fails in the host reader's words; SAM text on "-" is still SAM text.  Every stream is read in a child process under a time limit."""
import os
import subprocess
import sys

import numpy as np
import pytest

from bamqc_amd import hostio
from tests.bam_stream_util import READER, ROOT, TIMEOUT, read_columns, same


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    """name -> (the file's bytes, the host reader's columns of the file, compressed offsets worth cutting at)"""
    from tests import pybam
    from tests.test_host_io import _wild_bam
    tmp = str(tmp_path_factory.mktemp("bam_stream_cpu"))
    out = {}
    wild = os.path.join(tmp, "wild.bam")
    _wild_bam(wild, 23, 4000, extra_nm=True, pad_header=4000)  # (a header of ~150 KB: several blocks)
    synth = os.path.join(tmp, "synth.bam")
    hostio.synth_stream(synth, None, seed=7, n_reads=40_000, ref_names=["chr1", "chr2"], ref_lens=[600_000, 400_000], n_lanes=2)
    for name, path in (("wild", wild), ("synth", synth)):
        data = open(path, "rb").read()
        cols, _ = read_columns(tmp, data, "file", 3001)
        out[name] = (data, cols)
    text, _, _ = pybam.read_bam(wild)
    assert len(text) > 100_000
    return tmp, out


def _cuts(name, data):
    """prefix sizes: inside the header, inside a block, at a block boundary, at the stream's end, beyond it"""
    first_block = (data[16] | (data[17] << 8)) + 1  # BSIZE of the first member
    header_cut = 20_000 if name == "wild" else 60  # (wild: the header's text runs over the first ~30 KB of the file; synth: inside its first block)
    return [0, header_cut, first_block, len(data) // 2 + 13, len(data) - 28, len(data), len(data) + 1000]


@pytest.mark.parametrize("name", ["wild", "synth"])
def test_host_reader_over_prefix_and_descriptor(inputs, name):
    tmp, files = inputs
    data, want = files[name]
    assert len(want["flag"]) == (4000 if name == "wild" else 40_000)
    for cut in _cuts(name, data):
        for how in ("-", "fifo"):
            got, report = read_columns(tmp, data, how, 3001, env={"BQC_STREAM_HOLD": str(cut)})
            same(want, got)
            assert "handed_over=0" in report and "on_card=False" in report
    got, _ = read_columns(tmp, data, "/dev/stdin", 3001)  # (a path that is no regular file)
    same(want, got)


def _open_fails(data):
    r = subprocess.run([sys.executable, "-c", READER, "-", "1000", "host", os.devnull, ROOT], input=data, capture_output=True, timeout=TIMEOUT)
    assert r.returncode != 0
    return r.stderr.decode()


def test_streams_that_are_no_bam_fail_in_the_host_readers_words(inputs):
    from tests import pybam
    tmp, files = inputs
    data, _ = files["wild"]
    assert "not a BAM file" in _open_fails(pybam._bgzf_block(b"BAX\1" + bytes(100)) + pybam._bgzf_block(b""))
    assert "not a BAM file" in _open_fails(pybam._bgzf_block(b""))  # (BGZF magic, no byte of BAM)
    first_block = (data[16] | (data[17] << 8)) + 1
    assert "truncated BAM header" in _open_fails(data[:first_block] + pybam._bgzf_block(b""))  # cut at a block boundary inside the header's text
    assert "truncated BGZF file" in _open_fails(data[:first_block + 100])  # ... and inside a block: the BGZF layer's error, as for a file
    # the same bytes as files: the same words
    for bad, words in ((data[:first_block] + pybam._bgzf_block(b""), "truncated BAM header"), (data[:first_block + 100], "truncated BGZF file")):
        p = os.path.join(tmp, "bad.bam")
        open(p, "wb").write(bad)
        with pytest.raises(IOError, match=words):
            hostio.BamFile(p)


def test_sam_text_on_stdin_is_still_sam_text(inputs, tmp_path):
    """"-" without BGZF magic: parsed as SAM text, the columns of the equivalent BAM."""
    tmp, _ = inputs
    lens = [50_000, 30_000]
    cols = hostio.synth_slice(5, 2000, 0, 2000, lens)
    sam, bam = str(tmp_path / "x.sam"), str(tmp_path / "x.bam")
    hostio.write_sam(sam, cols, ["chr1", "chr2"], lens)
    hostio.write_bam(bam, cols, ["chr1", "chr2"], lens)
    want, _ = read_columns(tmp, open(bam, "rb").read(), "file", 777)
    got, _ = read_columns(tmp, open(sam, "rb").read(), "-", 777)
    same(want, got)
    # a FIFO named *.sam is SAM text, read once — a path that ends in ".sam" is never a BAM stream
    got, report = read_columns(tmp, open(sam, "rb").read(), "fifo.sam", 777)
    same(want, got)
    assert "on_card=False" in report
    # ... and a line that starts with 0x1f but not with a gzip member's two bytes is text as well (and no record)
    r = subprocess.run([sys.executable, "-c", READER, "-", "1000", "host", str(tmp_path / "n.npz"), ROOT], input=b"\x1fx\n", capture_output=True, timeout=TIMEOUT)
    assert r.returncode != 0 and "SAM record" in r.stderr.decode()
