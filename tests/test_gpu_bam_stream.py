"""GPU: BAM STREAMS on the card — BAM bytes on "-", through /dev/stdin and through a FIFO, read once, in order:
the reader's columns against the host reader's of the same bytes as a file; the program's output against the file run's and the
oracle's; a batch handed over inside a stream; damaged streams (the host reader's error, in one pass); the edges.

Every stream is read in a child process under a time limit (tests/bam_stream_util.py).  Seams: BQC_GPU_DECODE=1 (the card, whatever
the size), BQC_GB_CHUNK_KB=256 and BQC_GB_RUN_MB=1 — the ring of six chunks wraps and the stream is several runs — and BQC_STREAM_HOLD=N,
a prefix cut at N (several runs of prefix; the whole stream in memory before the reader exists)."""
import filecmp
import os
import re
import struct
import zlib

import pytest

from bamqc_amd import hostio
from tests import pybam
from tests.bam_stream_util import program, read_columns, same

pytestmark = pytest.mark.gpu
SEAMS = {"BQC_GPU_DECODE": "1", "BQC_GB_CHUNK_KB": "256", "BQC_GB_RUN_MB": "1"}
NAMES, LENS = ["chr1", "chr2"], [600_000, 400_000]


@pytest.fixture(scope="module")
def shapes(tmp_path_factory):
    """name -> (the BAM's bytes, the host reader's columns of the file): made once, shared, left unchanged"""
    from tests.test_host_io import _wild_bam
    tmp = str(tmp_path_factory.mktemp("bam_stream"))
    paths = {k: os.path.join(tmp, k + ".bam") for k in ("short", "long", "wild")}
    hostio.synth_stream(paths["short"], os.path.join(tmp, "ref.fa"), seed=7, n_reads=40_000, ref_names=NAMES, ref_lens=LENS, n_lanes=2)
    hostio.synth_stream(paths["long"], None, seed=8, n_reads=600, ref_names=NAMES, ref_lens=LENS, n_lanes=2, read_len=9000, long_reads=True)
    _wild_bam(paths["wild"], 23, 4000, extra_nm=False)  # stored blocks, every tag type, blocks of random size
    out = {}
    for k, p in paths.items():
        data = open(p, "rb").read()
        out[k] = (data, read_columns(tmp, data, "file", 3001)[0])
    return tmp, out, paths


# (the seams and the default sizes through both kinds of descriptor; a prefix of several runs and a stream held whole once each)
_CASES = [(shape, sizes, how) for shape in ("short", "long", "wild")
          for sizes, how in (("seams", "-"), ("seams", "fifo"), ("default", "-"), ("default", "fifo"), ("seams_prefix_runs", "-"), ("seams_all_held", "fifo"))]


@pytest.mark.parametrize("shape,sizes,how", _CASES)
def test_columns_of_a_stream(shapes, shape, sizes, how):
    tmp, files, _ = shapes
    data, want = files[shape]
    env = {"BQC_GPU_DECODE": "1"} if sizes == "default" else dict(SEAMS)
    if sizes == "seams_prefix_runs":
        env["BQC_STREAM_HOLD"] = str(len(data) * 2 // 3 + 7)  # (the prefix is several runs of 1 MB and ends inside a block)
    if sizes == "seams_all_held":
        env["BQC_STREAM_HOLD"] = str(len(data) + 1)  # (the stream has ended before the reader exists: no ring)
    for batch_reads in (3001, 1 << 20):
        got, report = read_columns(tmp, data, how, batch_reads, gpu=0, env=env)
        same(want, got)
        assert "handed_over=0" in report and "on_card=True" in report, report  # (the reader on the card, not a host reader behind the same call)


@pytest.mark.parametrize("shape,every", [("short", 1), ("short", 2), ("long", 1), ("wild", 2)])
def test_the_host_walk_on_clean_streams(shapes, shape, every):
    """BQC_TEST_STREAM_TROUBLE=k: every k-th call distrusts its window's first record, so the host reader's walk runs over CLEAN bytes —
    it accepts records up to one that is not all there while the stream goes on (the card continues from that position), and meets
    windows without one whole record (widened, or the next run's bytes behind them: runs of 1 MB, reads of 9 kb).  Same columns."""
    tmp, files, _ = shapes
    data, want = files[shape]
    for batch_reads in (3001, 1 << 20):
        got, report = read_columns(tmp, data, "-", batch_reads, gpu=0, env=dict(SEAMS, BQC_TEST_STREAM_TROUBLE=str(every)))
        same(want, got)
        m = re.search(r"batches=(\d+) handed_over=(\d+) on_card=True", report)
        assert m and int(m.group(2)) >= 1, report
        if every == 1:
            assert m.group(1) == m.group(2), report  # every batch came from the host's walk


def test_a_sam_fifo_is_sam_text_on_the_card(shapes, tmp_path):
    """A FIFO named *.sam through bqc_bam_open_gpu: the reader of SAM text, as before BAM streams existed."""
    tmp, _, _ = shapes
    lens = [50_000, 30_000]
    cols = hostio.synth_slice(5, 2000, 0, 2000, lens)
    sam, bam = str(tmp_path / "x.sam"), str(tmp_path / "x.bam")
    hostio.write_sam(sam, cols, NAMES, lens)
    hostio.write_bam(bam, cols, NAMES, lens)
    want, _ = read_columns(tmp, open(bam, "rb").read(), "file", 777)
    got, report = read_columns(tmp, open(sam, "rb").read(), "fifo.sam", 777, gpu=0)
    same(want, got)
    assert "on_card=True" in report, report


def _run(tmp, name, args_in, data=None, fifo=None, env=None, extra=()):
    out = os.path.join(tmp, name + ".bamqc")
    if os.path.exists(out):
        os.unlink(out)
    r = program(["-r", os.path.join(tmp, "ref.fa"), "-o", out] + list(extra) + [args_in], data=data, fifo=fifo, env=env)
    return r.returncode, r.stderr.decode(), out


def _errors(stderr, path):
    """the program's ERROR lines, with the input's name taken out"""
    return [re.sub(r"(?<= )%s(?= |$)" % re.escape(path), "INPUT", l) for l in stderr.splitlines() if l.startswith("ERROR")]


@pytest.fixture(scope="module")
def file_run(shapes):
    """the short BAM as a FILE through the program (the reader on the card), and the oracle's output for the same reads"""
    from tests.cli_oracle import oracle_bamqualcheck
    tmp, _, paths = shapes
    rc, err, out = _run(tmp, "file", paths["short"], env={"BQC_GPU_DECODE": "1"})
    assert rc == 0 and "records decoded on the GPU" in err, err[-2000:]
    want = os.path.join(tmp, "oracle.bamqc")
    assert oracle_bamqualcheck(paths["short"], os.path.join(tmp, "ref.fa"), want) == 0
    assert filecmp.cmp(out, want, shallow=False)
    return out


@pytest.mark.parametrize("how", ["-", "/dev/stdin", "fifo"])
def test_program_reads_a_bam_stream_on_the_card(shapes, file_run, how):
    tmp, files, _ = shapes
    data = files["short"][0]
    for env in ({"BQC_GPU_DECODE": "1"}, SEAMS):
        if how == "fifo":
            rc, err, out = _run(tmp, "stream", os.path.join(tmp, "in.bam"), data=data, fifo=os.path.join(tmp, "in.bam"), env=env)
        else:
            rc, err, out = _run(tmp, "stream", how, data=data, env=env)
        assert rc == 0, err[-2000:]
        assert filecmp.cmp(out, file_run, shallow=False)  # (file_run equals the oracle's file)
        assert "records decoded on the GPU" in err, err[-2000:]
        m = re.search(r"\[timing\] (\d+) batches anchored on the card", err)
        assert m and int(m.group(1)) >= 1, err[-2000:]
        assert "hands over to the host reader" not in err


def _members(data):
    """(offset, size) of every BGZF member"""
    out, p = [], 0
    while p < len(data):
        n = (data[p + 16] | (data[p + 17] << 8)) + 1
        out.append((p, n))
        p += n
    return out


def _inflate_all(data):
    return b"".join(zlib.decompress(data[p + 18:p + n - 8], -15) for p, n in _members(data))


def _record_starts(u):
    """offsets of the records in the uncompressed stream u (behind the header)"""
    l_text = struct.unpack_from("<i", u, 4)[0]
    p = 8 + l_text
    n_ref = struct.unpack_from("<i", u, p)[0]
    p += 4
    for _ in range(n_ref):
        p += 8 + struct.unpack_from("<i", u, p)[0]
    starts = []
    while p < len(u):
        starts.append(p)
        p += 4 + struct.unpack_from("<i", u, p)[0]
    return starts


def _blocks(u, ends=(), eof=True):
    """u as BGZF members of at most 60 000 bytes, one of them ending at each offset of `ends`"""
    out, p = [], 0
    cuts = sorted(set(e for e in ends if 0 < e < len(u))) + [len(u)]
    for c in cuts:
        while p < c:
            n = min(60_000, c - p)
            out.append(pybam._bgzf_block(u[p:p + n], level=1))
            p += n
    return b"".join(out) + (pybam._bgzf_block(b"") if eof else b"")


def test_a_batch_handed_over_inside_a_stream(shapes, file_run):
    """A record whose read group is not in the header, appended to the clean stream: ITS batch goes through the host decoder, the
    stream stays on the card, and the output is the file run's of the same bytes."""
    tmp, files, _ = shapes
    data = files["short"][0]
    assert data[-28:] == pybam._bgzf_block(b"")
    name = b"odd\0"
    body = struct.pack("<iiBBHHHiiii", 1, 399_000, len(name), 30, 4680, 1, 0x41, 4, -1, -1, 0) + name + struct.pack("<I", (4 << 4) | 0) + bytes([0x12, 0x48]) + bytes([30] * 4) + b"RGZnot_in_header\0"
    odd = data[:-28] + pybam._bgzf_block(struct.pack("<i", len(body)) + body) + pybam._bgzf_block(b"")
    path = os.path.join(tmp, "odd.bam")
    open(path, "wb").write(odd)
    env = dict(SEAMS)
    rc0, err0, out0 = _run(tmp, "odd_file", path, env={"BQC_GPU_DECODE": "1"}, extra=["--batch-reads", "10000"])
    assert rc0 == 0 and "1 batches held records" in err0, err0[-2000:]
    want = open(out0, "rb").read()
    rc, err, out = _run(tmp, "odd_stream", "-", data=odd, env=env, extra=["--batch-reads", "10000"])
    assert rc == 0, err[-2000:]
    assert "records decoded on the GPU" in err and "1 batches held records" in err, err[-2000:]
    assert open(out, "rb").read() == want
    assert want != open(file_run, "rb").read()  # (the odd record counts: a lane of its own)


# The reference of the damaged streams is the host reader on the same bytes as a FILE, and that reader opens a file through a first run of
# 32 MB of compressed bytes (host/bgzf.cpp: plan_run; more with more than 32 host threads, hence BQC_IO_THREADS below): BGZF damage inside it
# is "could not open", behind it "could not read record" — which is what any reader of a STREAM says, having parsed the header from the
# stream's first bytes.  So the two cases of BGZF damage use a stream of 520 K reads (~44 MB) with the damage at nine tenths; the two
# cases of damaged RECORDS, which no reader meets at open, use the 40 K reads.
_DAMAGE_ENV = {"BQC_IO_THREADS": "8"}


@pytest.fixture(scope="module")
def damaged(shapes):
    """name -> bytes: a BAM, damaged"""
    tmp, files, _ = shapes
    data = files["short"][0]
    u = _inflate_all(data)
    starts = _record_starts(u)
    assert len(starts) == 40_000
    k = starts[30_000]
    big_path = os.path.join(tmp, "big.bam")
    hostio.synth_stream(big_path, None, seed=7, n_reads=520_000, ref_names=NAMES, ref_lens=LENS, n_lanes=2)
    big = open(big_path, "rb").read()
    os.unlink(big_path)
    mem = _members(big)
    late = mem[len(mem) * 9 // 10]
    assert late[0] > (36 << 20)  # (well behind the 32 MB)
    flipped = bytearray(big)
    flipped[late[0] + 18 + late[1] // 2] ^= 0x55
    return {
        "cut_inside_a_block": big[:late[0] + late[1] // 2],
        "cut_inside_a_record_at_a_block_boundary": _blocks(u[:k + 10], eof=False),  # (30 000 whole records in front: ten batches of 3001)
        "block_size_below_32": _blocks(u[:k] + struct.pack("<i", 8) + bytes(8) + u[k:], ends=[k - 100, k + 200]),
        "flipped_byte_in_a_block": bytes(flipped),
    }


@pytest.mark.parametrize("case", ["cut_inside_a_block", "cut_inside_a_record_at_a_block_boundary", "block_size_below_32", "flipped_byte_in_a_block"])
@pytest.mark.parametrize("sizes", ["seams", "default"])
def test_damaged_streams_fail_as_the_host_reader_does_in_one_pass(shapes, damaged, case, sizes):
    tmp, _, _ = shapes
    bad = damaged[case]
    path = os.path.join(tmp, case + ".bam")
    open(path, "wb").write(bad)
    rc0, err0, _ = _run(tmp, "bad_file", path, env=dict(_DAMAGE_ENV, BQC_GPU_DECODE="0"), extra=["--batch-reads", "3001"])
    os.unlink(path)
    assert rc0 == 1 and "records decoded on the host" in err0 and _errors(err0, path), err0[-2000:]
    env = dict(_DAMAGE_ENV, **(SEAMS if sizes == "seams" else {"BQC_GPU_DECODE": "1"}))
    rc, err, _ = _run(tmp, "bad_stream", "-", data=bad, env=env, extra=["--batch-reads", "3001"])
    assert rc == rc0, err[-2000:]
    assert _errors(err, "-") == _errors(err0, path), (err[-2000:], err0[-2000:])
    assert "records decoded on the GPU" in err, err[-2000:]
    assert "hands over to the host reader" not in err and err.count("records decoded on") == 1  # no second pass
    m = re.search(r"\[timing\] (\d+) records: decode thread", err)
    if case in ("cut_inside_a_record_at_a_block_boundary", "block_size_below_32"):  # the records in front were delivered first
        assert m and int(m.group(1)) >= 3001, err[-2000:]


def test_edges_of_a_stream(shapes, file_run):
    tmp, files, paths = shapes
    data = files["short"][0]
    u = _inflate_all(data)
    first = _record_starts(u)[0]
    # a stream that ends right behind the header: no records, the file run's (empty-handed) output
    empty = _blocks(u[:first])
    p = os.path.join(tmp, "empty.bam")
    open(p, "wb").write(empty)
    rc0, err0, out0 = _run(tmp, "empty_file", p, env={"BQC_GPU_DECODE": "1"})
    want = open(out0, "rb").read()
    rc, err, out = _run(tmp, "empty_stream", "-", data=empty, env=SEAMS)
    assert (rc, open(out, "rb").read()) == (rc0, want) and rc == 0, (err[-1500:], err0[-1500:])
    assert "records decoded on the GPU" in err
    # an EOF block only: no BAM — the file's failure
    p = os.path.join(tmp, "eof.bam")
    open(p, "wb").write(pybam._bgzf_block(b""))
    rc0, err0, _ = _run(tmp, "eof_file", p, env={"BQC_GPU_DECODE": "1"})
    rc, err, _ = _run(tmp, "eof_stream", "-", data=pybam._bgzf_block(b""), env={"BQC_GPU_DECODE": "1"})
    assert rc == rc0 == 1 and _errors(err, "-") == _errors(err0, p) != [], (err, err0)
    # shorter than the threshold, BQC_GPU_DECODE unset: the host reader, from memory, and the same output
    rc, err, out = _run(tmp, "held_stream", "-", data=data, env={"BQC_GPU_DECODE": None})
    assert rc == 0 and "records decoded on the host" in err, err[-1500:]
    assert filecmp.cmp(out, file_run, shallow=False)


def test_sam_text_on_stdin_is_untouched(shapes, tmp_path):
    """SAM text on "-" with BQC_GPU_DECODE=1: still SAM text, on the card; the .bamqc of the equivalent BAM's file run."""
    tmp, _, _ = shapes
    cols = hostio.synth_slice(7, 40_000, 0, 40_000, LENS, n_lanes=2)
    sam, bam = str(tmp_path / "x.sam"), str(tmp_path / "x.bam")
    hostio.write_sam(sam, cols, NAMES, LENS, n_lanes=2)
    hostio.write_bam(bam, cols, NAMES, LENS, n_lanes=2)
    rc0, err0, out0 = _run(tmp, "sam_bam_file", bam, env={"BQC_GPU_DECODE": "1"})
    assert rc0 == 0, err0[-1500:]
    rc, err, out = _run(tmp, "sam_stream", "-", data=open(sam, "rb").read(), env={"BQC_GPU_DECODE": "1"})
    assert rc == 0 and "csrc/gpu_sam.hip" in err, err[-1500:]
    assert filecmp.cmp(out, out0, shallow=False)
