"""GPU: SAM text inside BGZF inflated and decoded on the card (csrc/gpu_bam.hip's producer feeding csrc/gpu_sam.hip)
against the host reader of the plain text (columns) and the oracle (`.bamqc` bytes): the seams of the new source — a line over a run
boundary, the ring wrapping, member kinds — hand-over and errors as for plain text, BGZF damage in the host reader's words, the
program on x.sam, x.sam.gz and streams, sessions that mix the three input forms."""
import filecmp
import os
import re
import subprocess

import numpy as np
import pytest

from bamqc_amd import hostio
from tests import pybam, sam_sweeps
from tests.bam_stream_util import program
from tests.cli_oracle import oracle_bamqualcheck
from tests.sam_bgzf_util import EOF_MEMBER, cut_at, error_of, members, read
from tests.test_gpu_reader import all_columns, same

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "bin", "bamqualcheck")
SMALL = {"BQC_GPU_DECODE": "1", "BQC_GB_CHUNK_KB": "256", "BQC_GB_RUN_MB": "1"}  # several runs, and the ring wraps
RUN_SPAN = (1 << 20) + (256 << 10) + (64 << 10)  # a run ends at the first chunk end at or behind BQC_GB_RUN_MB (less a cut member): no run spans more compressed bytes


def read_all(path, batch_reads, **kw):
    """In this process (a file): columns (further NM values with the index of their read in the FILE), batches handed over, on the card?, lanes, error."""
    b = hostio.BamFile(path, **kw)
    cols, base, err = {}, 0, None
    try:
        for batch in b.batches(batch_reads):
            for k, v in batch.items():
                cols.setdefault(k, []).append(np.array(v, copy=True) + (base if k == "nm_extra_read" else 0))
            base += len(batch["flag"])
    except IOError as e:
        err = str(e)
    handed, on_card, lanes = b.batches_handed_over, b.on_card, b.lanes()
    b.close()
    return {k: np.concatenate(v) for k, v in cols.items()}, handed, on_card, lanes, err


def packed(tmp, name, data):
    p = os.path.join(str(tmp), name)
    with open(p, "wb") as f:
        f.write(data)
    return p


@pytest.fixture(scope="module")
def shapes(tmp_path_factory):
    """name -> (directory, the text as BGZF of 0xff00-byte members at level 1, the host reader's columns of the plain text)"""
    d = tmp_path_factory.mktemp("sam_bgzf_shapes")
    out = {}
    for name, kw in (("short", dict(seed=31, n_reads=30_000, ref_names=["chr1", "chr2", "chrM"], ref_lens=[400_000, 250_000, 16_000], n_lanes=2)),
                     ("long", dict(seed=32, n_reads=300, ref_names=["chr1", "chr2"], ref_lens=[3_000_000, 2_000_000], read_len=9000, long_reads=True))):
        bam, sam = str(d / (name + ".bam")), str(d / (name + ".sam"))
        hostio.synth_stream(bam, None, **kw)
        cols, _ = all_columns(bam, 1 << 20)
        hostio.write_sam(sam, cols, kw["ref_names"], kw["ref_lens"], n_lanes=kw.get("n_lanes", 1))
        host, _ = all_columns(sam, 1 << 20)
        data, csizes = members(open(sam, "rb").read(), [0xff00])
        assert sum(csizes) > RUN_SPAN  # (more than one run, whatever the first one takes)
        out[name] = (d, data, host)
    return out


@pytest.mark.parametrize("how", ["file", "-", "fifo.sam.gz"])
@pytest.mark.parametrize("shape", ["short", "long"])
def test_columns_equal_the_host_readers(shapes, monkeypatch, shape, how):
    tmp, data, host = shapes[shape]
    for batch_reads in (777, 10_000, 1 << 20):
        if how == "file":
            for k, v in SMALL.items():
                monkeypatch.setenv(k, v)
            got, handed, on_card, _, err = read_all(packed(tmp, shape + ".sam.gz", data), batch_reads, gpu=0)
            assert err is None and handed == 0 and on_card
        else:
            got, report, rc = read(tmp, data, how, batch_reads, gpu=0, env=SMALL)
            assert rc == 0 and error_of(report) is None and "handed_over=0 on_card=True" in report, report
        same(host, got)


def test_columns_with_default_chunk_and_run_sizes(shapes):
    tmp, data, host = shapes["short"]
    got, handed, on_card, _, err = read_all(packed(tmp, "default.sam.gz", data), 10_000, gpu=0)
    assert err is None and handed == 0 and on_card
    same(host, got)
    got, report, rc = read(tmp, data, "-", 10_000, gpu=0, env={"BQC_GPU_DECODE": "1"})
    assert rc == 0 and error_of(report) is None and "handed_over=0 on_card=True" in report, report
    same(host, got)


@pytest.fixture(scope="module")
def boundary(tmp_path_factory):
    """(directory, text, the host reader's columns): sam_sweeps.boundary's text — the probe lines around every multiple of 64 KiB, the
    100 000-base line — with twenty more 100 000-base lines behind it, a stretch of text in which every byte belongs to a 200 KB line."""
    tmp = tmp_path_factory.mktemp("sam_bgzf_boundary")
    path = str(tmp / "boundary.sam")
    n_probe = sam_sweeps.boundary(path)
    text = open(path, "rb").read()
    long_at = text.index(b"\nlong\t") + 1
    long_line = text[long_at:text.index(b"\n", long_at) + 1]
    assert len(long_line) > 200_000
    text += b"".join(long_line.replace(b"long\t", b"long%d\t" % k, 1) for k in range(20))
    open(path, "wb").write(text)
    host, _ = all_columns(path, 1 << 20)
    assert int((host["l_seq"] == 100_000).sum()) == 21
    return tmp, text, host, n_probe


def _compressed_span(text, data_members, a, b):
    """compressed bytes of the members that lie wholly inside text[a, b) — data_members: [(payload size, compressed size)] in order"""
    at, span = 0, 0
    for usize, csize in data_members:
        if at >= a and at + usize <= b:
            span += csize
        at += usize
    return span


def test_lines_across_run_boundaries(boundary, monkeypatch):
    """Member boundaries — the only places a run can end — fall INSIDE the probe lines all along the probes' stretch of the text, and inside
    200 KB lines all along the long lines' stretch; each stretch is longer, compressed, than any run can be, so at least one run
    boundary falls in each: a probe line and a 200 KB line straddle a run boundary, whatever the reader's first run takes."""
    tmp, text, host, n_probe = boundary
    probe = sam_sweeps.PROBE.encode()
    starts = [m.start() for m in re.finditer(re.escape(probe), text)]
    assert len(starts) == n_probe
    inside = [s + 1 + i % (len(probe) - 2) for i, s in enumerate(starts)]  # a cut inside every probe line, at a different offset of the line each time
    assert max(b - a for a, b in zip(inside, inside[1:])) <= 65536
    long0 = text.index(b"\nlong0\t") + 1
    line_starts = {m.start() + 1 for m in re.finditer(b"\n", text[long0:])}
    long_cuts = [x for x in range(long0 + 1000, len(text), 0xff00)]
    assert not any(c - long0 in line_starts for c in long_cuts)
    cuts = inside + long_cuts + list(range(0xff00, inside[0] - 70_000, 0xff00)) + list(range(inside[-1] + 0xff00, long0, 0xff00))
    data = cut_at(text, cuts, limit=65536)
    # the members as written: (payload, compressed) sizes, from the bytes themselves
    mem, p = [], 0
    while p < len(data):
        bsize = (data[p + 16] | (data[p + 17] << 8)) + 1
        mem.append((int.from_bytes(data[p + bsize - 4:p + bsize], "little"), bsize))
        p += bsize
    assert sum(u for u, _ in mem) == len(text)
    edges = set(np.cumsum([u for u, _ in mem]).tolist())
    probes_stretch = (inside[0], inside[-1])
    assert {e for e in edges if probes_stretch[0] <= e <= probes_stretch[1]} == set(inside)  # no member boundary there but inside a probe line
    assert _compressed_span(text, mem, *probes_stretch) > RUN_SPAN
    assert _compressed_span(text, mem, long0 + 1000, len(text)) > RUN_SPAN and not any(e - long0 in line_starts for e in edges if long0 < e < len(text))
    for k, v in SMALL.items():
        monkeypatch.setenv(k, v)
    path = packed(tmp, "boundary.sam.gz", data)
    for batch_reads in (1 << 20, 5000):
        got, handed, on_card, _, err = read_all(path, batch_reads, gpu=0)
        assert err is None and handed == 0 and on_card
        same(host, got)
    got, report, rc = read(tmp, data, "-", 5000, gpu=0, env=SMALL)
    assert rc == 0 and error_of(report) is None and "handed_over=0 on_card=True" in report, report
    same(host, got)
    # the same text, its first twentieth in members of 1..200 bytes with empty members in between
    rng = np.random.default_rng(12)
    n20 = len(text) // 20
    tiny = members(text[:n20], (int(x) for x in rng.integers(1, 201, size=n20)), empty_between=True, eof=False)[0] + members(text[n20:], [0xff00])[0]
    got, handed, on_card, _, err = read_all(packed(tmp, "tiny.sam.gz", tiny), 5000, gpu=0)
    assert err is None and handed == 0 and on_card
    same(host, got)


def test_member_kinds(tmp_path, monkeypatch):
    path = str(tmp_path / "wild.sam")
    sam_sweeps.wild(path)
    text = open(path, "rb").read()
    host, _ = all_columns(path, 777)
    rng = np.random.default_rng(21)
    out, at, k, seen = [], 0, 0, set()
    while at < len(text):
        kind = pybam.MEMBER_KINDS[k % len(pybam.MEMBER_KINDS)]
        k += 1
        if kind == "empty":
            out.append(EOF_MEMBER)
            continue
        n = int(rng.integers(1, 30_000))
        m = pybam._bgzf_member(text[at:at + n], kind, rng)
        assert m is not None
        out.append(m); seen.add(kind)
        at += n
    assert seen == set(pybam.MEMBER_KINDS) - {"empty"}
    monkeypatch.setenv("BQC_GPU_DECODE", "1")
    for batch_reads in (777, 1 << 20):
        got, handed, on_card, _, err = read_all(packed(tmp_path, "kinds.sam.gz", b"".join(out) + EOF_MEMBER), batch_reads, gpu=0)
        assert err is None and handed == 0 and on_card
        same(host, got)


def test_odd_lines_are_handed_over_as_from_plain_text(tmp_path):
    rng = np.random.default_rng(8)
    odd = sam_sweeps.odd_lines(rng)
    text, k = sam_sweeps.header(), 0
    for _, line in odd + [odd[2]]:
        text += "".join(sam_sweeps.plain_line(rng, "g%d" % (k + i)) + "\n" for i in range(3000)) + line + "\n"
        k += 3000
    text += "".join(sam_sweeps.plain_line(rng, "z%d" % i) + "\n" for i in range(3000))
    plain = str(tmp_path / "odd.sam")
    open(plain, "w", newline="").write(text)
    host, _, _, host_lanes, err = read_all(plain, 777)
    assert err is None and ("newcomer", 0) in host_lanes
    card, handed_plain, on_card, lanes, err = read_all(plain, 777, gpu=0)
    assert err is None and on_card and handed_plain == len(odd)
    got, handed, on_card, lanes, err = read_all(packed(tmp_path, "odd.sam.gz", members(text.encode(), [0xff00])[0]), 777, gpu=0)
    assert err is None and on_card and lanes == host_lanes
    same(host, got)
    assert handed == handed_plain


@pytest.mark.parametrize("which", range(8))
def test_errors_are_the_host_readers(tmp_path, which):
    rng = np.random.default_rng(4)
    what, line, code, msg = sam_sweeps.bad_lines(rng)[which]
    good = [sam_sweeps.plain_line(rng, "g%d" % i) for i in range(5000)]
    text = (sam_sweeps.header() + "\n".join(good[:2500] + [line] + good[2500:]) + "\n").encode()
    plain = str(tmp_path / "bad.sam")
    open(plain, "wb").write(text)
    host, _, _, _, host_err = read_all(plain, 777)
    card, _, _, _, card_err = read_all(plain, 777, gpu=0)
    got, _, on_card, _, err = read_all(packed(tmp_path, "bad.sam.gz", members(text, [0xff00])[0]), 777, gpu=0)
    assert host_err is not None and host_err.startswith("bam read error %d: %s" % (code, msg)), what
    assert on_card and err == host_err == card_err
    same(card, got)  # the records delivered in front of the failing line: those the card delivers from the plain text
    assert len(got["flag"]) == 2500


def test_damage_is_an_io_error_in_the_host_readers_words(shapes, tmp_path):
    tmp, data, _ = shapes["short"]
    sizes, p = [], 0
    while p < len(data):
        sizes.append((data[p + 16] | (data[p + 17] << 8)) + 1)
        p += sizes[-1]
    k = int(np.searchsorted(np.cumsum(sizes), 2 << 20))  # the member that holds the stream's byte 2 MB
    at = sum(sizes[:k]) + 18 + (sizes[k] - 26) // 2
    flipped = data[:at] + bytes([data[at] ^ 0x55]) + data[at + 1:]
    cut = data[:sum(sizes[:k]) + 100]
    fa = str(tmp_path / "g.fa")
    hostio.write_fasta(fa, ["chr1", "chr2", "chrM"], [np.zeros(n, np.uint8) for n in (400_000, 250_000, 16_000)])
    for bad, words in ((flipped, "BGZF block failed to inflate (corrupt data)"), (cut, "truncated BGZF file")):
        _, host_report, host_rc = read(tmp, bad, "-", 10_000)  # the host reader of the same bytes
        _, report, rc = read(tmp, bad, "-", 10_000, gpu=0, env=SMALL)
        assert host_rc == 0 and error_of(host_report) == "bam read error 7: " + words, host_report
        assert rc == 0 and error_of(report) == error_of(host_report) and "on_card=True" in report, report  # (2 MB in: behind the first runs)
        r = program(["-r", fa, "-o", str(tmp_path / "x.bamqc"), "--no-sketch", "-"], data=bad, env=SMALL)
        assert r.returncode == 1 and b"Could not read record from BAM File" in r.stderr, r.stderr[-2000:]


def test_an_error_of_the_source_is_every_later_calls_answer(shapes, monkeypatch):
    """A caller that asks again after BGZF damage gets the damage again — not what was left in the window taken for the stream's last line."""
    tmp, data, _ = shapes["short"]
    at = 2 << 20
    for k, v in SMALL.items():
        monkeypatch.setenv(k, v)
    b = hostio.BamFile(packed(tmp, "flipped.sam.gz", data[:at] + bytes([data[at] ^ 0x55]) + data[at + 1:]), gpu=0)
    errs, n = [], 0
    for _ in range(3):
        try:
            for batch in b.batches(10_000):
                n += len(batch["flag"])
        except IOError as e:
            errs.append(str(e))
    b.close()
    assert 0 < n < 30_000 and len(errs) == 3 and errs[0].startswith("bam read error 7: ") and errs[1] == errs[0] == errs[2], (n, errs)


def test_a_line_longer_than_the_room_in_front_of_a_run_is_an_io_error(tmp_path, monkeypatch):
    """what is left of a run goes into the 16 MB in front of the next one — an 18 MB line that crosses run boundaries is an
    I/O error of this source, behind the records in front of it (the plain source takes such a line)."""
    rng = np.random.default_rng(17)
    L = 9_000_000
    seq = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, size=L)].tobytes()
    qual = rng.integers(33, 74, size=L).astype(np.uint8).tobytes()
    huge = b"\t".join([b"huge", b"0", b"chr1", b"1000", b"60", b"%dM" % L, b"*", b"0", b"0", seq, qual, b"RG:Z:L1", b"NM:i:0", b"AS:i:9"]) + b"\n"
    front = "".join(sam_sweeps.plain_line(rng, "f%d" % i) + "\n" for i in range(2000)).encode()
    text = sam_sweeps.header().encode() + front + huge + "".join(sam_sweeps.plain_line(rng, "b%d" % i) + "\n" for i in range(100)).encode()
    for k, v in SMALL.items():
        monkeypatch.setenv(k, v)
    got, handed, on_card, _, err = read_all(packed(tmp_path, "huge.sam.gz", members(text, [0xff00])[0]), 777, gpu=0)
    assert on_card and err is not None and err.startswith("bam read error 7: a line longer than the room in front of a run of inflated text"), err
    assert len(got["flag"]) == 2000


@pytest.fixture(scope="module")
def reads(tmp_path_factory):
    """One set of reads as m.bam, m.sam and m.sam.gz beside their genome, the options of every run, and the oracle's file."""
    d = tmp_path_factory.mktemp("sam_bgzf_program")
    bam, fa, sam, gz, want = (str(d / x) for x in ("m.bam", "genome.fa", "m.sam", "m.sam.gz", "oracle.bamqc"))
    names, lens = ["chr1", "chr2", "chrX", "chrUn_1"], [400_000, 300_000, 200_000, 50_000]
    hostio.synth_write(bam, fa, seed=7, n_reads=30_000, ref_names=names, ref_lens=lens, n_lanes=3)
    cols, _ = all_columns(bam, 1 << 20)
    hostio.write_sam(sam, cols, names, lens, n_lanes=3)
    open(gz, "wb").write(members(open(sam, "rb").read(), [0xff00])[0])
    assert oracle_bamqualcheck(bam, fa, want, isize=500, klist=(21, 32), qlist=(10,), batch_reads=4000) == 0
    return d, bam, fa, sam, gz, want, ["-i", "500", "--batch-reads", "7001", "-k", "21,32", "-q", "10"]


def _decoded(r):
    m = re.search(rb"\[timing\] records decoded (.*)", r.stderr)
    assert m, r.stderr[-2000:]
    return m.group(1).decode()


def test_program_reads_sam_files_and_sam_gz_files(reads):
    d, bam, fa, sam, gz, want, args = reads
    for path, decode, where in ((sam, "1", "on the GPU (csrc/gpu_sam.hip)"), (sam, "0", "on the host"),
                                (gz, "1", "on the GPU (csrc/gpu_inflate.hip + csrc/gpu_sam.hip)"), (gz, "0", "on the host")):
        out = str(d / "file.bamqc")
        r = program(["-r", fa, "-o", out] + args + [path], env={"BQC_GPU_DECODE": decode})
        assert r.returncode == 0, r.stderr[-2000:]
        assert _decoded(r) == where, (path, decode)
        assert filecmp.cmp(out, want, shallow=False), (path, decode)


def test_program_reads_bgzf_sam_streams(reads):
    d, bam, fa, sam, gz, want, args = reads
    data = open(gz, "rb").read()
    out = str(d / "stream.bamqc")
    r = program(["-r", fa, "-o", out] + args + ["-"], data=data, env={"BQC_GPU_DECODE": "1"})
    assert r.returncode == 0 and _decoded(r) == "on the GPU (csrc/gpu_inflate.hip + csrc/gpu_sam.hip)", r.stderr[-2000:]
    assert filecmp.cmp(out, want, shallow=False)
    os.unlink(out)
    r = program(["-r", fa, "-o", out] + args + ["-"], data=data, env={"BQC_GPU_DECODE": "0"})
    assert r.returncode == 0 and _decoded(r) == "on the host", r.stderr[-2000:]
    assert filecmp.cmp(out, want, shallow=False)
    os.unlink(out)
    fifo = str(d / "nameless")  # a FIFO without an extension: what it carries is decided by its inflated bytes
    r = program(["-r", fa, "-o", out] + args + [fifo], data=data, fifo=fifo, env={"BQC_GPU_DECODE": "1"})
    assert r.returncode == 0 and _decoded(r) == "on the GPU (csrc/gpu_inflate.hip + csrc/gpu_sam.hip)", r.stderr[-2000:]
    assert filecmp.cmp(out, want, shallow=False)
    os.unlink(out)
    r = program(["-r", fa, "-o", out] + args + ["-"], data=open(bam, "rb").read(), env={"BQC_GPU_DECODE": "1"})  # a BAM stream is still one
    assert r.returncode == 0 and _decoded(r) == "on the GPU (csrc/gpu_bam.hip)", r.stderr[-2000:]
    assert filecmp.cmp(out, want, shallow=False)


def test_a_session_mixes_bam_sam_and_sam_gz_jobs(reads, tmp_path):
    d, bam, fa, sam, gz, want, args = reads
    bam2 = str(d / "m2.bam")
    if not os.path.exists(bam2):
        os.link(bam, bam2)
    jobs = [(bam, "1.bamqc"), (sam, "2.bamqc"), (gz, "3.bamqc"), (bam2, "4.bamqc")]
    lst = tmp_path / "jobs.tsv"
    lst.write_text("".join("%s\t%s\n" % (i, tmp_path / o) for i, o in jobs))
    r = program(["-r", "{dir}/genome.fa", "--manifest", str(lst)] + args, env={"BQC_GPU_DECODE": "1"})
    assert r.returncode == 0, r.stderr[-3000:]
    single = str(tmp_path / "single.bamqc")
    for i, o in jobs:
        q = program(["-r", fa, "-o", single] + args + [i], env={"BQC_GPU_DECODE": "1"})
        assert q.returncode == 0 and filecmp.cmp(str(tmp_path / o), single, shallow=False) and filecmp.cmp(single, want, shallow=False), i
    assert re.findall(rb"\[timing\] records decoded (.*)", r.stderr) == [b"on the GPU (csrc/gpu_bam.hip)", b"on the GPU (csrc/gpu_sam.hip)",
                                                                         b"on the GPU (csrc/gpu_inflate.hip + csrc/gpu_sam.hip)", b"on the GPU (csrc/gpu_bam.hip)"]
    # a damaged x.sam.gz in second place: that job fails alone
    data = open(gz, "rb").read()
    bad = str(d / "bad.sam.gz")
    open(bad, "wb").write(data[:len(data) // 2] + bytes([data[len(data) // 2] ^ 0x55]) + data[len(data) // 2 + 1:])
    jobs = [(bam, "a.bamqc"), (bad, "b.bamqc"), (gz, "c.bamqc")]
    lst.write_text("".join("%s\t%s\n" % (i, tmp_path / o) for i, o in jobs))
    r = program(["-r", "{dir}/genome.fa", "--manifest", str(lst)] + args, env={"BQC_GPU_DECODE": "1"})
    assert r.returncode == 1 and b"job 2 (%s): failed" % bad.encode() in r.stderr and r.stderr.count(b"): failed") == 1, r.stderr[-3000:]
    assert filecmp.cmp(str(tmp_path / "a.bamqc"), want, shallow=False) and filecmp.cmp(str(tmp_path / "c.bamqc"), want, shallow=False)


def test_gpus_refuses_sam_gz_before_it_forks(reads, tmp_path):
    d, bam, fa, sam, gz, want, args = reads
    for path in (gz, sam):
        r = subprocess.run([EXE, "--gpus", "2", "-r", fa, "-o", str(tmp_path / "x.bamqc"), path], capture_output=True, text=True, timeout=120,
                           env=dict(os.environ, BQC_TIMING="1"))
        assert r.returncode == 1
        lines = [x for x in r.stderr.splitlines() if x.strip()]
        assert len(lines) == 1 and "SAM text cannot be read in shards" in lines[0], r.stderr  # (one line, and none of a worker's)
        assert not os.path.exists(str(tmp_path / "x.bamqc"))
