"""GPU: the BAM reader on the card (csrc/gpu_bam.hip: inflate, CRC, record walk, column decode) against the host reader —
identical columns whatever the batch size; inputs it must hand over to the host reader instead of decoding."""
import numpy as np
import pytest

from bamqc_amd import hostio

pytestmark = pytest.mark.gpu


def all_columns(path, batch_reads, batch_bases=1 << 28, **kw):
    b = hostio.BamFile(path, **kw)
    cols = {}
    n_batches = 0
    for batch in b.batches(batch_reads, batch_bases):
        n_batches += 1
        for k, v in batch.items():
            if isinstance(v, np.ndarray):
                cols.setdefault(k, []).append(np.array(v, copy=True))
    b.close()
    return {k: np.concatenate(v) for k, v in cols.items()}, n_batches


def same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert len(a[k]) == len(b[k]), k
        assert np.array_equal(a[k], b[k]), k


@pytest.mark.parametrize("shape", ["short_pe", "lanes", "long_reads", "level6"])
def test_gpu_reader_matches_host_reader(tmp_path, shape):
    path = str(tmp_path / "x.bam")
    kw = dict(seed=31, n_reads=700_000, ref_names=["chr1", "chr2", "chrM"], ref_lens=[4_000_000, 2_500_000, 16_000])
    if shape == "lanes":
        kw.update(n_lanes=5, n_reads=400_000)
    if shape == "long_reads":
        kw.update(long_reads=True, n_reads=12_000, read_len=9000)
    if shape == "level6":
        kw.update(level=6, n_reads=300_000)
    hostio.synth_stream(path, None, **kw)
    host, _ = all_columns(path, 250_000)
    for batch_reads in (250_000, 1 << 20, 3001):
        if shape == "long_reads" and batch_reads == 3001:
            continue
        gpu, nb = all_columns(path, batch_reads, gpu=0)
        assert nb >= 1
        same(host, gpu)
    if shape == "long_reads":  # the base limit of a batch
        gpu, nb = all_columns(path, 1 << 20, 20_000_000, gpu=0)
        assert nb >= 4
        same(host, gpu)


def test_small_runs_and_the_size_limit_of_a_run(tmp_path, monkeypatch):
    """Runs of 8 MB of compressed file, each cut off at 24 MB of inflated bytes (a window's offsets are 32-bit: 3.2 GB in production):
    the blocks behind the cut go to the next run, records run across every kind of boundary."""
    path = str(tmp_path / "x.bam")
    hostio.synth_stream(path, None, seed=41, n_reads=600_000, ref_names=["chr1", "chr2"], ref_lens=[3_000_000, 2_000_000], n_lanes=2, level=6)
    host, _ = all_columns(path, 200_000)
    monkeypatch.setenv("BQC_GB_RUN_MB", "8")
    monkeypatch.setenv("BQC_GB_MAX_RUN_OUT_MB", "24")
    for batch_reads in (50_000, 1 << 20):
        gpu, nb = all_columns(path, batch_reads, gpu=0)
        assert nb >= 7
        same(host, gpu)


def test_wild_records_every_tag_type(tmp_path):
    """Python-written BAM: records straddling BGZF blocks of random size and compression level (stored blocks too), every tag
    type around RG / NM / AS, reads without bases or qualities."""
    from tests.test_host_io import _wild_bam
    path = str(tmp_path / "wild.bam")
    _wild_bam(path, 23, 4000, extra_nm=False)
    host, _ = all_columns(path, 777)
    for batch_reads in (777, 100_000):
        gpu, _ = all_columns(path, batch_reads, gpu=0)
        same(host, gpu)


def test_gpu_reader_hands_over_a_batch_not_the_file(tmp_path):
    """Records with a second NM tag (an extra value in the host reader's batch) are not decoded on the card: the BATCH that holds
    one goes through the host decoder (same columns, extra values included), the others stay on the card."""
    from tests.test_host_io import _wild_bam
    path = str(tmp_path / "wild.bam")
    _, extra = _wild_bam(path, 21, 3000)
    assert extra
    host, _ = all_columns(path, 100_000)
    assert len(host["flag"]) == 3000 and len(host["nm_extra_read"]) == len(extra)
    b = hostio.BamFile(path, gpu=0)
    got = [dict((k, np.array(v, copy=True)) for k, v in x.items() if isinstance(v, np.ndarray)) for x in b.batches(100_000)]
    assert b.batches_handed_over == 1 and len(got) == 1
    b.close()
    same(host, got[0])
    # one odd record at the END of a clean file: one batch of several is handed over
    clean = str(tmp_path / "clean.bam")
    hostio.synth_stream(clean, None, seed=11, n_reads=700_000, ref_names=["chr1", "chr2"], ref_lens=[4_000_000, 2_000_000])
    from tests import pybam
    import struct
    raw = open(clean, "rb").read()
    assert raw[-28:] == pybam._bgzf_block(b"")
    name = b"odd\0"
    body = struct.pack("<iiBBHHHiiii", 1, 1_999_000, len(name), 30, 4680, 1, 0x41, 4, -1, -1, 0) + name + struct.pack("<I", (4 << 4) | 0) + bytes([0x12, 0x48]) + bytes([30] * 4) + b"RGZnot_in_header\0"
    odd = str(tmp_path / "odd.bam")
    open(odd, "wb").write(raw[:-28] + pybam._bgzf_block(struct.pack("<i", len(body)) + body) + pybam._bgzf_block(b""))
    host, _ = all_columns(odd, 250_000)
    b = hostio.BamFile(odd, gpu=0)
    got = [dict((k, np.array(v, copy=True)) for k, v in x.items() if isinstance(v, np.ndarray)) for x in b.batches(250_000)]
    assert b.batches_handed_over == 1 and len(got) >= 3
    assert ("not_in_header", 0) in b.lanes()
    b.close()
    same(host, {k: np.concatenate([c[k] for c in got]) for k in got[0]})
    # through the program: the odd file costs about what the clean one does (one batch by the host's rules, not the file twice)
    import os, subprocess, time
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    fa = str(tmp_path / "r.fa")
    from bamqc_amd import synth
    hostio.write_fasta(fa, ["chr1", "chr2"], [synth.reference(11, 0, 4_000_000), synth.reference(11, 1, 2_000_000)])
    wall, err = {}, {}
    for name, path in (("clean", clean), ("odd", odd)) * 3:  # (the best of three each: start-up times of small runs scatter)
        t0 = time.perf_counter()
        r = subprocess.run([os.path.join(root, "bin", "bamqualcheck"), "-r", fa, "-o", str(tmp_path / (name + ".bamqc")), "-c", "chr1,chr2", "--batch-reads", "100000", path],  # (batches of 100 K reads: the odd record's batch is the last of eight)
                           env=dict(os.environ, BQC_GPU_DECODE="1", BQC_TIMING="1", BQC_NO_FORK="1", BQC_GB_TIMING="1"), capture_output=True, text=True)
        wall[name] = min(wall.get(name, 1e9), time.perf_counter() - t0)
        assert r.returncode == 0, r.stderr
        assert "records decoded on the GPU" in r.stderr and ("1 batches held records" in r.stderr) == (name == "odd"), r.stderr
        err[name] = r.stderr
    # (the line "1 batches held records" above is the proof that one batch, not the file, went through the host decoder; the wall
    # times of runs this short scatter with the box — 0.19 against 0.44 s was seen once — so the bound is loose)
    assert wall["odd"] < 2.0 * wall["clean"] + 0.3, (wall, err)


def test_damaged_blocks_are_an_error_for_both_readers(tmp_path):
    """A flipped byte in the compressed data (inflate fails, or inflates to other bytes: the CRC-32 kernel) and one in a block's
    CRC field, far enough into the file that the header is read without meeting them: an I/O error from the reader on the card
    as from the host reader, never the end of the file."""
    path = str(tmp_path / "x.bam")
    hostio.synth_stream(path, None, seed=5, n_reads=700_000, ref_names=["chr1"], ref_lens=[2_000_000])
    data = bytearray(open(path, "rb").read())
    assert len(data) > 50_000_000
    where = len(data) * 9 // 10
    for kind in ("data", "crc"):
        bad = bytearray(data)
        p = 0
        while True:  # the block that holds `where`
            bsize = (bad[p + 16] | (bad[p + 17] << 8)) + 1
            if p + bsize > where:
                break
            p += bsize
        bad[p + (bsize // 2 if kind == "data" else bsize - 8)] ^= 0x10
        f = str(tmp_path / (kind + ".bam"))
        open(f, "wb").write(bad)
        for gpu in (None, 0):
            with pytest.raises(IOError) as e:
                b = hostio.BamFile(f, gpu=gpu)
                n = sum(len(x["flag"]) for x in b.batches(100_000))
                raise AssertionError("read %d records to the end of a damaged file" % n)
            assert "1000" not in str(e.value)  # an error, not a hand-over


def _shard_hints(path, n):
    import os
    size = os.path.getsize(path)
    return [(size // n * i, None if i + 1 == n else size // n * (i + 1)) for i in range(n)]


@pytest.mark.parametrize("shape,n", [("short_pe", 2), ("short_pe", 5), ("long_reads", 3), ("lanes", 7)])
def test_gpu_range_reader_matches_host_range_reader(tmp_path, monkeypatch, shape, n):
    """A shard of the file (records that START between two block boundaries) through the reader on the card: the same columns and
    the same chain words (first / over) as the host reader's shard; the shards together are the whole file; only the shard's
    bytes are read.  Runs of 8 MB so that the end block lies in a later run than the start and records cross run boundaries."""
    path = str(tmp_path / "x.bam")
    kw = dict(seed=33, n_reads=600_000, ref_names=["chr1", "chr2", "chrM"], ref_lens=[4_000_000, 2_500_000, 16_000])
    if shape == "lanes":
        kw.update(n_lanes=3, n_reads=400_000)
    if shape == "long_reads":
        kw.update(long_reads=True, n_reads=12_000, read_len=9000)
    hostio.synth_stream(path, None, **kw)
    whole, _ = all_columns(path, 250_000)
    monkeypatch.setenv("BQC_GB_RUN_MB", "8")
    parts = []
    prev_over = None
    for lo, hi in _shard_hints(path, n):
        hb = hostio.BamFile(path, begin_hint=lo, end_hint=hi)
        hcols = [dict((k, np.array(v, copy=True)) for k, v in b.items() if isinstance(v, np.ndarray)) for b in hb.batches(100_000)]
        hinfo = hb.range_info
        hb.close()
        gb = hostio.BamFile(path, begin_hint=lo, end_hint=hi, gpu=0)
        gcols = [dict((k, np.array(v, copy=True)) for k, v in b.items() if isinstance(v, np.ndarray)) for b in gb.batches(77_000)]
        ginfo = gb.range_info
        gb.close()
        assert ginfo == hinfo, (lo, hi)
        assert hcols and gcols
        h = {k: np.concatenate([c[k] for c in hcols]) for k in hcols[0]}
        g = {k: np.concatenate([c[k] for c in gcols]) for k in gcols[0]}
        same(h, g)
        if prev_over is not None:
            assert ginfo[2] == prev_over  # the chain: this shard begins where its predecessor's last record ended
        prev_over = ginfo[3]
        parts.append(g)
    same(whole, {k: np.concatenate([p[k] for p in parts]) for k in parts[0]})


def test_gpu_reader_against_an_independent_decoder(tmp_path):
    """The reader on the card against tests/pybam.py (gzip + struct, shares nothing with the product): the wild file with
    every tag type, and a synthetic file — every column, not through the host reader."""
    from tests import pybam
    from tests.test_host_io import _wild_bam
    wild = str(tmp_path / "wild.bam")
    _wild_bam(wild, 29, 3000, extra_nm=False)
    synth = str(tmp_path / "s.bam")
    hostio.synth_stream(synth, None, seed=3, n_reads=40_000, ref_names=["chr1", "chr2"], ref_lens=[900_000, 400_000], n_lanes=2)
    for path, main in ((wild, [1, 1, 1]), (synth, [1, 0])):
        want, refs, _, _ = pybam.columns(path, main)
        b = hostio.BamFile(path, gpu=0)
        b.set_main_chrom(np.array(main[:len(refs)], np.uint8))
        got = [dict((k, np.array(v, copy=True)) for k, v in x.items() if isinstance(v, np.ndarray)) for x in b.batches(1777)]
        b.close()
        same(want, {k: np.concatenate([c[k] for c in got]) for k in got[0]})


def test_gpu_reader_on_adversarial_bgzf_members(tmp_path, monkeypatch):
    """The reader on the card against tests/pybam.columns on a file no writer in the field produces but every reader must take
    (tests/pybam.py: write_bam_adversarial): BGZF members alternating stored / fixed-Huffman / level-9 / Z_FULL_FLUSH-split (several
    deflate blocks per member) / level-1 / EMPTY, payloads from 1 to 65 280 bytes, every record of the file's first half across at
    least one member boundary, a header of 150 KB that spans many members.  Whole, in runs of 1 MB (records and members across run
    boundaries), and with every inflate kernel variant."""
    from tests import pybam
    from tests.test_host_io import _wild_bam
    path = str(tmp_path / "adv.bam")
    _wild_bam(path, 37, 5000, extra_nm=False, adversarial=True, pad_header=4000)
    want, refs, _, _ = pybam.columns(path, [1, 1, 1])
    for env in ({}, {"BQC_GB_RUN_MB": "1"}, {"BQC_GI_WAVE": "0"}, {"BQC_GI_WAVE": "0", "BQC_GI_TWO_PHASE": "0"}, {"BQC_GI_TWO_PHASE": "0", "BQC_GI_LEAN": "32"}):
        with monkeypatch.context() as mp:
            for k, v in env.items():
                mp.setenv(k, v)
            b = hostio.BamFile(path, gpu=0)
            b.set_main_chrom(np.ones(3, np.uint8))
            got = [dict((k, np.array(v, copy=True)) for k, v in x.items() if isinstance(v, np.ndarray)) for x in b.batches(1234)]
            b.close()
        same(want, {k: np.concatenate([c[k] for c in got]) for k in got[0]})


def test_gpu_reader_on_handbuilt_deflate_members(tmp_path, monkeypatch):
    """The reader on the card on members whose DEFLATE streams no zlib encoder writes (tests/pybam.py kind `handbuilt`, through
    tests/deflate_build.py: farthest matches up to distance 32 768, dynamic codes up to 15 bits over skewed frequencies, one-code and
    empty distance sets, several deflate blocks per member, empty members between them): the columns of tests/pybam.columns
    (gzip + struct) and of the host reader, by the default kernels and a lane per block, decoded on the card (no batch handed over)."""
    from tests import pybam
    from tests.test_host_io import _wild_bam
    path = str(tmp_path / "hand.bam")
    _wild_bam(path, 43, 2000, extra_nm=False, adversarial=True, pad_header=300, kinds=pybam.HANDBUILT_KINDS, tiny_until=0.05)
    want, refs, _, _ = pybam.columns(path, [1, 1, 1])
    assert len(want["flag"]) == 2000
    h = hostio.BamFile(path)
    h.set_main_chrom(np.ones(3, np.uint8))
    host = [dict((k, np.array(v, copy=True)) for k, v in x.items() if isinstance(v, np.ndarray)) for x in h.batches(1234)]
    h.close()
    host = {k: np.concatenate([c[k] for c in host]) for k in host[0]}
    same(want, host)
    for env in ({}, {"BQC_GI_WAVE": "0"}):
        with monkeypatch.context() as mp:
            for k, v in env.items():
                mp.setenv(k, v)
            b = hostio.BamFile(path, gpu=0)
            b.set_main_chrom(np.ones(3, np.uint8))
            got = [dict((k, np.array(v, copy=True)) for k, v in x.items() if isinstance(v, np.ndarray)) for x in b.batches(1234)]
            handed = b.batches_handed_over
            b.close()
        got = {k: np.concatenate([c[k] for c in got]) for k in got[0]}
        same(want, got)
        same(host, got)
        assert handed == 0, env


# ---- the record rules (host/bam_record.h) on the card: the sweep files of tests/bam_sweeps.py ------------------------------------
def _digest(cols):
    import hashlib
    h = hashlib.sha256()
    for k in sorted(cols):
        h.update(np.ascontiguousarray(cols[k]).tobytes())
    return h.hexdigest()


def _sweep_columns(path, batch_reads, **kw):
    """(columns, batches handed over) of a sweep file, every reference a main chromosome as in pybam.columns"""
    b = hostio.BamFile(path, **kw)
    b.set_main_chrom(np.ones(2, np.uint8))
    got = [dict((k, np.array(v, copy=True)) for k, v in x.items() if isinstance(v, np.ndarray)) for x in b.batches(batch_reads)]
    handed = b.batches_handed_over if "gpu" in kw else 0
    info = b.range_info
    b.close()
    return {k: np.concatenate([c[k] for c in got]) for k in got[0]}, handed, info


@pytest.fixture(scope="module")
def sweeps(tmp_path_factory):
    """{name: (path, columns by the independent decoder, columns by the host reader)}"""
    from tests import bam_sweeps, pybam
    d = tmp_path_factory.mktemp("sweeps")
    out = {}
    for name, write in (("tags", bam_sweeps.tag_sweep), ("sizes", bam_sweeps.size_sweep)):
        p = str(d / (name + ".bam"))
        write(p)
        out[name] = (p, pybam.columns(p)[0], _sweep_columns(p, 1 << 20)[0])
    return out


@pytest.mark.parametrize("name", ["tags", "sizes"])
def test_sweep_files_through_the_reader_on_the_card(sweeps, name):
    """Every column as the independent decoder and the host reader have it — decoded on the card: no batch went through the host decoder."""
    path, want, host = sweeps[name]
    for batch_reads in (257, 1 << 20):
        gpu, handed, _ = _sweep_columns(path, batch_reads, gpu=0)
        assert handed == 0
        same(want, gpu)
        same(host, gpu)


def test_tag_sweep_with_a_second_nm_is_handed_over(tmp_path):
    """One second NM tag, in a record whose fields cross the end of the card's stage: that batch goes to the host decoder, with the
    host reader's columns and extra values."""
    from tests import bam_sweeps
    path = str(tmp_path / "nm2.bam")
    bam_sweeps.tag_sweep(path, second_nm=True)
    host, _, _ = _sweep_columns(path, 1 << 20)
    assert len(host["nm_extra_read"]) == 1 and host["nm_extra_val"][0] == 77
    gpu, handed, _ = _sweep_columns(path, 1 << 20, gpu=0)
    assert handed == 1
    same(host, gpu)


def test_tag_sweep_with_a_field_cut_short_is_the_same_error(tmp_path):
    from tests import bam_sweeps
    path = str(tmp_path / "cut.bam")
    bam_sweeps.tag_sweep(path, cut_last=True)
    said = []
    for kw in ({}, {"gpu": 0}):
        with pytest.raises(IOError) as e:
            _sweep_columns(path, 1 << 20, **kw)
        said.append(str(e.value))
    assert said[0] == said[1] and "corrupt BAM tags" in said[0]


def test_size_sweep_in_three_shards(sweeps):
    """Shards that start in the middle of the file: the card guesses their first record (k_gb_walk*: exact == UINT64_MAX) where the
    host range reader does; same columns, same chain words."""
    path, want, _ = sweeps["sizes"]
    parts = []
    for lo, hi in _shard_hints(path, 3):
        h, _, hinfo = _sweep_columns(path, 1 << 20, begin_hint=lo, end_hint=hi)
        g, handed, ginfo = _sweep_columns(path, 257, begin_hint=lo, end_hint=hi, gpu=0)
        assert handed == 0 and ginfo == hinfo, (lo, hi)
        same(h, g)
        parts.append(g)
    same(want, {k: np.concatenate([p[k] for p in parts]) for k in parts[0]})


def test_lane_per_segment_walk_kernel_reads_the_sweep_files_alike(sweeps):
    """BQC_GB_WALK=lane (k_gb_walk, a lane per segment) in a fresh process — the switch is read once per process — against the
    default kernel (k_gb_walk_wave) here: the same bytes in every column of both files.  Which kernel walked is what the reader's
    BQC_GB_TIMING line says of every batch."""
    import os, subprocess, sys, textwrap
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    paths = [sweeps[name][0] for name in ("tags", "sizes")]
    prog = textwrap.dedent("""
        import sys
        sys.path.insert(0, %r)
        from tests.test_gpu_reader import _digest, _sweep_columns
        for path in %r:
            for batch_reads in (257, 1 << 20):
                cols, handed, _ = _sweep_columns(path, batch_reads, gpu=0)
                print(_digest(cols), handed)
        """) % (root, paths)
    r = subprocess.run([sys.executable, "-c", prog], env=dict(os.environ, BQC_GB_WALK="lane", BQC_GB_TIMING="1"), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert r.stderr.count("(a lane per segment)") >= 4 and "(a wave per segment)" not in r.stderr, r.stderr
    here = []
    for path in paths:
        for batch_reads in (257, 1 << 20):
            cols, handed, _ = _sweep_columns(path, batch_reads, gpu=0)
            here.append("%s %d" % (_digest(cols), handed))
    assert r.stdout.split("\n")[:-1] == here and all(x.endswith(" 0") for x in here)
