"""GPU: the hot-path kernels at the limits of their data layout — base qualities over the whole Phred byte range, and reads
longer than one row of k_long per CU.

k_short, k_long and the sketch turn the reference's signed-char quality arithmetic into byte-wise SWAR: a triplet position
counts for Phred 20..94 only ((signed char)(phred + 33) >= '5'); the sketch's SWAR branch covers the thresholds
(signed char)(33 + q) in 1..127, every other threshold is compared byte by byte; Phred > 222 is refused (q + 33 wraps a char);
k_short keeps per-cycle quality sums in 16-bit fields flushed every 255 groups.  Every test compares with the oracle AND with
a closed form computed here from the input columns (the oracle and the kernels share an author)."""
import filecmp
import os
import subprocess

import numpy as np
import pytest

from bamqc_amd import hostio
from tests import synth
from tests.cli_oracle import oracle_bamqualcheck
from tests.long_layout import dna_ref, expected_triplets, reads_on_ref  # (shared with the k_long layout tests)
from tests.parity import assert_parity, run_gpu, split

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "bin", "bamqualcheck")
ERR_RANGE = 6
QUAL_MSG = "base quality above 222 cannot be represented by the reference (q+33 wraps)"
SPECIAL = np.array([19, 20, 93, 94, 95, 96, 126, 127, 128, 221, 222], np.uint8)
EMPTY_SKETCH = (0, 9223372036854775808, 9223372036854775808, 0)  # sumCount F0 f1 F2 of a sketch that saw no k-mer
KL_ROW = 992


def band_quals(rng, n):
    """Phred 0..222: half uniform, half the values where a signed-char rule flips (19/20, 94/95, 127/128, 222)."""
    q = rng.integers(0, 223, n).astype(np.uint8)
    pick = rng.random(n) < 0.5
    q[pick] = SPECIAL[rng.integers(0, len(SPECIAL), int(pick.sum()))]
    return q


def with_band_quals(cols, seed):
    cols = dict(cols)
    q = band_quals(np.random.default_rng(seed), cols["qual"].size)
    cols["qual"] = np.where(cols["qual"] == 0xFF, 0xFF, q).astype(np.uint8)  # (reads without qualities stay so)
    return cols


def signed(b):
    return ((np.asarray(b, np.int64) + 128) % 256) - 128


def qual_passes(phred, q):
    """ReadQualityHasher's test: (signed char)(phred + 33) >= (signed char)(q + 33)."""
    return signed(np.asarray(phred) + 33) >= signed(q + 33)


def uniform_batch(seed, n, L, phred, ref, reverse_every=2):
    """n primary first-mate reads of length L, all-M on the reference, every base of Phred `phred`, a part on the reverse strand."""
    rng = np.random.default_rng(seed)
    pos = np.sort(rng.integers(0, len(ref) - L + 1, n))
    flag = np.full(n, 0x1 | 0x2 | 0x40 | 0x1000, np.uint16)
    flag[::reverse_every] |= 0x10
    return reads_on_ref(ref, pos, np.full(n, L), flag, np.full(n * L, phred, np.uint8))


def n_cu():
    """The CU count of device 0, from the HIP runtime the library is linked against (tests/hipmem.py: torch brings a runtime of
    its own, which finds no GPU in a process that has used the card already)."""
    import ctypes as C
    from tests.hipmem import Hip
    v = C.c_int(0)
    assert Hip().rt.hipDeviceGetAttribute(C.byref(v), 63, 0) == 0  # 63: hipDeviceAttributeMultiprocessorCount
    assert v.value > 0
    return v.value


# ---------------------------------------------------------------------------------------------------------------------------
# 1. quality bands on every path
# ---------------------------------------------------------------------------------------------------------------------------
BAND_SKETCH = dict(klist=[5, 31], qlist=[17, 95, 128])


@pytest.mark.parametrize("path", ["k_short", "k_long", "generic"])
def test_quality_bands_every_path(path, monkeypatch):
    if path == "generic":
        monkeypatch.setenv("BQC_NO_FAST", "1")
    if path == "k_long":
        cols, refs = synth.synth(seed=41, n_reads=1500, L=700, n_refs=1, ref_len=400_000, long_cigar=True, var_len=True)
        opts = dict(max_read_len=1024, isize=2000)
    else:
        cols, refs = synth.synth(seed=42, n_reads=8000, n_refs=2, ref_len=150_000, var_len=True, p_noqual=0.01)
        opts = {}
    cols = with_band_quals(cols, 7)
    q = cols["qual"]
    assert (q == 95).any() and (q == 128).any() and (q == 222).any() and q[q != 0xFF].max() == 222
    assert (cols["flag"] & 0x10).any() and (~cols["flag"] & 0x10).any()
    co, cg, _, _ = assert_parity(split(cols, [len(cols["flag"]) // 3]), refs, **BAND_SKETCH, **opts)
    # independent of the oracle: the quality sums of the first mates (every primary record with qualities)
    fl = cols["flag"]
    L = cols["l_seq"].astype(np.int64)
    rid = np.repeat(np.arange(len(L)), L)
    first = ((fl & 0x40) != 0) & ((fl & 0x900) == 0) & ((fl & 0x8000) == 0)
    assert int(cg[0]["r1.qualcount"].sum()) == int(q[first[rid]].astype(np.int64).sum())
    assert int(cg[0]["triplet"].sum()) > 0


# ---------------------------------------------------------------------------------------------------------------------------
# 2. closed forms
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("phred,L", [(94, 150), (94, 255), (94, 700), (95, 150), (95, 700), (200, 255), (200, 700), (222, 255)])
def test_uniform_quality_closed_forms(phred, L):
    """One lane, primary first mates, all-M reads copied from an N-free contig, every base of one Phred value."""
    ref = dna_ref(3, 200_000)
    n = 3000 if L <= 255 else 600
    cols = uniform_batch(phred * 7 + L, n, L, phred, ref)
    k = 17
    co, cg, _, _ = assert_parity(split(cols, [n // 2]), [ref], klist=[k], qlist=[17], max_read_len=1024, isize=2000)
    g = cg[0]
    want = expected_triplets(ref, cols, phred)
    assert np.array_equal(g["triplet"], want)
    assert int(g["triplet"].sum()) == (n * (L - 2) if phred <= 94 else 0)
    sk = g["sketch"][0]
    if qual_passes(phred, 17):
        assert sk[:3] == (17, k, n * (L - k + 1))
    else:
        assert sk == (17, k) + EMPTY_SKETCH
    assert np.array_equal(g["r1.qualcount"], np.full(L, n * phred, np.uint64))
    assert g["r1.qualcount_readnr"] == n
    assert int(g["r1.averageQual"][phred]) == n and int(g["r1.averageQual"].sum()) == n
    dna = sum(g["r1.dnacount%d" % b] for b in range(5))
    assert np.array_equal(dna, np.full(L, n, np.uint64))


def test_phred_222_quality_sums_pass_the_255_group_flush():
    """k_short adds a cycle's qualities into 16-bit register fields and flushes them every 255 groups (k_short.hip:467):
    222 * 295 < 65536 < 222 * 296, so a wave that added 296 groups of Phred 222 without its flush would wrap.

    The chunk layout (k_prep.hip, k_short.hip): a batch whose longest fast read has 241..255 bases gets fast_w = 16 lanes per
    read, rpw = 64 / 16 = 4 read slots per group, the first h0 = 2 of them for first mates; a chunk holds BQC_FAST_WAVES * (64 /
    rpw) = 256 groups (512 first mates), and each of the 16 waves takes one tile of 16 groups of it.  k_short has one workgroup
    per CU and a workgroup walks every n_cu-th chunk, keeping its registers across chunks of one read group.  With
    n = 19 * n_cu * 512 first mates, every workgroup walks 19 chunks and every wave adds 19 * 16 = 304 groups: it passes the
    flush at least once, and without the flush the fields of the first cycles would wrap.  (One read in eight is 255 bases long,
    the others 16: the fields of cycles 0..15 see every group; the column bytes stay near 200 MB.)"""
    cu = n_cu()
    n = 19 * cu * 512
    L = np.where(np.arange(n) % 8 == 0, 255, 16)
    ref = dna_ref(11, 2_000_000)
    rng = np.random.default_rng(12)
    pos = np.sort(rng.integers(0, len(ref) - 256, n))
    flag = np.full(n, 0x1 | 0x2 | 0x40 | 0x1000, np.uint16)
    flag[rng.random(n) < 0.5] |= 0x10
    cols = reads_on_ref(ref, pos, L, flag, np.full(int(L.sum()), 222, np.uint8))
    co, cg, _, _ = assert_parity(cols, [ref], max_read_len=1024)
    g = cg[0]
    want = 222 * np.array([(L > j).sum() for j in range(255)], np.uint64)
    assert np.array_equal(g["r1.qualcount"], want)
    assert int(g["r1.averageQual"][222]) == n and int(g["r1.averageQual"].sum()) == n


# ---------------------------------------------------------------------------------------------------------------------------
# 3. sketch thresholds at the SWAR boundary
# ---------------------------------------------------------------------------------------------------------------------------
THRESHOLDS = [93, 94, 95, 127, 128, 222, 223]  # (signed char)(33 + q): 126, 127, -128, -96, -95, -1, 0


def test_sketch_thresholds_band_qualities():
    cols, refs = synth.synth(seed=51, n_reads=3000, n_refs=1, ref_len=120_000, var_len=True, p_noqual=0.01, p_iupac=0.005)
    cols = with_band_quals(cols, 52)
    co, cg, _, _ = assert_parity(split(cols, [1300]), refs, klist=[5, 31], qlist=THRESHOLDS)
    assert sorted(s[:2] for s in cg[0]["sketch"]) == sorted((q, k) for q in THRESHOLDS for k in (5, 31))


@pytest.mark.parametrize("L", [150, 700])
def test_sketch_thresholds_closed_form(L):
    """Reads of one Phred value each (eight values around the flips); every threshold's sketch counts every k-mer of the reads
    that pass the signed-char rule and none of the others: sumCount = sum over passing reads of L - k + 1."""
    phreds = [93, 94, 95, 126, 127, 128, 200, 222]
    ref = dna_ref(21, 300_000)
    n = 300 if L <= 255 else 100
    cols = synth.concat([uniform_batch(100 + i, n, L, p, ref) for i, p in enumerate(phreds)])
    order = np.argsort(cols["pos"], kind="stable")  # (coordinate sorted, as a BAM would be)
    cols = synth.concat([synth.slice_batch(cols, int(i), int(i) + 1) for i in order])
    k = 9
    co, cg, _, _ = assert_parity(cols, [ref], klist=[k], qlist=THRESHOLDS, max_read_len=1024, isize=2000)
    got = {s[0]: s for s in cg[0]["sketch"]}
    assert sorted(got) == sorted(THRESHOLDS)
    for q in THRESHOLDS:
        n_pass = sum(n for p in phreds if qual_passes(p, q))
        assert 0 < n_pass < len(phreds) * n or q in (95, 128)
        assert got[q][1:3] == (k, n_pass * (L - k + 1)), (q, got[q])


# ---------------------------------------------------------------------------------------------------------------------------
# 4. refusal of Phred > 222
# ---------------------------------------------------------------------------------------------------------------------------
SHAPES = {"k_short": (150, False), "k_long": (700, False), "generic": (150, True)}


def _bad_read_batch(L, where, value, reverse, seed):
    ref = dna_ref(31, 100_000)
    good = uniform_batch(seed, 300, L, 37, ref)
    bad = uniform_batch(seed + 1, 1, L, 37, ref)
    if reverse:
        bad["flag"] = bad["flag"] | 0x10
    else:
        bad["flag"] = bad["flag"] & ~np.uint16(0x10)
    bad["qual"] = bad["qual"].copy()
    bad["qual"][{"first": 0, "middle": L // 2, "last": L - 1}[where]] = value
    cols = synth.concat([synth.slice_batch(good, 0, 150), bad, synth.slice_batch(good, 150, 300)])
    return cols, ref


CASES = [(w, v) for v in (223, 254) for w in ("first", "middle", "last")] + [("middle", 255), ("last", 255)]


@pytest.mark.parametrize("shape", list(SHAPES))
def test_phred_above_222_is_refused(shape, monkeypatch):
    L, no_fast = SHAPES[shape]
    if no_fast:
        monkeypatch.setenv("BQC_NO_FAST", "1")
    for where, value in CASES:
        for reverse in (False, True):
            cols, ref = _bad_read_batch(L, where, value, reverse, 61)
            rc, _, a = run_gpu([cols], [ref], max_read_len=1024, isize=2000, klist=[17], qlist=[17])
            assert rc == ERR_RANGE, (shape, where, value, reverse, rc)
            msg = a.lib.bqc_last_error(a.h).decode()
            assert QUAL_MSG in msg, msg
            a.close()
    # the same reads with the byte at 222 pass, and match the oracle
    cols, ref = _bad_read_batch(L, "middle", 222, True, 61)
    assert_parity(cols, [ref], max_read_len=1024, isize=2000, klist=[17], qlist=[17])


@pytest.mark.parametrize("shape", list(SHAPES))
def test_read_without_qualities_is_not_refused(shape, monkeypatch):
    """A quality block that starts with 0xFF means "no qualities" (the decoder sets BQC_FLAG_NO_QUAL): its other
    bytes are never read, whatever they hold."""
    L, no_fast = SHAPES[shape]
    if no_fast:
        monkeypatch.setenv("BQC_NO_FAST", "1")
    ref = dna_ref(32, 100_000)
    good = uniform_batch(71, 200, L, 30, ref)
    nq = uniform_batch(72, 4, L, 30, ref)
    nq["flag"] = nq["flag"] | 0x8000
    q = np.random.default_rng(73).integers(223, 256, nq["qual"].size).astype(np.uint8)
    q[::L] = 0xFF
    nq["qual"] = q
    cols = synth.concat([synth.slice_batch(good, 0, 100), nq, synth.slice_batch(good, 100, 200)])
    co, cg, _, _ = assert_parity(cols, [ref], max_read_len=1024, isize=2000, klist=[17], qlist=[17])
    assert cg[0]["r1.qualcount_readnr"] == 204  # every read is counted, but the four without qualities add no quality sums
    assert np.array_equal(cg[0]["r1.qualcount"], np.full(L, 200 * 30, np.uint64))


def _cli_files(tmp, cols, ref):
    bam, fa = os.path.join(tmp, "q.bam"), os.path.join(tmp, "q.fa")
    hostio.write_bam(bam, cols, ["chr1"], [len(ref)])
    hostio.write_fasta(fa, ["chr1"], [ref])
    return bam, fa


@pytest.mark.parametrize("reader", ["0", "1"])
def test_cli_refuses_phred_above_222(tmp_path, reader):
    cols, ref = _bad_read_batch(150, "middle", 230, False, 81)
    bam, fa = _cli_files(str(tmp_path), cols, ref)
    out = str(tmp_path / "o.bamqc")
    r = subprocess.run([EXE, "-r", fa, "-o", out, "-c", "chr1", bam], capture_output=True, text=True,
                       env=dict(os.environ, BQC_GPU_DECODE=reader))
    assert r.returncode == 1, r.stderr  # (the program exits 1 on every library error, as the reference does)
    assert QUAL_MSG in r.stderr, r.stderr


# ---------------------------------------------------------------------------------------------------------------------------
# 5. reads longer than n_cu rows of k_long
# ---------------------------------------------------------------------------------------------------------------------------
def _long_read(rng, ref, L, clip, reverse, second):
    """One read of length L on the reference: soft clips (when `clip`), matches with a few insertions / deletions and
    substitutions; band qualities."""
    lead, trail = (37, 1000) if clip else (0, 0)
    body = L - lead - trail
    ops, parts = [], []
    if lead:
        ops.append((lead, "S"))
        parts.append(rng.integers(0, 4, lead).astype(np.uint8))
    span = body + 200
    p = int(rng.integers(0, len(ref) - span - 10))
    rp, left, nm = p, body, 0
    for m, ev in ((body // 3, ("I", 5)), (body // 3, ("D", 7))):
        ops.append((m, "M"))
        parts.append(ref[rp:rp + m].copy())
        rp += m
        left -= m
        ops.append((ev[1], ev[0]))
        if ev[0] == "I":
            parts.append(rng.integers(0, 4, ev[1]).astype(np.uint8))
            left -= ev[1]
        else:
            rp += ev[1]
        nm += ev[1]
    ops.append((left, "M"))
    parts.append(ref[rp:rp + left].copy())
    if trail:
        ops.append((trail, "S"))
        parts.append(rng.integers(0, 4, trail).astype(np.uint8))
    codes = np.concatenate(parts)
    assert len(codes) == L
    sub = np.nonzero(rng.random(L) < 1e-4)[0]
    codes[sub] = (codes[sub] + 1) % 4
    nibs = synth.NIB[codes]
    flag = 0x1 | 0x2 | (0x80 if second else 0x40) | 0x1000 | (0x10 if reverse else 0)
    return dict(flag=np.array([flag], np.uint16), mapq=np.array([60], np.uint8), lane=np.zeros(1, np.uint8),
                rid=np.zeros(1, np.int32), pos=np.array([p], np.int32), tlen=np.array([500], np.int32),
                nm=np.array([nm + len(sub)], np.int32), as_=np.array([L], np.int32), l_seq=np.array([L], np.uint32),
                n_cigar=np.array([len(ops)], np.uint16), seq=synth.pack_nibbles(nibs),
                qual=band_quals(rng, L), cigar=synth.cigar_words(ops))


def _by_pos(parts):
    cols = synth.concat(parts)
    order = np.argsort(cols["pos"], kind="stable")
    return synth.concat([synth.slice_batch(cols, int(i), int(i) + 1) for i in order])


def _long_lengths():
    cu = n_cu()
    return [cu * KL_ROW - 1, cu * KL_ROW, cu * KL_ROW + 1, 1_100_000]


LONG_OPTS = dict(max_read_len=1_100_000, hist_cap=4096, isize=2000, klist=[17], qlist=[17])


def _check_totals(cols, g):
    fl = cols["flag"]
    L = cols["l_seq"].astype(np.int64)
    rid = np.repeat(np.arange(len(L)), L)
    prim = ((fl & 0x900) == 0) & ((fl & 0x8000) == 0)
    for m, bit in (("r1", 0x40), ("r2", 0x80)):
        sel = prim & ((fl & bit) != 0)
        assert int(g[m + ".qualcount"].sum()) == int(cols["qual"][sel[rid]].astype(np.int64).sum()), m
        dna = sum(int(g[m + ".dnacount%d" % b].sum()) for b in range(5))
        assert dna == int(L[prim & ((fl & bit) != 0)].sum()), m


def test_long_reads_past_the_per_cu_rows():
    """Reads of n_cu * 992 - 1, n_cu * 992, n_cu * 992 + 1 and 1.1 M bases (more than 1024 rows): k_long's grid has more
    workgroups than the card has CUs.  Single reads, then all of them together with 150 bp reads (k_short's workgroups use the
    same scratch table in the same batch)."""
    ref = dna_ref(91, 1_400_000)
    rng = np.random.default_rng(92)
    lens = _long_lengths()
    longs = [_long_read(rng, ref, L, clip=(i % 2 == 1), reverse=(i % 2 == 0), second=(i == 2)) for i, L in enumerate(lens)]
    for r in longs:
        co, cg, _, _ = assert_parity(r, [ref], **LONG_OPTS)
        _check_totals(r, cg[0])
    short, _ = synth.synth(seed=93, n_reads=3000, n_refs=1, refs=[ref])
    cols = _by_pos(longs + [synth.slice_batch(short, i, i + 1) for i in range(0, 3000)])
    co, cg, _, _ = assert_parity(split(cols, [1000]), [ref], **LONG_OPTS)
    _check_totals(cols, cg[0])
    assert int(cg[0]["triplet"].sum()) > 0


def test_long_read_over_the_default_limit_is_refused_then_a_fresh_context_is_correct():
    ref = dna_ref(95, 400_000)
    rng = np.random.default_rng(96)
    bad = _long_read(rng, ref, 300_000, clip=False, reverse=False, second=False)
    short, _ = synth.synth(seed=97, n_reads=500, n_refs=1, refs=[ref])
    cols = synth.concat([synth.slice_batch(short, 0, 250), bad, synth.slice_batch(short, 250, 500)])
    rc, _, a = run_gpu([cols], [ref], max_read_len=65536, hist_cap=65536)
    assert rc == ERR_RANGE
    msg = a.lib.bqc_last_error(a.h).decode()
    assert "read 250 is 300000 bases long; max_read_len is 65536" in msg, msg
    a.close()
    good = _by_pos([_long_read(rng, ref, 60_000, clip=True, reverse=True, second=False), short])
    co, cg, _, _ = assert_parity(good, [ref], max_read_len=65536, hist_cap=65536)
    _check_totals(good, cg[0])


def test_cli_long_read_file(tmp_path):
    """One file with a read past n_cu rows and ordinary reads, through the program with --max-read-len raised: the same bytes as
    the oracle program."""
    ref = dna_ref(98, 600_000)
    rng = np.random.default_rng(99)
    L = n_cu() * KL_ROW + 1
    short, _ = synth.synth(seed=100, n_reads=2000, n_refs=1, refs=[ref])
    cols = _by_pos([_long_read(rng, ref, L, clip=True, reverse=True, second=False), short])
    bam, fa = _cli_files(str(tmp_path), cols, ref)
    got, want = str(tmp_path / "gpu.bamqc"), str(tmp_path / "oracle.bamqc")
    r = subprocess.run([EXE, "-r", fa, "-o", got, "-c", "chr1", "--max-read-len", str(L), bam], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert oracle_bamqualcheck(bam, fa, want, chroms="chr1", max_read_len=L) == 0
    assert filecmp.cmp(got, want, shallow=False)
