"""GPU: the adapter content by cycle (bqc_modules.adapter_by_cycle through bqc_create_ex, --adapter-by-cycle;
bamqc_amd/csrc/k_adp.hip) against the plain restatement of the statistic (tests/adp_ref.py): the views, and the whole module block
of the exported state.

A lane of the kernel owns 16 stored bases and looks 15 ahead, through aligned dwords of a payload whose reads start at any byte;
a read's lanes meet in an LDS slot per adapter; [2 mates][9 rows][1024 cycles] are counted in LDS for one read group at a time and
everything behind in device memory.  The shapes below cross each of those edges.

Not here: a read whose read group is n_lanes or more.  The pre-pass refuses such a batch as a whole (error key 2), so the rule of the
definition cannot be reached through the library; the restatement's side of it is in tests/test_adapter_by_cycle_cpu.py."""
import os
import subprocess

import numpy as np
import pytest

from bamqc_amd import Aggregator, BamQCError, hostio
from tests import adp_ref, adp_steps, pybam
from tests.adp_steps import FIRST, LAST, MAIN, P, REV, as_stored, cols_of, cols_of_nibbles
from tests.long_layout import dna_ref
from tests.parity import split
from tests.test_gpu_value_limits import n_cu

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "bin", "bamqualcheck")
ERR_ARG, ERR_STATE = 1, 8
UNI = "AGATCGGAAGAG"  # Illumina_Universal, slot 0 of the built-in set
LENGTHS = list(range(1, 71)) + [127, 128, 129, 255, 256, 257, 300, 1023, 1024, 1025]
ROWS = adp_ref.ROWS


def context(ref_len, n_lanes, N, adapters=None, **more):
    a = Aggregator(n_lanes=n_lanes, adapter_by_cycle=N, adapters=adapters, **dict(dict(n_refs=1, max_read_len=4096, isize=2000), **more))
    a.set_reference(0, dna_ref(77, ref_len))
    return a


def module_words(a, n_lanes, N, behind=0):
    """The module's words of the flat state vector: n_lanes x 2 x 9 x N, `behind` words from its end."""
    v = a.state_export_host()
    return v[len(v) - behind - n_lanes * 2 * ROWS * N:len(v) - behind].reshape(n_lanes, 2, ROWS, N)


def check_views(a, T, adapters=None):
    adapters = adapters or adp_ref.BUILTIN
    for l in range(T.shape[0]):
        for m in range(2):
            e, f, names = a.adapter_by_cycle(l, m)
            nc = adp_ref.sizes(T[l, m])
            assert names == list(adapters)
            assert e.shape == (nc,) and f.shape == (len(adapters), nc), (l, m, e.shape, f.shape, nc)
            assert np.array_equal(e, T[l, m, adp_ref.E_ROW, :nc]), (l, m)
            bad = np.argwhere(f != T[l, m, :len(adapters), :nc])
            assert not len(bad), "lane %d mate %d: %d bins differ, first (adapter, cycle) = %s: %d != %d" % (
                l, m, len(bad), bad[0].tolist(), f[tuple(bad[0])], T[l, m][tuple(bad[0])])


def run_and_check(cols, ref_len, n_lanes, N, adapters=None, **more):
    """One batch through a fresh context: the views and the whole block against the restatement -> the table."""
    T = adp_ref.table(cols, n_lanes, N, adapters)
    a = context(ref_len, n_lanes, N, adapters, **more)
    a.submit(cols)
    a.finalize()
    check_views(a, T, adapters)
    got = module_words(a, n_lanes, N)
    bad = np.argwhere(got != T)
    assert not len(bad), "%d words differ, first (lane, mate, row, cycle) = %s: %d != %d" % (len(bad), bad[0].tolist(), got[tuple(bad[0])], T[tuple(bad[0])])
    a.close()
    return T


def background(rng, L):
    return "".join(rng.choice(list("ACGT"), L))


def planted(rng, L, at, adapter):
    """A read of L bases in sequencing orientation with the adapter at cycle `at`, cut off at the read's end where it does not fit."""
    s = background(rng, L)
    return (s[:at] + adapter + s[at + len(adapter):])[:L]


# ---------------------------------------------------------------------------------------------------------------------------
# 1. positions
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sweep():
    """Every length of LENGTHS, both strands, both mates, the adapter at every start 0 .. 33, at L - m and (cut off) at L - m + 1."""
    rng = np.random.default_rng(11)
    m = len(UNI)
    reads = []
    for L in LENGTHS:
        for k, (rev, mate) in enumerate(((False, FIRST), (True, FIRST), (False, LAST), (True, LAST))):
            starts = [s for s in range(34) if s < L] + [L - m, L - m + 1]
            if L > 70:
                starts = starts[k::4] + [L - m, L - m + 1]  # (the long ones: a quarter of the starts per strand and mate)
            for s in starts:
                if s >= 0:
                    reads.append((as_stored(planted(rng, L, s, UNI), rev), P | MAIN | mate | (REV if rev else 0)))
            reads.append((as_stored(background(rng, L), rev), P | MAIN | mate | (REV if rev else 0)))
    # inside an occurrence: an N, an ambiguity code, a `=`; two occurrences on a forward and on a reverse read
    for rev in (False, True):
        f = P | MAIN | FIRST | (REV if rev else 0)
        for x in "NM=":
            reads.append((as_stored("GGTT" + UNI[:7] + x + UNI[8:] + "CC", rev), f))
        reads.append((as_stored("G" * 9 + UNI + "CCTCC" + UNI + "GG", rev), f))
        reads.append((as_stored("G" * 21 + UNI + UNI, rev), f))
    # the seam: a read that ends in eleven A (stored), directly followed in the payload by one that begins with A — with and without a
    # pad nibble between them; the same for T, which is what a reverse read is searched for
    for x in "AT":
        for L in (30, 31):
            for rev in (False, True):
                reads.append(("C" * (L - 11) + x * 11, P | MAIN | FIRST | (REV if rev else 0)))
                reads.append((x * 6 + "C" * 20, P | MAIN | LAST | (REV if rev else 0)))
    reads.append(("=" * 40, P | MAIN | FIRST))
    reads.append(("=" * 33, P | MAIN | LAST | REV))
    order = rng.permutation(len(reads))  # (lengths and kinds mixed: a step's lanes per read follow its longest)
    reads = [reads[i] for i in order] + reads[-18:]  # (the seam pairs once more, next to each other)
    return cols_of(reads)


@pytest.mark.parametrize("N", [1024, 16, 300])
def test_positions(sweep, N):
    cols, ref_len = sweep
    T = run_and_check(cols, ref_len, 1, N)
    assert T[0, 0, 0].any() and T[0, 1, 0].any() and not T[0, :, 6:8].any()
    if N == 1024:
        assert T[0, :, 0].sum(axis=0)[:34].all() and T[0, 0, 0, 1013] and T[0, 0, 0, 1012]  # every start, and L - m of 1025 and 1024


def test_short_batches_keep_their_lanes_per_read():
    """Batches of one length class each: the lanes a read gets follow the step's longest read (1, 2, 4, 8 ... 64 lanes)."""
    rng = np.random.default_rng(12)
    for L in (12, 16, 17, 33, 64, 65, 150, 513, 1025, 2100):
        reads = [(as_stored(planted(rng, L, s, UNI), rev), P | MAIN | FIRST | (REV if rev else 0)) for s in range(0, L, 3) for rev in (False, True)]
        cols, ref_len = cols_of(reads)
        T = run_and_check(cols, ref_len, 1, 4096)
        assert T[0, 0, 0].sum() >= 2 * len([s for s in range(0, L, 3) if s + len(UNI) <= L])


# ---------------------------------------------------------------------------------------------------------------------------
# 2. sets
# ---------------------------------------------------------------------------------------------------------------------------
SET3 = [("a8", "ACCAGGTA"), ("a12", "TGGAATTCTCGG"), ("a16", "TTGACCAGTACCGGTA")]
SET8 = SET3 + [("b8", "GGGGGGGG"), ("b9", "CATCATCAT"), ("b15", "ACGTTGCAACGTTGC"), ("b16", "T" * 16), ("b10", "GATTACAGAT")]


@pytest.mark.parametrize("adapters", [SET3, SET8, [("one", "CTGTCTCTTATACACA")], None], ids=["8-12-16", "eight", "one", "built-in"])
def test_sets(adapters):
    rng = np.random.default_rng(13)
    use = adapters or adp_ref.BUILTIN
    reads = []
    for L in (16, 31, 32, 47, 48, 90, 150):
        for name, seq in use:
            for s in sorted({0, 1, 15, 16, 17, L - len(seq) - 1, L - len(seq), L - len(seq) + 1}):
                if 0 <= s < L:
                    for rev in (False, True):
                        reads.append((as_stored(planted(rng, L, s, seq), rev), P | MAIN | (FIRST if s & 1 else LAST) | (REV if rev else 0)))
    # one read holding four different adapters (each counted once, at its own cycle), forward and reverse
    four = "".join("GC" + seq for name, seq in (use * 4)[:4]) + "CG"
    reads += [(four, P | MAIN | FIRST), (as_stored(four, True), P | MAIN | FIRST | REV)]
    cols, ref_len = cols_of(reads)
    T = run_and_check(cols, ref_len, 1, 1024, adapters)
    assert all(T[0, :, s].any() for s in range(len(use))) and not T[0, :, len(use):8].any()
    if len(use) >= 4:
        at = np.cumsum([2] + [len(seq) + 2 for name, seq in use[:3]])
        assert all(T[0, 0, s, at[s]] >= 2 for s in range(4))


# ---------------------------------------------------------------------------------------------------------------------------
# 3. counters: 70 000 increments of one E bin and one F bin in one launch
# ---------------------------------------------------------------------------------------------------------------------------
def test_70000_identical_reads():
    n, read = 70_000, "CGC" + UNI + "GTTAC"
    lut = {c: i for i, c in enumerate(adp_steps.CODES)}
    cols, ref_len = cols_of_nibbles(np.tile(np.array([lut[c] for c in read], np.uint8), n), np.full(n, len(read)), np.full(n, P | MAIN | FIRST))
    a = context(ref_len, 1, 1024)
    a.submit(cols)
    a.finalize()
    e, f, names = a.adapter_by_cycle(0, 0)
    want_e, want_f = np.zeros(20, np.uint64), np.zeros((6, 20), np.uint64)
    want_e[19], want_f[0, 3] = n, n
    assert np.array_equal(e, want_e) and np.array_equal(f, want_f)
    assert a.adapter_by_cycle(0, 1)[0].shape == (0,)
    assert module_words(a, 1, 1024).sum() == 2 * n
    a.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 4. read groups, and reads that are not examined
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def groups():
    """Three read groups: alternating read by read, then in runs of 1, 2 and 700 reads; one read in ten is not examined (secondary,
    supplementary, or a secondary record without a mate flag), some are unmapped, duplicates or without qualities (examined)."""
    rng = np.random.default_rng(14)
    lane = [i % 3 for i in range(60)]
    for g, run in ((0, 1), (1, 2), (2, 700), (0, 2), (1, 700), (2, 1), (0, 700), (1, 1)):
        lane += [g] * run
    reads = []
    for i in range(len(lane)):
        L = int(rng.choice([16, 40, 150, 255, 256, 300]))
        rev = bool(rng.random() < 0.5)
        mate = FIRST if rng.random() < 0.5 else LAST
        kind = rng.random()
        f = P | MAIN | (REV if rev else 0)
        f |= (mate | 0x100) if kind < 0.04 else (mate | 0x800) if kind < 0.08 else 0x100 if kind < 0.1 else (mate | 0x4) if kind < 0.15 else (mate | 0x400) if kind < 0.2 else (mate | 0x8000) if kind < 0.25 else mate
        seq = adp_ref.BUILTIN[int(rng.integers(0, 6))][1]
        s = planted(rng, L, int(rng.integers(0, L)), seq) if rng.random() < 0.7 else background(rng, L)
        reads.append((as_stored(s, rev), f))
    cols, ref_len = cols_of(reads, lane=lane)
    noq = np.repeat((cols["flag"] & 0x8000) != 0, cols["l_seq"].astype(np.int64))
    cols["qual"][noq] = 0xFF
    return cols, ref_len


def test_read_groups_one_batch_and_three(groups, tmp_path):
    cols, ref_len = groups
    T = run_and_check(cols, ref_len, 3, 1024)
    assert all(T[l, m, r].any() for l in range(3) for m in range(2) for r in (0, 1, 2, 3, 4, 5, 8))
    b = context(ref_len, 3, 1024)
    for part in split(cols, [7, 1300]):
        b.submit(part)
    b.finalize()
    check_views(b, T)
    assert np.array_equal(module_words(b, 3, 1024), T)
    out = str(tmp_path / "groups.adp")  # the text through the library's writer, lanes in an order of the caller's
    b.write_adapter_by_cycle(out, "S", ["g2", "g0", "g1"], [2, 0, 1])
    assert open(out).read() == adp_ref.text(T, "S", ["g2", "g0", "g1"], [2, 0, 1])
    b.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 5. more than one step per workgroup
# ---------------------------------------------------------------------------------------------------------------------------
def test_three_steps_per_workgroup():
    """More than 2 x 1024 x (CU count) reads of 20 bases in three read groups, one change exactly on a step's seam, one inside a step."""
    lay = adp_steps.step_layout(n_cu())
    adp_steps.assert_step_layout(lay)
    n = lay["n"]
    rng = np.random.default_rng(15)
    adapters = [("a8", "ACCAGGTA"), ("a12", UNI)]
    nib = np.array([1, 2, 4, 8], np.uint8)[rng.integers(0, 4, (n, 20))]
    flag = (P | MAIN | np.where(rng.random(n) < 0.5, REV, 0) | np.where(rng.random(n) < 0.5, FIRST, LAST)).astype(np.uint16)
    lut = {c: i for i, c in enumerate(adp_steps.CODES)}
    for k, (name, seq) in enumerate(adapters):  # planted in one read in eight each, forward and reverse-complemented, at any start (some cut off)
        rows = np.flatnonzero(np.arange(n) % 8 == 3 * k)
        at = rng.integers(0, 20, len(rows))
        fw = np.array([lut[c] for c in seq], np.uint8)
        rc = np.array([lut[c] for c in as_stored(seq, True)], np.uint8)
        for j in range(len(seq)):
            ok = at + j < 20
            nib[rows[ok], (at + j)[ok]] = np.where((flag[rows[ok]] & REV) != 0, rc[j], fw[j])
    cols, ref_len = cols_of_nibbles(nib.reshape(-1), np.full(n, 20), flag, lay["lane"])
    T = adp_ref.table_fast(cols, 3, 64, adapters)
    assert all(T[l, m, s].sum() > 1000 for l in range(3) for m in range(2) for s in (0, 1))
    a = context(ref_len, 3, 64, adapters)
    a.submit(cols)
    a.finalize()
    check_views(a, T, adapters)
    assert np.array_equal(module_words(a, 3, 64), T)
    a.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 6. long reads
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1024, 10_240])
def test_long_reads(N):
    rng = np.random.default_rng(16)
    m = len(UNI)
    reads = []
    for L in (10_000, 10_300):
        for rev in (False, True):
            f = P | MAIN | FIRST | (REV if rev else 0)
            for s in (0, 1023, 1024, 1025, 5000, N - 1, N, L - m, L - m + 1):
                if s < L:
                    reads.append((as_stored(planted(rng, L, s, UNI), rev), f ^ (FIRST | LAST if s & 1 else 0)))
            two = planted(rng, L, 7000, UNI)
            reads.append((as_stored(two[:9000] + UNI + two[9000 + m:], rev), f))  # two occurrences
    # a reverse read of 10 000 bases whose hit lies at stored position 0: cycle L - m
    stored0 = as_stored(UNI, True) + background(rng, 10_000 - m)
    reads.append((stored0, P | MAIN | LAST | REV))
    reads += [(planted(rng, 150, 60, UNI), P | MAIN | FIRST), (planted(rng, 20, 3, UNI), P | MAIN | LAST)]  # (short ones in the same step)
    cols, ref_len = cols_of(reads)
    T = run_and_check(cols, ref_len, 1, N, max_read_len=16_384)
    hits = T[0, :, 0].sum(axis=0)
    assert hits[1023] >= 4 and hits[N - 1] >= (4 if N <= 10_000 else 2)
    if N > 1024:
        assert hits[1024] >= 4 and T[0, 1, 0, 10_000 - m] >= 1 and T[0, :, adp_ref.E_ROW, 9_999].sum() >= 10 and T[0, :, adp_ref.E_ROW, N - 1].sum() >= 10


# ---------------------------------------------------------------------------------------------------------------------------
# 7. state
# ---------------------------------------------------------------------------------------------------------------------------
def test_state_words_and_order(groups):
    cols, ref_len = groups
    ref = dna_ref(77, ref_len)
    base = dict(n_lanes=3, n_refs=1, max_read_len=4096, isize=2000)
    off = Aggregator(**base)
    off.set_reference(0, ref)
    on = context(ref_len, 3, 16)
    assert on.state_words == off.state_words + 3 * 2 * 9 * 16
    all3 = context(ref_len, 3, 16, qual_by_cycle=8, mismatch_by_cycle=4)
    qbc = Aggregator(qual_by_cycle=8, **base)
    qbc.set_reference(0, ref)
    mbc = Aggregator(mismatch_by_cycle=4, **base)
    mbc.set_reference(0, ref)
    n_q, n_m = 3 * 2 * 8 * 224, 3 * 2 * 2 * 4 * 224
    assert all3.state_words == off.state_words + 3 * 2 * 9 * 16 + n_q + n_m
    for a in (off, on, all3, qbc, mbc):
        a.submit(cols)
    v_off, v_on, v3 = off.state_export_host(), on.state_export_host(), all3.state_export_host()
    T = adp_ref.table(cols, 3, 16)
    assert np.array_equal(v_on[:len(v_off)], v_off) and np.array_equal(v_on[len(v_off):].reshape(3, 2, 9, 16), T)
    # with all three modules on the last words are still qual_by_cycle's, the ones in front of them mismatch_by_cycle's
    assert np.array_equal(v3[len(v3) - n_q:], qbc.state_export_host()[-n_q:]) and v3[len(v3) - n_q:].any()
    assert np.array_equal(v3[len(v3) - n_q - n_m:len(v3) - n_q], mbc.state_export_host()[-n_m:])
    assert np.array_equal(module_words(all3, 3, 16, behind=n_q + n_m), T)
    assert np.array_equal(v3[:len(v_off)], v_off)
    # a context made by plain bqc_create has no such table
    off.finalize()
    with pytest.raises(BamQCError) as e:
        off.adapter_by_cycle(0, 0)
    assert e.value.code == ERR_STATE
    on.finalize()
    for lane, mate in ((3, 0), (0, 2)):
        with pytest.raises(BamQCError) as e:
            on.adapter_by_cycle(lane, mate)
        assert e.value.code == ERR_ARG
    for a in (off, on, all3, qbc, mbc):
        a.close()
    with pytest.raises(BamQCError) as e:  # a capacity behind max_read_len is refused
        Aggregator(adapter_by_cycle=4097, **base)
    assert e.value.code == ERR_ARG
    with pytest.raises(BamQCError) as e:
        Aggregator(adapters=[("x", "ACGT")], adapter_by_cycle=16, **base)
    assert e.value.code == ERR_ARG


def test_sums_reset_and_replay(groups):
    cols, ref_len = groups
    n = len(cols["flag"])
    T = adp_ref.table(cols, 3, 300)
    vecs = []
    for part in split(cols, [n // 2 + 3]):
        a = context(ref_len, 3, 300)
        a.submit(part)
        vecs.append(a.state_export_host())
        a.close()
    c = context(ref_len, 3, 300)
    c.state_import_host(vecs[0] + vecs[1])  # export + import into a fresh context adds
    assert np.array_equal(module_words(c, 3, 300), T)
    c.finalize()
    check_views(c, T)
    c.reset()
    with pytest.raises(BamQCError) as e:  # (nothing finalised since the reset)
        c.adapter_by_cycle(0, 0)
    assert e.value.code == ERR_STATE
    assert not module_words(c, 3, 300).any()
    c.finalize()
    assert c.adapter_by_cycle(0, 0)[0].shape == (0,) and c.adapter_by_cycle(0, 0)[1].shape == (6, 0)
    c.reset()
    d = c.upload(cols)
    c.process(d)
    c.process(d)  # two batches add
    c.finalize()
    assert np.array_equal(module_words(c, 3, 300), 2 * T)
    check_views(c, 2 * T)
    d.free()
    c.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 8. the program
# ---------------------------------------------------------------------------------------------------------------------------
CHROMS = ["-c", "chr1,chr2"]


def run(args, env=None, **kw):
    return subprocess.run([EXE] + args, capture_output=True, env=dict(os.environ, **(env or {})), timeout=120, **kw)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """About 20 000 synthetic paired reads in two read groups, the `.bamqc` of a run without the option, and the expected text.
    X: an adapter the file's reads do hold — the first twelve cycles of its first read."""
    d = tmp_path_factory.mktemp("adp")
    bam, fa = str(d / "in.bam"), str(d / "in.fa")
    hostio.synth_write(bam, fa, seed=21, n_reads=20_000, ref_names=["chr1", "chr2"], ref_lens=[400_000, 150_000], n_lanes=2)
    base = str(d / "base.bamqc")
    r = run(["-r", fa, "-o", base] + CHROMS + [bam])
    assert r.returncode == 0, r.stderr
    assert not os.path.exists(base + ".adp")
    cols, refs, lanes, sample = pybam.columns(bam)
    assert len(lanes) == 2
    names = sorted(lanes)  # the `.bamqc` lists the lanes by name
    idx = [lanes[nm] for nm in names]
    first = adp_ref.stored(cols, 0, 0)
    x = as_stored(first, bool(cols["flag"][0] & 0x10))[:12]
    assert set(x) <= set("ACGT")
    X = [("X", x[:8]), ("X12", x)]

    def want(N, adapters=None):
        return adp_ref.text(adp_ref.table_fast(cols, 2, N, adapters), sample, names, idx, adapters)
    assert adp_ref.table_fast(cols, 2, 1024, X)[:, :, 0].sum() > 20  # (an 8-mer: about one read in 450 holds it somewhere)
    return dict(dir=d, bam=bam, fa=fa, base=base, want=want, X=X, x_args=["--adapter", "X=" + x[:8], "--adapter=X12=" + x])


def same_bytes(a, b):
    return open(a, "rb").read() == open(b, "rb").read()


@pytest.mark.parametrize("decode", ["0", "1"])
def test_program_bam(files, decode):
    out = str(files["dir"] / ("bam%s.bamqc" % decode))
    r = run(["-r", files["fa"], "-o", out, "--adapter-by-cycle"] + CHROMS + [files["bam"]], env=dict(BQC_GPU_DECODE=decode))
    assert r.returncode == 0, r.stderr
    assert same_bytes(out, files["base"])
    assert open(out + ".adp").read() == files["want"](1024)


def test_program_adapter_replaces_the_built_in_set(files):
    out = str(files["dir"] / "x.bamqc")
    r = run(["-r", files["fa"], "-o", out] + files["x_args"] + CHROMS + [files["bam"]])
    assert r.returncode == 0, r.stderr
    assert same_bytes(out, files["base"])
    text = open(out + ".adp").read()
    assert text == files["want"](1024, files["X"]) and "Illumina" not in text and " X12 " in text


def test_program_sam_on_stdin(files):
    out = str(files["dir"] / "sam.bamqc")
    sam = pybam.bam_to_sam_text(files["bam"]).encode()
    r = run(["-r", files["fa"], "-o", out, "--adapter-by-cycle-len", "100"] + files["x_args"] + CHROMS + ["-"], input=sam)
    assert r.returncode == 0, r.stderr
    assert same_bytes(out, files["base"])
    assert open(out + ".adp").read() == files["want"](100, files["X"])


def test_program_two_workers_on_one_card(files):
    out = str(files["dir"] / "gpus2.bamqc")
    r = run(["--gpus", "2", "-r", files["fa"], "-o", out, "--adapter-by-cycle"] + files["x_args"] + CHROMS + [files["bam"]], env=dict(BQC_GPUS_SHARE_DEVICE="1"))
    assert r.returncode == 0, r.stderr
    assert same_bytes(out, files["base"])
    assert open(out + ".adp").read() == files["want"](1024, files["X"])


@pytest.mark.parametrize("which", ["built-in", "X"])
def test_program_manifest(files, which):
    """Two jobs through one resident worker, once per adapter set (a list's jobs share the command line's options)."""
    d = files["dir"]
    outs = [str(d / ("m1%s.bamqc" % which)), str(d / ("m2%s.bamqc" % which))]
    lst = str(d / ("jobs%s.tsv" % which))
    with open(lst, "w") as f:
        for o in outs:
            f.write("%s\t%s\n" % (files["bam"], o))
    extra, adapters = (files["x_args"], files["X"]) if which == "X" else ([], None)
    r = run(["-r", files["fa"], "--adapter-by-cycle-len", "300", "--manifest", lst] + extra + CHROMS)
    assert r.returncode == 0, r.stderr
    for o in outs:
        assert same_bytes(o, files["base"])
        assert open(o + ".adp").read() == files["want"](300, adapters)


def test_program_all_three_modules(files):
    d = files["dir"]
    two, three = str(d / "two.bamqc"), str(d / "three.bamqc")
    r = run(["-r", files["fa"], "-o", two, "--qual-by-cycle", "--mismatch-by-cycle"] + CHROMS + [files["bam"]])
    assert r.returncode == 0, r.stderr
    r = run(["-r", files["fa"], "-o", three, "--qual-by-cycle", "--mismatch-by-cycle", "--adapter-by-cycle"] + CHROMS + [files["bam"]])
    assert r.returncode == 0, r.stderr
    for ext in ("", ".qbc", ".mbc"):
        assert same_bytes(three + ext, two + ext), ext
    assert same_bytes(three, files["base"])
    assert open(three + ".adp").read() == files["want"](1024)


def test_program_reports_a_table_it_cannot_write(files):
    out = str(files["dir"] / "blocked.bamqc")
    os.mkdir(out + ".adp")  # (a directory where the table's file would go)
    r = run(["-r", files["fa"], "-o", out, "--adapter-by-cycle"] + CHROMS + [files["bam"]])
    assert r.returncode == 1
    assert b"Could not write output file" in r.stderr and b".adp" in r.stderr
