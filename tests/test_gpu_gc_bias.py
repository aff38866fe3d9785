"""GPU: the GC bias (bqc_enable_gc_bias, --gc-bias; bamqc_amd/csrc/k_gcb.hip) against the restatement of the statistic
(tests/gcb_ref.py): all four tables of the view word for word, and the module's block of the exported state.

k_gcb_genome takes shares of 8192 window starts, scans a share's dwords in runs of nine per thread and looks two prefix counts up per
start; k_gcb_reads gives a read a power of two of lanes, masks the first and last dword of the window and of the qualities, and keeps
3 x 101 words in LDS for one read group at a time.  The shapes below cross each of those edges.

Not here, because the library refuses the batch before the kernel sees it (the restatement's side of each is in
tests/test_gc_bias_cpu.py): a primary read without a mate flag (error key 6 of the pre-pass), a read group at or behind n_lanes
(error key 2), and a quality byte above 222 (BQC_ERR_RANGE from the per-read kernels) — the quality bytes here span 0 ... 222."""
import os
import subprocess

import numpy as np
import pytest

from bamqc_amd import Aggregator, BamQCError, _abi, hostio
from tests import gcb_ref, gcb_steps, pybam
from tests.gcb_steps import FIRST, LAST, MAIN, P, REV, cols_flat, cols_of
from tests.parity import split
from tests.test_gpu_value_limits import n_cu

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "bin", "bamqualcheck")
ERR_ARG, ERR_STATE = 1, 8
BINS = gcb_ref.BINS
A, C, G, T, N = 0, 1, 2, 3, 4


def context(refs, n_lanes, W, **more):
    a = Aggregator(n_lanes=n_lanes, gc_bias=W, **dict(dict(n_refs=len(refs), max_read_len=4096, isize=2000), **more))
    for rid, r in enumerate(refs):
        if r is not None:
            a.set_reference(rid, r)
    return a


def module_words(a, n_lanes, behind=0):
    """The module's words of the flat state vector: n_lanes x 3 x 101, `behind` words from its end."""
    v = a.state_export_host()
    return v[len(v) - behind - n_lanes * 3 * BINS:len(v) - behind].reshape(n_lanes, 3, BINS)


def check_views(a, Gw, Tw, W):
    for l in range(Tw.shape[0]):
        got = a.gc_bias(l)
        assert a.gc_bias_window == W and all(x.shape == (BINS,) and x.dtype == np.uint64 for x in got)
        for name, g, w in zip(("genome_windows", "read_starts", "bases", "qual_sum"), got, (Gw, Tw[l, 0], Tw[l, 1], Tw[l, 2])):
            bad = np.flatnonzero(g != w)
            assert not len(bad), "lane %d %s: %d bins differ, first %d: %d != %d" % (l, name, len(bad), bad[0], g[bad[0]], w[bad[0]])


def run_and_check(cols_list, refs, n_lanes, W, **more):
    """The batches through a fresh context: the views and the module's block against the restatement -> (G, T)."""
    Gw, Tw = gcb_ref.table_fast(cols_list, refs, n_lanes, W)
    a = context(refs, n_lanes, W, **more)
    for cols in ([cols_list] if isinstance(cols_list, dict) else cols_list):
        a.submit(cols)
    a.finalize()
    check_views(a, Gw, Tw, W)
    assert np.array_equal(module_words(a, n_lanes), Tw)
    a.close()
    return Gw, Tw


# ---------------------------------------------------------------------------------------------------------------------------
# 1. the genome kernel
# ---------------------------------------------------------------------------------------------------------------------------
def genome_set(W):
    """About 40 contigs: W - 1, W, W + 1 and 1 bases; one of three shares whose last is odd; all N, all G, all A; N runs of exactly
    four and exactly five; lengths of a few hundred, so that the contigs' windows begin at every alignment of their bytes; rid 20
    never given."""
    rng = np.random.default_rng(100 + W)

    def rnd(n):
        pn = min(0.02, 2.0 / W)  # (about two N a window at the most: most windows keep their bin)
        return rng.choice(5, n, p=[0.28 - pn, 0.22, 0.22, 0.28, pn]).astype(np.uint8)
    refs = [rnd(W - 1), rnd(W), rnd(W + 1), rnd(1), rnd(2 * gcb_steps.GG_SHARE + W - 1 + 4321),
            np.full(W + 200, N, np.uint8), np.full(W + 50, G, np.uint8), np.full(W + 50, A, np.uint8)]
    for run in (4, 5):
        r = rng.integers(0, 4, W + 300).astype(np.uint8)
        for at in (0, W // 2 + 7, W + 150, W + 300 - run):
            r[at:at + run] = N
        refs.append(r)
    while len(refs) < 40:
        refs.append(rnd(int(rng.integers(100, 700))))
    refs[20] = None
    return refs


@pytest.mark.parametrize("W", [100, 20, 21, 1000])
def test_genome_table(W):
    refs = genome_set(W)
    lens = [None if r is None else len(r) for r in refs]
    sh = gcb_steps.genome_shares(lens, W)
    assert [s for s in sh if s[0] == 4] == [(4, 0, 8192), (4, 8192, 8192), (4, 16384, 4321)] and len(sh) >= (30 if W < 1000 else 1)
    Gw, Tw = gcb_ref.table_fast([], refs, 2, W)
    assert Gw[100] >= 51 and Gw[0] >= 51 and Gw.sum() > 15_000  # (the long contig has 20 705 starts; a window loses its bin with five N)
    small = [r if r is not None and len(r) < 1200 and W <= 100 else None for r in refs]  # (the plain loop, where it is quick)
    assert np.array_equal(gcb_ref.genome(small, W), gcb_ref.table_fast([], small, 1, W)[0])
    a = context(refs, 2, W)
    a.finalize()
    check_views(a, Gw, Tw, W)
    a.reset()  # the genome table is the genome's: the same after a reset and the next finalize
    a.finalize()
    check_views(a, Gw, Tw, W)
    a.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 2. the read rule
# ---------------------------------------------------------------------------------------------------------------------------
def rule_case(W):
    """Contigs 0 (5000 bases: a run of five N at 1000, of four at 2000, single ones at 300 and 4500), 1 (never given), 2 (W + 40
    bases); every kind of read of the definition in three read groups."""
    rng = np.random.default_rng(200 + W)
    r0 = rng.integers(0, 4, 5000).astype(np.uint8)
    r0[1000:1005] = N
    r0[2000:2004] = N
    r0[[300, 4500]] = N
    refs = [r0, None, rng.integers(0, 4, W + 40).astype(np.uint8)]
    len0, len2 = len(r0), W + 40
    reads = []

    def add(**kw):
        kw.setdefault("lane", len(reads) % 3)
        kw.setdefault("flag", P | MAIN | (FIRST if len(reads) & 1 else LAST))
        reads.append(kw)
    # the contigs' ends, forward and reverse: s = -1, 0, len - W, len - W + 1
    for rid, ln in ((0, len0), (2, len2)):
        for s in (-1, 0, ln - W, ln - W + 1):
            add(pos=s, cigar=[(30, 0)], rid=rid)
            for span in (30, 150):  # reverse: s = pos + span - W
                add(pos=s + W - span, cigar=[(span, 0)], rid=rid, flag=P | MAIN | FIRST | REV)
    add(pos=2**31 - 50, cigar=[(150, 0)])
    add(pos=2**31 - 50, cigar=[(150, 0)], flag=P | MAIN | LAST | REV)
    add(pos=-3, cigar=[(150, 0)])
    add(pos=-3, cigar=[(W + 3, 0)], flag=P | MAIN | LAST | REV)     # s = 0
    add(pos=-3, cigar=[(W + 2, 0)], flag=P | MAIN | LAST | REV)     # s = -1
    # a reverse read of 600 operations, D and N among them
    ops = []
    for k in range(150):
        ops += [(2, 0), (1, 2), (3, 7), (1 + k % 3, 3)]
    add(pos=500, cigar=ops, flag=P | MAIN | FIRST | REV)
    add(pos=500, cigar=ops)
    add(pos=700, cigar=[(5, 4), (40, 0), (3, 1), (2, 2), (60, 8), (9, 3), (30, 0), (7, 5)], flag=P | MAIN | LAST | REV)
    # not examined; examined whatever else the flag says
    for f in (0x4, 0x100, 0x800, 0x104):
        add(pos=100, cigar=[(50, 0)], flag=P | MAIN | FIRST | f)
    add(pos=100, cigar=[], L=50)
    add(pos=100, cigar=[(50, 0)], rid=-1)
    add(pos=100, cigar=[(50, 0)], rid=1)
    for f in (0x400, 0x200, 0x600, 0x2 | 0x20, FIRST | LAST):
        add(pos=100, cigar=[(50, 0)], flag=P | MAIN | LAST | f)
    # lengths 1 .. 3000 in one batch, qualities over 0 .. 222, reads without qualities, the read groups interleaved
    for rep in range(40):
        for L in (1, 20, 150, 255, 256, 3000):
            rev = bool(rng.random() < 0.5)
            q = None if rng.random() < 0.15 else rng.integers(0, 223, L).astype(np.uint8)
            if q is not None and rep == 0:
                q[:] = np.arange(L) % 223
            add(pos=int(rng.integers(0, len0 - 3100)), cigar=[(L, 0)], qual=q, flag=P | MAIN | (FIRST if rng.random() < 0.5 else LAST) | (REV if rev else 0))
    for k in range(1500):  # windows at every byte alignment, around both N runs
        add(pos=int(rng.integers(900, 2200)), cigar=[(int(rng.integers(1, 300)), 0)], qual=int(rng.integers(0, 223)), flag=P | MAIN | FIRST | (REV if k & 2 else 0))
    for k in range(600):  # windows that hold the run of four and nothing else, whatever W
        add(pos=int(rng.integers(1005, 3400)), cigar=[(int(rng.integers(1, 200)), 0)], qual=int(rng.integers(0, 223)))
    return cols_of(reads), refs


@pytest.mark.parametrize("W", [100, 20, 21, 1000])
def test_read_rule(W):
    cols, refs = rule_case(W)
    Gp, Tp = gcb_ref.table(cols, refs, 3, W) if W == 100 else (None, None)
    Gw, Tw = run_and_check(cols, refs, 3, W)
    if W == 100:  # (the plain loops once)
        assert np.array_equal(Gp, Gw) and np.array_equal(Tp, Tw)
    assert all(Tw[l, r].sum() > 100 for l in range(3) for r in range(3)) and (Tw[:, 0] * 3000 >= Tw[:, 1]).all()


def test_steps_and_read_groups():
    """More than 1024 x (CU count) reads, so that every workgroup takes a second step; three read groups whose changes fall on a
    step's seam and inside a step (positions sorted: stream order is processing order)."""
    cu = n_cu()
    n = gcb_steps.GR_STEP * cu + 977
    while min(gcb_steps.reads_launch(n, cu)["steps"]) < 2:
        n += 1
    la = gcb_steps.reads_launch(n, cu)
    assert la["grid"] == cu and min(la["steps"]) >= 2
    rng = np.random.default_rng(31)
    ref = rng.choice(5, 300_000, p=[0.3, 0.2, 0.2, 0.29, 0.01]).astype(np.uint8)
    lane = np.zeros(n, np.uint8)
    lane[(cu // 3) * la["per"] + gcb_steps.GR_STEP:] += 1     # on a seam
    lane[(2 * cu // 3) * la["per"] + 333:] += 1               # inside a step
    L = rng.choice([36, 100, 151], n)
    flag = (P | MAIN | np.where(rng.random(n) < 0.5, REV, 0) | np.where(rng.random(n) < 0.5, FIRST, LAST)).astype(np.uint16)
    qual = rng.integers(0, 223, int(L.sum())).astype(np.uint8)
    cols = cols_flat(np.sort(rng.integers(0, len(ref) - 200, n)), flag, L, lane=lane, qual=qual)
    Gw, Tw = run_and_check(cols, [ref], 3, 100)
    assert all(Tw[l, 0].sum() > 10_000 for l in range(3))


# ---------------------------------------------------------------------------------------------------------------------------
# 3. contention: 70 000 reads into one bin of one read group
# ---------------------------------------------------------------------------------------------------------------------------
def test_70000_reads_one_bin():
    n = 70_000
    ref = np.concatenate([np.full(300, A, np.uint8), np.tile(np.array([C, A, G, T], np.uint8), 100)])  # windows at 300 + 4 k: bin 50
    cols = cols_flat(np.full(n, 304), np.full(n, P | MAIN | FIRST), np.full(n, 150), qual=222)
    a = context([ref], 2, 100)
    a.submit(cols)
    a.finalize()
    g, r, b, q = a.gc_bias(0)
    want = np.zeros(BINS, np.uint64)
    want[50] = 1
    assert np.array_equal(r, want * n) and np.array_equal(b, want * (150 * n)) and np.array_equal(q, want * (150 * 222 * n))
    assert not any(x.any() for x in a.gc_bias(1)[1:]) and np.array_equal(a.gc_bias(1)[0], g)
    assert g.sum() == len(ref) - 99 and g[0] == 201
    a.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 4. sums and life cycle
# ---------------------------------------------------------------------------------------------------------------------------
def test_sums_reset_export_import():
    cols, refs = rule_case(100)
    n = len(cols["flag"])
    Gw, Tw = gcb_ref.table_fast(cols, refs, 3, 100)
    parts = split(cols, [n // 2 + 3])
    run_and_check(parts, refs, 3, 100)  # two batches add
    vecs = []
    for part in parts:
        a = context(refs, 3, 100)
        a.submit(part)
        vecs.append(a.state_export_host())
        a.close()
    c = context(refs, 3, 100)
    c.state_import_host(vecs[0] + vecs[1])  # export + import into a fresh context adds
    assert np.array_equal(module_words(c, 3), Tw)
    c.finalize()
    check_views(c, Gw, Tw, 100)
    c.reset()
    with pytest.raises(BamQCError) as e:  # (nothing finalised since the reset)
        c.gc_bias(0)
    assert e.value.code == ERR_STATE
    assert not module_words(c, 3).any()
    c.finalize()
    check_views(c, Gw, 0 * Tw, 100)  # R, B and Q are zero, G is the genome's
    c.reset()
    d = c.upload(cols)
    c.process(d)
    c.process(d)
    c.finalize()
    check_views(c, Gw, 2 * Tw, 100)
    d.free()
    # a context with the module off has another bqc_state_words: the vector does not fit
    off = Aggregator(n_lanes=3, n_refs=3, max_read_len=4096, isize=2000)
    assert off.state_words == c.state_words - 3 * 3 * BINS
    with pytest.raises(AssertionError):
        off.state_import_host(vecs[0])
    off.finalize()
    with pytest.raises(BamQCError) as e:
        off.gc_bias(0)
    assert e.value.code == ERR_STATE
    with pytest.raises(BamQCError) as e:
        c.gc_bias(3)
    assert e.value.code == ERR_ARG
    off.close()
    c.close()


def test_enable_call_and_its_order():
    base = dict(n_lanes=2, n_refs=1, max_read_len=4096, isize=2000)
    ref = np.random.default_rng(41).integers(0, 4, 2000).astype(np.uint8)
    cols = cols_flat([5, 700], [P | MAIN | FIRST, P | MAIN | LAST | REV], [100, 100], lane=[0, 1])
    for w in (19, 1001, 0):
        with pytest.raises(BamQCError) as e:
            Aggregator(gc_bias=w, **base)
        assert e.value.code == ERR_ARG and str(w) in str(e.value)
    for w in (20, 1000):
        Aggregator(gc_bias=w, **base).close()
    plain = Aggregator(**base)
    on = Aggregator(gc_bias=100, **base)
    assert on.state_words == plain.state_words + 2 * 3 * BINS
    with pytest.raises(BamQCError) as e:  # twice
        on.enable_gc_bias(100)
    assert e.value.code == ERR_STATE
    on.close()

    def too_late(act):
        a = Aggregator(**base)
        a.set_reference(0, ref)
        words = a.state_words
        keep = act(a)
        with pytest.raises(BamQCError) as e:
            a.enable_gc_bias(100)
        assert e.value.code == ERR_STATE and a.state_words == words
        if hasattr(keep, "free"):
            keep.free()
        a.close()
    too_late(lambda a: a.submit(cols))
    too_late(lambda a: a.upload(cols))
    too_late(lambda a: a.state_export_host())
    too_late(lambda a: a.state_import_host(np.zeros(a.state_words, np.uint64)))
    too_late(lambda a: a.finalize())
    plain.set_reference(0, ref)  # setting references first is fine
    plain.enable_gc_bias(50)
    plain.submit(cols)
    plain.finalize()
    Gw, Tw = gcb_ref.table(cols, [ref], 2, 50)
    check_views(plain, Gw, Tw, 50)
    assert Tw[:, 0].sum() == 2
    plain.close()


def test_beside_the_other_modules():
    """With qual-, mismatch- and adapter-by-cycle on as well: their tables and the counts are those of a run without the GC bias, the
    module's words lie directly behind the sketch's, the `.qbc` words stay the vector's last."""
    rng = np.random.default_rng(51)
    n = 4000
    ref = rng.integers(0, 4, 50_000).astype(np.uint8)
    L = rng.choice([50, 150, 300], n)
    flag = (P | MAIN | np.where(rng.random(n) < 0.5, REV, 0) | np.where(rng.random(n) < 0.5, FIRST, LAST)).astype(np.uint16)
    cols = cols_flat(np.sort(rng.integers(0, len(ref) - 400, n)), flag, L, lane=rng.integers(0, 2, n), qual=rng.integers(0, 94, int(L.sum())).astype(np.uint8))
    base = dict(n_lanes=2, n_refs=1, max_read_len=4096, isize=2000, qual_by_cycle=64, mismatch_by_cycle=32, adapter_by_cycle=16, klist=[21], qlist=[17])
    three, four = Aggregator(**base), Aggregator(gc_bias=100, **base)
    bare = Aggregator(gc_bias=100, n_lanes=2, n_refs=1, max_read_len=4096, isize=2000)
    for a in (three, four, bare):
        a.set_reference(0, ref)
        a.submit(cols)
    v3, v4, vb = three.state_export_host(), four.state_export_host(), bare.state_export_host()
    nmod = 2 * 3 * BINS
    tail = 2 * 2 * 9 * 16 + 2 * 2 * 2 * 32 * 224 + 2 * 2 * 64 * 224  # adapter, mismatch, qual
    assert len(v4) == len(v3) + nmod
    head = len(v3) - tail
    assert np.array_equal(v4[:head], v3[:head]) and np.array_equal(v4[head + nmod:], v3[head:]) and v3[head:].any()
    Gw, Tw = gcb_ref.table_fast(cols, [ref], 2, 100)
    assert np.array_equal(v4[head:head + nmod].reshape(2, 3, BINS), Tw) and np.array_equal(vb[len(vb) - nmod:].reshape(2, 3, BINS), Tw)
    c3, c4 = three.finalize(), four.finalize()
    assert _abi.diff_counts(c3, c4) == [] and c3[0]["sketch"]
    for l in range(2):
        for m in range(2):
            assert np.array_equal(three.qual_by_cycle(l, m), four.qual_by_cycle(l, m))
            assert all(np.array_equal(x, y) for x, y in zip(three.mismatch_by_cycle(l, m), four.mismatch_by_cycle(l, m)))
            assert all(np.array_equal(x, y) for x, y in zip(three.adapter_by_cycle(l, m)[:2], four.adapter_by_cycle(l, m)[:2]))
    check_views(four, Gw, Tw, 100)
    for a in (three, four, bare):
        a.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 5. the program
# ---------------------------------------------------------------------------------------------------------------------------
CHROMS = ["-c", "chr1,chr2,chr3"]


def run(args, env=None, **kw):
    return subprocess.run([EXE] + args, capture_output=True, env=dict(os.environ, **(env or {})), timeout=120, **kw)


def fasta_codes(path):
    """The contigs of a FASTA file as Dna5 codes, by name (every letter outside ACGT is N)."""
    lut = np.full(256, 4, np.uint8)
    for k, ch in enumerate("ACGT"):
        lut[ord(ch)] = lut[ord(ch.lower())] = k
    out, name, parts = {}, None, []
    for line in open(path, "rb").read().split(b"\n") + [b">"]:
        if line.startswith(b">"):
            if name is not None:
                out[name] = lut[np.frombuffer(b"".join(parts), np.uint8)]
            name, parts = line[1:].split()[0].decode() if len(line) > 1 else None, []
        else:
            parts.append(line.strip())
    return out


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """About 20 000 synthetic paired reads in three read groups, the outputs of a run without the option, and the expected text."""
    d = tmp_path_factory.mktemp("gcb")
    bam, fa = str(d / "in.bam"), str(d / "in.fa")
    hostio.synth_write(bam, fa, seed=23, n_reads=20_000, ref_names=["chr1", "chr2", "chr3"], ref_lens=[300_000, 120_000, 9_000], n_lanes=3)
    base = str(d / "base.bamqc")
    mods = ["--qual-by-cycle", "--mismatch-by-cycle", "--adapter-by-cycle"]
    r = run(["-r", fa, "-o", base] + mods + CHROMS + [bam])
    assert r.returncode == 0, r.stderr
    assert not os.path.exists(base + ".gcb")
    cols, refs, lanes, sample = pybam.columns(bam)
    assert len(lanes) == 3
    names = sorted(lanes)  # the `.bamqc` lists the lanes by name
    idx = [lanes[nm] for nm in names]
    codes = fasta_codes(fa)
    genome = [codes.get(name) for name, length in refs]
    assert all(g is not None for g in genome)

    def want(W):
        Gw, Tw = gcb_ref.table_fast(cols, genome, 3, W)
        assert all(Tw[l, 0].sum() > 1000 for l in range(3))
        return gcb_ref.text(Gw, Tw, W, sample, names, idx)
    return dict(dir=d, bam=bam, fa=fa, base=base, want=want, mods=mods)


def same_bytes(a, b):
    return open(a, "rb").read() == open(b, "rb").read()


@pytest.mark.parametrize("decode", ["0", "1"])
def test_program_bam(files, decode):
    out = str(files["dir"] / ("bam%s.bamqc" % decode))
    r = run(["-r", files["fa"], "-o", out, "--gc-bias"] + CHROMS + [files["bam"]], env=dict(BQC_GPU_DECODE=decode))
    assert r.returncode == 0, r.stderr
    assert same_bytes(out, files["base"])
    assert open(out + ".gcb").read() == files["want"](100)
    assert not os.path.exists(out + ".qbc")


def test_program_window_and_all_four_modules(files):
    out = str(files["dir"] / "four.bamqc")
    r = run(["-r", files["fa"], "-o", out, "--gc-bias-window", "50"] + files["mods"] + CHROMS + [files["bam"]])
    assert r.returncode == 0, r.stderr
    for ext in ("", ".qbc", ".mbc", ".adp"):
        assert same_bytes(out + ext, files["base"] + ext), ext
    assert open(out + ".gcb").read() == files["want"](50)


def test_program_sam_on_stdin(files):
    out = str(files["dir"] / "sam.bamqc")
    sam = pybam.bam_to_sam_text(files["bam"]).encode()
    r = run(["-r", files["fa"], "-o", out, "--gc-bias"] + CHROMS + ["-"], input=sam)
    assert r.returncode == 0, r.stderr
    assert same_bytes(out, files["base"])
    assert open(out + ".gcb").read() == files["want"](100)


def test_program_manifest(files):
    """Two jobs through one resident worker: each gets the `.gcb` of its single run (the genome table is made again per job)."""
    d = files["dir"]
    outs = [str(d / "m1.bamqc"), str(d / "m2.bamqc")]
    lst = str(d / "jobs.tsv")
    with open(lst, "w") as f:
        for o in outs:
            f.write("%s\t%s\n" % (files["bam"], o))
    r = run(["-r", files["fa"], "--gc-bias-window", "50", "--manifest", lst] + CHROMS)
    assert r.returncode == 0, r.stderr
    for o in outs:
        assert same_bytes(o, files["base"])
        assert open(o + ".gcb").read() == files["want"](50)


def test_program_refuses_gpus_and_bad_windows(files):
    out = str(files["dir"] / "no.bamqc")
    r = run(["--gpus", "2", "-r", files["fa"], "-o", out, "--gc-bias"] + CHROMS + [files["bam"]], env=dict(BQC_GPUS_SHARE_DEVICE="1"))
    assert r.returncode == 1 and b"--gc-bias with --gpus is not supported" in r.stderr
    r = run(["-r", files["fa"], "-o", out, "--gc-bias-window", "19"] + CHROMS + [files["bam"]])
    assert r.returncode == 1 and b"--gc-bias-window wants 20 to 1000" in r.stderr
    assert not os.path.exists(out) and not os.path.exists(out + ".gcb")
