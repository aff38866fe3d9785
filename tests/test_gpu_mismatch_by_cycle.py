"""GPU: mismatches by cycle and base quality (bqc_options.mismatch_by_cycle, --mismatch-by-cycle; bamqc_amd/csrc/k_mbc.hip)
against the numpy restatement of the statistic (tests/mbc_ref.py).

The kernel turns every match-like CIGAR operation into a run of stored positions, keeps at most 768 runs in LDS at a time, gives
lane j of a wave the stored bases 4j .. 4j+3 of a run (256 positions a pass), loads qualities, nibbles and genome bytes as aligned
dwords wherever they start, counts A in an LDS tile of [2 mates][64 qualities][256 cycles] that belongs to one read group at a time,
and sends M and everything the tile does not hold to device memory.  The shapes below cross each of those edges and the capacity N."""
import os
import subprocess

import numpy as np
import pytest

from bamqc_amd import Aggregator, BamQCError, _abi, hostio
from tests import bamqc_text, mbc_ref, pybam, qbc_ref, synth
from tests.long_layout import dna_ref, reads_on_ref, records
from tests.parity import split

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "bin", "bamqualcheck")
QUALS = np.array([0, 2, 37, 63, 64, 93, 222], np.uint8)
LENGTHS = [1, 3, 4, 5, 15, 16, 17, 63, 64, 65, 150, 255, 256, 257, 300, 1023, 1024, 1025, 2000]
P, PR, REV, FIRST, LAST, MAIN = 0x1, 0x2, 0x10, 0x40, 0x80, 0x1000
ERR_ARG, ERR_STATE = 1, 8
OPTS = dict(n_refs=1, max_read_len=4096, isize=2000)
NEXT_BASE = {1: 2, 2: 4, 4: 8, 8: 1}  # a nibble that is another base


def draw_quals(rng, n):
    return QUALS[rng.integers(0, len(QUALS), n)]


def seq_offsets(cols):
    L = cols["l_seq"].astype(np.int64)
    return np.cumsum((L + 1) // 2) - (L + 1) // 2


def get_nib(cols, so, i, j):
    byte = int(cols["seq"][so[i] + j // 2])
    return byte & 15 if j & 1 else byte >> 4


def set_nib(cols, so, i, j, nib):
    k = so[i] + j // 2
    byte = int(cols["seq"][k])
    cols["seq"][k] = (byte & 0xF0) | nib if j & 1 else (byte & 0x0F) | (nib << 4)


def plant(cols, rng, frac=0.03, ends=True):
    """Mismatches by rewriting nibbles of cols["seq"]: the first and the last stored base of every read (ends), and a random `frac`
    of the others.  Only bases A, C, G, T are rewritten, into another of them."""
    so = seq_offsets(cols)
    for i, L in enumerate(cols["l_seq"].astype(np.int64)):
        where = set(np.flatnonzero(rng.random(L) < frac).tolist())
        if ends and L:
            where |= {0, int(L) - 1}
        for j in where:
            nib = get_nib(cols, so, i, j)
            if nib in NEXT_BASE:
                set_nib(cols, so, i, j, NEXT_BASE[nib])
    return cols


def context(refs, n_lanes, N, **more):
    """refs: the contig (one array), or a list by rid with None for a contig that is never set."""
    refs = refs if isinstance(refs, list) else [refs]
    a = Aggregator(n_lanes=n_lanes, mismatch_by_cycle=N, **dict(OPTS, n_refs=len(refs), **more))
    for rid, r in enumerate(refs):
        if r is not None:
            a.set_reference(rid, r)
    return a


def check_tables(a, counts, T):
    """Every lane's and mate's view against the restatement T (sizes and contents of both tables)."""
    for l in range(T.shape[0]):
        for m in range(2):
            nc, nq = mbc_ref.sizes(T[l, m], counts[l]["r%d.n_cycles" % (m + 1)])
            A, M = a.mismatch_by_cycle(l, m)
            assert A.shape == (nc, nq) and M.shape == (nc, nq), (l, m, A.shape, M.shape, (nc, nq))
            assert not T[l, m, :, nc:].any(), (l, m)  # (nothing is counted behind the mate's longest read)
            for name, got, want in (("A", A, T[l, m, 0]), ("M", M, T[l, m, 1])):
                bad = np.argwhere(got != want[:nc, :nq])
                assert not len(bad), "lane %d mate %d table %s: %d bins differ, first (cycle, q) = %s: %d != %d" % (
                    l, m, name, len(bad), bad[0].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])


def module_words(a, n_lanes, N, behind=0):
    """The module's words of the flat state vector: n_lanes x 2 x 2 x N x 224, with `behind` words (qual_by_cycle's) behind them."""
    v = a.state_export_host()
    n = n_lanes * 2 * 2 * N * 224
    return v[len(v) - behind - n:len(v) - behind].reshape(n_lanes, 2, 2, N, 224)


# ---------------------------------------------------------------------------------------------------------------------------
# 1. parity with the restatement
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sweep():
    clean = dna_ref(5, 8000)
    rng = np.random.default_rng(6)
    L, flag = [], []
    for n in LENGTHS:
        for rev in (0, REV):
            for mate in (FIRST, LAST):
                L.append(n)
                flag.append(P | PR | MAIN | rev | mate)
    order = rng.permutation(len(L))  # (the lengths and kinds mixed, not in ascending order)
    L, flag = np.array(L)[order], np.array(flag)[order]
    pos = 1 + 3 * np.arange(len(L))  # every read at another position: the genome's bytes start at every alignment mod 4
    assert {int(p) & 3 for p in pos} == {0, 1, 2, 3} and {int(p + l) & 3 for p, l in zip(pos, L)} == {0, 1, 2, 3}
    cols = plant(reads_on_ref(clean, pos, L, flag, draw_quals(rng, int(L.sum()))), rng)
    so = seq_offsets(cols)
    for i in rng.choice(len(L), 12, replace=False):  # a few read bases that are N, = and M (an ambiguity code)
        j = int(rng.integers(0, L[i]))
        set_nib(cols, so, int(i), j, (15, 0, 3)[int(i) % 3])
    ref = clean.copy()
    ref[rng.choice(2300, 40, replace=False)] = 4  # a few genome bases are N (under reads that hold a base there)
    assert {int(q) for q in cols["qual"]} >= {int(q) for q in QUALS}
    return cols, ref


@pytest.mark.parametrize("N", [1024, 16, 300])
def test_parity(sweep, N):
    cols, ref = sweep
    a = context(ref, 1, N)
    a.submit(cols)
    counts = a.finalize()
    T = mbc_ref.table(cols, [ref], 1, N)
    assert all(T[0, m, t].any() for m in range(2) for t in range(2))  # A and M, both mates
    check_tables(a, counts, T)
    assert np.array_equal(module_words(a, 1, N), T)  # the whole block, the cycles no view shows included
    a.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 2. CIGAR shapes
# ---------------------------------------------------------------------------------------------------------------------------
def on_ref(ref, pos, ops, rng, L=None):
    """Codes (0..3) of a read that lies on the reference at `pos` with this CIGAR: M, = copy, X takes another base, I and S draw,
    D and N skip, H and P do nothing; positions outside the contig draw.  L: cut (or fill up) to that many bases."""
    out, rp = [], pos
    for n, op in ops:
        if op in "M=X":
            idx = rp + np.arange(n)
            base = np.where((idx >= 0) & (idx < len(ref)), ref[np.clip(idx, 0, len(ref) - 1)], rng.integers(0, 4, n)).astype(np.uint8)
            out.append((base + 1) % 4 if op == "X" else base)
            rp += n
        elif op in "IS":
            out.append(rng.integers(0, 4, n).astype(np.uint8))
        elif op in "DN":
            rp += n
    codes = np.concatenate(out) if out else np.zeros(0, np.uint8)
    if L is not None:
        codes = np.concatenate([codes, rng.integers(0, 4, max(0, L - len(codes))).astype(np.uint8)])[:L]
    return codes


@pytest.fixture(scope="module")
def shapes():
    """One read per CIGAR shape and per rule of "a read is counted", and 300 reads of 9 operations, in one batch of two contigs of
    which only the first is ever set."""
    ref = dna_ref(31, 30_000)
    rng = np.random.default_rng(32)
    ok = P | PR | MAIN | FIRST     # a counted read
    lone = P | LAST | REV          # counted as well, and never eligible for the triplet counters (no proper pair)
    alt = [(90, "M") if k % 2 == 0 else ((11, "I") if k % 4 == 1 else (7, "D")) for k in range(41)]  # 21 M, 10 I, 10 D: 2000 bases
    assert sum(n for n, op in alt if op in "MI") == 2000
    nine = [(20, "M"), (3, "I"), (20, "M"), (2, "D"), (20, "M"), (3, "I"), (20, "M"), (2, "D"), (20, "M")]
    cases = [  # (ops, pos, flag, L or None, rid)
        ([(150, "M")], 101, ok, None, 0),
        ([(5, "S"), (140, "M"), (5, "S")], 202, ok, None, 0),
        ([(5, "H"), (5, "S"), (140, "M")], 303, ok | REV, None, 0),
        ([(50, "M"), (2, "I"), (98, "M")], 404, ok, None, 0),
        ([(50, "M"), (3, "D"), (100, "M")], 505, ok | REV, None, 0),
        ([(50, "M"), (1000, "N"), (100, "M")], 606, ok, None, 0),
        ([(10, "="), (1, "X"), (139, "=")], 707, ok, None, 0),
        ([(50, "M"), (2, "P"), (100, "M")], 808, ok | REV, None, 0),
        (alt, 1001, ok, None, 0),
        ([(150, "M")], len(ref) - 100, lone, None, 0),           # hangs over the contig's end
        ([(150, "M")], -3, lone, None, 0),                       # begins in front of it
        ([(100, "M")], 1500, lone, 60, 0),                       # the CIGAR consumes more than l_seq
        ([], 1600, lone, 80, 0),                                 # n_cigar = 0 on a mapped read
        ([(150, "M")], 1700, lone | 0x4, None, 0),               # unmapped with a position
        ([(150, "M")], 1800, lone, None, -1),                    # rid = -1
        ([(150, "M")], 1900, lone, None, 1),                     # a contig that was never set
        ([(150, "M")], 2000, ok | 0x100, None, 0),               # secondary
        ([(150, "M")], 2100, ok | 0x800, None, 0),               # supplementary
        ([(150, "M")], 2200, (ok & ~FIRST) | 0x100, None, 0),    # no mate flag (on a secondary record: a primary one ends the run)
        ([(150, "M")], 2300, ok | LAST, None, 0),                # both mate flags: first
        ([(150, "M")], 2400, ok | 0x8000, None, 0),              # no qualities
        ([(150, "M")], 2500, ok | 0x400, None, 0),               # a duplicate counts
        ([(150, "M")], 2600, ok | 0x200, None, 0),               # so does a QC fail
    ]
    cases += [(nine, 3000 + 37 * k, (P | PR | MAIN | (FIRST if k & 1 else LAST) | (REV if k & 2 else 0)), None, 0) for k in range(300)]
    recs = []
    for ops, pos, flag, L, rid in cases:
        codes = on_ref(ref, pos, ops, rng, L)
        qual = np.full(len(codes), 0xFF, np.uint8) if flag & 0x8000 else draw_quals(rng, len(codes))
        recs.append(dict(codes=codes.astype(np.int64), qual=qual, flag=flag, pos=pos, ops=ops, nm=sum(n for n, op in ops if op in "ID")))
    cols = records(recs)
    cols["rid"] = np.array([c[4] for c in cases], np.int32)
    cols["mapq"][:] = 30  # (no read is eligible for the triplet counters: what is looked at here is this module's own walk)
    so = seq_offsets(cols)
    set_nib(cols, so, 6, 3, NEXT_BASE[get_nib(cols, so, 6, 3)])  # a mismatch inside an `=` operation: compared, not believed
    plant(cols, rng)
    return cols, [ref, None], len(cases) - 300


def test_cigar_shapes(shapes):
    cols, refs, n_single = shapes
    T = mbc_ref.table(cols, refs, 1, 1024)
    one = lambda k: mbc_ref.table(synth.slice_batch(cols, k, k + 1), refs, 1, 1024)
    assert one(6)[0, 0, 1, 10].sum() == 1 and one(6)[0, 0, 1, 3].sum() == 1        # the X, and the planted base inside `=`
    assert one(0)[0, 0, 0].sum() == 150 and one(1)[0, 0, 0].sum() == 140 and one(5)[0, 0, 0].sum() == 150
    assert one(9)[0, 1, 0].sum() == 100 and one(10)[0, 1, 0].sum() == 147 and one(11)[0, 1, 0].sum() == 60
    assert not any(one(k).any() for k in (12, 13, 14, 15, 16, 17, 18, 20))
    assert one(19)[0, 0, 0].sum() == 150 and one(21)[0, 0, 0].sum() == 150 and one(22)[0, 0, 0].sum() == 150
    a = context(refs, 1, 1024)
    a.submit(cols)
    check_tables(a, a.finalize(), T)
    assert np.array_equal(module_words(a, 1, 1024), T)
    a.close()
    # read by read as well: what a read adds does not depend on its neighbours in the list of runs
    b = context(refs, 1, 1024)
    for part in split(cols, list(range(1, n_single + 1))):
        b.submit(part)
    b.finalize()
    assert np.array_equal(module_words(b, 1, 1024), T)
    b.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 3. identities with the per-cycle base quality histograms
# ---------------------------------------------------------------------------------------------------------------------------
def test_identities_with_qual_by_cycle(sweep):
    cols, ref = sweep
    N, NQ = 300, 1024
    a = context(ref, 1, N, qual_by_cycle=NQ)
    a.submit(cols)
    counts = a.finalize()
    H = qbc_ref.table(cols, 1, NQ)
    v = a.state_export_host()
    nq_words = 2 * NQ * 224
    assert np.array_equal(v[len(v) - nq_words:].reshape(1, 2, NQ, 224), H)  # qual_by_cycle's words are still the last
    T = mbc_ref.table(cols, [ref], 1, N)
    assert np.array_equal(module_words(a, 1, N, behind=nq_words), T)
    for m in range(2):
        got = a.qual_by_cycle(0, m)
        nc, nq = qbc_ref.sizes(H[0, m], counts[0]["r%d.n_cycles" % (m + 1)])
        assert np.array_equal(got, H[0, m, :nc, :nq])
        A, M = a.mismatch_by_cycle(0, m)
        assert (M <= A).all() and M.any()
        assert (A <= got[:A.shape[0], :A.shape[1]]).all()
        assert (A < got[:A.shape[0], :A.shape[1]]).any()  # (the read and genome N of the sweep)
    a.close()
    # all-M reads of A, C, G, T on the loaded contig: every base is compared
    clean = dna_ref(41, 6000)
    rng = np.random.default_rng(42)
    L = rng.choice([16, 150, 255, 256, 300], 200)
    flag = (P | PR | MAIN | np.where(rng.random(200) < 0.5, REV, 0) | np.where(rng.random(200) < 0.5, FIRST, LAST)).astype(np.uint16)
    cols2 = plant(reads_on_ref(clean, np.sort(rng.integers(0, 5600, 200)), L, flag, draw_quals(rng, int(L.sum()))), rng)
    b = context(clean, 1, NQ, qual_by_cycle=NQ)
    b.submit(cols2)
    b.finalize()
    for m in range(2):
        A, M = b.mismatch_by_cycle(0, m)
        assert np.array_equal(A, b.qual_by_cycle(0, m)) and A.any() and M.any()
    b.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 4. one bin: 70 000 increments of one cell of each table inside a launch
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [1, 16])
def test_70000_mismatches_in_one_bin(L):
    n = 70_000
    ref = dna_ref(9, 1000)
    flag = P | PR | MAIN | FIRST | 0x400  # (duplicates: identical reads, and out of the coverage windows' way)
    cols = reads_on_ref(3 - ref, np.full(n, 500), np.full(n, L), np.full(n, flag, np.uint16), np.full(n * L, 37, np.uint8))  # the complement: every base differs
    a = context(ref, 1, 1024)
    a.submit(cols)
    a.finalize()
    A, M = a.mismatch_by_cycle(0, 0)
    assert A.shape == (L, 38) and M.shape == (L, 38)
    for tbl in (A, M):
        assert np.array_equal(tbl[:, 37], np.full(L, n, np.uint64)) and not tbl[:, :37].any()
    assert a.mismatch_by_cycle(0, 1)[0].shape == (0, 0)
    a.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 5. several read groups
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def groups():
    """Three read groups: alternating read by read, then in runs of 1, 2 and 700 reads."""
    ref = dna_ref(7, 20_000)
    rng = np.random.default_rng(8)
    lane = [i % 3 for i in range(60)]
    for g, run in ((0, 1), (1, 2), (2, 700), (0, 2), (1, 700), (2, 1), (0, 700), (1, 1)):
        lane += [g] * run
    n = len(lane)
    L = rng.choice([16, 40, 150, 255, 256, 300], n)
    flag = (P | PR | MAIN | np.where(rng.random(n) < 0.5, REV, 0) | np.where(rng.random(n) < 0.5, FIRST, LAST)).astype(np.uint16)
    cols = reads_on_ref(ref, np.sort(rng.integers(0, 19_000, n)), L, flag, draw_quals(rng, int(L.sum())), lane=lane)
    return plant(cols, rng), ref, mbc_ref.table(cols, [ref], 3, 300)


def test_read_groups(groups):
    cols, ref, T = groups
    assert all(T[l, m, t].any() for l in range(3) for m in range(2) for t in range(2))
    a = context(ref, 3, 300)
    a.submit(cols)
    check_tables(a, a.finalize(), T)
    assert np.array_equal(module_words(a, 3, 300), T)
    a.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 6. pure sums, and off means off
# ---------------------------------------------------------------------------------------------------------------------------
def test_sums_reset_and_pieces(groups):
    cols, ref, T = groups
    n = len(cols["flag"])
    vecs = []
    for part in split(cols, [n // 2 + 3]):
        a = context(ref, 3, 300)
        a.submit(part)
        vecs.append(a.state_export_host())
        a.close()
    c = context(ref, 3, 300)
    c.state_import_host(vecs[0] + vecs[1])
    assert np.array_equal(module_words(c, 3, 300), T)
    check_tables(c, c.finalize(), T)
    c.reset()
    with pytest.raises(BamQCError) as e:  # (nothing finalised since the reset)
        c.mismatch_by_cycle(0, 0)
    assert e.value.code == ERR_STATE
    assert not module_words(c, 3, 300).any()
    c.finalize()
    assert c.mismatch_by_cycle(0, 0)[0].shape == (0, 0)
    c.reset()
    for part in split(cols, [7, 1300]):  # a batch in pieces equals the batch whole
        c.submit(part)
    check_tables(c, c.finalize(), T)
    assert np.array_equal(module_words(c, 3, 300), T)
    c.reset()
    d = c.upload(cols)  # a resident batch, processed twice
    c.process(d)
    c.process(d)
    c.finalize()
    assert np.array_equal(module_words(c, 3, 300), 2 * T)
    d.free()
    c.close()


@pytest.mark.parametrize("sketch", [{}, dict(klist=[5], qlist=[17])])
def test_off_means_off(groups, sketch):
    cols, ref, T = groups
    import ctypes
    parent_size = _abi.Options.mismatch_by_cycle.offset  # the structure as it was before the field
    assert parent_size == ctypes.sizeof(_abi.Options) - 8
    old = Aggregator(n_lanes=3, struct_size=parent_size, mismatch_by_cycle=16, **dict(OPTS, **sketch))  # (the field lies behind what the library reads)
    off = context(ref, 3, 0, **sketch)
    on = context(ref, 3, 16, **sketch)
    assert off.state_words == old.state_words
    assert on.state_words == off.state_words + 3 * 2 * 2 * 16 * 224
    old.close()
    off.submit(cols)
    on.submit(cols)
    v_off, v_on = off.state_export_host(), on.state_export_host()
    if not sketch:  # (the sketch's saturating counters are not plain words of the state; the rest is)
        assert np.array_equal(v_on[:len(v_off)], v_off)
    assert np.array_equal(v_on[len(v_off):].reshape(3, 2, 2, 16, 224), T[:, :, :, :16])
    off.finalize()
    with pytest.raises(BamQCError) as e:
        off.mismatch_by_cycle(0, 0)
    assert e.value.code == ERR_STATE
    on.finalize()
    for lane, mate in ((3, 0), (0, 2)):
        with pytest.raises(BamQCError) as e:
            on.mismatch_by_cycle(lane, mate)
        assert e.value.code == ERR_ARG
    off.close()
    on.close()
    with pytest.raises(BamQCError) as e:  # a capacity behind max_read_len is refused
        Aggregator(n_lanes=1, mismatch_by_cycle=4097, **OPTS)
    assert e.value.code == ERR_ARG


# ---------------------------------------------------------------------------------------------------------------------------
# 7. the program
# ---------------------------------------------------------------------------------------------------------------------------
CHROMS = ["-c", "chr1,chr2"]


def run(args, env=None, **kw):
    return subprocess.run([EXE] + args, capture_output=True, env=dict(os.environ, **(env or {})), timeout=120, **kw)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """4000 synthetic paired reads in two read groups (the generator plants substitutions, indels and clips), the same as SAM text,
    the `.bamqc` of a run without the option, and the expected texts."""
    d = tmp_path_factory.mktemp("mbc")
    bam, fa, sam = str(d / "in.bam"), str(d / "in.fa"), str(d / "in.sam")
    hostio.synth_write(bam, fa, seed=23, n_reads=4000, ref_names=["chr1", "chr2"], ref_lens=[400_000, 150_000], n_lanes=2)
    with open(sam, "w") as f:
        f.write(pybam.bam_to_sam_text(bam))
    base = str(d / "base.bamqc")
    r = run(["-r", fa, "-o", base] + CHROMS + [bam])
    assert r.returncode == 0, r.stderr
    assert not os.path.exists(base + ".mbc") and not os.path.exists(base + ".qbc")
    cols, refs, lanes, sample = pybam.columns(bam)
    assert len(lanes) == 2
    genome = dict(hostio.load_fasta(fa))
    contigs = [genome[name] for name, _ in refs]
    parsed = bamqc_text.parse(base)
    names = sorted(lanes)  # the `.bamqc` lists the lanes by name
    idx = [lanes[nm] for nm in names]
    cycles = np.zeros((2, 2), np.int64)
    for nm in names:
        cycles[lanes[nm]] = [len(parsed[nm]["As_by_position_first"]), len(parsed[nm]["As_by_position_second"])]
    T = mbc_ref.table(cols, contigs, 2, 1024)
    assert all(T[l, m, t].any() for l in range(2) for m in range(2) for t in range(2))

    def want(N):
        return mbc_ref.text(T[:, :, :, :N], cycles, sample, names, idx)
    return dict(dir=d, bam=bam, sam=sam, fa=fa, base=base, want=want)


def same_bytes(a, b):
    return open(a, "rb").read() == open(b, "rb").read()


@pytest.mark.parametrize("decode", ["0", "1"])
@pytest.mark.parametrize("kind", ["bam", "sam"])
def test_program(files, kind, decode):
    out = str(files["dir"] / ("%s%s.bamqc" % (kind, decode)))
    r = run(["-r", files["fa"], "-o", out, "--mismatch-by-cycle"] + CHROMS + [files[kind]], env=dict(BQC_GPU_DECODE=decode))
    assert r.returncode == 0, r.stderr
    assert same_bytes(out, files["base"])
    assert open(out + ".mbc").read() == files["want"](1024)
    assert not os.path.exists(out + ".qbc")


def test_program_two_workers_on_one_card(files):
    out = str(files["dir"] / "gpus2.bamqc")
    r = run(["--gpus", "2", "-r", files["fa"], "-o", out, "--mismatch-by-cycle-len", "100", "--qual-by-cycle"] + CHROMS + [files["bam"]],
            env=dict(BQC_GPUS_SHARE_DEVICE="1"))
    assert r.returncode == 0, r.stderr
    assert same_bytes(out, files["base"])
    assert open(out + ".mbc").read() == files["want"](100)
    assert os.path.exists(out + ".qbc")  # both options together


def test_program_manifest(files):
    d = files["dir"]
    outs = [str(d / "m1.bamqc"), str(d / "m2.bamqc")]
    lst = str(d / "jobs.tsv")
    with open(lst, "w") as f:
        for o in outs:
            f.write("%s\t%s\n" % (files["bam"], o))
    r = run(["-r", files["fa"], "--mismatch-by-cycle-len", "300", "--manifest", lst] + CHROMS)
    assert r.returncode == 0, r.stderr
    for o in outs:
        assert same_bytes(o, files["base"])
        assert open(o + ".mbc").read() == files["want"](300)


def test_program_reports_a_table_it_cannot_write(files):
    d = files["dir"]
    out = str(d / "blocked.bamqc")
    os.mkdir(out + ".mbc")  # (a directory where the tables' file would go)
    r = run(["-r", files["fa"], "-o", out, "--mismatch-by-cycle"] + CHROMS + [files["bam"]])
    assert r.returncode == 1
    assert b"Could not write output file" in r.stderr and b".mbc" in r.stderr


# ---------------------------------------------------------------------------------------------------------------------------
# 8. the Python writers
# ---------------------------------------------------------------------------------------------------------------------------
def test_python_writers(groups, tmp_path):
    cols, ref, T = groups
    a = context(ref, 3, 300, qual_by_cycle=300)
    a.submit(cols)
    counts = a.finalize()
    cycles = np.array([[counts[l]["r1.n_cycles"], counts[l]["r2.n_cycles"]] for l in range(3)])
    names, idx = ["zeta", "alpha", "mid"], [2, 0, 1]  # (an order of its own: lane `idx[k]` is printed as `names[k]`)
    mbc, qbc = str(tmp_path / "x.mbc"), str(tmp_path / "x.qbc")
    a.write_mismatch_by_cycle(mbc, sample_id="S1", lane_names=names, lane_index=idx)
    a.write_qual_by_cycle(qbc, sample_id="S1", lane_names=names, lane_index=idx)
    a.close()
    assert open(mbc).read() == mbc_ref.text(T, cycles, "S1", names, idx)
    assert open(qbc).read() == qbc_ref.text(qbc_ref.table(cols, 3, 300), cycles, "S1", names, idx)
