"""GPU: per-cycle base quality histograms (bqc_options.qual_by_cycle, --qual-by-cycle; bamqc_amd/csrc/k_qcyc.hip) against the
numpy restatement of the statistic (tests/qbc_ref.py), and the identity that ties the table to a number the oracle pins:
for every lane, mate and cycle  sum_q q * H[lane][mate][cycle][q] == qualcount[cycle].

The kernel keeps [2 mates][64 qualities][256 cycles] in LDS and sends everything else to device memory with atomics; a
workgroup's tile belongs to one read group at a time.  The shapes below cross each of those edges, the k_short / generic
boundary (255 / 256 bases) and the capacity N."""
import os
import subprocess

import numpy as np
import pytest

from bamqc_amd import Aggregator, BamQCError, hostio
from tests import bamqc_text, pybam, qbc_ref, synth
from tests.long_layout import dna_ref, reads_on_ref
from tests.parity import split

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "bin", "bamqualcheck")
QUALS = np.array([0, 2, 37, 63, 64, 93, 94, 222], np.uint8)  # both sides of the tile's quality edge (64), and the ends of the range
LENGTHS = [1, 15, 16, 17, 63, 64, 65, 150, 255, 256, 257, 300, 1023, 1024, 1025, 2000]
P, PR, REV, FIRST, LAST, MAIN = 0x1, 0x2, 0x10, 0x40, 0x80, 0x1000
ERR_ARG, ERR_STATE = 1, 8
OPTS = dict(n_refs=1, max_read_len=4096, isize=2000)


def draw_quals(rng, n):
    return QUALS[rng.integers(0, len(QUALS), n)]


def context(ref, n_lanes, N, **more):
    a = Aggregator(n_lanes=n_lanes, qual_by_cycle=N, **dict(OPTS, **more))
    a.set_reference(0, ref)
    return a


def check_tables(a, counts, H):
    """Every lane's and mate's view against the restatement H (sizes and contents), and the identity with qualcount."""
    for l in range(H.shape[0]):
        for m in range(2):
            nc, nq = qbc_ref.sizes(H[l, m], counts[l]["r%d.n_cycles" % (m + 1)])
            got = a.qual_by_cycle(l, m)
            assert got.shape == (nc, nq), (l, m, got.shape, (nc, nq))
            assert not H[l, m, nc:].any(), (l, m)  # (nothing is counted behind the mate's longest read)
            bad = np.argwhere(got != H[l, m, :nc, :nq])
            assert not len(bad), "lane %d mate %d: %d bins differ, first (cycle, q) = %s: %d != %d" % (
                l, m, len(bad), bad[0].tolist(), got[tuple(bad[0])], H[l, m][tuple(bad[0])])
            qsum = (got.astype(np.uint64) * np.arange(nq, dtype=np.uint64)).sum(axis=1)
            assert np.array_equal(qsum, counts[l]["r%d.qualcount" % (m + 1)][:nc]), (l, m)


def module_words(a, n_lanes, N):
    """The module's words of the flat state vector: the last n_lanes x 2 x N x 224."""
    v = a.state_export_host()
    return v[len(v) - n_lanes * 2 * N * 224:].reshape(n_lanes, 2, N, 224)


# ---------------------------------------------------------------------------------------------------------------------------
# 1. parity with the restatement, and the identity
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sweep():
    ref = dna_ref(5, 8000)
    rng = np.random.default_rng(6)
    L, flag = [], []
    for n in LENGTHS:
        for rev in (0, REV):
            for mate in (FIRST, LAST):
                L.append(n)
                flag.append(P | PR | MAIN | rev | mate)
    # one each: both mate flags (counts as first), secondary, supplementary, duplicate, and a read without qualities
    special = [(150, P | PR | MAIN | FIRST | LAST), (150, P | PR | MAIN | FIRST | 0x100), (150, P | PR | MAIN | LAST | 0x800 | REV),
               (150, P | PR | MAIN | LAST | 0x400 | REV), (150, P | PR | MAIN | FIRST | 0x8000)]
    L += [s[0] for s in special]
    flag += [s[1] for s in special]
    order = rng.permutation(len(L))  # (the lengths and kinds mixed, not in ascending order)
    L, flag = np.array(L)[order], np.array(flag)[order]
    qual = draw_quals(rng, int(L.sum()))
    off = np.cumsum(L) - L
    i_noq = int(np.flatnonzero(flag & 0x8000)[0])
    qual[off[i_noq]:off[i_noq] + L[i_noq]] = 0xFF
    cols = reads_on_ref(ref, np.arange(len(L)) * 3, L, flag, qual)
    empty = synth.single_read("", [], [], P | 0x4 | FIRST, pos=3 * len(L))  # a read of length 0
    cols = synth.concat([cols, empty])
    assert {int(q) for q in cols["qual"]} >= {int(q) for q in QUALS}
    return cols, ref


@pytest.mark.parametrize("N", [1024, 16, 300])
def test_parity_and_identity(sweep, N):
    cols, ref = sweep
    a = context(ref, 1, N)
    a.submit(cols)
    counts = a.finalize()
    H = qbc_ref.table(cols, 1, N)
    assert H[0, 0].any() and H[0, 1].any()
    check_tables(a, counts, H)
    assert np.array_equal(module_words(a, 1, N), H)  # the whole block, the cycles no view shows included
    a.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 2. several read groups
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
    return cols, ref


def test_read_groups_one_batch_and_three(groups):
    cols, ref = groups
    H = qbc_ref.table(cols, 3, 1024)
    assert all(H[l, m].any() for l in range(3) for m in range(2))
    a = context(ref, 3, 1024)
    a.submit(cols)
    check_tables(a, a.finalize(), H)
    whole = module_words(a, 3, 1024)
    a.close()
    b = context(ref, 3, 1024)
    for part in split(cols, [7, 1300]):
        b.submit(part)
    check_tables(b, b.finalize(), H)
    assert np.array_equal(module_words(b, 3, 1024), whole)
    b.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 3. counter width: more than 2^16 increments of one bin inside a launch
# ---------------------------------------------------------------------------------------------------------------------------
def test_70000_increments_of_one_bin():
    n, L = 70_000, 20
    ref = dna_ref(9, 100_000)
    pos = np.sort(np.random.default_rng(10).integers(0, 99_000, n))
    cols = reads_on_ref(ref, pos, np.full(n, L), np.full(n, P | PR | MAIN | FIRST, np.uint16), np.full(n * L, 37, np.uint8))
    a = context(ref, 1, 1024)
    a.submit(cols)
    a.finalize()
    got = a.qual_by_cycle(0, 0)
    assert got.shape == (L, 38)
    assert np.array_equal(got[:, 37], np.full(L, n, np.uint64)) and not got[:, :37].any()
    assert a.qual_by_cycle(0, 1).shape == (0, 0)
    a.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 4. pure sums
# ---------------------------------------------------------------------------------------------------------------------------
def test_sums_reset_and_replay(groups):
    cols, ref = groups
    n = len(cols["flag"])
    H = qbc_ref.table(cols, 3, 300)
    halves = split(cols, [n // 2 + 3])
    vecs = []
    for part in halves:
        a = context(ref, 3, 300)
        a.submit(part)
        vecs.append(a.state_export_host())
        a.close()
    c = context(ref, 3, 300)
    c.state_import_host(vecs[0] + vecs[1])
    assert np.array_equal(module_words(c, 3, 300), H)
    check_tables(c, c.finalize(), H)
    c.reset()
    with pytest.raises(BamQCError) as e:  # (nothing finalised since the reset)
        c.qual_by_cycle(0, 0)
    assert e.value.code == ERR_STATE
    assert not module_words(c, 3, 300).any()
    c.finalize()
    assert c.qual_by_cycle(0, 0).shape == (0, 0)
    c.reset()
    d = c.upload(cols)
    c.process(d)
    c.process(d)
    counts = c.finalize()
    assert np.array_equal(module_words(c, 3, 300), 2 * H)
    check_tables(c, counts, 2 * H)
    d.free()
    c.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 5. off means off
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sketch", [{}, dict(klist=[5], qlist=[17])])
def test_off_means_off(groups, sketch):
    cols, ref = groups
    off = context(ref, 3, 0, **sketch)
    on = context(ref, 3, 16, **sketch)
    assert on.state_words == off.state_words + 3 * 2 * 16 * 224  # the module's words, behind everything the vector held before
    off.submit(cols)
    on.submit(cols)
    v_off, v_on = off.state_export_host(), on.state_export_host()
    if not sketch:  # (the sketch's saturating counters are not plain words of the state; the rest is)
        assert np.array_equal(v_on[:len(v_off)], v_off)
    assert np.array_equal(v_on[len(v_off):].reshape(3, 2, 16, 224), qbc_ref.table(cols, 3, 16))
    off.finalize()
    with pytest.raises(BamQCError) as e:
        off.qual_by_cycle(0, 0)
    assert e.value.code == ERR_STATE
    on.finalize()
    for lane, mate in ((3, 0), (0, 2)):
        with pytest.raises(BamQCError) as e:
            on.qual_by_cycle(lane, mate)
        assert e.value.code == ERR_ARG
    off.close()
    on.close()
    with pytest.raises(BamQCError) as e:  # a capacity behind max_read_len is refused
        Aggregator(n_lanes=1, qual_by_cycle=4097, **OPTS)
    assert e.value.code == ERR_ARG


# ---------------------------------------------------------------------------------------------------------------------------
# 6. the program
# ---------------------------------------------------------------------------------------------------------------------------
CHROMS = ["-c", "chr1,chr2"]


def run(args, env=None, **kw):
    return subprocess.run([EXE] + args, capture_output=True, env=dict(os.environ, **(env or {})), timeout=120, **kw)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """About 20 000 synthetic paired reads in two read groups, the `.bamqc` of a run without the option, and the expected text."""
    d = tmp_path_factory.mktemp("qbc")
    bam, fa = str(d / "in.bam"), str(d / "in.fa")
    hostio.synth_write(bam, fa, seed=21, n_reads=20_000, ref_names=["chr1", "chr2"], ref_lens=[400_000, 150_000], n_lanes=2)
    base = str(d / "base.bamqc")
    r = run(["-r", fa, "-o", base] + CHROMS + [bam])
    assert r.returncode == 0, r.stderr
    assert not os.path.exists(base + ".qbc")
    cols, refs, lanes, sample = pybam.columns(bam)
    assert len(lanes) == 2
    parsed = bamqc_text.parse(base)
    names = sorted(lanes)  # the `.bamqc` lists the lanes by name
    idx = [lanes[nm] for nm in names]
    cycles = np.zeros((2, 2), np.int64)
    for nm in names:
        cycles[lanes[nm]] = [len(parsed[nm]["As_by_position_first"]), len(parsed[nm]["As_by_position_second"])]

    def want(N):
        return qbc_ref.text(qbc_ref.table(cols, 2, N), cycles, sample, names, idx)
    return dict(dir=d, bam=bam, fa=fa, base=base, want=want)


def same_bytes(a, b):
    return open(a, "rb").read() == open(b, "rb").read()


@pytest.mark.parametrize("decode", ["0", "1"])
def test_program_bam(files, decode):
    out = str(files["dir"] / ("bam%s.bamqc" % decode))
    r = run(["-r", files["fa"], "-o", out, "--qual-by-cycle"] + CHROMS + [files["bam"]], env=dict(BQC_GPU_DECODE=decode))
    assert r.returncode == 0, r.stderr
    assert same_bytes(out, files["base"])
    assert open(out + ".qbc").read() == files["want"](1024)


def test_program_sam_on_stdin(files):
    out = str(files["dir"] / "sam.bamqc")
    sam = pybam.bam_to_sam_text(files["bam"]).encode()
    r = run(["-r", files["fa"], "-o", out, "--qual-by-cycle-len", "100"] + CHROMS + ["-"], input=sam)
    assert r.returncode == 0, r.stderr
    assert same_bytes(out, files["base"])
    assert open(out + ".qbc").read() == files["want"](100)


def test_program_two_workers_on_one_card(files):
    out = str(files["dir"] / "gpus2.bamqc")
    r = run(["--gpus", "2", "-r", files["fa"], "-o", out, "--qual-by-cycle"] + CHROMS + [files["bam"]], env=dict(BQC_GPUS_SHARE_DEVICE="1"))
    assert r.returncode == 0, r.stderr
    assert same_bytes(out, files["base"])
    assert open(out + ".qbc").read() == files["want"](1024)


def test_program_manifest(files):
    d = files["dir"]
    outs = [str(d / "m1.bamqc"), str(d / "m2.bamqc")]
    lst = str(d / "jobs.tsv")
    with open(lst, "w") as f:
        for o in outs:
            f.write("%s\t%s\n" % (files["bam"], o))
    r = run(["-r", files["fa"], "--qual-by-cycle-len", "300", "--manifest", lst] + CHROMS)
    assert r.returncode == 0, r.stderr
    for o in outs:
        assert same_bytes(o, files["base"])
        assert open(o + ".qbc").read() == files["want"](300)


def test_program_reports_a_table_it_cannot_write(files):
    d = files["dir"]
    out = str(d / "blocked.bamqc")
    os.mkdir(out + ".qbc")  # (a directory where the table's file would go)
    r = run(["-r", files["fa"], "-o", out, "--qual-by-cycle"] + CHROMS + [files["bam"]])
    assert r.returncode == 1
    assert b"Could not write output file" in r.stderr and b".qbc" in r.stderr
