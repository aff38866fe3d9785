"""GPU: the indels by cycle and by length (bqc_enable_indel_by_cycle, --indel-by-cycle; bamqc_amd/csrc/k_ibc.hip) against the plain
restatement of the statistic (tests/ibc_ref.py): the views, and the whole module block of the exported state.

A read of at most IB_T = 8 CIGAR operations is walked by its own thread, a longer one by a wave, 64 operations a pass, with the stored
index of an operation from a 64-bit scan and a carry; [2 mates][3 rows][1024 cycles] and the length bins are counted in LDS for one
read group at a time and everything behind in device memory.  The shapes below cross each of those edges (tests/ibc_steps.py builds
them; tests/test_indel_by_cycle_cpu.py asserts that they do).

Not here, because the library refuses the batch before the kernel sees it (the restatement's side of each is in
tests/test_indel_by_cycle_cpu.py): a primary read without a mate flag (error key 6 of the pre-pass), a read group at or behind n_lanes
(error key 2), and inserted or deleted bases at or above hist_cap on a main chromosome (BQC_ERR_RANGE from the per-read kernels) —
the reads with long indels here lie on a contig that is not main."""
import os
import subprocess

import numpy as np
import pytest

from bamqc_amd import Aggregator, BamQCError, hostio
from tests import ibc_ref, ibc_steps, pybam
from tests.ibc_steps import IB_C, IB_T, cols_of
from tests.long_layout import dna_ref
from tests.parity import split
from tests.test_gpu_value_limits import n_cu

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "bin", "bamqualcheck")
ERR_ARG, ERR_STATE = 1, 8
K = 64
REF_LEN = 100_000


def context(n_lanes, N, **more):
    """Two contigs, the second one not main and never given: the genome is not read."""
    a = Aggregator(n_lanes=n_lanes, indel_by_cycle=N, **dict(dict(n_refs=2, main_chrom=[1, 0], max_read_len=16_384, isize=2000), **more))
    a.set_reference(0, dna_ref(77, REF_LEN))
    return a


def module_words(a, n_lanes, N, behind=0):
    """The module's words of the flat state vector: n_lanes x 2 x (3 N + 128), `behind` words from its end."""
    v = a.state_export_host()
    mw = ibc_ref.mate_words(N)
    return v[len(v) - behind - n_lanes * 2 * mw:len(v) - behind].reshape(n_lanes, 2, mw)


def check_views(a, T):
    for l in range(T.shape[0]):
        for m in range(2):
            got, want = a.indel_by_cycle(l, m), ibc_ref.views(T, l, m)
            for name, g, w in zip(("reads_by_length", "insertions", "deletions", "insertion_lengths", "deletion_lengths"), got, want):
                assert g.shape == w.shape, (l, m, name, g.shape, w.shape)
                bad = np.flatnonzero(g != w)
                assert not len(bad), "lane %d mate %d %s: %d bins differ, first %d: %d != %d" % (l, m, name, len(bad), bad[0], g[bad[0]], w[bad[0]])


def check_words(got, T):
    bad = np.argwhere(got != T)
    assert not len(bad), "%d words differ, first (lane, mate, word) = %s: %d != %d" % (len(bad), bad[0].tolist(), got[tuple(bad[0])], T[tuple(bad[0])])


def run_and_check(cols, n_lanes, N, T=None, **more):
    """One batch through a fresh context: the views and the whole block against the restatement -> the table."""
    if T is None:
        T = ibc_ref.table(cols, n_lanes, N)
    a = context(n_lanes, N, **more)
    a.submit(cols)
    a.finalize()
    check_views(a, T)
    check_words(module_words(a, n_lanes, N), T)
    a.close()
    return T


def rows(T, N):
    return T[:, :, :N], T[:, :, N:2 * N], T[:, :, 2 * N:3 * N], T[:, :, 3 * N:3 * N + K], T[:, :, 3 * N + K:]


# ---------------------------------------------------------------------------------------------------------------------------
# 1. the rule
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rule():
    return cols_of(ibc_steps.rule_reads())


@pytest.mark.parametrize("N", [16, 300, 1024])
def test_rule(rule, N):
    T = run_and_check(rule, 3, N)
    e, ic, dc, il, dl = rows(T, N)
    assert all(x[l, m].any() for x in (e, ic, dc, il, dl) for l in range(3) for m in range(2))
    assert ic[:, :, N - 1].sum() >= 2 and dc[:, :, N - 1].sum() >= 2 and il[:, :, 63].sum() >= 4 and dl[:, :, 63].sum() >= 8
    assert ic.sum() == il.sum() and dc.sum() == dl.sum()


# ---------------------------------------------------------------------------------------------------------------------------
# 2. thread path against wave path
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def paths():
    reads = ibc_steps.path_reads()
    return reads, cols_of(reads), ibc_ref.table_fast(cols_of(reads), 1, 1024)


def test_paths_mixed_in_one_step(paths):
    reads, cols, T = paths
    assert np.array_equal(T, ibc_ref.table(cols, 1, 1024))
    run_and_check(cols, 1, 1024, T, max_read_len=262_144)
    e, ic, dc, il, dl = rows(T, 1024)
    assert ic.sum() > 100 and dc.sum() > 100


def test_paths_each_read_alone(paths):
    """Every read of the mixed batch alone in a batch of its own, into one context: the same tables."""
    reads, cols, T = paths
    a = context(1, 1024, max_read_len=262_144)
    for r in reads:
        one = cols_of([r])
        a.submit(one)
    a.finalize()
    check_views(a, T)
    check_words(module_words(a, 1, 1024), T)
    a.close()
    for nc in (IB_T, IB_T + 1, 64, 65, 65_535):  # and against the restatement of the read itself
        r = [x for x in reads if len(x["cigar"]) == nc][1]
        run_and_check(cols_of([r]), 1, 1024, max_read_len=262_144)


# ---------------------------------------------------------------------------------------------------------------------------
# 3. no wrap in the scan
# ---------------------------------------------------------------------------------------------------------------------------
def test_no_wrap_past_2_to_the_32():
    cols = cols_of(ibc_steps.wrap_reads())
    T = run_and_check(cols, 1, 100)
    e, ic, dc, il, dl = rows(T, 100)
    assert ic.sum() == dc.sum() == 4 and not ic[0, 0, 26:30].any() and not dc[0, 0, 25:29].any()  # (where a 32-bit sum would put the later ones)
    assert ic[0, 0, 3] == dc[0, 0, 8] == 2


# ---------------------------------------------------------------------------------------------------------------------------
# 4. tile edges
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [10_240, IB_C, IB_C + 1])
def test_tile_edges(N):
    cols = cols_of(ibc_steps.tile_reads(10_240))
    T = run_and_check(cols, 1, N)
    e, ic, dc, il, dl = rows(T, N)
    assert ic[0, 0, IB_C - 1] >= 2 and dc[0, 1, IB_C - 1] >= 2 and e[0, :, IB_C - 1].sum() >= 2
    if N > IB_C:
        assert ic[0, 0, IB_C] >= 2 and dc[0, 1, IB_C] >= 2 and e[0, :, IB_C].sum() >= 2
    if N == 10_240:
        assert ic[0, 0, N - 1] >= 2 and dc[0, 1, N - 1] >= 2 and e[0, :, N - 1].sum() >= 2 and e[0, :, 1999].sum() >= 2


# ---------------------------------------------------------------------------------------------------------------------------
# 5. hot bins: 70 000 increments of one bin of every table in one launch
# ---------------------------------------------------------------------------------------------------------------------------
def test_70000_identical_reads():
    n = 70_000
    a = context(1, 1024)
    a.submit(ibc_steps.hot_cols(n))
    a.finalize()
    e, ic, dc, il, dl = a.indel_by_cycle(0, 0)
    want = [np.zeros(100, np.uint64) for _ in range(3)] + [np.zeros(K, np.uint64) for _ in range(2)]
    want[0][99], want[1][40], want[2][59], want[3][0], want[4][0] = n, n, n, n, n
    assert all(np.array_equal(g, w) for g, w in zip((e, ic, dc, il, dl), want))
    assert a.indel_by_cycle(0, 1)[0].shape == (0,) and a.indel_by_cycle(0, 1)[3].shape == (K,)
    assert module_words(a, 1, 1024).sum() == 5 * n
    a.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 6. read groups and steps
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def groups():
    cols = cols_of(ibc_steps.group_reads())
    return cols, ibc_ref.table(cols, 4, 300)


def test_read_groups_one_batch_and_three(groups, tmp_path):
    cols, T = groups
    run_and_check(cols, 4, 300, T)
    assert all(x[l, m].any() for x in rows(T, 300)[:3] for l in range(4) for m in range(2))
    b = context(4, 300)
    for part in split(cols, [7, 1300]):  # (the first batch is smaller than one step)
        b.submit(part)
    b.finalize()
    check_views(b, T)
    check_words(module_words(b, 4, 300), T)
    out = str(tmp_path / "groups.ibc")  # the text through the library's writer, lanes in an order of the caller's
    b.write_indel_by_cycle(out, "S", ["g2", "g0", "g3", "g1"], [2, 0, 3, 1])
    assert open(out).read() == ibc_ref.text(T, "S", ["g2", "g0", "g3", "g1"], [2, 0, 3, 1])
    b.close()


def test_three_steps_per_workgroup():
    """More than 2 x 1024 x (CU count) reads of 20 bases in four read groups: one change on a step's seam, two inside steps."""
    lay = ibc_steps.step_layout(n_cu())
    ibc_steps.assert_step_layout(lay)
    cols = ibc_steps.step_batch(lay)
    T = ibc_ref.table_fast(cols, 4, 64)
    assert all(x[l, m].sum() > 1000 for x in rows(T, 64) for l in range(4) for m in range(2))
    a = context(4, 64)
    a.submit(cols)
    a.finalize()
    check_views(a, T)
    check_words(module_words(a, 4, 64), T)
    a.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 7. state
# ---------------------------------------------------------------------------------------------------------------------------
def test_state_words_and_order(groups):
    cols, T300 = groups
    ref = dna_ref(77, REF_LEN)
    base = dict(n_lanes=4, n_refs=2, main_chrom=[1, 0], max_read_len=4096, isize=2000)
    N = 16
    n_i = 4 * 2 * (3 * N + 128)
    n_g = 4 * 3 * 101
    T = ibc_ref.table(cols, 4, N)
    off = Aggregator(**base)
    on = Aggregator(indel_by_cycle=N, **base)
    assert on.state_words == off.state_words + n_i
    gcb = Aggregator(gc_bias=50, **base)
    both = Aggregator(gc_bias=50, indel_by_cycle=N, **base)  # (gc bias enabled first)
    other = Aggregator(**base)                               # (and the other order of the two calls)
    other.enable_indel_by_cycle(N)
    other.enable_gc_bias(50)
    every = Aggregator(gc_bias=50, indel_by_cycle=N, adapter_by_cycle=8, qual_by_cycle=8, mismatch_by_cycle=4, **base)
    assert both.state_words == other.state_words == off.state_words + n_i + n_g
    n_rest = 4 * 2 * 9 * 8 + 4 * 2 * 8 * 224 + 4 * 2 * 2 * 4 * 224
    assert every.state_words == both.state_words + n_rest
    ctxs = (off, on, gcb, both, other, every)
    for a in ctxs:
        a.set_reference(0, ref)
        a.submit(cols)
    v_off, v_on, v_gcb, v_both, v_other, v_every = (a.state_export_host() for a in ctxs)
    assert np.array_equal(v_on[:len(v_off)], v_off)
    check_words(v_on[len(v_off):].reshape(4, 2, -1), T)
    # behind the sketch's words, in front of gc-bias's, in either order of the enable calls
    assert np.array_equal(v_both, v_other)
    check_words(v_both[len(v_off):len(v_off) + n_i].reshape(4, 2, -1), T)
    assert np.array_equal(v_both[len(v_off) + n_i:], v_gcb[len(v_off):]) and v_gcb[len(v_off):].any()
    assert np.array_equal(v_both[:len(v_off)], v_off)
    # and in front of everything else
    check_words(module_words(every, 4, N, behind=n_g + n_rest), T)
    assert np.array_equal(v_every[:len(v_off)], v_off) and np.array_equal(v_every[len(v_off) + n_i:len(v_off) + n_i + n_g], v_gcb[len(v_off):])
    # the view's errors
    off.finalize()
    with pytest.raises(BamQCError) as e:
        off.indel_by_cycle(0, 0)
    assert e.value.code == ERR_STATE
    with pytest.raises(BamQCError) as e:  # (finalised: the enable call comes too late)
        off.enable_indel_by_cycle(N)
    assert e.value.code == ERR_STATE
    on.finalize()
    for lane, mate in ((4, 0), (0, 2)):
        with pytest.raises(BamQCError) as e:
            on.indel_by_cycle(lane, mate)
        assert e.value.code == ERR_ARG
    for a in ctxs:
        a.close()


def test_enable_errors(groups):
    cols, T = groups
    base = dict(n_lanes=4, n_refs=2, main_chrom=[1, 0], max_read_len=4096, isize=2000)
    for bad in (0, 4097, 1 << 31):
        with pytest.raises(BamQCError) as e:
            Aggregator(indel_by_cycle=bad, **base)
        assert e.value.code == ERR_ARG and str(bad) in str(e.value), str(e.value)
    a = Aggregator(indel_by_cycle=4096, **base)  # (max_read_len itself is a capacity)
    with pytest.raises(BamQCError) as e:
        a.enable_indel_by_cycle(4096)
    assert e.value.code == ERR_STATE
    a.close()
    a = Aggregator(**base)
    a.set_reference(0, dna_ref(77, REF_LEN))
    a.submit(cols)
    with pytest.raises(BamQCError) as e:  # (the context has taken a batch)
        a.enable_indel_by_cycle(16)
    assert e.value.code == ERR_STATE
    a.close()
    a = Aggregator(**base)
    a.state_export_host()
    with pytest.raises(BamQCError) as e:  # (state has been exchanged)
        a.enable_indel_by_cycle(16)
    assert e.value.code == ERR_STATE
    a.close()


def test_sums_reset_and_replay(groups):
    cols, T = groups
    n = len(cols["flag"])
    vecs = []
    for part in split(cols, [n // 2 + 3]):
        a = context(4, 300)
        a.submit(part)
        vecs.append(a.state_export_host())
        a.close()
    c = context(4, 300)
    c.state_import_host(vecs[0] + vecs[1])  # export + import into a fresh context adds
    check_words(module_words(c, 4, 300), T)
    c.finalize()
    check_views(c, T)
    c.reset()
    with pytest.raises(BamQCError) as e:  # (nothing finalised since the reset)
        c.indel_by_cycle(0, 0)
    assert e.value.code == ERR_STATE
    assert not module_words(c, 4, 300).any()
    c.finalize()
    got = c.indel_by_cycle(0, 0)
    assert got[0].shape == got[1].shape == got[2].shape == (0,) and got[3].shape == (K,) and not got[3].any()
    c.reset()
    d = c.upload(cols)
    c.process(d)
    c.process(d)  # two batches add
    c.finalize()
    check_words(module_words(c, 4, 300), 2 * T)
    check_views(c, 2 * T)
    d.free()
    c.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 8. cross-checks against output that exists today
# ---------------------------------------------------------------------------------------------------------------------------
def test_against_the_reference_histograms():
    cols = cols_of(ibc_steps.cross_reads())
    N = 2048
    assert int(cols["l_seq"].max()) <= N
    a = context(2, N)
    a.submit(cols)
    counts = a.finalize()
    T = ibc_ref.table(cols, 2, N)
    check_views(a, T)
    length = np.arange(1, K + 1, dtype=np.uint64)
    for l in range(2):
        for m in range(2):
            e, ic, dc, il, dl = a.indel_by_cycle(l, m)
            assert not il[63] and not dl[63]
            inshist, delhist = counts[l]["r%d.inshist" % (m + 1)], counts[l]["r%d.delhist" % (m + 1)]
            assert (length * il).sum() == (np.arange(len(inshist), dtype=np.uint64) * inshist).sum() > 0
            assert (length * dl).sum() == (np.arange(len(delhist), dtype=np.uint64) * delhist).sum() > 0
            assert ic.sum() == il.sum() and dc.sum() == dl.sum()
            f = cols["flag"]
            assert e.sum() == int(((cols["lane"] == l) & (((f & 0x40) != 0) == (m == 0))).sum())
    a.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 9. the program
# ---------------------------------------------------------------------------------------------------------------------------
CHROMS = ["-c", "chr1,chr2"]


def run(args, env=None, **kw):
    return subprocess.run([EXE] + args, capture_output=True, env=dict(os.environ, **(env or {})), timeout=120, **kw)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """About 20 000 synthetic paired reads in two read groups, the `.bamqc` of a run without the option, and the expected text."""
    d = tmp_path_factory.mktemp("ibc")
    bam, fa = str(d / "in.bam"), str(d / "in.fa")
    hostio.synth_write(bam, fa, seed=23, n_reads=20_000, ref_names=["chr1", "chr2"], ref_lens=[400_000, 150_000], n_lanes=2)
    base = str(d / "base.bamqc")
    r = run(["-r", fa, "-o", base] + CHROMS + [bam])
    assert r.returncode == 0, r.stderr
    assert not os.path.exists(base + ".ibc")
    cols, refs, lanes, sample = pybam.columns(bam)
    assert len(lanes) == 2
    names = sorted(lanes)  # the `.bamqc` lists the lanes by name
    idx = [lanes[nm] for nm in names]

    def want(N):
        return ibc_ref.text(ibc_ref.table_fast(cols, 2, N), sample, names, idx)
    T = ibc_ref.table_fast(cols, 2, 1024)
    assert T[:, :, 1024:2048].sum() > 100 and T[:, :, 2048:3072].sum() > 100  # (the file's reads do have indels)
    return dict(dir=d, bam=bam, fa=fa, base=base, want=want)


def same_bytes(a, b):
    return open(a, "rb").read() == open(b, "rb").read()


@pytest.mark.parametrize("decode", ["0", "1"])
def test_program_bam(files, decode):
    out = str(files["dir"] / ("bam%s.bamqc" % decode))
    r = run(["-r", files["fa"], "-o", out, "--indel-by-cycle"] + CHROMS + [files["bam"]], env=dict(BQC_GPU_DECODE=decode))
    assert r.returncode == 0, r.stderr
    assert same_bytes(out, files["base"])
    assert open(out + ".ibc").read() == files["want"](1024)


def test_program_sam_on_stdin(files):
    out = str(files["dir"] / "sam.bamqc")
    sam = pybam.bam_to_sam_text(files["bam"]).encode()
    r = run(["-r", files["fa"], "-o", out, "--indel-by-cycle-len", "100"] + CHROMS + ["-"], input=sam)
    assert r.returncode == 0, r.stderr
    assert same_bytes(out, files["base"])
    assert open(out + ".ibc").read() == files["want"](100)


def test_program_two_workers_on_one_card(files):
    out = str(files["dir"] / "gpus2.bamqc")
    r = run(["--gpus", "2", "-r", files["fa"], "-o", out, "--indel-by-cycle"] + CHROMS + [files["bam"]], env=dict(BQC_GPUS_SHARE_DEVICE="1"))
    assert r.returncode == 0, r.stderr
    assert same_bytes(out, files["base"])
    assert open(out + ".ibc").read() == files["want"](1024)


def test_program_manifest(files):
    """Two jobs through one resident worker."""
    d = files["dir"]
    outs = [str(d / "m1.bamqc"), str(d / "m2.bamqc")]
    lst = str(d / "jobs.tsv")
    with open(lst, "w") as f:
        for o in outs:
            f.write("%s\t%s\n" % (files["bam"], o))
    r = run(["-r", files["fa"], "--indel-by-cycle-len", "300", "--manifest", lst] + CHROMS)
    assert r.returncode == 0, r.stderr
    for o in outs:
        assert same_bytes(o, files["base"])
        assert open(o + ".ibc").read() == files["want"](300)


def test_program_all_five_modules(files):
    d = files["dir"]
    four, five = str(d / "four.bamqc"), str(d / "five.bamqc")
    mods = ["--qual-by-cycle", "--mismatch-by-cycle", "--adapter-by-cycle", "--gc-bias"]
    r = run(["-r", files["fa"], "-o", four] + mods + CHROMS + [files["bam"]])
    assert r.returncode == 0, r.stderr
    r = run(["-r", files["fa"], "-o", five] + mods + ["--indel-by-cycle"] + CHROMS + [files["bam"]])
    assert r.returncode == 0, r.stderr
    for ext in ("", ".qbc", ".mbc", ".adp", ".gcb"):
        assert same_bytes(five + ext, four + ext), ext
    assert same_bytes(five, files["base"])
    assert open(five + ".ibc").read() == files["want"](1024)


def test_program_reports_a_table_it_cannot_write(files):
    out = str(files["dir"] / "blocked.bamqc")
    os.mkdir(out + ".ibc")  # (a directory where the table's file would go)
    r = run(["-r", files["fa"], "-o", out, "--indel-by-cycle"] + CHROMS + [files["bam"]])
    assert r.returncode == 1
    assert b"Could not write output file" in r.stderr and b".ibc" in r.stderr


def test_program_refuses_a_bad_length(files):
    out = str(files["dir"] / "no.bamqc")
    r = run(["-r", files["fa"], "-o", out, "--indel-by-cycle-len", "0"] + CHROMS + [files["bam"]])
    assert r.returncode == 1 and b"--indel-by-cycle-len wants 1 or more" in r.stderr
    r = run(["-r", files["fa"], "-o", out, "--indel-by-cycle-len", "12x"] + CHROMS + [files["bam"]])
    assert r.returncode == 1 and b"is not a number of cycles" in r.stderr
    assert not os.path.exists(out + ".ibc")
