"""GPU: substitutions by sequence context and by cycle (bqc_enable_substitutions, --substitutions; bamqc_amd/csrc/k_sbc.hip) against
the restatement of the statistic (tests/sbc_ref.py), through the C ABI: the views AND the module's whole block of the exported state,
word for word.

The kernel walks a read's CIGAR into runs of stored positions as k_mbc does (at most 768 in LDS at a time, lane j of a wave the stored
bases 4j .. 4j+3 of a run, 256 positions a pass), loads the genome bytes of a lane's positions and of one neighbour on either side as
one to three aligned dwords wherever they start and never outside [0, len) of the contig, counts Y in an LDS tile of [2 mates][16]
[1024 cycles] and X in one table, both of one read group at a time, and sends cycles at or behind 1024 to device memory.  The
batches (tests/sbc_steps.py; tests/test_substitutions_cpu.py asserts that they cross those edges) are compared at several capacities.

Two things the issue words differently from what a test can do here: the library starts every contig on a 256-byte boundary, so the
window sweep varies the residue of the contig's LENGTH (where its last byte lies in its dword), of `pos` and of the run's first stored
position instead of the pointer's; and a manifest's jobs share one command line, so jobs with different --substitutions-min-qual run
as two lists (as the adapter sets of --adapter-by-cycle do)."""
import os
import subprocess

import numpy as np
import pytest

from bamqc_amd import Aggregator, BamQCError, hostio
from tests import bamqc_text, mbc_ref, pybam, sbc_ref, sbc_steps
from tests.parity import split
from tests.test_gpu_value_limits import n_cu

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "bin", "bamqualcheck")
ERR_ARG, ERR_STATE = 1, 8
OPTS = dict(max_read_len=4096, isize=2000)
XW = 512


def context(refs, n_lanes, N, Q=20, MQ=30, **more):
    """refs: a list by rid, None for a contig that is never set."""
    a = Aggregator(n_lanes=n_lanes, substitutions=N, subst_min_qual=Q, subst_min_mapq=MQ, **dict(OPTS, n_refs=len(refs), **more))
    for rid, r in enumerate(refs):
        if r is not None:
            a.set_reference(rid, r)
    return a


def module_words(a, n_lanes, N, behind=0, front=None):
    """The module's words of the flat state vector: n_lanes x 2 x (512 + 16 N), `behind` words from its end (or from word `front`)."""
    v = a.state_export_host()
    n = n_lanes * 2 * sbc_ref.mate_words(N)
    lo = len(v) - behind - n if front is None else front
    return v[lo:lo + n].reshape(n_lanes, 2, -1)


def check_words(got, T):
    bad = np.argwhere(got != T)
    assert not len(bad), "%d words differ, first (lane, mate, word) = %s: %d != %d" % (len(bad), bad[0].tolist(), got[tuple(bad[0])], T[tuple(bad[0])])


def check_views(a, T, N):
    for l in range(T.shape[0]):
        for m in range(2):
            X, Y = a.substitutions(l, m)
            wx, wy = sbc_ref.views(T[l, m], N)
            assert X.shape == (2, 64, 4) and Y.shape == wy.shape, (l, m, X.shape, Y.shape, wy.shape)
            assert np.array_equal(X, wx) and np.array_equal(Y, wy), (l, m)


def run_and_check(cols, refs, n_lanes, N, Q=20, MQ=30, T=None):
    if T is None:
        T = sbc_ref.table_fast(cols, refs, n_lanes, N, Q, MQ)[0]
    a = context(refs, n_lanes, N, Q, MQ)
    a.submit(cols)
    a.finalize()
    check_words(module_words(a, n_lanes, N), T)
    check_views(a, T, N)
    a.close()
    return T


_made = {}


def made(name, *args):
    """A batch is built once and never changed."""
    if (name, args) not in _made:
        _made[(name, args)] = getattr(sbc_steps, name)(*args)
    return _made[(name, args)]


# ---------------------------------------------------------------------------------------------------------------------------
# 1. the rule
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [16, 300, 1024])
def test_rule(N):
    cols, refs = made("rule_batch")
    T, miss = sbc_ref.table(cols, refs, 3, N)  # (the loops: this batch is small)
    assert all(T[l, m, s * 256:(s + 1) * 256].any() for l in range(3) for m in range(2) for s in range(2))
    assert all(T[l, m, XW + 16 * c:XW + 16 * c + 16].any() for l in range(3) for m in range(2) for c in {0, 15, min(N, 300) - 1, N - 1})
    assert (miss > 0).all()
    run_and_check(cols, refs, 3, N, T=T)


# ---------------------------------------------------------------------------------------------------------------------------
# 2. the genome window at every alignment, 3. CIGAR shapes
# ---------------------------------------------------------------------------------------------------------------------------
def test_genome_window_alignment():
    cols, refs = made("window_batch")
    T = run_and_check(cols, refs, 1, 64, 0, 0)
    assert all(T[0, m, s * 256:(s + 1) * 256].any() for m in range(2) for s in range(2))
    # read by read in stream order as well, in pieces: what a read adds does not depend on its neighbours in the list of runs
    a = context(refs, 1, 64, 0, 0)
    for part in split(cols, [1, 2, 3, 900, 901, 5000]):
        a.submit(part)
    check_words(module_words(a, 1, 64), T)
    a.close()


@pytest.mark.parametrize("N", [1024, 16, 300, 4096])
def test_cigar_shapes(N):
    cols, refs = made("shapes_batch")
    T = run_and_check(cols, refs, 1, N)
    if N > sbc_steps.SB_C:  # both sides of the LDS tile's edge
        assert all(T[0, m, XW + 16 * c:XW + 16 * c + 16].any() for m in range(2) for c in (sbc_steps.SB_C - 1, sbc_steps.SB_C, 3999))


# ---------------------------------------------------------------------------------------------------------------------------
# 4. seams: more than one step per workgroup, a read-group change on a seam; long reads on both sides of the tile's edge
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant,N", [("short", 300), ("long", 64)])
def test_three_steps_per_workgroup(variant, N):
    cu = n_cu()
    lay = sbc_steps.step_layout(cu, variant, N)
    cols, ref = made("step_batch_of", cu, variant, N)
    assert min(lay["mbc"]["steps"]) >= 3 and lay["changes"][0] in lay["mbc_seams"]
    T = sbc_ref.table_fast(cols, [ref], 4, N)[0]
    assert all(T[l, m].any() for l in range(4) for m in range(2))
    a = Aggregator(n_lanes=4, substitutions=N, mismatch_by_cycle=N, n_refs=1, **OPTS)
    a.set_reference(0, ref)
    a.submit(cols)
    a.finalize()
    n_m = 4 * 2 * 2 * N * 224
    check_words(module_words(a, 4, N, behind=n_m), T)
    check_views(a, T, N)
    a.close()


def test_long_reads_across_the_tile():
    """Reads of 500 to 4096 bases on both strands at N = SB_C and at 4096 > SB_C: the LDS and the global path of Y, a cycle at
    SB_C - 1 and at SB_C; three read groups in runs."""
    from tests.long_layout import reads_on_ref
    rng = np.random.default_rng(81)
    ref = rng.integers(0, 4, 60_000).astype(np.uint8)
    C_ = sbc_steps.SB_C
    L = np.array([C_ - 1, C_, C_ + 1, 500, 511, 512, 513, 2000, 4096] * 12)
    n = len(L)
    flag = np.array([sbc_steps.flag_of((k // 9) & 1, (k // 18) & 1) for k in range(n)], np.uint16)  # (36 reads a read group: every length of every kind)
    cols = reads_on_ref(ref, 13 * np.arange(n), L, flag, sbc_steps.QUALS[rng.integers(0, 9, int(L.sum()))], lane=np.arange(n) * 3 // n)
    cols["mapq"][:] = 30
    sbc_steps.plant(cols, rng, 0.05)
    for N in (C_, 4096):
        T = run_and_check(cols, [ref], 3, N)
        assert all(T[l, m, XW + 16 * c:XW + 16 * c + 16].any() for l in range(3) for m in range(2) for c in (C_ - 1, min(C_, N - 1), N - 1))


# ---------------------------------------------------------------------------------------------------------------------------
# 5. one bin of X takes every pair
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mismatch", [False, True])
def test_70000_reads_in_one_bin(mismatch):
    n = 70_000
    cols, ref = sbc_steps.hot_batch(n, mismatch)
    a = context([ref], 1, 1024)
    a.submit(cols)
    a.finalize()
    X, Y = a.substitutions(0, 0)
    want_x = np.zeros((2, 64, 4), np.uint64)
    want_x[0, 0, 1 if mismatch else 0] = n * 16
    want_y = np.zeros((16, 4, 4), np.uint64)
    want_y[:, 0, 1 if mismatch else 0] = n
    assert np.array_equal(X, want_x) and np.array_equal(Y, want_y)
    assert a.substitutions(0, 1)[1].shape == (0, 4, 4) and not a.substitutions(0, 1)[0].any()
    check_words(module_words(a, 1, 1024), sbc_ref.table_fast(cols, [ref], 1, 1024)[0])
    a.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 6. thresholds, 7. identities with the mismatches by cycle
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Q,MQ", [(0, 0), (20, 30), (222, 255)])
def test_thresholds(Q, MQ):
    cols, ref = made("groups_batch")
    assert {0, 29, 30, 254, 255} <= set(cols["mapq"].tolist()) and {19, 20, 222} <= set(cols["qual"].tolist())
    T = run_and_check(cols, [ref], 3, 300, Q, MQ)
    assert all(T[l, m].any() for l in range(3) for m in range(2))


def test_identities_with_mismatch_by_cycle():
    cols, ref = made("groups_batch")
    N = 300
    a = Aggregator(n_lanes=3, substitutions=N, subst_min_qual=0, subst_min_mapq=0, mismatch_by_cycle=N, n_refs=1, **OPTS)
    a.set_reference(0, ref)
    a.submit(cols)
    a.finalize()
    T, miss = sbc_ref.table_fast(cols, [ref], 3, N, 0, 0)
    n_m = 3 * 2 * 2 * N * 224
    check_words(module_words(a, 3, N, behind=n_m), T)
    v = a.state_export_host()
    M = v[len(v) - n_m:].reshape(3, 2, 2, N, 224)
    assert np.array_equal(M, mbc_ref.table_fast(cols, [ref], 3, N))
    off_diag = np.array([t != b for t in range(4) for b in range(4)])
    for l in range(3):
        for m in range(2):
            X, Y = a.substitutions(l, m)
            Yn = np.zeros((N, 16), np.uint64)
            Yn[:len(Y)] = Y.reshape(-1, 16)
            assert np.array_equal(Yn.sum(axis=1), M[l, m, 0].sum(axis=1))               # sum of the 16 bins = sum_q aligned[c][q]
            assert np.array_equal(Yn[:, off_diag].sum(axis=1), M[l, m, 1].sum(axis=1))  # the bins with t' != b' = sum_q mismatch[c][q]
            assert int(X.sum()) == int(Y.sum()) - int(miss[l, m]) and miss[l, m] > 0
    a.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 8. pure sums
# ---------------------------------------------------------------------------------------------------------------------------
def test_sums_reset_and_pieces():
    cols, ref = made("groups_batch")
    T = sbc_ref.table_fast(cols, [ref], 3, 300)[0]
    n = len(cols["flag"])
    vecs = []
    for part in split(cols, [n // 2 + 3]):
        a = context([ref], 3, 300)
        a.submit(part)
        vecs.append(a.state_export_host())
        a.close()
    c = context([ref], 3, 300)
    c.state_import_host(vecs[0] + vecs[1])  # export + import into a fresh context adds
    check_words(module_words(c, 3, 300), T)
    c.finalize()
    check_views(c, T, 300)
    c.reset()
    with pytest.raises(BamQCError) as e:  # (nothing finalised since the reset)
        c.substitutions(0, 0)
    assert e.value.code == ERR_STATE
    assert not module_words(c, 3, 300).any()
    c.finalize()
    assert c.substitutions(0, 0)[1].shape == (0, 4, 4)
    c.reset()
    for part in split(cols, [7, 1300]):  # a batch in pieces equals the batch whole
        c.submit(part)
    c.finalize()
    check_words(module_words(c, 3, 300), T)
    check_views(c, T, 300)
    c.reset()
    d = c.upload(cols)  # a resident batch, processed twice
    c.process(d)
    c.process(d)
    c.finalize()
    check_words(module_words(c, 3, 300), 2 * T)
    d.free()
    # another capacity, or the module off: another vector, which the import does not take
    other, off = context([ref], 3, 16), Aggregator(n_lanes=3, n_refs=1, **OPTS)
    mw = lambda N: 3 * 2 * sbc_ref.mate_words(N)
    assert c.state_words - mw(300) == other.state_words - mw(16) == off.state_words
    for x in (other, off):
        with pytest.raises(AssertionError):
            x.state_import_host(c.state_export_host())
    for x in (c, other, off):
        x.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 9. the enable call
# ---------------------------------------------------------------------------------------------------------------------------
def test_enable_errors():
    cols, ref = made("groups_batch")
    base = dict(n_lanes=3, n_refs=1, **OPTS)
    for kw, word in ((dict(substitutions=0), "0"), (dict(substitutions=4097), "4097"), (dict(substitutions=1 << 31), str(1 << 31)),
                     (dict(substitutions=16, subst_min_qual=223), "223"), (dict(substitutions=16, subst_min_mapq=256), "256")):
        with pytest.raises(BamQCError) as e:
            Aggregator(**dict(base, **kw))
        assert e.value.code == ERR_ARG and word in str(e.value), str(e.value)
    a = Aggregator(substitutions=4096, subst_min_qual=222, subst_min_mapq=255, **base)  # (the limits themselves are values)
    with pytest.raises(BamQCError) as e:
        a.enable_substitutions(4096)
    assert e.value.code == ERR_STATE
    a.close()
    a = Aggregator(**base)
    a.set_reference(0, ref)
    a.submit(cols)
    with pytest.raises(BamQCError) as e:  # (the context has taken a batch)
        a.enable_substitutions(16)
    assert e.value.code == ERR_STATE
    a.finalize()
    with pytest.raises(BamQCError) as e:  # (the module is off)
        a.substitutions(0, 0)
    assert e.value.code == ERR_STATE
    a.close()
    a = Aggregator(**base)
    a.state_export_host()
    with pytest.raises(BamQCError) as e:  # (state has been exchanged)
        a.enable_substitutions(16)
    assert e.value.code == ERR_STATE
    a.close()
    a = Aggregator(**base)
    a.finalize()
    with pytest.raises(BamQCError) as e:  # (finalised)
        a.enable_substitutions(16)
    assert e.value.code == ERR_STATE
    a.close()
    a = context([ref], 3, 16)
    a.finalize()
    for lane, mate in ((3, 0), (0, 2)):
        with pytest.raises(BamQCError) as e:
            a.substitutions(lane, mate)
        assert e.value.code == ERR_ARG
    a.close()


def test_enable_calls_in_every_order():
    import itertools
    cols, ref = made("groups_batch")
    base = dict(n_lanes=3, n_refs=1, **OPTS)
    N = 16
    calls = dict(s=lambda a: a.enable_substitutions(N, 20, 30), i=lambda a: a.enable_indel_by_cycle(N), g=lambda a: a.enable_gc_bias(50))
    n_s, n_i, n_g = 3 * 2 * (512 + 16 * N), 3 * 2 * (3 * N + 128), 3 * 3 * 101
    off = Aggregator(**base)
    T = sbc_ref.table_fast(cols, [ref], 3, N)[0]
    vecs = []
    for order in itertools.permutations("sig"):
        a = Aggregator(**base)
        for k in order:
            calls[k](a)
        assert a.state_words == off.state_words + n_s + n_i + n_g, order
        a.set_reference(0, ref)
        a.submit(cols)
        vecs.append(a.state_export_host())
        check_words(module_words(a, 3, N, front=off.state_words), T)  # directly behind the sketch's words, in front of the others
        a.close()
    assert all(np.array_equal(v, vecs[0]) for v in vecs[1:])
    # the other modules' words are where they were: the same distance from the end
    ig = Aggregator(indel_by_cycle=N, gc_bias=50, **base)
    ig.set_reference(0, ref)
    ig.submit(cols)
    v = ig.state_export_host()
    assert np.array_equal(v[off.state_words:], vecs[0][off.state_words + n_s:]) and v[off.state_words:].any()
    assert np.array_equal(v[:off.state_words], vecs[0][:off.state_words])
    ig.close()
    off.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 10. off means off
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sketch", [{}, dict(klist=[5], qlist=[17])])
def test_off_means_off(sketch, tmp_path):
    cols, ref = made("groups_batch")
    N = 64
    mods = dict(qual_by_cycle=N, mismatch_by_cycle=N, adapter_by_cycle=N, gc_bias=50, indel_by_cycle=N)
    base = dict(n_lanes=3, n_refs=1, **dict(OPTS, **sketch))
    plain, off, on = Aggregator(**base), Aggregator(**dict(base, **mods)), Aggregator(substitutions=N, **dict(base, **mods))
    bare = Aggregator(substitutions=N, **base)
    n_s = 3 * 2 * (512 + 16 * N)
    assert on.state_words == off.state_words + n_s and bare.state_words == plain.state_words + n_s
    texts = {}
    for name, a in (("off", off), ("on", on)):
        a.set_reference(0, ref)
        a.submit(cols)
        v = a.state_export_host()
        a.finalize()
        views = [a.qual_by_cycle(l, m) for l in range(3) for m in range(2)]
        views += [x for l in range(3) for m in range(2) for x in a.mismatch_by_cycle(l, m)]
        views += [x for l in range(3) for m in range(2) for x in a.adapter_by_cycle(l, m)]
        views += [x for l in range(3) for x in a.gc_bias(l)]
        views += [x for l in range(3) for m in range(2) for x in a.indel_by_cycle(l, m)]
        files = []
        for ext, w in (("bamqc", a.write_bamqc), ("qbc", a.write_qual_by_cycle), ("mbc", a.write_mismatch_by_cycle), ("adp", a.write_adapter_by_cycle),
                       ("gcb", a.write_gc_bias), ("ibc", a.write_indel_by_cycle)):
            path = str(tmp_path / ("%s.%s" % (name, ext)))
            w(path, sample_id="S", lane_names=["a", "b", "c"])
            files.append(open(path, "rb").read())
        texts[name] = (v, views, files)
    (v_off, views_off, files_off), (v_on, views_on, files_on) = texts["off"], texts["on"]
    behind = len(v_off) - plain.state_words  # the other modules' words
    if not sketch:  # (the sketch's saturating counters are not plain words of the state; the rest is)
        assert np.array_equal(v_on[:plain.state_words], v_off[:plain.state_words])
    assert np.array_equal(v_on[len(v_on) - behind:], v_off[len(v_off) - behind:])
    check_words(v_on[plain.state_words:plain.state_words + n_s].reshape(3, 2, -1), sbc_ref.table_fast(cols, [ref], 3, N)[0])
    assert len(views_off) == len(views_on) and all(np.array_equal(x, y) for x, y in zip(views_off, views_on))
    assert files_off == files_on and all(files_off)
    for a in (plain, off, on, bare):
        a.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 11. the program
# ---------------------------------------------------------------------------------------------------------------------------
CHROMS = ["-c", "chr1,chr2"]


def run(args, env=None, **kw):
    return subprocess.run([EXE] + args, capture_output=True, env=dict(os.environ, **(env or {})), timeout=120, **kw)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """4000 synthetic paired reads in two read groups (the generator plants substitutions, indels and clips), the same as SAM text,
    the `.bamqc` of a run without the option, and the expected texts."""
    d = tmp_path_factory.mktemp("sbc")
    bam, fa, sam = str(d / "in.bam"), str(d / "in.fa"), str(d / "in.sam")
    hostio.synth_write(bam, fa, seed=29, n_reads=4000, ref_names=["chr1", "chr2"], ref_lens=[400_000, 150_000], n_lanes=2)
    with open(sam, "w") as f:
        f.write(pybam.bam_to_sam_text(bam))
    base = str(d / "base.bamqc")
    r = run(["-r", fa, "-o", base] + CHROMS + [bam])
    assert r.returncode == 0, r.stderr
    assert not os.path.exists(base + ".sbc")
    cols, refs, lanes, sample = pybam.columns(bam)
    assert len(lanes) == 2
    genome = dict(hostio.load_fasta(fa))
    contigs = [genome[name] for name, _ in refs]
    assert set(bamqc_text.parse(base)) == set(lanes)
    names = sorted(lanes)  # the `.bamqc` lists the lanes by name
    idx = [lanes[nm] for nm in names]
    done = {}

    def want(N=1024, Q=20, MQ=30):
        if (N, Q, MQ) not in done:
            T = sbc_ref.table_fast(cols, contigs, 2, N, Q, MQ)[0]
            assert all(T[l, m, :XW].any() and T[l, m, XW:].any() for l in range(2) for m in range(2))
            done[(N, Q, MQ)] = sbc_ref.text(T, N, Q, MQ, sample, names, idx)
        return done[(N, Q, MQ)]
    return dict(dir=d, bam=bam, sam=sam, fa=fa, base=base, want=want)


def same_bytes(a, b):
    return open(a, "rb").read() == open(b, "rb").read()


@pytest.mark.parametrize("decode", ["0", "1"])
@pytest.mark.parametrize("kind", ["bam", "sam"])
def test_program(files, kind, decode):
    out = str(files["dir"] / ("%s%s.bamqc" % (kind, decode)))
    r = run(["-r", files["fa"], "-o", out, "--substitutions"] + CHROMS + [files[kind]], env=dict(BQC_GPU_DECODE=decode))
    assert r.returncode == 0, r.stderr
    assert same_bytes(out, files["base"])
    assert open(out + ".sbc").read() == files["want"]()
    assert not os.path.exists(out + ".ibc") and not os.path.exists(out + ".mbc")


def test_program_two_workers_on_one_card(files):
    out = str(files["dir"] / "gpus2.bamqc")
    r = run(["--gpus", "2", "-r", files["fa"], "-o", out, "--substitutions-len", "100", "--substitutions-min-mapq", "10", "--indel-by-cycle"] + CHROMS +
            [files["bam"]], env=dict(BQC_GPUS_SHARE_DEVICE="1"))
    assert r.returncode == 0, r.stderr
    assert same_bytes(out, files["base"])
    assert open(out + ".sbc").read() == files["want"](100, 20, 10)
    assert os.path.exists(out + ".ibc")  # both options together


def test_program_manifests_with_their_own_values(files):
    """Two jobs through one resident worker, and a second list with another --substitutions-min-qual: each job gets the values of its
    own command line."""
    d = files["dir"]
    for q in (0, 37):
        outs = [str(d / ("m%d_%d.bamqc" % (q, k))) for k in (1, 2)]
        lst = str(d / ("jobs%d.tsv" % q))
        with open(lst, "w") as f:
            for o in outs:
                f.write("%s\t%s\n" % (files["bam"], o))
        r = run(["-r", files["fa"], "--substitutions-len", "300", "--substitutions-min-qual", str(q), "--manifest", lst] + CHROMS)
        assert r.returncode == 0, r.stderr
        for o in outs:
            assert same_bytes(o, files["base"])
            assert open(o + ".sbc").read() == files["want"](300, q, 30)
    assert files["want"](300, 0, 30) != files["want"](300, 37, 30)


def test_program_reports_a_table_it_cannot_write(files):
    out = str(files["dir"] / "blocked.bamqc")
    os.mkdir(out + ".sbc")  # (a directory where the tables' file would go)
    r = run(["-r", files["fa"], "-o", out, "--substitutions"] + CHROMS + [files["bam"]])
    assert r.returncode == 1
    assert b"Could not write output file" in r.stderr and b".sbc" in r.stderr


def test_program_refuses_bad_values(files):
    out = str(files["dir"] / "never.bamqc")
    for opt, bad, words in (("--substitutions-len", "0", b"--substitutions-len wants 1 or more"), ("--substitutions-min-qual", "223", b"0 to 222"),
                            ("--substitutions-min-mapq", "256", b"0 to 255")):
        r = run(["-r", files["fa"], "-o", out, opt, bad] + CHROMS + [files["bam"]])
        assert r.returncode != 0 and words in r.stderr, r.stderr
    r = run(["-r", files["fa"], "-o", out, "--substitutions-len", "100000"] + CHROMS + [files["bam"]])  # behind --max-read-len: the library's refusal
    assert r.returncode != 0 and not os.path.exists(out + ".sbc")


# ---------------------------------------------------------------------------------------------------------------------------
# 12. the Python writer
# ---------------------------------------------------------------------------------------------------------------------------
def test_python_writer_equals_the_programs_file(files, tmp_path):
    out = str(files["dir"] / "forpy.bamqc")
    r = run(["-r", files["fa"], "-o", out, "--substitutions-len", "200", "--substitutions-min-qual", "10"] + CHROMS + [files["bam"]])
    assert r.returncode == 0, r.stderr
    cols, refs, lanes, sample = pybam.columns(files["bam"])
    genome = dict(hostio.load_fasta(files["fa"]))
    a = context([genome[name] for name, _ in refs], 2, 200, 10, 30, max_read_len=1024)
    a.submit(cols)
    a.finalize()
    names = sorted(lanes)
    path = str(tmp_path / "py.sbc")
    a.write_substitutions(path, sample_id=sample, lane_names=names, lane_index=[lanes[nm] for nm in names])
    a.close()
    assert same_bytes(path, out + ".sbc") and open(path).read() == files["want"](200, 10, 30)
