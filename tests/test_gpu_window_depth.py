"""GPU: depth in fixed genome windows (bqc_enable_window_depth, --window-depth; bamqc_amd/csrc/k_wdp.hip) against the restatement of
the statistic (tests/wdp_ref.py), through the C ABI: the module's whole block of the exported state, word for word, AND the views that
bqc_finalize makes of it on the host.

k_wdp walks every examined read's CIGAR (a thread for at most 8 operations, a wave beyond), clips every run of covered bases to its
contig and adds its bases window by window; adds of neighbouring lanes to one word (read group, plane, window) are summed first and
leave as one (BQC_WDP_COMBINE=0: never, =2: in every wave; all give the same words).  The batches (tests/wdp_steps.py;
tests/test_window_depth_cpu.py asserts that they cross those edges) put no read on a main chromosome and load no contig, except where
the histogram over the main contigs is what is looked at.

An M of exactly k W bases is run at W = 100, 1000 and 1024; at W = 999 983 and 2^24 one such operation would need a read of 1 M to
50 M bases, so there the borders are crossed by short runs placed by pos and behind deletions."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from bamqc_amd import Aggregator, BamQCError, _abi, hostio
from tests import lane_limit, pybam, rcv_ref, synth, wdp_ref, wdp_steps
from tests.parity import split
from tests.wdp_steps import cols_of

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "bin", "bamqualcheck")
ERR_ARG, ERR_STATE = 1, 8
MODES = [None, "0", "2"]


def context(W, lens, n_lanes, MQ=20, **more):
    """No contig is main and none is given: the genome is not read."""
    return Aggregator(n_lanes=n_lanes, window_depth=(W, lens), window_min_mapq=MQ,
                      **dict(dict(n_refs=len(lens), main_chrom=[0] * len(lens), max_read_len=16_384, isize=2000), **more))


def lane_words(W, lens):
    return 4 + 3 * wdp_ref.layout(W, lens)[3]


def module_words(a, n_lanes, W, lens, behind=0, front=None):
    """The module's words of the flat state vector: n_lanes x (4 + 3 NW), `behind` words from its end (or from word `front`)."""
    v = a.state_export_host()
    n = n_lanes * lane_words(W, lens)
    lo = len(v) - behind - n if front is None else front
    return v[lo:lo + n].reshape(n_lanes, -1)


def check_words(got, St):
    assert got.shape == St.shape, (got.shape, St.shape)
    bad = np.argwhere(got != St)
    assert not len(bad), "%d words differ, first (lane, word) = %s: %d != %d" % (len(bad), bad[0].tolist(), got[tuple(bad[0])], St[tuple(bad[0])])


def check_views(a, prod, W, lens, MQ=20):
    ln, nw, woff, NW = wdp_ref.layout(W, lens)
    for l, want in enumerate(prod):
        got = a.window_depth(l)
        assert (got["window"], got["min_mapq"], got["n_windows"]) == (W, MQ, NW)
        assert got["woff"].tolist() == woff.tolist() and got["ref_len"].tolist() == ln.tolist()
        for key in ("reads_examined", "reads_low_mapq", "bases_outside"):
            assert got[key] == want[key], (l, key, got[key], want[key])
        for key in ("reads", "bases", "bases_low", "contigs", "hist"):
            assert got[key].shape == want[key].shape, (key, got[key].shape, want[key].shape)
            bad = np.argwhere(got[key] != want[key])
            assert not len(bad), "lane %d %s: %d entries differ, first %s: %d != %d" % (l, key, len(bad), bad[0].tolist(), got[key][tuple(bad[0])], want[key][tuple(bad[0])])


def run_and_check(cols, W, lens, n_lanes, MQ=20, St=None, **more):
    if St is None:
        St = wdp_ref.state_fast(cols, W, lens, n_lanes, MQ)
    a = context(W, lens, n_lanes, MQ, **more)
    a.submit(cols)
    a.finalize()
    check_words(module_words(a, n_lanes, W, lens), St)
    prod = wdp_ref.products(St, W, lens, [0] * len(lens))
    check_views(a, prod, W, lens, MQ)
    a.close()
    return St, prod


@pytest.fixture(params=MODES, ids=["default", "never", "always"])
def mode(request, monkeypatch):
    if request.param is None:
        monkeypatch.delenv("BQC_WDP_COMBINE", raising=False)
    else:
        monkeypatch.setenv("BQC_WDP_COMBINE", request.param)
    return request.param


# ---------------------------------------------------------------------------------------------------------------------------
# 1. the rule
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("MQ", [0, 20, 255])
def test_rule(MQ):
    cols = wdp_steps.rule_batch(MQ)
    St = wdp_ref.state(cols, wdp_steps.RULE_W, wdp_steps.RULE_LENS, 3, MQ)  # (the loops: this batch is small)
    St, prod = run_and_check(cols, wdp_steps.RULE_W, wdp_steps.RULE_LENS, 3, MQ, St=St)
    assert all(p["bases_outside"] > 0 and p["reads_examined"] > 0 and (p["reads_low_mapq"] > 0) == (MQ > 0) for p in prod)


# ---------------------------------------------------------------------------------------------------------------------------
# 2. window borders, 3. coordinates
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", wdp_steps.BORDER_WS)
def test_window_borders(W):
    cols, lens = wdp_steps.border_batch(W)
    St, prod = run_and_check(cols, W, lens, 2)
    assert all(p["contigs"][:, 1:].sum() > 0 for p in prod)


@pytest.mark.parametrize("W", wdp_steps.COORD_WS)
def test_coordinates(W):
    cols = wdp_steps.coord_batch(W)
    St, prod = run_and_check(cols, W, wdp_steps.COORD_LENS, 2)
    nw0 = int(wdp_ref.layout(W, wdp_steps.COORD_LENS)[1][0])
    assert prod[0]["bases"][nw0 - 1] > 0 and all(p["bases_outside"] > 0 for p in prod)


# ---------------------------------------------------------------------------------------------------------------------------
# 4. many windows under one operation; CIGAR lengths: thread path against wave path
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def paths():
    reads, lens = wdp_steps.path_batch()
    cols = cols_of(reads, 4)
    return reads, lens, cols, wdp_ref.state_fast(cols, wdp_steps.PATH_W, lens, 1, 20)


def test_paths_mixed_in_one_step(paths, mode):
    reads, lens, cols, St = paths
    run_and_check(cols, wdp_steps.PATH_W, lens, 1, 20, St=St)
    assert St[0, 2] > 4000 and (St[0, 4 + St.shape[1] // 3 + 10:4 + St.shape[1] // 3 + 100] >= 100).all()


def test_paths_each_read_alone(paths):
    """Every read of the mixed batch alone in a batch of its own, into one context: the same words."""
    reads, lens, cols, St = paths
    a = context(wdp_steps.PATH_W, lens, 1, 20)
    for k in range(len(reads)):
        a.submit(cols_of(reads[k:k + 1], 100 + k))
    a.finalize()
    check_words(module_words(a, 1, wdp_steps.PATH_W, lens), St)
    check_views(a, wdp_ref.products(St, wdp_steps.PATH_W, lens, [0, 0]), wdp_steps.PATH_W, lens)
    a.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 5. combining
# ---------------------------------------------------------------------------------------------------------------------------
def test_20000_reads_in_one_window(mode):
    n = 20_000
    cols = wdp_steps.hot_batch(n)
    a = context(wdp_steps.HOT_W, wdp_steps.HOT_LENS, 2)
    a.submit(cols)
    a.finalize()
    want = np.zeros((2, 4 + 15), np.uint64)
    want[:, 0] = n // 2
    want[:, 4 + 1] = n // 2           # the reads begin in window 1 ...
    want[:, 4 + 5 + 1] = n // 2 * 60  # ... and lie in it
    check_words(module_words(a, 2, wdp_steps.HOT_W, wdp_steps.HOT_LENS), want)
    a.close()


def test_runs_of_equal_words_across_waves(mode):
    run_and_check(wdp_steps.runs_batch(), wdp_steps.RUN_W, wdp_steps.RUN_LENS, 1)


@pytest.mark.parametrize("what", ["group", "class"])
def test_neighbours_of_another_group_or_class_are_not_merged(what, mode):
    n_lanes = 2 if what == "group" else 1
    St, prod = run_and_check(wdp_steps.alternating_batch(what), wdp_steps.RUN_W, wdp_steps.RUN_LENS, n_lanes)
    if what == "group":
        assert [p["bases"][1] for p in prod] == [5000, 5000]
    else:
        assert prod[0]["bases"][1] == prod[0]["bases_low"][1] == 5000 and prod[0]["reads"][1] == 100


@pytest.fixture(scope="module")
def limit():
    """256 read groups (tests/lane_limit.py): groups on both sides of 64, the LDS copy's limit, and the last one; both contigs loaded
    and main, so that the histogram is looked at as well."""
    lens = [lane_limit.REF_LEN] * 2
    batches = [lane_limit.sprinkled(256), lane_limit.ends(256, lane_limit.sprinkled_size(256))] + [lane_limit.solo(256, g) for g in (63, 64, 255)]
    St = wdp_ref.state_fast(synth.concat(batches), 1000, lens, 256)
    prod = wdp_ref.products(St, 1000, lens, [1, 1])
    assert St[63, 0] and St[64, 0] and St[255, 0] and prod[255]["hist"][1:].sum() > 0
    return lens, batches, St, prod


def test_read_groups_63_64_and_255_of_256(limit, mode):
    lens, batches, St, prod = limit
    a = Aggregator(n_lanes=256, n_refs=2, main_chrom=[1, 1], max_read_len=1024, isize=2000, window_depth=(1000, lens))
    for i, r in enumerate(lane_limit.refs()):
        a.set_reference(i, r)
    for b in batches:
        a.submit(b)
    a.finalize()
    check_words(module_words(a, 256, 1000, lens), St)
    check_views(a, prod, 1000, lens)
    a.close()


@pytest.fixture(scope="module")
def groups():
    cols = wdp_steps.groups_batch()
    St = wdp_ref.state_fast(cols, wdp_steps.GROUP_W, wdp_steps.GROUP_LENS, 4)
    return cols, St, wdp_ref.products(St, wdp_steps.GROUP_W, wdp_steps.GROUP_LENS, [0, 0])


def test_sorted_and_shuffled(groups, mode):
    cols, St, prod = groups
    W, lens = wdp_steps.GROUP_W, wdp_steps.GROUP_LENS
    run_and_check(cols, W, lens, 4, St=St)
    perm = np.random.default_rng(9).permutation(len(cols["flag"]))
    run_and_check(lane_limit.take(cols, perm), W, lens, 4, St=St)


# ---------------------------------------------------------------------------------------------------------------------------
# 6. one batch against seven submits
# ---------------------------------------------------------------------------------------------------------------------------
def test_one_batch_against_seven_submits(groups, tmp_path):
    cols, St, prod = groups
    W, lens = wdp_steps.GROUP_W, wdp_steps.GROUP_LENS
    a = context(W, lens, 4)
    for part in split(cols, [1, 3, 6, 906, 1807, 1808]):  # seven pieces
        a.submit(part)
    a.finalize()
    check_words(module_words(a, 4, W, lens), St)
    check_views(a, prod, W, lens)
    out = str(tmp_path / "groups.wdp")  # the text through the library's writer, lanes in an order of the caller's
    a.write_window_depth(out, ["c0", "c1"], "S", ["g2", "g0", "g3", "g1"], [2, 0, 3, 1])
    assert open(out).read() == wdp_ref.text(prod, W, 20, ["c0", "c1"], lens, "S", ["g2", "g0", "g3", "g1"], [2, 0, 3, 1])
    a.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 7. state
# ---------------------------------------------------------------------------------------------------------------------------
def test_export_import_reset_and_place(groups):
    cols, St, prod = groups
    W, lens = wdp_steps.GROUP_W, wdp_steps.GROUP_LENS
    n = len(cols["flag"])
    vec = []
    for part in split(cols, [n // 2]):
        x = context(W, lens, 4)
        x.submit(part)
        vec.append(x.state_export_host())
        x.close()
    wrap = np.zeros_like(vec[0])  # two exports added modulo 2^64: a pair of vectors that only sum to the state past the wrap
    nw = 4 * lane_words(W, lens)
    wrap[-nw:] = np.uint64(1 << 63)
    total = (vec[0] + wrap) + (vec[1] + wrap)  # (uint64: modulo 2^64)
    c = context(W, lens, 4)
    c.state_import_host(total)
    c.finalize()
    check_words(module_words(c, 4, W, lens), St)
    check_views(c, prod, W, lens)
    c.finalize()  # twice: the same views, the same words
    check_views(c, prod, W, lens)
    check_words(module_words(c, 4, W, lens), St)
    c.reset()  # the words go to zero, the tables stay
    assert not module_words(c, 4, W, lens).any()
    with pytest.raises(BamQCError) as e:  # (nothing finalised since the reset)
        c.window_depth(0)
    assert e.value.code == ERR_STATE
    c.reset()
    c.submit(cols)
    c.finalize()
    check_views(c, prod, W, lens)
    # module off, or another NW: another vector
    off = Aggregator(n_lanes=4, n_refs=2, main_chrom=[0, 0], max_read_len=16_384, isize=2000)
    other = context(W, [lens[0], lens[1] + W], 4)
    assert c.state_words - nw == other.state_words - nw - 4 * 3 == off.state_words
    # directly behind the sketch's words, in front of the ten other modules'
    S = 5
    regions = tuple(np.array(x, np.int32) for x in ([0, 1], [0, 0], lens))
    every = context(W, lens, 4, regions=regions, site_alleles=(np.zeros(S, np.int32), np.arange(S, dtype=np.int32)), substitutions=16, indel_by_cycle=16,
                    qual_by_cycle=8, mismatch_by_cycle=8, adapter_by_cycle=8, gc_bias=100, duplicate_sets=1 << 12)
    every.submit(cols)
    check_words(module_words(every, 4, W, lens, front=off.state_words), St)
    rcv = rcv_ref.state_fast(cols, regions, 4, 2)  # the region coverage's words follow directly
    got = every.state_export_host()[off.state_words + nw:off.state_words + nw + rcv.size].reshape(4, -1)
    check_words(got, rcv)
    for x in (c, off, other, every):
        x.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 8. errors
# ---------------------------------------------------------------------------------------------------------------------------
def test_enable_errors(groups):
    cols, St, prod = groups
    base = dict(n_lanes=4, n_refs=2, main_chrom=[0, 0], max_read_len=16_384, isize=2000)
    cases = [(dict(window_depth=(99, [10, 10])), ["window size 99"]),
             (dict(window_depth=((1 << 24) + 1, [10, 10])), ["window size 16777217"]),
             (dict(window_depth=(0, [10, 10])), ["window size 0"]),
             (dict(window_depth=(100, [10, 10]), window_min_mapq=256), ["quality 256"]),
             (dict(window_depth=(100, None)), ["2 contig lengths", "null"]),
             (dict(window_depth=(100, [10, -7])), ["contig 1", "length -7"]),
             (dict(window_depth=(100, [(1 << 31) - 1, 90_000_000])), ["22374837 windows", "of 100 bases", "4 read groups"])]
    for kw, words in cases:
        with pytest.raises(BamQCError) as e:
            Aggregator(**dict(base, **kw))
        assert e.value.code == ERR_ARG and all(w in str(e.value) for w in words), str(e.value)
    a = Aggregator(window_depth=(1 << 24, [(1 << 31) - 1, 0]), window_min_mapq=255, **base)  # (the limits are values; a contig of length 0 is one)
    with pytest.raises(BamQCError) as e:
        a.enable_window_depth(100, [10, 10])
    assert e.value.code == ERR_STATE and "on already" in str(e.value)
    a.finalize()
    assert a.window_depth(0)["n_windows"] == 128 and a.window_depth(3)["woff"].tolist() == [0, 128, 128]
    with pytest.raises(BamQCError) as e:
        a.window_depth(4)
    assert e.value.code == ERR_ARG
    a.close()
    for spoil in ("submit", "export", "finalize"):
        a = Aggregator(**base)
        a.submit(cols) if spoil == "submit" else a.state_export_host() if spoil == "export" else a.finalize()
        with pytest.raises(BamQCError) as e:
            a.enable_window_depth(100, [10, 10])
        assert e.value.code == ERR_STATE, spoil
        if spoil == "finalize":
            with pytest.raises(BamQCError) as e:  # (the module is off)
                a.window_depth(0)
            assert e.value.code == ERR_STATE
        a.close()
    a = Aggregator(window_depth=(100, [10, 10]), **base)
    a.submit(cols)
    with pytest.raises(BamQCError) as e:  # (before finalize: the call itself, Aggregator.window_depth would finalise first)
        a._chk(a.lib.bqc_window_depth(a.h, 0, C.byref(_abi.WdpView())))
    assert e.value.code == ERR_STATE
    a.close()
    off, on = Aggregator(**base), Aggregator(window_depth=(100, [250, 0]), **base)
    assert on.state_words == off.state_words + 4 * (4 + 3 * 3)
    off.close()
    on.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 9. against the region coverage
# ---------------------------------------------------------------------------------------------------------------------------
def test_against_region_coverage(groups):
    """Regions equal to the whole contigs and the same MQ: a region's sum of depths is the contig's sum of `bases`, and the examined
    reads are the good ones."""
    cols, St, prod = groups
    W, lens = wdp_steps.GROUP_W, wdp_steps.GROUP_LENS
    regions = tuple(np.array(x, np.int32) for x in ([0, 1], [0, 0], lens))
    a = context(W, lens, 4, regions=regions, region_min_mapq=20)
    a.submit(cols)
    a.finalize()
    for l in range(4):
        r, w = a.region_coverage(l), a.window_depth(l)
        assert r["regions"][:, 0].tolist() == w["contigs"][:, 1].tolist() and r["regions"][:, 0].sum() > 1000
        assert r["reads_examined"] == w["reads_examined"] > 0
        assert r["aligned_bases"] == int(w["bases"].sum()) + _good_outside(cols, l, lens)  # (A counts the good reads' bases off the contig as well)
    a.close()


def _good_outside(cols, lane, lens):
    """The outside bases of the good reads of a read group (X counts both classes; the region coverage's A only mapq >= 20)."""
    good = dict(cols, mapq=np.where(cols["mapq"] >= 20, cols["mapq"], 0), flag=np.where(cols["mapq"] >= 20, cols["flag"], 0x4).astype(np.uint16))
    return int(wdp_ref.state_fast(good, wdp_steps.GROUP_W, lens, 4)[lane, 2])


# ---------------------------------------------------------------------------------------------------------------------------
# 10. the program
# ---------------------------------------------------------------------------------------------------------------------------
CHROMS = ["-c", "chr1,chr2"]
NAMES, LENS = ["chr1", "chr2"], [400_000, 150_000]


def run(args, env=None, **kw):
    return subprocess.run([EXE] + args, capture_output=True, env=dict(os.environ, **(env or {})), timeout=120, **kw)


def same_bytes(a, b):
    return open(a, "rb").read() == open(b, "rb").read()


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """4000 synthetic paired reads in two read groups, the same reads in a file whose header lists the contigs (and so their lengths)
    the other way round, the `.bamqc` of runs without the option."""
    d = tmp_path_factory.mktemp("wdp")
    bam, fa, swapped = str(d / "in.bam"), str(d / "in.fa"), str(d / "swapped.bam")
    hostio.synth_write(bam, fa, seed=31, n_reads=4000, ref_names=NAMES, ref_lens=LENS, n_lanes=2)
    cols, refs, lanes, sample = pybam.columns(bam)
    assert len(lanes) == 2 and [nm for nm, _ in refs] == NAMES
    cols2 = dict(cols)
    cols2["rid"] = np.where(cols["rid"] >= 0, 1 - cols["rid"], cols["rid"]).astype(np.int32)
    hostio.write_bam(swapped, cols2, NAMES[::-1], LENS[::-1], n_lanes=2)
    bases = {}
    for name, path in (("bam", bam), ("swapped", swapped)):
        bases[name] = str(d / ("base_%s.bamqc" % name))
        r = run(["-r", fa, "-o", bases[name]] + CHROMS + [path])
        assert r.returncode == 0, r.stderr
        assert not os.path.exists(bases[name] + ".wdp")
    names = sorted(lanes)  # the `.bamqc` lists the lanes by name
    idx = [lanes[nm] for nm in names]
    done = {}

    def want(which="bam", W=1000, MQ=20):
        key = (which, W, MQ)
        if key not in done:
            c, nm, ln = (cols, NAMES, LENS) if which == "bam" else (cols2, NAMES[::-1], LENS[::-1])
            St = wdp_ref.state_fast(c, W, ln, 2, MQ)
            prod = wdp_ref.products(St, W, ln, [1, 1])
            assert all(p["reads_examined"] > 500 and p["bases"].sum() > 50_000 and p["hist"].sum() == len(p["bases"]) for p in prod)
            done[key] = wdp_ref.text(prod, W, MQ, nm, ln, sample, names, idx)
        return done[key]
    return dict(dir=d, bam=bam, swapped=swapped, fa=fa, base=bases["bam"], base_swapped=bases["swapped"], want=want, cols=cols)


@pytest.mark.parametrize("decode", ["0", "1"])
def test_program_bam(files, decode):
    out = str(files["dir"] / ("bam%s.bamqc" % decode))
    r = run(["-r", files["fa"], "-o", out, "--window-depth"] + CHROMS + [files["bam"]], env=dict(BQC_GPU_DECODE=decode))
    assert r.returncode == 0, r.stderr
    assert same_bytes(out, files["base"])
    assert open(out + ".wdp").read() == files["want"]()
    assert not os.path.exists(out + ".rcv") and not os.path.exists(out + ".ibc")


def test_program_sam_on_stdin(files):
    out = str(files["dir"] / "sam.bamqc")
    sam = pybam.bam_to_sam_text(files["bam"]).encode()
    r = run(["-r", files["fa"], "-o", out, "--window-depth-size", "999", "--window-depth-min-mapq=0"] + CHROMS + ["-"], input=sam)  # (each implies the option)
    assert r.returncode == 0, r.stderr
    assert same_bytes(out, files["base"])
    assert open(out + ".wdp").read() == files["want"]("bam", 999, 0) != files["want"]()


def test_program_two_workers_on_one_card(files):
    out = str(files["dir"] / "gpus2.bamqc")
    r = run(["--gpus", "2", "-r", files["fa"], "-o", out, "--window-depth", "--indel-by-cycle"] + CHROMS + [files["bam"]], env=dict(BQC_GPUS_SHARE_DEVICE="1"))
    assert r.returncode == 0, r.stderr
    assert same_bytes(out, files["base"])
    assert open(out + ".wdp").read() == files["want"]()
    assert os.path.exists(out + ".ibc")


def test_program_manifest_with_two_headers(files):
    d = files["dir"]
    jobs = [(files["bam"], str(d / "m1.bamqc"), "bam"), (files["swapped"], str(d / "m2.bamqc"), "swapped"), (files["bam"], str(d / "m3.bamqc"), "bam")]
    lst = str(d / "jobs.tsv")
    with open(lst, "w") as f:
        for i, o, _ in jobs:
            f.write("%s\t%s\n" % (i, o))
    r = run(["-r", files["fa"], "--window-depth-size", "100", "--manifest", lst] + CHROMS)
    assert r.returncode == 0, r.stderr
    for i, o, which in jobs:
        assert same_bytes(o, files["base"] if which == "bam" else files["base_swapped"])
        assert open(o + ".wdp").read() == files["want"](which, 100)
    assert files["want"]("bam", 100) != files["want"]("swapped", 100)


def test_program_all_modules(files):
    d = files["dir"]
    ten, eleven = str(d / "ten.bamqc"), str(d / "eleven.bamqc")
    sites, bed = str(d / "sites.tsv"), str(d / "panel.bed")
    with open(sites, "w") as f:
        f.write("".join("chr1\t%d\n" % p for p in range(1000, 3000, 7)))
    with open(bed, "w") as f:
        f.write("".join("chr1\t%d\t%d\n" % (p, p + 300) for p in range(1000, 300_000, 5000)))
    mods = ["--qual-by-cycle", "--mismatch-by-cycle", "--adapter-by-cycle", "--gc-bias", "--indel-by-cycle", "--substitutions", "--site-alleles", sites,
            "--regions", bed, "--duplicate-sets", "--duplicate-sets-capacity", "65536"]
    r = run(["-r", files["fa"], "-o", ten] + mods + CHROMS + [files["bam"]])
    assert r.returncode == 0, r.stderr
    r = run(["-r", files["fa"], "-o", eleven] + mods + ["--window-depth"] + CHROMS + [files["bam"]])
    assert r.returncode == 0, r.stderr
    for ext in ("", ".qbc", ".mbc", ".adp", ".gcb", ".ibc", ".sbc", ".sac", ".rcv", ".dup"):
        assert same_bytes(eleven + ext, ten + ext), ext
    assert same_bytes(eleven, files["base"])
    assert open(eleven + ".wdp").read() == files["want"]()
    assert not os.path.exists(ten + ".wdp")


def test_program_messages(files):
    d = files["dir"]
    never = str(d / "never.bamqc")
    for opt, bad, words in (("--window-depth-size", "99", b"100 to 16777216"), ("--window-depth-size", "16777217", b"100 to 16777216"),
                            ("--window-depth-size", "1k", b"100 to 16777216"), ("--window-depth-min-mapq", "256", b"0 to 255"),
                            ("--window-depth-min-mapq", "abc", b"0 to 255")):
        r = run(["-r", files["fa"], "-o", never, opt, bad] + CHROMS + [files["bam"]])
        assert r.returncode != 0 and words in r.stderr and ("'%s'" % bad).encode() in r.stderr and not os.path.exists(never), r.stderr
    # a header that needs more than 2^28 words: refused before the output is opened
    big = str(d / "big.bam")
    hostio.write_bam(big, files["cols"], NAMES + ["chr3"], [(1 << 31) - 1] * 3, n_lanes=2)
    r = run(["-r", files["fa"], "-o", never, "--window-depth-size", "100"] + CHROMS + [big])
    assert r.returncode != 0 and b"--window-depth-size" in r.stderr and b"64424511 windows" in r.stderr and b"2 read groups" in r.stderr, r.stderr
    assert not os.path.exists(never) and not os.path.exists(never + ".wdp")
    blocked = str(d / "blocked.bamqc")
    os.mkdir(blocked + ".wdp")  # (a directory where the table's file would go)
    r = run(["-r", files["fa"], "-o", blocked, "--window-depth"] + CHROMS + [files["bam"]])
    assert r.returncode == 1
    assert b"Could not write output file" in r.stderr and b".wdp" in r.stderr
