"""GPU: depth over given regions (bqc_enable_region_coverage, --regions; bamqc_amd/csrc/k_rcv.hip) against the restatement of the
statistic (tests/rcv_ref.py), through the C ABI: the module's whole block of the exported state, word for word, AND the views that
k_rcv_final makes of it.

k_rcv walks every examined read's CIGAR (a thread for at most 8 operations, a wave beyond), looks the first region of a run of covered
bases up through an index of buckets of 4096 bases over the regions' ends, and adds +1 / -1 to the difference words; k_rcv_final takes
the prefix sum over tiles of RC_TILE slots and folds it by region.  The batches (tests/rcv_steps.py; tests/test_region_coverage_cpu.py
asserts that they cross those edges) put no read on a main chromosome and load no contig: the genome is not read."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from bamqc_amd import Aggregator, BamQCError, _abi, hostio
from tests import pybam, rcv_ref, rcv_steps, synth
from tests.parity import split
from tests.rcv_steps import cols_of, regions_of

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "bin", "bamqualcheck")
ERR_ARG, ERR_STATE = 1, 8
THR = rcv_ref.DEFAULT_THRESHOLDS


def context(regions, n_lanes, n_refs, MQ=20, thresholds=THR, D=1000, **more):
    """No contig is main and none is given: the genome is not read."""
    return Aggregator(n_lanes=n_lanes, regions=regions, region_min_mapq=MQ, region_thresholds=thresholds, region_depth_cap=D,
                      **dict(dict(n_refs=n_refs, main_chrom=[0] * n_refs, max_read_len=16_384, isize=2000), **more))


def lane_words(regions):
    return 4 + int((regions[2].astype(np.int64) - regions[1]).sum()) + len(regions[0])


def module_words(a, n_lanes, regions, behind=0, front=None):
    """The module's words of the flat state vector: n_lanes x (4 + B + R), `behind` words from its end (or from word `front`)."""
    v = a.state_export_host()
    n = n_lanes * lane_words(regions)
    lo = len(v) - behind - n if front is None else front
    return v[lo:lo + n].reshape(n_lanes, -1)


def check_words(got, St):
    assert got.shape == St.shape, (got.shape, St.shape)
    bad = np.argwhere(got != St)
    assert not len(bad), "%d words differ, first (lane, word) = %s: %d != %d" % (len(bad), bad[0].tolist(), got[tuple(bad[0])], St[tuple(bad[0])])


def check_views(a, prod):
    for l, want in enumerate(prod):
        got = a.region_coverage(l)
        for key in ("reads_examined", "reads_on_target", "aligned_bases", "bases_on_target", "target_bases"):
            assert got[key] == want[key], (l, key, got[key], want[key])
        for key in ("regions", "hist"):
            assert got[key].shape == want[key].shape, (key, got[key].shape, want[key].shape)
            bad = np.argwhere(got[key] != want[key])
            assert not len(bad), "lane %d %s: %d entries differ, first %s: %d != %d" % (l, key, len(bad), bad[0].tolist(), got[key][tuple(bad[0])], want[key][tuple(bad[0])])


def run_and_check(cols, regions, n_lanes, n_refs, MQ=20, St=None, thresholds=THR, D=1000, **more):
    if St is None:
        St = rcv_ref.state_fast(cols, regions, n_lanes, n_refs, MQ)
    a = context(regions, n_lanes, n_refs, MQ, thresholds, D, **more)
    a.submit(cols)
    a.finalize()
    check_words(module_words(a, n_lanes, regions), St)
    prod = rcv_ref.products_fast(St, regions, n_refs, thresholds, D)
    check_views(a, prod)
    check_words(module_words(a, n_lanes, regions), St)  # (finalize left the difference words as they were)
    a.close()
    return St, prod


# ---------------------------------------------------------------------------------------------------------------------------
# 1. the rule
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("MQ", [0, 20, 255])
def test_rule(MQ):
    cols, regions = rcv_steps.rule_batch(MQ)
    St = rcv_ref.state(cols, regions, 3, rcv_steps.RULE_REFS, MQ)  # (the loops: this batch is small)
    St, prod = run_and_check(cols, regions, 3, rcv_steps.RULE_REFS, MQ, St=St)
    loops = rcv_ref.products(St, regions, rcv_steps.RULE_REFS)
    assert all(np.array_equal(loops[l][k], prod[l][k]) for l in range(3) for k in loops[l])
    assert all(0 < p["reads_on_target"] < p["reads_examined"] and p["regions"][:, 0].all() for p in prod)


# ---------------------------------------------------------------------------------------------------------------------------
# 2. lookup edges, 3. many regions under one operation
# ---------------------------------------------------------------------------------------------------------------------------
def test_lookup_edges():
    cols, regions = rcv_steps.lookup_batch()
    St, prod = run_and_check(cols, regions, 1, rcv_steps.LOOKUP_REFS, 0, max_read_len=32_768)
    assert prod[0]["regions"][:, 0].all() and int(regions[2].max()) == rcv_ref.END_MAX


def test_many_regions_under_one_operation():
    cols, regions = rcv_steps.many_batch()
    St, prod = run_and_check(cols, regions, 2, 1)
    assert all((p["regions"][:, 0] >= 1).all() and (p["regions"][:, 0] == 1).sum() == rcv_steps.BUCKET // 2 for p in prod)


# ---------------------------------------------------------------------------------------------------------------------------
# 4. CIGAR lengths: thread path against wave path
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def paths():
    reads, regions = rcv_steps.path_batch()
    cols = cols_of(reads, 4)
    return reads, regions, cols, rcv_ref.state_fast(cols, regions, 1, 1, 0)


def test_paths_mixed_in_one_step(paths):
    reads, regions, cols, St = paths
    run_and_check(cols, regions, 1, 1, 0, St=St)
    assert St[0, -40:].any() and St[0, 4:44].any()  # regions under the first and under the last passes of the longest CIGAR


def test_paths_each_read_alone(paths):
    """Every read of the mixed batch alone in a batch of its own, into one context: the same words."""
    reads, regions, cols, St = paths
    a = context(regions, 1, 1, 0)
    for k in range(len(reads)):
        a.submit(cols_of(reads[k:k + 1], 100 + k))
    a.finalize()
    check_words(module_words(a, 1, regions), St)
    check_views(a, rcv_ref.products_fast(St, regions, 1))
    a.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 5. contention
# ---------------------------------------------------------------------------------------------------------------------------
def test_20000_reads_on_one_region():
    n = 20_000
    cols, regions = rcv_steps.hot_batch(n)
    a = context(regions, 2, 1, D=16383)
    a.submit(cols)
    a.finalize()
    got = module_words(a, 2, regions)
    want = np.zeros((2, 4 + 101), np.uint64)
    want[:, 0] = want[:, 1] = n // 2
    want[:, 2] = n // 2 * 60
    want[:, 4 + 80] = n // 2                      # the reads begin at 480 ...
    want[:, 4 + 100] = (1 << 64) - n // 2         # ... and leave the region at its end: the closing slot
    check_words(got, want)
    for l in range(2):
        v = a.region_coverage(l)
        assert v["regions"].tolist() == [[20 * (n // 2), 0, n // 2] + [20] * 6] and v["bases_on_target"] == 20 * (n // 2)
        assert v["hist"][0] == 80 and v["hist"][n // 2] == 20 and v["hist"].sum() == 100
    a.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 6. sums
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def groups():
    cols, regions = rcv_steps.groups_batch()
    St = rcv_ref.state_fast(cols, regions, 4, 2)
    return cols, regions, St, rcv_ref.products_fast(St, regions, 2)


def test_one_batch_against_seven_shuffled(groups, tmp_path):
    cols, regions, St, prod = groups
    run_and_check(cols, regions, 4, 2, St=St)
    n = len(cols["flag"])
    perm = np.random.default_rng(9).permutation(n)
    shuffled = synth.concat([synth.slice_batch(cols, int(i), int(i) + 1) for i in perm])
    a = context(regions, 4, 2)
    for part in split(shuffled, [1, 3, 6, 906, 1807, 1808]):  # seven pieces
        a.submit(part)
    a.finalize()
    check_words(module_words(a, 4, regions), St)
    check_views(a, prod)
    out = str(tmp_path / "groups.rcv")  # the text through the library's writer, lanes in an order of the caller's
    a.write_region_coverage(out, ["c0", "c1"], "S", ["g2", "g0", "g3", "g1"], [2, 0, 3, 1])
    assert open(out).read() == rcv_ref.text(prod, regions, ["c0", "c1"], 20, THR, "S", ["g2", "g0", "g3", "g1"], [2, 0, 3, 1])
    a.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 7. finalize seams
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def seam():
    cols, regions, border = rcv_steps.seam_batch()
    return cols, regions, rcv_ref.state_fast(cols, regions, 2, 1)


@pytest.mark.parametrize("thresholds,D", [((1,), 1), ((1, (1 << 32) - 1), 7), ((1, 2, 3, 5, 8, 13, 21, 40), 30)])
def test_finalize_seams(seam, thresholds, D):
    cols, regions, St = seam
    a = context(regions, 2, 1, 20, thresholds, D)
    a.submit(cols)
    a.finalize()
    prod = rcv_ref.products_fast(St, regions, 1, thresholds, D)
    B = prod[0]["target_bases"]
    assert prod[0]["hist"][0] == B and (prod[0]["regions"][:, 1] == 0).all() and prod[1]["hist"][D] > 0 and prod[1]["regions"][:, 2].max() > D
    check_views(a, prod)
    a.finalize()  # twice: the same views, the same words
    check_views(a, prod)
    check_words(module_words(a, 2, regions), St)
    a.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 8. export / import
# ---------------------------------------------------------------------------------------------------------------------------
def test_export_import_and_reset(groups):
    cols, regions, St, prod = groups
    n = len(cols["flag"])
    halves = split(cols, [n // 2])
    vec = []
    for part in halves:
        x = context(regions, 4, 2)
        x.submit(part)
        vec.append(x.state_export_host())
        x.close()
    total = vec[0] + vec[1]  # (uint64: modulo 2^64)
    W = 4 * lane_words(regions)
    assert (vec[0][-W:] >= np.uint64(1 << 63)).any() and (vec[1][-W:] >= np.uint64(1 << 63)).any()  # the wrap is exercised
    c = context(regions, 4, 2)
    c.state_import_host(total)
    c.finalize()
    check_words(module_words(c, 4, regions), St)
    check_views(c, prod)
    c.reset()  # the words go to zero, the regions stay
    assert not module_words(c, 4, regions).any()
    with pytest.raises(BamQCError) as e:  # (nothing finalised since the reset)
        c.region_coverage(0)
    assert e.value.code == ERR_STATE
    c.reset()
    c.submit(cols)
    c.finalize()
    check_views(c, prod)
    # module off, or another B + R: another vector
    off = Aggregator(n_lanes=4, n_refs=2, main_chrom=[0, 0], max_read_len=16_384, isize=2000)
    fewer = tuple(a[:-1] for a in regions)
    other = context(fewer, 4, 2)
    assert c.state_words - W == other.state_words - 4 * lane_words(fewer) == off.state_words
    # directly behind the sketch's words, in front of every other module's
    S = 5
    every = context(regions, 4, 2, site_alleles=(np.zeros(S, np.int32), np.arange(S, dtype=np.int32)), substitutions=16, indel_by_cycle=16, qual_by_cycle=8)
    every.submit(cols)
    check_words(module_words(every, 4, regions, front=off.state_words), St)
    for x in (c, off, other, every):
        x.close()


def test_words_of_another_list_do_not_close():
    cols = rcv_steps.list_batch()
    a = context(rcv_steps.LIST_A, 1, 1)
    a.submit(cols)
    vec = a.state_export_host()
    a.finalize()
    a.close()
    with pytest.raises(rcv_ref.NotADifferenceArray):
        rcv_ref.products_fast(rcv_ref.state(cols, rcv_steps.LIST_A, 1, 1), rcv_steps.LIST_B, 1)
    b = context(rcv_steps.LIST_B, 1, 1)
    assert b.state_words == len(vec)
    b.state_import_host(vec)
    with pytest.raises(BamQCError) as e:
        b.finalize()
    assert e.value.code == ERR_STATE and "region 0 " in str(e.value), str(e.value)
    b.close()


def test_enable_errors(groups):
    cols, regions, St, prod = groups
    base = dict(n_lanes=4, n_refs=2, main_chrom=[0, 0], max_read_len=16_384, isize=2000)
    i32 = lambda x: np.array(x, np.int32)
    one = (i32([0]), i32([1]), i32([5]))
    cases = [((i32([]), i32([]), i32([])), {}, ["0 regions"]),
             ((i32([0, 0, 2]), i32([1, 5, 9]), i32([2, 6, 10])), {}, ["region 2", "contig 2"]),
             ((i32([0, -1]), i32([1, 5]), i32([2, 6])), {}, ["region 1", "contig -1"]),
             ((i32([0, 1]), i32([1, -5]), i32([2, 6])), {}, ["region 1", "start -5"]),
             ((i32([0, 0]), i32([1, 7]), i32([2, 7])), {}, ["region 1", "end 7"]),
             ((i32([0, 0, 0]), i32([1, 5, 8]), i32([4, 9, 12])), {}, ["region 2", "start 8"]),
             ((i32([0, 1, 0]), i32([1, 5, 8]), i32([4, 9, 12])), {}, ["region 2"]),
             ((i32([0]), i32([0]), i32([(1 << 26) - 4])), {}, ["67108860 bases", "4 read groups"]),
             (one, dict(region_min_mapq=256), ["256"]),
             (one, dict(region_depth_cap=0), ["cap 0"]),
             (one, dict(region_depth_cap=16384), ["cap 16384"]),
             (one, dict(region_thresholds=(0,)), ["threshold 0", " 0 is outside"]),
             (one, dict(region_thresholds=(1, 1 << 32)), ["threshold 1", "4294967296"]),
             (one, dict(region_thresholds=(5, 5)), ["threshold 1", "not above"]),
             (one, dict(region_thresholds=tuple(range(1, 10))), ["9 depth thresholds"])]
    for r, kw, words in cases:
        with pytest.raises(BamQCError) as e:
            Aggregator(regions=r, **dict(base, **kw))
        assert e.value.code == ERR_ARG and all(w in str(e.value) for w in words), str(e.value)
    a = Aggregator(regions=(i32([0, 0, 1]), i32([0, 4, (1 << 31) - 2]), i32([4, 9, (1 << 31) - 1])), region_min_mapq=255, region_depth_cap=16383, **base)  # (the limits are values; abutting is allowed)
    with pytest.raises(BamQCError) as e:
        a.enable_region_coverage(*one)
    assert e.value.code == ERR_STATE
    a.finalize()
    with pytest.raises(BamQCError) as e:
        a.region_coverage(4)
    assert e.value.code == ERR_ARG
    a.close()
    for spoil in ("submit", "export", "finalize"):
        a = Aggregator(**base)
        a.submit(cols) if spoil == "submit" else a.state_export_host() if spoil == "export" else a.finalize()
        with pytest.raises(BamQCError) as e:
            a.enable_region_coverage(*one)
        assert e.value.code == ERR_STATE, spoil
        if spoil == "finalize":
            with pytest.raises(BamQCError) as e:  # (the module is off)
                a.region_coverage(0)
            assert e.value.code == ERR_STATE
        a.close()
    a = Aggregator(regions=one, **base)
    a.submit(cols)
    with pytest.raises(BamQCError) as e:  # (before finalize: the call itself, Aggregator.region_coverage would finalise first)
        a._chk(a.lib.bqc_region_coverage(a.h, 0, C.byref(_abi.RcvView())))
    assert e.value.code == ERR_STATE
    a.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 9. against the site alleles
# ---------------------------------------------------------------------------------------------------------------------------
def test_against_site_alleles():
    """Reads of A, C, G, T only with qualities of at most 222; the sites are every position of the regions, Q = 0, the same MQ: the depth
    at p is the sum of the eight counts at p."""
    cols, regions = rcv_steps.groups_batch(seed=45, n=1500, n_lanes=3)
    pos = np.concatenate([np.arange(s, e) for s, e in zip(regions[1], regions[2])]).astype(np.int32)
    rid = np.repeat(regions[0], regions[2] - regions[1]).astype(np.int32)
    a = context(regions, 3, 2, 20, site_alleles=(rid, pos), site_min_qual=0, site_min_mapq=20)
    a.submit(cols)
    a.finalize()
    St = rcv_ref.state_fast(cols, regions, 3, 2)
    check_words(module_words(a, 3, regions, behind=3 * len(pos) * 8), St)
    inside = np.ones(St.shape[1] - 4, bool)
    inside[np.cumsum(regions[2].astype(np.int64) - regions[1] + 1) - 1] = False
    for l in range(3):
        depth = np.cumsum(St[l, 4:], dtype=np.uint64)[inside]
        counts = a.site_alleles(l).reshape(len(pos), 8).sum(axis=1)
        assert np.array_equal(depth, counts) and depth.sum() > 1000
        assert a.region_coverage(l)["bases_on_target"] == int(counts.sum())
    a.close()


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
    """4000 synthetic paired reads in two read groups, the same reads in a file whose header lists the contigs the other way round, a BED
    file with regions that overlap and abut and regions on a contig neither header names, the `.bamqc` of runs without the option."""
    d = tmp_path_factory.mktemp("rcv")
    bam, fa, swapped = str(d / "in.bam"), str(d / "in.fa"), str(d / "swapped.bam")
    hostio.synth_write(bam, fa, seed=31, n_reads=4000, ref_names=NAMES, ref_lens=LENS, n_lanes=2)
    cols, refs, lanes, sample = pybam.columns(bam)
    assert len(lanes) == 2 and [nm for nm, _ in refs] == NAMES
    cols2 = dict(cols)
    cols2["rid"] = np.where(cols["rid"] >= 0, 1 - cols["rid"], cols["rid"]).astype(np.int32)
    hostio.write_bam(swapped, cols2, NAMES[::-1], LENS[::-1], n_lanes=2)
    rng = np.random.default_rng(33)
    bed = str(d / "panel.bed")
    with open(bed, "w") as f:
        f.write("track name=panel\n#a comment\n\n")
        lines = ["chr2\t%d\t%d\tampl%d" % (p, p + 120, p) for p in rng.choice(LENS[1] // 400, 150, replace=False) * 400]
        lines += ["chr1\t%d\t%d" % (p, p + int(rng.integers(1, 700))) for p in rng.choice(LENS[0] // 1000, 200, replace=False) * 1000]
        lines += ["chr1\t1000\t1300", "chr1\t1300\t1400", "chr1\t1350\t1500"]  # (1000 may be among the draws: merged all the same)
        lines += ["chrY\t%d\t%d" % (p, p + 10) for p in (5, 90, 1000)]
        f.write("\r\n".join(lines) + "\r\n")
    bases = {}
    for name, path in (("bam", bam), ("swapped", swapped)):
        bases[name] = str(d / ("base_%s.bamqc" % name))
        r = run(["-r", fa, "-o", bases[name]] + CHROMS + [path])
        assert r.returncode == 0, r.stderr
        assert not os.path.exists(bases[name] + ".rcv")
    names = sorted(lanes)  # the `.bamqc` lists the lanes by name
    idx = [lanes[nm] for nm in names]
    done = {}

    def want(which="bam", MQ=20, thresholds=THR, D=1000):
        key = (which, MQ, thresholds, D)
        if key not in done:
            c, nm, ln = (cols, NAMES, LENS) if which == "bam" else (cols2, NAMES[::-1], LENS[::-1])
            rid, start, end, given, unnamed, merged = hostio.load_regions(bed, nm, ln)
            assert (given, unnamed) == (356, 3) and merged >= 2 and len(rid) == 353 - merged
            St = rcv_ref.state_fast(c, (rid, start, end), 2, 2, MQ)
            prod = rcv_ref.products_fast(St, (rid, start, end), 2, thresholds, D)
            assert all(p["reads_on_target"] > 50 for p in prod)
            done[key] = rcv_ref.text(prod, (rid, start, end), nm, MQ, thresholds, sample, names, idx)
        return done[key]
    return dict(dir=d, bam=bam, swapped=swapped, fa=fa, bed=bed, base=bases["bam"], base_swapped=bases["swapped"], want=want)


@pytest.mark.parametrize("decode", ["0", "1"])
def test_program_bam(files, decode):
    out = str(files["dir"] / ("bam%s.bamqc" % decode))
    r = run(["-r", files["fa"], "-o", out, "--regions", files["bed"]] + CHROMS + [files["bam"]], env=dict(BQC_GPU_DECODE=decode))
    assert r.returncode == 0, r.stderr
    assert same_bytes(out, files["base"])
    assert open(out + ".rcv").read() == files["want"]()
    assert not os.path.exists(out + ".sac") and not os.path.exists(out + ".ibc")
    assert b"3 of 356 regions" in r.stderr and b"overlap or abut their predecessor and were merged" in r.stderr


def test_program_sam_on_stdin(files):
    out = str(files["dir"] / "sam.bamqc")
    sam = pybam.bam_to_sam_text(files["bam"]).encode()
    r = run(["-r", files["fa"], "-o", out, "--regions", files["bed"], "--regions-min-mapq", "0", "--regions-thresholds", "1,3", "--regions-depth-cap", "4"] + CHROMS + ["-"], input=sam)
    assert r.returncode == 0, r.stderr
    assert same_bytes(out, files["base"])
    assert open(out + ".rcv").read() == files["want"]("bam", 0, (1, 3), 4) != files["want"]()


def test_program_two_workers_on_one_card(files):
    out = str(files["dir"] / "gpus2.bamqc")
    r = run(["--gpus", "2", "-r", files["fa"], "-o", out, "--regions", files["bed"], "--indel-by-cycle"] + CHROMS + [files["bam"]], env=dict(BQC_GPUS_SHARE_DEVICE="1"))
    assert r.returncode == 0, r.stderr
    assert same_bytes(out, files["base"])
    assert open(out + ".rcv").read() == files["want"]()
    assert os.path.exists(out + ".ibc")
    assert r.stderr.count(b"lie on contigs the header does not name") == 1


def test_program_manifest_with_two_contig_orders(files):
    d = files["dir"]
    jobs = [(files["bam"], str(d / "m1.bamqc"), "bam"), (files["swapped"], str(d / "m2.bamqc"), "swapped"), (files["bam"], str(d / "m3.bamqc"), "bam")]
    lst = str(d / "jobs.tsv")
    with open(lst, "w") as f:
        for i, o, _ in jobs:
            f.write("%s\t%s\n" % (i, o))
    r = run(["-r", files["fa"], "--regions", files["bed"], "--manifest", lst] + CHROMS)
    assert r.returncode == 0, r.stderr
    for i, o, which in jobs:
        assert same_bytes(o, files["base"] if which == "bam" else files["base_swapped"])
        assert open(o + ".rcv").read() == files["want"](which)
    assert files["want"]("bam") != files["want"]("swapped")


def test_program_all_eight_modules(files):
    d = files["dir"]
    seven, eight = str(d / "seven.bamqc"), str(d / "eight.bamqc")
    sites = str(d / "sites.tsv")
    with open(sites, "w") as f:
        f.write("".join("chr1\t%d\n" % p for p in range(1000, 3000, 7)))
    mods = ["--qual-by-cycle", "--mismatch-by-cycle", "--adapter-by-cycle", "--gc-bias", "--indel-by-cycle", "--substitutions", "--site-alleles", sites]
    r = run(["-r", files["fa"], "-o", seven] + mods + CHROMS + [files["bam"]])
    assert r.returncode == 0, r.stderr
    r = run(["-r", files["fa"], "-o", eight] + mods + ["--regions", files["bed"]] + CHROMS + [files["bam"]])
    assert r.returncode == 0, r.stderr
    for ext in ("", ".qbc", ".mbc", ".adp", ".gcb", ".ibc", ".sbc", ".sac"):
        assert same_bytes(eight + ext, seven + ext), ext
    assert same_bytes(eight, files["base"])
    assert open(eight + ".rcv").read() == files["want"]()


def test_program_messages(files):
    d = files["dir"]
    never = str(d / "never.bamqc")
    for opt, val in (("--regions-min-mapq", "10"), ("--regions-thresholds", "1,2"), ("--regions-depth-cap", "10")):  # a parameter without the regions
        r = run(["-r", files["fa"], "-o", never, opt, val] + CHROMS + [files["bam"]])
        assert r.returncode != 0 and b"needs --regions" in r.stderr and opt.encode() in r.stderr, r.stderr
    for opt, bad, words in (("--regions-min-mapq", "256", b"0 to 255"), ("--regions-depth-cap", "0", b"1 to 16383"), ("--regions-thresholds", "3,2", b"is not a list of depths")):
        r = run(["-r", files["fa"], "-o", never, "--regions", files["bed"], opt, bad] + CHROMS + [files["bam"]])
        assert r.returncode != 0 and words in r.stderr, r.stderr
    broken = str(d / "broken.bed")
    with open(broken, "w") as f:
        f.write("chr1\t5\t9\nchr1\t7\t7\n")
    r = run(["-r", files["fa"], "-o", never, "--regions", broken] + CHROMS + [files["bam"]])
    assert r.returncode != 0 and b"broken.bed: line 2" in r.stderr and not os.path.exists(never + ".rcv"), r.stderr
    blocked = str(d / "blocked.bamqc")
    os.mkdir(blocked + ".rcv")  # (a directory where the table's file would go)
    r = run(["-r", files["fa"], "-o", blocked, "--regions", files["bed"]] + CHROMS + [files["bam"]])
    assert r.returncode == 1
    assert b"Could not write output file" in r.stderr and b".rcv" in r.stderr


def test_module_off_changes_nothing():
    base = dict(n_lanes=2, n_refs=2, main_chrom=[0, 0], max_read_len=16_384, isize=2000)
    off = Aggregator(**base)
    S = 3
    sac = Aggregator(site_alleles=(np.zeros(S, np.int32), np.arange(S, dtype=np.int32)), **base)
    both = Aggregator(site_alleles=(np.zeros(S, np.int32), np.arange(S, dtype=np.int32)), regions=regions_of([(0, 5, 9)]), **base)
    assert sac.state_words == off.state_words + 2 * S * 8 and both.state_words == sac.state_words + 2 * (4 + 4 + 1)
    for x in (off, sac, both):
        x.close()
