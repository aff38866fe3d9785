"""GPU: allele counts at given sites (bqc_enable_site_alleles, --site-alleles; bamqc_amd/csrc/k_sac.hip) against the restatement of the
statistic (tests/sac_ref.py), through the C ABI: the views AND the module's whole block of the exported state, word for word.

The kernel is a join of the read stream against the sorted sites: a thread per read rejects it on its flags, looks its first site up
through an index of buckets of 4096 bases (a binary search inside one bucket) and, for a CIGAR of one match-like operation, compares
that site with the alignment's end; the survivors are listed in LDS and walked by a thread each (at most 8 operations) or by a wave
(64 operations a pass, stored index and genome position from exact 64-bit scans).  The batches (tests/sac_steps.py;
tests/test_site_alleles_cpu.py asserts that they cross those edges) put no read on a main chromosome and load no contig — the genome
is not read — except for the cross-check against the mismatches by cycle.

Restatement only, because the library refuses the batch first: a contig or a read group out of range and a quality of 223."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from bamqc_amd import Aggregator, BamQCError, _abi, hostio
from tests import mbc_ref, pybam, sac_ref, sac_steps, synth
from tests.parity import split
from tests.test_gpu_value_limits import n_cu

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "bin", "bamqualcheck")
ERR_ARG, ERR_STATE = 1, 8


def context(sites, n_lanes, n_refs, Q=20, MQ=20, **more):
    """No contig is main and none is given: the genome is not read."""
    return Aggregator(n_lanes=n_lanes, site_alleles=sites, site_min_qual=Q, site_min_mapq=MQ,
                      **dict(dict(n_refs=n_refs, main_chrom=[0] * n_refs, max_read_len=16_384, isize=2000), **more))


def module_words(a, n_lanes, S, behind=0, front=None):
    """The module's words of the flat state vector: n_lanes x S x 8, `behind` words from its end (or from word `front`)."""
    v = a.state_export_host()
    n = n_lanes * S * 8
    lo = len(v) - behind - n if front is None else front
    return v[lo:lo + n].reshape(n_lanes, S, 8)


def check_words(got, T):
    bad = np.argwhere(got != T)
    assert not len(bad), "%d words differ, first (lane, site, word) = %s: %d != %d" % (len(bad), bad[0].tolist(), got[tuple(bad[0])], T[tuple(bad[0])])


def check_views(a, T):
    for l in range(T.shape[0]):
        got = a.site_alleles(l)
        assert got.shape == (T.shape[1], 2, 4), got.shape
        check_words(got.reshape(1, -1, 8), T[l:l + 1])


def run_and_check(cols, sites, n_lanes, n_refs, Q=20, MQ=20, T=None, **more):
    if T is None:
        T = sac_ref.table_fast(cols, sites, n_lanes, n_refs, Q, MQ)
    a = context(sites, n_lanes, n_refs, Q, MQ, **more)
    a.submit(cols)
    a.finalize()
    check_words(module_words(a, n_lanes, len(sites[0])), T)
    check_views(a, T)
    a.close()
    return T


_made = {}


def made(name, *args):
    """A batch is built once and never changed."""
    if (name, args) not in _made:
        _made[(name, args)] = getattr(sac_steps, name)(*args)
    return _made[(name, args)]


# ---------------------------------------------------------------------------------------------------------------------------
# 1. the rule
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Q,MQ", [(20, 20), (0, 0), (222, 255)])
def test_rule(Q, MQ):
    cols, sites = made("rule_batch", Q, MQ)
    T = sac_ref.table(cols, sites, 3, sac_steps.RULE_REFS, Q, MQ)  # (the loops: this batch is small)
    assert all(T[l, :, 4 * s:4 * s + 4].any() for l in range(3) for s in range(2))
    run_and_check(cols, sites, 3, sac_steps.RULE_REFS, Q, MQ, T=T)


# ---------------------------------------------------------------------------------------------------------------------------
# 2. index edges, 3. a bucket of 4096 sites, 4. S = 1 and contigs behind the last one with sites, 5. position arithmetic
# ---------------------------------------------------------------------------------------------------------------------------
def test_index_edges():
    cols, sites = made("index_batch")
    T = run_and_check(cols, sites, 1, 1, 0, 0)
    assert all(T[0, k].sum() >= 4 for k in (0, 1, 2, 3, 5)) and sites[1][5] == sac_steps.POS_MAX  # every edge site is seen, 2^31 - 2 included
    assert not T[0, 4].any()  # (the site no read reaches: one read ends in front of it, one starts behind the contig's last bucket)


def test_every_position_of_a_bucket():
    cols, sites = made("region_batch")
    T = run_and_check(cols, sites, 2, 1, 0, 0)
    in_bucket = (sites[1] >= 3 * sac_steps.BUCKET) & (sites[1] < 4 * sac_steps.BUCKET)
    per_site = T[0, in_bucket].sum(axis=1)  # two reads across the whole bucket, one with 7 of its sites under a deletion
    assert in_bucket.sum() == 4096 and (per_site == 2).sum() == 4089 and (per_site == 1).sum() == 7 and (T[1, in_bucket].sum(axis=1) >= 1).all()


def test_one_site_and_contigs_behind_it():
    cols, sites = made("far_batch")
    T = run_and_check(cols, sites, 1, 4)
    assert len(sites[0]) == 1 and T.sum() > 0


def test_position_arithmetic_near_2_to_the_31():
    cols, sites = made("arith_batch")
    T = run_and_check(cols, sites, 1, 1, 0, 0)
    assert T[0, -1].sum() == 4 and T[0, 0].sum() == 2  # the site at 2^31 - 2: two reads on either path; the read from 0 on either path


# ---------------------------------------------------------------------------------------------------------------------------
# 6. CIGAR lengths: thread path against wave path
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def paths():
    reads, sites = sac_steps.path_batch()
    cols = sac_steps.cols_of(reads, 6)
    return reads, sites, cols, sac_ref.table_fast(cols, sites, 1, 1, 0, 0)


def test_paths_mixed_in_one_step(paths):
    reads, sites, cols, T = paths
    run_and_check(cols, sites, 1, 1, 0, 0, T=T, max_read_len=262_144)
    assert T[0, -40:].any() and T[0, :40].any()  # sites under the first and under the last passes of the longest CIGAR


def test_paths_each_read_alone(paths):
    """Every read of the mixed batch alone in a batch of its own, into one context: the same table."""
    reads, sites, cols, T = paths
    a = context(sites, 1, 1, 0, 0, max_read_len=262_144)
    for k in range(len(reads)):
        a.submit(sac_steps.cols_of(reads[k:k + 1], 100 + k))
    a.finalize()
    want = np.zeros_like(T)  # (a read alone draws other bases than in the mixed batch: the sum of the single restatements)
    for k in range(len(reads)):
        want += sac_ref.table_fast(sac_steps.cols_of(reads[k:k + 1], 100 + k), sites, 1, 1, 0, 0)
    assert want[0, -40:].any() and want.sum() > 1000
    check_words(module_words(a, 1, len(sites[0])), want)
    check_views(a, want)
    a.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 7. contention
# ---------------------------------------------------------------------------------------------------------------------------
def test_70000_reads_on_one_site():
    n = 70_000
    cols, sites = sac_steps.hot_batch(n)
    a = context(sites, 1, 1)
    a.submit(cols)
    a.finalize()
    want = np.zeros((1, 2, 4), np.uint64)
    want[0, 0, 1] = n  # stored index 5 of ACGTACGT...: C, forward
    assert np.array_equal(a.site_alleles(0), want)
    assert module_words(a, 1, 1).sum() == n
    a.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 8. seams and read groups
# ---------------------------------------------------------------------------------------------------------------------------
def test_three_steps_per_workgroup():
    cu = n_cu()
    lay = sac_steps.step_layout(cu)
    la = lay["launch"]
    assert min(la["steps"]) >= 3 and la["grid"] == cu and lay["changes"][0] in lay["seams"]
    cols, sites = sac_steps.step_batch(lay)
    T = sac_ref.table_fast(cols, sites, 4, 1)
    assert all(T[l].sum() > 1000 for l in range(4))
    run_and_check(cols, sites, 4, 1, T=T)


@pytest.fixture(scope="module")
def groups():
    cols, sites = sac_steps.groups_batch()
    return cols, sites, sac_ref.table_fast(cols, sites, 4, 2)


def test_read_groups_one_batch_and_three(groups, tmp_path):
    cols, sites, T = groups
    assert all(T[l, :, 4 * s:4 * s + 4].any() for l in range(4) for s in range(2))
    run_and_check(cols, sites, 4, 2, T=T)
    b = context(sites, 4, 2)
    for part in split(cols, [7, 1300]):  # (the first batch is smaller than one step)
        b.submit(part)
    b.finalize()
    check_words(module_words(b, 4, len(sites[0])), T)
    check_views(b, T)
    out = str(tmp_path / "groups.sac")  # the text through the library's writer, lanes in an order of the caller's
    b.write_site_alleles(out, ["c0", "c1"], "S", ["g2", "g0", "g3", "g1"], [2, 0, 3, 1])
    assert open(out).read() == sac_ref.text(T, sites, ["c0", "c1"], 20, 20, "S", ["g2", "g0", "g3", "g1"], [2, 0, 3, 1])
    b.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 9. order independence
# ---------------------------------------------------------------------------------------------------------------------------
def test_order_independence(groups):
    cols, sites, T = groups
    n = len(cols["flag"])
    perm = np.random.default_rng(9).permutation(n)
    shuffled = synth.concat([synth.slice_batch(cols, int(i), int(i) + 1) for i in perm])
    assert np.array_equal(sac_ref.table_fast(shuffled, sites, 4, 2), T)
    run_and_check(shuffled, sites, 4, 2, T=T)
    a = context(sites, 4, 2)
    for part in split(shuffled, [1, 3, 6, 906, 1807]):  # pieces of 1, 2, 3, 900, 901 and the rest
        a.submit(part)
    check_words(module_words(a, 4, len(sites[0])), T)
    a.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 10. pure sums
# ---------------------------------------------------------------------------------------------------------------------------
def test_sums_reset_and_import(groups):
    cols, sites, T = groups
    S = len(sites[0])
    a = context(sites, 4, 2)
    a.submit(cols)
    a.submit(cols)
    check_words(module_words(a, 4, S), 2 * T)
    a.reset()  # the table goes to zero, the sites stay
    assert not module_words(a, 4, S).any()
    a.reset()  # (the export closed the context for batches)
    a.submit(cols)
    vec = a.state_export_host()
    check_words(module_words(a, 4, S), T)
    c = context(sites, 4, 2)
    c.state_import_host(vec)
    c.finalize()
    check_views(c, T)
    assert np.array_equal(c.state_export_host(), vec)
    a.finalize()
    check_views(a, T)
    a.reset()
    with pytest.raises(BamQCError) as e:  # (nothing finalised since the reset)
        a.site_alleles(0)
    assert e.value.code == ERR_STATE
    # another number of sites, or the module off: another vector, which the import does not take
    fewer = (sites[0][:-1], sites[1][:-1])
    other = context(fewer, 4, 2)
    off = Aggregator(n_lanes=4, n_refs=2, main_chrom=[0, 0], max_read_len=16_384, isize=2000)
    assert a.state_words - 4 * S * 8 == other.state_words - 4 * (S - 1) * 8 == off.state_words
    for x in (other, off):
        with pytest.raises(AssertionError):
            x.state_import_host(vec)
    # directly behind the sketch's words, in front of every other module's
    every = context(sites, 4, 2, substitutions=16, indel_by_cycle=16, qual_by_cycle=8)
    every.submit(cols)
    check_words(module_words(every, 4, S, front=off.state_words), T)
    for x in (a, c, other, off, every):
        x.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 11. the enable call
# ---------------------------------------------------------------------------------------------------------------------------
def test_enable_errors(groups):
    cols, sites, T = groups
    base = dict(n_lanes=4, n_refs=2, main_chrom=[0, 0], max_read_len=16_384, isize=2000)
    i32 = lambda x: np.array(x, np.int32)
    big = (1 << 24) // 4 + 1
    cases = [((i32([]), i32([])), {}, ["0 sites"]),
             ((np.zeros(big, np.int32), np.arange(big, dtype=np.int32)), {}, [str(big), "4 read groups"]),
             ((i32([0, 0, 2]), i32([1, 2, 3])), {}, ["site 2", "contig 2"]),
             ((i32([0, -1]), i32([1, 2])), {}, ["site 1", "contig -1"]),
             ((i32([0, 0, 1, 1]), i32([1, 2, 3, -5])), {}, ["site 3", "position -5"]),
             ((i32([0, 0]), i32([1, (1 << 31) - 1])), {}, ["site 1", "position 2147483647"]),
             ((i32([0, 0, 0, 0]), i32([1, 2, 5, 5])), {}, ["site 3", "position 5"]),
             ((i32([0, 1, 0]), i32([1, 2, 3])), {}, ["site 2"]),
             ((i32([0]), i32([1])), dict(site_min_qual=223), ["223"]),
             ((i32([0]), i32([1])), dict(site_min_mapq=256), ["256"])]
    for s, kw, words in cases:
        with pytest.raises(BamQCError) as e:
            Aggregator(site_alleles=s, **dict(base, **kw))
        assert e.value.code == ERR_ARG and all(w in str(e.value) for w in words), str(e.value)
    a = Aggregator(site_alleles=(i32([0, 1]), i32([0, (1 << 31) - 2])), site_min_qual=222, site_min_mapq=255, **base)  # (the limits themselves are values)
    with pytest.raises(BamQCError) as e:
        a.enable_site_alleles(i32([0]), i32([1]))
    assert e.value.code == ERR_STATE
    a.finalize()
    with pytest.raises(BamQCError) as e:
        a.site_alleles(4)
    assert e.value.code == ERR_ARG
    a.close()
    a = Aggregator(**base)
    a.submit(cols)
    with pytest.raises(BamQCError) as e:  # (the context has taken a batch)
        a.enable_site_alleles(i32([0]), i32([1]))
    assert e.value.code == ERR_STATE
    a.finalize()
    with pytest.raises(BamQCError) as e:  # (the module is off)
        a.site_alleles(0)
    assert e.value.code == ERR_STATE
    a.close()
    a = Aggregator(**base)
    a.state_export_host()
    with pytest.raises(BamQCError) as e:  # (state has been exchanged)
        a.enable_site_alleles(i32([0]), i32([1]))
    assert e.value.code == ERR_STATE
    a.close()
    a = Aggregator(**base)
    a.finalize()
    with pytest.raises(BamQCError) as e:  # (finalised)
        a.enable_site_alleles(i32([0]), i32([1]))
    assert e.value.code == ERR_STATE
    a.close()
    a = Aggregator(site_alleles=(i32([0]), i32([1])), **base)
    a.submit(cols)
    with pytest.raises(BamQCError) as e:  # (before finalize: the call itself, Aggregator.site_alleles would finalise first)
        a._chk(a.lib.bqc_site_alleles(a.h, 0, C.byref(_abi.SacView())))
    assert e.value.code == ERR_STATE
    a.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 12. against the mismatches by cycle
# ---------------------------------------------------------------------------------------------------------------------------
def test_against_mismatch_by_cycle():
    """Reads without duplicates, QC-fail reads, N or ambiguity codes on a loaded contig without N; every position of the contig a site;
    Q = 0, MQ = 0: the sum of the counts is the `.mbc`'s aligned bases, the counts whose base differs from the contig's its mismatches."""
    from tests.long_layout import dna_ref, flags, reads_on_ref
    from tests.sbc_steps import QUALS, plant
    rng = np.random.default_rng(12)
    n, N, n_ref = 1500, 1024, 20_000
    ref = dna_ref(91, n_ref)
    L = rng.choice([16, 40, 150, 255, 256, 300, 700], n)
    cols = reads_on_ref(ref, np.sort(rng.integers(0, n_ref - 701, n)), L, flags(rng.random(n) < 0.5, rng.random(n) < 0.5), QUALS[rng.integers(0, len(QUALS), int(L.sum()))],
                        lane=np.arange(n) % 3)
    plant(cols, rng, 0.05)
    sites = (np.zeros(n_ref, np.int32), np.arange(n_ref, dtype=np.int32))
    a = Aggregator(n_lanes=3, n_refs=1, max_read_len=4096, isize=2000, mismatch_by_cycle=N, site_alleles=sites, site_min_qual=0, site_min_mapq=0)
    a.set_reference(0, ref)
    a.submit(cols)
    a.finalize()
    T = sac_ref.table_fast(cols, sites, 3, 1, 0, 0)
    n_m = 3 * 2 * 2 * N * 224
    check_words(module_words(a, 3, n_ref, behind=n_m), T)
    v = a.state_export_host()
    Mb = v[len(v) - n_m:].reshape(3, 2, 2, N, 224)
    assert np.array_equal(Mb, mbc_ref.table_fast(cols, [ref], 3, N))
    differs = np.arange(4)[None, :] != ref[:, None]  # [site][base]
    for l in range(3):
        got = a.site_alleles(l)
        assert int(got.sum()) == int(Mb[l, :, 0].sum()) > 0
        assert int(got[:, 0][differs].sum() + got[:, 1][differs].sum()) == int(Mb[l, :, 1].sum()) > 0
    a.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 13 - 18. the program
# ---------------------------------------------------------------------------------------------------------------------------
CHROMS = ["-c", "chr1,chr2"]
NAMES, LENS = ["chr1", "chr2"], [400_000, 150_000]


def run(args, env=None, **kw):
    return subprocess.run([EXE] + args, capture_output=True, env=dict(os.environ, **(env or {})), timeout=120, **kw)


def same_bytes(a, b):
    return open(a, "rb").read() == open(b, "rb").read()


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """4000 synthetic paired reads in two read groups, the same reads in a file whose header lists the contigs the other way round,
    a VCF-shaped sites file with sites on a contig neither header names, the `.bamqc` of runs without the option, the expected texts."""
    d = tmp_path_factory.mktemp("sac")
    bam, fa, swapped = str(d / "in.bam"), str(d / "in.fa"), str(d / "swapped.bam")
    hostio.synth_write(bam, fa, seed=31, n_reads=4000, ref_names=NAMES, ref_lens=LENS, n_lanes=2)
    cols, refs, lanes, sample = pybam.columns(bam)
    assert len(lanes) == 2 and [nm for nm, _ in refs] == NAMES
    cols2 = dict(cols)  # the same records in the same order under a header that numbers the contigs the other way round
    cols2["rid"] = np.where(cols["rid"] >= 0, 1 - cols["rid"], cols["rid"]).astype(np.int32)
    assert (cols["rid"] == 0).sum() > 100 and (cols["rid"] == 1).sum() > 100
    hostio.write_bam(swapped, cols2, NAMES[::-1], LENS[::-1], n_lanes=2)
    rng = np.random.default_rng(32)
    vcf = str(d / "sites.vcf")
    with open(vcf, "w") as f:
        f.write("##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\n\n")
        lines = ["chr2\t%d\trs%d\tA\tC" % (p + 1, p) for p in rng.choice(LENS[1], 600, replace=False)]
        lines += ["chr1\t%d\t.\tG\tT\t50\tPASS" % (p + 1) for p in rng.choice(LENS[0], 1500, replace=False)]
        lines += ["chrY\t%d\t.\tG\tT" % p for p in (5, 9, 1000)]
        f.write("\r\n".join(lines) + "\r\n")
    bases = {}
    for name, path in (("bam", bam), ("swapped", swapped)):
        bases[name] = str(d / ("base_%s.bamqc" % name))
        r = run(["-r", fa, "-o", bases[name]] + CHROMS + [path])
        assert r.returncode == 0, r.stderr
        assert not os.path.exists(bases[name] + ".sac")
    names = sorted(lanes)  # the `.bamqc` lists the lanes by name
    idx = [lanes[nm] for nm in names]
    done = {}

    def want(which="bam", Q=20, MQ=20):
        if (which, Q, MQ) not in done:
            c, nm, ln = (cols, NAMES, LENS) if which == "bam" else (cols2, NAMES[::-1], LENS[::-1])
            srid, spos, given, unnamed = hostio.load_sites(vcf, nm, ln)
            assert (given, unnamed, len(srid)) == (2103, 3, 2100)
            T = sac_ref.table_fast(c, (srid, spos), 2, 2, Q, MQ)
            assert all(T[l, :, 4 * s:4 * s + 4].sum() > 50 for l in range(2) for s in range(2))
            done[(which, Q, MQ)] = sac_ref.text(T, (srid, spos), nm, Q, MQ, sample, names, idx)
        return done[(which, Q, MQ)]
    return dict(dir=d, bam=bam, swapped=swapped, fa=fa, vcf=vcf, base=bases["bam"], base_swapped=bases["swapped"], want=want)


@pytest.mark.parametrize("decode", ["0", "1"])
def test_program_bam(files, decode):
    out = str(files["dir"] / ("bam%s.bamqc" % decode))
    r = run(["-r", files["fa"], "-o", out, "--site-alleles", files["vcf"]] + CHROMS + [files["bam"]], env=dict(BQC_GPU_DECODE=decode))
    assert r.returncode == 0, r.stderr
    assert same_bytes(out, files["base"])
    assert open(out + ".sac").read() == files["want"]()
    assert not os.path.exists(out + ".sbc") and not os.path.exists(out + ".ibc")


def test_program_sam_on_stdin(files):
    out = str(files["dir"] / "sam.bamqc")
    sam = pybam.bam_to_sam_text(files["bam"]).encode()
    r = run(["-r", files["fa"], "-o", out, "--site-alleles", files["vcf"], "--site-alleles-min-qual", "30", "--site-alleles-min-mapq", "0"] + CHROMS + ["-"], input=sam)
    assert r.returncode == 0, r.stderr
    assert same_bytes(out, files["base"])
    assert open(out + ".sac").read() == files["want"]("bam", 30, 0) != files["want"]()


def test_program_two_workers_on_one_card(files):
    out = str(files["dir"] / "gpus2.bamqc")
    r = run(["--gpus", "2", "-r", files["fa"], "-o", out, "--site-alleles", files["vcf"], "--indel-by-cycle"] + CHROMS + [files["bam"]], env=dict(BQC_GPUS_SHARE_DEVICE="1"))
    assert r.returncode == 0, r.stderr
    assert same_bytes(out, files["base"])
    assert open(out + ".sac").read() == files["want"]()
    assert os.path.exists(out + ".ibc")
    assert r.stderr.count(b"lie on contigs the header does not name") == 1


def test_program_manifest_with_two_contig_orders(files):
    """Two files whose headers list the contigs in different order (and the first one again) through one resident worker: the sites
    are mapped to every job's header, and each job's `.sac` is its single run's."""
    d = files["dir"]
    single = str(d / "single_swapped.bamqc")
    r = run(["-r", files["fa"], "-o", single, "--site-alleles", files["vcf"]] + CHROMS + [files["swapped"]])
    assert r.returncode == 0, r.stderr
    assert open(single + ".sac").read() == files["want"]("swapped")
    jobs = [(files["bam"], str(d / "m1.bamqc"), "bam"), (files["swapped"], str(d / "m2.bamqc"), "swapped"), (files["bam"], str(d / "m3.bamqc"), "bam")]
    lst = str(d / "jobs.tsv")
    with open(lst, "w") as f:
        for i, o, _ in jobs:
            f.write("%s\t%s\n" % (i, o))
    r = run(["-r", files["fa"], "--site-alleles", files["vcf"], "--manifest", lst] + CHROMS)
    assert r.returncode == 0, r.stderr
    for i, o, which in jobs:
        assert same_bytes(o, files["base"] if which == "bam" else files["base_swapped"])
        assert open(o + ".sac").read() == files["want"](which)
    assert same_bytes(jobs[1][1] + ".sac", single + ".sac")
    assert files["want"]("bam") != files["want"]("swapped")


def test_program_all_seven_modules(files):
    d = files["dir"]
    six, seven = str(d / "six.bamqc"), str(d / "seven.bamqc")
    mods = ["--qual-by-cycle", "--mismatch-by-cycle", "--adapter-by-cycle", "--gc-bias", "--indel-by-cycle", "--substitutions"]
    r = run(["-r", files["fa"], "-o", six] + mods + CHROMS + [files["bam"]])
    assert r.returncode == 0, r.stderr
    r = run(["-r", files["fa"], "-o", seven] + mods + ["--site-alleles", files["vcf"]] + CHROMS + [files["bam"]])
    assert r.returncode == 0, r.stderr
    for ext in ("", ".qbc", ".mbc", ".adp", ".gcb", ".ibc", ".sbc"):
        assert same_bytes(seven + ext, six + ext), ext
    assert same_bytes(seven, files["base"])
    assert open(seven + ".sac").read() == files["want"]()


def test_program_messages(files):
    d = files["dir"]
    out = str(d / "msg.bamqc")
    r = run(["-r", files["fa"], "-o", out, "--site-alleles", files["vcf"]] + CHROMS + [files["bam"]])
    assert r.returncode == 0
    assert ("bamqualcheck: 3 of 2103 sites of %s lie on contigs the header does not name\n" % files["vcf"]).encode() in r.stderr
    never = str(d / "never.bamqc")
    for opt, val in (("--site-alleles-min-qual", "10"), ("--site-alleles-min-mapq", "10")):  # a threshold without the sites
        r = run(["-r", files["fa"], "-o", never, opt, val] + CHROMS + [files["bam"]])
        assert r.returncode != 0 and b"needs --site-alleles" in r.stderr and opt.encode() in r.stderr, r.stderr
    for opt, bad, words in (("--site-alleles-min-qual", "223", b"0 to 222"), ("--site-alleles-min-mapq", "256", b"0 to 255"), ("--site-alleles-min-qual", "x", b"is not a base quality")):
        r = run(["-r", files["fa"], "-o", never, "--site-alleles", files["vcf"], opt, bad] + CHROMS + [files["bam"]])
        assert r.returncode != 0 and words in r.stderr, r.stderr
    r = run(["-r", files["fa"], "-o", never, "--site-alleles"] + CHROMS)
    assert r.returncode != 0
    broken = str(d / "broken.tsv")
    with open(broken, "w") as f:
        f.write("chr1\t5\nchr1 7\n")
    r = run(["-r", files["fa"], "-o", never, "--site-alleles", broken] + CHROMS + [files["bam"]])
    assert r.returncode != 0 and b"broken.tsv: line 2" in r.stderr and not os.path.exists(never + ".sac"), r.stderr
    blocked = str(d / "blocked.bamqc")
    os.mkdir(blocked + ".sac")  # (a directory where the table's file would go)
    r = run(["-r", files["fa"], "-o", blocked, "--site-alleles", files["vcf"]] + CHROMS + [files["bam"]])
    assert r.returncode == 1
    assert b"Could not write output file" in r.stderr and b".sac" in r.stderr
