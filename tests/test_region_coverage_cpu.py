"""CPU: the options of --regions in the program's parser, the Python mirror of bqc_rcv_view, the restatement of the statistic
(tests/rcv_ref.py) on reads worked out by hand, its text, its vectorised twin on every batch of tests/test_gpu_region_coverage.py, the
edges those batches are meant to cross, the BED file's reader (hostio.load_regions) and the constants of tests/rcv_steps.py against
the kernel's."""
import ctypes
import os
import re

import numpy as np
import pytest

from bamqc_amd import _abi, _lib, hostio
from tests import rcv_ref, rcv_steps
from tests.rcv_steps import BUCKET, D, EQ, FIRST, I, LAST, M, N_, P, RC_T, RC_TILE, REV, S, X, cols_of, regions_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNEL = open(os.path.join(ROOT, "bamqc_amd", "csrc", "k_rcv.hip")).read()
WALK = open(os.path.join(ROOT, "bamqc_amd", "csrc", "cigar_walk.h")).read()  # (the wave's pass: stated once)


def ask(*args):
    lib = _lib.load()
    argv = (ctypes.c_char_p * (len(args) + 1))(b"bamqualcheck", *[a.encode() for a in args])
    buf = ctypes.create_string_buffer(4096)
    rc = lib.bqc_program_args(len(args) + 1, argv, buf, 4096)
    return rc, buf.value.decode()


def test_parser_knows_the_options(capfd):
    base = ("-r", "g.fa", "-o", "x.bamqc")
    assert ask(*base, "--regions", "panel.bed", "in.bam") == (0, "in.bam")
    assert ask(*base, "--regions=panel.bed", "--regions-min-mapq", "0", "--regions-depth-cap=16383", "--regions-thresholds", "1,2,4294967295", "in.bam") == (0, "in.bam")
    assert ask(*base, "--regions-thresholds=1,2,3,4,5,6,7,8", "--regions", "panel.bed", "--site-alleles", "s.vcf", "--indel-by-cycle", "in.bam") == (0, "in.bam")
    for opt, bads in (("--regions-min-mapq", ("256", "-1", "q", "")), ("--regions-depth-cap", ("0", "16384", "x", "2x")),
                      ("--regions-thresholds", ("0", "1,1", "2,1", "1,,2", "1,", ",1", "4294967296", "1,2,3,4,5,6,7,8,9", "a", ""))):
        for bad in bads:
            assert ask(*base, "--regions", "p.bed", opt, bad, "in.bam")[0] == 1, (opt, bad)
    assert ask(*base, "in.bam", "--regions")[0] == 1  # no value
    ctypes.CDLL(None).fflush(None)
    err = capfd.readouterr().err
    assert "--regions-min-mapq wants 0 to 255" in err and "--regions-depth-cap wants 1 to 16383" in err and "--regions-thresholds wants up to 8 increasing numbers" in err
    for opt, val in (("--regions-min-mapq", "10"), ("--regions-thresholds", "1,5"), ("--regions-depth-cap", "100")):  # a parameter without the regions is a usage error
        assert ask(*base, opt, val, "in.bam")[0] == 1
        ctypes.CDLL(None).fflush(None)
        assert "option %s needs --regions FILE" % opt in capfd.readouterr().err


def test_help_names_the_options(capfd):
    assert ask("--help")[0] == 2
    ctypes.CDLL(None).fflush(None)  # (the library printed through C's stdout)
    out = capfd.readouterr().out
    for opt in ("--regions FILE", "--regions-min-mapq INT", "--regions-thresholds LIST", "--regions-depth-cap INT", "OUT.rcv"):
        assert opt in out, opt


def test_abi_mirror():
    names = [f[0] for f in _abi.RcvView._fields_]
    assert names == ["n_regions", "min_mapq", "n_thresholds", "depth_cap", "rid", "start", "end", "reads_examined", "reads_on_target", "aligned_bases",
                     "bases_on_target", "target_bases", "thresholds", "regions", "hist"]
    p = ctypes.sizeof(ctypes.c_void_p)
    assert ctypes.sizeof(_abi.RcvView) == 16 + 3 * p + 40 + 3 * p and _abi.RcvView.rid.offset == 16 and _abi.RcvView.reads_examined.offset == 16 + 3 * p
    lib = _lib.load()
    for name in ("bqc_enable_region_coverage", "bqc_region_coverage", "bqc_write_region_coverage", "bqc_regions_load", "bqc_regions_free"):
        assert name in _lib._SIGNATURES and getattr(lib, name)
    assert lib.bqc_abi_version() == 2
    assert [f[0] for f in _abi.Options._fields_][-3:] == ["qual_by_cycle", "mismatch_by_cycle", "pad_tail"]
    header = open(os.path.join(ROOT, "include", "bamqc.h")).read()
    for rule in ("flag & 0xF04 == 0", "m = min(n, max(0, l_seq - j))", "lo = max(g, start), hi = min(g + m, end)", "BQC_FLAG_NO_QUAL is NOT looked at",
                 "n_lanes * (B + R + 4) <= 2^28", "n_lanes * (4 + B + R) words directly behind the", "a deletion or a skip covers nothing",
                 "int bqc_region_coverage(bqc_ctx* ctx, uint32_t lane, bqc_rcv_view* out);"):
        assert rule in header, rule


def test_constants_are_the_kernels():
    def define(name):
        return re.search(r"#define %s\s+(\S+)" % name, KERNEL).group(1)
    assert int(define("RC_THREADS")) == rcv_steps.RC_STEP and define("RC_STEP") == "RC_THREADS"
    assert int(define("RC_T")) == RC_T == 8 and 1 << int(define("RC_BUCKET_SHIFT")) == BUCKET == 4096 and int(define("RC_TILE")) == RC_TILE
    assert int(define("RC_POS_MAX").rstrip("l"), 16) == rcv_ref.END_MAX - 1
    assert RC_TILE % int(define("RC_FTHREADS")) == 0 and int(define("RC_HBINS")) == 16384
    assert "p0 += WAVE" in KERNEL and "p0 + WAVE + ln" in WALK and rcv_steps.PASS == 64
    assert "gadd(" in KERNEL and "asm" not in KERNEL and "gadd(" in WALK and "asm" not in WALK
    api = open(os.path.join(ROOT, "bamqc_amd", "csrc", "bqc_api.cpp")).read()
    assert "end[first[r + 1] - 1] >> 12" in api and "k << 12" in api  # (the host builds the index with the kernel's bucket)


# ---------------------------------------------------------------------------------------------------------------------------
# the restatement on reads worked out by hand
# ---------------------------------------------------------------------------------------------------------------------------
REGIONS = regions_of([(0, 100, 110), (0, 110, 120), (0, 200, 205)])  # slots: 0 ... 10, 11 ... 21, 22 ... 27


def one(cigar, pos, L=None, MQ=20, **kw):
    """(E, T, A, {position: depth}) of one read by both restatements and both ways to the depth."""
    r = dict(cigar=cigar, pos=pos, **kw)
    if L is not None:
        r["L"] = L
    cols = cols_of([r])
    St = rcv_ref.state(cols, REGIONS, 1, 1, MQ)
    assert np.array_equal(St, rcv_ref.state_fast(cols, REGIONS, 1, 1, MQ)) and St[0, 3] == 0
    for k in range(3):  # a region's slots sum to 0
        lo, hi = 4 + [0, 11, 22][k], 4 + [11, 22, 28][k]
        assert int(St[0, lo:hi].sum(dtype=np.uint64)) == 0
    pr = rcv_ref.products(St, REGIONS, 1, (1, 2), 3)[0]
    pf = rcv_ref.products_fast(St, REGIONS, 1, (1, 2), 3)[0]
    assert all(np.array_equal(pr[k], pf[k]) for k in pr)
    depth = np.cumsum(St[0, 4:], dtype=np.uint64)
    at = {}
    for k, (s, e, off) in enumerate(((100, 110, 0), (110, 120, 11), (200, 205, 22))):
        for p in range(s, e):
            if depth[off + p - s]:
                at[p] = int(depth[off + p - s])
        assert int(pr["regions"][k][0]) == sum(v for q, v in at.items() if s <= q < e)
    assert pr["bases_on_target"] == sum(at.values()) and pr["target_bases"] == 25 and int(pr["hist"].sum()) == 25
    return int(St[0, 0]), int(St[0, 1]), int(St[0, 2]), at


def span(*ab):
    return {p: 1 for a, b in zip(ab[0::2], ab[1::2]) for p in range(a, b)}


@pytest.mark.parametrize("rev", [0, REV])
def test_worked_out_by_hand(rev):
    f = P | FIRST | rev
    assert one([(10, M)], 100, flag=f) == (1, 1, 10, span(100, 110))
    assert one([(30, M)], 95, flag=f) == (1, 1, 30, span(100, 120))                    # before the first region to behind the second
    assert one([(10, M)], 90, flag=f) == (1, 0, 10, {})                                # ends exactly at a start
    assert one([(10, M)], 120, flag=f) == (1, 0, 10, {})                               # begins exactly at an end
    for gap in (D, N_):
        assert one([(4, M), (12, gap), (6, M)], 100, flag=f) == (1, 1, 10, span(100, 104, 116, 120))
    assert one([(5, M), (3, I), (5, M)], 105, flag=f) == (1, 1, 10, span(105, 115))   # an insertion moves nothing on the genome
    assert one([(6, S), (4, M)], 108, flag=f) == (1, 1, 4, span(108, 112))
    assert one([(4, EQ), (2, X), (4, EQ)], 198, flag=f) == (1, 1, 10, span(200, 205))
    assert one([(30, M)], 100, L=6, flag=f) == (1, 1, 6, span(100, 106))               # the cut at m
    assert one([(4, M), (4, I), (30, M)], 100, L=10, flag=f) == (1, 1, 6, span(100, 106))
    assert one([(4, M), (8, S), (30, M)], 100, L=10, flag=f) == (1, 1, 4, span(100, 104))
    assert one([(6, M)] + [(4, op) for op in range(9, 16)] + [(4, M)], 104, flag=f) == (1, 1, 10, span(104, 114))
    assert one([(50, D), (10, M), (85, N_), (10, M)], 50, flag=f) == (1, 1, 20, span(100, 110, 200, 205))


def test_reads_that_are_not_examined():
    none = (0, 0, 0, {})
    for extra in (0x4, 0x100, 0x200, 0x400, 0x800):
        assert one([(10, M)], 100, flag=P | FIRST | extra) == none
    assert one([(10, M)], 100, mapq=19) == none and one([(10, M)], 100, mapq=20)[0] == 1 and one([(10, M)], 100, mapq=0, MQ=0)[0] == 1
    assert one([(10, M)], 100, mapq=254, MQ=255) == none and one([(10, M)], 100, mapq=255, MQ=255)[0] == 1
    assert one([(10, M)], 100, rid=-1) == none and one([(10, M)], 100, rid=1) == none and one([(10, M)], 100, lane=1) == none
    assert one([(10, M)], 100, flag=P | FIRST | rcv_steps.NO_QUAL)[:3] == (1, 1, 10)  # no qualities stored: it counts
    assert one([(10, M)], 100, flag=P | FIRST | 0x20 | 0x8)[:3] == (1, 1, 10)         # the mate's flags are not looked at
    cols = cols_of([dict(cigar=[(10, M)], pos=100)])
    for key in ("n_cigar", "l_seq"):
        c = dict(cols, **{key: np.zeros(1, cols[key].dtype)})
        c["cigar"] = cols["cigar"][:int(c["n_cigar"][0])]
        assert not rcv_ref.examined(c, 1, 1, 20).any()


def test_what_the_library_refuses_first():
    """The restatement's checks are the enable call's: each list below trips the assertion of rcv_ref.layout."""
    for trip, n_refs in (([], 1), ([(1, 0, 5)], 1), ([(0, -1, 5)], 1), ([(0, 5, 5)], 1), ([(0, 0, 10), (0, 9, 12)], 1), ([(1, 0, 5), (0, 0, 5)], 2)):
        with pytest.raises(AssertionError):
            rcv_ref.layout(tuple(np.array([t[i] for t in trip], np.int32) for i in range(3)), n_refs)  # (as given: not sorted)
    rcv_ref.layout(regions_of([(0, 0, 10), (0, 10, 12), (1, rcv_ref.END_MAX - 5, rcv_ref.END_MAX)]), 2)  # abutting, and the last end there can be
    with pytest.raises(AssertionError):
        rcv_ref.layout(regions_of([(0, 0, (1 << 28) - 4)]), 1)                          # one word more than 2^28
    rcv_ref.layout(regions_of([(0, 0, (1 << 28) - 5)]), 1)


# ---------------------------------------------------------------------------------------------------------------------------
# the step batches: the two restatements agree, and each batch crosses the edge it is named for
# ---------------------------------------------------------------------------------------------------------------------------
def both(cols, regions, n_lanes, n_refs, MQ=20, thresholds=rcv_ref.DEFAULT_THRESHOLDS, Dcap=1000, loop_products=True):
    St = rcv_ref.state_fast(cols, regions, n_lanes, n_refs, MQ)
    assert np.array_equal(St, rcv_ref.state(cols, regions, n_lanes, n_refs, MQ))
    pf = rcv_ref.products_fast(St, regions, n_refs, thresholds, Dcap)
    if loop_products:
        pr = rcv_ref.products(St, regions, n_refs, thresholds, Dcap)
        assert all(np.array_equal(pr[l][k], pf[l][k]) for l in range(n_lanes) for k in pr[l])
    return St, pf


@pytest.mark.parametrize("MQ", [0, 20, 255])
def test_rule_batch(MQ):
    cols, regions = rcv_steps.rule_batch(MQ)
    St, pf = both(cols, regions, 3, rcv_steps.RULE_REFS, MQ)
    ops = set((cols["cigar"] & 15).tolist())
    assert ops == set(range(16)) and 25 <= len(cols["flag"]) // 3 <= 45
    assert (cols["flag"] & rcv_steps.NO_QUAL).any() and (cols["pos"] == 0).any()
    assert all(0 < pf[l]["reads_on_target"] < pf[l]["reads_examined"] for l in range(3))
    assert all(pf[l]["regions"][:, 0].all() for l in range(3))  # every region is covered in every read group


def test_lookup_batch():
    cols, regions = rcv_steps.lookup_batch()
    St, pf = both(cols, regions, 1, rcv_steps.LOOKUP_REFS, loop_products=False)
    rid, start, end = (a.astype(np.int64) for a in regions)
    assert {int(x) % BUCKET for x in np.concatenate([start, end])} >= {0, 1, BUCKET - 1}
    big = int(np.argmax(end - start))
    assert end[big] - start[big] == 1 << 20 and 0 < pf[0]["regions"][big, 0] < 400 and pf[0]["regions"][big, 1] == 0
    assert int(end.max()) == rcv_ref.END_MAX and pf[0]["regions"][np.argmax(end), 2] >= 2  # the last base there can be is covered
    assert 1 not in rid and {0, 2, 3} <= set(rid.tolist()) and (cols["rid"] == 1).any()
    last3 = int(end[rid == 3].max())
    assert ((cols["rid"] == 3) & (cols["pos"] >= last3)).sum() == 2
    assert pf[0]["regions"][:, 0].all()


def test_many_batch():
    cols, regions = rcv_steps.many_batch()
    St, pf = both(cols, regions, 2, 1, loop_products=False)
    assert len(regions[0]) == BUCKET and (regions[2] - regions[1] == 1).all()
    assert (cols["n_cigar"] <= RC_T).sum() == 2 and (cols["n_cigar"] > RC_T).sum() == 2
    for l in range(2):  # one read over all of them, one whose deletion jumps over half of them
        d = pf[l]["regions"][:, 0]
        assert (d == 2).sum() > 1000 and (d == 1).sum() == BUCKET // 2 and (d >= 1).all()


def test_path_batch():
    reads, regions = rcv_steps.path_batch()
    cols = cols_of(reads, 4)
    both(cols, regions, 1, 1, 0, loop_products=False)
    assert sorted(set(cols["n_cigar"].tolist())) == [1, RC_T, RC_T + 1, 64, 65, 129, 1000]


def test_sum_and_seam_batches():
    cols, regions = rcv_steps.groups_batch()
    St, pf = both(cols, regions, 4, 2, loop_products=False)
    assert (St[:, 4:] >= np.uint64(1 << 63)).any() and all(p["reads_on_target"] > 100 for p in pf)
    assert (regions[1][1:] == regions[2][:-1]).any()  # abutting regions
    cols, regions, border = rcv_steps.seam_batch()
    ln = (regions[2] - regions[1]).astype(np.int64)
    assert {1, RC_TILE - 1, RC_TILE, RC_TILE + 1, 3 * RC_TILE + 5} <= set(ln.tolist())
    closing = np.cumsum(ln + 1) - 1
    assert border % RC_TILE == 0 and border - 1 in closing and border + RC_TILE in closing
    St = rcv_ref.state_fast(cols, regions, 2, 1)
    pf = rcv_ref.products_fast(St, regions, 1, (1,), 1)
    B = int(ln.sum())
    assert not St[0].any() and pf[0]["hist"].tolist() == [B, 0] and (pf[0]["regions"][:, 1] == 0).all()
    assert pf[1]["regions"][:, 2].max() >= 40  # depths above small caps


def test_another_list_of_the_same_size_does_not_close():
    cols = rcv_steps.list_batch()
    St = rcv_ref.state(cols, rcv_steps.LIST_A, 1, 1)
    rcv_ref.products(St, rcv_steps.LIST_A, 1)
    for f in (rcv_ref.products, rcv_ref.products_fast):
        with pytest.raises(rcv_ref.NotADifferenceArray) as e:
            f(St, rcv_steps.LIST_B, 1)
        assert e.value.region == 0


def test_text():
    cols = cols_of([dict(cigar=[(30, M)], pos=95), dict(cigar=[(3, M)], pos=201, lane=1)])
    St = rcv_ref.state(cols, REGIONS, 2, 1)
    pr = rcv_ref.products(St, REGIONS, 1, (1, 2), 2)
    got = rcv_ref.text(pr, REGIONS, ["chrA"], 20, (1, 2), "S1", ["b", "a"], [1, 0])
    assert got == ("sample_id S1\nlane b\nregion_min_mapq 20\nregion_reads_examined 1\nregion_reads_on_target 1\nregion_aligned_bases 3\nregion_bases_on_target 3\n"
                   "region_target_bases 25\nregion_depth_thresholds 1 2\nregion_depth_histogram 3 22 3 0\nregions 3\n"
                   "chrA 100 110 0 0 0 0 0\nchrA 110 120 0 0 0 0 0\nchrA 200 205 3 0 1 3 0\n"
                   "sample_id S1\nlane a\nregion_min_mapq 20\nregion_reads_examined 1\nregion_reads_on_target 1\nregion_aligned_bases 30\nregion_bases_on_target 20\n"
                   "region_target_bases 25\nregion_depth_thresholds 1 2\nregion_depth_histogram 3 5 20 0\nregions 3\n"
                   "chrA 100 110 10 1 1 10 0\nchrA 110 120 10 1 1 10 0\nchrA 200 205 0 0 0 0 0\n")


# ---------------------------------------------------------------------------------------------------------------------------
# the BED file
# ---------------------------------------------------------------------------------------------------------------------------
def test_load_regions(tmp_path):
    names, lens = ["chr1", "chr2"], [1000, 500]
    bed = str(tmp_path / "panel.bed")
    with open(bed, "w") as f:
        f.write("#a comment\ntrack name=panel\nbrowser position chr1:1-100\n\n"
                "chr2\t100\t200\tampl1\t0\t+\r\nchr1\t300\t400\nchr1\t10\t20\nchr1\t15\t30\nchr1\t30\t40\nchrUn\t5\t9\nchr1\t50\t60\nchr2\t0\t500\nchr1\t999\t1000\n")
    rid, start, end, given, unnamed, merged = hostio.load_regions(bed, names, lens)
    assert (given, unnamed, merged) == (9, 1, 3)  # 10-20 + 15-30 (overlap) + 30-40 (abutting); chr2 100-200 inside 0-500
    assert rid.dtype == start.dtype == end.dtype == np.int32
    assert list(zip(rid.tolist(), start.tolist(), end.tolist())) == [(0, 10, 40), (0, 50, 60), (0, 300, 400), (0, 999, 1000), (1, 0, 500)]
    rcv_ref.layout((rid, start, end), 2)
    rid2, start2, end2, *_ = hostio.load_regions(bed, names[::-1], lens[::-1])  # another header's numbering
    assert list(zip(rid2.tolist(), start2.tolist(), end2.tolist())) == [(0, 0, 500), (1, 10, 40), (1, 50, 60), (1, 300, 400), (1, 999, 1000)]
    for body, line, words in (("chr1\t5\t9\nchr1 7 9\n", 2, "no tab"), ("chr1\t5\n", 1, "no tab between the start and the end"), ("chr1\t5\t5\n", 1, "does not lie behind"),
                              ("chr1\t9\t5\n", 1, "does not lie behind"), ("chr1\t1\t2\nchr1\t5\t1001\n", 2, "behind the end of contig chr1"),
                              ("chr1\tx\t5\n", 1, "the start 'x' is not a number"), ("chr1\t1\t5x\n", 1, "the end '5x' is not a number"),
                              ("chr1\t-1\t5\n", 1, "is not a number"), ("chrUn\t1\t5\n", 1, "no region left"), ("# nothing\n", 1, "no region left")):
        bad = str(tmp_path / "bad.bed")
        with open(bad, "w") as f:
            f.write(body)
        with pytest.raises(IOError) as e:
            hostio.load_regions(bad, names, lens)
        assert "bad.bed: line %d: " % line in str(e.value) and words in str(e.value), str(e.value)
    with pytest.raises(IOError) as e:
        hostio.load_regions(str(tmp_path / "missing.bed"), names, lens)
    assert "could not be opened" in str(e.value)
