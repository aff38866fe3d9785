"""CPU: the options of --site-alleles in the program's parser, the Python mirror of bqc_sac_view, the restatement of the statistic
(tests/sac_ref.py) on reads worked out by hand, its text, its vectorised twin on every batch of tests/test_gpu_site_alleles.py, the
edges those batches are meant to cross, the sites file's reader (hostio.load_sites) and the launch constants of tests/sac_steps.py
against the kernel's."""
import ctypes
import os
import re

import numpy as np
import pytest

from bamqc_amd import _abi, _lib, hostio
from tests import sac_ref, sac_steps
from tests.sac_steps import D, EQ, FIRST, H, I, LAST, M, N_, P, P_, REV, S, X, cols_of, sites_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNEL = open(os.path.join(ROOT, "bamqc_amd", "csrc", "k_sac.hip")).read()  # (what tests/sac_steps.py restates the constants of)
WALK = open(os.path.join(ROOT, "bamqc_amd", "csrc", "cigar_walk.h")).read()  # (the wave's pass and the launch geometry: stated once)
A, C, G, T = 0, 1, 2, 3


def ask(*args):
    lib = _lib.load()
    argv = (ctypes.c_char_p * (len(args) + 1))(b"bamqualcheck", *[a.encode() for a in args])
    buf = ctypes.create_string_buffer(4096)
    rc = lib.bqc_program_args(len(args) + 1, argv, buf, 4096)
    return rc, buf.value.decode()


def test_parser_knows_the_options(capfd):
    base = ("-r", "g.fa", "-o", "x.bamqc")
    assert ask(*base, "--site-alleles", "sites.vcf", "in.bam") == (0, "in.bam")
    assert ask(*base, "--site-alleles=sites.vcf", "--site-alleles-min-qual", "0", "--site-alleles-min-mapq=255", "in.bam") == (0, "in.bam")
    assert ask(*base, "--site-alleles-min-qual", "222", "--site-alleles", "sites.vcf", "--substitutions", "--indel-by-cycle", "in.bam") == (0, "in.bam")
    for opt, bads in (("--site-alleles-min-qual", ("223", "-1", "x", "", "2x")), ("--site-alleles-min-mapq", ("256", "-1", "q"))):
        for bad in bads:
            assert ask(*base, "--site-alleles", "s.vcf", opt, bad, "in.bam")[0] == 1, (opt, bad)
    assert ask(*base, "in.bam", "--site-alleles")[0] == 1  # no value
    ctypes.CDLL(None).fflush(None)
    err = capfd.readouterr().err
    assert "--site-alleles-min-qual wants 0 to 222" in err and "--site-alleles-min-mapq wants 0 to 255" in err
    for opt in ("--site-alleles-min-qual", "--site-alleles-min-mapq"):  # a threshold without the sites is a usage error
        assert ask(*base, opt, "10", "in.bam")[0] == 1
        ctypes.CDLL(None).fflush(None)
        assert "option %s needs --site-alleles FILE" % opt in capfd.readouterr().err


def test_help_names_the_options(capfd):
    assert ask("--help")[0] == 2
    ctypes.CDLL(None).fflush(None)  # (the library printed through C's stdout)
    out = capfd.readouterr().out
    for opt in ("--site-alleles FILE", "--site-alleles-min-qual INT", "--site-alleles-min-mapq INT", "OUT.sac"):
        assert opt in out, opt


def test_abi_mirror():
    assert [f[0] for f in _abi.SacView._fields_] == ["n_sites", "min_base_qual", "min_mapq", "rid", "pos", "counts"]
    assert ctypes.sizeof(_abi.SacView) == 16 + 3 * ctypes.sizeof(ctypes.c_void_p) and _abi.SacView.rid.offset == 16
    lib = _lib.load()
    for name in ("bqc_enable_site_alleles", "bqc_site_alleles", "bqc_write_site_alleles", "bqc_sites_load", "bqc_sites_free"):
        assert name in _lib._SIGNATURES and getattr(lib, name)
    assert lib.bqc_abi_version() == 2
    assert [f[0] for f in _abi.Options._fields_][-3:] == ["qual_by_cycle", "mismatch_by_cycle", "pad_tail"]
    header = open(os.path.join(ROOT, "include", "bamqc.h")).read()
    for rule in ("flag & 0xF04 == 0", "g <= p < g + n and i = j + (p - g) < l_seq", "T[lane][site][4 s + b] += 1", "Q <= q <= 222", "BOTH count",
                 "n_lanes * S * 8 words directly behind the sketch's words",
                 "int bqc_enable_site_alleles(bqc_ctx* ctx, uint32_t n_sites, const int32_t* rid, const int32_t* pos, uint32_t min_base_qual, uint32_t min_mapq);"):
        assert rule in header, rule


def test_constants_are_the_kernels():
    src = KERNEL

    def define(name):
        return re.search(r"#define %s\s+(\S+)" % name, src).group(1)
    assert int(define("SA_THREADS")) == sac_steps.SA_STEP and define("SA_STEP") == "SA_THREADS"
    assert int(define("SA_T")) == sac_steps.SA_T and 1 << int(define("SA_BUCKET_SHIFT")) == sac_steps.BUCKET
    assert int(define("SA_POS_MAX").rstrip("l"), 16) == sac_steps.POS_MAX == sac_ref.POS_MAX
    assert "share_grid(b.n_reads" in src and "n_reads + 255) / 256" in WALK and sac_steps.WG_READS == 256
    assert "p0 += WAVE" in src and "p0 + WAVE + ln" in WALK and sac_steps.PASS == 64
    assert "gadd(" in src and "asm" not in src and "gadd(" in WALK and "asm" not in WALK


# ---------------------------------------------------------------------------------------------------------------------------
# the restatement on reads worked out by hand
# ---------------------------------------------------------------------------------------------------------------------------
SITES = sites_of([(0, p) for p in (100, 109, 110, 115, 120, 121, 125, 130, 140, 141)])
PATTERN = [1, 2, 4, 8, 1, 2, 4, 8, 1, 2]  # the read's codes: stored index i shows the base (i % 10) % 4


def one(cigar, pos, L=None, Q=20, MQ=20, nib=None, qual=None, **kw):
    """{site position: [(strand, base), ...]} of one read by both restatements."""
    L = sac_steps.query_len(cigar) if L is None else L
    L += L & 1
    r = dict(cigar=cigar, pos=pos, L=L, nib=(PATTERN * (L // 10 + 1))[:L] if nib is None else nib, qual=np.full(L, 40, np.uint8) if qual is None else qual, **kw)
    cols = cols_of([r])
    Tl = sac_ref.table(cols, SITES, 1, 1, Q, MQ)
    assert np.array_equal(Tl, sac_ref.table_fast(cols, SITES, 1, 1, Q, MQ))
    assert Tl.max() <= 1  # (a read adds at most 1 to a site)
    return {int(SITES[1][k]): (int(w) // 4, int(w) % 4) for k, w in np.argwhere(Tl[0])}


@pytest.mark.parametrize("rev", [0, REV])
def test_worked_out_by_hand(rev):
    s = 1 if rev else 0
    f = P | FIRST | rev
    # a site on the first and on the last base of a match run; 110 is one behind it
    assert one([(10, M)], 100, flag=f) == {100: (s, A), 109: (s, C)}
    # 105 ... 108 match, 109 ... 120 lie under the deletion (or the skip), 121 is the first base behind it: stored index 4
    for gap in (D, N_):
        assert one([(4, M), (12, gap), (6, M)], 105, flag=f) == {121: (s, A), 125: (s, A)}
    # beside an insertion: 115 at index 0, then three inserted bases, 120 and 121 at index 8 and 9
    assert one([(5, M), (3, I), (2, M)], 115, flag=f) == {115: (s, A), 120: (s, A), 121: (s, C)}
    # a soft clip lies in front of pos: 115 gets nothing, 120 is stored index 6
    assert one([(6, S), (4, M)], 120, flag=f) == {120: (s, G), 121: (s, T)}
    # H and P move nothing
    assert one([(3, H), (2, P_), (6, M), (2, P_), (4, M), (5, H)], 120, flag=f) == {120: (s, A), 121: (s, C), 125: (s, C)}
    # = and X runs are match runs
    assert one([(4, EQ), (2, X), (4, EQ)], 121, flag=f) == {121: (s, A), 125: (s, A), 130: (s, C)}
    # a CIGAR longer than the read: 125 at index 5 < 6 counts, 130 at index 10 does not
    assert one([(30, M)], 120, L=6, flag=f) == {120: (s, A), 121: (s, C), 125: (s, C)}
    # codes 9 ... 15 do nothing
    assert one([(6, M)] + [(4, op) for op in range(9, 16)] + [(4, M)], 120, flag=f) == {120: (s, A), 121: (s, C), 125: (s, C)}
    # a read that starts in front of the contig
    assert one([(115, M)], -5, flag=f) == {100: (s, C), 109: (s, A)}  # stored index 105 and 114


def test_codes_and_qualities_by_hand():
    # codes 0 (=), 15 (N) and an ambiguity code count nowhere: sites 120, 121, 125 at index 0, 1, 5
    nib = [0, 15, 1, 1, 1, 3, 2, 2, 2, 2]
    assert one([(10, M)], 120, nib=nib) == {}
    nib = [4, 8, 1, 1, 1, 2, 2, 2, 2, 2]
    assert one([(10, M)], 120, nib=nib) == {120: (0, G), 121: (0, T), 125: (0, C)}
    for Q in (20, 1, 222):  # Q - 1, Q and 222 on 120, 121, 125; 223 on 130 never counts
        qual = np.array([Q - 1, Q, 0, 0, 0, 222, 0, 0, 0, 0, 223, 255], np.uint8)
        assert one([(12, M)], 120, Q=Q, qual=qual) == {121: (0, C), 125: (0, C)}
    assert one([(12, M)], 120, Q=0, qual=np.array([0, 222, 0, 0, 0, 223, 0, 0, 0, 0, 255, 0], np.uint8)) == {120: (0, A), 121: (0, C)}


def test_reads_that_are_not_examined():
    hit = {100: (0, A), 109: (0, C)}
    for MQ in (20, 1, 255):
        assert one([(10, M)], 100, MQ=MQ, mapq=MQ - 1) == {} and one([(10, M)], 100, MQ=MQ, mapq=MQ) == hit
    assert one([(10, M)], 100, MQ=0, mapq=0) == hit
    for extra in (0x4, 0x100, 0x200, 0x400, 0x800, 0x8000):  # each excluded flag bit alone; BQC_FLAG_NO_QUAL
        assert one([(10, M)], 100, flag=P | FIRST | extra) == {}
    for extra in (0x2, 0x8, 0x20, 0x40, 0x80, 0x1000, 0x2000, 0x4000):  # the mate flags and the other annotations are not looked at
        assert one([(10, M)], 100, flag=P | extra) == hit
    assert one([(10, M)], 100, flag=0) == hit
    for kw in (dict(rid=-1), dict(rid=1), dict(lane=1)):
        assert one([(10, M)], 100, **kw) == {}
    cols = cols_of([dict(cigar=[], pos=100, L=10), dict(cigar=[(10, M)], pos=100, L=0)])
    assert not sac_ref.table(cols, SITES, 1, 1).any() and not sac_ref.table_fast(cols, SITES, 1, 1).any()


def test_what_the_library_refuses_first():
    """A contig or a read group out of range and a quality of 223 end the batch in the library's checks: the restatement alone says
    what the rule makes of them (tests/sac_steps.py: rule_batch(refused=True))."""
    cols, sites = sac_steps.rule_batch(refused=True)
    plain, _ = sac_steps.rule_batch()
    Tr, Tp = sac_ref.table(cols, sites, 3, 3), sac_ref.table(plain, sites, 3, 3)
    assert np.array_equal(Tr, sac_ref.table_fast(cols, sites, 3, 3))
    k50 = int(np.flatnonzero((sites[0] == 2) & (sites[1] == 50))[0])
    diff = Tr.astype(np.int64) - Tp.astype(np.int64)
    assert diff.sum() == 6 and diff[:, k50].sum() == 6  # only the quality 222 at site 50 counts, once per lane and strand


# ---------------------------------------------------------------------------------------------------------------------------
# the two restatements on every batch, and the edges the batches are meant to cross
# ---------------------------------------------------------------------------------------------------------------------------
CASES = dict(rule=(lambda: sac_steps.rule_batch(), 3, 3, 20, 20), rule0=(lambda: sac_steps.rule_batch(0, 0), 3, 3, 0, 0),
             rule_max=(lambda: sac_steps.rule_batch(222, 255), 3, 3, 222, 255), index=(sac_steps.index_batch, 1, 1, 0, 0),
             region=(sac_steps.region_batch, 2, 1, 0, 0), far=(sac_steps.far_batch, 1, 4, 20, 20), arith=(sac_steps.arith_batch, 1, 1, 0, 0),
             groups=(sac_steps.groups_batch, 4, 2, 20, 20))


@pytest.mark.parametrize("case", sorted(CASES))
def test_the_two_restatements_agree(case):
    make, n_lanes, n_refs, Q, MQ = CASES[case]
    cols, sites = make()
    Tl = sac_ref.table(cols, sites, n_lanes, n_refs, Q, MQ)
    assert np.array_equal(Tl, sac_ref.table_fast(cols, sites, n_lanes, n_refs, Q, MQ)) and Tl.any()


def first_site(sites, rid, pos):
    """(s0, end of the contig's run) as the kernel's look-up defines them."""
    key = sites[0].astype(np.int64) << 32 | sites[1]
    return int(np.searchsorted(key, (rid << 32) | min(max(pos, 0), sac_ref.POS_MAX + 1))), int(np.searchsorted(key, (rid + 1) << 32))


def test_batches_cross_their_edges():
    # hits on the thread path and on the wave path, at every operation count around the limit and the pass
    reads, sites = sac_steps.path_batch()
    assert [len(r["cigar"]) for r in reads[::3]] == sac_steps.PATH_NCIGARS and {sac_steps.SA_T, sac_steps.SA_T + 1, 64, 65, 128, 129, 65_535} <= set(sac_steps.PATH_NCIGARS)
    for r in reads:
        cols = cols_of([r], 1)
        Tl = sac_ref.table(cols, sites, 1, 1, 0, 0)
        assert np.array_equal(Tl, sac_ref.table_fast(cols, sites, 1, 1, 0, 0))
        hit = np.flatnonzero(Tl[0].sum(axis=1))
        span = sac_steps.genome_len(r["cigar"])
        assert len(hit) >= 2 and sites[1][hit[-1]] > r["pos"] + span - 40, len(r["cigar"])  # sites under the operations of the last pass
    # reads rejected by the one-operation shortcut, by the walk, and on the index alone; a read group change inside a step
    cols, sites = sac_steps.groups_batch()
    ok = sac_ref.examined(cols, 4, 2, 20)
    so, qo, co = sac_ref.offsets(cols)
    shortcut = walk = 0
    for r in np.flatnonzero(ok):
        s0, send = first_site(sites, int(cols["rid"][r]), int(cols["pos"][r]))
        assert s0 < send
        w = int(cols["cigar"][co[r]])
        if cols["n_cigar"][r] == 1:
            shortcut += int(sites[1][s0]) >= int(cols["pos"][r]) + min(w >> 4, int(cols["l_seq"][r]))
        else:
            span = sum(int(x) >> 4 for x in cols["cigar"][co[r]:co[r] + int(cols["n_cigar"][r])] if (int(x) & 15) in sac_steps.GENOME_OPS)
            walk += int(sites[1][s0]) >= int(cols["pos"][r]) + span
    assert shortcut > 50 and walk >= 3 and (cols["n_cigar"] > sac_steps.SA_T).sum() > 50
    cols, sites = sac_steps.index_batch()
    assert first_site(sites, 0, 5 * sac_steps.BUCKET)[0] < len(sites[0]) and sac_steps.buckets(sites, 1)[0][:4] == [2, 2, 0, 1]  # 0, 4095 | 4096, 4097 | an empty bucket | 12295
    # a bucket with 4096 sites, empty buckets, a contig without sites between two with sites, S = 1
    cols, sites = sac_steps.region_batch()
    b = sac_steps.buckets(sites, 1)[0]
    assert b[3] == 4096 and b[0] == 1 and b[1] == b[2] == b[4] == b[5] == 0 and b[6] == 1 and len(b) == 7
    cols, sites = sac_steps.rule_batch()
    b = sac_steps.buckets(sites, 3)
    assert b[0] == [10] and b[1] == [] and b[2] == [4, 1] and (cols["rid"] == 1).any()
    cols, sites = sac_steps.far_batch()
    assert len(sites[0]) == 1 and (cols["rid"] > sites[0][0]).any() and (cols["rid"] < sites[0][0]).any()
    # position arithmetic: g passes 2^31 and 2^32 would be passed by a 32-bit sum of three deletions
    cols, sites = sac_steps.arith_batch()
    assert cols["pos"].max() == (1 << 31) - 300 and (cols["cigar"] >> 4).max() == sac_steps.OPMAX and sites[1][-1] == sac_steps.POS_MAX
    # seams: three steps per workgroup on cards of several sizes, the first read-group change on a seam
    for cu in (8, 104, 256, 304):
        lay = sac_steps.step_layout(cu)
        assert min(lay["launch"]["steps"]) >= 3 and lay["launch"]["grid"] == cu and lay["changes"][0] in lay["seams"]
        assert lay["changes"][1] not in lay["seams"] and lay["changes"][2] not in lay["seams"]
    cols, sites = sac_steps.step_batch(sac_steps.step_layout(8))
    Ts = sac_ref.table_fast(cols, sites, 4, 1)
    assert np.array_equal(Ts, sac_ref.table(cols, sites, 4, 1)) and all(Ts[l].sum() > 100 for l in range(4))
    cols, sites = sac_steps.hot_batch(1000)
    assert sac_ref.table_fast(cols, sites, 1, 1)[0, 0].tolist() == [0, 1000, 0, 0, 0, 0, 0, 0]


def test_text():
    cols, sites = sac_steps.rule_batch()
    Tl = sac_ref.table(cols, sites, 3, 3)
    txt = sac_ref.text(Tl, sites, ["c0", "c1", "c2"], 20, 20, "S", ["b", "a"], [1, 0]).split("\n")
    S_ = len(sites[0])
    assert txt[:5] == ["sample_id S", "lane b", "site_allele_min_base_qual 20", "site_allele_min_mapq 20", "site_alleles %d" % S_]
    assert txt[5] == "c0 101 " + " ".join(str(int(x)) for x in Tl[1, 0]) and txt[5 + S_ - 1].startswith("c2 5001 ")
    assert txt[5 + S_:5 + S_ + 2] == ["sample_id S", "lane a"] and len(txt) == 2 * (5 + S_) + 1 and txt[-1] == ""


# ---------------------------------------------------------------------------------------------------------------------------
# the sites file
# ---------------------------------------------------------------------------------------------------------------------------
NAMES, LENS = ["chr1", "chr2", "chr3"], [1000, 500, 2_147_483_647]


def test_load_sites(tmp_path):
    p = str(tmp_path / "sites.vcf")
    with open(p, "wb") as f:
        f.write(b"##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\n\nchr2\t500\trs1\tA\tC\r\nchr1\t10\t.\tG\tT\tmore\tcolumns\r\n\r\nchrY\t7\n"
                b"chr3\t2147483647\nchr1\t1\nchrUn\t99999999999\t.\nchr2\t3\t\nchr1\t1000")  # (no line end behind the last line)
    rid, pos, given, unnamed = hostio.load_sites(p, NAMES, LENS)
    assert rid.dtype == np.int32 and pos.dtype == np.int32
    assert list(zip(rid.tolist(), pos.tolist())) == [(0, 0), (0, 9), (0, 999), (1, 2), (1, 499), (2, 2147483646)]
    assert (given, unnamed) == (8, 2)
    rid2, pos2, _, unnamed2 = hostio.load_sites(p, ["chr2", "chrY"], [500, 10])  # another header: another numbering, other contigs left out
    assert list(zip(rid2.tolist(), pos2.tolist())) == [(0, 2), (0, 499), (1, 6)] and unnamed2 == 5


@pytest.mark.parametrize("body,line,words", [
    (b"chr1\t5\nchr1 7\n", 2, "no tab"),
    (b"#c\nchr1\t0\n", 2, "'0' is not a number of 1 or more"),
    (b"chr1\t5\n\nchr1\t-3\n", 3, "'-3' is not a number"),
    (b"chr1\t12x\n", 1, "'12x' is not a number"),
    (b"chr1\t\n", 1, "'' is not a number"),
    (b"chr1\t5\r\nchr2\t501\r\n", 2, "behind the end of contig chr2 (500 bases)"),
    (b"chr1\t5\nchr2\t7\n# note\nchr1\t5\tagain\n", 4, "chr1:5 is given twice (first on line 1)"),
    (b"# nothing\n\n", 2, "no site left"),
    (b"chrY\t5\nchrM\t6\n", 2, "no site left: all 2 sites lie on contigs the header does not name"),
])
def test_load_sites_errors(tmp_path, body, line, words):
    p = str(tmp_path / "bad.tsv")
    with open(p, "wb") as f:
        f.write(body)
    with pytest.raises(IOError) as e:
        hostio.load_sites(p, NAMES, LENS)
    assert str(e.value).startswith("%s: line %d: " % (p, line)) and words in str(e.value), str(e.value)


def test_load_sites_without_a_file(tmp_path):
    with pytest.raises(IOError) as e:
        hostio.load_sites(str(tmp_path / "none.vcf"), NAMES, LENS)
    assert "none.vcf" in str(e.value) and "could not be opened" in str(e.value)
