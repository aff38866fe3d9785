"""CPU: the options of the GC bias in the program's parser, the Python mirror of bqc_gcb_view, the restatement of the statistic
(tests/gcb_ref.py) on windows and reads worked out by hand, its text, its vectorised twin, the reciprocals the kernels divide with,
and the launch constants of tests/gcb_steps.py against the kernel's."""
import ctypes
import os
import re

import numpy as np

from bamqc_amd import _abi, _lib
from tests import gcb_ref, gcb_steps
from tests.gcb_steps import FIRST, LAST, MAIN, P, REV, cols_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A, C, G, T, N = 0, 1, 2, 3, 4


def ask(*args):
    lib = _lib.load()
    argv = (ctypes.c_char_p * (len(args) + 1))(b"bamqualcheck", *[a.encode() for a in args])
    buf = ctypes.create_string_buffer(4096)
    rc = lib.bqc_program_args(len(args) + 1, argv, buf, 4096)
    return rc, buf.value.decode()


def test_parser_knows_the_options(capfd):
    base = ("-r", "g.fa", "-o", "x.bamqc")
    assert ask(*base, "--gc-bias", "in.bam") == (0, "in.bam")
    assert ask(*base, "--gc-bias-window", "50", "in.bam") == (0, "in.bam")
    assert ask(*base, "--gc-bias-window=1000", "--gc-bias", "in.bam") == (0, "in.bam")
    assert ask(*base, "--gc-bias-window", "20", "--qual-by-cycle", "--mismatch-by-cycle", "--adapter-by-cycle", "in.bam") == (0, "in.bam")
    assert ask("-r", "g.fa", "--gc-bias", "--manifest", os.devnull)[0] in (0, 1)  # (an empty list is the list's matter, not the option's)
    for bad in ("19", "1001", "0", "-20", "x", "100x", "", "1e2"):
        assert ask(*base, "--gc-bias-window", bad, "in.bam")[0] == 1, bad
    assert ask(*base, "in.bam", "--gc-bias-window")[0] == 1  # no value
    capfd.readouterr()
    assert ask(*base, "--gpus", "2", "--gc-bias", "in.bam")[0] == 1
    assert ask(*base, "--gc-bias-window", "50", "--gpus", "2", "in.bam")[0] == 1
    ctypes.CDLL(None).fflush(None)
    err = capfd.readouterr().err
    assert err.count("--gc-bias with --gpus is not supported") == 2, err


def test_help_names_the_options(capfd):
    assert ask("--help")[0] == 2
    ctypes.CDLL(None).fflush(None)  # (the library printed through C's stdout)
    out = capfd.readouterr().out
    for opt in ("--gc-bias\n", "--gc-bias-window INT", "OUT.gcb", "Not with --gpus"):
        assert opt in out, opt


def test_abi_mirror():
    assert [f[0] for f in _abi.GcbView._fields_] == ["window", "n_bins", "genome_windows", "read_starts", "bases", "qual_sum"]
    assert ctypes.sizeof(_abi.GcbView) == 8 + 4 * ctypes.sizeof(ctypes.c_void_p) and _abi.GcbView.genome_windows.offset == 8
    lib = _lib.load()
    for name in ("bqc_enable_gc_bias", "bqc_gc_bias", "bqc_write_gc_bias"):
        assert name in _lib._SIGNATURES and getattr(lib, name)
    # bqc_options, bqc_modules and the ABI version are what they were
    assert lib.bqc_abi_version() == 2
    assert [f[0] for f in _abi.Options._fields_][-3:] == ["qual_by_cycle", "mismatch_by_cycle", "pad_tail"]
    assert _abi.Options.mismatch_by_cycle.offset + 8 == ctypes.sizeof(_abi.Options)
    assert [f[0] for f in _abi.Modules._fields_] == ["struct_size", "adapter_by_cycle", "n_adapters", "pad", "adapters"]
    assert ctypes.sizeof(_abi.Modules) == 16 + ctypes.sizeof(ctypes.c_void_p)
    header = open(os.path.join(ROOT, "include", "bamqc.h")).read()
    for rule in ("g = floor(100 * gc / (W - n))", "flag & 0x904 == 0", "s = end - W", "n_lanes * 3 * 101 words", "int bqc_enable_gc_bias(bqc_ctx* ctx, uint32_t window);"):
        assert rule in header, rule


def test_genome_windows_worked_out_by_hand():
    c40 = np.array([C] * 25 + [G] * 15 + [A] * 30 + [T] * 30, np.uint8)
    g = gcb_ref.genome([c40], 100)
    assert g[40] == 1 and g.sum() == 1
    w20 = np.array([N] * 4 + [C] * 5 + [G] * 3 + [A] * 8, np.uint8)  # 8 of 16 counted bases
    g = gcb_ref.genome([w20], 20)
    assert g[50] == 1 and g.sum() == 1
    g = gcb_ref.genome([np.array([N] * 5 + [C] * 15, np.uint8)], 20)  # five N: no bin
    assert g.sum() == 0
    assert gcb_ref.genome([np.full(99, C, np.uint8)], 100).sum() == 0 and gcb_ref.genome([np.full(19, C, np.uint8)], 20).sum() == 0
    assert gcb_ref.genome([None, np.full(22, G, np.uint8), None], 20)[100] == 3  # contigs not given add nothing
    # sliding over a run of five N: the windows that hold all five have no bin
    ref = np.array([A] * 30 + [N] * 5 + [C] * 30, np.uint8)
    g, fast = gcb_ref.genome([ref], 20), gcb_ref.table_fast([], [ref], 1, 20)[0]
    assert np.array_equal(g, fast) and g.sum() == len(ref) - 19 - 16  # starts 15 .. 30 hold the whole run
    four = np.array([A] * 30 + [N] * 4 + [C] * 30, np.uint8)
    assert gcb_ref.genome([four], 20).sum() == len(four) - 19


REF200 = np.array([A] * 100 + [C] * 100, np.uint8)  # W = 20: the window at s has max(0, s - 80) C for s <= 100, then 20


def tables(reads, refs=(REF200,), n_lanes=1, W=20):
    cols = cols_of(reads)
    g, t = gcb_ref.table(cols, list(refs), n_lanes, W)
    g2, t2 = gcb_ref.table_fast(cols, list(refs), n_lanes, W)
    assert np.array_equal(g, g2) and np.array_equal(t, t2)
    return t


def hits(t, row=0, lane=0):
    return {int(g): int(t[lane, row, g]) for g in np.flatnonzero(t[lane, row])}


def test_reads_worked_out_by_hand():
    cig = [(50, 0), (2, 2), (48, 0)]  # 50M2D48M: 98 bases over 100 of the genome
    t = tables([dict(pos=90, cigar=cig, qual=30)])
    assert hits(t) == {50: 1} and hits(t, 1) == {50: 98} and hits(t, 2) == {50: 98 * 30}        # forward: s = 90, ten C of 20
    t = tables([dict(pos=90, cigar=cig, qual=30, flag=P | FIRST | REV)])
    assert hits(t) == {100: 1} and hits(t, 1) == {100: 98}                                       # reverse: end = 190, s = 170
    t = tables([dict(pos=75, cigar=[(3, 4), (10, 0), (7, 3), (2, 1), (8, 7), (4, 8), (5, 5)], flag=P | LAST | REV)])
    assert hits(t) == {20: 1} and hits(t, 1) == {20: 27}                                         # M, N, =, X: end = 104, s = 84, four C
    # the contig's ends: s = 0 and s + W = len are counted, s = -1 and s + W = len + 1 are not
    fw = [dict(pos=p, cigar=[(30, 0)]) for p in (-1, 0, 180, 181)]
    assert hits(tables(fw)) == {0: 1, 100: 1}
    rv = [dict(pos=p, cigar=[(n, 0)], flag=P | FIRST | REV) for p, n in ((0, 19), (0, 20), (150, 50), (150, 51))]
    assert hits(tables(rv)) == {0: 1, 100: 1}
    # a read shorter than the window still has a window of W genome bases; a read longer than the contig's rest too
    assert hits(tables([dict(pos=95, cigar=[(1, 0)])])) == {75: 1}
    assert hits(tables([dict(pos=180, cigar=[(500, 0)])])) == {100: 1}


def test_which_reads_are_examined():
    one = [(30, 0)]
    not_examined = [dict(pos=0, cigar=one, flag=P | FIRST | 0x4), dict(pos=0, cigar=one, flag=P | FIRST | 0x100), dict(pos=0, cigar=one, flag=P | FIRST | 0x800),
                    dict(pos=0, cigar=[], L=30), dict(pos=0, cigar=one, rid=-1), dict(pos=0, cigar=one, rid=1), dict(pos=0, cigar=one, rid=2),
                    dict(pos=0, cigar=one, lane=1)]
    assert tables(not_examined, refs=(REF200, None)).sum() == 0
    examined = [dict(pos=0, cigar=one, flag=P | FIRST | 0x400), dict(pos=0, cigar=one, flag=P | LAST | 0x200), dict(pos=0, cigar=one, flag=0),
                dict(pos=0, cigar=one, flag=REV), dict(pos=0, cigar=one, flag=P | FIRST | LAST | MAIN)]
    t = tables(examined, refs=(REF200, None))
    assert hits(t) == {0: 5} and hits(t, 1) == {0: 150} and hits(t, 2) == {0: 150 * 30}
    # a read without qualities enters R only; quality bytes count as stored, 0 .. 255
    t = tables([dict(pos=100, cigar=one, qual=None), dict(pos=100, cigar=[(3, 0)], qual=[0, 255, 254])])
    assert hits(t) == {100: 2} and hits(t, 1) == {100: 3} and hits(t, 2) == {100: 509}
    # read groups, and two batches add
    cols = cols_of([dict(pos=0, cigar=one, lane=1), dict(pos=90, cigar=one, lane=0)])
    g, t = gcb_ref.table([cols, cols], [REF200], 2, 20)
    assert hits(t, 0, 0) == {50: 2} and hits(t, 0, 1) == {0: 2} and g.sum() == 181


def test_text_line_by_line():
    cols = cols_of([dict(pos=90, cigar=[(4, 0)], qual=7, lane=1)])
    g, t = gcb_ref.table(cols, [REF200], 2, 20)
    lines = gcb_ref.text(g, t, 20, "S", ["L1", "L0"], [1, 0]).split("\n")
    zeros = ["0"] * 101
    gline = list(zeros)
    gline[0], gline[100] = "81", "81"
    for k in range(1, 20):
        gline[5 * k] = "1"

    def row(at, v):
        r = list(zeros)
        r[at] = str(v)
        return " ".join(r)
    assert lines == ["sample_id S", "lane L1", "gc_bias_window 20", "genome_windows_by_gc " + " ".join(gline), "read_starts_by_gc " + row(50, 1),
                     "bases_by_gc " + row(50, 4), "base_qual_sum_by_gc " + row(50, 28),
                     "sample_id S", "lane L0", "gc_bias_window 20", "genome_windows_by_gc " + " ".join(gline), "read_starts_by_gc " + " ".join(zeros),
                     "bases_by_gc " + " ".join(zeros), "base_qual_sum_by_gc " + " ".join(zeros), ""]


def random_case(seed, n, n_lanes, W):
    """Three contigs with N runs (one not given), n reads of every flag kind at positions around and beyond the contigs' ends."""
    rng = np.random.default_rng(seed)
    refs = []
    for ln in (700, W + 3, 400):
        r = rng.choice(5, ln, p=[0.3, 0.2, 0.2, 0.25, 0.05]).astype(np.uint8)
        r[ln // 2:ln // 2 + 7] = N
        refs.append(r)
    refs.insert(1, None)
    reads = []
    for i in range(n):
        ops = [(int(rng.integers(1, 40)), int(rng.choice([0, 0, 0, 1, 2, 3, 4, 7, 8]))) for k in range(int(rng.integers(0, 6)))]
        f = int(rng.choice([P | FIRST, P | LAST, 0, P | FIRST | 0x400, P | LAST | 0x200, P | FIRST | 0x4, P | FIRST | 0x100, P | LAST | 0x800])) | (REV if rng.random() < 0.5 else 0)
        reads.append(dict(pos=int(rng.integers(-30, 760)), cigar=ops, flag=f, rid=int(rng.integers(-1, 5)), lane=int(rng.integers(0, n_lanes + 1)),
                          qual=None if rng.random() < 0.1 else int(rng.integers(0, 256))))
    return cols_of(reads), refs


def test_table_fast_is_table():
    for W in (20, 33, 100):
        cols, refs = random_case(5 + W, 1500, 2, W)
        cols2, _ = random_case(6 + W, 300, 2, W)
        g, t = gcb_ref.table([cols, cols2], refs, 2, W)
        assert g.sum() > 300 and all(t[l, r].any() for l in range(2) for r in range(3))
        g2, t2 = gcb_ref.table_fast([cols, cols2], refs, 2, W)
        assert np.array_equal(g, g2) and np.array_equal(t, t2)


def test_reciprocals_divide_exactly():
    """floor(100 gc / (W - n)) == (100 gc * ceil(2^32 / (W - n))) >> 32 for every window length, N count and gc the kernels can meet."""
    for W in range(gcb_steps.W_MIN, gcb_steps.W_MAX + 1):
        for n, m in enumerate(gcb_steps.reciprocals(W)):
            assert m < 1 << 32
            x = 100 * np.arange(W - n + 1, dtype=np.uint64)
            assert np.array_equal((x * np.uint64(m)) >> np.uint64(32), x // np.uint64(W - n)), (W, n)


def test_launch_constants_are_the_kernels():
    src = open(os.path.join(ROOT, "bamqc_amd", "csrc", "k_gcb.hip")).read()

    def define(name):
        return re.search(r"#define %s\s+(\S+)" % name, src).group(1)
    assert int(define("GG_THREADS")) == gcb_steps.GG_THREADS and int(define("GG_ITEMS")) == gcb_steps.GG_ITEMS and int(define("GG_SHARE")) == gcb_steps.GG_SHARE
    assert int(define("GR_THREADS")) == gcb_steps.GR_STEP and define("GR_STEP") == "GR_THREADS"
    walk = open(os.path.join(ROOT, "bamqc_amd", "csrc", "cigar_walk.h")).read()  # (the launch geometry: stated once)
    assert "share_grid(b.n_reads" in src and "+ 255) / 256" in walk  # WG_READS
    types = open(os.path.join(ROOT, "bamqc_amd", "csrc", "device_types.h")).read()
    assert re.search(r"#define BQC_GCB_WMIN\s+20\b", types) and re.search(r"#define BQC_GCB_WMAX\s+1000\b", types) and re.search(r"#define BQC_GCB_BINS\s+101\b", types)
    la = gcb_steps.reads_launch(1000, 256)
    assert (la["grid"], la["per"], la["steps"]) == (4, 250, [1, 1, 1, 1])
    assert gcb_steps.reads_launch(256 * 1024 + 1, 256)["steps"][0] == 2
    assert gcb_steps.genome_shares([99, 100, None, 100 + 8192, 100 + 8191], 100) == [(1, 0, 1), (3, 0, 8192), (3, 8192, 1), (4, 0, 8192)]
    # the share's bytes fit the kernel's LDS image at the longest window, from the worst alignment
    assert (3 + gcb_steps.GG_SHARE + gcb_steps.W_MAX - 1 + 3) // 4 + 1 <= gcb_steps.GG_THREADS * gcb_steps.GG_ITEMS
