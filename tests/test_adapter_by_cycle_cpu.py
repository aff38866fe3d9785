"""CPU: the options of the adapter content by cycle in the program's parser, the Python mirror of bqc_modules, what bqc_create_ex
refuses before it asks for a device, the restatement of the statistic (tests/adp_ref.py) on reads worked out by hand, its text, its
vectorised twin, and the launch constants of tests/adp_steps.py against the kernel's."""
import ctypes
import os
import re

import numpy as np
import pytest

from bamqc_amd import _abi, _lib
from tests import adp_ref, adp_steps
from tests.adp_steps import FIRST, LAST, P, REV, as_stored, cols_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = 1
UNI = "AGATCGGAAGAG"  # Illumina_Universal, slot 0 of the built-in set
ONE = [("uni", UNI)]


def ask(*args):
    lib = _lib.load()
    argv = (ctypes.c_char_p * (len(args) + 1))(b"bamqualcheck", *[a.encode() for a in args])
    buf = ctypes.create_string_buffer(4096)
    rc = lib.bqc_program_args(len(args) + 1, argv, buf, 4096)
    return rc, buf.value.decode()


def test_parser_knows_the_options():
    base = ("-r", "g.fa", "-o", "x.bamqc")
    assert ask(*base, "--adapter-by-cycle", "in.bam") == (0, "in.bam")
    assert ask(*base, "--adapter-by-cycle-len", "300", "in.bam") == (0, "in.bam")
    assert ask(*base, "--adapter-by-cycle-len=300", "--adapter-by-cycle", "--qual-by-cycle", "--mismatch-by-cycle", "in.bam") == (0, "in.bam")
    assert ask(*base, "--adapter", "X=ACGTACGT", "in.bam") == (0, "in.bam")
    assert ask(*base, "--adapter=X=ACGTACGT", "--adapter", "Y.2-b_=ACGTACGTACGTACGT", "--adapter-by-cycle-len", "50", "in.bam") == (0, "in.bam")
    assert ask(*base, "--adapter-by-cycle-len", "0", "in.bam")[0] == 1
    assert ask(*base, "--adapter-by-cycle-len", "x", "in.bam")[0] == 1
    assert ask(*base, "--adapter-by-cycle-len", "-3", "in.bam")[0] == 1
    assert ask(*base, "in.bam", "--adapter-by-cycle-len")[0] == 1  # no value
    assert ask(*base, "in.bam", "--adapter")[0] == 1
    for bad in ("ACGTACGT", "=ACGTACGT", "X=ACGTACG", "X=ACGTACGTACGTACGTA", "X=ACGTACGN", "X=acgtacgt", "a b=ACGTACGT", "x" * 32 + "=ACGTACGT", "X="):
        assert ask(*base, "--adapter", bad, "in.bam")[0] == 1, bad
    assert ask(*base, "--adapter", "X=ACGTACGT", "--adapter", "X=ACGTACGA", "in.bam")[0] == 1  # a name twice
    nine = [a for i in range(9) for a in ("--adapter", "n%d=ACGTACGT" % i)]
    assert ask(*base, *nine[:16], "in.bam")[0] == 0 and ask(*base, *nine, "in.bam")[0] == 1


def test_help_names_the_options(capfd):
    assert ask("--help")[0] == 2
    ctypes.CDLL(None).fflush(None)  # (the library printed through C's stdout)
    out = capfd.readouterr().out
    for opt in ("--adapter-by-cycle\n", "--adapter-by-cycle-len INT", "--adapter NAME=SEQ", "OUT.adp"):
        assert opt in out, opt


def test_abi_mirror():
    assert [f[0] for f in _abi.Modules._fields_] == ["struct_size", "adapter_by_cycle", "n_adapters", "pad", "adapters"]
    assert ctypes.sizeof(_abi.Modules) % 8 == 0 and ctypes.sizeof(_abi.Modules) == 16 + ctypes.sizeof(ctypes.c_void_p)
    assert _abi.Modules.adapters.offset == 16
    assert [f[0] for f in _abi.Adapter._fields_] == ["name", "seq"]
    assert [f[0] for f in _abi.AdpView._fields_] == ["n_cycles", "n_adapters", "stride", "reads_by_length", "first_hit", "adapters"]
    m, keep = _abi.make_modules()
    assert (m.struct_size, m.adapter_by_cycle, m.n_adapters) == (ctypes.sizeof(_abi.Modules), 0, 0) and not m.adapters
    m, keep = _abi.make_modules(adapter_by_cycle=300, adapters=[("a", "ACGTACGT"), ("b", "TTTTTTTTTT")])
    assert (m.adapter_by_cycle, m.n_adapters) == (300, 2) and m.adapters[1].name == b"b" and m.adapters[1].seq == b"TTTTTTTTTT"
    # bqc_options is what it was
    assert [f[0] for f in _abi.Options._fields_][-3:] == ["qual_by_cycle", "mismatch_by_cycle", "pad_tail"]
    assert _lib.load().bqc_abi_version() == 2


def create_ex(N, adapters, struct_size=None, max_read_len=1024):
    lib = _lib.load()
    opt, keep = _abi.make_options(n_refs=1, max_read_len=max_read_len)
    mod, keep2 = _abi.make_modules(N, adapters, struct_size=struct_size)
    h = ctypes.c_void_p()
    rc = lib.bqc_create_ex(ctypes.byref(opt), ctypes.byref(mod), ctypes.byref(h))
    msg = (lib.bqc_last_error(None) or b"").decode()
    if rc == 0:
        lib.bqc_destroy(h)
    return rc, msg


@pytest.mark.parametrize("N, adapters, more, names", [
    (16, None, dict(struct_size=16), ["struct_size"]),
    (0, ONE, {}, ["adapter_by_cycle"]),
    (1025, None, {}, ["adapter_by_cycle", "1025", "max_read_len"]),
    (16, [("n%d" % i, "ACGTACGT") for i in range(9)], {}, ["9 adapters"]),
    (16, [("short", "ACGTACG")], {}, ["short", "ACGTACG"]),
    (16, [("long", "ACGTACGTACGTACGTA")], {}, ["long", "ACGTACGTACGTACGTA"]),
    (16, [("n", "ACGTACGN")], {}, ["'N'"]),
    (16, [("lower", "acgtacgt")], {}, ["'a'"]),
    (16, [("bad name", "ACGTACGT")], {}, ["bad name"]),
    (16, [("", "ACGTACGT")], {}, ["name"]),
    (16, [("x" * 32, "ACGTACGT")], {}, ["x" * 32]),
    (16, [("twice", "ACGTACGT"), ("other", "ACGTACGT"), ("twice", "ACGTACGA")], {}, ["twice"]),
])
def test_create_ex_refuses_before_it_asks_for_a_device(N, adapters, more, names):
    rc, msg = create_ex(N, adapters, **more)
    assert rc == ERR_ARG, (rc, msg)  # (BQC_ERR_DEVICE, 2, would mean the device was asked first)
    for word in names:
        assert word in msg, (word, msg)


def test_create_ex_takes_a_good_set_as_far_as_the_device():
    import torch
    rc, msg = create_ex(16, [("a", "ACGTACGT"), ("b", "ACGTACGTACGTACGT")])
    assert rc == (0 if torch.cuda.is_available() else 2), (rc, msg)
    rc, msg = create_ex(0, None)  # the module off
    assert rc == (0 if torch.cuda.is_available() else 2), (rc, msg)


def first_hits(T, mate=0, slot=0, lane=0):
    return {int(c): int(T[lane, mate, slot, c]) for c in np.flatnonzero(T[lane, mate, slot])}


def test_restatement_on_reads_worked_out_by_hand():
    fwd = "CC" + UNI + "TTTTTT"                       # forward, first mate, 20 bases: the adapter at cycle 2
    rev = as_stored("CCCCC" + UNI + "GGG", True)      # reverse, second mate, 20 bases: cycle 5 — stored, its reverse complement lies at 3
    assert rev == "CCC" + "CTCTTCCGATCT" + "GGGGG"
    cols, _ = cols_of([(fwd, P | FIRST), (rev, P | LAST | REV)])
    T = adp_ref.table(cols, 1, 32, ONE)
    assert first_hits(T, 0) == {2: 1} and first_hits(T, 1) == {5: 1}
    assert first_hits(T, 0, adp_ref.E_ROW) == {19: 1} and first_hits(T, 1, adp_ref.E_ROW) == {19: 1}
    assert T.sum() == 4 and T.shape == (1, 2, 9, 32)
    # the adapter ending exactly at L, and one base short of it (cut off: no occurrence)
    T = adp_ref.table(cols_of([("GGGG" + UNI, P | FIRST), ("GGGG" + UNI[:-1], P | FIRST)])[0], 1, 32, ONE)
    assert first_hits(T) == {4: 1} and first_hits(T, 0, adp_ref.E_ROW) == {14: 1, 15: 1}
    # an N, an ambiguity code and a `=` inside an occurrence match nothing; two occurrences count once, at the first
    odd = [("GG" + UNI[:5] + x + UNI[6:] + "GG", P | FIRST) for x in "NM="]
    two = [("G" + UNI + "CC" + UNI, P | FIRST), (as_stored("GGG" + UNI + "C" + UNI, True), P | FIRST | REV)]
    T = adp_ref.table(cols_of(odd + two)[0], 1, 64, ONE)
    assert first_hits(T) == {1: 1, 3: 1}
    # a first hit at N - 1 is counted, one at N is not; E is cut at N - 1
    T = adp_ref.table(cols_of([("G" * 7 + UNI, P | FIRST), ("G" * 8 + UNI, P | FIRST), ("G" * 3, P | FIRST)])[0], 1, 8, ONE)
    assert first_hits(T) == {7: 1} and first_hits(T, 0, adp_ref.E_ROW) == {7: 2, 2: 1}
    # not examined: secondary, supplementary, no mate flag, no bases, a read group behind n_lanes; examined: unmapped, duplicate, no qualities
    reads = [(UNI, P | FIRST | 0x100), (UNI, P | FIRST | 0x800), (UNI, P | 0x100), ("", P | FIRST), (UNI, P | FIRST),
             (UNI, P | FIRST | 0x4), (UNI, P | LAST | 0x400), (UNI, P | FIRST | 0x8000), (UNI, P | FIRST | LAST)]
    cols, _ = cols_of(reads, lane=[0, 0, 0, 0, 1, 0, 0, 0, 0])
    T = adp_ref.table(cols, 1, 16)  # (the built-in set)
    assert first_hits(T, 0) == {0: 3} and first_hits(T, 1) == {0: 1} and T[:, :, 1:8].sum() == 0
    assert adp_ref.sizes(T[0, 0]) == 12 and adp_ref.sizes(np.zeros((9, 16), np.uint64)) == 0
    # two batches add
    assert np.array_equal(adp_ref.table([cols, cols], 1, 16), 2 * T)


def test_text_line_by_line():
    cols, _ = cols_of([("CC" + UNI, P | FIRST), ("C" + UNI, P | FIRST)])
    T = adp_ref.table(cols, 2, 16, [("uni", UNI), ("g8", "GGGGGGGG")])
    lines = adp_ref.text(T, "S", ["L1", "L0"], [1, 0], [("uni", UNI), ("g8", "GGGGGGGG")]).split("\n")
    assert lines == ["sample_id S", "lane L1", "adapter_reads_by_length_first", "adapter_first_hit_by_position_first uni " + UNI,
                     "adapter_first_hit_by_position_first g8 GGGGGGGG", "adapter_reads_by_length_second",
                     "adapter_first_hit_by_position_second uni " + UNI, "adapter_first_hit_by_position_second g8 GGGGGGGG",
                     "sample_id S", "lane L0", "adapter_reads_by_length_first " + " ".join(["0"] * 12 + ["1", "1"]),
                     "adapter_first_hit_by_position_first uni " + UNI + " " + " ".join(["0", "1", "1"] + ["0"] * 11),
                     "adapter_first_hit_by_position_first g8 GGGGGGGG " + " ".join(["0"] * 14), "adapter_reads_by_length_second",
                     "adapter_first_hit_by_position_second uni " + UNI, "adapter_first_hit_by_position_second g8 GGGGGGGG", ""]


def random_batch(seed, n, n_lanes):
    """n reads of 0..80 bases over a skewed alphabet (so that 8-mers repeat), adapters planted in half of them, every flag kind."""
    rng = np.random.default_rng(seed)
    sets = [("a8", "ACCAGGTA"), ("a12", UNI), ("a16", "TTGACCAGTACCGGTA"), ("poly", "AAAAAAAAAA")]
    reads = []
    for i in range(n):
        L = int(rng.integers(0, 81))
        s = "".join(rng.choice(list("ACGTN=M"), L, p=[0.4, 0.2, 0.2, 0.15, 0.02, 0.02, 0.01]))
        for k in range(int(rng.integers(0, 3))):
            a = sets[int(rng.integers(0, 4))][1]
            at = int(rng.integers(0, max(1, L)))
            s = (s[:at] + a + s[at + len(a):])[:L]  # (cut off at the read's end where it does not fit)
        rev = bool(rng.random() < 0.5)
        f = P | (REV if rev else 0) | [FIRST, LAST, FIRST | LAST, 0x100][int(rng.choice(4, p=[0.45, 0.45, 0.05, 0.05]))] | (0x800 if rng.random() < 0.03 else 0)
        reads.append((as_stored(s, rev), f))
    return cols_of(reads, lane=rng.integers(0, n_lanes + 1, n))[0], sets  # (a read group behind n_lanes among them)


@pytest.mark.parametrize("N", [1024, 20])
def test_table_fast_is_table(N):
    cols, sets = random_batch(3, 3000, 2)
    cols2, _ = random_batch(4, 500, 2)
    T = adp_ref.table([cols, cols2], 2, N, sets)
    assert all(T[l, m, s].any() for l in range(2) for m in range(2) for s in (0, 1, 2, 3, 8)) and not T[:, :, 4:8].any()
    assert np.array_equal(adp_ref.table_fast([cols, cols2], 2, N, sets), T)
    assert np.array_equal(adp_ref.table_fast(cols, 2, N), adp_ref.table(cols, 2, N))  # the built-in set


def test_launch_constants_are_the_kernels():
    src = open(os.path.join(ROOT, "bamqc_amd", "csrc", "k_adp.hip")).read()

    def define(name):
        return re.search(r"#define %s\s+(\S+)" % name, src).group(1)
    assert int(define("AD_THREADS")) == adp_steps.AD_STEP and define("AD_STEP") == "AD_THREADS" and int(define("AD_C")) == adp_steps.AD_C
    walk = open(os.path.join(ROOT, "bamqc_amd", "csrc", "cigar_walk.h")).read()  # (the launch geometry: stated once)
    assert "share_grid(b.n_reads" in src and "+ 255) / 256" in walk  # WG_READS
    la = adp_steps.adp_launch(1000, 256)
    assert (la["grid"], la["per"], la["steps"]) == (4, 250, [1, 1, 1, 1])
    lay = adp_steps.step_layout(8)
    adp_steps.assert_step_layout(lay)
    assert lay["n"] == 2 * 1024 * 8 + 977 and set(lay["lane"]) == {0, 1, 2}
