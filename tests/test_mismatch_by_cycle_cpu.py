"""CPU: the options of the mismatches by cycle and base quality in the program's parser, their mirror in the Python ABI, and the
numpy restatement of the statistic (tests/mbc_ref.py) on two reads worked out by hand."""
import ctypes

import numpy as np

from bamqc_amd import _abi, _lib
from tests import mbc_ref, synth


def ask(*args):
    lib = _lib.load()
    argv = (ctypes.c_char_p * (len(args) + 1))(b"bamqualcheck", *[a.encode() for a in args])
    buf = ctypes.create_string_buffer(4096)
    rc = lib.bqc_program_args(len(args) + 1, argv, buf, 4096)
    return rc, buf.value.decode()


def test_parser_knows_the_options():
    base = ("-r", "g.fa", "-o", "x.bamqc")
    assert ask(*base, "--mismatch-by-cycle", "in.bam") == (0, "in.bam")
    assert ask(*base, "--mismatch-by-cycle-len", "300", "in.bam") == (0, "in.bam")
    assert ask(*base, "--mismatch-by-cycle-len=300", "--mismatch-by-cycle", "--qual-by-cycle", "in.bam") == (0, "in.bam")
    assert ask(*base, "--mismatch-by-cycle-len", "0", "in.bam")[0] == 1
    assert ask(*base, "--mismatch-by-cycle-len", "x", "in.bam")[0] == 1
    assert ask(*base, "--mismatch-by-cycle-len", "-3", "in.bam")[0] == 1
    assert ask(*base, "in.bam", "--mismatch-by-cycle-len")[0] == 1  # no value


def test_abi_mirror():
    names = [f[0] for f in _abi.Options._fields_]
    assert names[-3:] == ["qual_by_cycle", "mismatch_by_cycle", "pad_tail"]
    assert _abi.Options.mismatch_by_cycle.offset == _abi.Options.qual_by_cycle.offset + 4
    assert ctypes.sizeof(_abi.Options) == _abi.Options.mismatch_by_cycle.offset + 8  # the field and its padding: 8 more than before
    assert ctypes.sizeof(_abi.Options) % 8 == 0
    o, keep = _abi.make_options(n_refs=1, mismatch_by_cycle=300)
    assert o.mismatch_by_cycle == 300 and o.qual_by_cycle == 0 and o.struct_size == ctypes.sizeof(_abi.Options)
    assert _abi.make_options(n_refs=1)[0].mismatch_by_cycle == 0
    assert [f[0] for f in _abi.MbcView._fields_] == ["n_cycles", "n_q", "stride", "aligned", "mismatch"]


def test_restatement_on_two_reads():
    ref = np.array([0, 1, 2, 3] * 5, np.uint8)  # ACGTACGTAC...
    # forward, first mate, at 2: the genome reads GTACGTAC; stored bases 1 (T -> A) and 6 (A -> C) are planted mismatches
    fwd = synth.single_read("GAACGTCC", [30, 20, 30, 30, 30, 30, 10, 30], [(8, "M")], 0x1 | 0x40, pos=2)
    # reverse, second mate, at 5: the genome reads CGTA; stored base 0 (C -> T) is planted: cycle L - 1 - 0 = 3
    rev = synth.single_read("TGTA", [5, 6, 7, 8], [(4, "M")], 0x1 | 0x80 | 0x10, pos=5)
    cols = synth.concat([fwd, rev])
    T = mbc_ref.table(cols, [ref], n_lanes=1, N=7)  # N = 7: cycle 7 of the forward read is behind the capacity
    want = np.zeros((1, 2, 2, 7, 224), np.uint64)
    for c, q in enumerate([30, 20, 30, 30, 30, 30, 10]):
        want[0, 0, 0, c, q] = 1
    want[0, 0, 1, 1, 20] = want[0, 0, 1, 6, 10] = 1
    want[0, 1, 0, 3, 5] = want[0, 1, 0, 2, 6] = want[0, 1, 0, 1, 7] = want[0, 1, 0, 0, 8] = 1
    want[0, 1, 1, 3, 5] = 1
    assert np.array_equal(T, want)
    assert mbc_ref.sizes(T[0, 0], 8) == (7, 31) and mbc_ref.sizes(T[0, 1], 4) == (4, 9)
    assert mbc_ref.sizes(np.zeros((2, 7, 224), np.uint64), 0) == (0, 0)
    lines = mbc_ref.text(T, np.array([[8, 4]]), "S", ["L1"]).split("\n")
    assert lines[:3] == ["sample_id S", "lane L1", "aligned_bases_by_position_and_qual_first 7 31"]
    assert lines[3] == " ".join(["0"] * 30 + ["1"])
    assert lines[10] == "mismatches_by_position_and_qual_first 7 31" and lines[12] == " ".join(["0"] * 20 + ["1"] + ["0"] * 10)
    assert lines[18] == "aligned_bases_by_position_and_qual_second 4 9" and lines[23] == "mismatches_by_position_and_qual_second 4 9"
    assert lines[27] == "0 0 0 0 0 1 0 0 0" and lines[28] == "" and len(lines) == 29
    # what does not count: a read base N and an ambiguity code, a genome N, an insertion and a soft clip, an unmapped read
    refn = ref.copy()
    refn[4] = 4
    odd = synth.single_read("GNMCGTAC", [30] * 8, [(8, "M")], 0x1 | 0x40, pos=2)      # stored 1, 2 are no bases; stored 2 lies on the genome's N
    ins = synth.single_read("GGGTAAACG", [30] * 9, [(2, "S"), (2, "M"), (3, "I"), (2, "M")], 0x1 | 0x40, pos=2)  # 2S, GT on genome 2..3, 3I, CG on genome 4..5
    unm = synth.single_read("GTAC", [30] * 4, [(4, "M")], 0x1 | 0x40 | 0x4, pos=2)
    T2 = mbc_ref.table(synth.concat([odd, ins, unm]), [refn], 1, 16)
    # odd: stored 0, 3..7 compared, none differs.  ins: stored 2, 3 against genome 2, 3 (G, T: equal), stored 7, 8 (C, G) against genome 4 (N: not counted), 5 (C != G)
    a = np.zeros(16, np.uint64)
    a[[0, 3, 4, 5, 6, 7]] += 1
    a[[2, 3, 8]] += 1
    assert np.array_equal(T2[0, 0, 0, :, 30], a) and T2[0, 0, 0].sum() == a.sum()
    m = np.zeros(16, np.uint64)
    m[8] = 1
    assert np.array_equal(T2[0, 0, 1, :, 30], m) and T2[0, 0, 1].sum() == 1
    # two batches add
    assert np.array_equal(mbc_ref.table([cols, cols], [ref], 1, 7), 2 * want)
