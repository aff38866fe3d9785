"""CPU: the options of the per-cycle base quality histograms in the program's parser, and the numpy restatement of the statistic
(tests/qbc_ref.py) on three reads worked out by hand."""
import ctypes

import numpy as np

from bamqc_amd import _lib
from tests import qbc_ref, synth


def ask(*args):
    lib = _lib.load()
    argv = (ctypes.c_char_p * (len(args) + 1))(b"bamqualcheck", *[a.encode() for a in args])
    buf = ctypes.create_string_buffer(4096)
    rc = lib.bqc_program_args(len(args) + 1, argv, buf, 4096)
    return rc, buf.value.decode()


def test_parser_knows_the_options():
    base = ("-r", "g.fa", "-o", "x.bamqc")
    assert ask(*base, "--qual-by-cycle", "in.bam") == (0, "in.bam")
    assert ask(*base, "--qual-by-cycle-len", "300", "in.bam") == (0, "in.bam")
    assert ask(*base, "--qual-by-cycle-len=300", "--qual-by-cycle", "in.bam") == (0, "in.bam")
    assert ask(*base, "--qual-by-cycle-len", "0", "in.bam")[0] == 1
    assert ask(*base, "--qual-by-cycle-len", "x", "in.bam")[0] == 1
    assert ask(*base, "--qual-by-cycle-len", "-3", "in.bam")[0] == 1
    assert ask(*base, "in.bam", "--qual-by-cycle-len")[0] == 1  # no value


def test_restatement_on_three_reads():
    fwd1 = synth.single_read("ACGT", [10, 20, 30, 40], [(4, "M")], 0x1 | 0x40)            # cycles 0..3 as stored
    rev2 = synth.single_read("ACG", [5, 20, 222], [(3, "M")], 0x1 | 0x80 | 0x10)          # cycle 0 is the LAST stored byte
    noq = synth.single_read("ACGTA", [0xFF] * 5, [(5, "M")], 0x1 | 0x40 | 0x8000)         # no qualities: not counted
    cols = synth.concat([fwd1, rev2, noq])
    H = qbc_ref.table(cols, n_lanes=1, N=3)  # N = 3: cycle 3 of the first read is behind the capacity
    want = np.zeros((1, 2, 3, 224), np.uint64)
    want[0, 0, 0, 10] = want[0, 0, 1, 20] = want[0, 0, 2, 30] = 1
    want[0, 1, 0, 222] = want[0, 1, 1, 20] = want[0, 1, 2, 5] = 1
    assert np.array_equal(H, want)
    assert qbc_ref.sizes(H[0, 0], 5) == (3, 31)   # the mate's longest read has 5 bases (the one without qualities): min(N, 5)
    assert qbc_ref.sizes(H[0, 1], 3) == (3, 223)
    assert qbc_ref.sizes(np.zeros((3, 224), np.uint64), 0) == (0, 0)
    text = qbc_ref.text(H, np.array([[5, 3]]), "S", ["L1"])
    lines = text.split("\n")
    assert lines[:3] == ["sample_id S", "lane L1", "base_qual_histogram_by_position_first 3 31"]
    assert lines[3] == " ".join(["0"] * 10 + ["1"] + ["0"] * 20)
    assert lines[6] == "base_qual_histogram_by_position_second 3 223" and lines[7].endswith(" 1") and len(lines[7].split()) == 223
    assert lines[10] == "" and len(lines) == 11
    # two batches add
    assert np.array_equal(qbc_ref.table([cols, cols], 1, 3), 2 * want)
