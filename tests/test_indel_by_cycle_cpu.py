"""CPU: the options of the indel tables in the program's parser, the Python mirror of bqc_ibc_view, the restatement of the statistic
(tests/ibc_ref.py) on reads worked out by hand, its text, its vectorised twin on every case of tests/test_gpu_indel_by_cycle.py, and
the launch constants of tests/ibc_steps.py against the kernel's."""
import ctypes
import os
import re

import numpy as np
import pytest

from bamqc_amd import _abi, _lib
from tests import ibc_ref, ibc_steps
from tests.ibc_steps import D, EQ, FIRST, H, I, LAST, M, MAIN, N_, OPMAX, P, P_, REV, S, X, cols_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = 64


def ask(*args):
    lib = _lib.load()
    argv = (ctypes.c_char_p * (len(args) + 1))(b"bamqualcheck", *[a.encode() for a in args])
    buf = ctypes.create_string_buffer(4096)
    rc = lib.bqc_program_args(len(args) + 1, argv, buf, 4096)
    return rc, buf.value.decode()


def test_parser_knows_the_options(capfd):
    base = ("-r", "g.fa", "-o", "x.bamqc")
    assert ask(*base, "--indel-by-cycle", "in.bam") == (0, "in.bam")
    assert ask(*base, "--indel-by-cycle-len", "50", "in.bam") == (0, "in.bam")
    assert ask(*base, "--indel-by-cycle-len=300", "--indel-by-cycle", "in.bam") == (0, "in.bam")
    assert ask(*base, "--indel-by-cycle", "--qual-by-cycle", "--mismatch-by-cycle", "--adapter-by-cycle", "--gc-bias", "in.bam") == (0, "in.bam")
    assert ask("-r", "g.fa", "--indel-by-cycle", "--manifest", os.devnull)[0] in (0, 1)  # (an empty list is the list's matter, not the option's)
    for bad in ("0", "-20", "x", "100x", "", "1e2", "1073741824"):
        assert ask(*base, "--indel-by-cycle-len", bad, "in.bam")[0] == 1, bad
    assert ask(*base, "in.bam", "--indel-by-cycle-len")[0] == 1  # no value
    ctypes.CDLL(None).fflush(None)
    assert "--indel-by-cycle-len wants 1 or more" in capfd.readouterr().err


def test_help_names_the_options(capfd):
    assert ask("--help")[0] == 2
    ctypes.CDLL(None).fflush(None)  # (the library printed through C's stdout)
    out = capfd.readouterr().out
    for opt in ("--indel-by-cycle\n", "--indel-by-cycle-len INT", "OUT.ibc"):
        assert opt in out, opt


def test_abi_mirror():
    assert [f[0] for f in _abi.IbcView._fields_] == ["n_cycles", "n_len", "reads_by_length", "insertions", "deletions", "insertion_lengths", "deletion_lengths"]
    assert ctypes.sizeof(_abi.IbcView) == 8 + 5 * ctypes.sizeof(ctypes.c_void_p) and _abi.IbcView.reads_by_length.offset == 8
    lib = _lib.load()
    for name in ("bqc_enable_indel_by_cycle", "bqc_indel_by_cycle", "bqc_write_indel_by_cycle"):
        assert name in _lib._SIGNATURES and getattr(lib, name)
    # bqc_options, bqc_modules and the ABI version are what they were
    assert lib.bqc_abi_version() == 2
    assert [f[0] for f in _abi.Options._fields_][-3:] == ["qual_by_cycle", "mismatch_by_cycle", "pad_tail"]
    assert [f[0] for f in _abi.Modules._fields_] == ["struct_size", "adapter_by_cycle", "n_adapters", "pad", "adapters"]
    header = open(os.path.join(ROOT, "include", "bamqc.h")).read()
    for rule in ("It is an event iff n >= 1 and j + n <= L", "c = L - j - n with 0x10 set", "It is an event iff n >= 1 and 0 < j < L",
                 "c = j - 1 for a forward read, c = L - 1 - j with 0x10 set", "E[min(L, N) - 1] += 1", "n_lanes * 2 * (3 N + 128) words",
                 "int bqc_enable_indel_by_cycle(bqc_ctx* ctx, uint32_t n_cycles);"):
        assert rule in header, rule


def test_constants_are_the_kernels():
    src = open(os.path.join(ROOT, "bamqc_amd", "csrc", "k_ibc.hip")).read()
    dev = open(os.path.join(ROOT, "bamqc_amd", "csrc", "device_types.h")).read()
    walk = open(os.path.join(ROOT, "bamqc_amd", "csrc", "cigar_walk.h")).read()  # (the wave's pass and the launch geometry: stated once)

    def define(name, text=src):
        return re.search(r"#define %s\s+(\S+)" % name, text).group(1)
    assert int(define("IB_THREADS")) == ibc_steps.IB_STEP and define("IB_STEP") == "IB_THREADS"
    assert int(define("IB_T")) == ibc_steps.IB_T and int(define("IB_C")) == ibc_steps.IB_C
    assert int(define("BQC_IBC_K", dev)) == ibc_steps.K == ibc_ref.K and int(define("BQC_IBC_ROWS", dev)) == 3
    assert "p += WAVE" in src and "p0 + WAVE + ln" in walk and ibc_steps.PASS == 64
    assert "share_grid(b.n_reads" in src and "((uint64_t)n_reads + 255) / 256" in walk and ibc_steps.WG_READS == 256
    la = ibc_steps.ibc_launch(1000, 256)
    assert la["grid"] == 4 and la["per"] == 250 and la["steps"] == [1, 1, 1, 1]
    la = ibc_steps.ibc_launch(256 * 1024 + 1, 256)
    assert la["grid"] == 256 and la["per"] == 1025 and la["steps"][0] == 2 and la["steps"][-1] == 1


def one(cigar, N=16, L=None, flag=P | FIRST | MAIN, lane=0, n_lanes=1):
    """The plain restatement on one read -> (E, IC, DC as {index: count}, IL, DL as {length bin + 1: count}) of its lane and mate."""
    r = dict(cigar=cigar, flag=flag, lane=lane)
    if L is not None:
        r["L"] = L
    T = ibc_ref.table(cols_of([r]), n_lanes, N)
    w = T[min(lane, n_lanes - 1), 0 if flag & 0x40 else 1]

    def nz(a, shift=0):
        return {int(i) + shift: int(a[i]) for i in np.flatnonzero(a)}
    return nz(w[:N]), nz(w[N:2 * N]), nz(w[2 * N:3 * N]), nz(w[3 * N:3 * N + K], 1), nz(w[3 * N + K:], 1)


def test_worked_out_by_hand():
    # forward: 4M 2I 3M 1D 5M, L = 14: insertion at j = 4, deletion between stored bases 8 and 9
    assert one([(4, M), (2, I), (3, M), (1, D), (5, M)]) == ({13: 1}, {4: 1}, {8: 1}, {2: 1}, {1: 1})
    # the same read reversed: the insertion's first base in sequencing order is cycle 14 - 4 - 2, the deletion follows cycle 14 - 1 - 9
    assert one([(4, M), (2, I), (3, M), (1, D), (5, M)], flag=P | LAST | MAIN | REV) == ({13: 1}, {8: 1}, {4: 1}, {2: 1}, {1: 1})
    # an insertion at j = 0, and one ending exactly at L
    assert one([(3, I), (7, M)]) == ({9: 1}, {0: 1}, {}, {3: 1}, {})
    assert one([(7, M), (3, I)]) == ({9: 1}, {7: 1}, {}, {3: 1}, {})
    assert one([(7, M), (3, I)], flag=P | FIRST | MAIN | REV) == ({9: 1}, {0: 1}, {}, {3: 1}, {})
    # an insertion running past L is no event, and j moves on: the deletion behind it lies at j = 12 >= L
    assert one([(7, M), (5, I), (1, D), (2, M)], L=11) == ({10: 1}, {}, {}, {}, {})
    assert one([(7, M), (5, I), (1, D), (2, M)], L=12) == ({11: 1}, {7: 1}, {}, {5: 1}, {})  # (ends at L; the deletion at j = L)
    assert one([(7, M), (5, I), (1, D), (2, M)], L=13) == ({12: 1}, {7: 1}, {11: 1}, {5: 1}, {1: 1})
    # a deletion at j = 0 and one at j = L; one between two bases
    assert one([(2, D), (9, M)]) == ({8: 1}, {}, {}, {}, {})
    assert one([(9, M), (2, D)]) == ({8: 1}, {}, {}, {}, {})
    assert one([(1, M), (2, D), (8, M)]) == ({8: 1}, {}, {0: 1}, {}, {2: 1})
    assert one([(1, M), (2, D), (8, M)], flag=P | FIRST | MAIN | REV) == ({8: 1}, {}, {7: 1}, {}, {2: 1})
    # S, = and X advance; N, H, P and the codes 9 ... 15 do nothing; zero-length operations are no events
    assert one([(2, H), (3, S), (1, EQ), (1, I), (2, X), (9, N_), (4, P_), (1, D), (2, M), (3, H)]) == ({8: 1}, {4: 1}, {6: 1}, {1: 1}, {1: 1})
    assert one([(2, M)] + [(5, op) for op in range(9, 16)] + [(1, I), (2, M)]) == ({4: 1}, {2: 1}, {}, {1: 1}, {})
    assert one([(2, M), (0, I), (0, D), (3, M), (0, D)]) == ({4: 1}, {}, {}, {}, {})
    # a reference skip is not a deletion
    assert one([(3, M), (100, N_), (3, M)]) == ({5: 1}, {}, {}, {}, {})
    # an event at cycle N - 1 counts, one at cycle N enters no table — the length tables included; E sits at min(L, N) - 1
    assert one([(15, M), (1, I), (1, D), (9, M)], N=16) == ({15: 1}, {15: 1}, {15: 1}, {1: 1}, {1: 1})
    assert one([(16, M), (1, I), (1, D), (9, M)], N=16) == ({15: 1}, {}, {}, {}, {})
    assert one([(16, M), (1, I), (1, D), (9, M)], N=17) == ({16: 1}, {16: 1}, {16: 1}, {1: 1}, {1: 1})
    assert one([(9, M), (1, D), (1, I), (16, M)], N=16, flag=P | FIRST | MAIN | REV) == ({15: 1}, {}, {}, {}, {})  # (reverse: cycles 16 and 16)
    assert one([(10, M), (1, D), (1, I), (15, M)], N=16, flag=P | FIRST | MAIN | REV) == ({15: 1}, {15: 1}, {15: 1}, {1: 1}, {1: 1})
    # lengths 63, 64, 65 and 2^28 - 1: the last bin holds everything from 64 on
    for n, b in ((63, 63), (64, 64), (65, 64)):
        assert one([(2, M), (n, I), (2, M), (n, D), (2, M)], N=100) == ({n + 5: 1}, {2: 1}, {n + 3: 1}, {b: 1}, {b: 1})
    assert one([(2, M), (OPMAX, D), (2, M)]) == ({3: 1}, {}, {1: 1}, {}, {64: 1})
    assert one([(2, M), (OPMAX, I), (2, M)], L=4) == ({3: 1}, {}, {}, {}, {})  # (no read holds 2^28 - 1 inserted bases behind j = 2)


def test_reads_that_are_not_examined():
    cig = [(4, M), (1, I), (4, M)]
    empty = ({}, {}, {}, {}, {})
    for f in (P | FIRST | MAIN | 0x100, P | FIRST | MAIN | 0x800, P | LAST | MAIN | 0x4):
        assert one(cig, flag=f) == empty
    assert one([], L=9) == empty and one(cig, L=0) == empty
    for f in (0x400, 0x200, 0x8000, 0x20, 0x8):  # duplicates, QC fail, no qualities, mate's strand, mate unmapped: examined
        assert one(cig, flag=P | LAST | MAIN | f) == ({8: 1}, {4: 1}, {}, {1: 1}, {})


def test_what_the_library_refuses_first():
    """The restatement's side of batches that cannot reach k_ibc (tests/test_gpu_indel_by_cycle.py's docstring): a primary read
    without a mate flag and a read group at or behind n_lanes are simply not examined; inserted or deleted bases at or above hist_cap
    on a main chromosome are events like any other — the definition knows no hist_cap and no main chromosome."""
    cig = [(4, M), (1, I), (4, M)]
    T = ibc_ref.table(cols_of([dict(cigar=cig, flag=P | MAIN)]), 1, 16)
    assert not T.any() and not ibc_ref.table_fast(cols_of([dict(cigar=cig, flag=P | MAIN)]), 1, 16).any()
    for lane in (1, 2, 255):
        cols = cols_of([dict(cigar=cig, lane=lane), dict(cigar=cig, lane=0)])
        T = ibc_ref.table(cols, 1, 16)
        assert T.sum() == 3 and np.array_equal(T, ibc_ref.table_fast(cols, 1, 16))
    assert one([(4, M), (5000, D), (4, M), (4096, I), (4, M)], N=16) == ({15: 1}, {8: 1}, {3: 1}, {64: 1}, {64: 1})


def test_no_wrap_by_hand():
    """Query-consuming lengths past 2^32: only the events before them count (a sum taken in 32 bits would put the later ones at the
    stored indices 26 and 27)."""
    cols = cols_of(ibc_steps.wrap_reads())
    T = ibc_ref.table(cols, 1, 100)
    assert np.array_equal(T, ibc_ref.table_fast(cols, 1, 100))
    e, ic, dc, il, dl = ibc_ref.views(T, 0, 0)
    want_ic, want_dc = np.zeros(100, np.uint64), np.zeros(100, np.uint64)
    want_ic[[3, 100 - 3 - 2]] = 2  # forward: j = 3; reverse: L - j - n
    want_dc[[8, 100 - 1 - 9]] = 2  # forward: j - 1 = 8; reverse: L - 1 - j
    assert e[99] == 4 and np.array_equal(ic, want_ic) and np.array_equal(dc, want_dc) and il[1] == 4 and dl[0] == 4 and il.sum() == dl.sum() == 4


CASES = {
    "rule": (lambda: cols_of(ibc_steps.rule_reads()), 3),
    "paths": (lambda: cols_of(ibc_steps.path_reads()), 1),
    "wrap": (lambda: cols_of(ibc_steps.wrap_reads()), 1),
    "tile": (lambda: cols_of(ibc_steps.tile_reads(10_240)), 1),
    "groups": (lambda: cols_of(ibc_steps.group_reads()), 4),
    "cross": (lambda: cols_of(ibc_steps.cross_reads()), 2),
    "hot": (lambda: ibc_steps.hot_cols(3000), 1),
    "steps": (lambda: ibc_steps.step_batch(ibc_steps.step_layout(4)), 4),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_the_two_restatements_agree(case):
    make, n_lanes = CASES[case]
    cols = make()
    for N in (16, 300, 1024, 10_240):
        a, b = ibc_ref.table(cols, n_lanes, N), ibc_ref.table_fast(cols, n_lanes, N)
        assert np.array_equal(a, b), (case, N)
        ic, il = a[:, :, N:2 * N].sum(), a[:, :, 3 * N:3 * N + K].sum()
        dc, dl = a[:, :, 2 * N:3 * N].sum(), a[:, :, 3 * N + K:].sum()
        assert ic == il and dc == dl and a[:, :, :N].sum() > 0


def test_shapes_cross_their_edges():
    T_, C_ = ibc_steps.IB_T, ibc_steps.IB_C
    nc = sorted({len(r["cigar"]) for r in ibc_steps.path_reads()})
    assert nc == sorted(ibc_steps.PATH_NCIGARS) and {T_ - 1, T_, T_ + 1, 63, 64, 65, 127, 128, 129, 1000, 65_535} == set(nc)
    for n in (65, 129, 1000, 65_535):  # an event in the last operation of a pass and in the first of the next
        cig = ibc_steps.seam_cigar(n)
        assert all(cig[k][1] in (I, D) for s in range(64, n, 64) for k in (s - 1, s) if k < n) and cig[0][1] in (I, D) and cig[-1][1] in (I, D)
    w = ibc_steps.wrap_reads()
    assert all(len(r["cigar"]) > T_ for r in w) and len(w[0]["cigar"]) <= 64 < len(w[2]["cigar"])
    t = ibc_steps.tile_reads(10_240)
    assert {C_, C_ + 1} <= {ibc_steps.query_len(r["cigar"]) for r in t} and {True, False} == {len(r["cigar"]) > T_ for r in t}
    T = ibc_ref.table(cols_of(t), 1, 10_240)
    for c in (C_ - 1, C_, 10_239):
        assert T[0, 0, 10_240 + c] >= 2 and T[0, 1, 2 * 10_240 + c] >= 2, c
    g = ibc_steps.group_reads()
    assert {len(r["cigar"]) > T_ for r in g} == {True, False} and len(g) > 2 * ibc_steps.IB_STEP
    lay = ibc_steps.step_layout(256)
    ibc_steps.assert_step_layout(lay)
    assert ibc_steps.ibc_launch(len(g), 256)["grid"] < 256  # (a workgroup's share of the group batch holds several read groups)


def test_text():
    cols = cols_of([dict(cigar=[(2, M), (1, I), (2, M)], lane=1), dict(cigar=[(3, M), (70, D), (1, M)], lane=1, flag=P | LAST | MAIN)])
    text = ibc_ref.text(ibc_ref.table(cols, 2, 8), "S", ["b", "a"], [1, 0])
    lines = text.split("\n")
    assert lines[:5] == ["sample_id S", "lane b", "indel_reads_by_length_first 0 0 0 0 1", "insertions_by_position_first 0 0 1 0 0", "deletions_by_position_first 0 0 0 0 0"]
    assert lines[5] == "insertion_length_histogram_first 1" + " 0" * 63 and lines[6] == "deletion_length_histogram_first" + " 0" * 64
    assert lines[7:10] == ["indel_reads_by_length_second 0 0 0 1", "insertions_by_position_second 0 0 0 0", "deletions_by_position_second 0 0 1 0"]
    assert lines[11] == "deletion_length_histogram_second" + " 0" * 63 + " 1"
    assert lines[12:16] == ["sample_id S", "lane a", "indel_reads_by_length_first", "insertions_by_position_first"] and len(lines) == 25 and lines[-1] == ""
