"""CPU: the options of the substitution tables in the program's parser, the Python mirror of bqc_sbc_view, the exported symbols, the
restatement of the statistic (tests/sbc_ref.py) on reads worked out by hand, its vectorised twin on every fixture of
tests/test_gpu_substitutions.py, and the fixtures against the edges of the kernel (bamqc_amd/csrc/k_sbc.hip) they are meant to cross."""
import ctypes
import os
import re

import numpy as np
import pytest

from bamqc_amd import _abi, _lib
from tests import cycle_steps, sbc_ref, sbc_steps
from tests.sbc_steps import A, C, FIRST, G, LAST, MAIN, N_, P, REV, T, build, flag_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
XW = 512


def ask(*args):
    lib = _lib.load()
    argv = (ctypes.c_char_p * (len(args) + 1))(b"bamqualcheck", *[a.encode() for a in args])
    buf = ctypes.create_string_buffer(4096)
    rc = lib.bqc_program_args(len(args) + 1, argv, buf, 4096)
    return rc, buf.value.decode()


def test_parser_knows_the_options(capfd):
    base = ("-r", "g.fa", "-o", "x.bamqc")
    assert ask(*base, "--substitutions", "in.bam") == (0, "in.bam")
    assert ask(*base, "--substitutions-len", "50", "in.bam") == (0, "in.bam")
    assert ask(*base, "--substitutions-min-qual=0", "--substitutions-min-mapq", "255", "in.bam") == (0, "in.bam")
    assert ask(*base, "--substitutions", "--indel-by-cycle", "--qual-by-cycle", "--mismatch-by-cycle", "--adapter-by-cycle", "in.bam") == (0, "in.bam")
    for bad in ("0", "-20", "x", "100x", "", "1e2", "1073741824"):
        assert ask(*base, "--substitutions-len", bad, "in.bam")[0] == 1, bad
    for bad in ("223", "-1", "x", "", "20x"):
        assert ask(*base, "--substitutions-min-qual", bad, "in.bam")[0] == 1, bad
    for bad in ("256", "-1", "x", "", "3.5"):
        assert ask(*base, "--substitutions-min-mapq", bad, "in.bam")[0] == 1, bad
    assert ask(*base, "in.bam", "--substitutions-len")[0] == 1  # no value
    ctypes.CDLL(None).fflush(None)
    err = capfd.readouterr().err
    for words in ("--substitutions-len wants 1 or more", "--substitutions-min-qual wants 0 to 222", "--substitutions-min-mapq wants 0 to 255"):
        assert words in err, words


def test_help_names_the_options(capfd):
    assert ask("--help")[0] == 2
    ctypes.CDLL(None).fflush(None)
    out = capfd.readouterr().out
    for opt in ("--substitutions\n", "--substitutions-len INT", "--substitutions-min-qual INT", "--substitutions-min-mapq INT", "OUT.sbc"):
        assert opt in out, opt


def test_symbols_and_abi_mirror():
    """Fails on the parent commit: the library exports the three symbols and include/bamqc.h declares them."""
    lib = _lib.load()
    for name in ("bqc_enable_substitutions", "bqc_substitutions", "bqc_write_substitutions"):
        assert name in _lib._SIGNATURES and getattr(lib, name)
    assert [f[0] for f in _abi.SbcView._fields_] == ["n_cycles", "min_base_qual", "min_mapq", "by_context", "by_cycle"]
    assert ctypes.sizeof(_abi.SbcView) == 16 + 2 * ctypes.sizeof(ctypes.c_void_p) and _abi.SbcView.by_context.offset == 16
    assert lib.bqc_abi_version() == 2
    assert [f[0] for f in _abi.Options._fields_][-3:] == ["qual_by_cycle", "mismatch_by_cycle", "pad_tail"]
    assert [f[0] for f in _abi.Modules._fields_] == ["struct_size", "adapter_by_cycle", "n_adapters", "pad", "adapters"]
    header = open(os.path.join(ROOT, "include", "bamqc.h")).read()
    for rule in ("int bqc_enable_substitutions(bqc_ctx* ctx, uint32_t n_cycles, uint32_t min_base_qual, uint32_t min_mapq);",
                 "int bqc_substitutions(bqc_ctx* ctx, uint32_t lane, uint32_t mate, bqc_sbc_view* out);",
                 "int bqc_write_substitutions(bqc_ctx* ctx, const bqc_header_info* hdr, const char* path);",
                 "ctx = 16 g[rr-1] + 4 t + g[rr+1]", "ctx = 16 (3 - g[rr+1]) + 4 (3 - t) + (3 - g[rr-1])", "512 + 16 N words",
                 "Y[lane][mate][c][t'][b'] += 1", "X[lane][mate][s][ctx][b'] += 1"):
        assert rule in header, rule


def test_constants_are_the_kernels():
    src = open(os.path.join(ROOT, "bamqc_amd", "csrc", "k_sbc.hip")).read()
    dev = open(os.path.join(ROOT, "bamqc_amd", "csrc", "device_types.h")).read()

    def define(name, text=src):
        return re.search(r"#define %s\s+(\S+)" % name, text).group(1)
    assert int(define("SB_C")) == sbc_steps.SB_C and int(define("SB_STEP")) == sbc_steps.SB_STEP == cycle_steps.MB_STEP
    assert int(define("SB_RUNS")) == sbc_steps.SB_RUNS == cycle_steps.MB_RUNS and int(define("SB_THREADS")) == 1024
    assert int(define("BQC_SBC_X_WORDS", dev)) == XW == sbc_ref.XW
    assert "256ull * it" in src and sbc_steps.PASS == 256
    assert "(b.n_reads + 255u) / 256u" in src and cycle_steps.WG_READS == 256
    # the LDS budget: Y, the table X, the run list and its control words within 160 KiB
    assert (2 * 16 * sbc_steps.SB_C + 1024 + 8 * sbc_steps.SB_RUNS + 8) * 4 <= 160 * 1024


# ---------------------------------------------------------------------------------------------------------------------------
# known answers
# ---------------------------------------------------------------------------------------------------------------------------
GEN = np.array([A, C, G, T, T, G, N_, C, A, A, G, C], np.uint8)  # 12 bases, an N at 6


def one(codes, pos, flag=P | FIRST | MAIN, ops=None, qual=None, mapq=60, N=16, Q=20, MQ=30, nibs=None, gen=GEN):
    """Both restatements on one read -> (X as {(strand, context name, read base): count}, Y as {(cycle, genome base, read base):
    count}, pairs without a context), bases as letters, as sequenced."""
    from tests.long_layout import records
    codes = np.asarray(codes, np.int64)
    cols = records([dict(codes=codes, qual=np.full(len(codes), 40, np.uint8) if qual is None else np.asarray(qual, np.uint8), flag=flag, pos=pos,
                         ops=[(len(codes), "M")] if ops is None else ops)])
    cols["mapq"][:] = mapq
    for j, nib in (nibs or {}).items():
        sbc_steps.set_nib(cols, sbc_steps.seq_offsets(cols), 0, j, nib)
    Tt, miss = sbc_ref.table(cols, [gen], 1, N, Q, MQ)
    Tf, missf = sbc_ref.table_fast(cols, [gen], 1, N, Q, MQ)
    assert np.array_equal(Tt, Tf) and np.array_equal(miss, missf)
    m = 0 if flag & 0x40 else 1
    assert not Tt[0, 1 - m].any()
    w = Tt[0, m]
    name = lambda ctx: "ACGT"[ctx >> 4] + "ACGT"[(ctx >> 2) & 3] + "ACGT"[ctx & 3]
    X = {(int(i) // 256, name((int(i) // 4) % 64), "ACGT"[int(i) % 4]): int(w[i]) for i in np.flatnonzero(w[:XW])}
    Y = {(int(i) // 16, "ACGT"[(int(i) // 4) % 4], "ACGT"[int(i) % 4]): int(w[XW + i]) for i in np.flatnonzero(w[XW:])}
    return X, Y, int(miss[0, m])


def test_forward_and_reverse_give_complementary_contexts():
    # genome 1..4 = C G T T, read = the genome with T -> A at rr = 3
    X, Y, miss = one([C, G, A, T], 1)
    assert X == {(0, "ACG", "C"): 1, (0, "CGT", "G"): 1, (0, "GTT", "A"): 1, (0, "TTG", "T"): 1} and miss == 0
    assert Y == {(0, "C", "C"): 1, (1, "G", "G"): 1, (2, "T", "A"): 1, (3, "T", "T"): 1}
    # the same record on the reverse strand: sequenced AACG -> ATCG against the template AACG, cycles from the other end
    X, Y, miss = one([C, G, A, T], 1, flag=P | LAST | MAIN | REV)
    assert X == {(1, "CGT", "G"): 1, (1, "ACG", "C"): 1, (1, "AAC", "T"): 1, (1, "CAA", "A"): 1} and miss == 0
    assert Y == {(3, "G", "G"): 1, (2, "C", "C"): 1, (1, "A", "T"): 1, (0, "A", "A"): 1}


def test_contig_ends_and_genome_n():
    X, Y, miss = one([A, C], 0)  # rr = 0 enters Y and not X
    assert Y == {(0, "A", "A"): 1, (1, "C", "C"): 1} and X == {(0, "ACG", "C"): 1} and miss == 1
    X, Y, miss = one([G, C], 10)  # rr = len - 1 as well
    assert Y == {(0, "G", "G"): 1, (1, "C", "C"): 1} and X == {(0, "AGC", "G"): 1} and miss == 1
    # 4..8 = T G N C A: the N as the right neighbour (rr = 5), as the base (rr = 6: no pair at all), as the left neighbour (rr = 7)
    X, Y, miss = one([T, G, A, C, A], 4)
    assert Y == {(0, "T", "T"): 1, (1, "G", "G"): 1, (3, "C", "C"): 1, (4, "A", "A"): 1}
    assert X == {(0, "TTG", "T"): 1, (0, "CAA", "A"): 1} and miss == 2
    # a run of one position beside an insertion, a deletion and a clip has the genome's context all the same
    X, Y, miss = one([A, A, G, A, T], 2, ops=[(2, "S"), (1, "M"), (1, "I"), (1, "M")])
    assert X == {(0, "CGT", "G"): 1, (0, "GTT", "T"): 1} and Y == {(2, "G", "G"): 1, (4, "T", "T"): 1} and miss == 0
    X, Y, miss = one([C, A], 1, ops=[(1, "M"), (6, "D"), (1, "M")])
    assert X == {(0, "ACG", "C"): 1, (0, "CAA", "A"): 1} and miss == 0
    # the neighbour may lie outside the alignment: a read of one base
    assert one([G], 2)[0] == {(0, "CGT", "G"): 1}


def test_read_codes_qualities_and_mapq():
    # read codes N (15), = (0) and an ambiguity code (3) are not examined
    X, Y, miss = one([C, G, T, T], 1, nibs={0: 15, 1: 0, 2: 3})
    assert Y == {(3, "T", "T"): 1} and X == {(0, "TTG", "T"): 1}
    # q at Q - 1, Q, 222 and 223
    X, Y, miss = one([C, G, T, T], 1, qual=[19, 20, 222, 223])
    assert Y == {(1, "G", "G"): 1, (2, "T", "T"): 1}
    assert len(one([C, G, T, T], 1, qual=[19, 20, 222, 223], Q=0)[1]) == 3 and len(one([C, G, T, T], 1, qual=[221, 222, 222, 223], Q=222)[1]) == 2
    # mapq at MQ - 1 and MQ; 255 is a number like any other
    assert one([C, G], 1, mapq=29) == ({}, {}, 0) and len(one([C, G], 1, mapq=30)[1]) == 2
    assert one([C, G], 1, mapq=254, MQ=255) == ({}, {}, 0) and len(one([C, G], 1, mapq=255, MQ=255)[1]) == 2
    # the capacity: cycle N - 1 counts, cycle N does not — on the reverse strand the record's first bases fall out
    assert sorted(c for c, _, _ in one([C, G, T, T], 1, N=3)[1]) == [0, 1, 2]
    assert one([C, G, T, T], 1, N=3, flag=P | FIRST | MAIN | REV)[1] == {(0, "A", "A"): 1, (1, "A", "A"): 1, (2, "C", "C"): 1}
    # reads that are not examined
    for f in (P | FIRST | MAIN | 0x100, P | FIRST | MAIN | 0x800, P | LAST | MAIN | 0x4, P | FIRST | MAIN | 0x8000, P | MAIN | 0x100):
        assert one([C, G], 1, flag=f) == ({}, {}, 0)
    for f in (0x400, 0x200):  # duplicates and QC fail count
        assert len(one([C, G], 1, flag=P | LAST | MAIN | f)[1]) == 2


# ---------------------------------------------------------------------------------------------------------------------------
# the fixtures
# ---------------------------------------------------------------------------------------------------------------------------
CASES = {
    "rule": (lambda: sbc_steps.rule_batch(), 3),
    "rule_0_0": (lambda: sbc_steps.rule_batch(0, 0), 3),
    "window": (lambda: sbc_steps.window_batch(), 1),
    "shapes": (lambda: sbc_steps.shapes_batch(), 1),
    "hot": (lambda: (lambda c, r: (c, [r]))(*sbc_steps.hot_batch(2000, False)), 1),
    "hot_mismatch": (lambda: (lambda c, r: (c, [r]))(*sbc_steps.hot_batch(2000, True)), 1),
}
_made = {}


def case(name):
    if name not in _made:
        _made[name] = CASES[name][0]()
    return _made[name] + (CASES[name][1],)


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_two_restatements_agree(name):
    cols, refs, n_lanes = case(name)
    for N, Q, MQ in ((16, 20, 30), (300, 0, 0), (1024, 20, 30), (1024, 222, 255)):
        (a, ma), (b, mb) = sbc_ref.table(cols, refs, n_lanes, N, Q, MQ), sbc_ref.table_fast(cols, refs, n_lanes, N, Q, MQ)
        assert np.array_equal(a, b) and np.array_equal(ma, mb), (name, N, Q, MQ)
        x, y = a[:, :, :XW].sum(axis=2).astype(np.int64), a[:, :, XW:].sum(axis=2).astype(np.int64)
        assert np.array_equal(y - x, ma)  # sum X = sum Y minus the pairs without a context


def test_the_restatements_agree_on_the_group_and_step_batches():
    cols, ref = sbc_steps.groups_batch()
    for Q, MQ in ((0, 0), (20, 30)):
        (a, ma), (b, mb) = sbc_ref.table(cols, [ref], 3, 300, Q, MQ), sbc_ref.table_fast(cols, [ref], 3, 300, Q, MQ)
        assert np.array_equal(a, b) and np.array_equal(ma, mb) and a.any()
    lay = sbc_steps.step_layout(2, "short", 64)
    cols, ref = sbc_steps.step_batch(lay)
    (a, ma), (b, mb) = sbc_ref.table(cols, [ref], 4, 64, 20, 30), sbc_ref.table_fast(cols, [ref], 4, 64, 20, 30)
    assert np.array_equal(a, b) and np.array_equal(ma, mb) and all(a[l, m].any() for l in range(4) for m in range(2))


def test_fixtures_cross_the_kernels_edges():
    C_ = sbc_steps.SB_C
    # the rule batch: every lane, mate and strand has contexts; pairs at both contig ends and beside N are without one
    cols, refs, _ = case("rule")
    T_, miss = sbc_ref.table(cols, refs, 3, 2048)
    assert all(T_[l, m, s * 256:(s + 1) * 256].any() for l in range(3) for m in range(2) for s in range(2)) and (miss > 0).all()
    assert all(T_[l, m, XW + 16 * c:XW + 16 * c + 16].any() for l in range(3) for m in range(2) for c in (0, 15, 16, 299, 300, 1023, C_ - 1, C_))
    f, pos = cols["flag"].astype(np.int64), cols["pos"].astype(np.int64)
    assert ((pos == 0) & (cols["rid"] == 0)).any() and ((pos + cols["l_seq"] == 96) & (cols["rid"] == 0)).any()
    assert {29, 30} <= set(cols["mapq"].tolist()) and {19, 20, 221, 222} <= set(cols["qual"].tolist())
    # the window batch: every residue of the run's first stored position, of pos and of the contig's length mod 4, runs of 1..9, both
    # strands, the contig's first and last base
    cols, refs, _ = case("window")
    assert len(cols["flag"]) == 6912 and {len(r) & 3 for r in refs} == {0, 1, 2, 3}
    nc = cols["n_cigar"].astype(np.int64)
    co = np.cumsum(nc) - nc
    first = cols["cigar"][co].astype(np.int64)
    clip = np.where((first & 15) == 4, first >> 4, 0)
    run = np.where((first & 15) == 4, cols["cigar"][co + 1].astype(np.int64) >> 4, first >> 4)
    pos = cols["pos"].astype(np.int64)
    rev = (cols["flag"].astype(np.int64) >> 4) & 1
    lens = np.array([len(r) for r in refs])[cols["rid"]]
    seen = {(int(a), int(b), int(c), int(d), int(e)) for a, b, c, d, e in zip(clip, pos & 3, run, rev, lens & 3)}
    assert len(seen) == 4 * 4 * 9 * 2 * 4
    for r in range(1, 10):
        assert ((pos == 0) & (run == r)).any() and ((pos + run == lens) & (run == r)).any() and ((pos > 8) & (pos + run < lens - 8) & (run == r)).any()
    # the shapes batch: reads of dozens of runs, more runs than the list holds, runs of several passes, runs cut at both contig ends,
    # reverse reads far above N, and cycles on both sides of the LDS tile's edge
    cols, refs, _ = case("shapes")
    runs = cycle_steps.mbc_runs(cols, [len(refs[0]), 0], 1024)
    assert runs.max() >= 48 and runs.sum() > sbc_steps.SB_RUNS and (runs == 0).sum() >= 7
    L = cols["l_seq"].astype(np.int64)
    assert (L > 2 * sbc_steps.PASS).any() and (cols["pos"] < 0).any() and (cols["pos"].astype(np.int64) + L > len(refs[0])).any()
    assert ((L > 3 * 1024) & ((cols["flag"] & 0x10) != 0)).any()
    T_, _ = sbc_ref.table_fast(cols, refs, 1, 4096)
    for m in range(2):
        assert all(T_[0, m, XW + 16 * c:XW + 16 * c + 16].any() for c in (C_ - 1, C_, 3999))
    # the hot batches: one bin of X takes every pair
    for name, base in (("hot", 0), ("hot_mismatch", 1)):
        cols, refs, _ = case(name)
        T_, miss = sbc_ref.table_fast(cols, refs, 1, 1024)
        assert T_[0, 0, base] == 2000 * 16 == T_[0, 0, :XW].sum() and miss.sum() == 0
    # the step batch of tests/cycle_steps.py gives every workgroup three steps with more runs than the list holds (k_mbc's launch)
    lay = sbc_steps.step_layout(256, "short", 300)
    assert min(lay["mbc"]["steps"]) >= 3 and lay["changes"][0] in lay["mbc_seams"]


def test_text():
    from tests.long_layout import records
    cols = records([dict(codes=[C, G, A, T], qual=[40] * 4, flag=P | FIRST | MAIN, pos=1, ops=[(4, "M")], lane=1)])
    Tt, _ = sbc_ref.table(cols, [GEN], 2, 8)
    lines = sbc_ref.text(Tt, 8, 20, 30, "S", ["b", "a"], [1, 0]).split("\n")
    assert lines[:4] == ["sample_id S", "lane b", "substitution_min_base_qual 20", "substitution_min_mapq 30"]
    assert lines[4] == "substitutions_by_context_first_forward AAA 0 0 0 0" and lines[4 + 6] == "substitutions_by_context_first_forward ACG 0 1 0 0"
    assert lines[4 + 0x2F] == "substitutions_by_context_first_forward GTT 1 0 0 0" and lines[4 + 64] == "substitutions_by_context_first_reverse AAA 0 0 0 0"
    assert lines[4 + 128] == "substitutions_by_position_first 4 16" and lines[4 + 129] == "0 0 0 0 0 1 0 0 0 0 0 0 0 0 0 0"
    assert lines[4 + 131] == "0 0 0 0 0 0 0 0 0 0 0 0 1 0 0 0" and lines[4 + 133] == "substitutions_by_context_second_forward AAA 0 0 0 0"
    assert lines[4 + 133 + 128] == "substitutions_by_position_second 0 16"
    per_lane = 4 + 2 * 129 + 4
    assert lines[per_lane:per_lane + 2] == ["sample_id S", "lane a"] and lines[per_lane + 4 + 128] == "substitutions_by_position_first 0 16"
    assert len(lines) == 2 * per_lane - 4 + 1 and lines[-1] == ""
