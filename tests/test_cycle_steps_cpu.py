"""CPU: what the step tests of the two per-cycle kernels stand on (tests/test_gpu_cycle_steps.py, tests/test_gpu_cycle_long_reads.py).

1. The vectorised restatements qbc_ref.table_fast and mbc_ref.table_fast equal the loop restatements bit for bit, on a batch made to
   meet every rule of the two definitions and on the scaled-down step batch: table_fast is trusted as far as this goes.
2. The constants of tests/cycle_steps.py are the kernels' (#define lines and the launchers' literals of k_qcyc.hip and k_mbc.hip): a
   change of one of them fails here instead of quietly emptying the layouts.
3. The step batch has the layout it claims, for cards of 2, 80, 256 and 304 CUs."""
import os
import re

import numpy as np
import pytest

from tests import cycle_steps as cs
from tests import mbc_ref, qbc_ref, synth

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bamqc_amd", "csrc")
OPS = "MIDNSHP=X"
TOP = (1 << 28) - 1


# ---------------------------------------------------------------------------------------------------------------------------
# 1. table_fast == table
# ---------------------------------------------------------------------------------------------------------------------------
def rule_batch(seed, n):
    """n reads in 3 read groups on three contigs (the first holds N, the second is never set): every CIGAR operation, operation
    lengths 0 and 2^28 - 1, CIGARs that consume more or less than l_seq or are absent, l_seq 0, 1 and 300, positions in front of the
    contig and over its end, rid -1 / unset / the second set contig, read codes N, = and M, qualities 0..255, every flag the rules
    name in every combination."""
    rng = np.random.default_rng(seed)
    ref0 = rng.integers(0, 4, 3000).astype(np.uint8)
    ref0[rng.choice(3000, 150, replace=False)] = 4
    refs = [ref0, None, rng.integers(0, 4, 1200).astype(np.uint8)]
    parts = []
    for i in range(n):
        L = int(rng.choice([0, 1, 2, 5, 16, 40, 150, 300], p=[.03, .05, .05, .1, .2, .27, .2, .1]))
        flag = 0x1
        for bit, p in ((0x4, .05), (0x10, .5), (0x40, .55), (0x80, .5), (0x100, .06), (0x800, .06), (0x8000, .05), (0x400, .1), (0x200, .05)):
            if rng.random() < p:
                flag |= bit
        rid = int(rng.choice([0, 2, 1, -1], p=[.6, .3, .05, .05]))
        length = len(refs[rid]) if rid in (0, 2) else 1000
        pos = int(rng.choice([rng.integers(0, length), rng.integers(-30, 3), length - rng.integers(0, 60)], p=[.8, .1, .1]))
        kind = rng.random()
        if kind < 0.05:
            ops = []
        elif kind < 0.4:
            ops = [(L + int(rng.integers(-3, 4)) if L > 3 else L + 1, "M")]  # one M: more, less or exactly l_seq
        else:
            ops = []
            for _ in range(int(rng.integers(1, 10))):
                u = rng.random()
                ops.append((0 if u < 0.05 else TOP if u < 0.08 else int(rng.integers(1, 60)), OPS[int(rng.integers(0, 9))]))
        nibs = rng.integers(0, 16, L)  # any code; mostly the contig's bases as they lie at pos
        if rid in (0, 2):
            at = pos + np.arange(L)
            on = (at >= 0) & (at < length) & (rng.random(L) < 0.9)
            nibs[on] = synth.NIB[refs[rid][at[on]]]
        parts.append(dict(flag=np.array([flag], np.uint16), mapq=np.array([30], np.uint8), lane=np.array([rng.integers(0, 3)], np.uint8),
                          rid=np.array([rid], np.int32), pos=np.array([pos], np.int32), tlen=np.array([0], np.int32), nm=np.array([0], np.int32),
                          as_=np.array([0], np.int32), l_seq=np.array([L], np.uint32), n_cigar=np.array([len(ops)], np.uint16),
                          seq=synth.pack_nibbles(nibs.astype(np.uint8)) if L else np.zeros(0, np.uint8),
                          qual=rng.integers(0, 256, L).astype(np.uint8), cigar=synth.cigar_words(ops).astype(np.uint32)))
    return synth.concat(parts), refs


@pytest.fixture(scope="module")
def rules():
    cols, refs = rule_batch(11, 2500)
    f, L = cols["flag"].astype(np.int64), cols["l_seq"].astype(np.int64)
    op, n = cols["cigar"] & 15, cols["cigar"] >> 4
    assert set(op.tolist()) == set(range(9)) and (n == 0).any() and (n == TOP).any()
    assert {0, 1, 300} <= set(L.tolist()) and (cols["n_cigar"] == 0).any()
    assert {-1, 0, 1, 2} == set(cols["rid"].tolist()) and (cols["pos"] < 0).any() and set(cols["lane"].tolist()) == {0, 1, 2}
    for bits in (0x100, 0x800, 0x900, 0x8000, 0x4, 0x10, 0x40, 0x80, 0xC0):
        assert ((f & bits) == bits).any(), hex(bits)
    assert ((f & 0xC0) == 0).any() and cols["qual"].max() == 255 and cols["qual"].min() == 0
    return cols, refs


@pytest.mark.parametrize("N", [100, 300, 400])  # below, at and above the longest read
def test_table_fast_is_table_on_every_rule(rules, N):
    cols, refs = rules
    H, T = qbc_ref.table(cols, 3, N), mbc_ref.table(cols, refs, 3, N)
    assert all(H[l, m].any() and T[l, m, t].any() for l in range(3) for m in range(2) for t in range(2))
    assert T[:, :, 1].sum() * 20 > T[:, :, 0].sum() > T[:, :, 1].sum() * 2  # (neither table is a trivial copy of the other)
    assert np.array_equal(qbc_ref.table_fast(cols, 3, N), H)
    assert np.array_equal(mbc_ref.table_fast(cols, refs, 3, N), T)


def test_table_fast_is_table_on_two_batches_and_on_none():
    a, refs = rule_batch(12, 400)
    b, _ = rule_batch(13, 300)
    assert np.array_equal(qbc_ref.table_fast([a, b], 3, 64), qbc_ref.table([a, b], 3, 64))
    assert np.array_equal(mbc_ref.table_fast([a, b], refs, 3, 64), mbc_ref.table([a, b], refs, 3, 64))
    assert np.array_equal(mbc_ref.table_fast([a, b], refs, 3, 64), mbc_ref.table_fast(a, refs, 3, 64) + mbc_ref.table_fast(b, refs, 3, 64))
    none = synth.slice_batch(a, 0, 0)
    assert not qbc_ref.table_fast(none, 3, 8).any() and not mbc_ref.table_fast(none, refs, 3, 8).any()
    empty = synth.single_read("", [], [], 0x1 | 0x40, pos=5)  # a batch of one read of length 0 without a CIGAR
    assert not qbc_ref.table_fast(empty, 3, 8).any() and not mbc_ref.table_fast(empty, refs, 3, 8).any()


@pytest.mark.parametrize("variant", ["short", "long"])
@pytest.mark.parametrize("N", [64, 300])
def test_table_fast_is_table_on_the_small_step_batch(variant, N):
    lay = cs.step_layout(2, variant, N)
    cols, ref = cs.step_batch(lay)
    H, T = qbc_ref.table(cols, 4, N), mbc_ref.table(cols, [ref], 4, N)
    assert np.array_equal(qbc_ref.table_fast(cols, 4, N), H)
    assert np.array_equal(mbc_ref.table_fast(cols, [ref], 4, N), T)


# ---------------------------------------------------------------------------------------------------------------------------
# 2. the constants
# ---------------------------------------------------------------------------------------------------------------------------
def defines(*names):
    """The integer #define lines of the files, evaluated (a value may be an expression over earlier ones)."""
    out = {}
    for name in names:
        for line in open(os.path.join(CSRC, name)):
            m = re.match(r"#define[ \t]+(\w+)[ \t]+(.+)", line)
            if not m:
                continue
            expr = re.sub(r"\b(0x[0-9A-Fa-f]+|\d+)[uU]?[lL]*\b", r"\1", m.group(2).split("//")[0].strip()).replace("/", "//")
            try:
                out[m.group(1)] = int(eval(expr, {"__builtins__": {}}, dict(out)))
            except Exception:
                pass  # (not an integer expression: no constant of ours)
    return out


def test_the_helper_states_the_kernels_constants():
    q = defines("kernels_common.h", "device_types.h", "k_qcyc.hip")
    m = defines("kernels_common.h", "device_types.h", "k_mbc.hip")
    assert (q["QC_STEP"], q["QC_C"], q["QC_U"], q["QC_THREADS"]) == (cs.QC_STEP, cs.ROW_CYCLES, cs.QC_U, 1024)
    assert (m["MB_STEP"], m["MB_RUNS"], m["MB_U"], m["MB_C"], m["MB_THREADS"]) == (cs.MB_STEP, cs.MB_RUNS, cs.MB_U, cs.ROW_CYCLES, 1024)
    assert q["BQC_FAST_MAXLEN"] == cs.FAST_MAXLEN and q["QC_QPAD"] == qbc_ref.QPAD and m["MB_QPAD"] == mbc_ref.QPAD
    assert cs.QC_STEP <= q["QC_THREADS"] and cs.MB_STEP <= m["MB_THREADS"]  # one thread fetches one read of a step
    # the launchers' literals: 256 reads per workgroup at the least, 64 rows at the most
    qsrc, msrc = open(os.path.join(CSRC, "k_qcyc.hip")).read(), open(os.path.join(CSRC, "k_mbc.hip")).read()
    assert "std::min((top + QC_C - 1) / QC_C, %du)" % cs.MAX_ROWS in qsrc
    assert "(w0 + %d) / %d)" % (cs.WG_READS - 1, cs.WG_READS) in qsrc and "(w1 + %d) / %d)" % (cs.WG_READS - 1, cs.WG_READS) in qsrc
    assert "std::min(n_cu, (b.n_reads + %du) / %du)" % (cs.WG_READS - 1, cs.WG_READS) in msrc
    assert "base += QC_STEP" in qsrc and "base += MB_STEP" in msrc and "slot >= MB_RUNS" in msrc


def test_the_restated_launches_on_shapes_worked_out_by_hand():
    # 70 000 short reads on 256 CUs (the largest batch of the older by-cycle tests): one step
    assert cs.mbc_launch(70_000, 256)["per"] == 274 and set(cs.mbc_launch(70_000, 256)["steps"]) == {1}
    q = cs.qcyc_launch(np.full(70_000, 20), 1024, 256)
    assert (q["rows"], q["g0"], q["g1"], q["per0"]) == (1, 256, 1, 274) and set(q["steps0"]) == {1}
    # a second step needs n_reads > STEP * n_cu
    assert set(cs.mbc_launch(768 * 256, 256)["steps"]) == {1} and max(cs.mbc_launch(768 * 256 + 1, 256)["steps"]) == 2
    assert set(cs.qcyc_launch(np.full(960 * 256, 20), 64, 256)["steps0"]) == {1} and max(cs.qcyc_launch(np.full(960 * 256 + 1, 20), 64, 256)["steps0"]) == 2
    # 300 reads of 2000 bases, N = 1024: 4 rows; 16 640 bases at N = 17 408: 64 rows, the last one 512 cycles wide
    q = cs.qcyc_launch(np.full(300, 2000), 1024, 256)
    assert (q["rows"], q["g0"], q["g1"], q["last_width"]) == (4, 2, 2, 256)
    q = cs.qcyc_launch([16_640, 100], 17_408, 256)
    assert (q["rows"], q["g0"], q["g1"], q["last_width"]) == (64, 1, 1, 512)
    assert cs.seams(2000, 2, 768) == [768, 1768] and cs.seams(700, 2, 768) == []
    # rounds: a thread of 3080 runs needs five rounds alone; 300 threads of 3 runs need two
    assert cs.mbc_rounds([3080], [0])[0] == 5 and len(cs.mbc_rounds([3080], [0])[1]) == 5
    bound, rounds = cs.mbc_rounds([3] * 300, [0] * 150 + [1] * 150)
    assert bound == 2 and rounds == [{0, 1}, {1}]
    # runs: M I M on the contig, a read cut by N on either strand, a read behind the contig, an unmapped one
    ref = np.zeros(100, np.uint8)
    reads = [synth.single_read("A" * 10, [30] * 10, [(4, "M"), (1, "I"), (5, "M")], 0x41, pos=3),
             synth.single_read("A" * 10, [30] * 10, [(4, "M"), (1, "D"), (6, "M")], 0x41, pos=3),
             synth.single_read("A" * 10, [30] * 10, [(4, "M"), (1, "D"), (6, "M")], 0x51, pos=3),
             synth.single_read("A" * 10, [30] * 10, [(10, "M")], 0x41, pos=100),
             synth.single_read("A" * 10, [30] * 10, [(10, "M")], 0x45, pos=3)]
    assert cs.mbc_runs(synth.concat(reads), [len(ref)], 64).tolist() == [2, 2, 2, 0, 0]
    assert cs.mbc_runs(synth.concat(reads), [len(ref)], 4).tolist() == [1, 1, 1, 0, 0]  # forward: cycles 0..3; reverse: stored 6..9


# ---------------------------------------------------------------------------------------------------------------------------
# 3. the step batch's layout
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_cu", [2, 80, 256, 304])
@pytest.mark.parametrize("variant", ["short", "long"])
def test_step_batch_layout(n_cu, variant):
    built = {}
    for N in (64, 300):
        lay = cs.step_layout(n_cu, variant, N)
        key = (lay["n"], lay["changes"])
        if key not in built:
            built[key] = cs.step_batch(lay)
        cols, ref = built[key]
        fewest = cs.assert_step_layout(lay, cols, len(ref))
        print("n_cu %d %s N %d: %s; fewest runs of a full k_mbc step %d" % (n_cu, variant, N, cs.describe(lay), fewest))
        H, T = qbc_ref.table_fast(cols, 4, N), mbc_ref.table_fast(cols, [ref], 4, N)
        assert all(H[l, m].any() and T[l, m, t].any() for l in range(4) for m in range(2) for t in range(2))
        assert lay["n"] - (2 * cs.QC_STEP * n_cu + 977) < 2 * cs.QC_STEP  # (grown by less than one share)
