"""GPU: the k-mer sketch's exported tables (bamqc_amd/csrc/sketch.hip: k_sketch, k_sketch_levels, k_sketch_export, k_sketch_import)
word by word against the oracle's StreamCounter dumped in the same layout (Oracle.sketch_state, tests/sketch_state.py).

The other sketch tests compare sumCount, F0, f1 and F2.  F0 and f1 read the zero and one counts of one level out of 32, so the counter
index of every other level, the level choice, every clamp to 15 and the saturated-level mask are invisible to them
(tests/test_sketch_state_cpu.py shows three such changes).  Here every word of the sketch block is compared: it is
the last n_lanes x n_pairs x words_per_sketch words of the state vector of a context without an optional module, [lane][pair] order.

What the library's contract makes of the cases:
* bqc_state_export flushes the context and a flushed context takes no further batch, so "the export after each batch" is the export of
  a context that took the batches up to that one, one context per prefix; the masks a later batch runs under are the same.
* bqc_state_import leaves the context flushed too: no batch can follow an import (asserted below), so the levels an import re-enables
  are never counted into again; what an import must get right is the saturating sum, which the export after it shows.
* the device path runs on a buffer of the HIP runtime the library is linked against (tests/hipmem.py), not on a torch tensor: torch's
  own runtime finds no GPU in a process that has used the card already.
Not here: level 31's clamp for a hash whose low word is zero (probability 2^-32 per hash: no input of a test's size reaches it), a
zero-length read, and sums over worker processes (one process and one multiply stand for them)."""
import numpy as np
import pytest

from bamqc_amd import Aggregator, BamQCError
from tests import sketch_state as ss
from tests import synth
from tests.long_layout import dna_ref
from tests.parity import split

pytestmark = pytest.mark.gpu
ERR_STATE = 8


def context(ref, **opts):
    a = Aggregator(**dict(ss.CONTEXT, **opts))
    a.set_reference(0, ref)
    return a


def sketch_block(a, opts):
    n = opts.get("n_lanes", 1) * len(opts["klist"]) * len(opts["qlist"]) * ss.sizes(opts["e"])[2]
    v = a.state_export_host()
    assert len(v) == a.state_words > n
    return v[len(v) - n:]


def compare(batches, ref, opts, what, before=()):
    """The helper of this file: the batches (after those of `before`) through a fresh context and a fresh oracle; every word of the
    exported sketch block against the oracle's.  -> (the block, the oracle)"""
    a, o = context(ref, **opts), ss.oracle(ref, **opts)
    for b in list(before) + list(batches):
        a.submit(b)
        assert o.process(b) == 0
    block = sketch_block(a, opts)
    a.close()
    ss.assert_block(block, o, opts.get("n_lanes", 1), len(opts["klist"]) * len(opts["qlist"]), opts["e"], what)
    return block, o


# ---------------------------------------------------------------------------------------------------------------------------
# 1. saturation across batches
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def saturation():
    batches, ref_len = ss.saturation_batches()
    ref = dna_ref(77, ref_len)
    o = ss.oracle(ref, **ss.SAT)
    states = []
    for b in batches:
        assert o.process(b) == 0
        states.append(o.sketch_state(0, 0))
    ss.assert_saturation_conditions(states)  # (before any GPU compare)
    return batches, ref, states


def test_saturation_across_batches(saturation):
    """After batch 1 the raw counts of level 0 (87 a counter) are clamped; batch 2 runs with level 0 masked off, batch 3 with levels 0
    and 1; level 2 ends with counters at 15 and below."""
    batches, ref, states = saturation
    for n in (1, 2, 3):
        block, o = compare(batches[:n], ref, ss.SAT, "after batch %d" % n)
        assert np.array_equal(block, states[n - 1])


# ---------------------------------------------------------------------------------------------------------------------------
# 2. read groups inside a workgroup
# ---------------------------------------------------------------------------------------------------------------------------
GROUPS = dict(klist=[32], qlist=[17], e=0.2, seed=1, n_lanes=3)


@pytest.fixture(scope="module")
def groups():
    """Three read groups: alternating read by read for 90 reads, then in runs of 1, 2, 700, 2, 700, 1, 700, 1 and 300 reads; 30 .. 300 bp,
    every other strand pattern.  A workgroup's 1024-read step holds reads of a foreign read group and flushes its LDS copy at a change."""
    rng = np.random.default_rng(31)
    lane = [i % 3 for i in range(90)]
    for g, run in ((0, 1), (1, 2), (2, 700), (0, 2), (1, 700), (2, 1), (0, 700), (1, 1), (2, 300)):
        lane += [g] * run
    n = len(lane)
    cols, ref_len = ss.random_reads(32, rng.choice([30, 31, 32, 33, 47, 48, 49, 100, 150, 255, 256, 300], n), lane=lane, rev=rng.random(n) < 0.5)
    return cols, dna_ref(77, ref_len)


def test_read_groups_one_batch_and_three(groups):
    cols, ref = groups
    one, o = compare([cols], ref, GROUPS, "one batch")
    assert all(ss.parse(o.sketch_state(l, 0), 0.2)[0] > 50_000 for l in range(3))
    three, o = compare(split(cols, [7, 1300]), ref, GROUPS, "three batches")
    assert np.array_equal(one, three)


def test_a_read_groups_mask_is_its_own(groups, saturation):
    """The same reads after a batch that saturated level 0 of read group 0 only: its mask must not suppress the increments of the
    other two (nor theirs be missing in a level that read group 0 no longer counts)."""
    cols, ref = groups
    first = saturation[0][0]  # (read group 0 throughout)
    ref = ref if len(ref) >= len(saturation[1]) else saturation[1]
    block, o = compare([cols], ref, GROUPS, "after a batch that filled level 0 of read group 0", before=[first])
    c = [ss.parse(o.sketch_state(l, 0), 0.2)[2] for l in range(3)]
    assert (c[0][0] == 15).all() and all((c[l][0] < 15).any() and (c[l][0] > 0).any() for l in (1, 2))


# ---------------------------------------------------------------------------------------------------------------------------
# 3. pairs and restarts
# ---------------------------------------------------------------------------------------------------------------------------
PAIRS = dict(klist=[1, 15, 16, 17, 31, 32, 33, 63], qlist=[0, 17, 60, 93, 94, 95, 100], e=0.2, seed=1, n_lanes=1)


def pairs_input():
    """3 000 reads of synth.synth(var_len, IUPAC codes, records without qualities) and 4 reads of every length k - 1, k, k + 1 (k of
    PAIRS; not 0) and 16 n - 1, 16 n, 16 n + 1 (n = 1 .. 9).  A fifth of the qualities are drawn from 0 .. 16: base by base in half of
    the reads (restarts inside every 16-base chunk), as one stretch in the others (k-mers of 63 bases survive beside it).  The other
    qualities of the stretch reads: all 94 in a third of them (the only reads that count for q 93 and 94), 61 .. 94 in another third
    (q 60), 17 .. 60 in the rest.  Both strands; each flag that excludes a read is present (a record without a mate flag is a secondary
    one: any other is an error of the whole batch); three reads are all N."""
    cols, refs = synth.synth(seed=51, n_reads=3000, n_refs=1, ref_len=60_000, var_len=True, p_iupac=0.03, p_noqual=0.02)
    lens = sorted({x for k in PAIRS["klist"] for x in (k - 1, k, k + 1) if x > 0} | {16 * n + d for n in range(1, 10) for d in (-1, 0, 1)})
    more, _ = ss.random_reads(52, np.repeat(lens, 4), rev=np.tile([False, True, True, False], len(lens)))
    more["pos"] = (int(cols["pos"].max()) + np.arange(len(more["pos"])) // 8).astype(np.int32)
    cols = synth.concat([cols, more])
    rng = np.random.default_rng(53)
    L = cols["l_seq"].astype(np.int64)
    n, end = len(L), np.cumsum(L)
    read = np.repeat(np.arange(n), L)           # the read of every quality byte
    at = np.arange(int(end[-1])) - np.repeat(end - L, L)  # its position in the read
    kind = rng.integers(0, 6, n)                # 0 .. 2: a fifth low base by base; 3: stretch + all 94; 4: stretch + 61 .. 94; 5: stretch + 17 .. 60
    q = cols["qual"].copy()
    hi = np.where(kind[read] == 3, 94, np.where(kind[read] == 4, rng.integers(61, 95, q.size), rng.integers(17, 61, q.size)))
    q = np.where(kind[read] >= 3, hi, q).astype(np.uint8)
    start = (rng.random(n) * 0.8 * L).astype(np.int64)
    low = np.where(kind[read] >= 3, (at >= start[read]) & (at < start[read] + (L[read] + 4) // 5), rng.random(q.size) < 0.2)
    q[low] = rng.integers(0, 17, int(low.sum()))
    noq = np.repeat((cols["flag"] & 0x8000) != 0, L)
    cols["qual"] = np.where(noq, 0xFF, q).astype(np.uint8)
    usable = np.flatnonzero((kind[:3000] == 3) & (L[:3000] >= 64) & ((cols["flag"][:3000] & 0x8F00) == 0))
    for r, f in zip(usable[:4], (0x100, 0x200, 0x400, 0x800)):
        cols["flag"][r] |= f
    cols["flag"][usable[4]] = (cols["flag"][usable[4]] & ~np.uint16(0xC0)) | 0x100  # (without 0x100 the batch is refused: bamqualcheck.cpp:385-389)
    seq_end = np.cumsum((L + 1) // 2)
    for r in usable[5:8]:                       # all N (a pad nibble stays 0)
        cols["seq"][seq_end[r] - (L[r] + 1) // 2:seq_end[r]] = 0xFF
        if L[r] & 1:
            cols["seq"][seq_end[r] - 1] = 0xF0
    for f in (0x100, 0x200, 0x400, 0x800, 0x10):
        assert (cols["flag"] & f).any()
    assert ((cols["flag"] & 0xC0) == 0).any() and (cols["qual"] <= 16).mean() > 0.18 and ((cols["qual"] >= 61) & (cols["qual"] <= 94)).any()
    return cols, refs[0]


def test_pairs_and_restarts():
    cols, ref = pairs_input()
    block, o = compare(split(cols, [1100]), ref, PAIRS, "56 pairs")
    filled = sum(int(w[0]) > 0 and bool(w[1:].any()) for w in block.reshape(56, -1))
    assert filled >= 50, filled


# ---------------------------------------------------------------------------------------------------------------------------
# 4. table sizes
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("e", [0.01, 0.0078])
def test_table_sizes(e):
    """e = 0.01: 32 768 F2 entries in LDS, 524 288 counters per level; e = 0.0078: 65 536 F2 entries, the global-F2 instantiation,
    1 048 576 counters per level.  Two read groups in runs of 500 reads, two batches."""
    f2, r, words = ss.sizes(e)
    assert (f2, r) == ((32768, 524288) if e == 0.01 else (65536, 1048576))
    cols, ref_len = ss.random_reads(41, np.full(4000, 150), lane=(np.arange(4000) // 500) & 1)
    compare(split(cols, [1700]), dna_ref(77, ref_len), dict(klist=[32], qlist=[17], e=e, seed=1, n_lanes=2), "e = %g" % e)


# ---------------------------------------------------------------------------------------------------------------------------
# 5. sums, import, reset
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def halves(saturation):
    """The first saturating batch cut in two: the exports vA, vB of two contexts that took a half each (whole vectors), the oracle's
    dump of each half and of both."""
    batches, ref, states = saturation
    parts = split(batches[0], [ss.SAT_READS // 2])
    vecs, dumps = [], []
    for p in parts:
        a = context(ref, **ss.SAT)
        a.submit(p)
        vecs.append(a.state_export_host())
        a.close()
        o = ss.oracle(ref, **ss.SAT)
        assert o.process(p) == 0
        dumps.append(o.sketch_state(0, 0))
        assert ss.describe(vecs[-1][-len(dumps[-1]):], dumps[-1], 0.2) is None
    return parts, ref, vecs, dumps, states[0]


def imported(ref, vec):
    m = context(ref, **ss.SAT)
    m.state_import_host(vec)
    return m


def test_import_of_a_sum_is_the_saturating_sum(halves):
    parts, ref, (va, vb), (da, db), both = halves
    ca, cb = ss.parse(da, 0.2)[2], ss.parse(db, 0.2)[2]
    assert ((ca[0] < 15) & (cb[0] < 15)).any() and (ss.parse(both, 0.2)[2][0] == 15).all()  # (level 0 fills only in the sum)
    m = imported(ref, va + vb)
    d = ss.describe(sketch_block(m, ss.SAT), both, 0.2)
    assert d is None, "import of vA + vB: " + d
    with pytest.raises(BamQCError) as ei:  # no batch follows an import (see the top of this file)
        m.submit(parts[0])
    assert ei.value.code == ERR_STATE
    m.close()


@pytest.mark.parametrize("n", [2, 17, 18, 64])
def test_import_of_n_equal_vectors(halves, n):
    """n workers that each counted the same reads: min(15, n c) per counter, n F2, n sumCount.  A byte per counter held 17 x 15; a 16-bit
    field holds 4 369 x 15."""
    parts, ref, (va, vb), (da, db), both = halves
    s, f2, c = ss.parse(da, 0.2)
    assert (c == 15).any() and (c == 1).any()
    want = ss.build(n * s, n * f2, np.minimum(15, n * c.astype(np.uint32)))
    m = imported(ref, np.uint64(n) * va)
    d = ss.describe(sketch_block(m, ss.SAT), want, 0.2)
    m.close()
    assert d is None, "import of %d x vA: %s" % (n, d)


def test_device_path_equals_host_path(halves):
    from tests.hipmem import Hip
    parts, ref, (va, vb), dumps, both = halves
    hip = Hip()
    a = context(ref, **ss.SAT)
    a.submit(parts[0])
    buf = hip.alloc(a.state_words * 8)
    a.state_export_device(buf.value)
    got = hip.get(buf, a.state_words * 8, np.uint64)
    assert np.array_equal(got, a.state_export_host()) and np.array_equal(got, va)
    a.close()
    m = context(ref, **ss.SAT)
    m.state_import_device(buf.value)
    again = m.state_export_host()
    m.close()
    hip.free()
    d = ss.describe(again[-len(dumps[0]):], dumps[0], 0.2)
    assert d is None, "device import, then export: " + d
    assert np.array_equal(again, va)


def test_reset_forgets_the_tables_and_the_mask(saturation):
    batches, ref, states = saturation
    a = context(ref, **ss.SAT)
    a.submit(batches[0])
    a.submit(batches[1])  # (levels 0 and 1 are masked off now)
    a.reset()
    assert not sketch_block(a, ss.SAT).any()
    a.reset()  # (the export flushed the context)
    a.submit(batches[2])
    block = sketch_block(a, ss.SAT)
    a.close()
    o = ss.oracle(ref, **ss.SAT)
    assert o.process(batches[2]) == 0
    want = o.sketch_state(0, 0)
    assert (ss.parse(want, 0.2)[2][0] == 15).all() and (ss.parse(want, 0.2)[2][1] > 0).all()
    d = ss.describe(block, want, 0.2)
    assert d is None, "one batch after reset: " + d
