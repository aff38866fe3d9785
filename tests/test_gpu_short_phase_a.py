"""Parity of k_short's phase A (k_short.hip), the lane-per-read code that loads a tile's per-read columns together, then the contig's
tables and the ends of the CIGAR, and hands read_stats (read_stats.h) the values.  The batches sit where a load that was moved in front
of the test that used to guard it could leave its array or pick up the wrong value: a lone lane, a tile one short of full, a full tile, one
read over and a second chunk of one read; unmapped reads (rid -1, pos -1, no CIGAR) at both ends of the batch, so that the last read's
CIGAR offset is the end of the CIGAR array; a batch without any CIGAR word; reads on a contig whose reference was never set; secondary,
supplementary, duplicate and QC-failed reads between primary ones; CIGARs of 1, 2, 3 and 6 operations on both strands with a soft clip
in front, a soft clip behind, deletions and insertions (first word, last word, the inner walk, triplet-segment tiles); reads at position
0 and reads that end at the contig's last base; two read groups in turn.

Every batch is compared count for count with the oracle in this process (k_short<15>) and in one child with BQC_SHORT_XCD=1 (k_short<0>),
and the CPU half checks that the oracle accepts every batch, so that a GPU failure cannot hide behind an input the reference refuses."""
import functools
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

from bamqc_amd import _abi
from tests import synth
from tests.parity import run_gpu, run_oracle

P, PR, UNM, MUNM, REV, FIRST, LAST, SEC, QCF, DUP, SUPP = 0x1, 0x2, 0x4, 0x8, 0x10, 0x40, 0x80, 0x100, 0x200, 0x400, 0x800
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS4 = [P | PR | FIRST, P | PR | LAST, P | PR | FIRST | REV, P | PR | LAST | REV]  # both mates, both strands
REF_LEN = 40_000
L = 150

CIGARS = [  # 1, 2, 3 and 6 operations; every one spans 150 read bases
    [(150, "M")],
    [(10, "S"), (140, "M")],                                              # soft clip in front: cg[0]
    [(140, "M"), (10, "S")],                                              # soft clip behind: cg[ncig - 1]
    [(70, "M"), (2, "D"), (80, "M")],                                     # one inner word
    [(70, "M"), (1, "I"), (79, "M")],
    [(5, "S"), (40, "M"), (2, "D"), (50, "M"), (3, "I"), (52, "M")],      # four inner words, clip in front
    [(30, "M"), (1, "I"), (40, "M"), (3, "D"), (74, "M"), (5, "S")],      # four inner words, clip behind
]


def _ref_span(ops):
    return sum(n for n, c in ops if c in "MDN")


def _read(rng, ref, ops, flag, pos, rid=0, lane=0, mapq=60, as_=90):
    """A read that follows `ops` along `ref` from `pos` (clips and insertions: random bases), 1 % mismatches, 0.5 % N."""
    parts, p = [], pos
    for n, c in ops:
        if c == "M":
            parts.append(ref[p:p + n].astype(np.int64))
        if c in "IS":
            parts.append(rng.integers(0, 4, n))
        if c in "MDN":
            p += n
    codes = np.concatenate(parts)
    m = rng.random(len(codes)) < 0.01
    codes[m] = (codes[m] + rng.integers(1, 4, int(m.sum()))) % 4
    codes[rng.random(len(codes)) < 0.005] = 4
    seq = "".join("ACGTN"[int(c)] for c in codes)
    return synth.single_read(seq, rng.integers(15, 41, size=len(codes)).tolist(), ops, flag, pos=pos, rid=rid, mapq=mapq, as_=as_,
                             nm=sum(n for n, c in ops if c in "ID"), lane=lane)


def _unmapped(rng, flag, lane=0):
    """flag 0x4 with the mate flags, no contig, no position, no CIGAR"""
    seq = "".join("ACGT"[int(c)] for c in rng.integers(0, 4, L))
    return synth.single_read(seq, rng.integers(15, 41, size=L).tolist(), [], flag, pos=-1, rid=-1, mapq=0, tlen=0, nm=0, as_=0, lane=lane)


def _pos(rng, ops):
    return int(rng.integers(1, REF_LEN - _ref_span(ops) - 1))


def _plain(seed, n):
    """n reads of 150 M in one read group, mates and strands in turn (balanced mates: 960 reads fill a chunk)"""
    rng = np.random.default_rng(seed)
    ref = rng.integers(0, 4, size=REF_LEN).astype(np.uint8)
    recs = [_read(rng, ref, CIGARS[0], FLAGS4[i % 4], _pos(rng, CIGARS[0])) for i in range(n)]
    return synth.concat(recs), [ref], dict(n_refs=1, n_lanes=1, max_read_len=512)


def _unmapped_ends(seed, n=200):
    """the first and the last read unmapped; every CIGAR shape between them; two read groups in turn"""
    rng = np.random.default_rng(seed)
    ref = rng.integers(0, 4, size=REF_LEN).astype(np.uint8)
    recs = [_unmapped(rng, P | UNM | FIRST, lane=0)]
    for i in range(1, n - 1):
        ops = CIGARS[i % len(CIGARS)]
        recs.append(_read(rng, ref, ops, FLAGS4[(i // 2) % 4], _pos(rng, ops), lane=i % 2))
    recs.append(_unmapped(rng, P | UNM | LAST, lane=(n - 1) % 2))
    cols = synth.concat(recs)
    assert cols["n_cigar"][0] == 0 and cols["n_cigar"][-1] == 0 and cols["rid"][-1] == -1
    return cols, [ref], dict(n_refs=1, n_lanes=2, max_read_len=512)


def _no_cigar(seed, n=130):
    """no read has a CIGAR: the batch's CIGAR array is empty"""
    rng = np.random.default_rng(seed)
    ref = rng.integers(0, 4, size=REF_LEN).astype(np.uint8)
    recs = [_unmapped(rng, P | UNM | (FIRST if i % 2 == 0 else LAST) | (MUNM if i % 3 == 0 else 0), lane=i % 2) for i in range(n)]
    cols = synth.concat(recs)
    assert len(cols["cigar"]) == 0
    return cols, [ref], dict(n_refs=1, n_lanes=2, max_read_len=512)


def _unloaded_contig(seed, n=300):
    """Two contigs, the reference of contig 0 alone set: reads on both, four at a time, so that both mates and strands land on each.  The
    reference's run ends at a triplet-eligible read on a contig without a sequence (and at one that steps back to an earlier contig), so
    the reads on contig 1 carry an alignment score below 50, which keeps them out of the triplets and in every other count."""
    rng = np.random.default_rng(seed)
    ref = rng.integers(0, 4, size=REF_LEN).astype(np.uint8)
    recs = []
    for i in range(n):
        ops = CIGARS[i % len(CIGARS)]
        rid = (i // 4) % 2
        recs.append(_read(rng, ref, ops, FLAGS4[i % 4], _pos(rng, ops), rid=rid, lane=i % 2, as_=30 if rid else 90))
    return synth.concat(recs), [ref, None], dict(n_refs=2, n_lanes=2, max_read_len=512)


def _flag_mix(seed, n=400):
    """secondary, supplementary, duplicate and QC-failed reads between primary ones"""
    rng = np.random.default_rng(seed)
    ref = rng.integers(0, 4, size=REF_LEN).astype(np.uint8)
    extra = [0, SEC, 0, SUPP, 0, DUP, 0, QCF, 0, SEC | SUPP, DUP | QCF]
    recs = []
    for i in range(n):
        ops = CIGARS[(i // 3) % len(CIGARS)]
        recs.append(_read(rng, ref, ops, FLAGS4[(i // 2) % 4] | extra[i % len(extra)], _pos(rng, ops), lane=i % 2))
    return synth.concat(recs), [ref], dict(n_refs=1, n_lanes=2, max_read_len=512)


def _cigars(seed, n=700):
    """every CIGAR shape on both strands and both mates: 7 shapes x 4 flag sets x 25"""
    rng = np.random.default_rng(seed)
    ref = rng.integers(0, 4, size=REF_LEN).astype(np.uint8)
    recs = []
    for i in range(n):
        ops = CIGARS[i % len(CIGARS)]
        recs.append(_read(rng, ref, ops, FLAGS4[(i // len(CIGARS)) % 4], _pos(rng, ops), lane=i % 2))
    return synth.concat(recs), [ref], dict(n_refs=1, n_lanes=2, max_read_len=512)


def _contig_ends(seed, n=240):
    """reads at position 0 and reads whose last base is the contig's last: the triplet range is clamped at either end"""
    rng = np.random.default_rng(seed)
    ref = rng.integers(0, 4, size=REF_LEN).astype(np.uint8)
    recs = []
    for i in range(n):
        ops = CIGARS[(i // 3) % len(CIGARS)]
        ops = ops if ops[0][1] == "M" and ops[-1][1] == "M" else CIGARS[0]  # (a clip at the end in question would keep the range inside)
        pos = [0, REF_LEN - _ref_span(ops), _pos(rng, ops)][i % 3]
        recs.append(_read(rng, ref, ops, FLAGS4[(i // 3) % 4], pos, lane=i % 2))
    return synth.concat(recs), [ref], dict(n_refs=1, n_lanes=2, max_read_len=512)


# name -> (maker, the batch holds triplet-eligible reads)
BATCHES = {
    "reads_1": (lambda: _plain(2001, 1), True),        # a lone lane
    "reads_59": (lambda: _plain(2002, 59), True),      # a tile one short of full
    "reads_60": (lambda: _plain(2003, 60), True),      # a full tile
    "reads_61": (lambda: _plain(2004, 61), True),      # one read over
    "reads_961": (lambda: _plain(2005, 961), True),    # a second chunk that holds one read
    "unmapped_ends": (lambda: _unmapped_ends(2006), True),
    "no_cigar": (lambda: _no_cigar(2007), False),
    "unloaded_contig": (lambda: _unloaded_contig(2008), True),
    "flag_mix": (lambda: _flag_mix(2009), True),
    "cigars": (lambda: _cigars(2010), True),
    "contig_ends": (lambda: _contig_ends(2011), True),
}


@functools.lru_cache(maxsize=None)
def _made(name):
    return BATCHES[name][0]()


@functools.lru_cache(maxsize=None)
def _oracle(name):
    """the oracle's counts of a batch: computed once, shared by the CPU and the GPU test, never changed"""
    cols, refs, opts = _made(name)
    rc, want, _ = run_oracle([cols], refs, **opts)
    return rc, want


@pytest.mark.parametrize("name", list(BATCHES))
def test_oracle_accepts_the_batch(name):
    rc, want = _oracle(name)
    assert rc == 0
    n_lanes = _made(name)[2]["n_lanes"]
    trip = sum(int(want[i]["triplet"].sum()) for i in range(n_lanes))
    eight = sum(int(want[i]["eightmer"].sum()) for i in range(n_lanes))
    print("%s: triplet %d, eightmer %d" % (name, trip, eight))
    assert eight > 0, "the batch must count something"
    assert (trip > 0) == BATCHES[name][1]


_CHILD = r"""
import pickle, sys
sys.path.insert(0, sys.argv[1])
from tests import test_gpu_short_phase_a as t
from tests.parity import run_gpu
out = {}
for name in t.BATCHES:
    cols, refs, opts = t._made(name)
    rc, counts, _ = run_gpu([cols], refs, **opts)
    out[name] = (rc, counts)
pickle.dump(out, open(sys.argv[2], "wb"))
"""


@pytest.fixture(scope="module")
def runtime_mask_results(tmp_path_factory):
    """Every batch through k_short<0>: one child process with BQC_SHORT_XCD=1 (mask 15 | 16; the variable is read once per process)."""
    path = str(tmp_path_factory.mktemp("short_phase_a") / "child.pkl")
    env = dict(os.environ, BQC_SHORT_XCD="1")
    env.pop("BQC_SHORT_PARTS", None)
    out = subprocess.run([sys.executable, "-c", _CHILD, ROOT, path], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    return pickle.load(open(path, "rb"))


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(BATCHES))
def test_phase_a_matches_the_oracle(name, runtime_mask_results):
    assert "BQC_SHORT_PARTS" not in os.environ and "BQC_SHORT_XCD" not in os.environ  # this process runs k_short<15>
    cols, refs, opts = _made(name)
    rc_o, want = _oracle(name)
    rc_g, fixed, _ = run_gpu([cols], refs, **opts)
    rc_c, runtime = runtime_mask_results[name]
    assert (rc_o, rc_g, rc_c) == (0, 0, 0)
    d = _abi.diff_counts(want, fixed)
    assert not d, "k_short<15> against the oracle:\n" + "\n".join(d[:20])
    d = _abi.diff_counts(want, runtime)
    assert not d, "k_short<0> against the oracle:\n" + "\n".join(d[:20])
