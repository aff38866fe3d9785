"""Batches for tests/test_gpu_prepass_paths.py (TEST INFRASTRUCTURE): hand-made reads that take k_prep_reads' common path (at most one
CIGAR operation) or its deferred path (several operations), placed read by read inside a thread's quad of four consecutive reads."""
import functools

import numpy as np

from tests import synth

P, PR, REV, FIRST, LAST = 0x1, 0x2, 0x10, 0x40, 0x80
L = 150
REF_LEN = 40_000
BLOCK = 1024  # reads per workgroup of k_prep_reads; a thread owns four consecutive ones

# CIGARs of the deferred path, 150 read bases each
DEFERRED = [
    [(100, "M"), (50, "X")],                                          # two operations, the second a triplet segment
    [(145, "M"), (5, "S")],                                           # two operations, trailing clip
    [(40, "M"), (1, "I"), (60, "M"), (49, "X")],                      # exactly four words
    [(30, "M"), (2, "D"), (40, "M"), (1, "I"), (79, "M")],            # five: one word beyond the first four
    [(12, "M"), (1, "D")] * 5 + [(10, "M"), (80, "=")],               # twelve
    [(60, "M"), (10, "S"), (80, "M")],                                # a clip between two match operations: a second covered interval
    [(5, "S"), (140, "M"), (5, "S")],                                 # leading and trailing clips
    [(50, "M"), (2, "I"), (48, "M"), (3, "D"), (50, "M")],            # insertion and deletion
    [(7, "H"), (150, "M")],                                           # hard clip: no read bases
]
assert all(sum(n for n, c in ops if c in "MIS=X") == L for ops in DEFERRED)


@functools.lru_cache(maxsize=None)
def reference():
    return np.random.default_rng(9001).integers(0, 4, size=REF_LEN).astype(np.uint8)


def read(i, pos, ops, lane=0, rid=0, mapq=60, as_=90, length=L):
    """read number i of a batch: strand and mate from its index, bases from the reference (synth.single_read without its strings)"""
    codes = reference()[pos:pos + length]
    codes = np.concatenate([codes, np.zeros(length - len(codes), np.uint8)])
    flag = P | PR | (REV if (i // 2) & 1 else 0) | (FIRST if i & 1 == 0 else LAST)
    nm = sum(n for n, c in ops if c in "ID")
    return dict(flag=np.array([flag], np.uint16), mapq=np.array([mapq], np.uint8), lane=np.array([lane], np.uint8), rid=np.array([rid], np.int32),
                pos=np.array([pos], np.int32), tlen=np.array([300], np.int32), nm=np.array([nm], np.int32), as_=np.array([as_], np.int32),
                l_seq=np.array([length], np.uint32), n_cigar=np.array([len(ops)], np.uint16), seq=synth.pack_nibbles(synth.NIB[codes]),
                qual=((np.arange(length) + 7 * i) % 21 + 20).astype(np.uint8), cigar=synth.cigar_words(ops))


def common(i, pos, **kw):
    return read(i, pos, [(kw.get("length", L), "M")], **kw)


UNCLIPPED = [k for k, ops in enumerate(DEFERRED) if not any(c in "SH" for _, c in ops)]  # (eligible for triplets)


def deferred(i, pos, kind=None, **kw):
    return read(i, pos, DEFERRED[(i if kind is None else kind) % len(DEFERRED)], **kw)


def quad_positions(n_blocks):
    """(first read of the quad, pattern): every pattern of {common, deferred} over four reads (bit j set: read j deferred) at the start of
    a block and in the last whole quad of one"""
    out = {}
    for p in range(16):
        out[(p % n_blocks) * BLOCK] = p
        out[((p + 5) % n_blocks) * BLOCK + BLOCK - 4] = p
    return out


@functools.lru_cache(maxsize=None)
def pattern_batch(n_lanes=1, n_blocks=16, tail=3):
    """n_blocks * 1024 + tail reads in coordinate order.  The quads of quad_positions hold the 16 patterns; every other read is
    common, but for one in eight."""
    n = n_blocks * BLOCK + tail
    quads = quad_positions(n_blocks)
    assert len(quads) == 32
    rng = np.random.default_rng(9002)
    pos = np.sort(rng.integers(0, REF_LEN - 2 * L, size=n))
    recs = []
    for i in range(n):
        q0 = i - i % 4
        if q0 in quads:
            d = bool((quads[q0] >> (i % 4)) & 1)
        else:
            d = rng.random() < 0.125
        recs.append((deferred if d else common)(i, int(pos[i]), lane=i % n_lanes))
    cols = synth.concat(recs)
    # what the placement promises
    nc = cols["n_cigar"]
    for q0, p in quads.items():
        assert [int(nc[q0 + j] > 1) for j in range(4)] == [(p >> j) & 1 for j in range(4)]
    return cols


def take(cols, idx):
    """the reads idx (any order) of a column dict as a new one"""
    idx = np.asarray(idx, np.int64)
    l = cols["l_seq"].astype(np.int64)
    so = np.concatenate([[0], np.cumsum((l + 1) // 2)])
    qo = np.concatenate([[0], np.cumsum(l)])
    co = np.concatenate([[0], np.cumsum(cols["n_cigar"].astype(np.int64))])
    out = {}
    for k, v in cols.items():
        if k in ("seq", "qual", "cigar"):
            o = {"seq": so, "qual": qo, "cigar": co}[k]
            out[k] = np.concatenate([v[o[i]:o[i + 1]] for i in idx]) if len(idx) else v[:0]
        else:
            out[k] = v[idx]
    return out
