"""CPU: the payload offsets of a batch come from two levels of sums (k_prep_sizes: inside groups of PR_GROUP blocks of 1024 reads, and
per group; k_prep_reads: the groups before its own).  bqc_prep_bases is that arithmetic on the host, step by step as the kernels do it
and through the same inline (prep.h): block totals in, bases and the first block whose inclusive end exceeds 32-bit offsets out.
Checked against a plain numpy.cumsum.  A batch with 4 GB of payload cannot be a GPU test: this is where the 32-bit rule is tested.
Host functions of the library only: no GPU call."""
import ctypes

import numpy as np
import pytest

from bamqc_amd import _lib

NONE = 0xFFFFFFFF
LIMIT = 0xFFFFFFFF  # the largest inclusive end a block may have


def _fns():
    lib = _lib.load()
    bases, group = lib.bqc_prep_bases, lib.bqc_prep_group
    bases.argtypes = [ctypes.POINTER(ctypes.c_uint64), ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint64)]
    bases.restype = ctypes.c_uint32
    group.argtypes = []
    group.restype = ctypes.c_uint32
    return bases, group()


def _run(totals):
    fn, _ = _fns()
    totals = np.ascontiguousarray(totals, dtype=np.uint64)
    out = np.full(totals.shape, 0xDEADBEEF, dtype=np.uint64)
    u64p = ctypes.POINTER(ctypes.c_uint64)
    bad = fn(totals.ctypes.data_as(u64p), totals.shape[0], out.ctypes.data_as(u64p))
    return out, bad


def _expect(totals):
    incl = np.cumsum(totals.astype(np.uint64), axis=0, dtype=np.uint64)
    excl = incl - totals.astype(np.uint64)
    over = np.nonzero((incl > LIMIT).any(axis=1))[0]
    return excl, (int(over[0]) if len(over) else NONE)


def _block_counts():
    g = _fns()[1]
    return [1, g - 1, g, g + 1, 3 * g + 5]


def test_group_is_a_power_of_two():
    g = _fns()[1]
    assert g >= 2 and g & (g - 1) == 0


@pytest.mark.parametrize("which", range(5))
def test_bases_are_the_exclusive_prefix_sums(which):
    n = _block_counts()[which]
    rng = np.random.default_rng(100 + which)
    # totals that differ per block and per quantity: ceil(L/2), L, n_cigar of 1024 reads of up to ~300 bases (far from the limit)
    totals = np.stack([rng.integers(1, 160_000, n), rng.integers(1, 320_000, n), rng.integers(0, 9_000, n)], axis=1).astype(np.uint64)
    got, bad = _run(totals)
    want, want_bad = _expect(totals)
    assert want_bad == NONE and bad == NONE
    assert np.array_equal(got, want)


def _totals_with_end(n, at, k, end, rng):
    """n blocks of differing totals whose inclusive end in quantity k is exactly `end` at block `at` (the other quantities stay small)"""
    t = np.stack([rng.integers(1, 1000, n), rng.integers(1, 1000, n), rng.integers(1, 1000, n)], axis=1).astype(np.uint64)
    before = int(t[:at, k].sum())
    assert end > before
    t[at, k] = end - before
    return t


def _places():
    g = _fns()[1]
    n = 3 * g + 5
    return n, {"first block of a group": 2 * g, "last block of a group": 2 * g - 1, "first block of the batch": 0,
               "last block of the batch": n - 1, "inside a group": g + 3}


@pytest.mark.parametrize("k", [0, 1, 2])
@pytest.mark.parametrize("place", ["first block of a group", "last block of a group", "first block of the batch", "last block of the batch", "inside a group"])
def test_an_inclusive_end_of_exactly_the_limit_is_allowed_and_one_more_is_refused_at_that_block(place, k):
    n, places = _places()
    at = places[place]
    rng = np.random.default_rng(7 * at + k)
    ok = _totals_with_end(n, at, k, LIMIT, rng)
    ok[at + 1:, k] = 0  # (nothing behind it in that quantity: the end stays at the limit)
    got, bad = _run(ok)
    want, want_bad = _expect(ok)
    assert want_bad == NONE and bad == NONE, (place, k, bad)
    assert np.array_equal(got, want)
    over = ok.copy()
    over[at, k] += 1  # 0x100000000
    got, bad = _run(over)
    want, want_bad = _expect(over)
    assert want_bad == at and bad == at, (place, k, bad)
    assert np.array_equal(got, want)  # (the bases stay the 64-bit sums: the batch fails, nothing wraps)


@pytest.mark.parametrize("k", [0, 1, 2])
def test_the_first_failing_block_is_reported_when_later_blocks_fail_too(k):
    g = _fns()[1]
    n = 3 * g + 5
    rng = np.random.default_rng(31 + k)
    t = np.stack([rng.integers(1, 1000, n)] * 3, axis=1).astype(np.uint64)
    t[g - 1, k] = 0xC0000000  # the last block of the first group: still fine
    t[g, k] = 0x50000000      # the first block of the second group: over, and so is every block behind it
    got, bad = _run(t)
    want, want_bad = _expect(t)
    assert want_bad == g and bad == g
    assert np.array_equal(got, want)


def test_one_block_over_on_its_own():
    for k in range(3):
        t = np.array([[5, 6, 7]], dtype=np.uint64)
        t[0, k] = 0x100000000
        got, bad = _run(t)
        assert bad == 0 and np.array_equal(got, np.zeros((1, 3), dtype=np.uint64))
        t[0, k] = LIMIT
        assert _run(t)[1] == NONE
