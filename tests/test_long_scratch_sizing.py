"""CPU: k_long's scratch (a slot of 8-mer rows and a per-cycle tile per workgroup) is sized by bqc_create from the read-length
limit; the grid a launch has comes from the batch's longest generic read.  The launch must never have more workgroups than the
context allocated slots, for reads just below, at and above n_cu rows of 992 cycles, past 1024 rows, and for a refused read
longer than the limit.  Host functions of the library only: no GPU call."""
import ctypes

import pytest

from bamqc_amd import _lib

KL_ROW = 992  # cycles a row of k_long owns (k_long.hip)


def _fns():
    lib = _lib.load()
    slots, cap = lib.bqc_long_slots, lib.bqc_long_slots_cap
    slots.argtypes = [ctypes.c_uint32] * 4
    slots.restype = ctypes.c_uint32
    cap.argtypes = [ctypes.c_uint32] * 2
    cap.restype = ctypes.c_uint32
    return slots, cap


def _t8_cap(kl_cap, n_cu):  # bqc_create: the 8-mer slot table holds at least one k_long launch
    return max(1024, 4 * n_cu, kl_cap)


def _lengths(n_cu):
    out = [1_100_000]
    for n in (n_cu, 1024):
        out += [n * KL_ROW - 1, n * KL_ROW, n * KL_ROW + 1]
    return out


@pytest.mark.parametrize("n_cu", [256, 304, 80])
def test_a_launch_never_has_more_workgroups_than_the_context_allocates(n_cu):
    slots, cap = _fns()
    for L in _lengths(n_cu):
        for max_read_len in (L, L + 1, 1_200_000, 2_000_000):
            c = cap(max_read_len, n_cu)
            for n_chunks in (1, 7, n_cu, 1 << 20):
                s = slots(L, max_read_len, n_chunks, n_cu)
                assert 0 < s <= c, (L, max_read_len, n_chunks, s, c)
                assert s <= _t8_cap(c, n_cu)
        # one row per KL_ROW cycles, each with at least one workgroup: a read longer than n_cu rows needs more than n_cu slots
        rows = -(-L // KL_ROW)
        assert slots(L, L, 1 << 20, n_cu) == (rows if rows > n_cu else (n_cu // rows) * rows)
        assert cap(L, n_cu) == max(n_cu, rows)


@pytest.mark.parametrize("n_cu", [256, 304])
def test_a_refused_read_does_not_size_the_grid(n_cu):
    """A read longer than max_read_len is refused (k_prep), but its length is still the batch's upper bound: the grid stops at
    the limit, so the workgroups that start and exit at once stay inside the context's scratch too."""
    slots, cap = _fns()
    for max_read_len in (1024, 65536, 200_000):
        c = cap(max_read_len, n_cu)
        assert c == max(n_cu, -(-max_read_len // KL_ROW))
        for L in (300_000, 1_100_000, 0xFFFFFFFF):
            assert slots(L, max_read_len, 1 << 20, n_cu) <= c, (max_read_len, L)


def test_default_options_allocate_no_more_than_before():
    # the default limit (65 536 bases, 67 rows) keeps bqc_create's k_long scratch at one slot per CU
    _, cap = _fns()
    for n_cu in (80, 256, 304):
        assert cap(65536, n_cu) == n_cu
    assert cap(0xFFFFFFFF, 256) == -(-0xFFFFFFFF // KL_ROW)


def test_no_launch_without_generic_chunks():
    slots, _ = _fns()
    assert slots(1_100_000, 1_100_000, 0, 256) == 0
