"""CPU: the oracle's StreamCounter (oracle/sketch_oracle.c) against the reference's own, compiled into oracle/_ref, at error rates
other than the default 0.01 — the table sizes the GPU sketch now runs: the 8192-counter floor (0.2), F2 tables smaller than 32768
entries (0.05) and larger ones (0.005, 0.002)."""
import ctypes as C
import os

import numpy as np
import pytest

from tests.oracle_lib import lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.path.join(ROOT, "oracle", "_ref", "libref_kmerstream.so")
u64p = C.POINTER(C.c_uint64)


@pytest.mark.skipif(not os.path.exists(REF), reason="oracle/_ref is only built where the reference sources exist")
@pytest.mark.parametrize("e", [0.2, 0.05, 0.005, 0.002])
def test_streamcounter_matches_compiled_reference_at_error_rate(e):
    L = lib()
    R = C.CDLL(REF)
    rng = np.random.default_rng(int(e * 1e6))
    h = rng.integers(0, 2 ** 64, size=4_000_000, dtype=np.uint64)  # enough distinct hashes that F0 / f1 stop after a few limits
    h[::3] = h[0]  # a heavy hitter: F2 far from sumCount
    h[1::7] = h[1::7] & np.uint64(0xFFFFFFFF00000000)  # low words of zero: the last level
    ra = (C.c_uint64 * 4)()
    rb = (C.c_uint64 * 4)()
    L.orc_streamcounter_run(C.c_double(e), h.ctypes.data_as(u64p), len(h), ra)
    R.ref_streamcounter_run(C.c_double(e), h.ctypes.data_as(u64p), len(h), rb)
    assert list(ra) == list(rb)
    assert ra[0] == len(h)
