"""GPU: the inflate kernels (csrc/gpu_inflate.hip, gpu_inflate_wave.inc: all six variants, and k_inflate_resolve with its CRC) on
hand-built DEFLATE streams no zlib encoder emits (tests/deflate_build.py): distances up to 32 768, 48-bit symbols at every refill
phase, code sets with the largest second-level demand, degenerate code sets, block headers at every bit alignment — and streams
that are invalid by construction.  The expected bytes are the builder's own expansion of its tokens (checked against zlib in
tests/test_deflate_handbuilt_cpu.py)."""
import ctypes as C
import functools
import zlib

import numpy as np
import pytest

from bamqc_amd import _lib
from tests import deflate_build as db
from tests.hipmem import Hip
from tests.test_gpu_inflate import _launch_on_card, gi, kernel_variant, raw_deflate, run  # noqa: F401 (gi, kernel_variant: fixtures; every test runs through each kernel variant)

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def random_streams():
    out = []
    for seed in range(200):
        s, toks = db.random_stream(seed)
        out.append(("random/seed%d" % seed, s, db.expand(toks)))
    return out


@functools.lru_cache(maxsize=None)
def fillers():
    """small zlib-made blocks of odd sizes: the neighbours of the placement test"""
    rng = np.random.default_rng(41)
    datas = [bytes(rng.integers(0, 1 + 5 * (k % 50), n, dtype=np.uint8)) for k, n in enumerate((1, 2, 3, 5, 31, 33, 63, 65, 127, 257, 601, 4097, 0, 7, 1023))]
    return [(raw_deflate(d, 1 + k % 9), d) for k, d in enumerate(datas)]


@functools.lru_cache(maxsize=None)
def good_block():
    rng = np.random.default_rng(3)
    data = bytes(rng.integers(0, 9, 30000, dtype=np.uint8))
    return raw_deflate(data), data


def check_each(entries, got):
    """every stream's bytes; the failure message names all streams that differ"""
    o, wrong = 0, []
    for name, _, want in entries:
        if got[o:o + len(want)] != want:
            wrong.append(name)
        o += len(want)
    assert not wrong, "%d streams differ: %s" % (len(wrong), " ".join(wrong))
    assert o == len(got)


def launch_with_guard(streams, wants, crcs):
    """bqc_gpu_inflate_launch on device-resident operands with the output buffer — the blocks' outputs back to back and 64 spare bytes
    behind them — filled with 0xA5 beforehand: returns (status bits, all of it)."""
    fn = C.CDLL(_lib.LIB_PATH).bqc_gpu_inflate_launch
    fn.restype = None
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    n = len(streams)
    tab = np.zeros(n, dtype=[("coff", "<u8"), ("uoff", "<u8"), ("csize", "<u4"), ("usize", "<u4")])
    co = uo = 0
    for i, s in enumerate(streams):
        tab[i] = (co, uo, len(s), len(wants[i]))
        co += len(s)
        uo += len(wants[i])
    hip = Hip()
    try:
        d_comp = hip.put(np.frombuffer(b"".join(streams), np.uint8), extra=256)
        d_tab = hip.put(tab.view(np.uint8))
        d_crc = hip.put(np.array(crcs, np.uint32))
        d_out = hip.put(np.full(uo + 64, 0xA5, np.uint8), extra=4096)
        d_st = hip.put(np.zeros(16, np.uint32))
        d_tok = hip.put(np.zeros(uo // 32 + n + 64, np.uint32))
        d_ntok = hip.put(np.zeros(n + 16, np.uint32))
        fn(d_comp, d_tab, n, uo, d_out, d_crc, d_st, d_tok, d_ntok, None)
        assert hip.rt.hipDeviceSynchronize() == 0
        return int(hip.get(d_st, 4, np.uint32)[0]), hip.get(d_out, uo + 64).tobytes()
    finally:
        hip.free()


def test_legal_streams(gi):
    """The whole legal catalogue in one launch, random_stream(0..199) in one more: accepted, byte for byte the tokens' expansion."""
    for entries in (db.legal_streams(), random_streams()):
        rc, got = run(gi, [s for _, s, _ in entries], [len(w) for _, _, w in entries])
        check_each(entries, got)
        assert rc == 0


def test_placement_among_neighbours():
    """Every catalogue stream first, in the middle and last in a group of three blocks whose other two are small zlib-made fillers of
    odd sizes — the groups back to back in one launch, three launches: the neighbours' outputs abut the stream's, so a write past a
    block's end or before its start lands in a neighbour (or in the 64 spare bytes behind the last block, which keep their fill), and
    every block's start takes three different alignments.  With the CRC-32s checked on the card."""
    entries, fill = db.legal_streams(), fillers()
    for shift in range(3):
        seq, k = [], 0
        for i, e in enumerate(entries):
            f = []
            for _ in range(2):
                s, d = fill[k % len(fill)]
                k += 1
                f.append(("filler", s, d))
            place = (i + shift) % 3
            seq += f[:place] + [e] + f[place:]
        st, got = launch_with_guard([s for _, s, _ in seq], [w for _, _, w in seq], [zlib.crc32(w) & 0xFFFFFFFF for _, _, w in seq])
        assert got[-64:] == b"\xA5" * 64, "the spare bytes behind the last block were written (shift %d)" % shift
        o, wrong = 0, []
        for j, (name, _, want) in enumerate(seq):
            if got[o:o + len(want)] != want:
                wrong.append("%s (block %d; before it %s, behind it %s)" % (name, j, seq[j - 1][0] if j else "-", seq[j + 1][0] if j + 1 < len(seq) else "-"))
            o += len(want)
        assert not wrong, "shift %d, %d blocks differ: %s" % (shift, len(wrong), "; ".join(wrong))
        assert st == 0, shift


@pytest.mark.parametrize("name", [n for n, _, _ in db.illegal_streams()])
def test_illegal_streams_are_reported(gi, name):
    """Each illegal catalogue entry at index 33 of 70 good blocks: reported (the paths through k_inflate, k_inflate_lean and the wave
    kernel end in a status bit — code set checks before any table is filled, symbol checks before any byte is written)."""
    (bad, size), = [(s, n) for nm, s, n in db.illegal_streams() if nm == name]
    good, data = good_block()
    streams, sizes = [good] * 70, [len(data)] * 70
    streams[33], sizes[33] = bad, size
    rc, got = run(gi, streams, sizes)
    assert rc > 0
    o = 0
    for i in range(70):   # the good blocks around it are whole
        if i != 33:
            assert got[o:o + sizes[i]] == data, i
        o += sizes[i]


def test_crc_on_the_card():
    """The legal catalogue with its CRC-32s (inside k_inflate_resolve for two phases, k_gi_crc for one): status 0, identical bytes; one
    wrong CRC on a block whose every byte behind the first 32 768 comes from the farthest possible source: status 8."""
    entries = db.legal_streams()
    streams, wants = [s for _, s, _ in entries], [w for _, _, w in entries]
    crcs = [zlib.crc32(w) & 0xFFFFFFFF for w in wants]
    st, got = _launch_on_card(streams, wants, crcs)
    check_each(entries, got)
    assert st == 0
    k = [n for n, _, _ in entries].index("dist/full_block_fixed")
    assert len(wants[k]) == 65536
    bad = list(crcs)
    bad[k] ^= 0x00010000
    st, _ = _launch_on_card(streams, wants, bad)
    assert st == 8
