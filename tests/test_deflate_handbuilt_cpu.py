"""Hand-built DEFLATE streams (tests/deflate_build.py) — what zlib's encoder never emits and other encoders legally do, and what zlib
rejects by construction — against zlib itself (the builder is checked first) and through the host decoder
(bamqc_amd/host/inflate_fast.cpp) with the guard bytes of tests/test_inflate.py."""
import random
import zlib

import pytest

from tests import deflate_build as db
from tests.test_inflate import inflate_raw

TRAILERS = (b"\xAA" * 8, b"\x00" * 8, b"\xFF" * 8)


def zlib_verdict(stream, size):
    """(accepted: the stream ends inside its bytes and yields `size` bytes, the bytes)"""
    d = zlib.decompressobj(-15)
    try:
        out = d.decompress(stream)
    except zlib.error:
        return False, b""
    return d.eof and len(out) == size, out


def test_catalogue_covers_every_group():
    names = [n for n, _, _ in db.legal_streams()]
    assert len(set(names)) == len(names)
    groups = {g: sum(1 for n in names if n.startswith(g + "/")) for g in ("dist", "sym48", "dset", "demand", "struct")}
    assert groups == {"dist": 77, "sym48": 65, "dset": 10, "demand": 12, "struct": 47}, groups
    assert all(len(s) <= 65536 + 64 and len(w) <= 65536 for _, s, w in db.legal_streams())
    assert len(db.illegal_streams()) == 34


def test_second_level_demands():
    """The second-level table demands the catalogue's code sets reach: literal/length behind a 9-bit root (the card's wave kernel,
    GW_LX 352: 340 possible) 328 and 336; behind the host decoder's 11-bit root (kLitEnough: 294 possible) 290; distance behind an
    8-bit root (both: 146 possible) 144.  Checked on the blocks' own code lengths in legal_streams(); here on the counts."""
    for counts, n, root, want in ((db.COUNTS_LL_ROOT9, 285, 9, 328), (db.COUNTS_LL_ROOT9B, 285, 9, 336), (db.COUNTS_LL_ROOT11, 285, 11, 290), (db.COUNTS_D_ROOT8, 30, 8, 144)):
        lens = [l for l in range(1, 16) for _ in range(counts[l])]
        assert len(lens) == n and db.kraft(lens) == 32768
        assert db.second_level_entries(lens, root) == want
    assert db.second_level_entries([l for l in range(1, 16) for _ in range(db.COUNTS_LL_ROOT9[l])], 9) >= 320
    # the rule itself on a code small enough to lay out by hand: root 2, codes 00 01 10 110 1110 1111 -> one shared prefix (11), longest 4
    assert db.second_level_entries([2, 2, 2, 3, 4, 4], 2) == 4
    assert db.second_level_entries([2, 2, 2, 3, 4, 4], 3) == 2
    assert db.second_level_entries([1, 2, 3, 3], 3) == 0


def test_builder_pieces():
    assert db.LEN_TAB[0] == (3, 0) and db.LEN_TAB[8] == (11, 1) and db.LEN_TAB[27] == (227, 5) and db.LEN_TAB[28] == (258, 0)
    assert db.DIST_TAB[0] == (1, 0) and db.DIST_TAB[4] == (5, 1) and db.DIST_TAB[29] == (24577, 13) and db.DIST_TAB[28] == (16385, 13)
    assert db.length_symbol(258) == (285, 0, 0) and db.length_symbol(258, True) == (284, 31, 5) and db.length_symbol(257) == (284, 30, 5)
    assert db.dist_symbol(32768) == (29, 8191, 13) and db.dist_symbol(24577) == (29, 0, 13) and db.dist_symbol(24576) == (28, 8191, 13) and db.dist_symbol(1) == (0, 0, 0)
    assert [c for c, _ in db.canonical([3, 3, 3, 3, 3, 2, 4, 4])] == [2, 3, 4, 5, 6, 0, 14, 15]   # RFC 1951, 3.2.2
    w = db.BitWriter()
    w.bits(1, 1); w.bits(1, 2); w.code(0, 7)                            # a final fixed block that holds the end-of-block code only
    assert w.bit_length() == 10 and w.getvalue() == b"\x03\x00" and zlib.decompress(w.getvalue(), -15) == b""
    w = db.BitWriter()
    w.code(0b110, 3)                                                    # a code's first bit goes out first: 1, 1, 0 from bit 0 upwards
    assert w.getvalue() == b"\x03"
    for f in ([5, 1], [1] * 19, [1 << k for k in range(30)], [3, 0, 0, 9, 0, 1]):
        for maxlen in (7, 15):
            lens = db.limited_lengths(f, maxlen)
            assert db.kraft(lens) == 32768 and max(lens) <= maxlen and all((l > 0) == (x > 0) for l, x in zip(lens, f))
    assert max(db.limited_lengths([1 << k for k in range(30)], 15)) == 15


def test_legal_streams_inflate_with_zlib_to_their_tokens():
    """The builder against zlib: every legal catalogue entry, and random_stream for seeds 0..299.  A stream zlib rejects is a builder
    bug."""
    for name, s, want in db.legal_streams():
        assert zlib.decompress(s, -15) == want, name
        assert zlib_verdict(s, len(want)) == (True, want), name
    for seed in range(300):
        s, toks = db.random_stream(seed)
        assert zlib.decompress(s, -15) == db.expand(toks), seed


def test_illegal_streams_are_rejected_by_zlib():
    for name, s, size in db.illegal_streams():
        if name.startswith("size/"):
            assert len(zlib.decompress(s, -15)) != size, name
        else:
            with pytest.raises(zlib.error):
                zlib.decompress(s, -15)
        assert zlib_verdict(s, size)[0] is False, name


def test_host_decoder_on_legal_streams():
    for name, s, want in db.legal_streams():
        for trailer in TRAILERS:
            ok, out = inflate_raw(s, len(want), trailer)
            assert ok == 1, name
            assert out == want, name


def test_host_decoder_on_random_streams():
    for seed in range(300):
        s, toks = db.random_stream(seed)
        want = db.expand(toks)
        for trailer in TRAILERS:
            ok, out = inflate_raw(s, len(want), trailer)
            assert ok == 1 and out == want, seed


def test_host_decoder_rejects_illegal_streams():
    for name, s, size in db.illegal_streams():
        for trailer in TRAILERS:
            ok, _ = inflate_raw(s, size, trailer)
            assert ok == 0, name


def test_tokenizer_round_trip():
    from tests.test_gpu_inflate import payloads
    saw_far = False
    for data in payloads():
        data = data[:65280]
        for far in (False, True):
            toks = db.lz_tokens(data, far=far)
            assert db.expand(toks) == data
            saw_far |= any(not isinstance(t, int) and t[1] > 32768 - 262 for t in toks)
    assert saw_far  # (beyond zlib's MAX_DIST)


def test_member_streams_round_trip():
    """The hand-built BGZF member kind of tests/pybam.py: farthest-match tokens in 1-4 deflate blocks, through zlib and the host decoder."""
    rng = random.Random(3)
    kinds = set()
    for k in range(12):
        data = bytes(rng.choice(b"ACGT\x00\x11\x22\xff") for _ in range(rng.choice((0, 1, 2, 700, 9000)))) + b"read%05d" % k * rng.randrange(40)
        s = db.member_stream(data, rng)
        assert zlib.decompress(s, -15) == data
        assert inflate_raw(s, len(data)) == (1, data)
        kinds.add(s[0] >> 1 & 3)
    assert 2 in kinds
