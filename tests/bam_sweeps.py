"""Two small BAM files (written with tests/pybam.py, BGZF blocks of 40 000 bytes) that put the readers' record rules
(bamqc_amd/host/bam_record.h) on every byte position at which the host reader and the reader on the card take different paths.

tag_sweep: the optional fields RG:Z, NM and AS in each of their six orders behind a padding field XA:Z with k = 0 .. 80 value
bytes (the field is 4 + k bytes; k = 0 is no field at all), so that the start of each of the three fields, its value bytes and
a string's NUL fall on every offset from 48 to 80 of the optional fields — across byte 64, where the card's LDS stage ends.  NM in
each of cCsSiI, AS in each of AcCsSiIf, an NM:Z that must be ignored, B arrays of every subtype and an H field astride byte 64.

size_sweep: about 4 000 records with names of 1 .. 254 characters and 0 .. 700 bases (some without bases, some without
qualities), sized so that record starts fall on every residue mod 4 and on each of the last 40 bytes of a 16 KiB segment of the
record stream (the card walks it in such segments), and three records of 20 000 / 40 000 bases: segments in which no record
starts, and plausibility chains that leave the bytes the card has staged.  Both properties are asserted here."""
import itertools
import struct

import numpy as np

from tests import pybam

REFS = [("chr1", 5_000_000), ("chr2", 3_000_000)]
LANES = ["A", "lane2", "a_longer_read_group_id"]
HEADER = "@HD\tVN:1.6\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % r for r in REFS) + "".join("@RG\tID:%s\tSM:S\n" % x for x in LANES)
SEG = 16384  # bamqc_amd/csrc/gpu_bam.hip: GB_SEG
_FMT = {"A": "<B", "c": "<b", "C": "<B", "s": "<h", "S": "<H", "i": "<i", "I": "<I", "f": "<f"}
_NM = {"c": -7, "C": 200, "s": -300, "S": 60_000, "i": -70_000, "I": 4_000_000_000}
_AS = {"A": ord("Q"), "c": -5, "C": 201, "s": -1234, "S": 60_001, "i": -100_000, "I": 3_000_000_000, "f": -37.75}


def _field(key, ty, value):
    return key + ty.encode() + struct.pack(_FMT[ty], value)


def _record(i, l_seq, tags, name=None, rng=None, no_qual=False):
    rng = rng or np.random.default_rng(i)
    return dict(rid=int(rng.integers(-1, 2)), pos=int(rng.integers(-1, 2_000_000)), mapq=int(rng.integers(0, 61)), flag=int(rng.integers(0, 4096)),
                rnext=int(rng.integers(-1, 2)), pnext=int(rng.integers(-1, 2_000_000)), tlen=int(rng.integers(-900, 900)), name=name or "t%d" % i,
                cigar=[(l_seq << 4) | 0] if l_seq else [], seq=rng.integers(0, 256, (l_seq + 1) // 2).astype(np.uint8),
                qual=np.full(l_seq, 0xFF, np.uint8) if no_qual else rng.integers(0, 42, l_seq).astype(np.uint8), l_seq=l_seq, tags=tags)


def tag_sweep(path, second_nm=False, cut_last=False):
    """Writes the file; returns the number of records.  second_nm: one record whose fields cross byte 64 gets a second NM tag (the
    card hands its batch over to the host decoder); cut_last: the last record's final field is cut short (corrupt tags)."""
    recs, starts, values = [], {"RG": set(), "NM": set(), "AS": set()}, {"RG": set(), "NM": set(), "AS": set(), "NUL": set()}
    orders = list(itertools.permutations(("RG", "NM", "AS")))
    for k in range(81):
        for o, order in enumerate(orders):
            i = len(recs)
            nm_ty, as_ty = "cCsSiI"[(k + o) % 6], "AcCsSiIf"[(k + 3 * o) % 8]
            f = {"RG": b"RGZ" + LANES[i % 3].encode() + b"\0", "NM": _field(b"NM", nm_ty, _NM[nm_ty] + i % 3), "AS": _field(b"AS", as_ty, _AS[as_ty] + i % 5)}
            tags = b"XAZ" + bytes(33 + (i + j) % 90 for j in range(k)) + b"\0" if k else b""
            if i % 3 == 0:
                tags += b"NMZ7\0"  # not an integer: ignored (QualityCheck.hpp:201-209)
            for key in order:
                starts[key].add(len(tags))
                values[key].update(range(len(tags) + 3, len(tags) + len(f[key])))
                if key == "RG":
                    values["NUL"].add(len(tags) + len(f[key]) - 1)
                tags += f[key]
            if second_nm and k == 50 and o == 0:
                tags += _field(b"NM", "C", 77)
            recs.append(_record(i, 10 + i % 7, tags))
    for key, at in list(starts.items()) + list(values.items()):  # each field's start, and its value bytes, on every offset 48 .. 80
        assert set(range(48, 81)) <= at, (key, sorted(set(range(48, 81)) - at))
    # arrays of every subtype and a hex string whose type byte, subtype, count and data lie astride byte 64
    for st, d in itertools.product("cCsSiIf", range(1, 9)):
        arr = b"XBB" + st.encode() + struct.pack("<i", 3) + struct.pack("<3" + _FMT[st][1], 1, 2, 3)
        i = len(recs)
        recs.append(_record(i, 9, b"XAZ" + b"p" * (64 - d - 4) + b"\0" + arr + b"RGZ" + LANES[i % 3].encode() + b"\0" + _field(b"NM", "C", d) + _field(b"AS", "s", -d)))
    for d in range(1, 9):
        i = len(recs)
        recs.append(_record(i, 9, b"XAZ" + b"p" * (64 - d - 4) + b"\0" + b"XHH1AE301F2\0" + _field(b"AS", "f", 2.5 + d) + b"RGZ" + LANES[i % 3].encode() + b"\0" + _field(b"NM", "S", 300 + d)))
    if cut_last:
        recs[-1]["tags"] = recs[-1]["tags"][:-5] + b"NMi\1\2"  # (in place of NM:S) an NM:i with two of its four value bytes
    pybam.write_bam(path, HEADER, REFS, recs, block=40000)
    return len(recs)


def _sized(i, size, rng, tags):
    """A record of exactly `size` bytes (block_size field included): the bases and the name's length are chosen to fit."""
    fixed = 4 + 32 + len(tags)
    for l_seq in sorted(range(0, 701), key=lambda x: abs(x - max(0, (size - fixed - 100) * 2 // 3))):
        l_name = size - fixed - (4 if l_seq else 0) - (l_seq + 1) // 2 - l_seq
        if 2 <= l_name <= 255:
            return _record(i, l_seq, tags, name="n" * (l_name - 1), rng=rng)
    raise AssertionError("no record of %d bytes" % size)


def size_sweep(path):
    """Writes the file; returns the number of records."""
    rng = np.random.default_rng(7)
    recs, starts, off = [], [], 0
    while len(recs) < 4000:
        i = len(recs)
        tags = b"RGZ" + LANES[i % 3].encode() + b"\0" + _field(b"NM", "C", i % 200) + _field(b"AS", "s", -(i % 3000))
        seg = off // SEG
        want = (seg + 1) * SEG - 1 - seg % 40 - off  # the next record is to start on one of the segment's last 40 bytes: each in turn
        if i in (1000, 2000, 3000):
            r = _record(i, (20_000, 40_000, 20_000)[i // 1000 - 1], tags, rng=rng)
        elif 70 <= want <= 1300:
            r = _sized(i, want, rng, tags)
        elif 1300 < want <= 2600:
            r = _sized(i, want // 2, rng, tags)
        else:
            r = _record(i, int(701 * rng.random() ** 2), tags, name="n" * int(1 + 254 * rng.random() ** 3), rng=rng, no_qual=i % 97 == 0)
        if i < 4:  # the extremes, whatever the draw
            r = _record(i, (0, 700, 0, 700)[i], tags, name="n" * (1, 254, 254, 1)[i], rng=rng, no_qual=i == 3)
        recs.append(r)
        starts.append(off)
        off += 4 + 32 + len(r["name"]) + 1 + 4 * len(r["cigar"]) + len(r["seq"]) + len(r["qual"]) + len(tags)
    assert {s % 4 for s in starts} == {0, 1, 2, 3}
    assert {SEG - 1 - s % SEG for s in starts} >= set(range(40)), sorted(set(range(40)) - {SEG - 1 - s % SEG for s in starts})
    assert {len(r["name"]) for r in recs} >= {1, 254} and {r["l_seq"] for r in recs} >= {0, 700}
    assert set(range(off // SEG)) - {s // SEG for s in starts}, "no segment without a record start"
    pybam.write_bam(path, HEADER, REFS, recs, block=40000)
    return len(recs)
