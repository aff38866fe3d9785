"""SAM text files for the readers of SAM text (host: SamReader; card: csrc/gpu_sam.hip).

wild(path)      ~3000 lines of every form the readers decode alike, with the columns they must give (known by construction)
odd_lines()     lines the host decodes and the card hands over (its batch goes through the host's line parser)
bad_lines()     lines the host reader ends the run at, with its error code and message
boundary(path)  a short line slid byte by byte across 64 KiB boundaries (which are 16 KiB segment boundaries too), and a 100 kb read
"""
import numpy as np

NIB = "=ACMGRSVTWYHKDBN"
OPS = "MIDNSHP=X"
REFS = [("chr1", 400_000), ("chr2", 300_000), ("chr3", 50_000)]
LANES = ["L1", "L2"]


def header(pad_to=None):
    text = "@HD\tVN:1.6\tSO:unsorted\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % r for r in REFS) + "".join("@RG\tID:%s\tSM:S1\n" % x for x in LANES)
    if pad_to is not None:  # the first record line starts at this offset exactly
        fill = pad_to - len(text) - len("@CO\t\n")
        assert fill >= 0
        text += "@CO\t" + "x" * fill + "\n"
        assert len(text) == pad_to
    return text


def _i32(v):
    return int(np.array(v & 0xFFFFFFFF, np.uint32).view(np.int32))


def plain_line(rng, name, l_seq=150, lane=None):
    """An ordinary aligned read as a line (no line end)."""
    lane = int(rng.integers(0, len(LANES))) if lane is None else lane
    rid = int(rng.integers(0, len(REFS)))
    pos = int(rng.integers(1, REFS[rid][1] - l_seq))
    seq = "".join("ACGT"[x] for x in rng.integers(0, 4, size=l_seq))
    qual = bytes(rng.integers(33, 74, size=l_seq).astype(np.uint8)).decode()
    return "\t".join([name, str(int(rng.choice([99, 147, 83, 163]))), REFS[rid][0], str(pos), str(int(rng.integers(0, 61))), "%dM" % l_seq, "=", str(pos + 200), "350",
                      seq, qual, "RG:Z:" + LANES[lane], "NM:i:%d" % int(rng.integers(0, 5)), "AS:i:%d" % int(rng.integers(0, l_seq))])


def wild(path, seed=5, n=3000):
    """Writes the file; returns the columns of its records (flag as with every contig a main chromosome) as a dict of arrays."""
    rng = np.random.default_rng(seed)
    names = [r[0] for r in REFS]
    want = dict(flag=[], mapq=[], lane=[], rid=[], pos=[], tlen=[], nm=[], as_=[], l_seq=[], n_cigar=[], seq=[], qual=[], cigar=[])
    out = [header()]
    for i in range(n):
        kind = i % 25
        if kind == 3:
            out.append("\r\n" if i % 2 else "\n")  # an empty line
        if kind == 7:
            out.append("@CO\ta header line in mid-stream, line %d\n" % i)
        # SEQ / QUAL
        if kind == 1:
            l_seq, seq = 0, "*"
        else:
            l_seq = 1 if kind == 2 else 150 if kind == 4 else int(rng.integers(1, 200))
            alphabet = "ACGTN" if kind % 3 else "ACGTNacgtnRYKMSWBDHVrykm=."
            seq = "".join(alphabet[x] for x in rng.integers(0, len(alphabet), size=l_seq))
        if kind in (2, 4) or l_seq == 0 or kind == 5:
            qual, qbytes = "*", [0xFF] * l_seq
        else:
            q = rng.integers(33, 127, size=l_seq).astype(np.uint8)
            if l_seq == 1 and q[0] == ord("*"):
                q[0] = ord("I")
            qual, qbytes = bytes(q).decode(), list(q - 33)
        codes = [NIB.index(c.upper()) if c.upper() in NIB else 15 for c in (seq if l_seq else "")]
        if len(codes) % 2:
            codes.append(0)
        # CIGAR
        if kind == 6 or l_seq == 0:
            cig, words = "*", []
        else:
            words, cig = [], ""
            for _ in range(int(rng.integers(1, 6))):
                ln, op = int(rng.integers(0, 1 << 20)) if kind == 8 else int(rng.integers(1, 200)), int(rng.integers(0, 9))
                words.append((ln << 4) | op)
                cig += "%d%s" % (ln, OPS[op])
            if kind == 9:
                words.append((((1 << 28) - 1) << 4) | 0); cig += "%dM" % ((1 << 28) - 1)
        # numbers
        flag = int(rng.integers(0, 4096))
        flag_txt = str(flag)
        if kind == 10:  # ten digits: only the low 12 bits count
            flag_txt = str(9_999_990_000 + int(rng.integers(0, 9999)))
            flag = int(flag_txt) & 0xFFF
        rname = "*" if kind == 11 else "chrUnknown" if kind == 12 else names[int(rng.integers(0, 3))]
        rid = names.index(rname) if rname in names else -1
        pos = 0 if kind == 13 else int(rng.integers(1, 40_000))
        rnext = ["=", "*", "chrNowhere", names[int(rng.integers(0, 3))]][i % 4]
        rn = rid if rnext == "=" else names.index(rnext) if rnext in names else -1
        tlen = int(rng.integers(-2000, 2000))
        if kind == 14:
            tlen = int(rng.choice([-9_999_999_999, 9_999_999_999, 2_147_483_648, -2_147_483_649]))
        mapq = int(rng.integers(0, 256))
        # tags
        lane = int(rng.integers(0, 2))
        nm = int(rng.integers(0, 50)) if kind != 15 else None
        tags = ["RG:Z:" + LANES[lane]]
        if nm is not None:
            tags.append("NM:i:%d" % nm)
        as_kind = ["i", "A", "Z", "none", "neg", "Zi"][i % 6]
        as_val = 0x80000000
        if as_kind == "i":
            as_val = int(rng.integers(0, 300)); tags.append("AS:i:%d" % as_val)
        elif as_kind == "neg":
            as_val = -int(rng.integers(1, 300)); tags.append("AS:i:%d" % as_val)
        elif as_kind == "A":
            as_val = int(rng.integers(33, 127)); tags.append("AS:A:" + chr(as_val))
        elif as_kind == "Z":
            tags.append("AS:Z:high")
        elif as_kind == "Zi":
            tags += ["AS:Z:first", "AS:i:17"]  # (the first AS field of any type is decisive)
        junk = ["XA:Z:chr1,+100,50M,1;", "X:1", "ab", "", "NM:Z:7", "RGX", "XB:B:c,1,2,3", "NM:f:1.5", "R:Z:L2", "AS:i"]
        for _ in range(int(rng.integers(0, 4))):
            j = junk[int(rng.integers(0, len(junk)))]
            tags.insert(int(rng.integers(0, len(tags) + 1)) if j[:2] not in ("RG", "AS") else len(tags), j)
        if kind == 16:  # RG behind everything else
            tags.remove("RG:Z:" + LANES[lane]); tags.append("RG:Z:" + LANES[lane])
        if kind == 17:  # a second RG field is not looked at
            tags.append("RG:i:5")
        line = "\t".join(["w%d" % i, flag_txt, rname, str(pos), str(mapq), cig, rnext, "0", str(tlen), seq, qual] + tags)
        last = i == n - 1
        out.append(line + ("" if last else "\r\n" if kind in (18, 19) else "\n"))  # (no final newline)
        f = flag
        if rn >= 0:
            f |= 0x1000
        if l_seq > 0 and qual == "*":
            f |= 0x8000
        want["flag"].append(f); want["mapq"].append(mapq); want["lane"].append(lane); want["rid"].append(rid); want["pos"].append(pos - 1)
        want["tlen"].append(_i32(tlen)); want["nm"].append(-1 if nm is None else nm); want["as_"].append(_i32(as_val)); want["l_seq"].append(l_seq)
        want["n_cigar"].append(len(words)); want["cigar"] += words; want["qual"] += qbytes
        want["seq"] += [(codes[k] << 4) | codes[k + 1] for k in range(0, len(codes), 2)]
    with open(path, "w", newline="") as fh:
        fh.write("".join(out))
    dt = dict(flag=np.uint16, mapq=np.uint8, lane=np.uint8, rid=np.int32, pos=np.int32, tlen=np.int32, nm=np.int32, as_=np.int32, l_seq=np.uint32, n_cigar=np.uint16,
              seq=np.uint8, qual=np.uint8, cigar=np.uint32)
    return {k: np.array(v, np.int64).astype(dt[k]) for k, v in want.items()}


def odd_lines(rng):
    """[(what, line)]: lines the host reader decodes by rules the card does not have."""
    def edit(field, value, tags=None):
        f = plain_line(rng, "odd").split("\t")
        if field is not None:
            f[field] = value
        if tags is not None:
            f = f[:11] + tags
        return "\t".join(f)
    return [("second NM:i", edit(None, None, ["RG:Z:L1", "NM:i:3", "AS:i:40", "NM:i:9"])),
            ("AS:f", edit(None, None, ["RG:Z:L2", "NM:i:1", "AS:f:41.75"])),
            ("RG id not in the header", edit(None, None, ["RG:Z:newcomer", "NM:i:1", "AS:i:30"])),
            ("+5", edit(3, "+5")), (" 5", edit(4, " 5")), ("11 digits", edit(1, "12345678999"))]


def bad_lines(rng):
    """[(what, line, error code, message or its start)]: lines the host reader ends the run at."""
    f = plain_line(rng, "bad").split("\t")
    def with_(field, value):
        g = list(f); g[field] = value; return "\t".join(g)
    return [("fewer than 11 fields", "\t".join(f[:10]), 7, "corrupt SAM record (fewer than 11 fields)"),
            ("a bad CIGAR", with_(5, "75M3Q72M"), 7, "corrupt SAM record (CIGAR)"),
            ("digits behind the last CIGAR letter", with_(5, "75M3"), 7, "corrupt SAM record (CIGAR)"),
            ("a CIGAR of digits only", with_(5, "150"), 7, "corrupt SAM record (CIGAR)"),
            ("SEQ / QUAL lengths differ", with_(10, f[10][:-1]), 7, "corrupt SAM record (SEQ and QUAL differ in length)"),
            ("RG:i", "\t".join(f[:11] + ["RG:i:1", "NM:i:1", "AS:i:9"]), 1, "Read does not have Z"),
            ("no RG", "\t".join(f[:11] + ["NM:i:1", "AS:i:9"]), 1, "ERROR: read without RG tag (record "),
            ("NM:i:-1", "\t".join(f[:11] + ["RG:Z:L1", "NM:i:-1", "AS:i:9"]), 6, "NM tag value 0xFFFFFFFF is not representable")]


PROBE = "p\t99\tchr1\t100\t60\t8M\t=\t300\t208\tACGTACGT\tIIIIIIII\tRG:Z:L2\tNM:i:1\tAS:i:8\n"
BOUNDARY_FIRST = 17  # (the reader takes its first MiB in one piece: chunk boundaries exist from there on)


def boundary(path, seed=9):
    """The first record line starts at offset 16384 of the file, so that the segments of a window that holds the whole file begin at
    multiples of 16 KiB of the file, and with 64 KiB chunks every multiple of 64 KiB behind the first MiB is a chunk's end as well.  The
    probe line (70 bytes: its start, 11 tabs, three tags and its newline at different offsets) starts at B + 40 - s for s = 0 .. 149 around
    successive multiples B of 64 KiB: every byte of it lies on every offset of [B - 40, B + 40) once.  Lines in between are ordinary
    reads; the last but one line is a 100 kb read."""
    rng = np.random.default_rng(seed)
    out, at = [header(pad_to=16384)], 16384
    n_probe = len(PROBE) + 80
    k = 0
    for s in range(n_probe):
        target = (BOUNDARY_FIRST + s) * 65536 + 40 - s
        while target - at > 1500:
            line = plain_line(rng, "f%d" % k) + "\n"
            k += 1
            out.append(line); at += len(line)
        f = (plain_line(rng, "f%d" % k) + "\n").split("\t")  # the last one before the probe: its QNAME padded so that it ends exactly there
        k += 1
        pad = target - at - len("\t".join(f))
        assert pad >= 0
        f[0] += "_" * pad
        out.append("\t".join(f)); at = target
        out.append(PROBE); at += len(PROBE)
    L = 100_000
    seq = "".join("ACGT"[x] for x in rng.integers(0, 4, size=L))
    qual = bytes(rng.integers(33, 74, size=L).astype(np.uint8)).decode()
    # (121 operations, 486 characters: the CIGAR kernel's rounds of 256 characters hand their count on)
    cig = "".join("%d%s" % (n, op) for n, op in [(1000, "M"), (10, "I")] * 60 + [(39_400, "M")])
    out.append("\t".join(["long", "0", "chr1", "1000", "60", cig, "*", "0", "0", seq, qual, "RG:Z:L1", "NM:i:35", "AS:i:90000"]) + "\n")
    out.append(plain_line(rng, "last") + "\n")
    with open(path, "w", newline="") as fh:
        fh.write("".join(out))
    return n_probe
