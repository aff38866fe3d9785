"""A bit-exact DEFLATE (RFC 1951) stream builder for tests: pure Python, sharing nothing with the product.  It writes what zlib's
encoder never does and other encoders (libdeflate, igzip, zopfli-style) legally do — distances up to 32 768, 15-bit length and
distance codes in the same block, sparse and degenerate code sets, block headers at every bit alignment — and, through the raw bit
writer, streams that are invalid in exactly one named way.  legal_streams() / illegal_streams() are the catalogues the inflate tests
run (tests/test_deflate_handbuilt_cpu.py, tests/test_gpu_inflate_handbuilt.py); random_stream(seed) is a seeded generator of
multi-block streams of the same kind.  Tokens: an int is a literal, (length, distance) a match."""
import functools
import heapq
import random
import struct
import zlib

PRE_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
# RFC 1951, 3.2.5: length symbols 257..285 and distance symbols 0..29 as (base, extra bits)
LEN_TAB = [(3 + i, 0) for i in range(8)] + [(((4 + (i & 3)) << ((i - 4) >> 2)) + 3, (i - 4) >> 2) for i in range(8, 28)] + [(258, 0)]
DIST_TAB = [(1 + i, 0) for i in range(4)] + [(((2 + (i & 1)) << ((i >> 1) - 1)) + 1, (i >> 1) - 1) for i in range(4, 30)]
FIXED_LL = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_D = [5] * 32
MAX_OUT = 65536
MAX_STREAM = 65536 + 64


class BitWriter:
    """Bits go out LSB first (RFC 1951, 3.1.1); Huffman codes are written starting from their most significant bit."""

    def __init__(self):
        self.buf = bytearray()
        self.acc = 0
        self.n = 0

    def bits(self, value, nbits):
        assert 0 <= value < (1 << nbits) or nbits == 0 and value == 0
        self.acc |= value << self.n
        self.n += nbits
        if self.n >= 64:
            k = self.n >> 3
            self.buf += (self.acc & ((1 << (8 * k)) - 1)).to_bytes(k, "little")
            self.acc >>= 8 * k
            self.n -= 8 * k

    def code(self, code, length):
        self.bits(_rev(code, length), length)

    def bit_length(self):
        return 8 * len(self.buf) + self.n

    def align(self):
        self.bits(0, -self.bit_length() & 7)

    def raw(self, data):
        assert self.bit_length() & 7 == 0
        k = self.n >> 3
        self.buf += self.acc.to_bytes(k, "little")
        self.acc = self.n = 0
        self.buf += data

    def getvalue(self):
        return bytes(self.buf) + self.acc.to_bytes((self.n + 7) >> 3, "little")


def _rev(code, length):
    r = 0
    for _ in range(length):
        r = (r << 1) | (code & 1)
        code >>= 1
    return r


def canonical(lengths):
    """[(code, length)] per symbol for a list of code lengths (RFC 1951, 3.2.2); length 0: no code."""
    count = [0] * 16
    for l in lengths:
        count[l] += 1
    count[0] = 0
    nxt, code = [0] * 16, 0
    for l in range(1, 16):
        code = (code + count[l - 1]) << 1
        nxt[l] = code
    out = []
    for l in lengths:
        out.append((nxt[l], l))
        if l:
            nxt[l] += 1
    return out


def kraft(lengths):
    """Sum of 2^-l in units of 2^-15: 32768 for a complete code."""
    return sum(1 << (15 - l) for l in lengths if l)


def length_symbol(length, via284=False):
    """(symbol, extra value, extra bits); 258 is symbol 285, or with `via284` symbol 284 + extra 31."""
    assert 3 <= length <= 258
    if length == 258 and not via284:
        return 285, 0, 0
    for s in range(27, -1, -1):
        if LEN_TAB[s][0] <= length:
            return 257 + s, length - LEN_TAB[s][0], LEN_TAB[s][1]


def dist_symbol(dist):
    assert 1 <= dist <= 32768
    n = (dist - 1).bit_length()
    s = dist - 1 if dist <= 4 else 2 * n - 2 + (((dist - 1) >> (n - 2)) & 1)
    assert DIST_TAB[s][0] <= dist < DIST_TAB[s][0] + (1 << DIST_TAB[s][1])
    return s, dist - DIST_TAB[s][0], DIST_TAB[s][1]


def expand(tokens):
    out = bytearray()
    for t in tokens:
        if isinstance(t, int):
            out.append(t)
        else:
            n, d = t
            assert 3 <= n <= 258 and 1 <= d <= len(out), (t, len(out))
            if d >= n:
                out += out[len(out) - d:len(out) - d + n]
            else:
                for _ in range(n):
                    out.append(out[-d])
    return bytes(out)


def used_symbols(tokens, via284=False):
    """(set of literal/length symbols incl. 256, set of distance symbols) the tokens need"""
    ll, dd = {256}, set()
    for t in tokens:
        if isinstance(t, int):
            ll.add(t)
        else:
            ll.add(length_symbol(t[0], via284)[0])
            dd.add(dist_symbol(t[1])[0])
    return ll, dd


def frequencies(tokens, via284=False):
    fl, fd = [0] * 286, [0] * 30
    fl[256] = 1
    for t in tokens:
        if isinstance(t, int):
            fl[t] += 1
        else:
            fl[length_symbol(t[0], via284)[0]] += 1
            fd[dist_symbol(t[1])[0]] += 1
    return fl, fd


def limited_lengths(freqs, maxlen):
    """Code lengths of a COMPLETE prefix code, none longer than `maxlen`, for the symbols with a frequency > 0 (Huffman's lengths, cut
    at maxlen and repaired along the Kraft sum).  A lone symbol gets a partner (its neighbour) so that the code is complete."""
    freqs = list(freqs)
    live = [s for s, f in enumerate(freqs) if f > 0]
    assert live and len(live) <= (1 << maxlen)
    if len(live) == 1:
        freqs[live[0] + 1 if live[0] + 1 < len(freqs) else live[0] - 1] = 1
        live = [s for s, f in enumerate(freqs) if f > 0]
    heap = [(freqs[s], s, (s,)) for s in live]
    heapq.heapify(heap)
    depth = dict.fromkeys(live, 0)
    while len(heap) > 1:
        fa, ka, a = heapq.heappop(heap)
        fb, kb, b = heapq.heappop(heap)
        for s in a + b:
            depth[s] += 1
        heapq.heappush(heap, (fa + fb, min(ka, kb), a + b))
    lens = {s: min(d, maxlen) for s, d in depth.items()}
    full = 1 << maxlen
    k = sum(1 << (maxlen - l) for l in lens.values())
    order = sorted(live, key=lambda s: (freqs[s], s))             # rarest first
    while k > full:                                               # over-subscribed by the cut: lengthen the rarest code that can still grow
        fits = [s for s in order if lens[s] < maxlen and (1 << (maxlen - lens[s] - 1)) <= k - full]
        s = fits[0] if fits else max((s for s in order if lens[s] < maxlen), key=lambda s: lens[s])
        k -= 1 << (maxlen - lens[s] - 1)
        lens[s] += 1
    while k < full:                                               # room left: shorten the most frequent code that fits the gap
        s = next(s for s in reversed(order) if lens[s] > 1 and (1 << (maxlen - lens[s])) <= full - k)
        k += 1 << (maxlen - lens[s])
        lens[s] -= 1
    out = [0] * len(freqs)
    for s, l in lens.items():
        out[s] = l
    assert kraft(out) == 32768
    return out


def second_level_entries(lengths, root):
    """Entries behind a root table of `root` bits: for every root prefix shared by longer codes, 2^(longest code under it - root) —
    the layout rule of a two-level table builder (zlib's inftrees / `enough`)."""
    longest = {}
    for code, l in canonical(lengths):
        if l > root:
            p = code >> (l - root)
            longest[p] = max(longest.get(p, 0), l)
    return sum(1 << (l - root) for l in longest.values())


def lengths_from_counts(counts, symbols, n):
    """A length list of n entries that gives counts[l] codes of length l to `symbols`, in their order (shortest codes first)."""
    out = [0] * n
    it = iter(symbols)
    for l in range(1, 16):
        for _ in range(counts[l]):
            out[next(it)] = l
    return out


def search_counts(n_symbols, root, seed, restarts, moves=4000, start=None):
    """A seeded search for per-length counts of a complete code of n_symbols with a large second-level demand at `root` bits (how
    the constants below were found): from `start` or random complete codes (leaf splitting), split-one-leaf / merge-two-leaves
    moves that keep the symbol count and the Kraft sum, taken when the demand does not fall."""
    rng = random.Random(seed)

    def demand(c):
        return second_level_entries([l for l in range(1, 16) for _ in range(c[l])], root)

    def rand_counts():
        c = [0] * 16
        c[0] = 1
        for _ in range(n_symbols - 1):
            l = rng.choice([l for l in range(15) if c[l]])
            c[l] -= 1
            c[l + 1] += 2
        return c
    best, best_d = None, -1
    for _ in range(restarts):
        c = list(start) if start else rand_counts()
        d = demand(c)
        for _ in range(moves):
            a = rng.choice([l for l in range(1, 15) if c[l]])           # split a leaf at a, merge two at b
            c2 = list(c)
            c2[a] -= 1; c2[a + 1] += 2
            b = rng.choice([l for l in range(2, 16) if c2[l] >= 2])
            c2[b] -= 2; c2[b - 1] += 1
            d2 = demand(c2)
            if d2 >= d:
                c, d = c2, d2
        if d > best_d:
            best, best_d = c, d
    best[0] = 0
    return best, best_d


# ---------------------------------------------------------------------------------------------------
# code-length sequences (RFC 1951, 3.2.7)
# ---------------------------------------------------------------------------------------------------
def cl_encode(seq, use=(16, 17, 18), barrier=None, rng=None):
    """The sequence of code lengths as code-length symbols [(symbol, extra value, extra bits)].  `use`: which of the repeat codes may
    appear; `barrier`: an index no run may cross (None: runs cross from the literal/length lengths into the distance lengths);
    `rng`: a run is taken with probability 1/2 only and gets a random admissible length."""
    out, i, n = [], 0, len(seq)
    while i < n:
        v = seq[i]
        end = n if barrier is None or i >= barrier else barrier
        run = 1
        while i + run < end and seq[i + run] == v:
            run += 1
        if rng is not None and rng.random() < 0.5:
            run = 1
        if v == 0 and run >= 11 and 18 in use:
            r = min(run, 138) if rng is None else rng.randint(11, min(run, 138))
            out.append((18, r - 11, 7)); i += r
        elif v == 0 and run >= 3 and 17 in use:
            r = min(run, 10) if rng is None else rng.randint(3, min(run, 10))
            out.append((17, r - 3, 3)); i += r
        elif i > 0 and seq[i - 1] == v and run >= 3 and 16 in use:
            r = min(run, 6) if rng is None else rng.randint(3, min(run, 6))
            out.append((16, r - 3, 2)); i += r
        elif run >= 4 and 16 in use:
            out.append((v, 0, 0)); i += 1
        else:
            out.append((v, 0, 0)); i += 1
    return out


class Stream:
    """A DEFLATE stream under construction: blocks through stored / fixed / dynamic, anything else through the bit writer `w`."""

    def __init__(self):
        self.w = BitWriter()

    def header(self, final, btype):
        self.w.bits(1 if final else 0, 1)
        self.w.bits(btype, 2)

    def stored(self, data, final=False):
        assert len(data) <= 65535
        self.header(final, 0)
        self.w.align()
        self.w.raw(struct.pack("<HH", len(data), len(data) ^ 0xFFFF) + bytes(data))
        return self

    def symbols(self, tokens, ll_lens, d_lens, via284=False):
        """the tokens and the end-of-block code, in the given code sets"""
        w = self.w
        llc, dc = canonical(ll_lens), canonical(d_lens)
        litcache, lcache, dcache = {}, {}, {}
        for t in tokens:
            if isinstance(t, int):
                e = litcache.get(t)
                if e is None:
                    c, l = llc[t]
                    assert l, "literal %d has no code" % t
                    e = litcache[t] = (_rev(c, l), l)
                w.bits(*e)
                continue
            n, d = t
            e = lcache.get(n)
            if e is None:
                s, xv, xb = length_symbol(n, via284)
                c, l = llc[s]
                assert l, "length symbol %d has no code" % s
                e = lcache[n] = (_rev(c, l) | (xv << l), l + xb)
            w.bits(*e)
            e = dcache.get(d)
            if e is None:
                s, xv, xb = dist_symbol(d)
                c, l = dc[s]
                assert l, "distance symbol %d has no code" % s
                e = dcache[d] = (_rev(c, l) | (xv << l), l + xb)
            w.bits(*e)
        c, l = llc[256]
        assert l
        w.code(c, l)
        return self

    def fixed(self, tokens, final=False, via284=False):
        self.header(final, 1)
        return self.symbols(tokens, FIXED_LL, FIXED_D, via284)

    def dynamic_header(self, ll_lens, d_lens, hlit=None, hdist=None, cl_syms=None, use=(16, 17, 18), cross=True, hclen19=False, rng=None,
                       pre_lens=None):
        """HLIT / HDIST / HCLEN, the code-length code (complete: limited_lengths over the code-length symbols' frequencies, unless
        `pre_lens` sets it by hand) and the code lengths.  hlit / hdist default to the trimmed counts; `cl_syms` replaces the
        run-length encoding of cl_encode."""
        ll_lens, d_lens = list(ll_lens), list(d_lens)
        if hlit is None:
            hlit = max(257, max(i + 1 for i, l in enumerate(ll_lens) if l))
        if hdist is None:
            hdist = max([1] + [i + 1 for i, l in enumerate(d_lens) if l])
        ll_lens += [0] * (hlit - len(ll_lens))
        d_lens += [0] * (hdist - len(d_lens))
        assert not any(ll_lens[hlit:]) and not any(d_lens[hdist:])
        seq = ll_lens[:hlit] + d_lens[:hdist]
        if cl_syms is None:
            cl_syms = cl_encode(seq, use, None if cross else hlit, rng)
        if pre_lens is None:
            f = [0] * 19
            for s, _, _ in cl_syms:
                f[s] += 1
            pre_lens = limited_lengths(f, 7)
        hclen = 19 if hclen19 else max(4, max(i + 1 for i, s in enumerate(PRE_ORDER) if pre_lens[s]))
        w = self.w
        w.bits(hlit - 257, 5); w.bits(hdist - 1, 5); w.bits(hclen - 4, 4)
        for i in range(hclen):
            w.bits(pre_lens[PRE_ORDER[i]], 3)
        pc = canonical(pre_lens)
        for s, xv, xb in cl_syms:
            assert pc[s][1], "code-length symbol %d has no code" % s
            w.code(*pc[s])
            w.bits(xv, xb)
        return self

    def dynamic(self, tokens, ll_lens, d_lens, final=False, via284=False, **header):
        self.header(final, 2)
        self.dynamic_header(ll_lens, d_lens, **header)
        return self.symbols(tokens, ll_lens, d_lens, via284)

    def bit_length(self):
        return self.w.bit_length()

    def getvalue(self):
        return self.w.getvalue()


def auto_lengths(tokens, maxlen=15, via284=False, extra_ll=(), extra_d=(), skew=None):
    """Code sets for the tokens: limited_lengths over their frequencies.  `extra_*`: symbols that get a code without being used;
    `skew`: a random.Random — frequencies are replaced by a steep geometric ladder in random order (15-bit codes for the rare ones).
    A block without matches gets the empty distance set, one with a single distance symbol the one-code set."""
    fl, fd = frequencies(tokens, via284)
    for s in extra_ll:
        fl[s] += 1
    for s in extra_d:
        fd[s] += 1
    if skew is not None:
        for f in (fl, fd):
            live = [s for s, x in enumerate(f) if x]
            skew.shuffle(live)
            for k, s in enumerate(live):
                f[s] = 1 << min(k, 40)
    ll = limited_lengths(fl, maxlen)
    nd = sum(1 for x in fd if x)
    d = [0] if nd == 0 else [1 if x else 0 for x in fd] if nd == 1 else limited_lengths(fd, maxlen)
    return ll, d


def lz_tokens(data, far=False, min_len=3, max_dist=32768, chain=8):
    """A small greedy LZ77 tokenizer over at most 65 280 bytes: a hash of 3-byte strings; `far`: the farthest usable match is preferred
    (the oldest occurrences are tried first) — distances up to 32 768, beyond what zlib's encoder ever emits."""
    data = bytes(data)
    n = len(data)
    assert n <= 65280
    table, out, p = {}, [], 0

    def insert(q):
        if q + 3 <= n:
            table.setdefault(data[q:q + 3], []).append(q)
    while p < n:
        best_n, best_d = 0, 0
        cands = table.get(data[p:p + 3]) if p + 3 <= n else None
        if cands:
            lo = 0
            while cands[lo] < p - max_dist:   # (positions ascend)
                lo += 1
                if lo == len(cands):
                    break
            pick = cands[lo:lo + chain] if far else cands[:-chain - 1:-1]
            for c in pick:
                if c < p - max_dist:
                    continue
                k = 3
                lim = min(258, n - p)
                while k < lim and data[c + k] == data[p + k]:
                    k += 1
                if k > best_n or (far and k == best_n and p - c > best_d):
                    best_n, best_d = k, p - c
                if far and best_n >= min_len:
                    break
        if best_n >= min_len:
            out.append((best_n, best_d))
            for q in range(p, p + best_n):
                insert(q)
            p += best_n
        else:
            out.append(data[p])
            insert(p)
            p += 1
    return out


def bgzf_member(stream, payload):
    """The stream as a BGZF member: header with BSIZE, CRC-32 and ISIZE of the payload."""
    bsize = 18 + len(stream) + 8
    assert bsize <= 65536
    return (bytes([31, 139, 8, 4, 0, 0, 0, 0, 0, 255, 6, 0, 66, 67, 2, 0]) + struct.pack("<H", bsize - 1) + stream +
            struct.pack("<II", zlib.crc32(payload) & 0xFFFFFFFF, len(payload)))


def member_stream(payload, rng):
    """A hand-built DEFLATE stream for a BGZF member's payload: lz_tokens with farthest-match preference, cut into 1-4 deflate
    blocks of dynamic codes from limited_lengths over skewed frequencies (15-bit codes), the one-code distance set where a block
    has a single distance class, the empty set where it has no match; now and then a fixed or a stored block between them."""
    toks = lz_tokens(payload, far=True)
    nb = 1 if len(toks) < 4 else rng.randint(1, 4)
    cuts = sorted(rng.randrange(len(toks) + 1) for _ in range(nb - 1)) + [len(toks)]
    s, last = Stream(), 0
    for k, cut in enumerate(cuts):
        part, final = toks[last:cut], k == len(cuts) - 1
        last = cut
        r = rng.random()
        if r < 0.1:
            s.fixed(part, final)
        elif r < 0.15 and all(isinstance(t, int) for t in part):
            s.stored(bytes(part), final)
        else:
            ll, d = auto_lengths(part, skew=rng if rng.random() < 0.7 else None)
            s.dynamic(part, ll, d, final, hclen19=rng.random() < 0.3, cross=rng.random() < 0.7)
    return s.getvalue()


# ---------------------------------------------------------------------------------------------------
# the catalogues
# ---------------------------------------------------------------------------------------------------
# per-length counts (lengths 0..15) of complete codes with a large second-level demand: 285 literal/length symbols behind a 9-bit root
# (the card's wave kernel: 340 entries possible) and behind an 11-bit root (the host decoder: 294 possible), 30 distance symbols behind
# an 8-bit root (both: 146 possible) — the values search_counts finds with the seeds noted, asserted in legal_streams()
COUNTS_LL_ROOT9 = [0, 0, 3, 1, 0, 3, 0, 2, 0, 0, 4, 7, 1, 0, 0, 264]      # (nearly all codes 15 bits long)
DEMAND_LL_ROOT9 = 328
COUNTS_LL_ROOT9B = [0, 1, 1, 0, 1, 1, 1, 0, 1, 0, 89, 49, 89, 17, 33, 2]  # search_counts(285, 9, 1, 3)
DEMAND_LL_ROOT9B = 336
COUNTS_LL_ROOT11 = [0, 1, 1, 1, 0, 3, 0, 0, 0, 0, 0, 0, 63, 77, 73, 66]   # search_counts(285, 11, 1, 3)
DEMAND_LL_ROOT11 = 290
COUNTS_D_ROOT8 = [0, 1, 1, 1, 1, 1, 0, 0, 1, 9, 9, 1, 1, 1, 1, 2]         # search_counts(30, 8, 1, 20, 1000)
DEMAND_D_ROOT8 = 144


def _rand_bytes(rng, n, lo=0, hi=256):
    return rng.randbytes(n) if (lo, hi) == (0, 256) else bytes(rng.randrange(lo, hi) for _ in range(n))


def _demand_block(counts, syms, rng, dist_lens=None):
    """tokens + code sets: a literal/length set with the given per-length counts over n_sym symbols (256 and the length symbols among
    them), every symbol of the set used at least once"""
    syms = list(syms)
    # the long (rare) codes go to most symbols; which symbol gets which length is shuffled, the end-of-block code included
    rng.shuffle(syms)
    ll = lengths_from_counts(counts, syms, 286)
    d = dist_lens if dist_lens is not None else limited_lengths([1] * 30, 15)
    dsyms = [s for s, l in enumerate(d) if l]
    toks = [s for s in range(256) if ll[s]]
    rng.shuffle(toks)
    lsyms = [s for s in range(257, 286) if ll[s]]
    for k in range(max(len(lsyms), len(dsyms))):                          # (the caller puts a 32 768-byte window in front: every distance is there)
        s, ds = lsyms[k % len(lsyms)], dsyms[k % len(dsyms)]
        base, xb = LEN_TAB[s - 257]
        dbase, dxb = DIST_TAB[ds]
        toks.append((base + (rng.randrange(1 << xb) if s != 284 else rng.randrange(31)), dbase + rng.randrange(1 << dxb)))
        toks.append(rng.choice([s for s in range(256) if ll[s]]))
    return toks, ll, d


@functools.lru_cache(maxsize=None)
def legal_streams():
    """[(name, stream, expected bytes)]: names are `group/what`; groups dist, sym48, dset, demand, struct."""
    rng = random.Random(20240611)
    out = []

    def add(name, s, toks_or_bytes):
        data = s.getvalue() if isinstance(s, Stream) else s
        want = toks_or_bytes if isinstance(toks_or_bytes, (bytes, bytearray)) else expand(toks_or_bytes)
        assert len(data) <= MAX_STREAM and len(want) <= MAX_OUT, (name, len(data), len(want))
        assert all(n != name for n, _, _ in out), name
        out.append((name, data, bytes(want)))

    # ---- dist: the farthest distances with the shortest and longest lengths, in fixed and dynamic blocks.  The window in front is a
    # stored block of random bytes (cheap to build); in the dynamic cases its last 300 bytes are literals of the match's own block.
    window = _rand_bytes(rng, 32768)
    for dist in (32768, 32767, 32507, 24577, 16385, 16384):
        for ln, via in ((3, False), (257, False), (258, False), (258, True)):
            tag = "d%d_l%d%s" % (dist, ln, "_via284" if via else "")
            pre = window[:dist]                                            # the match's source starts at byte 0
            toks = [(ln, dist), 7, (ln, dist), 9]
            s = Stream().stored(pre).fixed(toks, True, via)
            add("dist/fixed_" + tag, s, pre + expand(list(pre) + toks)[len(pre):])
            # dynamic: symbol 29 (or the distance's class) among 15-bit distance codes, the literals in the same block
            body = list(pre[dist - 300:]) + toks
            s = Stream().stored(pre[:dist - 300]).dynamic(body, *auto_lengths(body, via284=via, extra_d=range(30), skew=random.Random(dist + ln)), final=True, via284=via)
            add("dist/dynamic_" + tag, s, expand(list(pre) + toks))
    # a block of exactly 65 536 bytes: every byte behind the first 32 768 comes from the farthest possible source, the last match
    # ends on the last byte (destination ends at byte 65 535)
    for kind in ("fixed", "dynamic"):
        for via in (False, True):
            body = [(258, 32768)] * 126 + [(257, 32768), (3, 32768)]     # 126 * 258 + 257 + 3 = 32 768
            assert sum(t[0] for t in body) == 32768
            s = Stream().stored(window)
            if kind == "fixed":
                s.fixed(body, True, via)
            else:
                s.dynamic(body, *auto_lengths(body, via284=via, extra_d=(28, 29), extra_ll=(0, 1, 2)), final=True, via284=via)
            add("dist/full_block_%s%s" % (kind, "_via284" if via else ""), s, window + window)
    # the last match 0, 1, 2 and 3 bytes before the end of the block, lengths 3, 4 and 258 (the three-byte description's tail path), at an
    # output size that is and is not a multiple of four
    for tail in (0, 1, 2, 3):
        for ln in (3, 4, 258):
            for pad in (0, 1):
                pre = window[:32768 - pad]
                toks = [(ln, len(pre))] + [1 + k for k in range(tail)]
                add("dist/tail%d_l%d_pad%d" % (tail, ln, pad), Stream().stored(pre).fixed(toks, True), pre + pre[:ln] + bytes(1 + k for k in range(tail)))
    toks = [65, 66, 67] + [(258, 3)] * 253 + [(256, 3), (3, 3)]                     # 65 536 bytes out of three literals: the longest chains
    add("dist/full_block_distance3", Stream().fixed(toks, True), toks)

    # ---- sym48: consecutive 48-bit symbols (15-bit length code + 5 extra bits + 15-bit distance code + 13 extra bits), behind 0..63
    # literals of one bit each: the symbols at every phase of a 32-bit refill
    fl = [0] * 286
    fd = [0] * 30
    fl[0] = 1 << 30                                                       # literal 0: the one-bit code
    for k, s in enumerate([256] + list(range(1, 12))):
        fl[s] = 1 << (28 - 2 * k)
    for s in (281, 282, 283, 284):
        fl[s] = 1
    for k in range(20):
        fd[k] = 1 << (30 - k)
    fd[28] = fd[29] = 1
    ll48, d48 = limited_lengths(fl, 15), limited_lengths(fd, 15)
    assert ll48[0] == 1 and all(ll48[s] == 15 for s in (281, 282, 283, 284)) and d48[28] == 15 and d48[29] == 15
    r48 = random.Random(48)
    base48, n48 = [], 16385 + 63                                          # 300 of them behind a window of 16 385 bytes and up to 63 literals
    for k in range(300):
        ln = r48.choice((131, 132, 133, 162, 163, 194, 195, 226, 227, 257, 258)) if r48.random() < 0.3 else r48.randrange(131, 136)   # symbols 281..284 (258 through 284)
        if n48 + ln + 131 * (299 - k) > MAX_OUT:
            ln = 131
        base48.append((ln, r48.choice((16385, 16386, min(24576, n48 - 63), min(24577, n48 - 63), min(32767, n48 - 63), min(32768, n48 - 63), r48.randrange(16385, min(32768, n48 - 63) + 1)))))
        n48 += ln
    assert n48 <= MAX_OUT and all(dist_symbol(d)[0] >= 28 for _, d in base48) and all(281 <= length_symbol(n, True)[0] <= 284 for n, _ in base48)
    w48 = window[:16385]
    for lead in range(64):
        toks = [0] * lead + base48
        s = Stream().stored(w48).dynamic(toks, ll48, d48, True, via284=True)
        add("sym48/lead%02d" % lead, s, w48 + expand(list(w48) + toks)[16385:])
    # the same symbols behind 16 385 literals of the same block (no stored block in front)
    toks = [0, 1, 2, 3, 4] * 3277 + base48
    add("sym48/after_literals_same_block", Stream().dynamic(toks, ll48, d48, True, via284=True), toks)

    # ---- dset: distance code sets
    lits = list(_rand_bytes(rng, 40, 97, 123))
    pre = window
    far = [(3 + k % 40, DIST_TAB[k % 30][0] + ((1 << DIST_TAB[k % 30][1]) - 1) * (k & 1)) for k in range(120)]   # every class, lowest and highest extra value
    dmax = limited_lengths([1 << max(0, 29 - 2 * k) for k in range(30)], 15)                             # maximal lengths: a ladder down to 15 bits
    assert max(dmax) == 15
    toks = lits + far
    add("dset/max_lengths", Stream().stored(pre).dynamic(toks, auto_lengths(toks)[0], dmax, True), pre + expand(list(pre) + toks)[32768:])
    dlong = limited_lengths([1 << (40 - 5 * k) for k in range(7)] + [1] * 23, 15)                     # a ladder of seven short codes, 23 codes of 11 and 12 bits
    assert sum(1 for l in dlong if l > 8) >= 20, dlong
    add("dset/many_long_codes", Stream().stored(pre).dynamic(toks, auto_lengths(toks)[0], dlong, True), pre + expand(list(pre) + toks)[32768:])
    dlong7 = limited_lengths([1 << 24] + [1 << 20] * 2 + [1 << 12] * 3 + [16] * 8 + [1] * 16, 15)        # codes of 8 bits (longer than a 7-bit root, inside an 8-bit one) and longer
    add("dset/around_the_roots", Stream().stored(pre).dynamic(toks, auto_lengths(toks)[0], dlong7, True), pre + expand(list(pre) + toks)[32768:])
    for ds in (0, 5, 29):                                                                                  # the one-code set (incomplete by design)
        one = [0] * 30
        one[ds] = 1
        toks = lits + [(3 + k, DIST_TAB[ds][0] + k % (1 << DIST_TAB[ds][1])) for k in range(50)]
        for hd in sorted({ds + 1, 30}):
            add("dset/one_code_sym%d_hdist%d" % (ds, hd), Stream().stored(pre).dynamic(toks, auto_lengths(toks)[0], one, True, hdist=hd), pre + expand(list(pre) + toks)[32768:])
    toks = lits * 20
    for hd in (1, 30):                                                                                     # no distance code at all
        add("dset/empty_hdist%d" % hd, Stream().dynamic(toks, auto_lengths(toks)[0], [0] * hd, True, hdist=hd), toks)

    # ---- demand: second-level table demand
    n9 = second_level_entries([l for l in range(1, 16) for _ in range(COUNTS_LL_ROOT9[l])], 9)
    assert n9 == DEMAND_LL_ROOT9 >= 320, n9
    for k, (counts, root, want_demand) in enumerate(((COUNTS_LL_ROOT9, 9, DEMAND_LL_ROOT9), (COUNTS_LL_ROOT9B, 9, DEMAND_LL_ROOT9B), (COUNTS_LL_ROOT11, 11, DEMAND_LL_ROOT11))):
        assert sum(counts) == 285
        for rep in range(3):
            r = random.Random(900 + 10 * k + rep)
            syms = [s for s in range(286) if s != (285, 77, 0)[rep]]      # 285 of the 286 symbols: all but one, the end-of-block code always among them
            toks, ll, d = _demand_block(counts, syms, r, dist_lens=None if rep < 2 else lengths_from_counts(COUNTS_D_ROOT8, list(range(30)), 30))
            assert second_level_entries(ll, root) == want_demand
            used = used_symbols(toks)
            assert all(s in used[0] for s in range(286) if ll[s]) and all(s in used[1] for s in range(30) if d[s])
            add("demand/ll_root%d_%d_%d" % (root, want_demand, rep), Stream().stored(pre).dynamic(toks, ll, d, True), pre + expand(list(pre) + toks)[32768:])
    dl = lengths_from_counts(COUNTS_D_ROOT8, list(range(30)), 30)
    assert second_level_entries(dl, 8) == DEMAND_D_ROOT8
    for rep in range(3):
        r = random.Random(950 + rep)
        syms = list(range(30))
        r.shuffle(syms)
        dl = lengths_from_counts(COUNTS_D_ROOT8, syms, 30)
        toks = []
        for ds in range(30):
            for xv in (0, (1 << DIST_TAB[ds][1]) - 1):
                toks.append((3 + r.randrange(256), DIST_TAB[ds][0] + xv))
        r.shuffle(toks)
        toks = lits + toks
        add("demand/d_root8_%d" % rep, Stream().stored(pre).dynamic(toks, auto_lengths(toks)[0], dl, True), pre + expand(list(pre) + toks)[32768:])

    # ---- struct: block structure
    small = list(_rand_bytes(rng, 30, 65, 70))
    smalld = small + [(5, 7), (3, 1), 66, (30, 20)]
    for padbits in range(8):
        for kind in ("stored", "fixed", "dynamic"):
            # an empty non-final fixed block is 10 bits, a literal of the fixed code 8 or 9: k empty blocks move the next header by 2k bits
            # (mod 8), a nine-bit literal (>= 144) by one more
            s = Stream()
            lead = [200] if padbits & 1 else []                            # 3 + 9 + 7 = 19 bits, or 3 + 7 = 10
            s.fixed(lead, False)
            while (s.bit_length() & 7) != padbits:
                s.fixed([], False)
                assert s.bit_length() < 200
            want = list(lead)
            if kind == "stored":
                s.stored(bytes(small)); want += small
            elif kind == "fixed":
                s.fixed(smalld); want += smalld
            else:
                s.dynamic(smalld, *auto_lengths(smalld)); want += smalld
            mid = [70, 71, (4, 2)]
            s.fixed(mid, False); want += mid                               # then a stored block in mid-stream after that alignment
            s.stored(b"mid-stream stored")
            want2 = expand(want) + b"mid-stream stored"
            s.dynamic(smalld, *auto_lengths(smalld), final=True)
            add("struct/align%d_%s" % (padbits, kind), s, want2 + expand(list(want2) + smalld)[len(want2):])
    s, want = Stream(), []                                                 # 60 tiny blocks of mixed kinds
    for k in range(60):
        part = [65 + (k + j) % 26 for j in range(1 + k % 5)] + ([(3 + k % 9, 1 + k % 4)] if k % 3 else [])
        if k % 4 == 0 and all(isinstance(t, int) for t in part):
            s.stored(bytes(part), k == 59)
        elif k % 4 == 1 or k % 4 == 0:
            s.fixed(part, k == 59)
        elif k % 4 == 2:
            s.dynamic(part, *auto_lengths(part), final=k == 59, hclen19=bool(k & 8))
        else:
            s.dynamic(part, *auto_lengths(part, extra_ll=range(257, 286), extra_d=range(30), skew=random.Random(k)), final=k == 59, cross=True)
        want += part
    add("struct/sixty_tiny_blocks", s, want)
    s = Stream()
    for _ in range(200):
        s.fixed([], False)
    body = list(_rand_bytes(rng, 3000, 0, 5))
    body = lz_tokens(bytes(body))
    s.dynamic(body, *auto_lengths(body), final=True)
    add("struct/200_empty_fixed_then_data", s, body)
    s = Stream()
    for _ in range(59):
        s.fixed([], False)
    s.fixed([], True)
    add("struct/sixty_empty_fixed", s, b"")
    add("struct/stored_len0", Stream().stored(b"", True), b"")
    add("struct/stored_len0_between", Stream().fixed(small).stored(b"").stored(b"").fixed(small, True), small + small)
    add("struct/stored_len1", Stream().stored(b"Z", True), b"Z")
    big = _rand_bytes(rng, 65535)
    add("struct/stored_len65535", Stream().stored(big, True), big)
    add("struct/stored_len65535_then_literal", Stream().stored(big).fixed([33], True), big + b"!")
    add("struct/stored_after_fixed_bits", Stream().fixed([1, 2, 3]).stored(big[:65533], True), bytes([1, 2, 3]) + big[:65533])
    # blocks shorter than the wave's shortest piece (1024 bits), one after another, each with its own tables
    s, want = Stream(), []
    for k in range(25):
        part = list(_rand_bytes(random.Random(k), 20 + 3 * k, 97, 105)) + [(10 + k, 5 + k)]
        s.dynamic(part, *auto_lengths(part), final=k == 24)
        want += part
    add("struct/short_dynamic_blocks", s, want)
    # degenerate literal sets
    eob_only = [0] * 256 + [1]
    add("struct/eob_only_set", Stream().dynamic([], eob_only, [0], True), b"")
    add("struct/eob_only_set_then_data", Stream().dynamic([], eob_only, [0]).fixed(smalld, True), smalld)
    add("struct/eob_only_set_hlit286_hclen19", Stream().dynamic([], eob_only, [0], True, hlit=286, hdist=30, hclen19=True), b"")
    two = [0] * 257
    two[120] = 1; two[256] = 1
    add("struct/literal_and_eob", Stream().dynamic([120] * 500, two, [0], True), b"x" * 500)
    # HLIT = 286 with symbols 284 / 285 in use, HCLEN = 19
    toks = small + [(258, 3), (257, 5), (227, 9)]
    toks = toks + [(258, 4), (256, 6)]                                     # symbols 285 and 284 both in use
    ll, d = auto_lengths(toks)
    add("struct/hlit286_hclen19", Stream().dynamic(toks, ll, d, True, hlit=286, hdist=30, hclen19=True), toks)
    toks = toks[:-2]
    ll, d = auto_lengths(toks, via284=True, extra_ll=(285,))
    add("struct/hlit286_258_via284", Stream().dynamic(toks, ll, d, True, via284=True, hlit=286), toks)
    # code-length runs that cross from the literal lengths into the distance lengths: 16 (the last literal lengths equal the first
    # distance lengths), 17 and 18 (zeros on both sides of the boundary)
    toks = small + [(258, 3), (60, 1), (100, 2)]
    ll = [0] * 286
    for s in set(small) | {256}:
        ll[s] = 6
    for s in range(276, 286):
        ll[s] = 5                                                          # ten length symbols of 5 bits at the end of the literal set ...
    k = kraft(ll)
    spare = [s for s in range(200, 256)]
    while k < 32768:                                                       # (made complete with unused literal codes)
        s = spare.pop()
        l = 15 - min(14, (32768 - k).bit_length() - 1)
        ll[s] = l
        k += 1 << (15 - l)
    assert kraft(ll) == 32768
    d = [5] * 4 + [3] * 4 + [4] * 6                                         # ... and distance lengths that begin with 5s: one run of 16s over the boundary
    assert kraft(d) == 32768
    for use, name in (((16,), "16"), ((16, 17, 18), "all")):
        cl = cl_encode(ll + d, use)
        pos, crossing = 0, False
        for sym, xv, xb in cl:
            n = 1 if sym < 16 else 3 + xv if sym < 18 else 11 + xv
            crossing |= pos < 286 < pos + n and sym == 16
            pos += n
        assert crossing
        add("struct/run16_crosses_hlit_%s" % name, Stream().dynamic(toks, ll, d, True, hlit=286, use=use), toks)
    ll2 = limited_lengths([1 if s in small or s in (256, 257, 258) else 0 for s in range(259)], 15)
    toks2 = small + [(3, 1), (4, 30)]                                      # distance symbols 0 and 9: zeros at the start of the distance lengths
    d2 = [1] + [0] * 8 + [1]
    for use, name in (((17,), "17"), ((18,), "18"), ((16, 17, 18), "all")):
        ll3 = ll2 + [0] * (270 - len(ll2)) if name != "17" else ll2 + [0] * 3
        add("struct/zero_run_crosses_hlit_%s" % name, Stream().dynamic(toks2, ll3, d2, True, hlit=len(ll3), use=use), toks2)
    add("struct/no_run_codes", Stream().dynamic(toks2, ll2, d2, True, use=()), toks2)
    add("struct/runs_stop_at_hlit", Stream().dynamic(toks, ll, d, True, hlit=286, cross=False), toks)
    return out


def _pad_tail(s):
    """valid bits behind the defect: a final empty fixed block and a stored one, so that a decoder that reads on meets no second fault"""
    s.fixed([1, 2, 3], False)
    s.stored(b"tail", True)
    return s.getvalue()


@functools.lru_cache(maxsize=None)
def illegal_streams():
    """[(name, stream, claimed size)]: each stream is wrong in the one way its name says (zlib rejects it, or inflates it to another
    size than the claimed one)."""
    out = []
    body = [97, 98, 99, 100, (5, 2), (3, 4), 101, (4, 9)]
    n_body = len(expand(body))
    ll, d = auto_lengths(body)
    cl = cl_encode((ll + [0] * 286)[:max(257, max(i + 1 for i, l in enumerate(ll) if l))] + d[:max(i + 1 for i, l in enumerate(d) if l)])   # (as dynamic_header will encode them)
    f = [0] * 19
    for sym, _, _ in cl:
        f[sym] += 1
    pre = limited_lengths(f, 7)

    def add(name, s, size):
        out.append((name, s if isinstance(s, bytes) else _pad_tail(s), size))

    def shorter(lens, lo=2):   # one code one bit shorter: over-subscribed
        v = list(lens)
        i = max(range(len(v)), key=lambda i: (v[i] >= lo, -v[i]))
        assert v[i] >= lo
        v[i] -= 1
        assert kraft(v) > 32768
        return v

    def longer(lens, hi=15):    # one code one bit longer: incomplete
        v = list(lens)
        i = max(range(len(v)), key=lambda i: (0 < v[i] < hi, v[i]))
        assert 0 < v[i] < hi
        v[i] += 1
        assert kraft(v) < 32768
        return v
    # ---- code sets
    add("sets/precode_oversubscribed", Stream().dynamic(body, ll, d, pre_lens=shorter(pre)), n_body + 7)
    add("sets/precode_incomplete", Stream().dynamic(body, ll, d, pre_lens=longer(pre, 7)), n_body + 7)
    s = Stream()
    s.header(False, 2)
    s.w.bits(0, 5); s.w.bits(0, 5); s.w.bits(15, 4)                     # HLIT 257, HDIST 1, HCLEN 19; a precode of one one-bit code (symbol 0)
    for i in range(19):
        s.w.bits(1 if PRE_ORDER[i] == 0 else 0, 3)
    s.w.bits(0, 258)
    add("sets/precode_single_code", s, 7)
    add("sets/litlen_oversubscribed", Stream().dynamic(body, shorter(ll), d), n_body + 7)
    add("sets/litlen_incomplete", Stream().dynamic(body, longer(ll), d), n_body + 7)
    d3 = limited_lengths([4, 2, 1, 1] + [0] * 26, 15)
    body3 = [97, 98, 99, 100, (5, 1), (3, 2), 101, (4, 3), (3, 4)]
    ll3 = auto_lengths(body3)[0]
    add("sets/dist_oversubscribed", Stream().dynamic(body3, ll3, shorter(d3)), len(expand(body3)) + 7)
    add("sets/dist_incomplete", Stream().dynamic(body3, ll3, longer(d3)), len(expand(body3)) + 7)
    add("sets/dist_two_codes_incomplete", Stream().dynamic([97, 98, 99, 100, (5, 1), (3, 2)], auto_lengths(body3)[0], [1, 2]), 12 + 7)
    # ---- no end-of-block code: two literals of one bit each
    s = Stream()
    s.header(False, 2)
    two = [0] * 257
    two[97] = two[98] = 1
    s.dynamic_header(two, [0])
    s.w.bits(0b0110, 4)
    add("header/no_end_of_block_code", s, 4 + 7)
    # ---- repeat codes
    hl = max(257, max(i + 1 for i, l in enumerate(ll) if l))
    dt = d[:max(i + 1 for i, l in enumerate(d) if l)]
    full = ll[:hl] + dt
    assert full[:3] == [0, 0, 0] and full[-1] != 0
    s = Stream()
    s.header(False, 2)
    s.dynamic_header(ll[:hl], dt, cl_syms=[(16, 0, 2)] + cl_encode(full[3:]))   # (were "previous" zero before the first length, the block would be a good one)
    s.symbols(body, ll, d)
    add("header/repeat_in_first_position", s, n_body + 7)
    for sym, xv, xb, name in ((16, 0, 2, "16"), (17, 0, 3, "17"), (18, 0, 7, "18"), (18, 127, 7, "18_max")):
        s = Stream()
        s.header(False, 2)
        s.dynamic_header(ll[:hl], dt, cl_syms=cl_encode(full[:-1]) + [(sym, xv, xb)])   # the last length replaced by a run of 3 or more
        s.symbols(body, ll, d)
        add("header/repeat_%s_overruns" % name, s, n_body + 7)
    # ---- HLIT / HDIST beyond the alphabet
    for hlit in (287, 288):
        add("header/hlit_%d" % hlit, Stream().dynamic(body, ll, d, hlit=hlit), n_body + 7)
    for hdist in (31, 32):
        add("header/hdist_%d" % hdist, Stream().dynamic(body, ll, d, hdist=hdist), n_body + 7)
    # ---- symbols of the fixed code that are none
    fixed = canonical(FIXED_LL)
    for sym in (286, 287):
        s = Stream()
        s.header(False, 1)
        for t in (97, 98, 99):
            s.w.code(*fixed[t])
        s.w.code(*fixed[sym])
        s.w.bits(0, 5)                                                    # (what would be its distance code)
        s.w.code(*fixed[256])
        add("symbols/fixed_literal_%d" % sym, s, 3 + 3 + 7)
    for ds in (30, 31):
        s = Stream()
        s.header(False, 1)
        for t in (97, 98, 99):
            s.w.code(*fixed[t])
        s.w.code(*fixed[257])
        s.w.code(ds, 5)
        s.w.code(*fixed[256])
        add("symbols/fixed_distance_%d" % ds, s, 3 + 3 + 7)
    # ---- the unused pattern of a one-code distance set
    lits = [97, 98, 99, 100]
    ll1 = auto_lengths(lits + [(3, 1)])[0]
    c = canonical(ll1)
    for hd in (1, 30):
        s = Stream()
        s.header(False, 2)
        s.dynamic_header(ll1, [1], hdist=hd)
        for t in lits:
            s.w.code(*c[t])
        s.w.code(*c[257]); s.w.bits(0, 1)                                 # a good match first: distance 1, the set's one code
        s.w.code(*c[257]); s.w.bits(1, 1)                                 # then the pattern that is no code
        s.w.code(*c[256])
        add("symbols/one_code_distance_set_unused_pattern_hdist%d" % hd, s, 4 + 3 + 3 + 7)
    s = Stream()
    s.header(False, 2)
    s.dynamic_header(ll1, [0])
    for t in lits:
        s.w.code(*c[t])
    s.w.code(*c[257]); s.w.bits(0, 1)
    s.w.code(*c[256])
    add("symbols/match_with_the_empty_distance_set", s, 4 + 3 + 7)
    # ---- a distance one byte too far
    add("distance/too_far_in_the_first_block", Stream().fixed([97, 98, 99, (3, 4)]), 6 + 7)
    add("distance/too_far_in_a_later_block", Stream().fixed([97, 98, 99]).stored(b"defg").fixed([104, (4, 9), 105]), 3 + 4 + 6 + 7)
    add("distance/too_far_in_a_later_dynamic_block", Stream().fixed([97, 98, 99]).dynamic([104, (4, 5), 105], *auto_lengths([104, (4, 5), 105])), 3 + 6 + 7)
    win = random.Random(7).randbytes(32767)
    add("distance/32768_behind_32767_bytes", Stream().stored(win).fixed([(258, 32768)]), 32767 + 258 + 7)
    add("distance/32768_behind_32767_bytes_dynamic", Stream().stored(win[:32000]).dynamic(list(win[32000:]) + [(3, 32768)], *auto_lengths(list(win[32000:]) + [(3, 32768)], extra_d=range(30))),
        32767 + 3 + 7)
    # ---- sizes: a good stream, another size claimed
    good = Stream().stored(win[:100]).dynamic(body, ll, d, True).getvalue()
    add("size/claimed_one_more", good, 100 + n_body + 1)
    add("size/claimed_one_less", good, 100 + n_body - 1)
    good = Stream().stored(win).fixed([(258, 32767)] * 127, True).getvalue()
    add("size/claimed_one_less_ends_in_a_match", good, 32767 + 127 * 258 - 1)
    add("size/claimed_one_more_ends_in_a_match", good, 32767 + 127 * 258 + 1)
    return out


@functools.lru_cache(maxsize=None)
def random_stream(seed):
    """(stream, tokens): 1 to 5 blocks of mixed kinds over alphabets of 1 to 256 symbols, matches biased to the distance and length
    extremes, frequency skews that force 15-bit codes, coded-but-unused symbols, random use of the repeat codes and of HLIT / HDIST
    trimming.  Stored blocks appear as literal tokens."""
    rng = random.Random(seed * 7919 + 13)
    s, toks, n_out = Stream(), [], 0
    nb = rng.randint(1, 5)
    for b in range(nb):
        final = b == nb - 1
        kind = rng.choice(("stored", "fixed", "dynamic", "dynamic", "dynamic"))
        alpha = rng.sample(range(256), rng.randint(1, 256))
        if kind == "stored":
            n = rng.choice((0, 1, rng.randint(0, 200), rng.randint(0, 33000)))
            n = min(n, MAX_OUT - n_out)
            part = [rng.choice(alpha) for _ in range(n)]
            s.stored(bytes(part), final)
        else:
            part, budget = [], rng.choice((0, 1, 5, 50, 400, 1500))
            start = n_out
            for _ in range(budget):
                if n_out > start and rng.random() < 0.4:
                    ln = rng.choice((3, 4, 257, 258, 258, rng.randint(3, 258)))
                    dmax = min(n_out, 32768)
                    dist = rng.choice((1, 2, dmax, max(1, dmax - 1), rng.randint(1, dmax), DIST_TAB[rng.randrange(30)][0], DIST_TAB[rng.randrange(4, 30)][0] - 1))
                    if dist > dmax:
                        dist = dmax
                    if n_out + ln > MAX_OUT:
                        break
                    part.append((ln, dist)); n_out += ln
                else:
                    if n_out + 1 > MAX_OUT:
                        break
                    part.append(rng.choice(alpha)); n_out += 1
            n_out = start
            via = rng.random() < 0.5
            if kind == "fixed":
                s.fixed(part, final, via)
            else:
                extra_ll = rng.sample(range(286), rng.choice((0, 0, 3, 40, 286)))
                extra_d = rng.sample(range(30), rng.choice((0, 0, 2, 30)))
                ll, d = auto_lengths(part, via284=via, extra_ll=extra_ll, extra_d=extra_d, skew=rng if rng.random() < 0.6 else None)
                need_l = max(257, max(i + 1 for i, l in enumerate(ll) if l))
                need_d = max([1] + [i + 1 for i, l in enumerate(d) if l])
                use = tuple(c for c in (16, 17, 18) if rng.random() < 0.7)
                s.dynamic(part, ll, d, final, via, hlit=rng.choice((need_l, 286, rng.randint(need_l, 286))), hdist=rng.choice((need_d, 30, rng.randint(need_d, 30))),
                          use=use, cross=rng.random() < 0.7, hclen19=rng.random() < 0.3, rng=rng if rng.random() < 0.4 else None)
        toks += part
        n_out = len(expand(toks)) if part and not all(isinstance(t, int) for t in part) else n_out + len(part)
    data = s.getvalue()
    assert len(data) <= MAX_STREAM and n_out <= MAX_OUT
    return data, toks


def _find_counts():
    """(how COUNTS_LL_ROOT9B / COUNTS_LL_ROOT11 / COUNTS_D_ROOT8 were found: about fifteen seconds)"""
    return search_counts(285, 9, 1, 3), search_counts(285, 11, 1, 3), search_counts(30, 8, 1, 20, 1000)


