"""The adapter content by cycle (--adapter-by-cycle) restated from its definition in include/bamqc.h as a plain loop over the reads of a
column dict: decode the read to a string, reverse-complement it with 0x10, str.find per adapter.  Shares nothing with the kernel's
arithmetic (bamqc_amd/csrc/k_adp.hip).

The statistic.  Adapter set: 1 to 8 adapters, each a name (1 to 31 characters of [A-Za-z0-9_.-]) and a sequence (8 to 16 letters of
ACGT); BUILTIN when none is given.  A read is examined when flag & 0x900 == 0, flag & 0xC0 != 0, l_seq > 0 and lane < n_lanes; the
mate is 0 with 0x40, else 1; no quality, mapping or duplicate condition.  The base of cycle c of a read of length L is stored base c,
or the complement of stored base L-1-c with 0x10; stored codes 1, 2, 4, 8 are A, C, G, T and every other code matches nothing.
Adapter a of length m occurs at cycle c when c + m <= L and the bases of cycles c .. c+m-1 equal a letter for letter; its first hit
is the lowest such c.  For a capacity N, F[lane][mate][slot][c] counts the examined reads whose first hit of adapter `slot` is c (a
first hit at or behind N is not counted) and E[lane][mate][min(L,N)-1] the examined reads by length.  The words are
[n_lanes][2 mates][9 rows: slots 0..7, then E][N]; unused slots stay zero."""
import numpy as np

ROWS = 9
E_ROW = 8
CODES = "=ACMGRSVTWYHKDBN"
COMPLEMENT = str.maketrans("ACGT", "TGCA")  # (every other letter stays what it is: it matches nothing either way)
BUILTIN = [("Illumina_Universal", "AGATCGGAAGAG"), ("Illumina_SmallRNA_3p", "TGGAATTCTCGG"), ("Illumina_SmallRNA_5p", "GATCGTCGGACT"),
           ("Nextera_Transposase", "CTGTCTCTTATA"), ("PolyA", "AAAAAAAAAAAA"), ("PolyG", "GGGGGGGGGGGG")]


def _batches(cols_list):
    return [cols_list] if isinstance(cols_list, dict) else cols_list


def stored(cols, i, soff):
    """Read i of a column dict as a string over CODES, as stored."""
    L = int(cols["l_seq"][i])
    b = cols["seq"][soff:soff + (L + 1) // 2]
    return "".join(CODES[(int(b[j >> 1]) >> (0 if j & 1 else 4)) & 15] for j in range(L))


def table(cols_list, n_lanes, N, adapters=None):
    """T[lane][mate][row][c] over the batches: rows 0..7 the first hits F of the adapters, row 8 the reads by length E."""
    adapters = adapters or BUILTIN
    T = np.zeros((n_lanes, 2, ROWS, N), np.uint64)
    for cols in _batches(cols_list):
        L = cols["l_seq"].astype(np.int64)
        soff = np.cumsum((L + 1) // 2) - (L + 1) // 2
        for i, f in enumerate(cols["flag"].astype(np.int64)):
            lane = int(cols["lane"][i])
            if f & 0x900 or not f & 0xC0 or L[i] == 0 or lane >= n_lanes:
                continue
            s = stored(cols, i, int(soff[i]))
            if f & 0x10:
                s = s[::-1].translate(COMPLEMENT)
            mate = 0 if f & 0x40 else 1
            for slot, (name, seq) in enumerate(adapters):
                c = s.find(seq)
                if 0 <= c < N:
                    T[lane, mate, slot, c] += 1
            T[lane, mate, E_ROW, min(int(L[i]), N) - 1] += 1
    return T


def table_fast(cols_list, n_lanes, N, adapters=None):
    """table(), vectorised for batches of hundreds of thousands of reads: one entry per base in sequencing orientation (np.repeat),
    per adapter the positions at which all its letters stand inside one read, the lowest of them per read, one np.bincount.  Written
    from the same definition; tests/test_adapter_by_cycle_cpu.py holds the two against each other bit for bit."""
    adapters = adapters or BUILTIN
    T = np.zeros(n_lanes * 2 * ROWS * N, np.int64)
    code_of = np.full(16, 4, np.int64)
    code_of[[1, 2, 4, 8]] = [0, 1, 2, 3]
    for cols in _batches(cols_list):
        L = cols["l_seq"].astype(np.int64)
        f = cols["flag"].astype(np.int64)
        lane = cols["lane"].astype(np.int64)
        ok = ((f & 0x900) == 0) & ((f & 0xC0) != 0) & (L > 0) & (lane < n_lanes)
        mate = np.where((f & 0x40) != 0, 0, 1)
        row_base = (np.where(ok, lane, 0) * 2 + mate) * ROWS
        np.add.at(T, ((row_base + E_ROW) * N + np.minimum(L, N) - 1)[ok], 1)
        total = int(L.sum())
        if not total:
            continue
        nb = (L + 1) // 2
        first = np.cumsum(L) - L
        read = np.repeat(np.arange(len(L)), L)
        c = np.arange(total, dtype=np.int64) - first[read]          # the cycle of every entry
        rev = (f[read] & 0x10) != 0
        j = np.where(rev, L[read] - 1 - c, c)                       # its stored index
        byte = cols["seq"][(np.cumsum(nb) - nb)[read] + (j >> 1)].astype(np.int64)
        code = code_of[np.where(j & 1, byte & 15, byte >> 4)]
        code = np.where(rev & (code < 4), 3 - code, code)
        for slot, (name, seq) in enumerate(adapters):
            m = len(seq)
            if total < m:
                continue
            hit = np.ones(total - m + 1, bool)
            for k, ch in enumerate(seq):
                hit &= code[k:total - m + 1 + k] == "ACGT".index(ch)
            hit &= read[:total - m + 1] == read[m - 1:]              # (all m letters in one read)
            at = np.flatnonzero(hit)
            r, idx = np.unique(read[at], return_index=True)          # (at ascends: the first entry of a read is its lowest cycle)
            ch = c[at[idx]]
            keep = ok[r] & (ch < N)
            np.add.at(T, ((row_base[r] + slot) * N + ch)[keep], 1)
    return T.reshape(n_lanes, 2, ROWS, N).astype(np.uint64)


def sizes(T_lm):
    """n_cycles of one lane and mate: 1 + the highest index with a non-zero E, 0 when there is none."""
    nz = np.flatnonzero(T_lm[E_ROW])
    return int(nz[-1]) + 1 if len(nz) else 0


def text(T, sample_id, lane_names, lane_index=None, adapters=None):
    """The `.adp` text: lanes in the order given, per mate the reads by length, then a line of first hits per adapter of the set."""
    adapters = adapters or BUILTIN
    out = []
    for k, name in enumerate(lane_names):
        l = k if lane_index is None else lane_index[k]
        out += ["sample_id " + sample_id, "lane " + name]
        for m, key in enumerate(("first", "second")):
            nc = sizes(T[l, m])
            out.append(" ".join(["adapter_reads_by_length_" + key] + [str(int(v)) for v in T[l, m, E_ROW, :nc]]))
            for slot, (aname, seq) in enumerate(adapters):
                out.append(" ".join(["adapter_first_hit_by_position_" + key, aname, seq] + [str(int(v)) for v in T[l, m, slot, :nc]]))
    return "\n".join(out) + "\n"
