"""Restatement of the per-read statistics (no GPU use): from a batch's columns to the per-read-group counts, in the shape that
bamqc_amd._abi.diff_counts compares, written from the rules quoted in bamqc_amd/csrc/read_stats.h (the reference's
bamqualcheck.cpp:318-434 and QualityCheck.hpp:168-271) with one loop per read and Python's unbounded integers.  Nothing here comes from
the oracle (tests/oracle_lib.py) or from the kernels: tests/test_read_stats_cpu.py holds the two against each other.

The rules, per record, in the reference's order:
  L > max_read_len                      the run ends: ERR_RANGE
  0x800                                 supplementary += 1, nothing else
  0x100                                 not_primary += 1, nothing else
  0x400 / 0x200                         duplicates / QCfailed += 1 (the read goes on)
  every read that gets here             readcount += 1, totalbps += L
  0x40 (first) else 0x80 (second)       the mate's readnr += 1, readLength[L] += 1; neither: the run ends with ERR_NO_MATE_FLAG
  first: 0x4 -> firstunmapped (and 0x8 -> bothunmapped); 0x2 -> properpair (and strands equal -> FF_RR);  second: 0x4 -> secondunmapped
  on a main chromosome (0 <= rid < n_refs and main_chrom[rid]), mapped (0x4 clear):
      the CIGAR in read orientation (reversed with 0x10): a first word S marks the cycles j < min(n, L) in sc5; ELSE a last word S
      marks the cycles L - n <= j < L in sc3 (n > L: none); D and I lengths are summed; either sum >= hist_cap ends the run (ERR_RANGE);
      delhist[D] += 1, inshist[I] += 1, mapQ[mapq] += 1; for every integer NM tag: mm = (NM - D - I) mod 2^32, mm >= hist_cap ends the
      run (ERR_RANGE), mismatch[mm] += 1;  first mate with 0x8 clear and BQC_FLAG_MATE_MAIN: insertSize[min(|tlen|, isize)] += 1
  first mate on a main chromosome: first_and_or_second_mapped (0x4 or 0x8 clear, 0x400 clear), auto_properpair (0x2, 0x400 clear)

Vectors grow as the reference's do: readLength to the longest read + 1, the per-cycle vectors (sc5, sc3) to the longest read, mapQ /
mismatch / delhist / inshist to the largest value + 1, insertSize has isize + 1 entries from the start; a vector nothing was added to is
empty.  Counters of the reference's type `unsigned` are taken mod 2^32, totalbps is 64 bits wide.

NOT modelled (UNMODELLED below): everything derived from the bases, the qualities or the alignment's position.  A batch of
tests/rs_steps.py keeps every read out of the triplets (alignment score below 50), so that no record ends the run for a reason this
file does not know (AS tag, FASTA)."""
import numpy as np

# the kernels' constants (tests/test_read_stats_cpu.py pins them to read_stats.h and device_types.h)
RS_HB = 64             # mismatch / deletion / insertion bins kept in LDS
RS_INS = 1024          # insert-size bins kept in LDS
BQC_CT = 304           # read lengths and clip lengths up to here stay in LDS
BQC_FAST_MAXLEN = 255  # longest read of k_short

ERR_NO_MATE_FLAG, ERR_RANGE = 3, 6
NM_ABSENT = -1
FLAG_MATE_MAIN = 0x1000
U32 = 0xFFFFFFFF

# include/bamqc.h: enum bqc_scalar
S_SUPPLEMENTARY, S_DUPLICATES, S_QCFAILED, S_NOT_PRIMARY, S_READCOUNT, S_TOTALBPS, S_BOTHUNMAPPED, S_FIRSTUNMAPPED, S_SECONDUNMAPPED, \
    S_FIRST_AND_OR_SECOND_MAPPED, S_FF_RR, S_PROPERPAIR, S_AUTO_PROPERPAIR, N_SCALARS = range(14)

MATE_KEYS = ("n_cycles", "qualcount_readnr", "readLength", "mapQ", "mismatch", "delhist", "inshist", "sc5", "sc3", "insertSize")
MODELLED = ("scalars",) + tuple("r%d.%s" % (m, k) for m in (1, 2) for k in MATE_KEYS)
# what a counts dict holds besides (bamqc_amd._abi.counts_to_dict): the sequence-derived counts
UNMODELLED = ("poscov", "eightmer", "triplet", "sketch") + tuple(
    "r%d.%s" % (m, k) for m in (1, 2) for k in ("dnacount0", "dnacount1", "dnacount2", "dnacount3", "dnacount4", "qualcount", "Ncount", "GCcount", "averageQual"))


class _Mate:
    def __init__(self, isize):
        self.readnr = 0
        self.max_len = -1
        self.readlen = {}
        self.mapq = {}
        self.mm = {}
        self.dele = {}
        self.ins = {}
        self.sc5 = {}
        self.sc3 = {}
        self.insert = [0] * (isize + 1)


def _vec(d):
    """A vector that grew to its largest index + 1 (empty: nothing was added)."""
    v = np.zeros(max(d) + 1 if d else 0, np.uint64)
    for k, n in d.items():
        v[k] = n & U32
    return v


def _cycles(d, n):
    v = np.zeros(n, np.uint64)
    for k, c in d.items():
        v[k] = c & U32
    return v


def counts(batches, n_lanes=1, n_refs=1, main_chrom=None, isize=1000, max_read_len=1024, hist_cap=4096, **ignored):
    """(error code, counts): counts is None when a record ends the run, else a list by read group of {key: value} over MODELLED.
    batches: a column dict or a list of them (with their optional nm_extra_read / nm_extra_val); the other arguments are the options of
    the context (those that do not bear on these counts are ignored)."""
    if isinstance(batches, dict):
        batches = [batches]
    main = [1] * n_refs if main_chrom is None else [int(x) for x in main_chrom]
    scal = [[0] * N_SCALARS for _ in range(n_lanes)]
    mates = [(_Mate(isize), _Mate(isize)) for _ in range(n_lanes)]
    for cols in batches:
        flag_c, L_c, mapq_c, lane_c = cols["flag"].tolist(), cols["l_seq"].tolist(), cols["mapq"].tolist(), cols["lane"].tolist()
        rid_c, tlen_c, nm_c, nc_c = cols["rid"].tolist(), cols["tlen"].tolist(), cols["nm"].tolist(), cols["n_cigar"].tolist()
        cig = cols["cigar"].tolist()
        extra = {}
        for r, v in zip(np.asarray(cols.get("nm_extra_read", []), np.int64).tolist(), np.asarray(cols.get("nm_extra_val", []), np.int64).tolist()):
            extra.setdefault(r, []).append(v)
        co = 0
        for i in range(len(flag_c)):
            flag, L, nc = flag_c[i], L_c[i], nc_c[i]
            c0 = co
            co += nc
            if L > max_read_len:
                return ERR_RANGE, None
            lane = lane_c[i]
            assert lane < n_lanes
            S = scal[lane]
            if flag & 0x800:
                S[S_SUPPLEMENTARY] += 1
                continue
            if flag & 0x100:
                S[S_NOT_PRIMARY] += 1
                continue
            dup = flag & 0x400
            if dup:
                S[S_DUPLICATES] += 1
            if flag & 0x200:
                S[S_QCFAILED] += 1
            S[S_READCOUNT] += 1
            S[S_TOTALBPS] += L
            unm, nunm, proper = flag & 0x4, flag & 0x8, flag & 0x2
            first = flag & 0x40
            if first:
                if unm:
                    S[S_FIRSTUNMAPPED] += 1
                    if nunm:
                        S[S_BOTHUNMAPPED] += 1
                if proper:
                    S[S_PROPERPAIR] += 1
                    if bool(flag & 0x10) == bool(flag & 0x20):
                        S[S_FF_RR] += 1
                M = mates[lane][0]
            elif flag & 0x80:
                if unm:
                    S[S_SECONDUNMAPPED] += 1
                M = mates[lane][1]
            else:
                return ERR_NO_MATE_FLAG, None
            M.readnr += 1
            M.readlen[L] = M.readlen.get(L, 0) + 1
            if L > M.max_len:
                M.max_len = L
            rid = rid_c[i]
            if not (0 <= rid < n_refs and main[rid]):
                continue
            if not unm:
                dele = ins = 0
                if nc:
                    words = cig[c0:c0 + nc]
                    if flag & 0x10:
                        words = words[::-1]
                    if words[0] & 15 == 4:
                        for j in range(min(words[0] >> 4, L)):
                            M.sc5[j] = M.sc5.get(j, 0) + 1
                    elif words[-1] & 15 == 4:
                        n = words[-1] >> 4
                        if n <= L:  # (a clip longer than the read: the reference's unsigned start L - n lies behind L, its loop is empty)
                            for j in range(L - n, L):
                                M.sc3[j] = M.sc3.get(j, 0) + 1
                    for w in words:
                        if w & 15 == 2:
                            dele += w >> 4
                        elif w & 15 == 1:
                            ins += w >> 4
                if dele >= hist_cap or ins >= hist_cap:
                    return ERR_RANGE, None
                M.dele[dele] = M.dele.get(dele, 0) + 1
                M.ins[ins] = M.ins.get(ins, 0) + 1
                mq = mapq_c[i]
                M.mapq[mq] = M.mapq.get(mq, 0) + 1
                tags = ([] if nm_c[i] == NM_ABSENT else [nm_c[i]]) + extra.get(i, [])
                for nm in tags:
                    mm = (nm - dele - ins) & U32  # unsigned arithmetic: NM < D + I wraps
                    if mm >= hist_cap:
                        return ERR_RANGE, None
                    M.mm[mm] = M.mm.get(mm, 0) + 1
                if first and not nunm and flag & FLAG_MATE_MAIN:
                    M.insert[min(abs(tlen_c[i]), isize)] += 1
            if first:
                if (not unm or not nunm) and not dup:
                    S[S_FIRST_AND_OR_SECOND_MAPPED] += 1
                if proper and not dup:
                    S[S_AUTO_PROPERPAIR] += 1
    out = []
    for lane in range(n_lanes):
        d = {"scalars": np.array([v if k == S_TOTALBPS else v & U32 for k, v in enumerate(scal[lane])], np.uint64)}
        for m in (0, 1):
            M, p = mates[lane][m], "r%d." % (m + 1)
            n_cyc = max(M.max_len, 0)
            d[p + "n_cycles"] = n_cyc
            d[p + "qualcount_readnr"] = M.readnr & U32
            d[p + "readLength"] = _vec(M.readlen)
            d[p + "mapQ"] = _vec(M.mapq)
            d[p + "mismatch"] = _vec(M.mm)
            d[p + "delhist"] = _vec(M.dele)
            d[p + "inshist"] = _vec(M.ins)
            d[p + "sc5"] = _cycles(M.sc5, n_cyc)
            d[p + "sc3"] = _cycles(M.sc3, n_cyc)
            d[p + "insertSize"] = np.array([v & U32 for v in M.insert], np.uint64)
        out.append(d)
    return 0, out


def diff(want, got):
    """The differences between the restatement's counts and a counts dict of the library or the oracle, over exactly the keys this
    file models; the other keys of `got` must be the ones listed as UNMODELLED."""
    from bamqc_amd import _abi
    assert len(want) == len(got), (len(want), len(got))
    for w, g in zip(want, got):
        assert sorted(w) == sorted(MODELLED) and sorted(set(g) - set(w)) == sorted(UNMODELLED), sorted(set(g) ^ set(w))
    return _abi.diff_counts(want, [{k: g[k] for k in MODELLED} for g in got])
