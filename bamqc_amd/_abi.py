"""ctypes mirror of include/bamqc.h (the C ABI of the aggregation path).

Only structure layouts and small marshalling helpers live here; the library
itself is loaded in `bamqc_amd._lib`.  The test suite's CPU checker accepts the same
structures, so tests marshal one batch and hand it to both sides.
"""
import ctypes as C

import numpy as np

BQC_N_SCALARS = 13
BQC_COVSIZE = 100
BQC_N_8MER = 65536
BQC_N_TRIPLET = 64 * 4 * 4
BQC_FLAG_MATE_MAIN = 0x1000
BQC_FLAG_NO_QUAL = 0x8000
BQC_NM_ABSENT = -1
BQC_AS_ABSENT = -(2 ** 31)

SCALAR_NAMES = [
    "supplementary", "duplicates", "QCfailed", "not_primary_alignment", "readcount", "totalbps",
    "bothunmapped", "firstunmapped", "secondunmapped", "first_and_or_second_mapped",
    "FF_RR_orientation", "properpair_count", "auto_properpair_count",
]

ERR_NAMES = {0: "OK", 1: "ARG", 2: "DEVICE", 3: "NO_MATE_FLAG", 4: "AS_TAG", 5: "FASTA", 6: "RANGE", 7: "IO", 8: "STATE"}

u8p = C.POINTER(C.c_uint8)
u16p = C.POINTER(C.c_uint16)
u32p = C.POINTER(C.c_uint32)
i32p = C.POINTER(C.c_int32)
u64p = C.POINTER(C.c_uint64)


class SketchOptions(C.Structure):
    _fields_ = [("n_k", C.c_uint32), ("klist", i32p), ("n_q", C.c_uint32), ("qlist", u32p),
                ("e", C.c_double), ("seed", C.c_int32)]


class Options(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("n_lanes", C.c_uint32), ("n_refs", C.c_uint32),
                ("isize", C.c_int32), ("max_read_len", C.c_uint32), ("hist_cap", C.c_uint32),
                ("main_chrom", u8p), ("fasta_index", i32p), ("device", C.c_int32),
                ("sketch", SketchOptions), ("shard_tail", C.c_uint32), ("qual_by_cycle", C.c_uint32),
                ("mismatch_by_cycle", C.c_uint32), ("pad_tail", C.c_uint32)]


class Batch(C.Structure):
    _fields_ = [("n_reads", C.c_uint32),
                ("flag", u16p), ("mapq", u8p), ("lane", u8p), ("rid", i32p), ("pos", i32p),
                ("tlen", i32p), ("nm", i32p), ("as_", i32p), ("l_seq", u32p), ("n_cigar", u16p),
                ("seq", u8p), ("qual", u8p), ("cigar", u32p),
                ("n_nm_extra", C.c_uint32), ("nm_extra_read", u32p), ("nm_extra_val", i32p)]


class MateCounts(C.Structure):
    _fields_ = [("n_cycles", C.c_uint32), ("dnacount", u64p * 5), ("qualcount", u64p),
                ("qualcount_readnr", C.c_uint64), ("sc5", u64p), ("sc3", u64p),
                ("n_Ncount", C.c_uint32), ("Ncount", u64p),
                ("n_GCcount", C.c_uint32), ("GCcount", u64p),
                ("n_averageQual", C.c_uint32), ("averageQual", u64p),
                ("n_insertSize", C.c_uint32), ("insertSize", u64p),
                ("n_mapQ", C.c_uint32), ("mapQ", u64p),
                ("n_readLength", C.c_uint32), ("readLength", u64p),
                ("n_mismatch", C.c_uint32), ("mismatch", u64p),
                ("n_delhist", C.c_uint32), ("delhist", u64p),
                ("n_inshist", C.c_uint32), ("inshist", u64p)]


class SketchCounts(C.Structure):
    _fields_ = [("q", C.c_uint32), ("k", C.c_uint32), ("sumCount", C.c_uint64), ("F0", C.c_uint64),
                ("f1", C.c_uint64), ("F2", C.c_uint64)]


class LaneCounts(C.Structure):
    _fields_ = [("scalars", C.c_uint64 * BQC_N_SCALARS), ("poscov", C.c_uint64 * (BQC_COVSIZE + 1)),
                ("eightmer", u64p), ("mate", MateCounts * 2), ("triplet", u64p),
                ("n_sketch", C.c_uint32), ("sketch", C.POINTER(SketchCounts))]


class Counts(C.Structure):
    _fields_ = [("n_lanes", C.c_uint32), ("lanes", C.POINTER(LaneCounts))]


class SynthParams(C.Structure):
    _fields_ = [("seed", C.c_uint64), ("first_read_index", C.c_uint64), ("n_reads", C.c_uint32),
                ("read_len", C.c_uint32), ("n_refs", C.c_uint32), ("ref_len", u32p), ("n_lanes", C.c_uint32),
                ("isize", C.c_int32), ("long_reads", C.c_int32)]


class ShardInfo(C.Structure):
    _fields_ = [("ctx", C.c_void_p), ("status", C.c_int32), ("begin_block", C.c_uint64), ("end_block", C.c_uint64),
                ("first", C.c_uint64), ("over", C.c_uint64), ("sample_id", C.c_char_p), ("n_lane_names", C.c_uint32),
                ("lane_names", C.POINTER(C.c_char_p)), ("lane_index", u32p)]


class ShardResult(C.Structure):
    _fields_ = [("n_lane_names", C.c_uint32), ("lane_names", C.POINTER(C.c_char_p)), ("lane_index", u32p)]


SHARD_HOOK = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(ShardInfo), C.POINTER(ShardResult))
SHARD_FAIL, SHARD_DONE, SHARD_FALLBACK, SHARD_WRITE = 0, 1, 2, 3  # (0 is what ctypes returns for a callback that raised)


class QbcView(C.Structure):  # bqc_qbc_view: element [c][q] is hist[c * stride + q]
    _fields_ = [("n_cycles", C.c_uint32), ("n_q", C.c_uint32), ("stride", C.c_uint32), ("hist", u64p)]


class MbcView(C.Structure):  # bqc_mbc_view: element [c][q] is aligned[c * stride + q] / mismatch[c * stride + q]
    _fields_ = [("n_cycles", C.c_uint32), ("n_q", C.c_uint32), ("stride", C.c_uint32), ("aligned", u64p), ("mismatch", u64p)]


class Adapter(C.Structure):  # bqc_adapter
    _fields_ = [("name", C.c_char_p), ("seq", C.c_char_p)]


class Modules(C.Structure):  # bqc_modules: the optional modules that bqc_create_ex takes beside bqc_options
    _fields_ = [("struct_size", C.c_uint32), ("adapter_by_cycle", C.c_uint32), ("n_adapters", C.c_uint32), ("pad", C.c_uint32),
                ("adapters", C.POINTER(Adapter))]


class AdpView(C.Structure):  # bqc_adp_view: reads_by_length[c], first_hit[a * stride + c]
    _fields_ = [("n_cycles", C.c_uint32), ("n_adapters", C.c_uint32), ("stride", C.c_uint32), ("reads_by_length", u64p),
                ("first_hit", u64p), ("adapters", C.POINTER(Adapter))]


class GcbView(C.Structure):  # bqc_gcb_view: four arrays of n_bins = 101 entries, by GC bin
    _fields_ = [("window", C.c_uint32), ("n_bins", C.c_uint32), ("genome_windows", u64p), ("read_starts", u64p), ("bases", u64p),
                ("qual_sum", u64p)]


class IbcView(C.Structure):  # bqc_ibc_view: three arrays of n_cycles entries by cycle, two of n_len = 64 entries by length (entry i: i + 1)
    _fields_ = [("n_cycles", C.c_uint32), ("n_len", C.c_uint32), ("reads_by_length", u64p), ("insertions", u64p), ("deletions", u64p),
                ("insertion_lengths", u64p), ("deletion_lengths", u64p)]


class SbcView(C.Structure):  # bqc_sbc_view: by_context of 512 entries [s][ctx][b'], by_cycle of 16 n_cycles entries [c][t'][b']
    _fields_ = [("n_cycles", C.c_uint32), ("min_base_qual", C.c_uint32), ("min_mapq", C.c_uint32), ("by_context", u64p), ("by_cycle", u64p)]


class SacView(C.Structure):  # bqc_sac_view: rid and pos of n_sites entries, counts of 8 n_sites entries [site][strand][base]
    _fields_ = [("n_sites", C.c_uint32), ("min_base_qual", C.c_uint32), ("min_mapq", C.c_uint32), ("rid", C.POINTER(C.c_int32)), ("pos", C.POINTER(C.c_int32)),
                ("counts", u64p)]


class RcvView(C.Structure):  # bqc_rcv_view: the list of n_regions entries, five scalars, thresholds, regions [n_regions][3 + n_thresholds], hist [depth_cap + 1]
    _fields_ = [("n_regions", C.c_uint32), ("min_mapq", C.c_uint32), ("n_thresholds", C.c_uint32), ("depth_cap", C.c_uint32),
                ("rid", C.POINTER(C.c_int32)), ("start", C.POINTER(C.c_int32)), ("end", C.POINTER(C.c_int32)),
                ("reads_examined", C.c_uint64), ("reads_on_target", C.c_uint64), ("aligned_bases", C.c_uint64), ("bases_on_target", C.c_uint64),
                ("target_bases", C.c_uint64), ("thresholds", u64p), ("regions", u64p), ("hist", u64p)]


class DupView(C.Structure):  # bqc_dup_view: by class (0 single, 1 pair) the sets, the largest set and 256 sets by size; lanes [n_lanes][5]
    _fields_ = [("capacity", C.c_uint64), ("n_lanes", C.c_uint32), ("pad", C.c_uint32), ("sets", C.c_uint64 * 2), ("largest", C.c_uint64 * 2),
                ("hist", u64p * 2), ("estimated_library_size", C.c_uint64), ("lanes", u64p)]


class OvrSeq(C.Structure):  # bqc_ovr_seq: a listed set's letters, its reads and its possible source
    _fields_ = [("seq", C.c_char_p), ("count", C.c_uint64), ("source", C.c_char_p)]


class OvrView(C.Structure):  # bqc_ovr_view: K, ppm, capacity, lanes [n_lanes][4], by mate the sets, the largest set, 256 sets by size, the threshold and the list
    _fields_ = [("prefix_len", C.c_uint32), ("ppm", C.c_uint32), ("capacity", C.c_uint64), ("n_lanes", C.c_uint32), ("pad", C.c_uint32), ("lanes", u64p),
                ("distinct", C.c_uint64 * 2), ("largest", C.c_uint64 * 2), ("hist", u64p * 2), ("threshold", C.c_uint64 * 2), ("n_listed", C.c_uint32 * 2),
                ("listed", C.POINTER(OvrSeq) * 2)]


class WdpView(C.Structure):  # bqc_wdp_view: W, MQ, NW, n_refs, woff [n_refs + 1], ref_len [n_refs], E, E_low, X, three planes [NW], contigs [n_refs][3], hist [1001]
    _fields_ = [("window", C.c_uint32), ("min_mapq", C.c_uint32), ("n_windows", C.c_uint32), ("n_refs", C.c_uint32), ("woff", u32p), ("ref_len", u32p),
                ("reads_examined", C.c_uint64), ("reads_low_mapq", C.c_uint64), ("bases_outside", C.c_uint64), ("reads", u64p), ("bases", u64p),
                ("bases_low", u64p), ("contigs", u64p), ("hist", u64p)]


def make_modules(adapter_by_cycle=0, adapters=None, struct_size=None):
    """bqc_modules: adapter_by_cycle = the cycle capacity N (0: off), adapters = [(name, sequence), ...] or None for the built-in set."""
    m = Modules()
    m.struct_size = C.sizeof(Modules) if struct_size is None else struct_size
    m.adapter_by_cycle = adapter_by_cycle
    keep = None
    if adapters:
        keep = (Adapter * len(adapters))(*[Adapter(n.encode() if isinstance(n, str) else n, s.encode() if isinstance(s, str) else s) for n, s in adapters])
        m.n_adapters = len(adapters)
        m.adapters = keep
    return m, keep


class HeaderInfo(C.Structure):
    _fields_ = [("sample_id", C.c_char_p), ("n_names", C.c_uint32),
                ("lane_names", C.POINTER(C.c_char_p)), ("lane_index", u32p)]


class RouteFacts(C.Structure):  # host/input_route.h: bqc_route_facts (the enums' values: there)
    _fields_ = [("caller", C.c_int32), ("kind", C.c_int32), ("regular", C.c_int32), ("size", C.c_uint64), ("dash_bgzf", C.c_int32),
                ("carries", C.c_int32), ("gpu_decode", C.c_int32), ("host_reader_only", C.c_int32), ("shard", C.c_int32),
                ("shard_found", C.c_int32), ("shard_bytes", C.c_uint64), ("has_rg", C.c_int32), ("ended", C.c_int32)]


class Route(C.Structure):  # bqc_route
    _fields_ = [("refuse", C.c_int32), ("sniff", C.c_int32), ("stream", C.c_int32), ("find_blocks", C.c_int32), ("header_by", C.c_int32),
                ("header_first", C.c_int32), ("hold", C.c_uint64), ("reader", C.c_int32), ("source", C.c_int32)]


_BATCH_COLS = [("flag", np.uint16, u16p), ("mapq", np.uint8, u8p), ("lane", np.uint8, u8p),
               ("rid", np.int32, i32p), ("pos", np.int32, i32p), ("tlen", np.int32, i32p),
               ("nm", np.int32, i32p), ("as_", np.int32, i32p), ("l_seq", np.uint32, u32p),
               ("n_cigar", np.uint16, u16p), ("seq", np.uint8, u8p), ("qual", np.uint8, u8p),
               ("cigar", np.uint32, u32p)]


def _ptr(a, ptype):
    return a.ctypes.data_as(ptype)


def make_batch(cols):
    """Build a `Batch` from a dict of numpy arrays (keys as in `_BATCH_COLS`, plus optional
    `nm_extra_read`/`nm_extra_val`).  Returns (batch, keepalive)."""
    n = len(cols["flag"])
    keep = {}
    b = Batch()
    b.n_reads = n
    if n:  # BQC_FLAG_NO_QUAL is the decoder's to set (include/bamqc.h): column dicts built by hand get it here
        l = np.asarray(cols["l_seq"], np.int64)
        qo = np.cumsum(l) - l
        q = np.asarray(cols["qual"], np.uint8)
        noq = (l > 0) & (q[np.minimum(qo, max(len(q) - 1, 0))] == 0xFF) if len(q) else np.zeros(n, bool)
        if noq.any():
            cols = dict(cols, flag=np.asarray(cols["flag"], np.uint16) | (noq.astype(np.uint16) << 15))
    for name, dt, pt in _BATCH_COLS:
        a = np.ascontiguousarray(cols[name], dtype=dt)
        if a.size == 0:
            a = np.zeros(1, dtype=dt)
        keep[name] = a
        setattr(b, name, _ptr(a, pt))
    xr = np.ascontiguousarray(cols.get("nm_extra_read", np.zeros(0)), dtype=np.uint32)
    xv = np.ascontiguousarray(cols.get("nm_extra_val", np.zeros(0)), dtype=np.int32)
    b.n_nm_extra = len(xr)
    if len(xr) == 0:
        xr = np.zeros(1, np.uint32)
        xv = np.zeros(1, np.int32)
    keep["xr"], keep["xv"] = xr, xv
    b.nm_extra_read = _ptr(xr, u32p)
    b.nm_extra_val = _ptr(xv, i32p)
    # consistency of the packed layout
    l = keep["l_seq"][:n].astype(np.int64)
    assert len(cols["seq"]) == int(((l + 1) // 2).sum()), "seq bytes != sum((l_seq+1)/2)"
    assert len(cols["qual"]) == int(l.sum()), "qual bytes != sum(l_seq)"
    assert len(cols["cigar"]) == int(keep["n_cigar"][:n].astype(np.int64).sum()), "cigar words != sum(n_cigar)"
    return b, keep


def make_options(n_lanes=1, n_refs=1, isize=1000, max_read_len=1024, hist_cap=4096, main_chrom=None,
                 fasta_index=None, device=0, klist=(), qlist=(), e=0.01, seed=1, shard_tail=0, qual_by_cycle=0,
                 mismatch_by_cycle=0, struct_size=None):
    keep = {}
    o = Options()
    o.struct_size = C.sizeof(Options) if struct_size is None else struct_size  # (a smaller one: a caller built against an earlier header)
    o.n_lanes, o.n_refs, o.isize = n_lanes, n_refs, isize
    o.max_read_len, o.hist_cap, o.device = max_read_len, hist_cap, device
    mc = np.ones(max(n_refs, 1), np.uint8) if main_chrom is None else np.ascontiguousarray(main_chrom, np.uint8)
    keep["mc"] = mc
    o.main_chrom = _ptr(mc, u8p)
    if fasta_index is not None:
        fi = np.ascontiguousarray(fasta_index, np.int32)
        keep["fi"] = fi
        o.fasta_index = _ptr(fi, i32p)
    kl = np.ascontiguousarray(list(klist), np.int32)
    ql = np.ascontiguousarray(list(qlist), np.uint32)
    keep["kl"], keep["ql"] = kl, ql
    o.sketch.n_k, o.sketch.n_q = len(kl), len(ql)
    if len(kl):
        o.sketch.klist = _ptr(kl, i32p)
    if len(ql):
        o.sketch.qlist = _ptr(ql, u32p)
    o.sketch.e, o.sketch.seed = e, seed
    o.shard_tail = 1 if shard_tail else 0
    o.qual_by_cycle = qual_by_cycle  # per-cycle base quality histograms: 0 = off, else the cycle capacity N
    o.mismatch_by_cycle = mismatch_by_cycle  # compared bases and mismatches by cycle and quality: 0 = off, else the cycle capacity N
    return o, keep


def _arr(p, n):
    if n == 0 or not p:
        return np.zeros(0, np.uint64)
    return np.ctypeslib.as_array(p, shape=(n,)).copy()


def counts_to_dict(cptr):
    """Deep-copy a `bqc_counts*` into {lane: {name: value/ndarray}} for comparison."""
    c = cptr.contents if hasattr(cptr, "contents") else cptr
    out = []
    for li in range(c.n_lanes):
        L = c.lanes[li]
        d = {"scalars": np.array(list(L.scalars), dtype=np.uint64),
             "poscov": np.array(list(L.poscov), dtype=np.uint64),
             "eightmer": _arr(L.eightmer, BQC_N_8MER),
             "triplet": _arr(L.triplet, BQC_N_TRIPLET)}
        for mi in range(2):
            m = L.mate[mi]
            p = "r%d." % (mi + 1)
            d[p + "n_cycles"] = int(m.n_cycles)
            for j in range(5):
                d[p + "dnacount%d" % j] = _arr(m.dnacount[j], m.n_cycles)
            d[p + "qualcount"] = _arr(m.qualcount, m.n_cycles)
            d[p + "qualcount_readnr"] = int(m.qualcount_readnr)
            d[p + "sc5"] = _arr(m.sc5, m.n_cycles)
            d[p + "sc3"] = _arr(m.sc3, m.n_cycles)
            for name in ("Ncount", "GCcount", "averageQual", "insertSize", "mapQ", "readLength",
                         "mismatch", "delhist", "inshist"):
                d[p + name] = _arr(getattr(m, name), getattr(m, "n_" + name))
        d["sketch"] = [(int(L.sketch[i].q), int(L.sketch[i].k), int(L.sketch[i].sumCount), int(L.sketch[i].F0),
                        int(L.sketch[i].f1), int(L.sketch[i].F2)) for i in range(L.n_sketch)]
        out.append(d)
    return out


def diff_counts(a, b):
    """Return a list of human-readable differences between two counts_to_dict results."""
    diffs = []
    if len(a) != len(b):
        return ["lane count %d != %d" % (len(a), len(b))]
    for li, (x, y) in enumerate(zip(a, b)):
        for k in x:
            u, v = x[k], y[k]
            if isinstance(u, np.ndarray):
                if u.shape != v.shape:
                    diffs.append("lane %d %s: length %d != %d" % (li, k, len(u), len(v)))
                elif not np.array_equal(u, v):
                    idx = np.nonzero(u != v)[0]
                    diffs.append("lane %d %s: %d bins differ, first at %d: %d != %d" % (
                        li, k, len(idx), idx[0], int(u[idx[0]]), int(v[idx[0]])))
            elif u != v:
                diffs.append("lane %d %s: %r != %r" % (li, k, u, v))
    return diffs
