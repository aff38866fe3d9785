"""Host-side mirror of the aggregation seam of BamQC (the body of the record loop,
reference src/bamqualcheck.cpp:303-453) over the C ABI of include/bamqc.h.

    agg = Aggregator(n_lanes=1, n_refs=4, isize=1000, main_chrom=[1, 1, 1, 1])
    agg.set_reference(rid, dna5_codes)      # Genome (TripletCounting.hpp:60-104)
    agg.submit(cols)                        # one SoA batch of decoded BAM records
    counts = agg.finalize()                 # host mirror of `struct Counts`
    agg.write_bamqc(path, sample_id, lane_names)

All computation happens in hand-written HIP kernels inside libbamqc_gpu.so; this module only
marshals numpy arrays into the ABI structures.
"""
import ctypes as C

import numpy as np

from . import _abi, _lib


class BamQCError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("bamqc error %d (%s): %s" % (code, _abi.ERR_NAMES.get(code, "?"), msg))
        self.code = code


class DeviceBatch:
    def __init__(self, agg, handle):
        self.agg, self.h = agg, handle

    @property
    def algorithmic_bytes(self):
        return int(self.agg.lib.bqc_dbatch_bytes(self.h))

    def free(self):
        if self.h:
            self.agg.lib.bqc_dbatch_free(self.agg.h, self.h)
            self.h = None


class Aggregator:
    def __init__(self, adapter_by_cycle=None, adapters=None, gc_bias=None, indel_by_cycle=None, substitutions=None, subst_min_qual=20, subst_min_mapq=30,
                 site_alleles=None, site_min_qual=20, site_min_mapq=20, regions=None, region_min_mapq=20, region_thresholds=(1, 10, 20, 30, 50, 100),
                 region_depth_cap=1000, duplicate_sets=None, window_depth=None, window_min_mapq=20, overrepresented=None, overrepresented_ppm=1000,
                 **options):
        self.lib = _lib.load()
        self.opt, self._keep = _abi.make_options(**options)
        self.h = C.c_void_p()
        if adapter_by_cycle is None and adapters is None:
            rc = self.lib.bqc_create(C.byref(self.opt), C.byref(self.h))
        else:  # the modules that are configured beside bqc_options (adapter content by cycle)
            mod, keep = _abi.make_modules(adapter_by_cycle or 0, adapters)
            rc = self.lib.bqc_create_ex(C.byref(self.opt), C.byref(mod), C.byref(self.h))
        if rc:
            raise BamQCError(rc, (self.lib.bqc_last_error(None) or b"").decode())
        self._counts = None
        if gc_bias is not None:  # the module that is switched on behind the creation (GC bias, window gc_bias)
            try:
                self.enable_gc_bias(gc_bias)
            except BamQCError:
                self.close()
                raise
        if indel_by_cycle is not None:  # the same way: indels by cycle and by length, cycle capacity indel_by_cycle
            try:
                self.enable_indel_by_cycle(indel_by_cycle)
            except BamQCError:
                self.close()
                raise

        if substitutions is not None:  # the same way: substitutions by context and by cycle, cycle capacity `substitutions`
            try:
                self.enable_substitutions(substitutions, subst_min_qual, subst_min_mapq)
            except BamQCError:
                self.close()
                raise

        if site_alleles is not None:  # the same way: allele counts at the sites (rid, pos), two arrays sorted by (rid, pos)
            try:
                self.enable_site_alleles(site_alleles[0], site_alleles[1], site_min_qual, site_min_mapq)
            except BamQCError:
                self.close()
                raise

        if regions is not None:  # the same way: depth over the regions (rid, start, end), three arrays sorted by (rid, start), disjoint
            try:
                self.enable_region_coverage(regions[0], regions[1], regions[2], region_min_mapq, region_thresholds, region_depth_cap)
            except BamQCError:
                self.close()
                raise

        if duplicate_sets is not None:  # the same way: duplicate sets by alignment signature, a table for `duplicate_sets` signatures
            try:
                self.enable_duplicate_sets(duplicate_sets)
            except BamQCError:
                self.close()
                raise

        if window_depth is not None:  # the same way: depth in windows of window_depth[0] bases over contigs of the lengths window_depth[1]
            try:
                self.enable_window_depth(window_depth[0], window_depth[1], window_min_mapq)
            except BamQCError:
                self.close()
                raise

        if overrepresented is not None:  # the same way: sets of equal read sequences, overrepresented = (K, capacity)
            try:
                self.enable_overrepresented(overrepresented[0], overrepresented_ppm, overrepresented[1])
            except BamQCError:
                self.close()
                raise

    def enable_overrepresented(self, prefix_len=50, ppm=1000, capacity=1 << 26):
        self._chk(self.lib.bqc_enable_overrepresented(self.h, prefix_len, ppm, capacity))

    def enable_window_depth(self, window=1000, ref_len=None, min_mapq=20):
        """ref_len: the lengths of the context's n_refs contigs (None: a null list, which the library refuses)."""
        if ref_len is None:
            self._chk(self.lib.bqc_enable_window_depth(self.h, window, None, min_mapq))
            return
        ln = np.ascontiguousarray(ref_len, np.int32)
        assert ln.shape == (self.opt.n_refs,)
        self._chk(self.lib.bqc_enable_window_depth(self.h, window, ln.ctypes.data_as(C.POINTER(C.c_int32)), min_mapq))

    def enable_duplicate_sets(self, capacity=1 << 26):
        self._chk(self.lib.bqc_enable_duplicate_sets(self.h, capacity))

    def enable_region_coverage(self, rid, start, end, min_mapq=20, thresholds=(1, 10, 20, 30, 50, 100), depth_cap=1000):
        rid, start, end = (np.ascontiguousarray(a, np.int32) for a in (rid, start, end))
        assert rid.shape == start.shape == end.shape and rid.ndim == 1
        thr = np.ascontiguousarray(thresholds, np.uint64)
        i32p = C.POINTER(C.c_int32)
        self._chk(self.lib.bqc_enable_region_coverage(self.h, len(rid), rid.ctypes.data_as(i32p), start.ctypes.data_as(i32p), end.ctypes.data_as(i32p), min_mapq,
                                                      len(thr), thr.ctypes.data_as(C.POINTER(C.c_uint64)), depth_cap))

    def enable_site_alleles(self, rid, pos, min_base_qual=20, min_mapq=20):
        rid, pos = np.ascontiguousarray(rid, np.int32), np.ascontiguousarray(pos, np.int32)
        assert rid.shape == pos.shape and rid.ndim == 1
        i32p = C.POINTER(C.c_int32)
        self._chk(self.lib.bqc_enable_site_alleles(self.h, len(rid), rid.ctypes.data_as(i32p), pos.ctypes.data_as(i32p), min_base_qual, min_mapq))

    def enable_substitutions(self, n_cycles=1024, min_base_qual=20, min_mapq=30):
        self._chk(self.lib.bqc_enable_substitutions(self.h, n_cycles, min_base_qual, min_mapq))

    def enable_gc_bias(self, window=100):
        self._chk(self.lib.bqc_enable_gc_bias(self.h, window))

    def enable_indel_by_cycle(self, n_cycles=1024):
        self._chk(self.lib.bqc_enable_indel_by_cycle(self.h, n_cycles))

    def _chk(self, rc):
        if rc:
            raise BamQCError(rc, (self.lib.bqc_last_error(self.h) or b"").decode())

    def set_reference(self, rid, dna5):
        a = np.ascontiguousarray(dna5, np.uint8)
        self._chk(self.lib.bqc_set_reference(self.h, rid, a.ctypes.data_as(_abi.u8p), len(a)))

    def submit(self, cols):
        b, keep = _abi.make_batch(cols)
        self._chk(self.lib.bqc_submit(self.h, C.byref(b)))

    def upload(self, cols):
        b, keep = _abi.make_batch(cols)
        h = C.c_void_p()
        self._chk(self.lib.bqc_upload(self.h, C.byref(b), C.byref(h)))
        return DeviceBatch(self, h)

    def process(self, dbatch):
        self._chk(self.lib.bqc_process(self.h, dbatch.h))

    def sync(self):
        self._chk(self.lib.bqc_sync(self.h))

    def reset(self):
        self._chk(self.lib.bqc_reset(self.h))

    def flush(self):
        self._chk(self.lib.bqc_flush(self.h))

    def set_timing(self, on=True):
        self._chk(self.lib.bqc_set_timing(self.h, 1 if on else 0))

    def last_timing(self):
        n = C.c_uint32()
        names = C.POINTER(C.c_char_p)()
        ms = C.POINTER(C.c_float)()
        self._chk(self.lib.bqc_last_timing(self.h, C.byref(n), C.byref(names), C.byref(ms)))
        return {names[i].decode(): float(ms[i]) for i in range(n.value)}

    @property
    def state_words(self):
        return int(self.lib.bqc_state_words(self.h))

    def state_export_host(self):
        a = np.zeros(self.state_words, np.uint64)
        self._chk(self.lib.bqc_state_export_host(self.h, a.ctypes.data_as(_abi.u64p)))
        return a

    def state_import_host(self, a):
        a = np.ascontiguousarray(a, np.uint64)
        assert len(a) == self.state_words
        self._chk(self.lib.bqc_state_import_host(self.h, a.ctypes.data_as(_abi.u64p)))

    def state_export_device(self, data_ptr):
        self._chk(self.lib.bqc_state_export(self.h, C.c_void_p(data_ptr)))

    def state_import_device(self, data_ptr):
        self._chk(self.lib.bqc_state_import(self.h, C.c_void_p(data_ptr)))

    def finalize_raw(self):
        p = C.POINTER(_abi.Counts)()
        self._chk(self.lib.bqc_finalize(self.h, C.byref(p)))
        self._counts = p
        return p

    def finalize(self):
        return _abi.counts_to_dict(self.finalize_raw())

    @staticmethod
    def _header(sample_id, lane_names, lane_index):
        hdr = _abi.HeaderInfo()
        names = (C.c_char_p * len(lane_names))(*[n.encode() for n in lane_names])
        idx = np.ascontiguousarray(lane_index if lane_index is not None else np.arange(len(lane_names)), np.uint32)
        hdr.sample_id = sample_id.encode()
        hdr.n_names = len(lane_names)
        hdr.lane_names = names
        hdr.lane_index = idx.ctypes.data_as(_abi.u32p)
        return hdr, (names, idx)

    def write_bamqc(self, path, sample_id="", lane_names=("",), lane_index=None):
        if self._counts is None:
            self.finalize_raw()
        hdr, keep = self._header(sample_id, lane_names, lane_index)
        self._chk(self.lib.bqc_write_bamqc(self._counts, C.byref(hdr), path.encode()))

    def qual_by_cycle(self, lane=0, mate=0):
        """The per-cycle base quality histogram of a read group and mate (0 first, 1 second) as a (n_cycles, n_q) uint64 array
        (option qual_by_cycle=N; valid after finalize)."""
        if self._counts is None:
            self.finalize_raw()
        v = _abi.QbcView()
        self._chk(self.lib.bqc_qual_by_cycle(self.h, lane, mate, C.byref(v)))
        if v.n_cycles == 0 or v.n_q == 0:
            return np.zeros((v.n_cycles, v.n_q), np.uint64)
        rows = np.ctypeslib.as_array(v.hist, shape=(v.n_cycles, v.stride))
        return rows[:, :v.n_q].copy()

    def write_qual_by_cycle(self, path, sample_id="", lane_names=("",), lane_index=None):
        if self._counts is None:
            self.finalize_raw()
        hdr, keep = self._header(sample_id, lane_names, lane_index)
        self._chk(self.lib.bqc_write_qual_by_cycle(self.h, C.byref(hdr), path.encode()))

    def mismatch_by_cycle(self, lane=0, mate=0):
        """(aligned, mismatch) of a read group and mate (0 first, 1 second): the bases compared with the genome and those of them
        that differ from it, each a (n_cycles, n_q) uint64 array (option mismatch_by_cycle=N; valid after finalize)."""
        if self._counts is None:
            self.finalize_raw()
        v = _abi.MbcView()
        self._chk(self.lib.bqc_mismatch_by_cycle(self.h, lane, mate, C.byref(v)))
        if v.n_cycles == 0 or v.n_q == 0:
            return np.zeros((v.n_cycles, v.n_q), np.uint64), np.zeros((v.n_cycles, v.n_q), np.uint64)
        return tuple(np.ctypeslib.as_array(p, shape=(v.n_cycles, v.stride))[:, :v.n_q].copy() for p in (v.aligned, v.mismatch))

    def write_mismatch_by_cycle(self, path, sample_id="", lane_names=("",), lane_index=None):
        if self._counts is None:
            self.finalize_raw()
        hdr, keep = self._header(sample_id, lane_names, lane_index)
        self._chk(self.lib.bqc_write_mismatch_by_cycle(self.h, C.byref(hdr), path.encode()))

    def adapter_by_cycle(self, lane=0, mate=0):
        """(reads_by_length, first_hit, adapters) of a read group and mate (0 first, 1 second): the examined reads by length, a
        (n_cycles,) uint64 array; per adapter of the set the reads whose first occurrence of it starts at each cycle, a
        (n_adapters, n_cycles) uint64 array; the set in use as [(name, sequence), ...] (option adapter_by_cycle=N; valid after finalize)."""
        if self._counts is None:
            self.finalize_raw()
        v = _abi.AdpView()
        self._chk(self.lib.bqc_adapter_by_cycle(self.h, lane, mate, C.byref(v)))
        names = [(v.adapters[a].name.decode(), v.adapters[a].seq.decode()) for a in range(v.n_adapters)]
        if v.n_cycles == 0:
            return np.zeros(0, np.uint64), np.zeros((v.n_adapters, 0), np.uint64), names
        e = np.ctypeslib.as_array(v.reads_by_length, shape=(v.n_cycles,)).copy()
        f = np.ctypeslib.as_array(v.first_hit, shape=(v.n_adapters, v.stride))[:, :v.n_cycles].copy()
        return e, f, names

    def write_adapter_by_cycle(self, path, sample_id="", lane_names=("",), lane_index=None):
        if self._counts is None:
            self.finalize_raw()
        hdr, keep = self._header(sample_id, lane_names, lane_index)
        self._chk(self.lib.bqc_write_adapter_by_cycle(self.h, C.byref(hdr), path.encode()))

    def gc_bias(self, lane=0):
        """(genome_windows, read_starts, bases, qual_sum) of a read group: four (101,) uint64 arrays by GC bin — the genome's windows
        (the same for every read group), the counted reads, their bases and the sum of their quality bytes (option gc_bias=W; valid
        after finalize).  The window length: gc_bias_window."""
        if self._counts is None:
            self.finalize_raw()
        v = _abi.GcbView()
        self._chk(self.lib.bqc_gc_bias(self.h, lane, C.byref(v)))
        self.gc_bias_window = int(v.window)
        return tuple(np.ctypeslib.as_array(p, shape=(v.n_bins,)).copy() for p in (v.genome_windows, v.read_starts, v.bases, v.qual_sum))

    def write_gc_bias(self, path, sample_id="", lane_names=("",), lane_index=None):
        if self._counts is None:
            self.finalize_raw()
        hdr, keep = self._header(sample_id, lane_names, lane_index)
        self._chk(self.lib.bqc_write_gc_bias(self.h, C.byref(hdr), path.encode()))

    def indel_by_cycle(self, lane=0, mate=0):
        """(reads_by_length, insertions, deletions, insertion_lengths, deletion_lengths) of a read group and mate (0 first, 1 second):
        the examined reads by length and the insertion and deletion events by cycle, three (n_cycles,) uint64 arrays, and the events by
        length, two (64,) uint64 arrays whose entry i counts length i + 1, the last one 64 and more (option indel_by_cycle=N; valid
        after finalize)."""
        if self._counts is None:
            self.finalize_raw()
        v = _abi.IbcView()
        self._chk(self.lib.bqc_indel_by_cycle(self.h, lane, mate, C.byref(v)))
        by_cycle = tuple(np.ctypeslib.as_array(p, shape=(v.n_cycles,)).copy() if v.n_cycles else np.zeros(0, np.uint64)
                         for p in (v.reads_by_length, v.insertions, v.deletions))
        return by_cycle + tuple(np.ctypeslib.as_array(p, shape=(v.n_len,)).copy() for p in (v.insertion_lengths, v.deletion_lengths))

    def write_indel_by_cycle(self, path, sample_id="", lane_names=("",), lane_index=None):
        if self._counts is None:
            self.finalize_raw()
        hdr, keep = self._header(sample_id, lane_names, lane_index)
        self._chk(self.lib.bqc_write_indel_by_cycle(self.h, C.byref(hdr), path.encode()))

    def substitutions(self, lane=0, mate=0):
        """(by_context, by_cycle) of a read group and mate (0 first, 1 second), as sequenced: by_context[strand][context][read base],
        (2, 64, 4) uint64, the context 16 * genome base before + 4 * genome base + genome base behind; by_cycle[cycle][genome base][read
        base], (n_cycles, 4, 4) uint64 (option substitutions=N; valid after finalize)."""
        if self._counts is None:
            self.finalize_raw()
        v = _abi.SbcView()
        self._chk(self.lib.bqc_substitutions(self.h, lane, mate, C.byref(v)))
        by_context = np.ctypeslib.as_array(v.by_context, shape=(2, 64, 4)).copy()
        by_cycle = np.ctypeslib.as_array(v.by_cycle, shape=(v.n_cycles, 4, 4)).copy() if v.n_cycles else np.zeros((0, 4, 4), np.uint64)
        return by_context, by_cycle

    def write_substitutions(self, path, sample_id="", lane_names=("",), lane_index=None):
        if self._counts is None:
            self.finalize_raw()
        hdr, keep = self._header(sample_id, lane_names, lane_index)
        self._chk(self.lib.bqc_write_substitutions(self.h, C.byref(hdr), path.encode()))

    def site_alleles(self, lane=0):
        """The allele counts of a read group at the given sites: counts[site][strand][base], (S, 2, 4) uint64, strand 0 forward and 1
        reverse, base A, C, G, T in genome orientation (option site_alleles=(rid, pos); valid after finalize)."""
        if self._counts is None:
            self.finalize_raw()
        v = _abi.SacView()
        self._chk(self.lib.bqc_site_alleles(self.h, lane, C.byref(v)))
        return np.ctypeslib.as_array(v.counts, shape=(v.n_sites, 2, 4)).copy()

    def write_site_alleles(self, path, ref_names, sample_id="", lane_names=("",), lane_index=None):
        """The `.sac` text; ref_names: the contigs' names by rid."""
        if self._counts is None:
            self.finalize_raw()
        hdr, keep = self._header(sample_id, lane_names, lane_index)
        names = (C.c_char_p * len(ref_names))(*[s.encode() for s in ref_names])
        self._chk(self.lib.bqc_write_site_alleles(self.h, C.byref(hdr), names, len(ref_names), path.encode()))

    def region_coverage(self, lane=0):
        """The depth of a read group over the given regions (option regions=(rid, start, end); valid after finalize): a dict of
        reads_examined, reads_on_target, aligned_bases, bases_on_target, target_bases, min_mapq, thresholds (n,), regions
        (R, 3 + n) uint64 — a region's sum, min and max of the depth, then its positions at or above each threshold — and hist
        (D + 1,), the positions by depth with the last bin open."""
        if self._counts is None:
            self.finalize_raw()
        v = _abi.RcvView()
        self._chk(self.lib.bqc_region_coverage(self.h, lane, C.byref(v)))
        n = v.n_thresholds
        return {"reads_examined": int(v.reads_examined), "reads_on_target": int(v.reads_on_target), "aligned_bases": int(v.aligned_bases),
                "bases_on_target": int(v.bases_on_target), "target_bases": int(v.target_bases), "min_mapq": int(v.min_mapq),
                "thresholds": np.ctypeslib.as_array(v.thresholds, shape=(n,)).copy() if n else np.zeros(0, np.uint64),
                "regions": np.ctypeslib.as_array(v.regions, shape=(v.n_regions, 3 + n)).copy(),
                "hist": np.ctypeslib.as_array(v.hist, shape=(v.depth_cap + 1,)).copy()}

    def write_region_coverage(self, path, ref_names, sample_id="", lane_names=("",), lane_index=None):
        """The `.rcv` text; ref_names: the contigs' names by rid."""
        if self._counts is None:
            self.finalize_raw()
        hdr, keep = self._header(sample_id, lane_names, lane_index)
        names = (C.c_char_p * len(ref_names))(*[s.encode() for s in ref_names])
        self._chk(self.lib.bqc_write_region_coverage(self.h, C.byref(hdr), names, len(ref_names), path.encode()))

    def duplicate_sets(self):
        """The duplicate sets by alignment signature over all read groups (option duplicate_sets=capacity; valid after finalize): a dict of
        capacity, sets (2,), largest (2,) and hist (2, 256) by class (0 single, 1 pair; hist[c][i - 1]: the sets of i reads, the last bin
        open), estimated_library_size, and lanes (n_lanes, 5): examined single, examined pair, flagged single, flagged pair, second ends."""
        if self._counts is None:
            self.finalize_raw()
        v = _abi.DupView()
        self._chk(self.lib.bqc_duplicate_sets(self.h, C.byref(v)))
        return {"capacity": int(v.capacity), "sets": np.array(list(v.sets), np.uint64), "largest": np.array(list(v.largest), np.uint64),
                "hist": np.stack([np.ctypeslib.as_array(v.hist[k], shape=(256,)).copy() for k in range(2)]),
                "estimated_library_size": int(v.estimated_library_size),
                "lanes": np.ctypeslib.as_array(v.lanes, shape=(v.n_lanes, 5)).copy()}

    def write_duplicate_sets(self, path, sample_id="", lane_names=("",), lane_index=None):
        """The `.dup` text."""
        if self._counts is None:
            self.finalize_raw()
        hdr, keep = self._header(sample_id, lane_names, lane_index)
        self._chk(self.lib.bqc_write_duplicate_sets(self.h, C.byref(hdr), path.encode()))

    def overrepresented(self):
        """The sets of equal read sequences over all read groups (option overrepresented=(K, capacity); valid after finalize): a dict of K,
        ppm, capacity, lanes (n_lanes, 4) — examined first, examined second, skipped first, skipped second — and by mate distinct (2,),
        largest (2,), hist (2, 256) (hist[m][i - 1]: the sets of i reads, the last bin open), threshold (2,) and listed: two lists of
        (sequence, count, possible source), sorted by count descending, then sequence."""
        if self._counts is None:
            self.finalize_raw()
        v = _abi.OvrView()
        self._chk(self.lib.bqc_overrepresented(self.h, C.byref(v)))
        return {"K": int(v.prefix_len), "ppm": int(v.ppm), "capacity": int(v.capacity),
                "lanes": np.ctypeslib.as_array(v.lanes, shape=(v.n_lanes, 4)).copy(),
                "distinct": np.array(list(v.distinct), np.uint64), "largest": np.array(list(v.largest), np.uint64),
                "hist": np.stack([np.ctypeslib.as_array(v.hist[m], shape=(256,)).copy() for m in range(2)]),
                "threshold": np.array(list(v.threshold), np.uint64),
                "listed": [[(v.listed[m][e].seq.decode(), int(v.listed[m][e].count), v.listed[m][e].source.decode()) for e in range(v.n_listed[m])] for m in range(2)]}

    def write_overrepresented(self, path, sample_id="", lane_names=("",), lane_index=None):
        """The `.ovr` text."""
        if self._counts is None:
            self.finalize_raw()
        hdr, keep = self._header(sample_id, lane_names, lane_index)
        self._chk(self.lib.bqc_write_overrepresented(self.h, C.byref(hdr), path.encode()))

    def window_depth(self, lane=0):
        """The depth of a read group in fixed genome windows (option window_depth=(W, ref_len); valid after finalize): a dict of window,
        min_mapq, n_windows, woff (n_refs + 1,), ref_len (n_refs,), reads_examined, reads_low_mapq, bases_outside, the planes reads, bases
        and bases_low (NW,) uint64, contigs (n_refs, 3) — a contig's sums of the three planes — and hist (1001,), the main contigs' windows
        by floor(bases / length) with the last bin open."""
        if self._counts is None:
            self.finalize_raw()
        v = _abi.WdpView()
        self._chk(self.lib.bqc_window_depth(self.h, lane, C.byref(v)))
        nw, nr = v.n_windows, v.n_refs
        arr = lambda p, shape, dt: np.ctypeslib.as_array(p, shape=shape).copy() if shape[0] else np.zeros(shape, dt)
        return {"window": int(v.window), "min_mapq": int(v.min_mapq), "n_windows": int(nw), "woff": arr(v.woff, (nr + 1,), np.uint32),
                "ref_len": arr(v.ref_len, (nr,), np.uint32), "reads_examined": int(v.reads_examined), "reads_low_mapq": int(v.reads_low_mapq),
                "bases_outside": int(v.bases_outside), "reads": arr(v.reads, (nw,), np.uint64), "bases": arr(v.bases, (nw,), np.uint64),
                "bases_low": arr(v.bases_low, (nw,), np.uint64), "contigs": arr(v.contigs, (nr, 3), np.uint64),
                "hist": np.ctypeslib.as_array(v.hist, shape=(1001,)).copy()}

    def write_window_depth(self, path, ref_names, sample_id="", lane_names=("",), lane_index=None):
        """The `.wdp` text; ref_names: the contigs' names by rid."""
        if self._counts is None:
            self.finalize_raw()
        hdr, keep = self._header(sample_id, lane_names, lane_index)
        names = (C.c_char_p * len(ref_names))(*[s.encode() for s in ref_names])
        self._chk(self.lib.bqc_write_window_depth(self.h, C.byref(hdr), names, len(ref_names), path.encode()))

    def close(self):
        if self.h:
            self.lib.bqc_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
