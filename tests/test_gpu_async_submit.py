"""GPU: the asynchronous and anchored submit paths of the C ABI (include/bamqc.h: bqc_submit_async, bqc_batch_uploaded,
bqc_anchor_*, bqc_submit_anchored) against the oracle, used the way an outside caller may use them: columns in page-locked memory
reused as soon as bqc_batch_uploaded says 1, the three slots wrapping while they grow, payload columns in device memory, errors
found by the card while batches are in flight, anchored batches pipelined without a sync on the compute stream, an anchored shard,
and the life cycle of an anchor handle."""
import ctypes as C
import mmap
import time

import numpy as np
import pytest

from bamqc_amd import Aggregator, _abi, _lib, synth
from tests import synth as tsynth
from tests.hipmem import Hip
from tests.parity import run_oracle, split
from tests.anchor_recurrence import reference_anchors
from tests.test_gpu_anchor import device_batch, with_positions
from tests.test_gpu_fuzz import wild_batch

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_AS_TAG, ERR_RANGE, ERR_STATE = 1, 4, 6, 8
POLL_LIMIT_S = 60.0
_EXTRA = [("nm_extra_read", "xr", np.uint32, _abi.u32p), ("nm_extra_val", "xv", np.int32, _abi.i32p)]


def _bytes(cols):
    _, keep = _abi.make_batch(cols)
    return sum(((a.nbytes + 255) & ~255) for a in keep.values()) + 4096


class Pinned:
    """One batch's columns in page-locked host memory: an anonymous mapping (page-aligned) registered with bqc_host_register."""

    def __init__(self, lib, nbytes):
        self.lib = lib
        self.nbytes = (nbytes + mmap.PAGESIZE - 1) // mmap.PAGESIZE * mmap.PAGESIZE
        self.mm = mmap.mmap(-1, self.nbytes)
        self.buf = np.frombuffer(self.mm, np.uint8)
        self.base = self.buf.ctypes.data
        self.registered = self.lib.bqc_host_register(C.c_void_p(self.base), self.nbytes) == 0
        assert self.registered
        self.view = {}

    def fill(self, cols, device_payload=None):
        """the batch into this buffer; returns its bqc_batch.  device_payload: {seq, qual, cigar: device pointer} (those columns
        then live in device memory, the fixed ones here)"""
        b, keep = _abi.make_batch(cols)
        at = 0
        self.view = {}
        for name, dt, pt in _abi._BATCH_COLS:
            if device_payload is not None and name in device_payload:
                setattr(b, name, C.cast(device_payload[name], pt))
                continue
            a = keep[name]
            assert at + a.nbytes <= self.nbytes
            v = self.buf[at:at + a.nbytes].view(dt)
            v[:] = a
            self.view[name] = v
            setattr(b, name, C.cast(C.c_void_p(self.base + at), pt))
            at = (at + a.nbytes + 255) & ~255
        for field, key, dt, pt in _EXTRA:
            a = keep[key]
            assert at + a.nbytes <= self.nbytes
            self.buf[at:at + a.nbytes].view(dt)[:] = a
            setattr(b, field, C.cast(C.c_void_p(self.base + at), pt))
            at = (at + a.nbytes + 255) & ~255
        return b

    def disturb(self):
        """overwrite the batch in place with a valid but different one: qualities shifted inside 0..60, bases rotated (A C G T),
        positions moved; qualities first (the column the host-to-device copy reaches last but one)"""
        v = self.view
        if "qual" in v and v["qual"].size:
            q = v["qual"]
            has = q != 0xFF
            np.add(q, 7, out=q, where=has)
            np.remainder(q, 61, out=q, where=has)
        if "seq" in v and v["seq"].size:
            v["seq"][:] = _ROT[v["seq"]]
        if "pos" in v and v["pos"].size:
            p = v["pos"]
            np.add(p, 7, out=p, where=p >= 0)

    def close(self):
        if self.registered:
            assert self.lib.bqc_host_unregister(C.c_void_p(self.base)) == 0
            self.registered = False
        self.view = {}
        self.buf = None


def _rot_table():
    nib = np.arange(16, dtype=np.uint8)
    rot = nib.copy()
    rot[1], rot[2], rot[4], rot[8] = 2, 4, 8, 1  # A -> C -> G -> T -> A
    b = np.arange(256, dtype=np.uint16)
    return ((rot[b >> 4].astype(np.uint16) << 4) | rot[b & 15]).astype(np.uint8)


_ROT = _rot_table()


def wait_uploaded(lib, h, ticket, wait):
    """bqc_batch_uploaded until it says 1: blocking (wait=1), or polled under a wall-clock limit (wait=0)"""
    if wait:
        rc = lib.bqc_batch_uploaded(h, ticket, 1)
        assert rc == 1, rc
        return
    limit = time.monotonic() + POLL_LIMIT_S
    while True:
        rc = lib.bqc_batch_uploaded(h, ticket, 0)
        assert rc in (0, 1), rc
        if rc == 1:
            return
        if time.monotonic() > limit:
            pytest.fail("bqc_batch_uploaded(%d) still 0 after %.0f s" % (ticket, POLL_LIMIT_S))
        time.sleep(0.0002)


def submit_async(lib, agg, b):
    t = C.c_uint64(12345)
    rc = lib.bqc_submit_async(agg.h, C.byref(b), C.byref(t))
    return rc, int(t.value)


def finalize_or_code(agg):
    try:
        return 0, agg.finalize()
    except Exception as e:  # BamQCError
        return getattr(e, "code", -1), None


def assert_counts(want, got):
    d = _abi.diff_counts(want, got)
    assert not d, "\n".join(d[:20])


def gpu_ctx(refs, **opts):
    a = Aggregator(**opts)
    for i, r in enumerate(refs):
        a.set_reference(i, r)
    return a


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. columns reused once bqc_batch_uploaded says 1
# ---------------------------------------------------------------------------------------------------------------------------------
def test_pinned_columns_reused_after_uploaded():
    """A ring of 2 registered buffers (fewer than the 3 slots) carries 8 batches; each is refilled only once the ticket that last
    used it is reported uploaded (waited for and polled in turn).  After the last submit every buffer is overwritten with a valid but
    different batch: a copy made too late gives other counts."""
    lib = _lib.load()
    lens = [3_000_000]
    refs = [synth.reference(11, 0, lens[0])]
    sizes = [20_000, 1, 60_000, 7, 90_000, 35_000, 2_000, 400_000]
    read_lens = [150, 100, 250, 150, 75, 150, 250, 150]
    batches = [synth.batch(200 + i, n, lens, refs, read_len=L, n_lanes=2) for i, (n, L) in enumerate(zip(sizes, read_lens))]
    opts = dict(n_refs=1, n_lanes=2, klist=[31], qlist=[17])
    rc, want, _ = run_oracle(batches, refs, **opts)
    assert rc == 0
    cap = max(_bytes(c) for c in batches)
    ring = []
    agg = gpu_ctx(refs, **opts)
    try:
        ring = [Pinned(lib, cap) for _ in range(2)]
        last = [0, 0]
        prev = 0
        for i, cols in enumerate(batches):
            j = i % 2
            if last[j]:
                wait_uploaded(lib, agg.h, last[j], wait=i % 4 < 2)
            b = ring[j].fill(cols)
            rc, t = submit_async(lib, agg, b)
            assert rc == 0, (lib.bqc_last_error(agg.h) or b"").decode()
            assert t > prev
            prev = last[j] = t
        # the last batch's buffer first: its copy may still be on its way
        for k, j in enumerate(((len(batches) - 1) % 2, len(batches) % 2)):
            wait_uploaded(lib, agg.h, last[j], wait=k)
            ring[j].disturb()
        got = agg.finalize()
        assert_counts(want, got)
        assert any(s[2] for s in got[0]["sketch"])  # (the sketch ran)
    finally:
        agg.close()
        for p in ring:
            p.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. the three slots wrapping while they grow
# ---------------------------------------------------------------------------------------------------------------------------------
def _long_reads(seed, lens, refs):
    # (the generator's long-read plan clips up to 2 000 bases: it takes reads of 3 000 and more, the shorter ones get the usual plan)
    parts = [synth.batch(seed + k, n, lens, refs, read_len=L, long_reads=L >= 3_000) for k, (n, L) in
             enumerate(((150, 300), (60, 3_000), (20, 12_000), (40, 1_000)))]
    return tsynth.concat(parts)


def test_slots_wrap_and_grow_without_a_sync():
    """Batches of 1, 200 000, 0, 3, 1 000 000 reads, long reads (k_long), then 150 bp again: every slot's page-locked image and device
    memory grow while the other two slots are in flight, with no sync in between."""
    lib = _lib.load()
    lens = [6_000_000]
    refs = [synth.reference(13, 0, lens[0])]
    kinds = [1, 200_000, 0, 3, 1_000_000, "long", 5_000, 0, 150_000, 2, "long", 40_000, 1]
    batches = []
    for i, k in enumerate(kinds):
        if k == "long":
            batches.append(_long_reads(400 + 10 * i, lens, refs))
        elif k == 0:
            batches.append(tsynth.slice_batch(synth.batch(400 + i, 8, lens, refs), 0, 0))
        else:
            batches.append(synth.batch(400 + i, k, lens, refs))
    opts = dict(n_refs=1, max_read_len=16_384)
    rc, want, _ = run_oracle(batches, refs, **opts)
    assert rc == 0
    pinned = []
    agg = gpu_ctx(refs, **opts)
    try:
        tickets = []
        for cols in batches:
            p = Pinned(lib, _bytes(cols))
            pinned.append(p)
            rc, t = submit_async(lib, agg, p.fill(cols))
            assert rc == 0, (lib.bqc_last_error(agg.h) or b"").decode()
            if len(cols["flag"]) == 0:
                assert t == 0
            else:
                assert not tickets or t > tickets[-1], (tickets, t)
                tickets.append(t)
        assert len(tickets) >= 10
        assert lib.bqc_batch_uploaded(agg.h, 0, 0) == 1
        assert lib.bqc_batch_uploaded(agg.h, tickets[-1] + 1 + 5, 0) == 1
        assert_counts(want, agg.finalize())
    finally:
        agg.close()
        for p in pinned:
            p.close()
    staged = gpu_ctx(refs, **opts)
    try:
        for cols in batches:
            staged.submit(cols)
        assert_counts(want, staged.finalize())
    finally:
        staged.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. payload columns in device memory
# ---------------------------------------------------------------------------------------------------------------------------------
def _with_nm_extra(cols, rng, every=5):
    """further NM values (a record with several NM tags) for every `every`-th mapped read: NM itself + 0..3"""
    c = dict(cols)
    n = len(cols["flag"])
    idx = np.flatnonzero((np.arange(n) % every == 0) & (cols["nm"] >= 0))
    reads, vals = [], []
    for i in idx:
        for _ in range(int(rng.integers(1, 3))):
            reads.append(i)
            vals.append(int(cols["nm"][i]) + int(rng.integers(0, 4)))
    c["nm_extra_read"] = np.array(reads, np.uint32)
    c["nm_extra_val"] = np.array(vals, np.int32)
    return c


def _device_payload(hip, cols):
    _, keep = _abi.make_batch(cols)
    return {name: hip.put(keep[name], front=512, extra=512) for name in ("seq", "qual", "cigar")}


@pytest.mark.parametrize("kind", ["synthetic", "wild"])
def test_device_payload_columns(kind):
    """seq / qual / cigar in device memory, the fixed columns in page-locked host memory; with further NM values and reads
    without qualities (synthetic), or wild records in three read groups.  bqc_submit refuses such a batch."""
    lib = _lib.load()
    rng = np.random.default_rng(17)
    if kind == "synthetic":
        cols, refs = tsynth.synth(seed=23, n_reads=40_000, n_refs=2, ref_len=400_000, p_noqual=0.03, var_len=True)
        batches = split(cols, [1, 9_000, 9_003, 25_000])
        batches = [_with_nm_extra(c, rng) if i in (1, 3) else c for i, c in enumerate(batches)]
        assert all(np.any(c["flag"] & 0x8000) for c in batches[1:]) and sum(len(c.get("nm_extra_read", ())) for c in batches) > 1000
        opts = dict(n_refs=2)
    else:
        cols, refs = wild_batch(501, 6_000)
        batches = split(cols, [1, 2_000, 2_001, 4_500])
        opts = dict(n_refs=len(refs), n_lanes=3, max_read_len=1024, isize=2000)
    rc_o, want, _ = run_oracle(batches, refs, **opts)
    hip = Hip()
    pinned = []
    agg = gpu_ctx(refs, **opts)
    try:
        dev = [_device_payload(hip, c) for c in batches]
        p0 = Pinned(lib, _bytes(batches[1]))
        pinned.append(p0)
        assert lib.bqc_submit(agg.h, C.byref(p0.fill(batches[1], dev[1]))) == ERR_ARG  # (the staged path copies with the host's memcpy)
        rc_g = 0
        for cols, d in zip(batches, dev):
            p = Pinned(lib, _bytes(cols))
            pinned.append(p)
            rc_g, t = submit_async(lib, agg, p.fill(cols, d))
            if rc_g:
                break
        if not rc_g:
            rc_g, got = finalize_or_code(agg)
        assert rc_g == rc_o, (rc_o, rc_g, (lib.bqc_last_error(agg.h) or b"").decode())
        if rc_o == 0:
            assert_counts(want, got)
    finally:
        agg.close()
        hip.free()
        for p in pinned:
            p.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. errors found by the card while batches are in flight
# ---------------------------------------------------------------------------------------------------------------------------------
QUAL_MSG = b"base quality above 222"


def _first_error_in_flight(lib, agg, stream, pinned):
    """the batches through bqc_submit_async without a sync: the first nonzero return code, from whichever call it surfaces at"""
    for cols in stream:
        p = Pinned(lib, _bytes(cols))
        pinned.append(p)
        rc, _ = submit_async(lib, agg, p.fill(cols))
        if rc:
            return rc
    return lib.bqc_sync(agg.h)


def test_first_error_in_stream_order_with_batches_in_flight():
    """Five batches in flight: the second has a Phred > 222, the third a negative AS.  The first error the caller sees is the
    second batch's (BQC_ERR_RANGE: the HIP path refuses what the reference's q + 33 would wrap, tests/test_gpu_value_limits.py; the
    oracle has no such refusal); without the second batch it is the third's, BQC_ERR_AS_TAG as the oracle's.  The context then
    refuses batches with BQC_ERR_STATE until bqc_reset, after which a clean stream matches the oracle again."""
    lib = _lib.load()
    lens = [2_000_000]
    refs = [synth.reference(19, 0, lens[0])]
    batches = [synth.batch(600 + i, 30_000, lens, refs) for i in range(5)]
    bad_q = dict(batches[1])
    bad_q["qual"] = bad_q["qual"].copy()
    bad_q["qual"][len(bad_q["qual"]) // 2] = 230
    bad_as = dict(batches[2])
    bad_as["as_"] = np.full(len(bad_as["flag"]), -7, np.int32)
    opts = dict(n_refs=1, klist=[17], qlist=[17])
    no_q = [batches[0], batches[1], bad_as, batches[3], batches[4]]
    rc_o, _, _ = run_oracle(no_q, refs, **opts)
    assert rc_o == ERR_AS_TAG
    clean = [batches[0], batches[4]]
    rc, want, _ = run_oracle(clean, refs, **opts)
    assert rc == 0
    pinned = []
    ctxs = []
    try:
        agg = gpu_ctx(refs, **opts)
        ctxs.append(agg)
        rc = _first_error_in_flight(lib, agg, no_q, pinned)
        assert rc == rc_o, (rc, (lib.bqc_last_error(agg.h) or b"").decode())
        agg = gpu_ctx(refs, **opts)
        ctxs.append(agg)
        rc = _first_error_in_flight(lib, agg, [batches[0], bad_q, bad_as, batches[3], batches[4]], pinned)
        assert rc == ERR_RANGE and QUAL_MSG in (lib.bqc_last_error(agg.h) or b""), (rc, lib.bqc_last_error(agg.h))
        p = Pinned(lib, _bytes(batches[3]))
        pinned.append(p)
        rc, _ = submit_async(lib, agg, p.fill(batches[3]))
        assert rc == ERR_STATE
        assert lib.bqc_reset(agg.h) == 0
        for cols in clean:
            p = Pinned(lib, _bytes(cols))
            pinned.append(p)
            rc, _ = submit_async(lib, agg, p.fill(cols))
            assert rc == 0, (lib.bqc_last_error(agg.h) or b"").decode()
        assert_counts(want, agg.finalize())
    finally:
        for a in ctxs:
            a.close()
        for p in pinned:
            p.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. anchored batches pipelined as an outside decoder would
# ---------------------------------------------------------------------------------------------------------------------------------
class DevSet:
    """device buffers for one batch at a time (every column, 1 KiB of the same allocation on either side, and the anchors)"""

    def __init__(self, hip, n_cap, payload_cap):
        self.hip = hip
        self.ptr, self.used = {}, {}
        for name, dt, pt in _abi._BATCH_COLS:
            nb = payload_cap[name] if name in payload_cap else n_cap * np.dtype(dt).itemsize
            self.ptr[name] = (hip.alloc(max(nb, 4), front=1024, extra=1024), nb)
        self.d_cov = (hip.alloc(8 * max(n_cap, 1)), 8 * n_cap)
        self.n = 0

    def fill(self, cols):
        _, keep = _abi.make_batch(cols)
        b = _abi.Batch()
        b.n_reads = self.n = len(cols["flag"])
        for name, dt, pt in _abi._BATCH_COLS:
            p, cap = self.ptr[name]
            a = keep[name][:self.n] if name not in ("seq", "qual", "cigar") else np.asarray(cols[name], dt)
            assert a.nbytes <= cap
            self.hip.write(p, a)
            self.used[name] = a.nbytes
            setattr(b, name, C.cast(p, pt))
        return b, (self.d_cov[0] if self.n else None)

    def poison(self):
        """overwrite what the batch used (the kernels must be through with it): zero columns, anchors BQC_COV_NONE"""
        for name, (p, _) in self.ptr.items():
            self.hip.memset(p, 0, self.used.get(name, 0))
        self.hip.memset(self.d_cov[0], 0xFF, 8 * self.n)
        self.used = {}


def _anchor_stream(seed):
    lens = [150_000_000]
    ref = synth.reference(seed, 0, lens[0])
    near = [2_000_000]
    head = [ref[:near[0]]]
    small = synth.batch(seed + 1, 20_000, near, head)
    base = synth.batch(seed + 2, 150_000, near, head)
    rng = np.random.default_rng(seed)
    gaps = rng.integers(900, 1000, size=150_000)  # no break: one slide per read, 140 000 windows > bqc_anchored::kInline
    gaps[::15_000] = 2_500                        # and a few resets
    sparse = with_positions(base, np.cumsum(gaps) + 10)
    big = synth.batch(seed + 3, 1_100_000, [20_000_000], [ref[:20_000_000]])  # > 1 048 576 reads: the engine's scratch grows
    empty = tsynth.slice_batch(small, 0, 0)
    batches = [small, sparse, empty, synth.batch(seed + 4, 3, near, head), big, synth.batch(seed + 5, 50_000, near, head),
               tsynth.slice_batch(small, 0, 1), synth.batch(seed + 6, 30_000, near, head)]
    return batches, [ref]


def test_anchored_batches_pipelined():
    """enqueue k -> sync its stream -> complete k -> submit_anchored k, up to three submitted batches in flight, no sync on the
    compute stream; a batch's device columns and anchors are overwritten as soon as its ticket is reported uploaded (which for an anchored
    batch means its kernels are through) and reused for a later batch."""
    lib = _lib.load()
    batches, refs = _anchor_stream(31)
    rc, want, _ = run_oracle(batches, refs, n_refs=1)
    assert rc == 0
    n_cap = max(len(c["flag"]) for c in batches)
    payload_cap = {k: max(np.asarray(c[k]).nbytes for c in batches) for k in ("seq", "qual", "cigar")}
    hip = Hip()
    agg = gpu_ctx(refs, n_refs=1)
    try:
        sets = [DevSet(hip, n_cap, payload_cap) for _ in range(3)]
        st = hip.stream()
        owner = [0, 0, 0]          # ticket of the batch each set holds (0: free)
        state = (True, 0, 0, 0)
        saw_rest = False
        for k, cols in enumerate(batches):
            j = k % 3
            if owner[j]:
                wait_uploaded(lib, agg.h, owner[j], wait=1)
                sets[j].poison()
                owner[j] = 0
            b, d_cov = sets[j].fill(cols)
            h = C.c_void_p()
            rc = lib.bqc_anchor_enqueue(agg.h, C.byref(b), d_cov, st, C.byref(h))
            assert rc == 0, (rc, (lib.bqc_anchor_error(agg.h) or b"").decode())
            hip.sync_stream(st)
            rc = lib.bqc_anchor_complete(agg.h, h, None)
            assert rc == 0, (rc, (lib.bqc_anchor_error(agg.h) or b"").decode())
            n = len(cols["flag"])
            win, off, state = reference_anchors(cols, state, 1, [1])
            if n:
                cov = hip.get(d_cov, 8 * n, np.uint32).reshape(-1, 2)
                assert np.array_equal(cov[:, 0].astype(np.uint64), win), k
                cand = win != 0xFFFFFFFF
                assert np.array_equal(cov[cand, 1], off[cand]), k
                saw_rest |= bool(cand.any()) and int(win[cand].max()) + 1 > (1 << 17)
            t = C.c_uint64(99)
            rc = lib.bqc_submit_anchored(agg.h, C.byref(b), h, C.byref(t))
            assert rc == 0, (lib.bqc_last_error(agg.h) or b"").decode()
            assert (t.value == 0) == (n == 0)
            if t.value:
                owner[j] = int(t.value)
            else:
                sets[j].poison()
            for i in range(3):  # the others as soon as they are reported through: a batch still being read would see the overwrite
                if owner[i] and i != j and lib.bqc_batch_uploaded(agg.h, owner[i], 0) == 1:
                    sets[i].poison()
                    owner[i] = 0
        assert saw_rest
        assert_counts(want, agg.finalize())
    finally:
        agg.close()
        hip.free()


# ---------------------------------------------------------------------------------------------------------------------------------
# 6. an anchored shard
# ---------------------------------------------------------------------------------------------------------------------------------
def test_anchored_shard_adds_up_with_an_async_predecessor():
    """The stream's head through bqc_submit_async; its tail through anchored batches of a shard_tail context, whose first reads are
    set aside on the card, then resolved from the head's exported state.  The two state vectors add up to the whole stream."""
    lib = _lib.load()
    lens = [2_000_000, 1_000_000]
    refs = [synth.reference(37, i, n) for i, n in enumerate(lens)]
    cols = synth.batch(37, 60_000, lens, refs)
    c1 = int(np.searchsorted(cols["rid"], 1))
    cuts = [12_000, 30_000, 33_000, c1 + 500, 52_000]
    parts = split(cols, cuts)
    head, tail = parts[:2], parts[2:]
    assert c1 > 33_000
    rc, want, _ = run_oracle(parts, refs, n_refs=2)
    assert rc == 0
    hip = Hip()
    pinned = []
    pred = gpu_ctx(refs, n_refs=2)
    succ = gpu_ctx(refs, n_refs=2, shard_tail=1)
    total = gpu_ctx(refs, n_refs=2)
    try:
        for c in head:
            p = Pinned(lib, _bytes(c))
            pinned.append(p)
            rc, _ = submit_async(lib, pred, p.fill(c))
            assert rc == 0
        pending = 0
        st = hip.stream()
        for c in tail:
            b, d_cov = device_batch(hip, c)
            h = C.c_void_p()
            assert lib.bqc_anchor_enqueue(succ.h, C.byref(b), d_cov, st, C.byref(h)) == 0, (lib.bqc_anchor_error(succ.h) or b"").decode()
            hip.sync_stream(st)
            assert lib.bqc_anchor_complete(succ.h, h, None) == 0, (lib.bqc_anchor_error(succ.h) or b"").decode()
            cov = hip.get(d_cov, 8 * len(c["flag"]), np.uint32).reshape(-1, 2)
            pending += int((cov[:, 0] == 0xFFFFFFFE).sum())
            assert lib.bqc_submit_anchored(succ.h, C.byref(b), h, None) == 0, (lib.bqc_last_error(succ.h) or b"").decode()
        nbytes = int(lib.bqc_shard_state_bytes(pred.h))
        buf = np.zeros(nbytes, np.uint8)
        assert lib.bqc_shard_export(pred.h, buf.ctypes.data_as(C.c_void_p)) == 0, (lib.bqc_last_error(pred.h) or b"").decode()
        assert lib.bqc_shard_resolve(succ.h, buf.ctypes.data_as(C.c_void_p)) == 0, (lib.bqc_last_error(succ.h) or b"").decode()
        vec = pred.state_export_host() + succ.state_export_host()
        total.state_import_host(vec)
        assert_counts(want, total.finalize())
        assert pending > 1000, pending  # (the tail's reads on the first contig were set aside)
    finally:
        for a in (pred, succ, total):
            a.close()
        hip.free()
        for p in pinned:
            p.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# 7. the life cycle of an anchor handle
# ---------------------------------------------------------------------------------------------------------------------------------
def _dense_pair(seed):
    refs = [synth.reference(seed, 0, 30_000_000)]
    near = [2_000_000]  # (the reads on the contig's first 2 Mb: dense)
    head = [refs[0][:near[0]]]
    return [synth.batch(seed + 1, 40_000, near, head), synth.batch(seed + 2, 25_000, near, head)], refs


def test_anchor_handle_lifecycle():
    lib = _lib.load()
    (a_cols, b_cols), refs = _dense_pair(43)
    rc, want, _ = run_oracle([a_cols, b_cols], refs, n_refs=1)
    assert rc == 0
    hip = Hip()
    pinned = []
    ctxs = []
    try:
        st = hip.stream()
        # (1) one outstanding handle: a second enqueue is refused and leaves the card's state alone
        agg = gpu_ctx(refs, n_refs=1)
        ctxs.append(agg)
        ba, cov_a = device_batch(hip, a_cols)
        bb, cov_b = device_batch(hip, b_cols)
        ha, hb = C.c_void_p(), C.c_void_p()
        assert lib.bqc_anchor_enqueue(agg.h, C.byref(ba), cov_a, st, C.byref(ha)) == 0
        hip.sync_stream(st)
        assert lib.bqc_anchor_enqueue(agg.h, C.byref(bb), cov_b, st, C.byref(hb)) == -ERR_STATE
        assert b"completed" in (lib.bqc_anchor_error(agg.h) or b"")
        hip.sync_stream(st)
        assert lib.bqc_anchor_complete(agg.h, ha, None) == 0
        win, off, state = reference_anchors(a_cols, (True, 0, 0, 0), 1, [1])
        cov = hip.get(cov_a, 8 * len(a_cols["flag"]), np.uint32).reshape(-1, 2)
        assert np.array_equal(cov[:, 0].astype(np.uint64), win)
        assert lib.bqc_submit_anchored(agg.h, C.byref(ba), ha, None) == 0
        assert lib.bqc_anchor_enqueue(agg.h, C.byref(bb), cov_b, st, C.byref(hb)) == 0
        hip.sync_stream(st)
        assert lib.bqc_anchor_complete(agg.h, hb, None) == 0
        win, off, state = reference_anchors(b_cols, state, 1, [1])
        cov = hip.get(cov_b, 8 * len(b_cols["flag"]), np.uint32).reshape(-1, 2)
        assert np.array_equal(cov[:, 0].astype(np.uint64), win)
        assert lib.bqc_submit_anchored(agg.h, C.byref(bb), hb, None) == 0
        assert_counts(want, agg.finalize())

        # (2) a discarded handle (enqueued only, or completed but not submitted) ends anchoring: the next enqueue says 1
        for complete_first in (False, True):
            agg = gpu_ctx(refs, n_refs=1)
            ctxs.append(agg)
            ba, cov_a = device_batch(hip, a_cols)
            bb, cov_b = device_batch(hip, b_cols)
            ha, hb = C.c_void_p(), C.c_void_p()
            assert lib.bqc_anchor_enqueue(agg.h, C.byref(ba), cov_a, st, C.byref(ha)) == 0
            hip.sync_stream(st)
            if complete_first:
                assert lib.bqc_anchor_complete(agg.h, ha, None) == 0
            lib.bqc_anchor_discard(agg.h, ha)
            assert lib.bqc_anchor_enqueue(agg.h, C.byref(bb), cov_b, st, C.byref(hb)) == 1
            for c in (a_cols, b_cols):
                p = Pinned(lib, _bytes(c))
                pinned.append(p)
                rc, _ = submit_async(lib, agg, p.fill(c))
                assert rc == 0, (lib.bqc_last_error(agg.h) or b"").decode()
            assert_counts(want, agg.finalize())

        # (3) complete says 1 (more breaks than the card's chain takes): the handle is released with it
        agg = gpu_ctx(refs, n_refs=1)
        ctxs.append(agg)
        sparse = with_positions(a_cols, np.arange(20_000, dtype=np.int64) * 1_200 + 3)  # (every read a break: 20 000 > 16 384)
        bs, cov_s = device_batch(hip, sparse)
        hs = C.c_void_p()
        assert lib.bqc_anchor_enqueue(agg.h, C.byref(bs), cov_s, st, C.byref(hs)) == 0
        hip.sync_stream(st)
        assert lib.bqc_anchor_complete(agg.h, hs, None) == 1
        assert lib.bqc_reset(agg.h) == 0  # (anchoring starts over: no handle may still count as outstanding)
        ba, cov_a = device_batch(hip, a_cols)
        ha = C.c_void_p()
        assert lib.bqc_anchor_enqueue(agg.h, C.byref(ba), cov_a, st, C.byref(ha)) == 0, (lib.bqc_anchor_error(agg.h) or b"").decode()
        hip.sync_stream(st)
        assert lib.bqc_anchor_complete(agg.h, ha, None) == 0
        assert lib.bqc_submit_anchored(agg.h, C.byref(ba), ha, None) == 0
        agg.submit(b_cols)
        assert_counts(want, agg.finalize())
    finally:
        for a in ctxs:
            a.close()
        hip.free()
        for p in pinned:
            p.close()
