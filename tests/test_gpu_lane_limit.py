"""GPU: the library at the read-group limit, through the C ABI: 64 to 256 read groups on every path that is indexed by read group
(the batches: tests/lane_limit.py; that they cross the edges they are named for: tests/test_lane_limit_cpu.py).  Every comparison
is exact.

* the core statistics against the oracle: streams of 65 and 256 groups, batches of one read group each from different words of the
  read-group mask in one context (the 8-mer folds of finalize), and the one out-of-range value a byte can take with 255 groups;
* the anchors and the processing order on the card at 64, 65, 128, 129, 255 and 256 groups (bits_for(n - 1) and bits_for(n) ballots);
* the k-mer sketch's tables, one per read group, at 65 and 256 groups;
* each of the nine optional modules at 256 groups against its own restatement, alone and all at once, and three writers with 256
  lane blocks in a permuted order."""
import ctypes as C
import functools
import hashlib

import numpy as np
import pytest

from bamqc_amd import Aggregator, BamQCError, _abi, _lib
from tests import adp_ref, dup_ref, ibc_ref, mbc_ref, qbc_ref, rcv_ref, sbc_ref, synth
from tests import lane_limit as ll
from tests import sketch_state as ss
from tests.cycle_steps import processing_order
from tests.hipmem import Hip
from tests.oracle_lib import Oracle
from tests.parity import assert_parity, run_oracle
from tests.test_gpu_anchor_read_groups import run_stream

pytestmark = pytest.mark.gpu
CORE = dict(max_read_len=1024, isize=2000)


# ---------------------------------------------------------------------------------------------------------------------------
# 1. the core statistics against the oracle
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [65, 256])
def test_stream_against_the_oracle(N):
    assert_parity(ll.stream(N), ll.refs(), n_lanes=N, **CORE)


def test_one_group_per_batch_from_every_mask_word():
    """solo batches of groups 63, 64, 127, 128, 191, 192 and 255 in ONE context, no reset: at finalize read groups of all four words of
    t8_lanes have 8-mer rows waiting to be folded"""
    batches = [ll.solo(256, g, k * ll.SOLO_READS) for k, g in enumerate(ll.SOLO_GROUPS)]
    co, cg, _, a = assert_parity(batches, ll.refs(), n_lanes=256, **CORE)
    for g in ll.SOLO_GROUPS:
        assert int(cg[g]["eightmer"].sum()) > 50_000, g
    assert not any(int(cg[g]["eightmer"].sum()) for g in range(256) if g not in ll.SOLO_GROUPS)
    a.close()


def test_read_group_255_of_255_is_the_oracles_error_and_reset_recovers():
    """n_lanes = 255: a byte's only out-of-range value.  The batch that holds it fails with the oracle's code; after bqc_reset the same
    context takes the stream of 255 groups and gives the oracle's counts."""
    good = ll.stream(255)
    bad = ll.sprinkled(255, seed=7)
    lane = np.array(bad["lane"], copy=True)
    lane[501] = 255
    bad = dict(bad, lane=lane)
    rc_o, _, _ = run_oracle([good[1], bad], ll.refs(), n_refs=2, n_lanes=255, **CORE)
    assert rc_o != 0
    a = Aggregator(n_refs=2, n_lanes=255, **CORE)
    for i, r in enumerate(ll.refs()):
        a.set_reference(i, r)
    a.submit(good[1])
    with pytest.raises(BamQCError) as e:
        a.submit(bad)
        a.finalize()
    assert e.value.code == rc_o, e.value
    assert "lane" in str(e.value)
    a.reset()
    for b in good:
        a.submit(b)
    got = a.finalize()
    rc, want, _ = run_oracle(good, ll.refs(), n_refs=2, n_lanes=255, **CORE)
    assert rc == 0
    d = _abi.diff_counts(want, got)
    assert not d, "\n".join(d[:20])
    a.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 2. anchors and processing order on the card
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", ll.COUNTS)
def test_anchored_stream(N):
    """per batch the windows and offsets of per_group_anchors; bqc_submit_anchored and bqc_submit leave the same state words, and both
    give the oracle's counts"""
    run_stream(ll.stream(N), ll.refs(), N, state_words=True)


def device_order(lib, hip, lane, n_lanes):
    """bqc_launch_lane_order (csrc/anchor.h) on a lane column in device memory -> the order"""
    n = len(lane)
    d_lane = hip.put(np.ascontiguousarray(lane, np.uint8), extra=1024)
    d_order = hip.alloc(4 * n)
    d_tmp = hip.alloc(4 * ((n + 1023) // 1024 * (n_lanes + 1) + 64))  # lane_order_tmp_words
    lib.bqc_launch_lane_order.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.bqc_launch_lane_order.restype = None
    lib.bqc_launch_lane_order(d_lane, n, n_lanes, d_order, d_tmp, None)
    assert hip.rt.hipDeviceSynchronize() == 0
    return hip.get(d_order, 4 * n, np.uint32)


@pytest.mark.parametrize("N", ll.COUNTS)
def test_processing_order_on_the_card(N):
    """k_lo_count / k_lo_scan / k_lo_scatter: the order of every layout is the stable order by read group; a column that also holds
    values at and above N (bin 0, in front of read group 0, beside the key N of read group N - 1) is ordered by the kernel's keys"""
    lib = _lib.load()
    hip = Hip()
    try:
        for name, cols in ll.stream_parts(N) + [("stream", synth.concat(ll.stream(N)))]:
            got = device_order(lib, hip, cols["lane"], N)
            assert np.array_equal(got, processing_order(cols["lane"])), name
        wild = np.random.default_rng(N).integers(0, 256, 3000).astype(np.uint8)
        wild[:70] = np.where(np.arange(70) % 2 == 0, N - 1, 255)  # (one wave with the highest key and, below 256 groups, bin 0)
        key = np.where(wild < N, wild.astype(np.int64) + 1, 0)
        assert np.array_equal(device_order(lib, hip, wild, N), np.argsort(key, kind="stable"))
    finally:
        hip.free()


# ---------------------------------------------------------------------------------------------------------------------------
# 3. the k-mer sketch: a table per read group
# ---------------------------------------------------------------------------------------------------------------------------
SKETCH_E = 0.0271


@pytest.mark.parametrize("N", [65, 256])
def test_sketch_tables_of_every_read_group(N):
    """One (k, q) pair, k = 32 and q = 17, sprinkled(N) with its qualities raised (lane_limit.high_quality: a read gives about a
    hundred 32-mers): every word of every read group's exported table against the oracle's.

    The error rate is 0.0271, not the default 0.01: a table of the default size has 4 227 073 words, 8.7 GB for 256 read groups on
    either side.  The table sizes are steps in e (powers of two); the oracle alone (process and dump of 256 tables, no finalize,
    whose F0 / f1 scans take 14 s and more on nearly empty tables at any size) took 0.5 s at 0.0766 (8192 counters a level), 1.5 s at
    0.0541, 1.9 s at 0.0383, 2.7 s at 0.0271 (65 536 counters a level, 528 385 words a table) and 6.7 s at 0.0192: 0.0271 is the
    smallest step above the default at which it finishes within a few seconds."""
    opts = dict(n_refs=2, n_lanes=N, klist=[32], qlist=[17], e=SKETCH_E, **CORE)
    cols = ll.high_quality(ll.sprinkled(N))
    o = Oracle(**opts)
    a = Aggregator(**opts)
    for i, r in enumerate(ll.refs()):
        o.reference(i, r)
        a.set_reference(i, r)
    assert o.process(cols) == 0
    a.submit(cols)
    n = ss.sizes(SKETCH_E)[2]
    v = a.state_export_host()
    a.close()
    block = v[len(v) - N * n:]
    del v
    ss.assert_block(block, o, N, 1, SKETCH_E, "sprinkled(%d)" % N)
    sums = block.reshape(N, n)[:, 0]
    present = np.bincount(cols["lane"], minlength=N) > 0
    assert (sums[~present] == 0).all() and (sums[[63, 64, N - 1]] > 50).all() and (sums > 0).sum() >= 0.9 * N
    o.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 4. the nine modules at 256 read groups
# ---------------------------------------------------------------------------------------------------------------------------
N_LANES = 256
WORD_ORDER = ["rcv", "sac", "sbc", "ibc", "gcb", "adp", "mbc", "qbc"]  # the modules' words at the end of the state vector (bqc_api.cpp)
LM = [(l, m) for l in range(N_LANES) for m in range(2)]


@functools.lru_cache(maxsize=None)
def batches():
    return ll.module_batches()


@functools.lru_cache(maxsize=None)
def want(name):
    """The module's table by its restatement: computed once, never changed."""
    t = ll.module_table(name, batches(), N_LANES)
    for x in (t.values() if isinstance(t, dict) else [t]):
        if isinstance(x, np.ndarray):
            x.setflags(write=False)
    return t


def module_context(names):
    opts = {}
    for name in names:
        opts.update(ll.module_options(name))
    a = Aggregator(n_refs=2, n_lanes=N_LANES, **dict(CORE, **opts))
    a.set_reference(0, ll.loaded_refs()[0])
    return a


def views(a, name):
    """Everything the module's view call gives, for every read group, as a flat list of arrays."""
    if name == "qbc":
        return [a.qual_by_cycle(l, m) for l, m in LM]
    if name == "mbc":
        return [x for l, m in LM for x in a.mismatch_by_cycle(l, m)]
    if name == "adp":
        return [x for l, m in LM for x in a.adapter_by_cycle(l, m)[:2]]
    if name == "gcb":
        return [x for l in range(N_LANES) for x in a.gc_bias(l)]
    if name == "ibc":
        return [x for l, m in LM for x in a.indel_by_cycle(l, m)]
    if name == "sbc":
        return [x for l, m in LM for x in a.substitutions(l, m)]
    if name == "sac":
        return [a.site_alleles(l) for l in range(N_LANES)]
    if name == "rcv":
        out = []
        for l in range(N_LANES):
            v = a.region_coverage(l)
            out += [np.array([v[k] for k in ("reads_examined", "reads_on_target", "aligned_bases", "bases_on_target", "target_bases")], np.uint64), v["regions"], v["hist"]]
        return out
    v = a.duplicate_sets()
    return [v["lanes"], v["sets"], v["largest"], v["hist"], np.array([v["estimated_library_size"], v["capacity"]], np.uint64)]


def want_views(name, counts):
    """The same list from the restatement's table (the cycle counts of `.qbc` and `.mbc` are the mates' n_cycles of the core counts)."""
    T = want(name)
    N = ll.CYCLES
    cyc = lambda l, m: int(counts[l]["r%d.n_cycles" % (m + 1)])
    if name == "qbc":
        out = []
        for l, m in LM:
            nc, nq = qbc_ref.sizes(T[l, m], cyc(l, m))
            out.append(T[l, m, :nc, :nq] if nc and nq else np.zeros((nc, nq), np.uint64))
        return out
    if name == "mbc":
        out = []
        for l, m in LM:
            nc, nq = mbc_ref.sizes(T[l, m], cyc(l, m))
            out += [T[l, m, k, :nc, :nq] if nc and nq else np.zeros((nc, nq), np.uint64) for k in range(2)]
        return out
    if name == "adp":
        out = []
        for l, m in LM:
            nc = adp_ref.sizes(T[l, m])
            out += [T[l, m, adp_ref.E_ROW, :nc], T[l, m, :len(adp_ref.BUILTIN), :nc]]
        return out
    if name == "gcb":
        G = ll.module_genome()
        return [x for l in range(N_LANES) for x in (G, T[l, 0], T[l, 1], T[l, 2])]
    if name == "ibc":
        return [x for l, m in LM for x in ibc_ref.views(T, l, m)]
    if name == "sbc":
        return [x for l, m in LM for x in sbc_ref.views(T[l, m], N)]
    if name == "sac":
        return [T[l].reshape(-1, 2, 4) for l in range(N_LANES)]
    if name == "rcv":
        out = []
        for p in rcv_ref.products_fast(T, ll.regions(), 2):
            out += [np.array([p[k] for k in ("reads_examined", "reads_on_target", "aligned_bases", "bases_on_target", "target_bases")], np.uint64), p["regions"], p["hist"]]
        return out
    return [T["lanes"], T["sets"], T["largest"], T["hist"], np.array([T["estimated_library_size"], T["capacity"]], np.uint64)]


def words_of(vec, names):
    """{name: the module's words} of a state vector of a context with the modules `names` on: they are its tail, in WORD_ORDER."""
    out, end = {}, len(vec)
    for name in reversed([n for n in WORD_ORDER if n in names]):
        shape = want(name).shape
        size = int(np.prod(shape))
        out[name] = vec[end - size:end].reshape(shape)
        end -= size
    return out, end


def run_modules(names):
    """The batches through a context with the modules `names` -> ({name: words}, {name: views}, counts, the SHA-256 of the words in
    front of the modules': the core state of 256 read groups is too large to keep nine copies of)"""
    a = module_context(names)
    for b in batches():
        a.submit(b)
    counts = a.finalize()
    vec = a.state_export_host()
    words, end = words_of(vec, names)
    words = {k: v.copy() for k, v in words.items()}
    got = {name: views(a, name) for name in names}
    a.close()
    return words, got, counts, hashlib.sha256(vec[:end].tobytes()).hexdigest()


@functools.lru_cache(maxsize=None)
def alone(name):
    return run_modules((name,))


def same_lists(got, exp, what):
    assert len(got) == len(exp), what
    for k, (g, w) in enumerate(zip(got, exp)):
        g, w = np.asarray(g), np.asarray(w)
        assert g.shape == w.shape and np.array_equal(g.astype(np.uint64), w.astype(np.uint64)), "%s: item %d of %d differs (256 read groups, in view order)" % (what, k, len(got))


def check_words(name, got):
    T = want(name)
    bad = np.argwhere(got != T)
    assert not len(bad), "%s: %d words differ, first (read group, ...) = %s: %d != %d" % (name, len(bad), bad[0].tolist(), got[tuple(bad[0])], T[tuple(bad[0])])


@pytest.mark.parametrize("name", ll.MODULES)
def test_module_alone(name):
    """sprinkled(256), solo(256, 200) and one_each(256): the whole table of every read group against the module's restatement, as words
    of the state vector and through the view call"""
    words, got, counts, _ = alone(name)
    if name != "dup":
        check_words(name, words[name])
    same_lists(got[name], want_views(name, counts), name)
    if name == "rcv":  # E, T and A of the read groups on both sides of rc_eta's LDS copy (RC_ETA_LANES = 64), by name
        S = want("rcv")
        for g in (63, 64):
            assert S[g, 0] > 0 and S[g, 2] > 0
            assert words["rcv"][g, :3].tolist() == S[g, :3].tolist(), "read group %d: E, T, A = %s, expected %s" % (g, words["rcv"][g, :3].tolist(), S[g, :3].tolist())
    if name == "dup":
        assert got["dup"][0].shape == (256, 5) and np.array_equal(got["dup"][0], want("dup")["lanes"])
        assert dup_ref.same_view(alone_dup_view(got["dup"]), want("dup")) is None


def alone_dup_view(items):
    lanes, sets, largest, hist, tail = items
    return dict(lanes=lanes, sets=sets, largest=largest, hist=hist, estimated_library_size=int(tail[0]), capacity=int(tail[1]))


def test_untouched_read_groups_stay_zero():
    """sprinkled(256) alone leaves a few read groups without a read: their rows are zero in every module's words (all nine on)"""
    cols = ll.sprinkled(256)
    absent = np.flatnonzero(np.bincount(cols["lane"], minlength=256) == 0)
    assert len(absent) >= 1
    a = module_context(ll.MODULES)
    a.submit(cols)
    vec = a.state_export_host()
    a.finalize()
    words, _ = words_of(vec, ll.MODULES)
    for name in WORD_ORDER:
        T = ll.module_table(name, [cols], N_LANES)
        assert not T[absent].any()
        assert not words[name][absent].any(), name
        bad = np.argwhere(words[name] != T)
        assert not len(bad), (name, len(bad), bad[0].tolist())
    assert not a.duplicate_sets()["lanes"][absent].any()
    assert np.array_equal(a.duplicate_sets()["lanes"], ll.module_table("dup", [cols], N_LANES)["lanes"])
    a.close()


def test_all_nine_modules_at_once():
    """all nine on: every table equals what the module gave alone (and the restatement), and the words in front of the modules' are
    those of a context with one module"""
    words, got, counts, front = run_modules(tuple(ll.MODULES))
    for name in ll.MODULES:
        w1, g1, c1, f1 = alone(name)
        if name != "dup":
            check_words(name, words[name])
            assert np.array_equal(words[name], w1[name]), name
        same_lists(got[name], g1[name], name + ", alone and with the others")
        same_lists(got[name], want_views(name, counts), name)
        assert front == f1, name
        assert not _abi.diff_counts(c1, counts)


# ---------------------------------------------------------------------------------------------------------------------------
# 5. the writers: 256 lane blocks in a permuted caller order
# ---------------------------------------------------------------------------------------------------------------------------
def test_writers_with_256_lanes_in_a_permuted_order(tmp_path):
    names = ["rg%03d" % k for k in range(256)]
    idx = np.random.default_rng(5).permutation(256)
    assert idx[0] != 0 and sorted(idx.tolist()) == list(range(256))
    a = module_context(("qbc", "rcv", "dup"))
    for b in batches():
        a.submit(b)
    counts = a.finalize()
    out = {k: str(tmp_path / ("out." + k)) for k in ("qbc", "rcv", "dup")}
    a.write_qual_by_cycle(out["qbc"], "S1", names, idx)
    a.write_region_coverage(out["rcv"], ["chr1", "chr2"], "S1", names, idx)
    a.write_duplicate_sets(out["dup"], "S1", names, idx)
    a.close()
    cycles = np.array([[int(counts[l]["r1.n_cycles"]), int(counts[l]["r2.n_cycles"])] for l in range(256)], np.int64)
    assert open(out["qbc"]).read() == qbc_ref.text(want("qbc"), cycles, "S1", names, idx.tolist())
    prod = rcv_ref.products_fast(want("rcv"), ll.regions(), 2)
    assert open(out["rcv"]).read() == rcv_ref.text(prod, ll.regions(), ["chr1", "chr2"], 20, rcv_ref.DEFAULT_THRESHOLDS, "S1", names, idx.tolist())
    assert open(out["dup"]).read() == dup_ref.text(want("dup"), "S1", names, idx.tolist())
