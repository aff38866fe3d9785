"""The batches of the read-group-limit tests (tests/test_gpu_lane_limit.py, tests/test_gpu_lane_limit_program.py;
tests/test_lane_limit_cpu.py asserts that each of them crosses the edge it is named for).  No GPU use.

bqc_create takes 1 to 256 read groups: the lane column is a byte.  Everything on the card is indexed by read group, and several
pieces change their path with the group's number or with the count: rc_eta (k_rcv.hip) keeps groups below 64 in LDS and sends the
others to device memory; lane_bits / t8_lanes (bqc_pipeline.cpp) are four 64-bit words; stable_slot (k_anchor.hip) takes
bits_for(n_lanes - 1) ballots for the anchors' scatter and bits_for(n_lanes) for the processing order, whose keys are lane + 1; the
per-cycle kernels make one round per read group of a step.  The layouts below put reads on both sides of every multiple of 64, at
group counts on both sides of every power of two.

One pool of reads (tests/synth.py: 150 bp on two contigs in coordinate order, with a few reads of 300 bp among them so that k_long and
the slow chunks meet high read groups too) is made once per process; a layout is a slice of it with its own lane column, so a
stream of layouts is in coordinate order throughout, and positions run forward within every read group."""
import functools

import numpy as np

from tests import synth

COUNTS = [64, 65, 128, 129, 255, 256]      # group counts on both sides of 2^6, 2^7 and 2^8 (bits_for(N - 1) / bits_for(N))
SOLO_GROUPS = [63, 64, 127, 128, 191, 192, 255]
EDGE_GROUPS = [0, 63, 64, 127, 128, 191, 192, 254, 255]
REF_LEN = 200_000
POOL_SHORT, POOL_LONG = 6000, 72
STEP = 1024                               # reads of a workgroup of k_an_count / k_lo_count, and of a step of the module kernels at the most
SOLO_READS, ENDS_READS = 531, 777
MQ_ALL = 30                               # the highest mapping-quality threshold among the modules' defaults (substitutions)


def bits_for(v):
    """k_anchor.hip bits_for: the bits of the largest key (32 - clz; 0 for 0)."""
    return int(v).bit_length()


def take(cols, idx):
    """The reads `idx` of a column dict in that order (the packed columns gathered)."""
    idx = np.asarray(idx, np.int64)
    L = cols["l_seq"].astype(np.int64)
    nc = cols["n_cigar"].astype(np.int64)

    def gather(v, size):
        first = (np.cumsum(size) - size)[idx]
        n = size[idx]
        at = np.repeat(first - (np.cumsum(n) - n), n) + np.arange(int(n.sum()), dtype=np.int64)
        return v[at]

    out = {}
    for k, v in cols.items():
        if k == "seq":
            out[k] = gather(v, (L + 1) // 2)
        elif k == "qual":
            out[k] = gather(v, L)
        elif k == "cigar":
            out[k] = gather(v, nc)
        else:
            out[k] = v[idx]
    return out


@functools.lru_cache(maxsize=None)
def pool():
    """(cols, refs): POOL_SHORT reads of 150 bp and POOL_LONG of 300 bp on two contigs, merged in coordinate order; one read in five
    carries an insertion or a deletion.  Never changed: a layout copies what it assigns."""
    short, refs = synth.synth(seed=71, n_reads=POOL_SHORT, L=150, n_refs=2, ref_len=REF_LEN, p_indel=0.2)
    long_, _ = synth.synth(seed=72, n_reads=POOL_LONG, L=300, refs=refs, p_indel=0.2)
    both = synth.concat([short, long_])
    order = np.lexsort((both["pos"], both["rid"]))  # (stable: rid, then pos)
    cols = take(both, order)
    for v in cols.values():
        v.setflags(write=False)
    return cols, refs


def clean(cols):
    """The reads that every module's rule examines when their contig is loaded: primary, mapped, neither duplicate nor failed, a mate
    flag, qualities, a CIGAR, mapq >= MQ_ALL."""
    f = cols["flag"].astype(np.int64)
    return ((f & 0xF04) == 0) & ((f & 0xC0) != 0) & ((f & 0x8000) == 0) & (cols["mapq"] >= MQ_ALL) & (cols["n_cigar"] > 0) & (cols["l_seq"] > 0) & (cols["rid"] >= 0)


def piece(at, n, lane):
    """Reads [at, at + n) of the pool with the lane column `lane`."""
    cols, _ = pool()
    assert at + n <= len(cols["flag"]), (at, n)
    out = synth.slice_batch(cols, at, at + n)
    out["lane"] = np.asarray(lane, np.uint8)
    assert len(out["lane"]) == n
    return out


def refs():
    return pool()[1]


def pin(cols, lane, groups):
    """Give the first clean reads of the slice to `groups`, one each (lane is changed in place)."""
    idx = np.flatnonzero(clean(cols))
    assert len(idx) >= len(groups)
    lane[idx[:len(groups)]] = groups


def edge_groups(N):
    return sorted({g for g in EDGE_GROUPS + [N - 1] if g < N})


def sprinkled_size(N):
    return 4 * N + 37


def sprinkled(N, at=0, seed=1):
    """4 N + 37 reads, the read group of each drawn uniformly over all N: every 1024 reads of the processing order hold many group
    seams.  Groups 63, 64 and N - 1 (and the other neighbours of a multiple of 64) get a clean read each for certain."""
    n = sprinkled_size(N)
    lane = np.random.default_rng(1000 * seed + N).integers(0, N, n)
    pin(synth.slice_batch(pool()[0], at, at + n), lane, edge_groups(N))
    return piece(at, n, lane)


def one_each(N, at=0, seed=2):
    """N reads, every read group exactly once, in a random order: a workgroup whose share is the whole batch makes one round per read
    group in its only step."""
    return piece(at, N, np.random.default_rng(1000 * seed + N).permutation(N))


def solo(N, g, at=0):
    """SOLO_READS reads of the one read group g: the batch has one read group, so the kernels take it in stream order."""
    assert 0 <= g < N
    return piece(at, SOLO_READS, np.full(SOLO_READS, g))


def ends(N, at=0, seed=3):
    """ENDS_READS reads of read groups 0 and N - 1 only."""
    return piece(at, ENDS_READS, np.where(np.random.default_rng(1000 * seed + N).random(ENDS_READS) < 0.5, 0, N - 1))


def runs_plan(N, seed=4):
    """[(group, run length)] of runs(N): five runs of 260 to 340 reads first, of N - 1, of 64 (63 when there is no 64) and three
    other groups; then runs of 1 to 9 reads of every other group that gets reads, in a random order, edge groups among them.  Of the
    groups that are no edge group every third one gets no read."""
    rng = np.random.default_rng(1000 * seed + N)
    edges = edge_groups(N)
    others = [g for g in range(N) if g not in edges]
    absent = set(others[::3])
    present = [g for g in range(N) if g not in absent]
    head = [N - 1, 64 if N > 64 else 63] + [int(g) for g in rng.choice([g for g in others if g not in absent], 3, replace=False)]
    plan = [(g, int(n)) for g, n in zip(head, (300, 260, 340, 281, 333))]
    rest = [g for g in present if g not in head]
    rest = [rest[i] for i in rng.permutation(len(rest))]
    plan += [(g, int(rng.integers(1, 10))) for g in rest]
    return plan


def runs_size(N):
    return sum(n for _, n in runs_plan(N))


def runs(N, at=0):
    """Read groups in runs of unequal length (runs_plan): the first 1024-read workgroups of k_an_count and k_lo_count hold a handful
    of groups, so most columns of their count tables are zero; a third of the groups has no read at all."""
    plan = runs_plan(N)
    return piece(at, sum(n for _, n in plan), np.concatenate([np.full(n, g) for g, n in plan]))


def stream_parts(N):
    """The layouts of stream(N) in order, one after the other in the pool: [(name, cols)]."""
    at, out = 0, []
    for name, make, n in (("sprinkled", lambda a: sprinkled(N, a), sprinkled_size(N)), ("solo", lambda a: solo(N, min(N - 1, 200), a), SOLO_READS),
                          ("ends", lambda a: ends(N, a), ENDS_READS), ("runs", lambda a: runs(N, a), runs_size(N)), ("one_each", lambda a: one_each(N, a), N)):
        out.append((name, make(at)))
        at += n
    return out


def stream_cuts(n):
    """Batches of 1, 1023, 1024 and 1025 reads where the stream has as many, and the rest in two at an odd place."""
    cuts = [c for c in (1, 1024, 2048, 3073) if c < n]
    rest = n - cuts[-1]
    if rest > 3:
        cuts.append(cuts[-1] + (rest // 2) | 1)
    return cuts


def stream(N):
    """sprinkled, solo (group min(N - 1, 200)), ends, runs and one_each of N groups, concatenated and cut again at stream_cuts: the
    seams of the batches lie inside the layouts, so a group's anchor state and its coverage carry must persist from batch to batch."""
    whole = synth.concat([c for _, c in stream_parts(N)])
    n = len(whole["flag"])
    edges = [0] + stream_cuts(n) + [n]
    return [synth.slice_batch(whole, edges[i], edges[i + 1]) for i in range(len(edges) - 1)]


def high_quality(cols, seed=6):
    """The batch with its qualities raised to 35 and more except for one base in fifty (the pool's qualities restart a 32-mer of
    q >= 17 every few bases: almost no k-mer reaches the sketch); a read without qualities keeps none."""
    q = cols["qual"]
    low = np.random.default_rng(seed).random(q.size) < 0.02
    return dict(cols, qual=np.where((q == 0xFF) | low, q, np.maximum(q, 35)).astype(np.uint8))


def lane_words(lane):
    """The four words of a bit per read group that occurs (m.lane_bits of bqc_pipeline.cpp)."""
    w = [0, 0, 0, 0]
    for g in np.unique(np.asarray(lane)).tolist():
        w[g >> 6] |= 1 << (g & 63)
    return w


# ---------------------------------------------------------------------------------------------------------------------------
# the modules' own lists over the pool's contigs
# ---------------------------------------------------------------------------------------------------------------------------
def sites():
    """A site every 53 bases of the first 125 000 of the first contig (where the module batches lie) and of the first 5 000 of the
    second: (rid, pos), sorted."""
    p0, p1 = np.arange(5, 125_000, 53, dtype=np.int32), np.arange(5, 5_000, 53, dtype=np.int32)
    return np.concatenate([np.zeros(len(p0), np.int32), np.ones(len(p1), np.int32)]), np.concatenate([p0, p1])


def regions():
    """Regions of 1 to 400 bases over the same stretches, some abutting: (rid, start, end), sorted and disjoint."""
    rng = np.random.default_rng(9)
    out = []
    for rid, top in ((0, 125_000), (1, 5_000)):
        at = 0
        while at < top:
            ln = int(rng.choice([1, 7, 64, 150, 400]))
            out.append((rid, at, at + ln))
            at += ln + int(rng.choice([0, 1, 90, 700, 3000]))
    return tuple(np.array([x[i] for x in out], np.int32) for i in range(3))


# ---------------------------------------------------------------------------------------------------------------------------
# the nine modules: one configuration, and their tables by the restatements of tests/*_ref.py
# ---------------------------------------------------------------------------------------------------------------------------
MODULES = ["qbc", "mbc", "adp", "gcb", "ibc", "sbc", "sac", "rcv", "dup"]
CYCLES = 40          # the cycle capacity of the per-cycle modules (256 read groups x 2 x 2 x CYCLES x 224 words for `.mbc`)
GC_WINDOW = 100
DUP_CAPACITY = 1 << 14


def module_options(name):
    """The options of Aggregator(...) that switch the module on."""
    return {"qbc": dict(qual_by_cycle=CYCLES), "mbc": dict(mismatch_by_cycle=CYCLES), "adp": dict(adapter_by_cycle=CYCLES), "gcb": dict(gc_bias=GC_WINDOW),
            "ibc": dict(indel_by_cycle=CYCLES), "sbc": dict(substitutions=CYCLES), "sac": dict(site_alleles=sites()), "rcv": dict(regions=regions()),
            "dup": dict(duplicate_sets=DUP_CAPACITY)}[name]


def loaded_refs():
    """The contigs a module context loads: the first one only (`.gcb`, `.mbc` and `.sbc` read it; a read on the other is not examined)."""
    return [refs()[0], None]


def module_table(name, batches, n_lanes):
    """What the module must hold after `batches`, by the module's own vectorised restatement: its words of the state vector with the
    read group as the first axis (`.gcb`: the rows R, B, Q without the genome's line; `.dup`: the whole view, `lanes` by read group)."""
    from tests import adp_ref, dup_ref, gcb_ref, ibc_ref, mbc_ref, qbc_ref, rcv_ref, sac_ref, sbc_ref
    whole = synth.concat(batches)
    if name == "qbc":
        return qbc_ref.table_fast(batches, n_lanes, CYCLES)
    if name == "mbc":
        return mbc_ref.table_fast(batches, loaded_refs(), n_lanes, CYCLES)
    if name == "adp":
        return adp_ref.table_fast(batches, n_lanes, CYCLES)
    if name == "gcb":
        return gcb_ref.table_fast(batches, loaded_refs(), n_lanes, GC_WINDOW)[1]
    if name == "ibc":
        return ibc_ref.table_fast(whole, n_lanes, CYCLES)
    if name == "sbc":
        return sbc_ref.table_fast(batches, loaded_refs(), n_lanes, CYCLES)[0]
    if name == "sac":
        return sac_ref.table_fast(whole, sites(), n_lanes, 2)
    if name == "rcv":
        return rcv_ref.state_fast(whole, regions(), n_lanes, 2)
    if name == "dup":
        return dup_ref.view_fast(whole, n_lanes, 2, DUP_CAPACITY)
    raise ValueError(name)


@functools.lru_cache(maxsize=None)
def module_genome():
    """The genome's line of `.gcb`: the windows of the loaded contig by GC bin."""
    from tests import gcb_ref
    return gcb_ref.table_fast([], loaded_refs(), 1, GC_WINDOW)[0]


def group_rows(name, table):
    """Per read group whether the module's table holds anything of it (the `examined` rule of the restatement took a read of it)."""
    t = table["lanes"] if name == "dup" else table
    return t.reshape(t.shape[0], -1).any(axis=1)


def module_batches():
    """The batches of the module tests at 256 read groups: sprinkled, solo of group 200, and every group once."""
    return [sprinkled(256, 0), solo(256, 200, sprinkled_size(256)), one_each(256, sprinkled_size(256) + SOLO_READS)]
