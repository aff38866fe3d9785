"""GPU: the optional modules' segments of the flat state vector through all four exchange calls (bqc_state_export / _import, the path
RCCL runs use, and their _host variants), bqc_reset and the refusals of the bqc_enable_* calls, on one context with the sketch and
every module on at its smallest sensible size.

Each module's own test pins its words, its views and the host exchange; the "every module on" checks of test_gpu_window_depth.py and
test_gpu_region_coverage.py pin the first two segments' places.  Here the nine segments are looked at together: the device path
against the host path word for word, every segment non-zero and in the vector's order (bamqc_amd/csrc/bqc_ctx.h: Seg)."""
import functools

import numpy as np
import pytest

from bamqc_amd import Aggregator, BamQCError
from tests import lane_limit, synth
from tests.hipmem import Hip
from tests.parity import split

pytestmark = pytest.mark.gpu

ERR_STATE = 8
N_LANES, N_READS = 4, 400
LENS = [lane_limit.REF_LEN] * 2
BASE = dict(n_lanes=N_LANES, n_refs=2, main_chrom=[1, 1], max_read_len=1024, isize=2000)
SKETCH = dict(klist=[32], qlist=[17])
ORDER = ["wdp", "rcv", "sac", "sbc", "ibc", "gcb", "adp", "mbc", "qcyc"]  # the segments behind the core's and the sketch's words


@functools.lru_cache(maxsize=None)
def setup():
    """(cols, modules): the first N_READS reads of the pool of tests/lane_limit.py (150 and 300 bp on the first contig, one in five with
    an insertion or a deletion, 0.5 % substitutions) dealt to four read groups, and behind them one read that begins with an adapter;
    the options of the ten modules, the sites and regions under a read that every module's rule examines."""
    cols = lane_limit.piece(0, N_READS, np.arange(N_READS) % N_LANES)
    plain = np.flatnonzero(lane_limit.clean(cols) & (cols["n_cigar"] == 1) & (cols["l_seq"] == 150))
    at = int(cols["pos"][plain[len(plain) // 2]])  # (one M of 150 bases from here)
    seq = "ACG" + "AGATCGGAAGAG" + "ACGT" * 9  # Illumina_Universal at cycle 3
    tail = synth.single_read(seq, [37] * len(seq), [(len(seq), "M")], 0x1 | 0x40 | 0x1000, pos=int(cols["pos"][-1]) + 1, lane=0)
    cols = synth.concat([cols, tail])
    sites = (np.zeros(5, np.int32), np.arange(at + 20, at + 25, dtype=np.int32))
    regions = tuple(np.array(x, np.int32) for x in ([0, 0], [at, at + 120], [at + 100, at + 220]))
    modules = dict(wdp=dict(window_depth=(100, LENS)), rcv=dict(regions=regions), sac=dict(site_alleles=sites), sbc=dict(substitutions=16),
                   ibc=dict(indel_by_cycle=16), gcb=dict(gc_bias=100), adp=dict(adapter_by_cycle=8), mbc=dict(mismatch_by_cycle=8),
                   qcyc=dict(qual_by_cycle=8), dup=dict(duplicate_sets=1 << 12))
    return cols, modules


def context(*names, sketch=True):
    """A context with the modules `names` on ("every": all ten) and both contigs loaded."""
    modules = setup()[1]
    opts = dict(BASE, **(SKETCH if sketch else {}))
    for nm in (list(modules) if names == ("every",) else names):
        opts.update(modules[nm])
    a = Aggregator(**opts)
    for i, r in enumerate(lane_limit.refs()):
        a.set_reference(i, r)
    return a


@pytest.fixture(scope="module")
def one():
    """The batch through one context with everything on: the context (exported, so it takes no further batch), its vector by the host
    path (never changed) and by the device path (a buffer of the runtime the library is linked against), and where the segments lie."""
    cols = setup()[0]
    hip = Hip()
    a = context("every")
    a.submit(cols)
    vec = a.state_export_host()
    vec.setflags(write=False)
    buf = hip.alloc(a.state_words * 8)
    a.state_export_device(buf.value)
    off = context()
    bounds = [off.state_words]
    off.close()
    for nm in ORDER:  # a segment's size: what the module alone adds to the vector
        x = context(nm)
        bounds.append(bounds[-1] + x.state_words - bounds[0])
        x.close()
    assert bounds[-1] == a.state_words == len(vec)
    yield dict(a=a, vec=vec, hip=hip, buf=buf, bounds=bounds, cols=cols)
    a.close()
    hip.free()


def segments(vec, bounds):
    return {nm: vec[bounds[k]:bounds[k + 1]] for k, nm in enumerate(ORDER)}


def check_words(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.flatnonzero(got != want)
    assert not len(bad), "%s: %d words differ, first at %d: %d != %d" % (what, len(bad), bad[0], got[bad[0]], want[bad[0]])


def same(a, b):
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(same(a[k], b[k]) for k in a)
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray):
        return a.shape == b.shape and np.array_equal(a, b)
    return a == b


def views(a):
    """Every module's view but the duplicate sets', through the accessors (which finalise first)."""
    lm = [(l, m) for l in range(N_LANES) for m in range(2)]
    return dict(qcyc=[a.qual_by_cycle(l, m) for l, m in lm], mbc=[a.mismatch_by_cycle(l, m) for l, m in lm], adp=[a.adapter_by_cycle(l, m) for l, m in lm],
                ibc=[a.indel_by_cycle(l, m) for l, m in lm], sbc=[a.substitutions(l, m) for l, m in lm], gcb=[a.gc_bias(l) for l in range(N_LANES)],
                sac=[a.site_alleles(l) for l in range(N_LANES)], rcv=[a.region_coverage(l) for l in range(N_LANES)],
                wdp=[a.window_depth(l) for l in range(N_LANES)])


def test_device_path_equals_host_path(one):
    got = one["hip"].get(one["buf"], len(one["vec"]) * 8, np.uint64)
    check_words(got, one["vec"], "device export against host export")
    for nm, seg in segments(one["vec"], one["bounds"]).items():
        assert seg.any(), "the batch leaves the segment of %s empty" % nm


def test_segments_in_order(one):
    """Segment k of the vector holds what the module alone counts of the same batch: the nine lie in ORDER."""
    segs = segments(one["vec"], one["bounds"])
    for nm in ORDER:
        x = context(nm, sketch=False)
        x.submit(one["cols"])
        alone = x.state_export_host()
        x.close()
        check_words(alone[len(alone) - len(segs[nm]):], segs[nm], nm)


def test_import_through_the_device(one):
    a, m = one["a"], context("every")
    m.state_import_device(one["buf"].value)
    check_words(m.state_export_host(), one["vec"], "device import, then host export")
    va, vm = views(a), views(m)
    for nm in va:
        assert same(va[nm], vm[nm]), nm
    # what the batch was chosen for, where a non-zero segment does not say it already
    assert sum(int(f.sum()) for e, f, names in va["adp"]) >= 1, "no adapter hit"
    assert sum(int(i.sum()) for e, i, d, il, dl in va["ibc"]) and sum(int(d.sum()) for e, i, d, il, dl in va["ibc"]), "no insertion or no deletion"
    assert sum(int(mm.sum()) for al, mm in va["mbc"]), "no mismatch"
    assert sum(int(c.sum()) for c in va["sac"]) and sum(r["bases_on_target"] for r in va["rcv"]), "no read over a site or a region"
    da, dm = a.duplicate_sets(), m.duplicate_sets()  # no part of the vector: the importer's table is empty
    assert da["lanes"][:, :2].sum() > 0 and da["sets"].sum() > 0
    assert not dm["sets"].any() and not dm["lanes"].any() and not dm["hist"].any() and dm["estimated_library_size"] == 0
    m.close()


def test_sum_of_two(one):
    first = one["bounds"][0]
    halves = []
    for part in split(one["cols"], [len(one["cols"]["flag"]) // 2]):
        x = context("every")
        x.submit(part)
        halves.append(x.state_export_host())
        x.close()
    total = halves[0] + halves[1]  # (the sketch's words do not add up this way: they are not looked at)
    h = context("every")
    h.state_import_host(total)
    check_words(h.state_export_host()[first:], one["vec"][first:], "sum of two through the host")
    h.close()
    d = context("every")
    buf = one["hip"].put(total)
    d.state_import_device(buf.value)
    check_words(d.state_export_host()[first:], one["vec"][first:], "sum of two through the device")
    d.close()


def test_reset(one):
    first = one["bounds"][0]
    a = context("every")
    a.submit(one["cols"])
    words = a.state_words
    check_words(a.state_export_host(), one["vec"], "before the reset")
    a.reset()
    assert a.state_words == words
    assert not a.state_export_host()[first:].any()
    a.reset()  # (an exported context takes no batch)
    a.submit(one["cols"])
    check_words(a.state_export_host(), one["vec"], "the batch again after the reset")
    a.close()


def test_enabling_fails_cleanly(one):
    modules = setup()[1]
    calls = [("enable_gc_bias", (100,)), ("enable_indel_by_cycle", (16,)), ("enable_substitutions", (16,)), ("enable_site_alleles", modules["sac"]["site_alleles"]),
             ("enable_region_coverage", modules["rcv"]["regions"]), ("enable_duplicate_sets", (1 << 12,)), ("enable_window_depth", (100, LENS))]
    on = context("every")
    off = context(sketch=False)
    off.submit(one["cols"])
    for a, words in ((on, "on already"), (off, "has taken a batch")):
        before = a.state_words
        for name, args in calls:
            with pytest.raises(BamQCError) as e:
                getattr(a, name)(*args)
            assert e.value.code == ERR_STATE and words in str(e.value), (name, str(e.value))
            assert a.state_words == before, name
    assert on.state_words == len(one["vec"])
    on.close()
    off.close()
