"""GPU: the coverage launches of a batch (k_cov or the started read groups, then the host's words) beside the chunk plan, on a stream
of their own between a fork behind k_prep_reads and a join in front of the batch's last launch (bqc_pipeline.cpp, enqueue_kernels) —
and on the compute stream with BQC_COV_STREAM=0 (read when the context is created).  Every case runs both ways against the oracle:
the state read right behind bqc_process without a sync, batches with and without coverage tiles in turn, windows carried across every
batch end with three read groups, the sketch beside it, and a failing batch behind two good ones."""
import numpy as np
import pytest

from bamqc_amd import Aggregator, BamQCError, _abi
from tests import synth
from tests.parity import assert_parity, run_gpu, run_oracle, split

pytestmark = pytest.mark.gpu

ERR_AS_TAG, ERR_STATE = 4, 8


@pytest.fixture(params=["1", "0"], ids=["cov-stream", "compute-stream"])
def switch(request, monkeypatch):
    monkeypatch.setenv("BQC_COV_STREAM", request.param)
    return request.param


def _same(co, cg):
    d = _abi.diff_counts(co, cg)
    assert not d, "\n".join(d[:10])


def _ctx(refs, **opts):
    a = Aggregator(n_refs=len(refs), **opts)
    for i, r in enumerate(refs):
        a.set_reference(i, r)
    return a


def test_state_is_read_right_behind_process_without_a_sync(switch):
    cols, refs = synth.synth(seed=901, n_reads=9000, n_refs=2, ref_len=120_000, n_lanes=2, p_indel=0.1, density=30)
    rc, co, _ = run_oracle([cols], refs, n_refs=2, n_lanes=2)
    assert rc == 0
    a = _ctx(refs, n_lanes=2)
    db = a.upload(cols)
    a.process(db)
    _same(co, a.finalize())  # finalize at once
    a.reset()
    a.process(db)
    st = a.state_export_host()  # the state vector at once
    a.sync()
    assert np.array_equal(st, a.state_export_host())
    _same(co, a.finalize())
    db.free()
    a.close()


def test_batches_without_and_with_coverage_tiles_in_turn(switch):
    refs = synth.make_reference(np.random.default_rng(902), 1, 150_000)
    unmapped = [synth.synth(seed=903 + k, n_reads=3000, refs=refs, n_lanes=2, p_unmapped=1.0)[0] for k in range(2)]
    mapped, _ = synth.synth(seed=905, n_reads=6000, refs=refs, n_lanes=2, density=25)
    for u in unmapped:
        assert (u["flag"] & 0x4).all()
    co, cg, _, a = assert_parity([unmapped[0], mapped, unmapped[1]], refs, n_refs=1, n_lanes=2)
    assert cg is not None and int(sum(int(c["poscov"].sum()) for c in cg)) > 0
    a.close()


def test_windows_carried_across_every_batch_end_with_three_read_groups(switch):
    # deep, position-sorted reads cut in the middle of their windows: every batch starts inside the two live windows of the one before
    cols, refs = synth.synth(seed=906, n_reads=12_000, n_refs=1, ref_len=200_000, n_lanes=3, p_indel=0.1, density=40)
    co, cg, _, a = assert_parity(split(cols, [3000, 6001, 9100]), refs, n_refs=1, n_lanes=3)
    assert cg is not None
    a.close()


def test_with_the_sketch(switch):
    cols, refs = synth.synth(seed=907, n_reads=6000, n_refs=2, ref_len=100_000, n_lanes=2, density=20)
    co, cg, _, a = assert_parity(split(cols, [2500]), refs, n_refs=2, n_lanes=2, klist=[17], qlist=[17])
    assert cg is not None
    a.close()


def test_a_failing_batch_behind_two_good_ones(switch):
    cols, refs = synth.synth(seed=908, n_reads=9000, n_refs=1, ref_len=150_000, n_lanes=2, density=25)
    good1, good2, bad = split(cols, [3000, 6000])
    bad = dict(bad)
    bad["as_"] = bad["as_"].copy()
    eligible = np.nonzero(((bad["flag"] & 0x3) == 0x3) & ((bad["flag"] & 0xF0C) == 0) & (bad["mapq"] >= 60))[0]
    assert len(eligible)
    bad["as_"][eligible[len(eligible) // 2]] = synth.BQC_AS_ABSENT  # a read with no usable AS tag
    rc_o, _, _ = run_oracle([good1, good2, bad], refs, n_refs=1, n_lanes=2)
    assert rc_o == ERR_AS_TAG
    rc_g, cg, a = run_gpu([good1, good2, bad], refs, n_refs=1, n_lanes=2)
    assert rc_g == rc_o and cg is None
    with pytest.raises(BamQCError) as e:  # the context is poisoned as before
        a.submit(good1)
    assert e.value.code == ERR_STATE
    a.close()
    assert not a.h
