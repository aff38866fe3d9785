"""GPU parity at the edges of the device pre-pass (k_prep.hip): batch sizes around blocks of 1024 reads and super-windows of
4096, the forward-only FASTA check across blocks and batches, segment runs padded at stretch boundaries, replays of one resident
batch and batches in flight."""
import numpy as np
import pytest

from tests import synth
from tests.parity import assert_parity, run_oracle, split

pytestmark = pytest.mark.gpu

P, PR, FIRST = 0x1, 0x2, 0x40


@pytest.mark.parametrize("n", [1, 1023, 1024, 1025, 4095, 4097])
def test_batch_sizes_at_block_and_super_window_edges(n):
    cols, refs = synth.synth(seed=600 + n, n_reads=n, n_refs=2, ref_len=200_000)
    assert_parity(cols, refs, n_refs=2)


def test_batch_of_a_million_reads_and_three():
    from bamqc_amd import synth as csynth
    lens = [3_000_000, 2_000_000]
    refs = [csynth.reference(601, i, n) for i, n in enumerate(lens)]
    cols = csynth.batch(601, (1 << 20) + 3, lens, refs, n_lanes=2)
    assert_parity(cols, refs, n_refs=2, n_lanes=2)


def _eligible(rid, pos):
    return synth.single_read("ACGT" * 5, [30] * 20, [(20, "M")], P | PR | FIRST, pos=pos, rid=rid, mapq=60, as_=60)


def _fasta_violation_at(n, bad):
    # n eligible reads on contig 1, except read `bad`, which goes back to contig 0 (the FASTA scan only moves forward)
    ref = np.zeros(1000, np.uint8)
    reads = [_eligible(0 if i == bad else 1, 10 + (i % 900)) for i in range(n)]
    return synth.concat(reads), [ref, ref]


@pytest.mark.parametrize("n,bad", [(5 * 1024 + 17, 4 * 1024), (3 * 1024 + 5, 3 * 1024 + 4), (2048, 2047)])
def test_fasta_order_violation_across_blocks(n, bad):
    cols, refs = _fasta_violation_at(n, bad)
    co, cg, o, a = assert_parity(cols, refs, n_refs=2)
    assert cg is None  # the batch fails


def test_fasta_order_violation_against_an_earlier_batch():
    cols, refs = _fasta_violation_at(3000, 10 ** 9)
    first, second = split(cols, [2500])
    second = synth.concat([synth.slice_batch(second, 0, 200), _eligible(0, 5), synth.slice_batch(second, 200, 500)])
    co, cg, o, a = assert_parity([first, second], refs, n_refs=2)
    assert cg is None


def test_read_groups_with_segment_runs_padded_at_stretch_boundaries():
    # multi-operation CIGARs in every read group: each stretch ends on a partial group of segment entries
    cols, refs = synth.synth(seed=602, n_reads=30_011, n_refs=2, ref_len=300_000, n_lanes=5, long_cigar=True, p_indel=0.3)
    assert_parity(cols, refs, n_refs=2, n_lanes=5)


def test_resident_batch_thirty_times():
    # every replay reruns the pre-pass over scratch that holds the previous launch's values: after a reset, each of the 30
    # passes must leave exactly the state of the first, and that state is the oracle's
    from bamqc_amd import Aggregator, _abi
    cols, refs = synth.synth(seed=603, n_reads=9000, n_refs=1, ref_len=150_000, n_lanes=2, p_indel=0.1)
    rc, co, _ = run_oracle([cols], refs, n_refs=1, n_lanes=2)
    assert rc == 0
    a = Aggregator(n_refs=1, n_lanes=2)
    a.set_reference(0, refs[0])
    db = a.upload(cols)
    first = None
    for k in range(30):
        a.reset()
        a.process(db)
        st = a.state_export_host()
        if first is None:
            first = st.copy()
        assert np.array_equal(st, first), "pass %d differs from the first" % k
    cg = a.finalize()
    db.free()
    d = _abi.diff_counts(co, cg)
    assert not d, "\n".join(d[:10])


def test_three_batches_in_flight():
    cols, refs = synth.synth(seed=604, n_reads=12_000, n_refs=2, ref_len=200_000, n_lanes=3, p_indel=0.1)
    assert_parity(split(cols, [1025, 5121, 9000]), refs, n_refs=2, n_lanes=3)
