"""GPU parity of k_short's two instantiations (k_short.hip): the one with the BQC_SHORT_PARTS mask fixed at 15, which every real run
launches, and the one that reads the mask at run time (ablations, BQC_SHORT_XCD).  Every batch is compared count for count with the
oracle twice — in this process (fixed mask) and in a child with BQC_SHORT_XCD=1 (run-time mask, every part on; the variable is read
once per process) — and the two GPU results with each other.  The shapes sit where the group loop changes its path: an even and an odd
group count per tile, the counter spill at the 15th group inside a tile, last lanes of a read with some, one or no counted 8-mer window
(a lane without one issues no 8-mer atomics), reads shorter than one 8-mer, a tile that is not full."""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

from bamqc_amd import _abi
from tests import synth
from tests.parity import run_gpu, run_oracle

pytestmark = pytest.mark.gpu

P, PR, REV, FIRST, LAST = 0x1, 0x2, 0x10, 0x40, 0x80
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS4 = [P | PR | FIRST, P | PR | LAST, P | PR | FIRST | REV, P | PR | LAST | REV]  # both mates, both strands
REF_LEN = 40_000


def _batch(seed, lengths, n_reads=2000, n_lanes=2):
    """Reads of the given lengths in turn on one 40 kb reference: mates and strands cycle per read, read groups alternate, 1 % mismatches,
    0.5 % N, and every third read (long enough for it) has a D / I / N CIGAR, so that the chunks carry triplet-segment tiles."""
    rng = np.random.default_rng(seed)
    ref = rng.integers(0, 4, size=REF_LEN).astype(np.uint8)
    recs = []
    for i in range(n_reads):
        L = int(lengths[i % len(lengths)])
        pos = int(rng.integers(0, REF_LEN - 300))
        codes = ref[pos:pos + L].astype(np.int64)
        m = rng.random(L) < 0.01
        codes[m] = (codes[m] + rng.integers(1, 4, int(m.sum()))) % 4
        codes[rng.random(L) < 0.005] = 4
        ops = [(L, "M")]
        if i % 3 == 0 and L >= 40:
            a = int(rng.integers(5, L - 20))
            kind = (i // 3) % 3
            if kind == 0: ops = [(a, "M"), (2, "D"), (L - a, "M")]
            elif kind == 1: ops = [(a, "M"), (1, "I"), (L - a - 1, "M")]
            else: ops = [(a // 2, "M"), (3, "N"), (a - a // 2, "M"), (2, "I"), (L - a - 2, "M")]
        seq = "".join("ACGTN"[int(c)] for c in codes)
        recs.append(synth.single_read(seq, rng.integers(15, 41, size=L).tolist(), ops, FLAGS4[(i // 2) % 4], pos=pos, mapq=60, as_=90,
                                      nm=sum(n for n, c in ops if c in "ID"), lane=i % n_lanes))
    return synth.concat(recs), [ref], dict(n_refs=1, n_lanes=n_lanes, max_read_len=512)


BATCHES = {
    # fast_w = 16, 4 reads per wave, tiles of 16 groups: the counter spill of the 15th group happens inside the group loop; even count
    "len_241_255": lambda: _batch(1001, list(range(241, 256))),
    # fast_w = 10: last lane with 15 / 6 / 7 valid cycles; at 143 the last lane but one loses windows too (some counted, not all)
    "len_143_150_151": lambda: _batch(1002, [143, 150, 151, 150]),
    # fast_w = 7, 9 reads per wave, tiles of 7 groups: an odd group count; the last lane holds cycles 96..99, no window
    "len_100": lambda: _batch(1003, [100]),
    # lanes with exactly one counted window (23 = 16 + 7: none in the second lane; 8: one window; 9: two), and a read below one 8-mer
    "len_8_9_23_150": lambda: _batch(1004, [8, 150, 9, 150, 23, 150, 7, 150]),
    # one read group, balanced mates, 4 reads per group: one full chunk of 256 groups and a chunk with a single partial tile
    # (read groups get chunks of their own, so two of them would leave no chunk full)
    "len_250_1030_reads": lambda: _batch(1005, [250], n_reads=1030, n_lanes=1),
}

_CHILD = r"""
import pickle, sys
sys.path.insert(0, sys.argv[1])
from tests import test_gpu_short_instantiations as t
from tests.parity import run_gpu
out = {}
for name, make in t.BATCHES.items():
    cols, refs, opts = make()
    rc, counts, _ = run_gpu([cols], refs, **opts)
    out[name] = (rc, counts)
pickle.dump(out, open(sys.argv[2], "wb"))
"""


@pytest.fixture(scope="module")
def runtime_mask_results(tmp_path_factory):
    """Every batch through the run-time instantiation: one child process with BQC_SHORT_XCD=1 (mask 15 | 16)."""
    path = str(tmp_path_factory.mktemp("short_inst") / "child.pkl")
    env = dict(os.environ, BQC_SHORT_XCD="1")
    env.pop("BQC_SHORT_PARTS", None)
    out = subprocess.run([sys.executable, "-c", _CHILD, ROOT, path], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    return pickle.load(open(path, "rb"))


@pytest.mark.parametrize("name", list(BATCHES))
def test_both_instantiations_match_the_oracle(name, runtime_mask_results):
    assert "BQC_SHORT_PARTS" not in os.environ and "BQC_SHORT_XCD" not in os.environ  # this process runs the fixed instantiation
    cols, refs, opts = BATCHES[name]()
    rc_o, want, _ = run_oracle([cols], refs, **opts)
    rc_g, fixed, _ = run_gpu([cols], refs, **opts)
    rc_c, runtime = runtime_mask_results[name]
    assert (rc_o, rc_g, rc_c) == (0, 0, 0)
    assert int(want[0]["triplet"].sum()) > 0 and int(want[0]["eightmer"].sum()) > 0, "the batch must count something"
    d = _abi.diff_counts(want, fixed)
    assert not d, "fixed mask against the oracle:\n" + "\n".join(d[:20])
    d = _abi.diff_counts(want, runtime)
    assert not d, "run-time mask against the oracle:\n" + "\n".join(d[:20])
    d = _abi.diff_counts(fixed, runtime)
    assert not d, "fixed against run-time mask:\n" + "\n".join(d[:20])
