"""GPU: the walk frame that k_sac, k_rcv and k_wdp share (bamqc_amd/csrc/cigar_walk.h: a workgroup's share of the processing order, the
list of a step's long reads, a wave's pass over a long CIGAR, three sums a read group) on ONE batch through the three modules enabled
together in one context, against the modules' restatements (tests/sac_ref.py, rcv_ref.py, wdp_ref.py): the modules' blocks of the
exported state, word for word.

The batch: 3 x 1024 + 1 reads, every one with a CIGAR of 9, 65 or 129 operations — more than the thread paths' 8, and one pass of a wave,
two and three with one operation in the last — so every read is listed and walked by a wave, and every workgroup's step lists more
reads than it has waves (16).  The read groups are 0, 1, 62, 63, 64 and 65 of 66: on both sides of the 64 whose sums a workgroup
keeps in LDS.  The batch is submitted once with its reads grouped by read group, so that the processing order is the file's, and once
shuffled, so that it is a permutation.

What that batch does not reach: the launches give a workgroup ceil(n / grid) reads with grid = min(CUs, ceil(n / 256)), so its 3073
reads are 13 shares of one step each wherever the card has 13 CUs or more, and the lists' three counters do not rotate.  A workgroup
comes back to its first counter in its FOURTH step, which needs more than 3 x 1024 reads per CU: test_four_steps_per_workgroup runs
tests/sac_steps.py's step batch (reads of 20 bases, sixteen CIGARs of 12 operations in every 1024 reads) at that size through the
same three modules."""
import numpy as np
import pytest

from bamqc_amd import Aggregator
from tests import lane_limit, rcv_ref, sac_ref, sac_steps, wdp_ref
from tests.rcv_steps import regions_of
from tests.sac_steps import FIRST, LAST, P, REV, cols_of, mixed_cigar, query_len, sac_launch, sites_of
from tests.test_gpu_value_limits import n_cu

pytestmark = pytest.mark.gpu

N = 3 * 1024 + 1
NCIGARS = (9, 65, 129)
GROUPS = (0, 1, 62, 63, 64, 65)
N_LANES = 66
LENS = [30_000, 12_000]  # (the reads of contig 1 run past its end: the windows' X)
W, MQ, MQ_WINDOWS, Q = 100, 20, 30, 20


@pytest.fixture(scope="module")
def frame():
    """(cols, sites, regions, the three expected blocks).  Built once, never changed."""
    reads = []
    for k in range(N):
        cig = mixed_cigar(NCIGARS[k % 3], k % 5)
        ql = query_len(cig)
        reads.append(dict(cigar=cig, L=ql - (1 if k % 7 == 0 else 0), pos=7 * k, rid=k % 2, lane=GROUPS[k * len(GROUPS) // N],
                          flag=P | (FIRST if k % 3 else LAST | REV), mapq=(20, 60)[k % 4 == 0]))
    cols = cols_of(reads, 5)
    cols["qual"] = np.full_like(cols["qual"], 40)  # (every base counts at a site: the bases are A, C, G, T)
    span = 7 * N + 400
    sites = sites_of([(r, p) for r in (0, 1) for p in range(0, span, 5)] + [(r["rid"], r["pos"]) for r in reads])
    regions = regions_of([(r, p, p + 7) for r in (0, 1) for p in range(0, span, 10)])
    T = sac_ref.table_fast(cols, sites, N_LANES, 2, Q, MQ)
    Sr = rcv_ref.state_fast(cols, regions, N_LANES, 2, MQ)
    Sw = wdp_ref.state_fast(cols, W, LENS, N_LANES, MQ_WINDOWS)
    # no read is skipped: every read is examined by all three, is long, and counts at the site under its first base
    assert int(Sr[:, 0].sum()) == N and int((Sw[:, 0] + Sw[:, 1]).sum()) == N and (Sw[:, 1] > 0).any() and (Sw[:, 2] > 0).any()
    assert (cols["n_cigar"] > 8).all() and sorted(set(cols["n_cigar"].tolist())) == list(NCIGARS)
    at = {(int(r), int(p)): i for i, (r, p) in enumerate(zip(*sites))}
    own = np.array([at[(r["rid"], r["pos"])] for r in reads])
    assert (T[cols["lane"].astype(np.int64), own].sum(axis=1) >= 1).all()
    for g in GROUPS:
        assert Sr[g, 0] > 0 and Sr[g, 1] > 0 and Sr[g, 2] > 0 and Sw[g, 0] > 0 and Sw[g, 1] > 0 and T[g].any(), g
    assert (Sw[[63, 64, 65], 2] > 0).all()  # (X on both sides of the LDS table)
    assert not Sr[2:62].any() and not Sw[2:62].any() and not T[2:62].any()
    # every workgroup lists more reads than it has waves, whatever the card's CUs (at most 13 workgroups)
    assert all(e - b > 16 for n_cu in (1, 13, 256) for b, e in sac_launch(N, n_cu)["shares"])
    return cols, sites, regions, (T, Sr, Sw)


def blocks(a, sites, regions, lens=LENS):
    """The three modules' words of the exported state: the windows', the regions', the sites', in that order at its end."""
    v = a.state_export_host()
    n_sac = N_LANES * len(sites[0]) * 8
    n_rcv = N_LANES * (4 + int((regions[2].astype(np.int64) - regions[1]).sum()) + len(regions[0]))
    n_wdp = N_LANES * (4 + 3 * wdp_ref.layout(W, lens)[3])
    sac = v[len(v) - n_sac:]
    rcv = v[len(v) - n_sac - n_rcv:len(v) - n_sac]
    wdp = v[len(v) - n_sac - n_rcv - n_wdp:len(v) - n_sac - n_rcv]
    return sac.reshape(N_LANES, -1, 8), rcv.reshape(N_LANES, -1), wdp.reshape(N_LANES, -1)


def run_and_check(cols, sites, regions, lens, want):
    a = Aggregator(n_lanes=N_LANES, n_refs=len(lens), main_chrom=[0] * len(lens), max_read_len=16_384, isize=2000, site_alleles=sites, site_min_qual=Q,
                   site_min_mapq=MQ, regions=regions, region_min_mapq=MQ, window_depth=(W, lens), window_min_mapq=MQ_WINDOWS)
    a.submit(cols)
    a.finalize()
    for name, got, exp in zip(("k_sac", "k_rcv", "k_wdp"), blocks(a, sites, regions, lens), want):
        assert got.shape == exp.shape, (name, got.shape, exp.shape)
        bad = np.argwhere(got != exp)
        assert not len(bad), "%s: %d words differ, first %s: %d != %d" % (name, len(bad), bad[0].tolist(), got[tuple(bad[0])], exp[tuple(bad[0])])
    a.close()


@pytest.mark.parametrize("order", ["file", "permuted"])
def test_three_walks_of_one_batch(frame, order):
    cols, sites, regions, want = frame
    if order == "permuted":
        perm = np.random.default_rng(11).permutation(N)
        cols = lane_limit.take(cols, perm)
        assert (np.diff(cols["lane"].astype(np.int64)) < 0).any()  # (the processing order is no longer the file's)
    else:
        assert (np.diff(cols["lane"].astype(np.int64)) >= 0).all()
    run_and_check(cols, sites, regions, LENS, want)


def test_four_steps_per_workgroup():
    """More than 3 x 1024 reads for every CU: every workgroup makes four steps, each with 16 listed reads for its 16 waves, and the
    fourth counts its listed reads in the counter of the first.  Read groups 0, 63, 64 and 65, changing on a step's seam and inside
    steps."""
    cu = n_cu()
    n = 3 * sac_steps.SA_STEP * cu + 977
    while min(sac_launch(n, cu)["steps"]) < 4:
        n += 1
    la = sac_launch(n, cu)
    assert la["grid"] == cu and min(la["steps"]) == 4
    lane = np.zeros(n, np.uint8)
    for c, g in (((cu // 3) * la["per"] + 3 * sac_steps.SA_STEP, 63), ((2 * cu // 3) * la["per"] + sac_steps.SA_STEP + 333, 64), ((5 * cu // 6) * la["per"] + 500, 65)):
        lane[c:] = g
    cols, sites = sac_steps.step_batch(dict(n=n, lane=lane))
    assert ((cols["n_cigar"] > 8).reshape(-1)[:n - n % 1024].reshape(-1, 1024).sum(axis=1) == 16).all()
    lens = [n // 8 + 200]
    regions = regions_of([(0, p, p + 20) for p in range(3, n // 8 + 120, 50)])
    want = (sac_ref.table_fast(cols, sites, N_LANES, 1, Q, MQ), rcv_ref.state_fast(cols, regions, N_LANES, 1, MQ), wdp_ref.state_fast(cols, W, lens, N_LANES, MQ_WINDOWS))
    assert int(want[1][:, 0].sum()) == n == int((want[2][:, 0] + want[2][:, 1]).sum()) and all(want[1][g, 1] > 1000 and want[0][g].sum() > 1000 for g in (0, 63, 64, 65))
    run_and_check(cols, sites, regions, lens, want)
