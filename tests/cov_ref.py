"""The coverage depth histogram restated in numpy / Python (TEST INFRASTRUCTURE): OverallNumbers::coverage as the oracle states it
(oracle/bamqc_oracle.c: coverage / update_coverage), one read at a time, with nothing of the kernels' data layout — no intervals, no
difference array, no tiles.  The windows and offsets come from tests/anchor_recurrence.per_group_anchors; a read's covered positions
from its CIGAR walked in sequenced order; the depth is kept per absolute window and read group and turned into the 101-bin histogram
at the end of the stream, the two live windows included.

Beside it a model of the plan the host makes for k_cov, restated from CovPlanner::finish (csrc/bqc_pipeline.cpp): the tiles per batch
and read group, each tile's read range, whether it is a common or a boundary tile, the host-side add for complete windows no tile
holds, and the extra intervals per batch.  tests/test_coverage_steps_cpu.py uses the model to prove that every batch of
tests/cov_steps.py crosses the edge it is named for."""
import numpy as np

from tests.anchor_recurrence import NO_WIN, per_group_anchors

VSIZE = 1000          # BQC_VSIZE: positions per window
COVSIZE = 100         # BQC_COVSIZE: the histogram's last (open) bin
TILE_WINDOWS = 4      # BQC_COV_TILE_WINDOWS
OPS = "MIDNSHP=X"


def read_ops(cols):
    """every read's CIGAR as [(count, operation), ...], as stored"""
    nc = np.asarray(cols["n_cigar"], np.int64)
    co = np.concatenate([[0], np.cumsum(nc)])
    cg = np.asarray(cols["cigar"], np.uint32)
    return [[(int(w) >> 4, OPS[int(w) & 15]) for w in cg[co[i]:co[i + 1]]] for i in range(len(nc))]


def covered_runs(ops, reverse):
    """the maximal runs [c0, c1) of covered positions relative to the read's offset: the CIGAR in sequenced order (reversed for a
    reverse read); S, M and D advance c; M and D cover; = X I N H P neither advance nor cover"""
    c, runs = 0, []
    for n, op in (reversed(ops) if reverse else ops):
        if op == "S":
            c += n
        elif op in "MD":
            if n:
                if runs and runs[-1][1] == c:
                    runs[-1][1] = c + n
                else:
                    runs.append([c, c + n])
            c += n
    return [(a, z) for a, z in runs]


def fresh_states(n_lanes):
    return [(True, 0, 0, 0)] * n_lanes


class ReadCov:
    """one read that enters coverage(): its index in the batch, read group, absolute window, offset, and covered runs [lo, hi) from the
    start of its first live window (not cut at 2000)"""
    __slots__ = ("index", "lane", "win", "rel", "off", "runs")

    def __init__(self, index, lane, win, rel, off, runs):
        self.index, self.lane, self.win, self.rel, self.off, self.runs = index, lane, win, rel, off, runs

    @property
    def counted(self):
        """the runs as they count: cut at 2000, empty ones dropped"""
        return [(lo, min(hi, 2 * VSIZE)) for lo, hi in self.runs if lo < 2 * VSIZE and lo < hi]

    @property
    def covered(self):
        return sum(hi - lo for lo, hi in self.counted)


def plan_tiles(reads, lanes, n, n_lanes, started_before):
    """CovPlanner::finish for one batch: reads = the batch's ReadCov in stream order, lanes = every read's lane.  Returns (tiles,
    untouched): a tile is a dict of lane, win_lo (relative to the read group's window at batch entry), win_final, list_begin, list_end,
    length, mixed, common; untouched[lane] = complete windows that no tile holds (the host's add to bin 0, in windows)"""
    lanes = np.asarray(lanes)
    in_range = lanes[lanes < n_lanes]
    mixed = len(set(in_range.tolist())) > 1 or (len(in_range) > 0 and len(in_range) < len(lanes))
    tiles, untouched = [], {}
    for l in range(n_lanes):
        mine = [r for r in reads if r.lane == l]
        if not mine:
            continue
        rel = np.array([r.rel for r in mine], np.int64)
        idx = np.array([r.index for r in mine], np.int64)
        assert np.all(np.diff(rel) >= 0)
        W1 = int(rel[-1])

        def first_at(k):  # the first read of the group whose window is >= k
            j = int(np.searchsorted(rel, k, "left"))
            return int(idx[j]) if j < len(idx) else n

        want = []
        if started_before[l]:
            want += [0, 1]
        for w in sorted(set(rel.tolist())):
            want += [w, w + 1]
        last_tile, covered_final = -1, 0
        for w in want:
            t = w // TILE_WINDOWS
            if t <= last_tile:
                continue
            last_tile = t
            wlo = t * TILE_WINDOWS
            begin, end = first_at(0 if wlo == 0 else wlo - 1), first_at(wlo + TILE_WINDOWS)
            tiles.append(dict(lane=l, win_lo=wlo, win_final=W1, list_begin=begin, list_end=end, length=end - begin, mixed=mixed,
                              common=wlo >= 2 and wlo + TILE_WINDOWS <= W1))
            covered_final += max(0, min(wlo + TILE_WINDOWS, W1) - wlo)
        untouched[l] = max(0, W1 - covered_final)
    return tiles, untouched


class Coverage:
    """what coverage() below returns: poscov (n_lanes, 101); per batch the reads that entered coverage(), the tiles, the untouched
    windows per read group and the number of extra intervals; depth[lane] = {absolute window: depth per position}, last[lane] = the
    read group's first live window at the end of the stream"""

    def __init__(self):
        self.poscov, self.reads, self.tiles, self.untouched, self.n_extra, self.depth, self.last = None, [], [], [], [], None, None

    def window_depth(self, lane, win):
        d = self.depth[lane].get(win)
        return d if d is not None else np.zeros(VSIZE, np.int64)


def coverage(batches, n_lanes, n_refs):
    out = Coverage()
    depth = [dict() for _ in range(n_lanes)]
    states = fresh_states(n_lanes)
    for cols in batches:
        n = len(cols["flag"])
        base = [s[3] for s in states]
        started_before = [not s[0] for s in states]
        win, off, states = per_group_anchors(cols, states, n_lanes, n_refs)
        ops = read_ops(cols)
        reads = []
        for i in range(n):
            if win[i] == NO_WIN:
                continue
            lane = int(cols["lane"][i])
            rel, p = int(win[i]), int(off[i])
            W = base[lane] + rel
            runs = [(p + a, p + z) for a, z in covered_runs(ops[i], bool(int(cols["flag"][i]) & 0x10))]
            r = ReadCov(i, lane, W, rel, p, runs)
            reads.append(r)
            for lo, hi in runs:
                for v in range(lo, min(hi, 2 * VSIZE)):  # positions at or beyond 2000 from the window start are dropped
                    d = depth[lane].setdefault(W + v // VSIZE, np.zeros(VSIZE, np.int64))
                    d[v % VSIZE] += 1
        tiles, untouched = plan_tiles(reads, cols["lane"], n, n_lanes, started_before)
        out.reads.append(reads)
        out.tiles.append(tiles)
        out.untouched.append(untouched)
        out.n_extra.append(sum(max(0, len(r.counted) - 1) for r in reads))
    # every window up to the two live ones of the end of the stream is histogrammed once (a read group that never entered
    # coverage() flushes two empty windows)
    poscov = np.zeros((n_lanes, COVSIZE + 1), np.uint64)
    for l in range(n_lanes):
        n_win = states[l][3] + 2
        assert all(w < n_win for w in depth[l])
        poscov[l, 0] += (n_win - len(depth[l])) * VSIZE
        for d in depth[l].values():
            poscov[l] += np.bincount(np.minimum(d, COVSIZE), minlength=COVSIZE + 1).astype(np.uint64)
    out.poscov, out.depth, out.last = poscov, depth, [s[3] for s in states]
    return out
