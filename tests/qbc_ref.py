"""The per-cycle base quality histogram (--qual-by-cycle) restated in numpy from its definition in include/bamqc.h: a loop over
the reads of a column dict.  Shares nothing with the kernel (bamqc_amd/csrc/k_qcyc.hip)."""
import numpy as np

QPAD = 224  # Phred 0..222, rows padded


def table(cols_list, n_lanes, N):
    """H[lane][mate][cycle][q] over the batches: reads that are neither supplementary nor secondary, have a mate flag (0x40 ->
    0, else 0x80 -> 1) and qualities; stored byte j of a read of length L is cycle j, or L-1-j with 0x10; cycles < N only."""
    H = np.zeros((n_lanes, 2, N, QPAD), np.uint64)
    for cols in ([cols_list] if isinstance(cols_list, dict) else cols_list):
        L = cols["l_seq"].astype(np.int64)
        off = np.cumsum(L) - L
        for i, f in enumerate(cols["flag"].astype(np.int64)):
            if f & 0x900 or not f & 0xC0 or f & 0x8000:
                continue
            q = cols["qual"][off[i]:off[i] + L[i]].astype(np.int64)
            cyc = np.arange(L[i])[::-1] if f & 0x10 else np.arange(L[i])
            keep = (cyc < N) & (q <= 222)
            np.add.at(H[cols["lane"][i], 0 if f & 0x40 else 1], (cyc[keep], q[keep]), 1)
    return H


def table_fast(cols_list, n_lanes, N):
    """table(), vectorised for batches of hundreds of thousands of reads: one entry per stored base (np.repeat), its cycle, mate
    and read group, and one np.bincount over the flat bin index.  Written from the same definition; tests/test_cycle_steps_cpu.py
    holds the two against each other bit for bit."""
    H = np.zeros(n_lanes * 2 * N * QPAD, np.int64)
    for cols in ([cols_list] if isinstance(cols_list, dict) else cols_list):
        L = cols["l_seq"].astype(np.int64)
        f = cols["flag"].astype(np.int64)
        counted = ((f & 0x900) == 0) & ((f & 0xC0) != 0) & ((f & 0x8000) == 0)
        read = np.repeat(np.arange(len(L)), L)                                   # the read of every stored base
        j = np.arange(int(L.sum()), dtype=np.int64) - np.repeat(np.cumsum(L) - L, L)  # its index in the read
        cyc = np.where((f[read] & 0x10) != 0, L[read] - 1 - j, j)
        q = cols["qual"][:len(read)].astype(np.int64)
        mate = np.where((f & 0x40) != 0, 0, 1)
        keep = counted[read] & (cyc < N) & (q <= 222)
        bins = ((cols["lane"].astype(np.int64)[read] * 2 + mate[read]) * N + cyc) * QPAD + q
        H += np.bincount(bins[keep], minlength=len(H))
    return H.reshape(n_lanes, 2, N, QPAD).astype(np.uint64)


def sizes(H_lm, mate_cycles):
    """(n_cycles, n_q) of one lane and mate: min(N, the mate's n_cycles in bqc_mate_counts), 1 + the highest Phred counted."""
    nz = np.nonzero(H_lm.sum(axis=0))[0]
    return min(H_lm.shape[0], mate_cycles), (int(nz[-1]) + 1 if len(nz) else 0)


def text(H, cycles, sample_id, lane_names, lane_index=None):
    """The `.qbc` text: lanes in the order given, per mate a key line with the sizes, then one line of n_q counts per cycle.
    cycles[lane][mate]: the mate's n_cycles in bqc_mate_counts (the length of its per-cycle lines in the `.bamqc`)."""
    out = []
    for k, name in enumerate(lane_names):
        l = k if lane_index is None else lane_index[k]
        out += ["sample_id " + sample_id, "lane " + name]
        for m, key in enumerate(("first", "second")):
            nc, nq = sizes(H[l, m], int(cycles[l, m]))
            out.append("base_qual_histogram_by_position_%s %d %d" % (key, nc, nq))
            if nq:
                out += [" ".join(str(int(v)) for v in H[l, m, c, :nq]) for c in range(nc)]
    return "\n".join(out) + "\n"
