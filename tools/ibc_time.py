"""Device time of the indel tables (k_ibc; --indel-by-cycle) beside k_adp and k_gcb_reads on the same batch, on reads resident in HBM:
the config-2 shape (10 M x 150 bp over 4 x 25 M bases) with an indel in about 1 % of the reads and with one in every read, and the
long-read shape (50 K x 10 kb over 250 M bases) with an ONT-like CIGAR of about one operation per five bases — once as the kernel is
(a wave per long CIGAR) and once with BQC_IBC_T raised so that every read is walked by its own thread, each at the capacity of the
whole read (16 384) and at the program's default (1024), where the events behind the capacity are dropped and the walk is what is left.

usage: python tools/ibc_time.py [--reads N] [--long-reads N] [--passes P] [--only VARIANT] [--out FILE]
Every variant runs in a process of its own (BQC_IBC_T is read once per process).  The reads are synth.batch's with the CIGAR columns
replaced (and the NM tag taken away: it would no longer fit them).  Times come from bqc_set_timing / bqc_last_timing (HIP events
around each launch), after three warm-up passes, as the median and the range of P passes.  The floor is the bytes k_ibc must read —
flag, lane, l_seq, n_cigar, cigar_off and the CIGAR words of every read — at the card's measured copy rate."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
COPY_CEILING = 6.29e12  # bytes/s, the card's measured copy rate
SHAPES = {"short": dict(seed=1002, lens=[25_000_000] * 4, read_len=150, long_reads=False, isize=1000, max_read_len=1024, hist_cap=4096, N=1024),
          "long": dict(seed=1005, lens=[250_000_000], read_len=10_000, long_reads=True, isize=30_000, max_read_len=16_384, hist_cap=16_384, N=16_384)}
VARIANTS = {"short_1pct": ("short", 0.01, None, None), "short_every_read": ("short", 1.0, None, None),
            "long_wave_path": ("long", None, None, None), "long_thread_path": ("long", None, 65_535, None),
            # the program's default capacity: events behind cycle 1024 are dropped, what is left is the walk
            "long_wave_path_n1024": ("long", None, None, 1024), "long_thread_path_n1024": ("long", None, 65_535, 1024)}
COLUMN_BYTES = 2 + 1 + 4 + 2 + 4  # flag, lane, l_seq, n_cigar, cigar_off


def short_cigars(np, L, frac, rng):
    """LM, or for a fraction of the reads aM 1I bM / aM 1D bM at a place of the read's own."""
    n = len(L)
    ev = (rng.random(n) < frac) & (L >= 8)
    dele = rng.random(n) < 0.5
    a = 1 + (rng.random(n) * (L - 3)).astype(np.int64)
    ncig = np.where(ev, 3, 1)
    at = np.cumsum(ncig) - ncig
    w = np.zeros(int(ncig.sum()), np.int64)
    w[at[~ev]] = L[~ev] << 4
    w[at[ev]] = a[ev] << 4
    w[at[ev] + 1] = (1 << 4) | np.where(dele[ev], 2, 1)
    w[at[ev] + 2] = (L[ev] - a[ev] - np.where(dele[ev], 0, 1)) << 4
    return ncig, w, int(ev.sum())


def long_cigars(np, L):
    """(9M 1I 9M 1D) x g, then the rest as M: about one operation per five bases."""
    g = np.maximum((L - 1) // 19, 0)
    ncig = 4 * g + 1
    at = np.cumsum(ncig) - ncig
    k = np.arange(int(ncig.sum())) - np.repeat(at, ncig)
    w = np.array([9 << 4, (1 << 4) | 1, 9 << 4, (1 << 4) | 2], np.int64)[k % 4]
    w[at + ncig - 1] = (L - 19 * g) << 4
    return ncig, w, int(2 * g.sum())


def child(variant, reads, passes):
    import numpy as np
    from bamqc_amd import Aggregator, synth
    shape, frac, t, n_cap = VARIANTS[variant]
    S = dict(SHAPES[shape])
    if n_cap:
        S["N"] = n_cap
    refs = [synth.reference(S["seed"], i, n) for i, n in enumerate(S["lens"])]
    cols = synth.batch(S["seed"], reads, S["lens"], refs, read_len=S["read_len"], isize=S["isize"], long_reads=S["long_reads"])
    L = cols["l_seq"].astype(np.int64)
    rng = np.random.default_rng(7)
    ncig, w, n_ev = short_cigars(np, L, frac, rng) if shape == "short" else long_cigars(np, L)
    ncig = np.where(L > 0, ncig, 0)
    assert int(ncig.sum()) == len(w) or (L == 0).any()
    cols["n_cigar"], cols["cigar"] = ncig.astype(np.uint16), w.astype(np.uint32)
    cols["nm"] = np.full(len(L), -1, np.int32)
    a = Aggregator(n_refs=len(refs), isize=S["isize"], max_read_len=S["max_read_len"], hist_cap=S["hist_cap"], adapter_by_cycle=1024, gc_bias=100,
                   indel_by_cycle=S["N"])
    for i, r in enumerate(refs):
        a.set_reference(i, r)
    db = a.upload(cols)
    for _ in range(3):  # warm-up: code objects, clocks
        a.process(db)
    a.sync()
    a.set_timing(True)
    kt = {}
    for _ in range(passes):
        a.process(db)
        for k, v in a.last_timing().items():
            kt.setdefault(k, []).append(v)
    a.finalize()
    f = cols["flag"].astype(np.int64)
    examined = ((f & 0x904) == 0) & ((f & 0xC0) != 0) & (L > 0) & (ncig > 0)
    ev_sum = sum(int(x.sum()) for m in range(2) for x in a.indel_by_cycle(0, m)[1:3])
    e_sum = sum(int(a.indel_by_cycle(0, m)[0].sum()) for m in range(2))
    floor_bytes = reads * COLUMN_BYTES + 4 * len(w)
    out = {"variant": variant, "reads": reads, "bases": int(L.sum()), "cigar_words": int(len(w)), "indel_operations": n_ev, "BQC_IBC_T": t or 8, "N": S["N"],
           "examined_reads_per_pass": int(examined.sum()), "E_sum": e_sum, "event_sum": ev_sum, "passes_counted": passes + 3,
           "floor_bytes": floor_bytes, "floor_ms": floor_bytes / COPY_CEILING * 1e3, "kernels_ms": {}}
    assert e_sum == (passes + 3) * int(examined.sum()), (e_sum, int(examined.sum()))
    for k in ("k_ibc", "k_adp", "k_gcb_reads"):
        v = np.array(kt[k])
        out["kernels_ms"][k] = {"median": float(np.median(v)), "min": float(v.min()), "max": float(v.max()), "passes": [float(x) for x in v]}
    out["k_ibc_over_floor"] = out["kernels_ms"]["k_ibc"]["median"] / out["floor_ms"]
    print("IBC_CHILD " + json.dumps(out), flush=True)


def run_child(variant, reads, passes):
    env = dict(os.environ)
    t = VARIANTS[variant][2]
    if t:
        env["BQC_IBC_T"] = str(t)
    else:
        env.pop("BQC_IBC_T", None)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", variant, "--reads", str(reads), "--passes", str(passes)], env=env,
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return json.loads(next(l for l in r.stdout.splitlines() if l.startswith("IBC_CHILD "))[10:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--long-reads", type=int, default=50_000)
    ap.add_argument("--passes", type=int, default=9)
    ap.add_argument("--only", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None)
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.reads, args.passes)
    res = {"what": "tools/ibc_time.py: k_ibc beside k_adp and k_gcb_reads on the same batch, HIP-event times, median and range of the passes", "variants": {}}
    if args.out and os.path.exists(args.out):
        with open(args.out) as f:
            res = json.load(f)
    for variant, (shape, frac, t, n_cap) in VARIANTS.items():
        if args.only and variant != args.only:
            continue
        res["variants"][variant] = run_child(variant, args.reads if shape == "short" else args.long_reads, args.passes)
        print(variant, json.dumps(res["variants"][variant]), flush=True)
        if args.out:
            with open(args.out, "w") as f:
                json.dump(res, f, indent=1)
    v = res["variants"]
    for sfx in ("", "_n1024"):
        if "long_wave_path" + sfx in v and "long_thread_path" + sfx in v:
            key = "long_thread_over_wave" + sfx
            res[key] = v["long_thread_path" + sfx]["kernels_ms"]["k_ibc"]["median"] / v["long_wave_path" + sfx]["kernels_ms"]["k_ibc"]["median"]
            print("%s: %.2f" % (key, res[key]))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
