"""SAM text inside BGZF (x.sam.gz) through this tree's program, against another build of it (the parent commit's, which reads the
same reads only as a BAM file or as plain SAM text on stdin), alternating; where the record loop's time goes; the stream size from which
the card is not slower than this build's host reader; and the inputs of the parent whose code paths this change touches.  Writes
profiles/sam_bgzf_ab.json.

usage: python tools/sam_bgzf_time.py --parent DIR [--reads 4000000] [--out profiles/sam_bgzf_ab.json] [--no-crossing] [--no-bench]
  DIR: a built checkout of the program to compare with (DIR/bin/bamqualcheck, DIR/bench.py).
The reads are those of `bench.py --full`'s generator (seed 1002, four contigs of 25 Mb), written as x.bam (level 1), as x.sam (bqc_sam_write) and
as x.sam.gz: the text in members of 0xff00 bytes at level 1, compressed here by a pool of threads.  Streams are fed from the page cache by
`cat`.  Every run has a time limit of its own; the first run that does not end with status 0 ends the script."""
import argparse
import json
import os
import re
import struct
import subprocess
import sys
import tempfile
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bamqc_amd import hostio  # noqa: E402

NAMES, LENS = ["chr1", "chr2", "chr3", "chr4"], [25_000_000] * 4
EOF_MEMBER = bytes([31, 139, 8, 4, 0, 0, 0, 0, 0, 255, 6, 0, 66, 67, 2, 0, 27, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0])


def member(payload):
    c = zlib.compressobj(1, zlib.DEFLATED, -15)
    comp = c.compress(payload) + c.flush()
    return (bytes([31, 139, 8, 4, 0, 0, 0, 0, 0, 255, 6, 0, 66, 67, 2, 0]) + struct.pack("<H", 18 + len(comp) + 8 - 1) + comp +
            struct.pack("<II", zlib.crc32(payload) & 0xFFFFFFFF, len(payload)))


def bgzf_file(src, dst):
    """src as BGZF: members of 0xff00 bytes at level 1 (zlib releases the interpreter lock: 16 threads), the EOF marker member at the end"""
    with open(src, "rb") as f, open(dst, "wb") as g, ThreadPoolExecutor(16) as pool:
        while True:
            piece = f.read(0xff00 * 1024)
            if not piece:
                break
            for m in pool.map(member, [piece[i:i + 0xff00] for i in range(0, len(piece), 0xff00)]):
                g.write(m)
        g.write(EOF_MEMBER)


def generate(tmp, reads, tag="x", fasta=True):
    import numpy as np
    bam, fa, sam, gz = (os.path.join(tmp, tag + e) for e in (".bam", ".fa", ".sam", ".sam.gz"))
    hostio.synth_stream(bam, fa if fasta else None, 1002, reads, NAMES, LENS, level=1)
    f = hostio.BamFile(bam)
    got = list(f.batches(1 << 20, 1 << 40))
    f.close()
    cols = {k: np.concatenate([b[k] for b in got]) for k in got[0]}
    hostio.write_sam(sam, cols, NAMES, LENS)
    bgzf_file(sam, gz)
    return bam, fa, sam, gz


def run(exe, path, fa, out, env, how, tmp, limit=300):
    """One run: how = "file" (`exe ... path`), "stdin" (`cat path | exe ... -`) or "fifo" (`cat path > FIFO` beside `exe ... FIFO`, the FIFO without an extension).  (wall seconds, stderr)"""
    fifo, cat, stdin = os.path.join(tmp, "stream"), None, subprocess.DEVNULL
    t0 = time.perf_counter()
    if how == "fifo":
        if os.path.exists(fifo):
            os.unlink(fifo)
        os.mkfifo(fifo)
        cat = subprocess.Popen("exec cat '%s' > '%s'" % (path, fifo), shell=True)
    elif how == "stdin":
        cat = subprocess.Popen(["cat", path], stdout=subprocess.PIPE)
        stdin = cat.stdout
    arg = path if how == "file" else "-" if how == "stdin" else fifo
    r = subprocess.run(["timeout", "-k", "10", str(limit), exe, "-r", fa, "-o", out, "-c", ",".join(NAMES), arg], stdin=stdin, capture_output=True, text=True,
                       env=dict(os.environ, BQC_TIMING="1", **env))
    dt = time.perf_counter() - t0
    if cat is not None:
        if how == "stdin":
            cat.stdout.close()
        if r.returncode != 0:
            cat.kill()
        cat.wait()
        if how == "fifo":
            os.unlink(fifo)
    if r.returncode != 0:
        print(r.stderr[-3000:])
        sys.exit("a run ended with status %d: nothing more is started" % r.returncode)
    return dt, r.stderr


def where_the_time_goes(err):
    m = re.search(r"records decoded (.*)", err)
    out = dict(reader=m.group(1) if m else "?", lines=[ln for ln in err.splitlines() if ln.startswith(("[sam reader]", "[timing] reader on the card", "[timing] phases"))])
    m = re.search(r"(\d+) records: decode thread busy ([\d.]+) s, .* loop ([\d.]+) s", err)
    if m:
        out["record_loop"] = dict(records=int(m.group(1)), decode_thread_busy_s=float(m.group(2)), loop_s=float(m.group(3)))
    m = re.search(r"text inflated on the card: .*? ([\d.]+) s in the producer's reader thread.*?, the producer waited ([\d.]+) s for chunks, the decode thread waited ([\d.]+) s for inflated runs", err)
    if m and "record_loop" in out:
        rd, chunks, runs = (float(x) for x in m.groups())
        loop = out["record_loop"]["loop_s"]
        out["producer_seconds"] = dict(reading=rd, producer_waiting_for_chunks=chunks, decode_thread_waiting_for_runs=runs)
        # the producer stands still for chunks: the pipe or file is behind; it does not, but the consumer waits for runs: copies and inflate kernels
        # are; neither: the text decode, the batch tail and the submitting thread
        out["bound_by"] = "pipe" if chunks > 0.5 * loop else "inflate" if runs > 0.5 * loop else "text decode and submit"
    return out


def series(label, legs, tmp, reads):
    """legs: [(name, exe, path, fa, env, how)] — three rounds, the legs in turn within each.  name -> walls, spread, where the last run's time went"""
    res = {name: dict(seconds=[]) for name, *_ in legs}
    for rep in range(3):
        for name, exe, path, fa, env, how in legs:
            dt, err = run(exe, path, fa, os.path.join(tmp, name + ".bamqc"), env, how, tmp)
            res[name]["seconds"].append(dt)
            res[name]["last"] = where_the_time_goes(err)
            print("%s: %s run %d: %.3f s = %.2f M reads/s (%s)" % (label, name, rep, dt, reads / dt / 1e6, res[name]["last"]["reader"]), flush=True)
    outs = {open(os.path.join(tmp, name + ".bamqc"), "rb").read() for name, *_ in legs}
    assert len(outs) == 1, "outputs differ"
    for v in res.values():
        v["best"], v["spread"] = min(v["seconds"]), max(v["seconds"]) - min(v["seconds"])
    return res


def bench_once(tree):
    r = subprocess.run(["timeout", "-k", "10", "200", sys.executable, "bench.py", "--gpus", "1", "--steps", "20", "--warmup", "5"], cwd=tree, capture_output=True, text=True)
    if r.returncode != 0:
        print(r.stderr[-3000:])
        sys.exit("bench.py ended with status %d: nothing more is started" % r.returncode)
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True)
    ap.add_argument("--reads", type=int, default=4_000_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sam_bgzf_ab.json"))
    ap.add_argument("--no-crossing", action="store_true")
    ap.add_argument("--no-bench", action="store_true")
    a = ap.parse_args()
    new_exe, old_exe = os.path.join(ROOT, "bin", "bamqualcheck"), os.path.join(a.parent, "bin", "bamqualcheck")
    res = dict(reads=a.reads, read_length=150, how="three rounds, the legs in turn within each round, on one box; streams fed from the page cache by cat")
    with tempfile.TemporaryDirectory(prefix="bqc_sam_bgzf_") as tmp:
        t0 = time.perf_counter()
        bam, fa, sam, gz = generate(tmp, a.reads)
        res["bytes"] = dict(bam=os.path.getsize(bam), sam=os.path.getsize(sam), sam_gz=os.path.getsize(gz))
        print("%d reads: x.bam %.0f MB, x.sam %.0f MB, x.sam.gz %.0f MB, generated in %.1f s" % (a.reads, res["bytes"]["bam"] / 1e6, res["bytes"]["sam"] / 1e6, res["bytes"]["sam_gz"] / 1e6,
                                                                                              time.perf_counter() - t0), flush=True)
        for p in (bam, sam, gz):
            subprocess.run(["cat", p], stdout=subprocess.DEVNULL)  # (into the page cache)
        # 2. against the parent: its two inputs for these reads, and this build's two new ones
        res["against_parent"] = series("against the parent", [("parent_bam_file", old_exe, bam, fa, {}, "file"), ("parent_sam_stdin", old_exe, sam, fa, {}, "stdin"),
                                                              ("new_sam_gz_file", new_exe, gz, fa, {}, "file"), ("new_sam_gz_stdin", new_exe, gz, fa, {}, "stdin")], tmp, a.reads)
        # 3. what was touched: the BAM file (gpu_bam.hip's producer) and plain SAM text on stdin (gpu_sam.hip's source side), parent and new in turn
        res["touched"] = series("touched paths", [("parent_bam_file", old_exe, bam, fa, {}, "file"), ("new_bam_file", new_exe, bam, fa, {}, "file"),
                                                  ("parent_sam_stdin", old_exe, sam, fa, {}, "stdin"), ("new_sam_stdin", new_exe, sam, fa, {}, "stdin")], tmp, a.reads)
        for what in ("bam_file", "sam_stdin"):
            p, n = res["touched"]["parent_" + what], res["touched"]["new_" + what]
            n["inside_parent_spread"] = n["best"] <= p["best"] + p["spread"]
        for p in (bam, sam, gz):
            os.unlink(p)
        # 1. the switch-over point of BGZF SAM: this build's host reader against the card forced, from a FIFO without an extension
        if not a.no_crossing:
            # (a short stream of this generator compresses less well than the long one: the reads for a size are found from a first try)
            cross = []
            for mb in (16, 64, 256):
                n = int((mb << 20) / (res["bytes"]["sam_gz"] / a.reads))
                _, _, _, part = generate(tmp, n, tag="head", fasta=False)
                n = int(n * (mb << 20) / os.path.getsize(part))
                _, _, _, part = generate(tmp, n, tag="head", fasta=False)
                row = dict(compressed_mb_wanted=mb, reads=n, compressed_bytes=os.path.getsize(part), host=[], card=[])
                for rep in range(3):
                    row["host"].append(run(new_exe, part, fa, os.path.join(tmp, "hh.bamqc"), {"BQC_GPU_DECODE": "0"}, "fifo", tmp, 200)[0])
                    row["card"].append(run(new_exe, part, fa, os.path.join(tmp, "hc.bamqc"), {"BQC_GPU_DECODE": "1"}, "fifo", tmp, 200)[0])
                assert open(os.path.join(tmp, "hh.bamqc"), "rb").read() == open(os.path.join(tmp, "hc.bamqc"), "rb").read(), "outputs differ at %d MB" % mb
                print("%3d MB wanted, %.1f MB written: host %s, card %s" % (mb, row["compressed_bytes"] / 1e6, ["%.3f" % x for x in row["host"]], ["%.3f" % x for x in row["card"]]), flush=True)
                cross.append(row)
            res["crossing"] = cross
            res["crossing_what"] = "both sides are this build's code: a switch-over point, no statement about speed against the parent"
            t_mb = None  # the smallest size from which (and above which) the card is not slower
            for r in reversed(cross):
                if min(r["card"]) > min(r["host"]):
                    break
                t_mb = r["compressed_bytes"] / 1e6
            res["card_not_slower_from_mb_written"] = t_mb
    if not a.no_bench:  # parent, new, parent, new, parent, new
        runs = [(who, bench_once(tree)) for who, tree in (("parent", a.parent), ("new", ROOT)) * 3]
        res["bench"] = [dict(build=who, line=line) for who, line in runs]
        for who, line in runs:
            print("bench %s: %s" % (who, json.dumps(line)[:300]), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
