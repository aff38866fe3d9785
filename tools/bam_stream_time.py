"""`cat x.bam > FIFO | bamqualcheck FIFO`: a BAM STREAM through this tree's program (the reader on the card) against another
build of it (the parent commit's: the host reader), alternating; where the record loop's time goes; the stream size from which the card is not
slower (T); and the FILE path of the two builds, whose producer this change touches.  Writes profiles/bam_stream_ab.json.

usage: python tools/bam_stream_time.py --parent DIR [--reads 10000000] [--out profiles/bam_stream_ab.json] [--no-level0] [--no-crossing] [--no-file] [--no-bench]
  DIR: a built checkout of the program to compare with (DIR/bin/bamqualcheck, DIR/bench.py).
The stream is the file of `bench.py --full` (seed 1002, four contigs of 25 Mb, BGZF level 1) and the same reads written at level 0, fed from the
page cache by `cat` into a FIFO named *.bam (a path both builds take: the parent refuses a path without the extension, /dev/stdin among them).
T: whole-program time on streams of the same generator of 16 / 64 / 256 MB of compressed bytes, the parent against the card forced, best of three.
Every run has a time limit of its own; the first run that does not end with status 0 ends the script."""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bamqc_amd import hostio  # noqa: E402

NAMES, LENS = ["chr1", "chr2", "chr3", "chr4"], [25_000_000] * 4


def run(exe, bam, fa, out, env, tmp, stream=True, limit=300):
    """One run: `cat bam > fifo` beside `exe ... fifo` (stream), or `exe ... bam` (file).  (wall seconds, stderr)"""
    fifo = os.path.join(tmp, "stream.bam")
    cat = None
    t0 = time.perf_counter()
    if stream:
        if os.path.exists(fifo):
            os.unlink(fifo)
        os.mkfifo(fifo)
        cat = subprocess.Popen("exec cat '%s' > '%s'" % (bam, fifo), shell=True)
    r = subprocess.run(["timeout", "-k", "10", str(limit), exe, "-r", fa, "-o", out, "-c", ",".join(NAMES), fifo if stream else bam], stdin=subprocess.DEVNULL, capture_output=True,
                       text=True, env=dict(os.environ, BQC_TIMING="1", **env))
    dt = time.perf_counter() - t0
    if cat is not None:
        if r.returncode != 0:
            cat.kill()
        cat.wait()
        os.unlink(fifo)
    if r.returncode != 0:
        print(r.stderr[-3000:])
        sys.exit("a run ended with status %d: nothing more is started" % r.returncode)
    return dt, r.stderr


def where_the_time_goes(err):
    out = dict(reader="card" if "records decoded on the GPU" in err else "host", timing_lines=[ln for ln in err.splitlines() if ln.startswith("[timing]")])
    m = re.search(r"(\d+) records: decode thread busy ([\d.]+) s, .* loop ([\d.]+) s", err)
    if m:
        out["record_loop"] = dict(records=int(m.group(1)), decode_thread_busy_s=float(m.group(2)), loop_s=float(m.group(3)), reads_per_s=int(m.group(1)) / max(float(m.group(3)), 1e-9))
    m = re.search(r"a stream, read\(\) and waiting for it ([\d.]+) s in its one reader thread, the producer waited ([\d.]+) s for chunks, the decode thread waited ([\d.]+) s for inflated runs", err)
    if m and "record_loop" in out:
        rd, chunks, runs = (float(x) for x in m.groups())
        loop = out["record_loop"]["loop_s"]
        out["stream_reader_seconds"] = dict(read_and_waiting_for_the_pipe=rd, producer_waiting_for_chunks=chunks, decode_thread_waiting_for_runs=runs)
        # the producer stands still for chunks: the pipe (and its one reader thread) is behind; it does not, but the consumer waits for runs: the
        # inflate kernels (and the copies in front of them) are; neither: the consumer's own work (walk, decode, copy, anchors) or the submitting thread
        out["bound_by"] = "pipe" if chunks > 0.5 * loop else "inflate" if runs > 0.5 * loop else "walk, decode and submit"
    return out


def ab(label, old_exe, new_exe, bam, fa, tmp, reads, stream, new_env):
    walls, last = dict(parent=[], new=[]), ""
    for rep in range(3):
        for who, exe in (("parent", old_exe), ("new", new_exe)):
            dt, err = run(exe, bam, fa, os.path.join(tmp, who + ".bamqc"), new_env if who == "new" else {}, tmp, stream)
            walls[who].append(dt)
            print("%s: %s run %d: %.3f s = %.2f M reads/s" % (label, who, rep, dt, reads / dt / 1e6), flush=True)
            last = err if who == "new" else last
            if who == "parent":
                parent_err = err
    same = open(os.path.join(tmp, "parent.bamqc"), "rb").read() == open(os.path.join(tmp, "new.bamqc"), "rb").read()
    assert same, "outputs differ"
    res = dict(program_seconds=walls, outputs_identical=True, parent_spread_seconds=max(walls["parent"]) - min(walls["parent"]), new_spread_seconds=max(walls["new"]) - min(walls["new"]),
               factor_best_of_three=min(walls["parent"]) / min(walls["new"]), new=where_the_time_goes(last), parent=where_the_time_goes(parent_err))
    res["new_inside_parent_spread"] = abs(min(walls["new"]) - min(walls["parent"])) <= res["parent_spread_seconds"]
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
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bam_stream_ab.json"))
    ap.add_argument("--no-level0", action="store_true")
    ap.add_argument("--no-crossing", action="store_true")
    ap.add_argument("--no-file", action="store_true")
    ap.add_argument("--no-bench", action="store_true")
    a = ap.parse_args()
    new_exe, old_exe = os.path.join(ROOT, "bin", "bamqualcheck"), os.path.join(a.parent, "bin", "bamqualcheck")
    res = dict(reads=a.reads, read_length=150, how="cat x.bam > FIFO (page cache) beside bamqualcheck FIFO; three alternating pairs (parent, new) on one box")
    with tempfile.TemporaryDirectory(prefix="bqc_bam_stream_") as tmp:
        bam, fa = os.path.join(tmp, "x.bam"), os.path.join(tmp, "x.fa")
        t0 = time.perf_counter()
        hostio.synth_stream(bam, fa, 1002, a.reads, NAMES, LENS, level=1)
        res["compressed_bytes"] = os.path.getsize(bam)
        print("stream: %d reads, %.0f MB at level 1, generated in %.1f s" % (a.reads, res["compressed_bytes"] / 1e6, time.perf_counter() - t0), flush=True)
        subprocess.run(["cat", bam], stdout=subprocess.DEVNULL)  # (into the page cache)
        res["stream_level1"] = ab("stream, level 1", old_exe, new_exe, bam, fa, tmp, a.reads, True, {})
        if not a.no_file:  # the file path (its producer is touched): the measurement of bench.py --full's e2e leg — wall time of the program on this file — as alternating pairs
            res["file_level1"] = ab("file, level 1", old_exe, new_exe, bam, fa, tmp, a.reads, False, {})
        if not a.no_crossing:
            per_read = res["compressed_bytes"] / a.reads
            cross = []
            for mb in (16, 64, 256):
                n = int((mb << 20) / per_read)
                part = os.path.join(tmp, "head.bam")
                hostio.synth_stream(part, None, 1002, n, NAMES, LENS, level=1)
                row = dict(compressed_mb=mb, reads=n, compressed_bytes=os.path.getsize(part), parent=[], card=[])
                for rep in range(3):
                    row["parent"].append(run(old_exe, part, fa, os.path.join(tmp, "hp.bamqc"), {}, tmp, True, 120)[0])
                    row["card"].append(run(new_exe, part, fa, os.path.join(tmp, "hc.bamqc"), {"BQC_GPU_DECODE": "1"}, tmp, True, 120)[0])
                assert open(os.path.join(tmp, "hp.bamqc"), "rb").read() == open(os.path.join(tmp, "hc.bamqc"), "rb").read(), "outputs differ at %d MB" % mb
                print("%3d MB: parent %s, card %s" % (mb, ["%.3f" % x for x in row["parent"]], ["%.3f" % x for x in row["card"]]), flush=True)
                cross.append(row)
                os.unlink(part)
            res["crossing"] = cross
            res["crossing_what"] = "streams of the same generator and seed with as many reads as make 16 / 64 / 256 MB at level 1 (a head of the 10 M-read stream cut at a byte count would end inside a record)"
            t_mb = None  # the smallest size from which (and above which) the card is not slower
            for r in reversed(cross):
                if min(r["card"]) > min(r["parent"]):
                    break
                t_mb = r["compressed_mb"]
            res["card_not_slower_from_mb"] = t_mb
        if not a.no_level0:
            os.unlink(bam)
            hostio.synth_stream(bam, None, 1002, a.reads, NAMES, LENS, level=0)
            head = open(bam, "rb").read(32)
            stored = (head[18] & 6) == 0  # BTYPE of the first member's first deflate block
            res["level0"] = dict(compressed_bytes=os.path.getsize(bam), stored_blocks=stored)
            print("level 0: %.0f MB, stored blocks: %s" % (os.path.getsize(bam) / 1e6, stored), flush=True)
            subprocess.run(["cat", bam], stdout=subprocess.DEVNULL)
            res["stream_level0"] = ab("stream, level 0", old_exe, new_exe, bam, fa, tmp, a.reads, True, {})
    if not a.no_bench:  # parent, new, parent, new
        runs = [(who, bench_once(tree)) for who, tree in (("parent", a.parent), ("new", ROOT)) * 2]
        res["bench"] = [dict(build=who, line=line) for who, line in runs]
        for who, line in runs:
            print("bench %s: %s" % (who, json.dumps(line)[:300]), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)
    print("wrote", a.out)


main()
