"""Test helper: BAM bytes as a STREAM — on a child's stdin or through a FIFO — read by `hostio.BamFile` or by
the program.  Every read of a stream happens in a child process under a time limit: a reader that opens a FIFO a second time
blocks, and a test must fail rather than wait.  (TEST INFRASTRUCTURE.)"""
import os
import subprocess
import sys
import threading

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "bin", "bamqualcheck")
TIMEOUT = 120

# argv: path ("-", a FIFO, a file), batch_reads, "host" or a device index, the .npz to write
READER = r'''
import sys
sys.path.insert(0, sys.argv[5])
import numpy as np
from bamqc_amd import hostio
path, batch_reads, gpu, out = sys.argv[1], int(sys.argv[2]), sys.argv[3], sys.argv[4]
b = hostio.BamFile(path) if gpu == "host" else hostio.BamFile(path, gpu=int(gpu))
cols, n = {}, 0
for batch in b.batches(batch_reads):
    n += 1
    for k, v in batch.items():
        cols.setdefault(k, []).append(np.array(v, copy=True))
np.savez(out, **{k: np.concatenate(v) for k, v in cols.items()})
print("batches=%d handed_over=%d on_card=%r lanes=%r" % (n, b.batches_handed_over, b.on_card, b.lanes()))
b.close()
'''


def through_fifo(fifo, data, run_child):
    """`data` into the FIFO from a daemon thread while run_child() (a subprocess call with a time limit) reads it; the writer is
    not waited for beyond the child: a child that never opened the FIFO leaves it blocked in open(), which is released here."""
    if os.path.exists(fifo):
        os.unlink(fifo)
    os.mkfifo(fifo)
    state = {}

    def write():
        try:
            with open(fifo, "wb") as f:
                f.write(data)
        except BrokenPipeError:  # (the reader stopped early: a damaged stream)
            state["epipe"] = True
        except Exception as e:
            state["error"] = e

    th = threading.Thread(target=write, daemon=True)
    th.start()
    try:
        return run_child()
    finally:
        th.join(timeout=5)
        if th.is_alive():  # (blocked in open: nobody read)
            fd = os.open(fifo, os.O_RDONLY | os.O_NONBLOCK)
            th.join(timeout=5)
            os.close(fd)
        os.unlink(fifo)
        assert "error" not in state, state


def read_columns(tmp, data, how, batch_reads, gpu="host", env=None):
    """The columns `hostio.BamFile` gives for the bytes `data`, read in a child: how = "-" (stdin), "/dev/stdin", "fifo" (named *.bam), "fifo.sam" (named *.sam) or "file".
    Returns (columns, the child's report line)."""
    out = os.path.join(tmp, "cols_%d.npz" % len(os.listdir(tmp)))
    e = dict(os.environ, **(env or {}))

    def child(path, **kw):
        r = subprocess.run([sys.executable, "-c", READER, path, str(batch_reads), str(gpu), out, ROOT], capture_output=True, env=e, timeout=TIMEOUT, **kw)
        assert r.returncode == 0, (how, r.stderr.decode()[-2000:])
        return r.stdout.decode()

    if how in ("-", "/dev/stdin"):
        report = child(how, input=data)
    elif how in ("fifo", "fifo.sam"):
        fifo = os.path.join(tmp, "s_%d.%s" % (len(os.listdir(tmp)), "sam" if how == "fifo.sam" else "bam"))
        report = through_fifo(fifo, data, lambda: child(fifo, stdin=subprocess.DEVNULL))
    else:
        path = os.path.join(tmp, "f_%d.bam" % len(os.listdir(tmp)))
        with open(path, "wb") as f:
            f.write(data)
        report = child(path, stdin=subprocess.DEVNULL)
    with np.load(out) as z:
        cols = {k: z[k] for k in z.files}
    os.unlink(out)
    return cols, report


def same(a, b):
    assert a.keys() == b.keys(), (sorted(a), sorted(b))
    for k in a:
        assert len(a[k]) == len(b[k]), k
        assert np.array_equal(a[k], b[k]), k


def program(args, data=None, fifo=None, env=None):
    """bin/bamqualcheck under a time limit: `data` on its stdin, or written into `fifo` (then the input path of args).  The completed process (text)."""
    e = dict(os.environ, BQC_TIMING="1")
    for k, v in (env or {}).items():  # (None: the variable is taken out of the child's environment)
        if v is None:
            e.pop(k, None)
        else:
            e[k] = v
    if fifo is not None:
        return through_fifo(fifo, data, lambda: subprocess.run([EXE] + list(args), stdin=subprocess.DEVNULL, capture_output=True, env=e, timeout=TIMEOUT))
    return subprocess.run([EXE] + list(args), input=data, capture_output=True, env=e, timeout=TIMEOUT)
