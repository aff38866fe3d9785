"""Test helper: SAM text inside BGZF — compressed here with tests/pybam.py's member writer, so that the member cuts are
the test's to place — and read as a file named *.sam.gz, on a child's stdin, through a FIFO or /dev/stdin, by `hostio.BamFile` on the host
or on a card.  Every read of a stream happens in a child process under a time limit, as tests/bam_stream_util.py does it.
(TEST INFRASTRUCTURE.)"""
import os
import subprocess
import sys

import numpy as np

from tests import pybam
from tests.bam_stream_util import ROOT, TIMEOUT, through_fifo

EOF_MEMBER = pybam._bgzf_block(b"")

# argv: path, batch_reads, "host" or a device index, the .npz to write, the repository root.  An error while reading is reported, with what
# was delivered in front of it; a failure to open is exit status 3.
CHILD = r'''
import sys
sys.path.insert(0, sys.argv[5])
import numpy as np
from bamqc_amd import hostio
path, batch_reads, gpu, out = sys.argv[1], int(sys.argv[2]), sys.argv[3], sys.argv[4]
try:
    b = hostio.BamFile(path) if gpu == "host" else hostio.BamFile(path, gpu=int(gpu))
except IOError as e:
    print("open_error=%s" % e)
    sys.exit(3)
cols, n, base, err = {}, 0, 0, None
try:
    for batch in b.batches(batch_reads):
        n += 1
        for k, v in batch.items():
            cols.setdefault(k, []).append(np.array(v, copy=True) + (base if k == "nm_extra_read" else 0))
        base += len(batch["flag"])
except IOError as e:
    err = str(e)
np.savez(out, **{k: np.concatenate(v) for k, v in cols.items()})
print("batches=%d handed_over=%d on_card=%r lanes=%r error=%s" % (n, b.batches_handed_over, b.on_card, b.lanes(), err))
b.close()
'''


def members(data, sizes, level=1, empty_between=False, eof=True):
    """`data` as BGZF: payloads of the sizes the iterator gives (its last value is repeated), an empty member behind each when asked,
    the EOF marker member at the end unless not.  Returns (bytes, [compressed size of each member that has a payload])."""
    out, csizes, at, it, size = [], [], 0, iter(sizes), 1
    while at < len(data):
        size = next(it, size)
        m = pybam._bgzf_block(data[at:at + size], level)
        out.append(m); csizes.append(len(m))
        if empty_between:
            out.append(EOF_MEMBER)
        at += size
    if eof:
        out.append(EOF_MEMBER)
    return b"".join(out), csizes


def cut_at(data, cuts, level=1, limit=0xff00):
    """`data` as BGZF with a member boundary at every offset of `cuts` (and at most `limit` bytes in a member)."""
    edges = sorted(set(c for c in cuts if 0 < c < len(data)) | {0, len(data)})
    out = []
    for a, b in zip(edges, edges[1:]):
        for x in range(a, b, limit):
            out.append(pybam._bgzf_block(data[x:min(b, x + limit)], level))
    return b"".join(out) + EOF_MEMBER


def read(tmp, data, how, batch_reads, gpu="host", env=None):
    """What `hostio.BamFile` gives for the bytes `data`, read in a child: how = "file" (named *.sam.gz), "-", "/dev/stdin", "fifo.sam.gz" (a
    FIFO of that name) or "fifo" (a FIFO without an extension).  Returns (columns, the child's report line, its exit status)."""
    tmp = str(tmp)
    out = os.path.join(tmp, "cols_%d.npz" % len(os.listdir(tmp)))
    e = dict(os.environ, **(env or {}))

    def child(path, **kw):
        r = subprocess.run([sys.executable, "-c", CHILD, path, str(batch_reads), str(gpu), out, ROOT], capture_output=True, env=e, timeout=TIMEOUT, **kw)
        assert r.returncode in (0, 3), (how, r.returncode, r.stderr.decode()[-2000:])
        return r.stdout.decode(), r.returncode

    if how in ("-", "/dev/stdin"):
        report, rc = child(how, input=data)
    elif how.startswith("fifo"):
        fifo = os.path.join(tmp, "s_%d%s" % (len(os.listdir(tmp)), how[4:]))
        report, rc = through_fifo(fifo, data, lambda: child(fifo, stdin=subprocess.DEVNULL))
    else:
        path = os.path.join(tmp, "f_%d.sam.gz" % len(os.listdir(tmp)))
        with open(path, "wb") as f:
            f.write(data)
        report, rc = child(path, stdin=subprocess.DEVNULL)
        os.unlink(path)
    cols = {}
    if rc == 0:
        with np.load(out) as z:
            cols = {k: z[k] for k in z.files}
        os.unlink(out)
    return cols, report, rc


def error_of(report):
    """the error the child met while reading (None: none), or the one it failed to open with"""
    if report.startswith("open_error="):
        return report[len("open_error="):].strip()
    msg = report.rsplit(" error=", 1)[1].strip()
    return None if msg == "None" else msg
