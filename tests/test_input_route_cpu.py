"""CPU: which reader takes an input ("which reader takes it").  bqc_input_route (host/input_route.h) is a pure function of
the facts; it is asked here over the full product of them and compared with the table of that section, written down again below as a dict
keyed by (caller, kind of source) with the conditions as small lambdas — from the document, not from the C++.  Then one pin per difference
between the callers that the section lists as found and kept, and per switch-over constant on both sides.  No I/O, no GPU call."""
import ctypes as C
import itertools

import pytest

from bamqc_amd import _abi, _lib

PROGRAM, LIB_CARD, LIB_HOST = 0, 1, 2
STDIN, SAM, SAM_BGZF, STREAM, BAM, OTHER = range(6)
UNSET, OFF, ON = 0, 1, 2
NEITHER, C_BAM, C_TEXT = 0, 1, 2
NO, STDIN_SHARD, SAM_SHARD, EMPTY_SHARD = 0, 1, 2, 3
SNIFF_NO, SNIFF_FD, SNIFF_STDIO = 0, 1, 2
HDR_BAM, HDR_SAM_STDIO, HDR_SAM_BGZF, HDR_GSAM = 0, 1, 2, 3
FILE, RANGE, STREAM_SRC = 0, 1, 2
RD_BAM, RD_SAM_STDIO, RD_SAM_BGZF, RD_GSAM_MEMORY, RD_GPU_BAM, RD_GPU_SAM, RD_GPU_SAM_BGZF = range(7)

BAM_FROM, SAM_FROM, SAM_BGZF_FROM = 256 << 20, 64 << 20, 22460726
SIZES = sorted({0, 1 << 40} | {k + d for k in (BAM_FROM, SAM_FROM, SAM_BGZF_FROM) for d in (-1, 0, 1)})
FIELDS = [n for n, _ in _abi.RouteFacts._fields_]


def route(**facts):
    f = _abi.RouteFacts(**facts)
    r = _abi.Route()
    _lib.load().bqc_input_route(C.byref(f), C.byref(r))
    return {n: getattr(r, n) for n, _ in _abi.Route._fields_}


# ---- the table of DESIGN section 4.5d -------------------------------------------------------------------------------------------------
def _source(f):
    """the row: what kind of source the facts describe"""
    if f["shard"]:
        return "shard"
    if f["kind"] == STDIN:
        stream = bool(f["dash_bgzf"])
    else:
        stream = f["kind"] == STREAM or (f["kind"] == SAM_BGZF and not f["regular"] and f["caller"] != LIB_HOST)
    if f["kind"] == SAM or (f["kind"] == STDIN and not stream):
        return "text"
    if f["kind"] == SAM_BGZF or (stream and f["carries"] == C_TEXT):
        return "bgzf text stream" if stream else "bgzf text file"
    return "bam stream" if stream else "bam file"


def _on(f):
    return f["gpu_decode"] == ON


def _not_off(f):
    return f["gpu_decode"] != OFF


def _first_pass(f):
    return not f["host_reader_only"]


def _stream_card(allowed):
    """a BGZF stream: the variable, an @RG line, and — variable unset — not ended within the hold"""
    return lambda f: allowed(f) and _not_off(f) and f["has_rg"] and (_on(f) or not f["ended"])


def _file_card(k):
    return lambda f: _first_pass(f) and _not_off(f) and f["regular"] and (_on(f) or f["size"] >= k) and f["has_rg"]


def _shard_card(f):
    return _first_pass(f) and _not_off(f) and f["regular"] and f["shard_found"] and (_on(f) or f["shard_bytes"] >= BAM_FROM) and f["has_rg"]


def _program_text(f):
    regular = f["kind"] == SAM and f["regular"]
    if not _not_off(f) or (regular and not _on(f) and f["size"] < SAM_FROM):
        return RD_SAM_STDIO
    return RD_GPU_SAM if f["has_rg"] and (_on(f) or not f["ended"]) else RD_GSAM_MEMORY


ALWAYS = lambda f: True  # noqa: E731
# (caller, source) -> (the reader on the card, the host's reader, when the card takes it)
TABLE = {
    (PROGRAM, "text"): None,  # three-way: _program_text
    (LIB_CARD, "text"): (RD_GPU_SAM, RD_SAM_STDIO, ALWAYS),
    (LIB_HOST, "text"): (RD_GPU_SAM, RD_SAM_STDIO, lambda f: False),
    (PROGRAM, "bgzf text stream"): (RD_GPU_SAM_BGZF, RD_SAM_BGZF, _stream_card(_first_pass)),
    (LIB_CARD, "bgzf text stream"): (RD_GPU_SAM_BGZF, RD_SAM_BGZF, _stream_card(ALWAYS)),
    (LIB_HOST, "bgzf text stream"): (RD_GPU_SAM_BGZF, RD_SAM_BGZF, lambda f: False),
    (PROGRAM, "bgzf text file"): (RD_GPU_SAM_BGZF, RD_SAM_BGZF, _file_card(SAM_BGZF_FROM)),
    (LIB_CARD, "bgzf text file"): (RD_GPU_SAM_BGZF, RD_SAM_BGZF, ALWAYS),
    (LIB_HOST, "bgzf text file"): (RD_GPU_SAM_BGZF, RD_SAM_BGZF, lambda f: False),
    (PROGRAM, "bam stream"): (RD_GPU_BAM, RD_BAM, _stream_card(_first_pass)),
    (LIB_CARD, "bam stream"): (RD_GPU_BAM, RD_BAM, _stream_card(ALWAYS)),
    (LIB_HOST, "bam stream"): (RD_GPU_BAM, RD_BAM, lambda f: False),
    (PROGRAM, "bam file"): (RD_GPU_BAM, RD_BAM, _file_card(BAM_FROM)),
    (LIB_CARD, "bam file"): (RD_GPU_BAM, RD_BAM, ALWAYS),
    (LIB_HOST, "bam file"): (RD_GPU_BAM, RD_BAM, lambda f: False),
    (PROGRAM, "shard"): (RD_GPU_BAM, RD_BAM, _shard_card),
    (LIB_CARD, "shard"): (RD_GPU_BAM, RD_BAM, ALWAYS),
    (LIB_HOST, "shard"): (RD_GPU_BAM, RD_BAM, lambda f: False),
}


def expect(f):
    """every field of the route the table gives for these facts"""
    caller, src = f["caller"], _source(f)
    r = dict(refuse=NO, sniff=SNIFF_NO, stream=0, find_blocks=0, header_by=HDR_BAM, header_first=0, hold=0, reader=RD_BAM, source=FILE)
    if src == "shard":
        if f["kind"] == STDIN and caller == PROGRAM:
            return dict(r, refuse=STDIN_SHARD)
        if f["kind"] in (SAM, SAM_BGZF) or (f["kind"] == STDIN and caller == LIB_CARD):
            return dict(r, refuse=SAM_SHARD)
        r["source"] = RANGE
        if caller == LIB_CARD:
            r.update(find_blocks=1, header_first=1, refuse=NO if f["shard_found"] else EMPTY_SHARD)
        if caller == PROGRAM:
            r["find_blocks"] = int(bool(_first_pass(f) and _not_off(f) and f["regular"]))
            r["header_first"] = int(bool(r["find_blocks"] and f["shard_found"] and (_on(f) or f["shard_bytes"] >= BAM_FROM)))
    else:
        if f["kind"] == STDIN:  # the first bytes through stdio where the host's SAM parser may read stdin
            r["sniff"] = SNIFF_STDIO if caller == LIB_HOST or (caller == PROGRAM and f["gpu_decode"] == OFF) else SNIFF_FD
        r["stream"] = int("stream" in src)
        r["source"] = STREAM_SRC if r["stream"] else FILE
    if src == "text" and caller == PROGRAM:
        r["reader"] = _program_text(f)
        if r["reader"] != RD_SAM_STDIO and not _on(f) and not (f["kind"] == SAM and f["regular"]):
            r["hold"] = SAM_FROM
    else:
        on_card, on_host, when = TABLE[(caller, src)]
        r["reader"] = on_card if when(f) else on_host
    if src == "text":
        r["header_by"] = HDR_SAM_STDIO if r["reader"] == RD_SAM_STDIO else HDR_GSAM
    if src.startswith("bgzf text"):
        r["header_by"] = HDR_SAM_BGZF
    if src.endswith("stream") and caller != LIB_HOST:  # held only where the card is still possible and the variable does not decide
        allowed = caller == LIB_CARD or _first_pass(f)
        if allowed and f["gpu_decode"] == UNSET and f["has_rg"]:
            r["hold"] = SAM_BGZF_FROM if src == "bgzf text stream" else BAM_FROM
    if src == "bam file":  # the small first run whenever the card will probably take the file
        r["header_first"] = int(caller == LIB_CARD or (caller == PROGRAM and bool(_file_card(BAM_FROM)(dict(f, has_rg=1)))))
    return r


def _rows():
    base = dict.fromkeys(FIELDS, 0)
    common = [dict(caller=c, gpu_decode=g, host_reader_only=h, has_rg=rg, ended=e)
              for c, g, h, rg, e in itertools.product((PROGRAM, LIB_CARD, LIB_HOST), (UNSET, OFF, ON), (0, 1), (0, 1), (0, 1))]
    files = [dict(regular=1, size=s) for s in SIZES] + [dict(regular=0, size=0)]
    per_kind = {STDIN: [dict(dash_bgzf=d, carries=c) for d in (0, 1) for c in (NEITHER, C_BAM, C_TEXT)],
                STREAM: [dict(carries=c) for c in (NEITHER, C_BAM, C_TEXT)],
                SAM: files, BAM: files, OTHER: files,
                SAM_BGZF: files + [dict(regular=0, carries=C_BAM)]}
    for kind, variants in per_kind.items():
        for c, v in itertools.product(common, variants):
            yield dict(base, kind=kind, **c, **v)
    shards = [dict(shard=1, regular=r, shard_found=sf, shard_bytes=sb) for r in (0, 1) for sf, sb in ((0, 0), (1, 1), (1, BAM_FROM - 1), (1, BAM_FROM), (1, 1 << 40))]
    for kind, c, v in itertools.product(per_kind, common, shards):
        yield dict(base, kind=kind, **c, **v)


def test_every_route_is_the_tables():
    n = 0
    for f in _rows():
        got, want = route(**f), expect(f)
        if want["refuse"] in (STDIN_SHARD, SAM_SHARD):  # nothing is opened: the other fields say nothing
            got = dict(want, refuse=got["refuse"])
        assert got == want, (f, got, want)
        n += 1
    assert n > 5000


def _facts(**kw):
    return dict(dict.fromkeys(FIELDS, 0), **kw)


def test_library_card_opener_takes_regular_files_whatever_size_variable_and_header():  # difference 1
    for kind, card in ((BAM, RD_GPU_BAM), (SAM_BGZF, RD_GPU_SAM_BGZF)):
        for g in (UNSET, OFF, ON):
            assert route(**_facts(caller=LIB_CARD, kind=kind, regular=1, size=1, gpu_decode=g, has_rg=0))["reader"] == card
        assert route(**_facts(caller=PROGRAM, kind=kind, regular=1, size=1, has_rg=1))["reader"] in (RD_BAM, RD_SAM_BGZF)
        assert route(**_facts(caller=PROGRAM, kind=kind, regular=1, size=1, gpu_decode=ON, has_rg=0))["reader"] in (RD_BAM, RD_SAM_BGZF)


def test_plain_sam_text_the_library_always_the_card_the_program_holds_or_takes_the_size():  # difference 2
    r = route(**_facts(caller=LIB_CARD, kind=SAM, gpu_decode=OFF, ended=1))
    assert (r["header_by"], r["hold"], r["reader"]) == (HDR_GSAM, 0, RD_GPU_SAM)
    r = route(**_facts(caller=PROGRAM, kind=STDIN, has_rg=1, ended=0))
    assert (r["hold"], r["reader"]) == (SAM_FROM, RD_GPU_SAM)
    assert route(**_facts(caller=PROGRAM, kind=STDIN, has_rg=1, ended=1))["reader"] == RD_GSAM_MEMORY
    assert route(**_facts(caller=PROGRAM, kind=STDIN, has_rg=0, ended=0))["reader"] == RD_GSAM_MEMORY
    assert route(**_facts(caller=PROGRAM, kind=STDIN, has_rg=1, ended=1, gpu_decode=ON))["reader"] == RD_GPU_SAM
    r = route(**_facts(caller=PROGRAM, kind=SAM, regular=1, size=SAM_FROM, has_rg=1))
    assert (r["hold"], r["reader"]) == (0, RD_GPU_SAM)


def test_the_variable_steers_the_library_for_streams_but_not_for_files():  # difference 3
    assert route(**_facts(caller=LIB_CARD, kind=STREAM, carries=C_BAM, gpu_decode=OFF, has_rg=1))["reader"] == RD_BAM
    assert route(**_facts(caller=LIB_CARD, kind=STREAM, carries=C_BAM, gpu_decode=ON, has_rg=1, ended=1))["reader"] == RD_GPU_BAM
    assert route(**_facts(caller=LIB_CARD, kind=BAM, regular=1, gpu_decode=OFF, has_rg=1))["reader"] == RD_GPU_BAM


def test_the_second_pass_does_not_apply_to_plain_sam_text():  # difference 4
    for h in (0, 1):
        assert route(**_facts(caller=PROGRAM, kind=SAM, regular=1, size=1, gpu_decode=ON, has_rg=1, host_reader_only=h))["reader"] == RD_GPU_SAM
    assert route(**_facts(caller=PROGRAM, kind=BAM, regular=1, gpu_decode=ON, has_rg=1, host_reader_only=1))["reader"] == RD_BAM
    assert route(**_facts(caller=PROGRAM, kind=SAM_BGZF, regular=1, gpu_decode=ON, has_rg=1, host_reader_only=1))["reader"] == RD_SAM_BGZF


def test_the_first_bytes_of_stdin_go_through_stdio_only_where_the_host_parser_reads_it():  # difference 5
    assert route(**_facts(caller=PROGRAM, kind=STDIN, gpu_decode=OFF))["sniff"] == SNIFF_STDIO
    assert route(**_facts(caller=PROGRAM, kind=STDIN, gpu_decode=UNSET))["sniff"] == SNIFF_FD
    assert route(**_facts(caller=PROGRAM, kind=STDIN, gpu_decode=ON))["sniff"] == SNIFF_FD
    assert route(**_facts(caller=LIB_CARD, kind=STDIN, gpu_decode=OFF))["sniff"] == SNIFF_FD
    assert route(**_facts(caller=LIB_HOST, kind=STDIN, gpu_decode=ON))["sniff"] == SNIFF_STDIO
    assert route(**_facts(caller=PROGRAM, kind=STREAM, gpu_decode=OFF))["sniff"] == SNIFF_NO


def test_what_a_failed_device_side_open_means_follows_from_the_route():  # difference 6: a file has a second pass, a stream and SAM text have none
    r = route(**_facts(caller=PROGRAM, kind=BAM, regular=1, gpu_decode=ON, has_rg=1))
    assert (r["reader"], r["stream"]) == (RD_GPU_BAM, 0)  # kUnsupported
    r = route(**_facts(caller=PROGRAM, kind=STREAM, carries=C_BAM, gpu_decode=ON, has_rg=1))
    assert (r["reader"], r["stream"]) == (RD_GPU_BAM, 1)  # BQC_ERR_DEVICE
    assert route(**_facts(caller=PROGRAM, kind=STDIN, gpu_decode=ON, has_rg=1))["reader"] == RD_GPU_SAM  # BQC_ERR_DEVICE


def test_shard_runs():  # difference 7
    assert route(**_facts(caller=PROGRAM, kind=STDIN, shard=1))["refuse"] == STDIN_SHARD
    for kind in (SAM, SAM_BGZF):
        for caller in (PROGRAM, LIB_CARD, LIB_HOST):
            assert route(**_facts(caller=caller, kind=kind, shard=1))["refuse"] == SAM_SHARD
    r = route(**_facts(caller=PROGRAM, kind=STREAM, shard=1, gpu_decode=ON, has_rg=1, carries=C_BAM))  # no regular file: the shard branch, the host reader
    assert (r["stream"], r["find_blocks"], r["reader"], r["source"]) == (0, 0, RD_BAM, RANGE)
    card = _facts(caller=PROGRAM, kind=BAM, shard=1, regular=1, shard_found=1, shard_bytes=BAM_FROM, has_rg=1)
    assert route(**card)["reader"] == RD_GPU_BAM and route(**card)["source"] == RANGE
    for change in (dict(regular=0), dict(shard_found=0, shard_bytes=0), dict(shard_bytes=BAM_FROM - 1), dict(has_rg=0), dict(gpu_decode=OFF), dict(host_reader_only=1)):
        r = route(**dict(card, **change))
        assert (r["reader"], r["source"]) == (RD_BAM, RANGE), change
    assert route(**dict(card, shard_bytes=1, gpu_decode=ON))["reader"] == RD_GPU_BAM
    r = route(**dict(card, has_rg=0))  # the header was read through the small first run: the host reader then opens the RANGE
    assert r["header_first"] == 1


def test_the_librarys_range_openers_differ_over_stdin_and_an_empty_shard():  # an eighth, as found
    assert route(**_facts(caller=LIB_CARD, kind=STDIN, shard=1))["refuse"] == SAM_SHARD
    assert route(**_facts(caller=LIB_HOST, kind=STDIN, shard=1))["refuse"] == NO
    assert route(**_facts(caller=LIB_CARD, kind=BAM, shard=1, regular=1, shard_found=0))["refuse"] == EMPTY_SHARD
    assert route(**_facts(caller=LIB_HOST, kind=BAM, shard=1, regular=1, shard_found=0))["refuse"] == NO
    r = route(**_facts(caller=LIB_HOST, kind=SAM_BGZF, regular=0))  # a FIFO named x.sam.gz: the host opener hands the path to the BGZF reader
    assert (r["stream"], r["reader"]) == (0, RD_SAM_BGZF)
    assert route(**_facts(caller=LIB_CARD, kind=SAM_BGZF, regular=0))["stream"] == 1


@pytest.mark.parametrize("name,k,facts_of", [
    ("BAM file", BAM_FROM, lambda s: _facts(caller=PROGRAM, kind=BAM, regular=1, size=s, has_rg=1)),
    ("shard", BAM_FROM, lambda s: _facts(caller=PROGRAM, kind=BAM, shard=1, regular=1, shard_found=1, shard_bytes=s, has_rg=1)),
    ("SAM file", SAM_FROM, lambda s: _facts(caller=PROGRAM, kind=SAM, regular=1, size=s, has_rg=1)),
    ("SAM.gz file", SAM_BGZF_FROM, lambda s: _facts(caller=PROGRAM, kind=SAM_BGZF, regular=1, size=s, has_rg=1)),
])
def test_each_constant_on_both_sides_for_sizes(name, k, facts_of):
    assert route(**facts_of(k - 1))["reader"] < RD_GPU_BAM, name
    assert route(**facts_of(k))["reader"] >= RD_GPU_BAM, name


def test_each_constant_is_the_hold_of_its_stream():
    assert route(**_facts(caller=PROGRAM, kind=STREAM, carries=C_BAM, has_rg=1))["hold"] == BAM_FROM == 268435456
    assert route(**_facts(caller=PROGRAM, kind=STREAM, carries=C_TEXT, has_rg=1))["hold"] == SAM_BGZF_FROM
    assert route(**_facts(caller=PROGRAM, kind=SAM_BGZF, regular=0, has_rg=1))["hold"] == SAM_BGZF_FROM
    assert route(**_facts(caller=PROGRAM, kind=STDIN))["hold"] == SAM_FROM == 67108864
    assert route(**_facts(caller=PROGRAM, kind=SAM, regular=0))["hold"] == SAM_FROM
