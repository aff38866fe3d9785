// input_route.h — what an input is, and which reader takes it ("which reader takes it"): the one statement of both,
// for the option parser, bqc_bam_open* and run_program (driver.cpp: InputOpener carries a route out).  Host only: no HIP header, no I/O
// beyond input_kind's one stat, no getenv beyond gpu_decode_env.
#pragma once
#include <cstdint>

// What an input is, by its name:
//   IN_STDIN     "-": SAM text, unless its first two bytes are a gzip member's — then a BGZF stream
//   IN_SAM       a path that ends in ".sam", whatever it is (a FIFO too): plain SAM text
//   IN_SAM_BGZF  a path that ends in ".sam.gz", whatever it is: SAM text inside BGZF (bgzip, samtools view -O sam,level=N); plain gzip is not read
//   IN_STREAM    any other path that is no regular file (a FIFO, /dev/stdin, /dev/fd/N): a BGZF stream
//   IN_BAM       any other path that ends in ".bam": a BAM file, no look at its content
//   IN_OTHER     anything else: the program's parser refuses the name; the library opens it as a BAM file
// A BGZF stream is BAM or SAM text by its first inflated bytes (host/bgzf.h: bgzf_stream_carries).
enum InputKind { IN_STDIN, IN_SAM, IN_SAM_BGZF, IN_STREAM, IN_BAM, IN_OTHER };
// regular / size (optional): what the one stat of the path says — a regular file, and its bytes
InputKind input_kind(const char* path, bool* regular = nullptr, uint64_t* size = nullptr);

// Where the card takes over when BQC_GPU_DECODE is unset (compressed bytes, or bytes of text); below, the host reader.
// BAM streams, BAM files and the block range of a shard.  Measured for streams (profiles/bam_stream_ab.json): whole-program
// time, host reader against the card, at 16 / 64 / 256 MB — the card is slower at 16, ties at 64 (0.231 against 0.226 s) and is not slower
// from 256 MB on (0.21 against 0.27 s); a file's reader on the card costs ~50 ms of set-up.
static const uint64_t kBamStreamCardFrom = 256ull << 20;
// Plain SAM text.  Measured for stdin (profiles/sam_reader_ab.json) at 1 / 4 / 16 / 64 MB of text: the card is not slower from
// 64 MB on (0.19 against 0.29 s).  A regular x.sam is held against the same constant by its size — measured for streams, not for files.
static const uint64_t kSamCardFrom = 64ull << 20;
// SAM text inside BGZF, stream or file.  Measured (profiles/sam_bgzf_ab.json): this build's host reader against the card forced,
// FIFOs of 22.5 / 85.2 / 276.0 MB, best of three — 0.274 against 0.194 s, 0.974 against 0.177 s, 3.33 against 0.221 s: the card is not slower at
// the smallest size measured, which is the constant (there the verdict rests on ONE of the card's three runs; from 85 MB on every card run is
// below every host run).  A switch-over point, no statement about speed; nothing smaller was measured, and files were not.
static const uint64_t kSamBgzfCardFrom = 22460726;

// BQC_GPU_DECODE: unset; off when atoi gives 0 (non-numeric text too); on
enum GpuDecode { GD_UNSET, GD_OFF, GD_ON };
GpuDecode gpu_decode_env();

enum RouteCaller { CALLER_PROGRAM, CALLER_LIB_CARD, CALLER_LIB_HOST }; // run_program; bqc_bam_open_gpu*; bqc_bam_open / bqc_bam_open_range
enum RouteCarries { CARRIES_NEITHER, CARRIES_BAM, CARRIES_SAM_TEXT };  // (the values of BgzfCarries)
// Everything the choice depends on.  A caller fills in what it knows so far and asks again when it knows more: what route() answers about
// an earlier step does not change with a later fact.
struct bqc_route_facts {
    int32_t caller;           // RouteCaller
    int32_t kind;             // InputKind
    int32_t regular;          // the path is a regular file ...
    uint64_t size;            // ... of this many bytes
    int32_t dash_bgzf;        // "-": its first two bytes are 1f 8b
    int32_t carries;          // a BGZF stream not named x.sam.gz: RouteCarries
    int32_t gpu_decode;       // GpuDecode
    int32_t host_reader_only; // the program's second pass (GpuBamReader::kUnsupported)
    int32_t shard;            // one process's part of the file
    int32_t shard_found;      // shard_blocks found a block range that is not empty ...
    uint64_t shard_bytes;     // ... of this many compressed bytes
    int32_t has_rg;           // after the header: lane_count != 0
    int32_t ended;            // after the hold: the stream ended inside what has been read
};
enum RouteRefuse { REFUSE_NO, REFUSE_STDIN_SHARD, REFUSE_SAM_SHARD, REFUSE_EMPTY_SHARD };
enum RouteSniff { SNIFF_NO, SNIFF_FD, SNIFF_STDIO }; // "-": its first bytes from descriptor 0 (handed on with preload), or through stdio (ungetc)
enum RouteHeader { HDR_BAM, HDR_SAM_STDIO, HDR_SAM_BGZF, HDR_GSAM }; // BamReader; SamReader on FILE*; SamReader over BGZF; GpuSamReader::start
enum RouteSource { SRC_FILE, SRC_RANGE, SRC_STREAM };
enum RouteReader { RD_BAM, RD_SAM_STDIO, RD_SAM_BGZF, RD_GSAM_MEMORY, RD_GPU_BAM, RD_GPU_SAM, RD_GPU_SAM_BGZF };
struct bqc_route {
    int32_t refuse;       // RouteRefuse: nothing is opened (REFUSE_EMPTY_SHARD: once shard_found is known)
    int32_t sniff;        // RouteSniff (needs caller, kind, gpu_decode)
    int32_t stream;       // a BGZF stream object over the descriptor (needs dash_bgzf)
    int32_t find_blocks;  // a shard the card may take: shard_blocks is asked (a regular file, or the library's card opener)
    int32_t header_by;    // RouteHeader (needs carries, shard_found)
    int32_t header_first; // BamReader::open: the small first run — the card will probably take the input; a shard without it is opened as a range at once
    uint64_t hold;        // bytes to hold before the choice: plain text before the header (GpuSamReader::start), a BGZF stream behind it (needs has_rg)
    int32_t reader;       // RouteReader (needs has_rg, ended) ...
    int32_t source;       // ... over RouteSource
};
extern "C" void bqc_input_route(const bqc_route_facts* facts, bqc_route* route); // (exported for tests/test_input_route_cpu.py)
inline bqc_route input_route(const bqc_route_facts& f) { bqc_route r; bqc_input_route(&f, &r); return r; }
inline bool route_on_card(const bqc_route& r) { return r.reader >= RD_GPU_BAM; }
inline bool route_gpu_sam(const bqc_route& r) { return r.reader == RD_GPU_SAM || r.reader == RD_GPU_SAM_BGZF; }
inline bool route_any_gsam(const bqc_route& r) { return r.reader == RD_GSAM_MEMORY || route_gpu_sam(r); }
