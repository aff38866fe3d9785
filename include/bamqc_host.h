/*
 * bamqc_host.h — host-side helpers that surround the aggregation path of bamqc.h:
 * the seeded synthetic-input generator, and (N2) the BGZF/BAM/FASTA readers and the
 * `bamqualcheck` driver that replace SeqAn's I/O (reference src/bamqualcheck.cpp:252-292,
 * 303-315; src/TripletCounting.hpp:71-104).  Plain C ABI, same conventions as bamqc.h.
 */
#ifndef BAMQC_HOST_H_
#define BAMQC_HOST_H_
#include "bamqc.h"
#ifdef __cplusplus
extern "C" {
#endif

/* ---- synthetic inputs ------------------------------------- */
typedef struct bqc_synth_params {
    uint64_t seed;
    uint64_t first_read_index; /* global index of read 0 (lets ranks draw disjoint streams) */
    uint32_t n_reads;
    uint32_t read_len;         /* 150 for the PE configs, 10000 for the long-read config    */
    uint32_t n_refs;
    const uint32_t* ref_len;
    uint32_t n_lanes;
    int32_t isize;
    int32_t long_reads;        /* 1: 20-60 CIGAR ops, indel/soft-clip heavy                 */
} bqc_synth_params;

/* Deterministic reference contig as Dna5 codes (uniform ACGT, 0.1 % N runs). */
int bqc_synth_reference(uint64_t seed, int32_t rid, uint64_t len, uint8_t* out);
/* Coordinate-sorted reads drawn from `refs` (may be NULL: random bases).  The returned batch and
 * its arrays are owned by the library; release with bqc_synth_batch_free. */
int bqc_synth_batch(const bqc_synth_params* p, const uint8_t* const* refs, bqc_batch** out);
void bqc_synth_batch_free(bqc_batch* b);
/* Reads [lo, lo + count) of the plan bqc_synth_batch would generate for p->n_reads reads (the same reads at the same
 * indices): lets a generator stream a plan that does not fit in memory.  Release with bqc_synth_batch_free. */
int bqc_synth_slice(const bqc_synth_params* p, uint64_t lo, uint32_t count, const uint8_t* const* refs, bqc_batch** out);

/* Writes a coordinate-sorted synthetic BAM (+ FASTA when fasta_path != NULL) for the parameters:
 * header with @SQ per contig and one @RG (ID:L<n>, SM:SYN) per lane; tags RG:Z, NM:i, AS:i. */
int bqc_synth_write(const bqc_synth_params* p, const char* const* ref_names, const char* bam_path, const char* fasta_path,
                    uint32_t batch_reads);

/* The same BAM, generated and written slice by slice (slice_reads reads in memory at a time; records serialised and BGZF
 * blocks compressed on all host threads; level 0 = stored blocks): for plans of hundreds of millions of reads.  bam_path
 * may be a FIFO that a reader drains meanwhile.  The FASTA is written first when fasta_path != NULL. */
int bqc_synth_stream(const bqc_synth_params* p, const char* const* ref_names, const char* bam_path, const char* fasta_path,
                     uint32_t slice_reads, int level);

/* Any batch as a BAM file with the header bqc_synth_write uses (@SQ per contig, @RG ID:L<n> SM:SYN per lane; read names
 * r<first_read_index + i>; tags RG:Z, NM:i, AS:i). */
int bqc_bam_write(const char* path, const bqc_batch* b, uint32_t n_refs, const char* const* ref_names, const uint32_t* ref_lens,
                  uint32_t n_lanes, uint64_t first_read_index, int level);

/* The same batch as SAM text, with the same header lines: one line per read, QNAME r<first_read_index + i>, PNEXT 0, RNEXT "=" on a
 * placed read, tags RG:Z, NM:i, AS:i; reads without qualities get QUAL "*". */
int bqc_sam_write(const char* path, const bqc_batch* b, uint32_t n_refs, const char* const* ref_names, const uint32_t* ref_lens,
                  uint32_t n_lanes, uint64_t first_read_index);

/* ---- BAM / FASTA input (replaces SeqAn BamStream / SequenceStream) --------- */
typedef struct bqc_bam bqc_bam;
/* What a path is, for this function, bqc_bam_open_gpu and the program alike (input_kind states it, host/input_route.h):
 *   - a path that ends in ".sam" is plain SAM text, whatever kind of file it is (a FIFO too: read once, as ever);
 *   - a path that ends in ".sam.gz" is SAM text inside BGZF (bgzip, samtools view -O sam,level=N), whatever kind of file it is; plain
 *     gzip — one serial DEFLATE stream without BGZF's BC subfield — is not read: it fails to open in the BGZF layer's words;
 *   - "-" (stdin) is plain SAM text unless its first two bytes are 1f 8b (a gzip member's: no SAM text starts with 0x1f);
 *   - "-" with those two bytes, and any other path that is not a regular file (a FIFO, /dev/stdin, /dev/fd/N), is a BGZF STREAM, read once
 *     and in order, and is what its first inflated bytes say (empty members in front skipped): "BAM\1" a BAM stream, a first byte of '@'
 *     SAM text inside BGZF, anything else or nothing "not a BAM file" — looked at inside the bytes the readers take anyway;
 *   - every other path is a BAM file, with no look at its content.
 * Here everything is read by the host readers.  SAM text inside BGZF gives the columns, lane names, messages and record numbers of the
 * same text read plain (a line may straddle any number of blocks); BGZF damage is the BGZF layer's I/O error, as for a BAM file.  A
 * stream that is no BAM, or ends inside its header, fails as a file does ("not a BAM file", "truncated BAM header", or the BGZF
 * layer's words). */
int bqc_bam_open(const char* path, bqc_bam** out);  /* on failure *out still holds the message */
/* One shard of the record stream (multi-GPU): the records that START in the BGZF blocks between the first block boundary at
 * or behind the compressed offset begin_hint and the first one at or behind end_hint (0 / UINT64_MAX: the file's ends).  A
 * shard in the middle of a file locates its first record by a plausibility test; shards verify each other afterwards:
 * bqc_bam_range_over of a shard must equal bqc_bam_range_first of its successor (else: process the file unsharded). */
int bqc_bam_open_range(const char* path, uint64_t begin_hint, uint64_t end_hint, bqc_bam** out);
/* The same reader with the file inflated and its records decoded on GPU `device` (the batches of bqc_bam_next are fetched back for
 * the caller).  A batch that holds a record the card does not decode (a read group missing from the header, a second NM tag, no
 * RG tag, ...) is decoded by the host reader's rules from the bytes on the card (bqc_bam_batches_handed_over counts them);
 * bqc_bam_next returns -1000 when the FILE needs the host reader (a record walk that cannot be verified, a corrupt record, a
 * file that ends inside a record): open it with bqc_bam_open then.
 * A path that ends in ".sam", and "-" (stdin), is SAM text and is decoded on the card as well (the reader takes the descriptor from
 * its first byte).  A stream cannot be started over, so -1000 never comes back for it: a batch with a line the card has no rule for
 * (bqc_bam_batches_handed_over counts them too) is parsed by the host's line parser, whose errors and messages are the ones reported;
 * the records in front of a failing line are delivered before its error.
 * SAM text inside BGZF (x.sam.gz, a FIFO of that name, a BGZF stream whose first inflated byte is '@') is inflated AND decoded on the card:
 * the header is parsed on the host, the BGZF producer of the reader of BAM files inflates the text run by run (CRC checked on the card),
 * and the reader of SAM text decodes it where it lies.  A file always goes to the card; a stream by the rules of a BAM stream below (with
 * 22.5 MB held instead of 256).  -1000 never comes back; BGZF damage is BQC_ERR_IO in the host reader's words, behind the records of the runs
 * in front of it; a line of 16 MB or more that crosses a run boundary is an I/O error of this reader (the room in front of a run).
 * A BAM STREAM (a path that is not a regular file and ends in neither ".sam" nor ".sam.gz"; "-" with the two bytes 1f 8b in front, looked at inside the bytes the reader takes
 * anyway) is read once, in order, and decoded on the card too: its header is parsed on the host from the stream's first bytes, which are
 * kept and become the card reader's first input.  BQC_GPU_DECODE=1 forces the card, =0 forbids it; unset, the calling thread holds the
 * stream's first 256 MB: a stream that ends inside them, and one without an @RG line, is read by the host reader from {those bytes, then
 * the descriptor}, and no device reader is set up.  -1000 never comes back for a stream either: where the card cannot vouch for the records
 * (a walk that cannot be verified, a corrupt record, a stream that ends inside a record) the records in front are delivered as a batch, and
 * the next call runs the host reader's own walk and decoder over the bytes from there (counted by bqc_bam_batches_handed_over): its records
 * are a batch, its error ("corrupt BAM record", "truncated BAM record", BQC_ERR_IO) is the answer, and where it only needs more bytes the card goes on. */
int bqc_bam_open_gpu(const char* path, int device, bqc_bam** out);
uint64_t bqc_bam_batches_handed_over(const bqc_bam* b);
int bqc_bam_on_card(const bqc_bam* b); /* 1: a reader on the card decodes this input; 0: a host reader (bqc_bam_open; a stream bqc_bam_open_gpu left to it) */
/* A shard (as bqc_bam_open_range) read, inflated and decoded on GPU `device`: only the shard's bytes of the file are touched.
 * SAM text, plain or inside BGZF (x.sam, x.sam.gz), has no shards: BQC_ERR_ARG, "SAM text cannot be read in shards" (bqc_bam_open_range too). */
int bqc_bam_open_gpu_range(const char* path, int device, uint64_t begin_hint, uint64_t end_hint, bqc_bam** out);
uint64_t bqc_bam_range_begin_block(const bqc_bam* b);
uint64_t bqc_bam_range_end_block(const bqc_bam* b);   /* UINT64_MAX: end of the file */
uint64_t bqc_bam_range_first(const bqc_bam* b);       /* valid after the first bqc_bam_next */
uint64_t bqc_bam_range_over(const bqc_bam* b);        /* valid after the last bqc_bam_next  */
uint64_t bqc_file_size(const char* path);
/* device >= 0: BAM readers inflate their BGZF blocks on that GPU from their next run of blocks on (the CRC-32 of every block is
 * still checked on the host; a card that cannot be used hands the work back to the CPU decoder); -1: on the CPU (the default). */
void bqc_gpu_inflate_device(int device);
uint64_t bqc_gpu_inflated_blocks(void);               /* BGZF blocks inflated on a GPU so far in this process */
void bqc_bam_close(bqc_bam* b);
const char* bqc_bam_error(const bqc_bam* b);
uint32_t bqc_bam_n_refs(const bqc_bam* b);
const char* bqc_bam_ref_name(const bqc_bam* b, uint32_t i);
uint32_t bqc_bam_ref_len(const bqc_bam* b, uint32_t i);
const char* bqc_bam_sample_id(const bqc_bam* b);      /* SM of the last @RG (bamqualcheck.cpp:58-61)        */
uint32_t bqc_bam_lane_count(const bqc_bam* b);        /* number of @RG IDs in the header                    */
uint32_t bqc_bam_n_lane_names(bqc_bam* b);            /* lane names in output (lexicographic) order,        */
const char* bqc_bam_lane_name(const bqc_bam* b, uint32_t i); /* including IDs first seen on a read (:86)  */
uint32_t bqc_bam_lane_index(const bqc_bam* b, uint32_t i);
int bqc_bam_set_main_chrom(bqc_bam* b, const uint8_t* main_chrom); /* [n_refs], for BQC_FLAG_MATE_MAIN  */
/* Keep only records whose refID is selected (refID -1 follows keep_unplaced): lets each rank of a
 * multi-GPU run take whole chromosomes of a coordinate-sorted BAM. */
int bqc_bam_set_rid_filter(bqc_bam* b, const uint8_t* keep, int keep_unplaced);
/* Next batch of decoded records: 1 = batch returned (owned by the reader until the next call),
 * 0 = end of file, < 0 = -(BQC_ERR_*) with the message in bqc_bam_error. */
int bqc_bam_next(bqc_bam* b, uint32_t max_reads, uint64_t max_bases, const bqc_batch** out);

/* Whole FASTA as Dna5 codes; ids cut at the first space/tab (TripletCounting.hpp:99-102). */
int bqc_fasta_load(const char* path, uint32_t* n_records, char*** names, uint8_t*** codes, uint64_t** lens);
void bqc_fasta_free(uint32_t n_records, char** names, uint8_t** codes, uint64_t* lens);

/* The sites file of --site-alleles (bqc_enable_site_alleles' list; no GPU is needed): text lines CONTIG<TAB>POS[<TAB>anything], POS
 * counted from 1 and the rest of the line ignored, so the body lines of a VCF are such lines.  Lines that start with '#' and empty
 * lines are skipped; "\r\n" is accepted.  The sites come back sorted by (index of the contig in ref_names, pos), pos counted from 0,
 * in arrays that bqc_sites_free releases.  A site on a contig that ref_names does not hold is left out and counted: *n_given is the
 * number of sites the file gives, *n_unnamed how many of them were left out (either pointer may be NULL).
 * BQC_ERR_IO, with "FILE: line N: reason" in err[err_cap] (err may be NULL): the file cannot be opened or read; a line without a
 * tab; a POS that is not a number of 1 or more; a POS behind the contig's length; a site given twice (the line of the second); no
 * site left (the file's last line). */
int bqc_sites_load(const char* path, const char* const* ref_names, const uint32_t* ref_lens, uint32_t n_refs, uint32_t* n_sites, int32_t** rid,
                   int32_t** pos, uint64_t* n_given, uint64_t* n_unnamed, char* err, uint64_t err_cap);
void bqc_sites_free(int32_t* rid, int32_t* pos);

/* The BED file of --regions (bqc_enable_region_coverage's list; no GPU is needed): text lines CONTIG<TAB>START<TAB>END[<TAB>anything],
 * START counted from 0, END exclusive, the rest of the line ignored.  Lines that start with '#', "track" and "browser" lines and
 * empty lines are skipped; "\r\n" is accepted; the order is free.  The regions come back sorted by (index of the contig in
 * ref_names, start), in arrays that bqc_regions_free releases.  Regions of one contig that overlap OR ABUT are merged into one:
 * *n_merged is the number of merges (regions given minus regions returned, among the named).  A region on a contig that ref_names
 * does not hold is left out and counted: *n_given is the number of regions the file gives, *n_unnamed how many of them were left out
 * (each of the three pointers may be NULL).
 * BQC_ERR_IO, with "FILE: line N: reason" in err[err_cap] (err may be NULL): the file cannot be opened or read; a line without its
 * two tabs; a START or END that is not a number; END <= START; an END behind the contig's length; no region left (the file's last
 * line). */
int bqc_regions_load(const char* path, const char* const* ref_names, const uint32_t* ref_lens, uint32_t n_refs, uint32_t* n_regions, int32_t** rid,
                     int32_t** start, int32_t** end, uint64_t* n_given, uint64_t* n_unnamed, uint64_t* n_merged, char* err, uint64_t err_cap);
void bqc_regions_free(int32_t* rid, int32_t* start, int32_t* end);

/* The BGZF reader's DEFLATE decoder on one raw deflate stream (host/inflate_fast.h; exposed for its tests): 1 when the
 * stream is valid, ends within in_n bytes and yields exactly out_n bytes, else 0.  The 8 bytes after in + in_n must be
 * readable (in a BGZF block: the CRC32 / ISIZE trailer). */
int bqc_inflate_raw(const uint8_t* in, uint64_t in_n, uint8_t* out, uint64_t out_n);
/* The reader's CRC-32 (gzip polynomial; host/crc32_fast.h), as zlib's crc32(0, p, n). */
uint32_t bqc_crc32(const uint8_t* p, uint64_t n);

/* Profiling aid: stream `bytes` of device memory `repeat` times with 4-byte-per-lane loads (kernel k_calib_read4),
 * used to calibrate the rocprofv3 FETCH_SIZE counter on a known byte count. */
int bqc_calib_read4(uint64_t bytes, int repeat);

/* ---- the program: drop-in for the reference's main() (bamqualcheck.cpp:239-457) ---- */
int bqc_main(int argc, const char** argv);

/* The program as one of shard_count processes (one per GPU) that split the BAM file's byte stream between them: this process
 * takes the records that start in its part of the compressed file (bqc_bam_open_range with hints i / n of the file size), its
 * context is a shard_tail context unless it is the first.  After its record loop it calls `hook` once — also when it failed,
 * so that all processes can agree — and the hook does what needs the other processes (launcher's business: torch.distributed
 * over RCCL in bamqc_amd/distributed.py): verify the split (range_over of a shard == range_first of its successor), hand the
 * coverage state down the chain (bqc_shard_export / bqc_shard_resolve), sum the state vectors onto the first process
 * (bqc_state_export / _import) and merge the lane names.  The hook returns BQC_SHARD_WRITE (this process finalises and writes
 * the output, with the lane names it put into `out`), BQC_SHARD_DONE (nothing more to do here), BQC_SHARD_FALLBACK (the split
 * could not be verified: this process runs the whole file again, unsharded) or BQC_SHARD_FAIL (exit status 1). */
typedef struct bqc_shard_info {
    bqc_ctx* ctx;                     /* NULL when the program failed before it was created                  */
    int32_t status;                   /* exit status so far: 0, or 1 after an error (message already printed) */
    uint64_t begin_block, end_block;  /* bqc_bam_range_*                                                      */
    uint64_t first, over;
    const char* sample_id;
    uint32_t n_lane_names;            /* lane names known to this process, incl. ids first seen on a read     */
    const char* const* lane_names;
    const uint32_t* lane_index;
} bqc_shard_info;
typedef struct bqc_shard_result {     /* filled by the hook for BQC_SHARD_WRITE: the merged lane names, output order */
    uint32_t n_lane_names;
    const char* const* lane_names;
    const uint32_t* lane_index;
} bqc_shard_result;
enum { BQC_SHARD_FAIL = 0, BQC_SHARD_DONE = 1, BQC_SHARD_FALLBACK = 2, BQC_SHARD_WRITE = 3 }; /* (0 — what a hook that died returns — never means "write") */
typedef int (*bqc_shard_hook)(void* user, const bqc_shard_info* info, bqc_shard_result* out);
int bqc_main_shard(int argc, const char** argv, uint32_t shard_index, uint32_t shard_count, bqc_shard_hook hook, void* user);

/* The program over n_gpus GPUs of one node as one binary (`bamqualcheck --gpus N`; reference: the single main() of
 * bamqualcheck.cpp:239-457): forks one worker per GPU — call it before anything in the process has touched a GPU — each of
 * which runs bqc_main_shard over its byte range of the BAM file; the shard hook is implemented in C++ over socket pairs for the
 * few words of agreement and the 8 KB coverage hand-over, and over librccl (loaded at run time) for the ONE reduce of the state
 * vectors: ncclReduce(uint64, sum) on device pointers.  BQC_REDUCE=pipe sums on the host instead (and so do workers that share
 * one card, BQC_GPUS_SHARE_DEVICE=1).  argv: the program's arguments (without --gpus).  Returns the exit status. */
int bqc_main_multi(int argc, const char** argv, int n_gpus);

/* The program's command line, parsed as bqc_main parses it (CommandLineParser.hpp:43-149) without running anything: 0 = valid
 * (the input path — a file name or "-" — is copied to input_path), 1 = usage error (message printed on stderr), 2 = -h /
 * --version answered on stdout.  bqc_main_multi calls it once before it forks its workers.
 * `--manifest LIST` (instead of the input and -o): the list is read and checked by the same rules — 0 with an EMPTY input_path for a
 * valid one, 1 for whatever is wrong with it (nothing on disk is touched either way). */
int bqc_program_args(int argc, const char** argv, char* input_path, uint64_t cap);

/* One process, many files (`bamqualcheck --manifest LIST` is a loop over these): a session owns what outlives a job — the HIP
 * runtime and its streams, the reference genome on the card (kept while the jobs name the same FASTA file and the same @SQ lines),
 * the context (kept — bqc_reset — while the options that size it stay the same; otherwise a new one takes the contigs over), the
 * reader's device and page-locked buffers (kept, grown where a file needs more, never shrunk).  Every job is a single run in all a
 * user can see: same messages, same exit status, byte-identical output file.
 * bqc_session_open: argv as the program's (argv[0] included), WITHOUT an input, -o and --manifest; 0, or 1 for a usage error
 * (message on stderr).  Nothing touches the card yet.
 * bqc_session_run: one job; returns its exit status (0 / 1).  After a job that failed on its INPUT the next one runs.  A HIP error
 * (BQC_ERR_DEVICE from any call) ends the session: that job returns 1, every later call 2 without starting anything on the card.
 * bqc_session_close: the one teardown.  One thread at a time; one session per process and device. */
typedef struct bqc_session bqc_session;
int bqc_session_open(int argc, const char** argv, bqc_session** out);
int bqc_session_run(bqc_session* session, const char* input, const char* output);
void bqc_session_close(bqc_session* session);

#ifdef __cplusplus
}
#endif
#endif
