// gpu_bam.h — BAM input decoded on the GPU (gpu_bam.hip): the compressed file goes to the card, the inflated bytes never come
// back.  Same interface as the host reader (host/bam_io.h: RecordReader), same columns: the fixed ones arrive in the batch's
// host arrays (the host pass of the aggregation needs them), the payload (bases, qualities, CIGARs) stays in device memory
// (HostBatch::d_seq / d_qual / d_cigar — bqc_submit_async copies from wherever the columns live).
#pragma once
#include <atomic>
#include <cstdint>
#include <string>
#include <vector>

#include <hip/hip_runtime_api.h>

#include "../host/bam_io.h"

class GpuBamReader : public RecordReader {
public:
    // err_code of next_batch when this input needs the host reader instead (a record walk that cannot be verified, a corrupt
    // record, a file that ends inside a record): nothing has been reported to the user, the caller starts over with BamReader, which
    // decides what is an error and what is not.  A BATCH with a record the card does not decode (a read group that is not in the
    // header, a second NM tag, no RG tag, ...) is not such a case: that batch is decoded by the host reader's rules
    // (bam_decode_records) from the bytes on the card, and the run continues.
    static const int kUnsupported = -1000;
    GpuBamReader();
    ~GpuBamReader() override;
    // hdr / first_record_u: the header as the host reader parsed it, and the offset of the first record in the uncompressed stream
    // batch_reads / batch_bases: the limits next_batch will be called with (buffers are allocated once, for full batches)
    bool open(const char* path, int device, const BamHeader& hdr, uint64_t first_record_u, size_t batch_reads, size_t batch_bases, std::string& err);
    // One shard of the record stream (multi-GPU; same meaning as BamReader::open_range, host/bam_io.h): call before open().  Only the
    // bytes of the compressed file from `begin_block` on are read (a BGZF block boundary: bgzf_find_block), and the records taken
    // are those that START before the block at `end_block` (UINT64_MAX: to the end of the file); the last one runs on into the
    // successor's blocks.  begin_block 0: from the first record (first_record_u of open()); otherwise the first record is located
    // by the walk's own guess (three records in a row that look like records) — neighbouring shards verify it afterwards:
    // range_over() of a shard must equal range_first() of its successor.
    void set_range(uint64_t begin_block, uint64_t end_block) { range_b0_ = begin_block; range_b1_ = end_block; ranged_ = true; }
    // A STREAM instead of a file (a pipe, a FIFO, stdin: DESIGN section 4.5c): call before open(), whose path is then not opened.  `fd`
    // is read once, in order, by one reader thread and is the reader's from here on (closed with the file unless it is 0); `prefix`
    // is every byte that has left it so far, from the stream's first one — the header's, and what was held while the runtime started —
    // and is the input of the first run or runs: it arrives by move and is not read again; `ended`: the descriptor has reported its
    // end.  A stream is never ranged, and next_batch never answers kUnsupported for one: there is no second pass over a stream.
    void set_stream(int fd, raw_vector<uint8_t>&& prefix, bool ended) { stream_fd_ = fd; stream_prefix_ = std::move(prefix); stream_ended_ = ended; stream_set_ = true; }
    uint64_t range_first() const { return range_first_; } // uncompressed offset of the shard's first record, relative to its begin block (valid after the first batch)
    uint64_t range_over() const { return range_over_; }   // where the record after the shard's last one starts, relative to the end block (valid after the last batch)
    // The file is read and copied to the card from open() on; the first inflate kernel waits for this call: a caller that still has
    // device set-up of its own to do (allocations, synchronous copies wait for a running kernel) makes it when that is done.
    void allow_kernels();
    BamHeader& header() override { return hdr_; }
    void set_main_chrom(const std::vector<uint8_t>& mc) override { main_ = mc; }
    int next_batch(HostBatch& out, size_t max_reads, size_t max_bases, std::string& err, int& err_code) override;
    uint64_t records() const { return nrec_; }
    uint64_t batches_handed_over() const { return n_handed_over_; } // batches decoded by the host reader's rules (see next_batch)
    // The program's context, once it exists: from then on the batches' coverage anchors are made on the card (include/bamqc.h:
    // bqc_anchor_*) and their fixed columns stay there — HostBatch::anchored — as long as the stream allows it (one read group, not a
    // shard in the middle of a stream, no batch handed over to the host decoder so far).  Without it: columns on the host, as ever.
    void set_anchor_context(bqc_ctx* ctx) { anchor_ctx_ = ctx; }
    uint64_t batches_anchored() const { return n_anchored_; }
    uint64_t batches() const { return n_batches_; } // batches of records the card has decoded (those handed over to the host decoder included)
    double seconds_reading() const { return t_read_; } // time spent in pread, summed over the reader threads (a stream: in read() and waiting for the pipe, one thread)
    double seconds_waiting_for_runs() const { return t_wait_run_; } // time the consumer waited for the next inflated run (file, copy or inflate behind)
    double seconds_producer_waiting_for_chunks() const { return t_wait_chunk_; } // time the producer waited for the ring's reader threads
    // set by open() once its device buffers are allocated (also when it fails before that): a caller that creates its own device
    // context in another thread starts doing so from here on
    std::atomic<bool> buffers_allocated{false};
    // One process, many files.  open() on a reader that has been open before keeps every buffer that is large enough (streams, events,
    // status words, the page-locked chunk ring, run / walk / column buffers, the batches' payload pool) and grows the others; nothing
    // shrinks; ranges, counters, lane tables and the anchor state start fresh.  end_file(): the file is over (or given up) — the
    // reader's threads end, its streams are waited for, the file is closed; call it before the next open() needs the card quiet and
    // before the two questions below.
    void end_file();
    void memory_held(size_t& device_bytes, size_t& pinned_bytes); // what the reader (and the batches' payload pool) holds now
    const char* buffers_report(); // "new": first open(); "kept": opened again and nothing had to grow since; "grown"
    // The PRODUCER alone, for BGZF that carries something other than BAM records (SAM text: gpu_sam.hip): the file or
    // stream (set_stream) is read, copied, inflated and CRC-checked run by run exactly as for next_batch — the same threads, ring,
    // buffers and kernel launches — and the caller consumes the inflated bytes itself, on the card.  open_runs instead of open(): no walk,
    // column or batch buffers; the first `skip_u` inflated bytes are dropped (a header the host has parsed); `spare` bytes in front of
    // and behind every window may be read (not written) by the caller's kernels.
    bool open_runs(const char* path, int device, uint64_t skip_u, size_t spare, std::string& err);
    hipStream_t consumer_stream(); // the stream next_run queues on (the reader's; nullptr: none could be made): the caller's kernels go there too
    // The caller is done with the first `used` bytes of the window it has (none before the first call); the next run joins what is left:
    // 1: the window is [window, window + n) — what was left, then the run's bytes (n may be 0: an empty run) — and `last` says that no
    // run follows; 0: no more runs (the window it had is all there is); -1: err / err_code — the BGZF layer's words for a damaged or cut
    // stream (BQC_ERR_IO, as the host reader's), a device error, or more left over than the room in front of a run (max_left()).
    // Window offsets fit 32 bits: n < 4 GB, checked where the runs are sized.
    int next_run(size_t used, const uint8_t*& window, size_t& n, bool& last, std::string& err, int& err_code);
    size_t max_left() const;

private:
    struct Impl;
    Impl* p_ = nullptr;
    BamHeader hdr_;
    std::vector<uint8_t> main_;
    uint64_t nrec_ = 0, n_handed_over_ = 0, n_anchored_ = 0, n_batches_ = 0;
    std::atomic<bqc_ctx*> anchor_ctx_{nullptr};
    bool anchors_ok_ = true; // (decode thread)
    double t_read_ = 0, t_wait_run_ = 0, t_wait_chunk_ = 0;
    bool ranged_ = false;
    bool stream_set_ = false, stream_ended_ = false;
    int stream_fd_ = -1;
    raw_vector<uint8_t> stream_prefix_;
    bool reopened_ = false;
    bool runs_only_ = false; // open_runs
    size_t runs_spare_ = 64;
    size_t held_before_ = 0; // bytes held when open() took the buffers over
    uint64_t range_b0_ = 0, range_b1_ = UINT64_MAX, range_first_ = 0, range_over_ = 0;
};
