// gpu_sam.h — SAM text decoded on the GPU (gpu_sam.hip): the text goes to the card, and the card produces the batch the reader of BAM
// files produces (gpu_bam.h, gpu_batch.h): payload and — when anchored — fixed columns stay in device memory.  Same interface as the
// host reader (host/bam_io.h: SamReader), same columns, same messages: a batch with a line the card has no rule for is parsed by the
// host's own line parser (SamLineParser), which is also the one to decide what is an error.
#pragma once
#include <atomic>
#include <cstdint>
#include <map>
#include <string>
#include <vector>

#include <memory>

#include "../host/bam_io.h"
#include "gpu_bam.h"

class GpuSamReader : public RecordReader {
public:
    GpuSamReader();
    ~GpuSamReader() override;
    // The reader owns the descriptor from its first byte (closed with the reader unless it is 0).  Reads, in the calling thread, until
    // the header is complete and `hold_bytes` bytes or the end of the stream have been seen, and parses the header (no device needed).
    bool start(int fd, size_t hold_bytes, std::string& err);
    // (before start()) the descriptor's first bytes, read by a caller that had to look at them: "-" may carry BGZF, which is BAM
    void preload(const void* p, size_t n) { pre_.assign((const char*)p, (const char*)p + n); }
    // A second source (instead of start()): SAM text inside BGZF — x.sam.gz, or a stream that carries it.  The text arrives
    // ON the card, as the output of the BGZF producer of gpu_bam.hip (GpuBamReader::open_runs / next_run: its ring, runs, inflate
    // launches and CRC check, unchanged), and the window of next_batch is pointed at the inflated bytes: nothing is copied but the
    // unfinished last line of a run, which goes in front of the next run's bytes.  hdr / ref_index / first_record_u: the header as the
    // host reader parsed it (SamReader::open_bgzf*) and where the first record line starts in the text.  A stream: producer().set_stream(...)
    // before open(); a file: `path` is opened by the producer.  BGZF damage is the stream's I/O error, in the host reader's words.
    void start_bgzf(const BamHeader& hdr, const std::map<std::string, int32_t>& ref_index, uint64_t first_record_u, const char* path);
    GpuBamReader& producer() { return *bg_; }
    bool from_bgzf() const { return bg_ != nullptr; }
    double seconds_producer_reading() const;            // the producer's reader threads in pread / read()
    double seconds_producer_waiting_for_chunks() const; // the producer waiting for them
    double seconds_waiting_for_runs() const;            // next_batch waiting for an inflated run
    // after start(): the whole stream is in memory.  A caller may then leave open() out: next_batch parses on the host.
    bool stream_ended() const { return pre_eof_; }
    // the device side: buffers for batches of batch_reads / batch_bases, the reader thread over the rest of the stream
    bool open(int device, size_t batch_reads, size_t batch_bases, std::string& err);
    // the first kernel waits for this call (a caller that still has device set-up of its own to do makes it when that is done)
    void allow_kernels();
    bool on_card() const { return p_ != nullptr; }
    BamHeader& header() override { return hdr_; }
    void set_main_chrom(const std::vector<uint8_t>& mc) override { main_ = mc; }
    int next_batch(HostBatch& out, size_t max_reads, size_t max_bases, std::string& err, int& err_code) override;
    void set_anchor_context(bqc_ctx* ctx) { anchor_ctx_ = ctx; } // as GpuBamReader's: a stream is whole from its first batch
    uint64_t records() const { return nrec_; }
    uint64_t batches() const { return n_batches_; }                 // batches the card has taken (those handed over included)
    uint64_t batches_handed_over() const { return n_handed_over_; } // ... of which parsed by the host's line parser
    uint64_t batches_anchored() const { return n_anchored_; }
    double seconds_reading() const { return t_read_; }           // reader thread inside read()
    double seconds_waiting_for_input() const { return t_wait_in_; } // next_batch waiting for the reader thread
    double seconds_copying() const { return t_copy_; }           // text to the card
    double seconds_in_kernels() const { return t_kern_; }        // launches to status word, per batch

private:
    struct Impl;
    std::unique_ptr<GpuBamReader> bg_; // (start_bgzf) the producer of inflated text; outlives p_, whose stream is its
    std::string bg_path_;
    uint64_t bg_skip_ = 0;
    Impl* p_ = nullptr;
    int fd_ = -1;
    BamHeader hdr_;
    std::map<std::string, int32_t> ref_index_;
    std::vector<uint8_t> main_;
    std::vector<char> pre_; // what start() has read
    size_t pre_at_ = 0;     // the first byte behind the header
    bool pre_eof_ = false;
    std::string pending_err_; // an error behind records that have been delivered: the next call's answer
    int pending_code_ = 0;
    uint64_t nrec_ = 0, n_batches_ = 0, n_handed_over_ = 0, n_anchored_ = 0;
    std::atomic<bqc_ctx*> anchor_ctx_{nullptr};
    bool anchors_ok_ = true;
    double t_read_ = 0, t_wait_in_ = 0, t_copy_ = 0, t_kern_ = 0;
    // the lines of text[0, n) by the host's rules, up to max_reads / max_bases; `used`: bytes taken.  1 / 0 / -1 as next_batch.
    int host_lines(const char* text, size_t n, bool last_line_open, HostBatch& o, size_t max_reads, size_t max_bases, size_t& used, std::string& err, int& err_code);
};
