// driver.cpp — the `bamqualcheck` program as a library function: drop-in for the reference's main()
// (src/bamqualcheck.cpp:239-457; its command line: host/program_options.h), with the
// record loop's body replaced by the GPU aggregation of include/bamqc.h.  Also: FASTA loader
// (replaces Genome / SequenceStream, src/TripletCounting.hpp:60-104) and the C wrappers of
// include/bamqc_host.h around the BAM reader.
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/prctl.h>
#include <sys/stat.h>
#include <unistd.h>
#include <zlib.h>

#include <atomic>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <functional>
#include <memory>
#include <mutex>
#include <string>
#include <chrono>
#include <thread>
#include <tuple>
#include <unordered_map>
#include <vector>

#include "../../include/bamqc_host.h"
#include "bam_io.h"
#include "raw_vector.h"
#include "parallel.h"
#include "crc32_fast.h"
#include "inflate_fast.h"
#include "host_tools.h"
#include "input_route.h"
#include "program_options.h"
#include "../csrc/gpu_bam.h"
#include "../csrc/gpu_sam.h"
#include <hip/hip_runtime_api.h>

// ---------------------------------------------------------------------------------------------------
// FASTA
// ---------------------------------------------------------------------------------------------------
struct FastaRecord { std::string name; raw_vector<uint8_t> codes; };

static inline uint8_t dna5_of_char(char c)
{
    switch (c) {
    case 'A': case 'a': return 0;
    case 'C': case 'c': return 1;
    case 'G': case 'g': return 2;
    case 'T': case 't': case 'U': case 'u': return 3;
    default: return 4;
    }
}

// An uncompressed FASTA file, mapped: where its records are (header lines found by all host threads: '>' outside a header line; a
// few thousand at most), and any record's sequence as Dna5 codes on demand — counted (bytes other than '\n' / '\r') and encoded
// chunk by chunk straight into the record's array by all host threads (a human genome is 3 GB of text: 2.2 s on one thread).
// The id is cut at the first space or tab (TripletCounting.hpp:99-102).  Same rules as the sequential loader below.
struct MappedFasta {
    struct Rec { std::string name; size_t lo, hi; }; // [lo, hi): the record's sequence lines in the file
    std::vector<Rec> recs;
    const char* m = nullptr;
    size_t size = 0;
    ~MappedFasta() { if (m) munmap((void*)m, size); }
    MappedFasta() = default;
    MappedFasta(const MappedFasta&) = delete;
    MappedFasta& operator=(const MappedFasta&) = delete;
    // 1: indexed, 0: not this kind of file (compressed, a pipe, empty)
    int open(const char* path)
    {
        const int fd = ::open(path, O_RDONLY);
        if (fd < 0) return 0;
        struct stat st;
        if (fstat(fd, &st) != 0 || !S_ISREG(st.st_mode) || st.st_size < 2) { close(fd); return 0; }
        size = (size_t)st.st_size;
        void* mp = mmap(nullptr, size, PROT_READ, MAP_PRIVATE, fd, 0);
        close(fd);
        if (mp == MAP_FAILED) { size = 0; return 0; }
        m = (const char*)mp;
        if ((uint8_t)m[0] == 0x1f && (uint8_t)m[1] == 0x8b) return 0; // gzip: the sequential loader inflates it
        (void)madvise(mp, size, MADV_WILLNEED);
        const unsigned nt = bqc_host_threads();
        // 1. every '>' of the file
        const size_t n_chunks = std::max<size_t>(1, std::min<size_t>((size + (1u << 20) - 1) >> 20, (size_t)nt * 4));
        std::vector<std::vector<size_t>> gts(n_chunks);
        parallel_ranges(n_chunks, nt, 1, [&](unsigned, size_t lo, size_t hi) {
            for (size_t c = lo; c < hi; ++c) {
                const char* p = m + size * c / n_chunks;
                const char* const e = m + size * (c + 1) / n_chunks;
                while (p < e) {
                    const char* g = (const char*)memchr(p, '>', (size_t)(e - p));
                    if (!g) break;
                    gts[c].push_back((size_t)(g - m));
                    p = g + 1;
                }
            }
        });
        // 2. those outside a header line start one; the line ends at the next '\n' (or with the file)
        struct Hdr { size_t gt, nl; };
        std::vector<Hdr> hdrs;
        size_t limit = 0;
        for (const auto& v : gts)
            for (size_t g : v) {
                if (g < limit) continue;
                const char* nl = (const char*)memchr(m + g, '\n', size - g);
                const size_t e = nl ? (size_t)(nl - m) : size;
                hdrs.push_back(Hdr{g, e});
                limit = e + 1;
            }
        recs.reserve(hdrs.size());
        for (size_t i = 0; i < hdrs.size(); ++i) {
            std::string hdr(m + hdrs[i].gt + 1, hdrs[i].nl - hdrs[i].gt - 1);
            const size_t cut = hdr.find_first_of(" \t");
            std::string name = hdr.substr(0, cut);
            if (!name.empty() && name.back() == '\r') name.pop_back();
            recs.push_back(Rec{name, std::min(size, hdrs[i].nl + 1), i + 1 < hdrs.size() ? hdrs[i + 1].gt : size});
        }
        return 1;
    }
    // the sequences of the records `which` (indices into recs), encoded together by all host threads; false: out of memory
    bool encode(const std::vector<size_t>& which, std::vector<raw_vector<uint8_t>*> const& out) const
    {
        const unsigned nt = bqc_host_threads();
        struct Task { size_t k, lo, hi, count, at; };
        std::vector<Task> tasks;
        const size_t kTask = 4u << 20;
        for (size_t k = 0; k < which.size(); ++k)
            for (size_t a = recs[which[k]].lo; a < recs[which[k]].hi; a += kTask) tasks.push_back(Task{k, a, std::min(recs[which[k]].hi, a + kTask), 0, 0});
        parallel_ranges(tasks.size(), nt, 1, [&](unsigned, size_t lo, size_t hi) {
            for (size_t t = lo; t < hi; ++t) {
                size_t n = 0;
                for (const char* q = m + tasks[t].lo; q < m + tasks[t].hi; ++q) n += (*q != '\n') & (*q != '\r');
                tasks[t].count = n;
            }
        });
        std::vector<size_t> total(which.size(), 0);
        for (auto& t : tasks) { t.at = total[t.k]; total[t.k] += t.count; }
        try {
            for (size_t k = 0; k < which.size(); ++k) { out[k]->clear(); if (total[k]) { out[k]->resize(total[k]); advise_huge(*out[k]); } }
        } catch (const std::bad_alloc&) { return false; }
        uint8_t lut[256];
        for (int i = 0; i < 256; ++i) lut[i] = dna5_of_char((char)i);
        parallel_ranges(tasks.size(), nt, 1, [&](unsigned, size_t lo, size_t hi) {
            for (size_t t = lo; t < hi; ++t) {
                uint8_t* w = out[tasks[t].k]->data() + tasks[t].at;
                const char* q = m + tasks[t].lo;
                const char* const hi_q = m + tasks[t].hi;
                while (q < hi_q) { // line by line: a run without '\n' is translated as a whole; a '\r' inside it (rare) takes the byte-wise path
                    const char* nl = (const char*)memchr(q, '\n', (size_t)(hi_q - q));
                    const char* const e = nl ? nl : hi_q;
                    const size_t n = (size_t)(e - q);
                    if (n && memchr(q, '\r', n)) {
                        for (size_t i = 0; i < n; ++i) if (q[i] != '\r') *w++ = lut[(uint8_t)q[i]];
                    } else {
                        for (size_t i = 0; i < n; ++i) w[i] = lut[(uint8_t)q[i]];
                        w += n;
                    }
                    q = e + 1;
                }
            }
        });
        return true;
    }
};

// Loads every record (`want`, optional, limits which sequences are kept in memory; all records keep their FASTA position) of a
// mapped file.  1: loaded, 0: not this kind of file (compressed, a pipe, empty), -1: error.
static int load_fasta_mapped(const char* path, const std::vector<std::string>* want, std::vector<FastaRecord>& out)
{
    MappedFasta mf;
    if (mf.open(path) != 1) return 0;
    out.clear();
    out.reserve(mf.recs.size());
    std::vector<size_t> which;
    for (size_t i = 0; i < mf.recs.size(); ++i) {
        bool keep = true;
        if (want) {
            keep = false;
            for (const auto& w : *want) if (w == mf.recs[i].name) { keep = true; break; }
        }
        out.push_back(FastaRecord{mf.recs[i].name, {}});
        if (keep) which.push_back(i);
    }
    std::vector<raw_vector<uint8_t>*> dst;
    for (size_t i : which) dst.push_back(&out[i].codes);
    return mf.encode(which, dst) ? 1 : -1;
}

static bool load_fasta(const char* path, const std::vector<std::string>* want, std::vector<FastaRecord>& out, std::string& err)
{
    if (!getenv("BQC_FASTA_SEQUENTIAL")) {
        const int rc = load_fasta_mapped(path, want, out);
        if (rc > 0) return true;
        if (rc < 0) { err = std::string("ERROR: out of memory while loading ") + path; return false; }
        out.clear();
    }
    gzFile f = gzopen(path, "rb");
    if (!f) { err = std::string("ERROR: Could not open fasta file ") + path; return false; }
    gzbuffer(f, 1 << 20);
    std::vector<char> buf(1 << 22);
    // An uncompressed file bounds every contig by the bytes that are left: reserving that much (address space only) saves
    // growing a multi-hundred-megabyte vector through a dozen reallocations, each faulting in fresh pages.
    uint64_t file_size = 0, consumed = 0, reserve_hint = 0; // (consumed: bytes of the buffers before the current one)
    {
        struct stat st;
        if (gzdirect(f) && stat(path, &st) == 0 && st.st_size > 0) file_size = (uint64_t)st.st_size;
    }
    FastaRecord* cur = nullptr;
    bool keep = false, in_header = false;
    std::string hdr;
    uint8_t lut[256];
    for (int i = 0; i < 256; ++i) lut[i] = dna5_of_char((char)i);
    auto finish_header = [&]() {
        size_t cut = hdr.find_first_of(" \t");
        std::string name = hdr.substr(0, cut);
        if (!name.empty() && name.back() == '\r') name.pop_back();
        out.push_back(FastaRecord{name, {}});
        cur = &out.back();
        keep = true;
        if (want) {
            keep = false;
            for (const auto& w : *want) if (w == name) { keep = true; break; }
        }
        if (keep && reserve_hint) { try { cur->codes.reserve((size_t)reserve_hint); } catch (const std::bad_alloc&) {} }
        hdr.clear();
    };
    int n;
    while ((n = gzread(f, buf.data(), (unsigned)buf.size())) > 0) {
        // Same rules as a byte-at-a-time scan ('>' anywhere outside a header line starts one; '\n' and '\r' are dropped from
        // sequence), but header lines and runs of sequence are handled in bulk: a whole genome is a few GB of text.
        const char* p = buf.data();
        const char* const end = p + n;
        while (p < end) {
            if (in_header) {
                const char* nl = (const char*)memchr(p, '\n', (size_t)(end - p));
                if (!nl) { hdr.append(p, (size_t)(end - p)); break; }
                hdr.append(p, (size_t)(nl - p));
                in_header = false;
                { const uint64_t at = consumed + (uint64_t)(nl - buf.data()); reserve_hint = file_size > at ? file_size - at : 0; }
                finish_header();
                p = nl + 1;
                continue;
            }
            const char* gt = (const char*)memchr(p, '>', (size_t)(end - p));
            const char* stop = gt ? gt : end;
            if (cur && keep && stop > p) {
                raw_vector<uint8_t>& codes = cur->codes;
                const size_t at = codes.size();
                codes.resize(at + (size_t)(stop - p));
                uint8_t* w = codes.data() + at;
                for (const char* q = p; q < stop; ++q) {
                    const char c = *q;
                    *w = lut[(uint8_t)c];
                    w += (c != '\n') & (c != '\r');
                }
                codes.resize((size_t)(w - codes.data()));
            }
            p = stop;
            if (gt) { in_header = true; ++p; }
        }
        consumed += (uint64_t)n;
    }
    if (in_header) finish_header();
    gzclose(f);
    return true;
}

// ---------------------------------------------------------------------------------------------------
// C wrappers around the reader (python drivers, tests)
// ---------------------------------------------------------------------------------------------------
static bool is_bgzf_magic(const uint8_t* p, size_t n) { return n >= 2 && p[0] == 0x1f && p[1] == 0x8b; }
// the first bytes of a descriptor nobody has read from yet: at least two, unless it ends before (into `first`)
static void sniff_fd(int fd, std::vector<uint8_t>& first)
{
    first.resize(1u << 16);
    size_t n = 0;
    while (n < 2) {
        const ssize_t r = read(fd, first.data() + n, first.size() - n);
        if (r < 0 && errno == EINTR) continue;
        if (r <= 0) break;
        n += (size_t)r;
    }
    first.resize(n);
}
// The same look at a stdio stream.  true: BGZF — the two bytes have been taken and are in `taken` (for BgzfStream::preload).  false: text,
// and the stream is as it was: one byte goes back with the one ungetc ISO C guarantees; only text that starts with 0x1f but is no gzip
// member — no SAM, a line the parser refuses either way — needs a second one, which glibc grants for bytes just read from the buffer.
static bool sniff_stdio_bgzf(FILE* f, std::vector<uint8_t>& taken)
{
    const int c0 = getc(f);
    if (c0 == EOF) return false;
    if (c0 != 0x1f) { ungetc(c0, f); return false; }
    const int c1 = getc(f);
    if (c1 == 0x8b) { taken = {0x1f, 0x8b}; return true; }
    if (c1 != EOF) ungetc(c1, f);
    ungetc(c0, f);
    return false;
}
// (tests) BQC_STREAM_HOLD=N: the stream object holds N bytes before its first reader exists — the header is then parsed, and the stream
// read, over {a prefix cut at N, then the descriptor}, wherever N lies: inside the header, inside a block, behind the stream's end
static void stream_test_hold(BgzfStream& src) { if (const char* e = getenv("BQC_STREAM_HOLD")) src.hold((size_t)strtoull(e, nullptr, 10)); }
// the block boundaries of a shard, as BamReader::open_range finds them (bgzf_find_block is a function of the hint), and the compressed bytes
// between them; 0: an empty shard (or an error: err set)
static uint64_t shard_blocks(const char* path, uint64_t begin_hint, uint64_t end_hint, uint64_t& b0, uint64_t& b1, std::string& err)
{
    const uint64_t size = bgzf_file_size(path);
    b1 = end_hint >= size ? UINT64_MAX : bgzf_find_block(path, end_hint, err);
    if (b1 >= size) b1 = UINT64_MAX;
    b0 = begin_hint == 0 ? 0 : bgzf_find_block(path, begin_hint, err);
    return err.empty() && b0 < std::min(b1, size) ? std::min(b1, size) - b0 : 0;
}

// One opener for every input: it carries out what input_route answers (host/input_route.h; DESIGN section 4.5d, "which reader takes it") for
// the program and for bqc_bam_open*, in the three steps the program needs at three moments.  It owns the readers, the stdio stream of plain
// text, the stream object and a shard's block boundaries; the reader of BAM on the card is its own or one lent to it (a session's, which
// survives from job to job).
struct InputOpener {
    explicit InputOpener(GpuBamReader* lent = nullptr) : gpu_(lent ? lent : &own_gpu_) { if (lent) lent->set_anchor_context(nullptr); } // (the context of the job before may not outlive this one's set-up)
    ~InputOpener() { if (fp_ && fp_ != stdin) fclose(fp_); }
    // No device needed.  Gathers the facts `f` leaves open (one stat, the look at "-", what a BGZF stream carries, a shard's blocks), has the host
    // reader of the route parse the header — from bytes that are kept, for a stream: nothing is read twice — holds a stream while the caller's
    // runtime starts beside it, and prepares the reader the route ends at.  false: route().refuse, or err (an I/O error).
    bool open(const char* path, bqc_route_facts f, uint64_t begin_hint, uint64_t end_hint, std::string& err)
    {
        path_ = path;
        bool regular = false;
        f.kind = input_kind(path, &regular, &f.size);
        f.regular = regular;
        f.gpu_decode = gpu_decode_env();
        rt_ = input_route(f);
        std::vector<uint8_t> first; // "-": its first bytes say what it carries
        if (rt_.sniff == SNIFF_FD) { sniff_fd(0, first); f.dash_bgzf = is_bgzf_magic(first.data(), first.size()); }
        if (rt_.sniff == SNIFF_STDIO) f.dash_bgzf = sniff_stdio_bgzf(stdin, first);
        std::string blocks_err;
        if (rt_.find_blocks) { f.shard_bytes = shard_blocks(path, begin_hint, end_hint, b0_, b1_, blocks_err); f.shard_found = f.shard_bytes != 0; }
        rt_ = input_route(f);
        if (rt_.refuse) {
            err = rt_.refuse == REFUSE_STDIN_SHARD ? "a stream on stdin cannot be split between processes" : rt_.refuse == REFUSE_SAM_SHARD ? "SAM text cannot be read in shards" : blocks_err.empty() ? "empty shard" : blocks_err;
            return false;
        }
        auto descriptor = [&]() { // (whoever takes it owns it from its first byte)
            const int fd = f.kind == IN_STDIN ? 0 : ::open(path, O_RDONLY);
            if (fd < 0) err = std::string("could not open ") + path;
            return fd;
        };
        if (rt_.stream) { // a BGZF stream (DESIGN sections 4.5c, 4.5d): what it carries is looked at inside the bytes the stream object keeps
            if (rt_.sniff == SNIFF_STDIO) src_ = std::make_shared<BgzfStream>(stdin);
            else {
                const int fd = descriptor();
                if (fd < 0) return false;
                src_ = std::make_shared<BgzfStream>(fd);
            }
            if (!first.empty()) src_->preload(first.data(), first.size());
            stream_test_hold(*src_);
            if (f.kind != IN_SAM_BGZF) { f.carries = bgzf_stream_carries(*src_); rt_ = input_route(f); }
        }
        const BamHeader* hdr = nullptr;
        if (rt_.header_by == HDR_GSAM) { // plain text: the reader takes the descriptor, holds, and parses the header itself
            const int fd = descriptor();
            if (fd < 0) return false;
            gsam_.preload(first.data(), first.size());
            if (!gsam_.start(fd, (size_t)rt_.hold, err)) return false;
            f.ended = gsam_.stream_ended();
            hdr = &gsam_.header();
        } else if (rt_.header_by == HDR_SAM_STDIO) {
            fp_ = f.kind == IN_STDIN ? stdin : fopen(path, "r");
            if (!fp_) { err = std::string("could not open ") + path; return false; }
            if (!sam_.open(fp_, err)) return false;
            hdr = &sam_.header();
        } else if (rt_.header_by == HDR_SAM_BGZF) {
            if (src_ ? !sam_.open_bgzf_stream(src_, err) : !sam_.open_bgzf(path, err)) return false;
            hdr = &sam_.header();
        } else if (f.shard && rt_.header_first) { // a shard the card may take: the header through a reader of its own, the range is opened below
            BamReader whole;
            if (!whole.open(path, err, true)) return false;
            gpu_->header() = whole.header();
            first_record_ = whole.stream_pos();
            hdr = &gpu_->header();
        } else {
            if (src_ ? !bam_.open_stream(src_, err) : f.shard ? !bam_.open_range(path, begin_hint, end_hint, err) : !bam_.open(path, err, rt_.header_first != 0)) return false;
            hdr = &bam_.header();
        }
        f.has_rg = hdr->lane_count != 0;
        rt_ = input_route(f);
        if (src_ && rt_.hold) { src_->hold((size_t)rt_.hold); f.ended = src_->has_ended(); rt_ = input_route(f); } // (the calling thread holds the stream meanwhile)
        if (src_ && !route_on_card(rt_)) src_->release(); // the host reader goes on, over {what is held, then the descriptor}; nothing more is kept
        if (rt_.reader == RD_GPU_BAM && hdr == &bam_.header()) {
            gpu_->header() = bam_.header(); // (complete once opened on the device)
            first_record_ = bam_.stream_pos();
            bam_.close(); // (its read-ahead has inflated the first run of blocks for the header; no more.  Nobody is inside the stream object any more)
        }
        if (rt_.reader == RD_GPU_BAM && rt_.source == SRC_RANGE) gpu_->set_range(b0_, b1_);
        if (rt_.reader == RD_BAM && hdr == &gpu_->header()) return bam_.open_range(path, begin_hint, end_hint, err); // (no @RG line: the host reader, over its range, decides what that means)
        if (rt_.reader == RD_GPU_SAM_BGZF) {
            gsam_.start_bgzf(sam_.header(), sam_.ref_index(), sam_.first_record_pos(), path);
            sam_.close();
        }
        return true;
    }
    // The device side of a reader on the card (nothing to do for the others): a stream changes hands — descriptor and prefix, by move: the prefix is
    // the first runs' input — and the reader opens.  false: err, and code says what the caller may do — GpuBamReader::kUnsupported for a BAM file
    // (the host reader can take a second pass), BQC_ERR_DEVICE for a stream (it cannot be started over) and for SAM text.
    bool start_card(int device, size_t batch_reads, size_t batch_bases, std::string& err, int& code)
    {
        bool ok = true;
        if (rt_.reader == RD_GPU_BAM) {
            if (src_) gpu_->set_stream(src_->release_fd(), std::move(src_->held), src_->has_ended());
            ok = gpu_->open(path_.c_str(), device, gpu_->header(), first_record_, batch_reads, batch_bases, err);
        } else if (route_gpu_sam(rt_)) {
            if (src_) gsam_.producer().set_stream(src_->release_fd(), std::move(src_->held), src_->has_ended());
            ok = gsam_.open(device, batch_reads, batch_bases, err);
        }
        code = ok ? 0 : rt_.reader == RD_GPU_BAM && !src_ ? GpuBamReader::kUnsupported : BQC_ERR_DEVICE;
        started_ = ok && route_on_card(rt_);
        return ok;
    }
    // The reader on the card may launch its first kernel (the caller's own device set-up is done); ctx: the batches' coverage anchors are made on
    // the card from the first batch on (BQC_DEVICE_ANCHORS=0, or no context: the host's pass, columns and all)
    void allow(bqc_ctx* ctx)
    {
        const char* da = getenv("BQC_DEVICE_ANCHORS");
        auto go = [&](auto& r) { if (ctx && !(da && da[0] == '0')) r.set_anchor_context(ctx); r.allow_kernels(); };
        if (rt_.reader == RD_GPU_BAM) go(*gpu_);
        else if (route_gpu_sam(rt_)) go(gsam_);
    }
    const bqc_route& route() const { return rt_; }
    RecordReader& reader()
    {
        if (rt_.reader == RD_GPU_BAM) return *gpu_;
        if (route_any_gsam(rt_)) return gsam_;
        return rt_.header_by == HDR_BAM ? static_cast<RecordReader&>(bam_) : sam_;
    }
    BamReader& bam() { return bam_; }
    GpuBamReader& gpu() { return *gpu_; }
    GpuSamReader& gsam() { return gsam_; }
    bool on_card() const { return started_; }
    uint64_t batches_handed_over() const { return rt_.reader == RD_GPU_BAM ? gpu_->batches_handed_over() : route_any_gsam(rt_) ? gsam_.batches_handed_over() : 0; }
    uint64_t range_begin_block() const { return rt_.reader == RD_GPU_BAM ? b0_ : bam_.range_begin_block(); }
    uint64_t range_end_block() const { return rt_.reader == RD_GPU_BAM ? b1_ : bam_.range_end_block(); }
    uint64_t range_first() const { return rt_.reader == RD_GPU_BAM ? gpu_->range_first() : bam_.range_first(); }
    uint64_t range_over() const { return rt_.reader == RD_GPU_BAM ? gpu_->range_over() : bam_.range_over(); }

private:
    bqc_route rt_{};
    std::string path_;
    BamReader bam_;
    SamReader sam_;
    FILE* fp_ = nullptr; // (plain text the host reader reads)
    GpuSamReader gsam_;
    std::shared_ptr<BgzfStream> src_;
    GpuBamReader own_gpu_;
    GpuBamReader* gpu_;
    uint64_t b0_ = 0, b1_ = UINT64_MAX, first_record_ = 0;
    bool started_ = false;
};

struct bqc_bam {
    InputOpener in;
    RecordReader& rd() { return in.reader(); }
    const BamHeader& hdr() const { return const_cast<bqc_bam*>(this)->rd().header(); }
    HostBatch hb;
    bqc_batch view;
    std::string err;
    std::vector<std::string> lane_sorted;
    std::vector<uint32_t> lane_idx;
    void refresh_lanes()
    {
        lane_sorted.clear(); lane_idx.clear();
        for (auto& kv : rd().header().lane_names) { lane_sorted.push_back(kv.first); lane_idx.push_back(kv.second); }
    }
};
// bqc_bam_open*: *out is set on failure too, so that the message can be read
static int bam_open_as(RouteCaller caller, const char* path, int device, bool shard, uint64_t begin_hint, uint64_t end_hint, bqc_bam** out)
{
    if (!path || !out) return BQC_ERR_ARG;
    auto* b = new bqc_bam();
    *out = b;
    bqc_route_facts f{};
    f.caller = caller; f.shard = shard;
    if (!b->in.open(path, f, begin_hint, end_hint, b->err)) return b->in.route().refuse ? BQC_ERR_ARG : BQC_ERR_IO;
    int code = 0;
    if (!b->in.start_card(device, 1u << 20, 256u << 20, b->err, code)) return BQC_ERR_DEVICE;
    b->in.allow(nullptr);
    b->refresh_lanes();
    return 0;
}
extern "C" int bqc_bam_open(const char* path, bqc_bam** out) { return bam_open_as(CALLER_LIB_HOST, path, 0, false, 0, 0, out); }
extern "C" int bqc_bam_open_range(const char* path, uint64_t begin_hint, uint64_t end_hint, bqc_bam** out) { return bam_open_as(CALLER_LIB_HOST, path, 0, true, begin_hint, end_hint, out); }
extern "C" int bqc_bam_open_gpu(const char* path, int device, bqc_bam** out) { return bam_open_as(CALLER_LIB_CARD, path, device, false, 0, 0, out); }
extern "C" int bqc_bam_open_gpu_range(const char* path, int device, uint64_t begin_hint, uint64_t end_hint, bqc_bam** out) { return bam_open_as(CALLER_LIB_CARD, path, device, true, begin_hint, end_hint, out); }
extern "C" uint64_t bqc_bam_range_begin_block(const bqc_bam* b) { return b->in.range_begin_block(); }
extern "C" uint64_t bqc_bam_range_end_block(const bqc_bam* b) { return b->in.range_end_block(); }
extern "C" uint64_t bqc_bam_range_first(const bqc_bam* b) { return b->in.range_first(); }
extern "C" uint64_t bqc_bam_range_over(const bqc_bam* b) { return b->in.range_over(); }
extern "C" int bqc_bam_on_card(const bqc_bam* b) { return b && b->in.on_card() ? 1 : 0; }
extern "C" uint64_t bqc_bam_batches_handed_over(const bqc_bam* b) { return b ? b->in.batches_handed_over() : 0; }
extern "C" uint64_t bqc_file_size(const char* path) { return path ? bgzf_file_size(path) : 0; }
extern "C" void bqc_gpu_inflate_device(int device) { bgzf_gpu_inflate_device(device); }
extern "C" uint64_t bqc_gpu_inflated_blocks(void) { return bgzf_gpu_inflated_blocks(); }
extern "C" int bqc_inflate_raw(const uint8_t* in, uint64_t in_n, uint8_t* out, uint64_t out_n)
{
    static thread_local Inflater inf;
    return inf.run(in, (size_t)in_n, out, (size_t)out_n) ? 1 : 0;
}
extern "C" uint32_t bqc_crc32(const uint8_t* p, uint64_t n) { return bqc_crc32_fast(p, (size_t)n); }
extern "C" void bqc_bam_close(bqc_bam* b) { delete b; }
extern "C" const char* bqc_bam_error(const bqc_bam* b) { return b ? b->err.c_str() : ""; }
extern "C" uint32_t bqc_bam_n_refs(const bqc_bam* b) { return (uint32_t)b->hdr().ref_names.size(); }
extern "C" const char* bqc_bam_ref_name(const bqc_bam* b, uint32_t i) { return b->hdr().ref_names[i].c_str(); }
extern "C" uint32_t bqc_bam_ref_len(const bqc_bam* b, uint32_t i) { return b->hdr().ref_lens[i]; }
extern "C" const char* bqc_bam_sample_id(const bqc_bam* b) { return b->hdr().sample_id.c_str(); }
extern "C" uint32_t bqc_bam_lane_count(const bqc_bam* b) { return b->hdr().lane_count; }
extern "C" uint32_t bqc_bam_n_lane_names(bqc_bam* b) { b->refresh_lanes(); return (uint32_t)b->lane_sorted.size(); }
extern "C" const char* bqc_bam_lane_name(const bqc_bam* b, uint32_t i) { return b->lane_sorted[i].c_str(); }
extern "C" uint32_t bqc_bam_lane_index(const bqc_bam* b, uint32_t i) { return b->lane_idx[i]; }
extern "C" int bqc_bam_set_main_chrom(bqc_bam* b, const uint8_t* mc)
{
    if (!b || !mc) return BQC_ERR_ARG;
    b->rd().set_main_chrom(std::vector<uint8_t>(mc, mc + b->hdr().ref_names.size()));
    return 0;
}
extern "C" int bqc_bam_set_rid_filter(bqc_bam* b, const uint8_t* keep, int keep_unplaced)
{
    if (!b || !keep) return BQC_ERR_ARG;
    if (b->in.route().header_by != HDR_BAM) return BQC_ERR_ARG; // (chromosome sharding needs the BAM reader)
    b->in.bam().set_rid_filter(std::vector<uint8_t>(keep, keep + b->hdr().ref_names.size()), keep_unplaced != 0);
    return 0;
}
extern "C" int bqc_bam_next(bqc_bam* b, uint32_t max_reads, uint64_t max_bases, const bqc_batch** out)
{
    if (!b || !out) return -BQC_ERR_ARG;
    int code = 0;
    const int rc = b->rd().next_batch(b->hb, max_reads, max_bases, b->err, code);
    if (rc < 0) return code < 0 ? code : -code; // (GpuBamReader::kUnsupported is negative already)
    if (b->hb.d_seq) { // callers of this wrapper read the columns on the host: fetch the payload
        HostBatch& h = b->hb;
        uint64_t so = 0, qo = 0, co = 0;
        for (size_t i = 0; i < h.n(); ++i) { so += (h.l_seq[i] + 1u) / 2u; qo += h.l_seq[i]; co += h.n_cigar[i]; }
        h.seq.resize(so); h.qual.resize(qo); h.cigar.resize(co);
        if ((so && hipMemcpy(h.seq.data(), h.d_seq, so, hipMemcpyDeviceToHost) != hipSuccess) || (qo && hipMemcpy(h.qual.data(), h.d_qual, qo, hipMemcpyDeviceToHost) != hipSuccess) ||
            (co && hipMemcpy(h.cigar.data(), h.d_cigar, 4 * co, hipMemcpyDeviceToHost) != hipSuccess)) { b->err = "copy from the device failed"; return -BQC_ERR_DEVICE; }
        h.d_seq = h.d_qual = nullptr; h.d_cigar = nullptr;
    }
    b->view = b->hb.view();
    *out = &b->view;
    return rc;
}

extern "C" int bqc_fasta_load(const char* path, uint32_t* n_records, char*** names, uint8_t*** codes, uint64_t** lens)
{
    std::vector<FastaRecord> recs;
    std::string err;
    if (!load_fasta(path, nullptr, recs, err)) return BQC_ERR_IO;
    *n_records = (uint32_t)recs.size();
    *names = (char**)calloc(recs.size() + 1, sizeof(char*));
    *codes = (uint8_t**)calloc(recs.size() + 1, sizeof(uint8_t*));
    *lens = (uint64_t*)calloc(recs.size() + 1, sizeof(uint64_t));
    for (size_t i = 0; i < recs.size(); ++i) {
        (*names)[i] = strdup(recs[i].name.c_str());
        (*codes)[i] = (uint8_t*)malloc(recs[i].codes.size() + 1);
        memcpy((*codes)[i], recs[i].codes.data(), recs[i].codes.size());
        (*lens)[i] = recs[i].codes.size();
    }
    return 0;
}
extern "C" void bqc_fasta_free(uint32_t n, char** names, uint8_t** codes, uint64_t* lens)
{
    for (uint32_t i = 0; i < n; ++i) { free(names[i]); free(codes[i]); }
    free(names); free(codes); free(lens);
}

// ---------------------------------------------------------------------------------------------------
// synthetic BAM + FASTA files
// ---------------------------------------------------------------------------------------------------
extern "C" int bqc_synth_write(const bqc_synth_params* p, const char* const* ref_names, const char* bam_path, const char* fasta_path,
                               uint32_t batch_reads)
{
    if (!p || !bam_path || !ref_names) return BQC_ERR_ARG;
    std::vector<std::vector<uint8_t>> refs(p->n_refs);
    std::vector<const uint8_t*> rp(p->n_refs);
    std::vector<std::string> names;
    std::vector<uint32_t> lens;
    for (uint32_t c = 0; c < p->n_refs; ++c) {
        refs[c].resize(p->ref_len[c]);
        bqc_synth_reference(p->seed, (int32_t)c, p->ref_len[c], refs[c].data());
        rp[c] = refs[c].data();
        names.push_back(ref_names[c]);
        lens.push_back(p->ref_len[c]);
    }
    if (fasta_path) {
        FILE* f = fopen(fasta_path, "wb");
        if (!f) return BQC_ERR_IO;
        std::string line;
        for (uint32_t c = 0; c < p->n_refs; ++c) {
            fprintf(f, ">%s synthetic contig %u\n", ref_names[c], c);
            for (uint64_t i = 0; i < refs[c].size(); i += 60) {
                line.clear();
                for (uint64_t k = i; k < std::min<uint64_t>(refs[c].size(), i + 60); ++k) line.push_back("ACGTN"[refs[c][k]]);
                line.push_back('\n');
                fwrite(line.data(), 1, line.size(), f);
            }
        }
        fclose(f);
    }
    std::string text = "@HD\tVN:1.6\tSO:coordinate\n";
    for (uint32_t c = 0; c < p->n_refs; ++c) text += "@SQ\tSN:" + names[c] + "\tLN:" + std::to_string(lens[c]) + "\n";
    std::vector<std::string> lane_ids;
    for (uint32_t l = 0; l < std::max(1u, p->n_lanes); ++l) {
        lane_ids.push_back("L" + std::to_string(l + 1));
        text += "@RG\tID:" + lane_ids.back() + "\tSM:SYN\tPL:ILLUMINA\n";
    }
    BamWriter w;
    std::string err;
    if (!w.open(bam_path, text, names, lens, err)) return BQC_ERR_IO;
    // One generator call for all reads keeps the coordinate order; written in slices.
    bqc_batch* b = nullptr;
    int rc = bqc_synth_batch(p, rp.data(), &b);
    if (rc) return rc;
    (void)batch_reads;
    const bool ok = w.write_batch(*b, lane_ids, p->first_read_index) && w.close();
    bqc_synth_batch_free(b);
    return ok ? 0 : BQC_ERR_IO;
}

static std::string synth_header_text(const std::vector<std::string>& names, const std::vector<uint32_t>& lens, uint32_t n_lanes, std::vector<std::string>& lane_ids)
{
    std::string text = "@HD\tVN:1.6\tSO:coordinate\n";
    for (size_t c = 0; c < names.size(); ++c) text += "@SQ\tSN:" + names[c] + "\tLN:" + std::to_string(lens[c]) + "\n";
    for (uint32_t l = 0; l < std::max(1u, n_lanes); ++l) {
        lane_ids.push_back("L" + std::to_string(l + 1));
        text += "@RG\tID:" + lane_ids.back() + "\tSM:SYN\tPL:ILLUMINA\n";
    }
    return text;
}

extern "C" int bqc_bam_write(const char* path, const bqc_batch* b, uint32_t n_refs, const char* const* ref_names, const uint32_t* ref_lens,
                             uint32_t n_lanes, uint64_t first_read_index, int level)
{
    if (!path || !b || (n_refs && (!ref_names || !ref_lens))) return BQC_ERR_ARG;
    std::vector<std::string> names, lane_ids;
    std::vector<uint32_t> lens;
    for (uint32_t c = 0; c < n_refs; ++c) { names.push_back(ref_names[c]); lens.push_back(ref_lens[c]); }
    const std::string text = synth_header_text(names, lens, n_lanes, lane_ids);
    for (uint32_t i = 0; i < b->n_reads; ++i) if (b->lane[i] >= lane_ids.size()) return BQC_ERR_ARG;
    BamWriter w;
    std::string err;
    if (!w.open(path, text, names, lens, err, level)) return BQC_ERR_IO;
    return w.write_batch_parallel(*b, lane_ids, first_read_index) && w.close() ? 0 : BQC_ERR_IO;
}

// The same batch as SAM text: the header's lines, then a line per read (PNEXT 0, RNEXT "=" on a placed read, integer tags as type i).
extern "C" int bqc_sam_write(const char* path, const bqc_batch* b, uint32_t n_refs, const char* const* ref_names, const uint32_t* ref_lens,
                             uint32_t n_lanes, uint64_t first_read_index)
{
    if (!path || !b || (n_refs && (!ref_names || !ref_lens))) return BQC_ERR_ARG;
    std::vector<std::string> names, lane_ids;
    std::vector<uint32_t> lens;
    for (uint32_t c = 0; c < n_refs; ++c) { names.push_back(ref_names[c]); lens.push_back(ref_lens[c]); }
    const std::string text = synth_header_text(names, lens, n_lanes, lane_ids);
    const size_t n = b->n_reads;
    for (size_t i = 0; i < n; ++i) if (b->lane[i] >= lane_ids.size() || b->rid[i] >= (int32_t)n_refs) return BQC_ERR_ARG;
    FILE* f = fopen(path, "wb");
    if (!f) return BQC_ERR_IO;
    setvbuf(f, nullptr, _IOFBF, 1 << 22);
    bool ok = fwrite(text.data(), 1, text.size(), f) == text.size();
    std::vector<uint64_t> so_at(n + 1), qo_at(n + 1), co_at(n + 1);
    for (size_t i = 0; i < n; ++i) { so_at[i + 1] = so_at[i] + (b->l_seq[i] + 1) / 2; qo_at[i + 1] = qo_at[i] + b->l_seq[i]; co_at[i + 1] = co_at[i] + b->n_cigar[i]; }
    const size_t slice = 1u << 18; // lines are made by all host threads, a slice at a time, and written in order
    for (size_t lo = 0; ok && lo < n; lo += slice) {
        const size_t cnt = std::min(slice, n - lo);
        const unsigned nt = std::max(1u, bqc_host_threads());
        std::vector<std::string> part(nt);
        parallel_ranges(cnt, nt, 4096, [&](unsigned t, size_t a, size_t z) {
            std::string& o = part[t];
            char num[32];
            for (size_t i = lo + a; i < lo + z; ++i) {
                const uint32_t L = b->l_seq[i], nc = b->n_cigar[i];
                o += 'r'; o += std::to_string(first_read_index + i); o += '\t';
                o += std::to_string(b->flag[i] & 0x0FFFu); o += '\t';
                if (b->rid[i] >= 0) o += names[b->rid[i]]; else o += '*';
                o += '\t'; o += std::to_string((int64_t)b->pos[i] + 1); o += '\t'; o += std::to_string(b->mapq[i]); o += '\t';
                if (!nc) o += '*';
                for (uint32_t k = 0; k < nc; ++k) { const uint32_t w = b->cigar[co_at[i] + k]; snprintf(num, sizeof num, "%u%c", w >> 4, (w & 15u) < 9 ? kSamOps[w & 15u] : '?'); o += num; }
                o += b->rid[i] >= 0 ? "\t=\t0\t" : "\t*\t0\t";
                o += std::to_string(b->tlen[i]); o += '\t';
                if (!L) o += '*';
                for (uint32_t k = 0; k < L; ++k) { const uint8_t by = b->seq[so_at[i] + k / 2]; o += kSamNib[k & 1 ? by & 15 : by >> 4]; }
                o += '\t';
                if (!L || b->qual[qo_at[i]] == 0xFF) o += '*';
                else for (uint32_t k = 0; k < L; ++k) o += (char)(b->qual[qo_at[i] + k] + 33);
                o += "\tRG:Z:"; o += lane_ids[b->lane[i]];
                if (b->nm[i] != BQC_NM_ABSENT) { o += "\tNM:i:"; o += std::to_string(b->nm[i]); }
                if (b->as[i] != BQC_AS_ABSENT) { o += "\tAS:i:"; o += std::to_string(b->as[i]); }
                o += '\n';
            }
        });
        for (const std::string& o : part) ok = ok && fwrite(o.data(), 1, o.size(), f) == o.size();
    }
    return (fclose(f) == 0) && ok ? 0 : BQC_ERR_IO;
}

// The plan of bqc_synth_write, streamed: slices of the plan are generated (bqc_synth_slice), serialised into BAM records by
// all host threads (sizes -> prefix sum -> every thread writes its records in place) and handed to the BGZF writer.
extern "C" int bqc_synth_stream(const bqc_synth_params* p, const char* const* ref_names, const char* bam_path, const char* fasta_path,
                                uint32_t slice_reads, int level)
{
    if (!p || !bam_path || !ref_names || p->n_refs == 0) return BQC_ERR_ARG;
    if (!slice_reads) slice_reads = 1u << 21;
    std::vector<std::vector<uint8_t>> refs(p->n_refs);
    std::vector<const uint8_t*> rp(p->n_refs);
    std::vector<std::string> names;
    std::vector<uint32_t> lens;
    for (uint32_t c = 0; c < p->n_refs; ++c) {
        refs[c].resize(p->ref_len[c]);
        bqc_synth_reference(p->seed, (int32_t)c, p->ref_len[c], refs[c].data());
        rp[c] = refs[c].data();
        names.push_back(ref_names[c]);
        lens.push_back(p->ref_len[c]);
    }
    if (fasta_path) {
        FILE* f = fopen(fasta_path, "wb");
        if (!f) return BQC_ERR_IO;
        setvbuf(f, nullptr, _IOFBF, 1 << 22);
        std::vector<char> text;
        for (uint32_t c = 0; c < p->n_refs; ++c) {
            fprintf(f, ">%s synthetic contig %u\n", ref_names[c], c);
            const std::vector<uint8_t>& r = refs[c];
            const size_t n = r.size(), lines = (n + 59) / 60;
            text.resize(n + lines);
            parallel_ranges(lines, bqc_host_threads(), 1 << 14, [&](unsigned, size_t lo, size_t hi) {
                for (size_t l = lo; l < hi; ++l) {
                    const size_t a = l * 60, z = std::min(n, a + 60);
                    char* w = text.data() + a + l;
                    for (size_t k = a; k < z; ++k) *w++ = "ACGTN"[r[k]];
                    *w = '\n';
                }
            });
            if (fwrite(text.data(), 1, text.size(), f) != text.size()) { fclose(f); return BQC_ERR_IO; }
        }
        if (fclose(f) != 0) return BQC_ERR_IO;
    }
    std::vector<std::string> lane_ids;
    const std::string text = synth_header_text(names, lens, p->n_lanes, lane_ids);
    BamWriter w;
    std::string err;
    if (!w.open(bam_path, text, names, lens, err, level)) return BQC_ERR_IO;
    const bool timing = getenv("BQC_TIMING") != nullptr;
    double t_gen = 0, t_write = 0;
    for (uint64_t lo = 0; lo < p->n_reads; lo += slice_reads) {
        const uint32_t cnt = (uint32_t)std::min<uint64_t>(slice_reads, p->n_reads - lo);
        bqc_batch* b = nullptr;
        const auto t0 = std::chrono::steady_clock::now();
        const int rc = bqc_synth_slice(p, lo, cnt, rp.data(), &b);
        if (rc) return rc;
        const auto t1 = std::chrono::steady_clock::now();
        const bool ok = w.write_batch_parallel(*b, lane_ids, p->first_read_index + lo);
        bqc_synth_batch_free(b);
        const auto t2 = std::chrono::steady_clock::now();
        t_gen += std::chrono::duration<double>(t1 - t0).count();
        t_write += std::chrono::duration<double>(t2 - t1).count();
        if (!ok) return BQC_ERR_IO;
    }
    if (timing) fprintf(stderr, "[timing] synthetic stream of %u reads: generate %.2f s, serialise + compress + write %.2f s\n", p->n_reads, t_gen, t_write);
    return w.close() ? 0 : BQC_ERR_IO;
}

using namespace bqc_cli; // the command line — ProgramOptions, parse_args, usage, the manifest's list: host/program_options.h

namespace {
// Page-locked decode buffers: the columns of every HostBatch the decoder fills are registered with the HIP runtime once
// (hipHostRegister, ~40 ms per GB of touched pages), so that bqc_submit_async copies them to the device without a staging
// copy; a block that a growing vector frees is released first (bqc_raw_vector_free_hook).
struct PinRegistry {
    std::mutex m;
    std::unordered_map<void*, size_t> blocks;
    double t_register = 0;
    void pin(const void* p, size_t bytes)
    {
        if (!p || bytes < (1u << 16)) return;
        std::lock_guard<std::mutex> lk(m);
        auto it = blocks.find((void*)p);
        if (it != blocks.end() && it->second >= bytes) return;
        if (it != blocks.end()) { (void)bqc_host_unregister((void*)p); blocks.erase(it); }
        const auto t0 = std::chrono::steady_clock::now();
        if (bqc_host_register((void*)p, bytes) == 0) blocks[(void*)p] = bytes;
        t_register += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    }
    void release(void* p)
    {
        std::lock_guard<std::mutex> lk(m);
        auto it = blocks.find(p);
        if (it == blocks.end()) return;
        (void)bqc_host_unregister(p);
        blocks.erase(it);
    }
    void release_all()
    {
        std::lock_guard<std::mutex> lk(m);
        for (auto& kv : blocks) (void)bqc_host_unregister(kv.first);
        blocks.clear();
    }
};
PinRegistry g_pins;
void pin_free_hook(void* p) { g_pins.release(p); }
void pin_hook(const void* p, size_t bytes) { g_pins.pin(p, bytes); }
template <typename V> void pin_column(const V& v) { g_pins.pin(v.data(), v.capacity() * sizeof(typename V::value_type)); }
void pin_batch(const HostBatch& hb)
{
    pin_column(hb.flag); pin_column(hb.n_cigar); pin_column(hb.mapq); pin_column(hb.lane); pin_column(hb.seq); pin_column(hb.qual);
    pin_column(hb.rid); pin_column(hb.pos); pin_column(hb.tlen); pin_column(hb.nm); pin_column(hb.as); pin_column(hb.l_seq); pin_column(hb.cigar);
}

struct BatchQueue { // decode thread -> submit thread
    std::mutex m;
    std::condition_variable cv;
    std::deque<std::unique_ptr<HostBatch>> q;
    std::vector<std::unique_ptr<HostBatch>> spare; // submitted batches go back to the decoder: their ~300 MB of columns are reused
    bool done = false, stop = false;
    int err_code = 0;
    std::string err;
};
} // namespace

namespace {
struct ShardArgs { uint32_t index, count; bqc_shard_hook hook; void* user; };

// What identifies the reference genome a job needs: the FASTA file (path and what stat says of it) and the BAM header's @SQ lines.
struct RefKey {
    bool valid = false; // (false: the file could not be examined — never equal to anything)
    std::string path;
    uint64_t dev = 0, ino = 0, size = 0;
    int64_t mtime_s = 0, mtime_ns = 0;
    std::vector<std::string> sq_names;
    std::vector<uint32_t> sq_lens;
    bool operator==(const RefKey& o) const
    {
        return valid && o.valid && path == o.path && dev == o.dev && ino == o.ino && size == o.size && mtime_s == o.mtime_s && mtime_ns == o.mtime_ns && sq_names == o.sq_names && sq_lens == o.sq_lens;
    }
};
RefKey make_ref_key(const std::string& fasta, const BamHeader& H)
{
    RefKey k;
    struct stat st;
    if (stat(fasta.c_str(), &st) != 0 || !S_ISREG(st.st_mode)) return k;
    k.valid = true; k.path = fasta;
    k.dev = (uint64_t)st.st_dev; k.ino = (uint64_t)st.st_ino; k.size = (uint64_t)st.st_size; k.mtime_s = (int64_t)st.st_mtim.tv_sec; k.mtime_ns = (int64_t)st.st_mtim.tv_nsec;
    k.sq_names = H.ref_names; k.sq_lens = H.ref_lens;
    return k;
}
// What a context was made with (bqc_options and the modules): equal ones mean bqc_reset instead of bqc_create.
struct CtxKey {
    ModuleSettings mod;                                        // the modules' settings in use (settings_in_use: a module that is off adds nothing)
    std::vector<std::pair<std::string, std::string>> adapters; // (empty: the built-in set)
    // what the options name, as mapped to the job's header (empty: off)
    std::vector<int32_t> site_rid, site_pos, region_rid, region_start, region_end, window_depth_lens;
    std::vector<uint8_t> main_chrom;
    uint32_t n_lanes = 0, n_refs = 0, max_read_len = 0, hist_cap = 0;
    int isize = 0, device = 0;
    bool sketch = false; // and with it:
    double e = 0;
    int seed = 0;
    std::vector<int32_t> klist;
    std::vector<uint32_t> qlist;
    auto members() const { return std::tie(mod, adapters, site_rid, site_pos, region_rid, region_start, region_end, window_depth_lens, main_chrom, n_lanes, n_refs, max_read_len, hist_cap, isize, device, sketch, e, seed, klist, qlist); }
    bool operator==(const CtxKey& o) const { return members() == o.members(); }
};
}

// One process, many files: what outlives a job.  run_program borrows from it and gives back; without one it
// creates and destroys as ever.  The runtime itself (bqc_warmup's streams, the pin hooks' registry g_pins) is the process's already.
struct bqc_session {
    std::vector<std::string> args; // argv[0] and the options every job runs with
    bqc_ctx* ctx = nullptr;        // the context of the job before (whatever way that job ended: bqc_reset clears a poisoned one)
    CtxKey ctx_key;
    RefKey ref_key;                // the genome whose contigs are on the card, in ctx
    std::vector<int32_t> fasta_index; // for ref_key: each BAM reference's position in the FASTA file (the cursor rule), -1: not there
    uint32_t contigs_on_card = 0;
    // --site-alleles: the file is read when a job's header lists other contigs than the job before's; the mapped list is kept with them
    bool sites_loaded = false;
    std::vector<std::string> sites_names;
    std::vector<uint32_t> sites_lens;
    std::vector<int32_t> sites_rid, sites_pos;
    // --regions: the same for the BED file
    bool regions_loaded = false;
    std::vector<std::string> regions_names;
    std::vector<uint32_t> regions_lens;
    std::vector<int32_t> regions_rid, regions_start, regions_end;
    GpuBamReader gpu_rd;          // opened again for every file it takes: its buffers stay
    std::vector<std::unique_ptr<HostBatch>> spare; // the decoder's batch objects: their columns, page locks and device buffers
    std::atomic<bool> ended{false}; // a HIP error: nothing more is started on the card
    uint32_t job = 0, n_jobs = 0;  // the job that runs (1-based), and how many there will be if known
    // a job that starts over with the host reader (GpuBamReader::kUnsupported) reports what its FIRST pass found in place
    bool started_over = false, first_ctx_kept = false;
    uint32_t first_contigs = 0;
    ~bqc_session() { spare.clear(); if (ctx) bqc_destroy(ctx); }
};
typedef bqc_session Session;

static int run_program(int argc, const char** argv, const ShardArgs* shard, bool host_reader_only = false, Session* S = nullptr)
{
    ProgramOptions opt;
    std::string perr;
    const int pr = parse_args(argc, argv, opt, perr);
    if (pr == 2) return 0;
    if (pr == 1) { fprintf(stderr, "%s\n", perr.c_str()); return 1; }
    // (a worker of --gpus N holds only the contigs its batches touch: none has the genome table; the front end says so before it forks)
    const ModuleSettings& mod = opt.mod;
    const std::string conflict = shard ? gpus_conflict(mod) : std::string();
    if (!conflict.empty()) { fprintf(stderr, "%s\n", conflict.c_str()); return 1; }
    using clk = std::chrono::steady_clock;
    const bool timing = getenv("BQC_TIMING") && getenv("BQC_TIMING")[0] == '1'; // BQC_TIMING=1: where the wall time of a run goes (stderr)
    auto since_launch = [&](const char* what) { // (BQC_T0: the launcher's CLOCK_MONOTONIC seconds when it started the program)
        if (!timing || !getenv("BQC_T0")) return;
        const double now = std::chrono::duration<double>(clk::now().time_since_epoch()).count();
        fprintf(stderr, "[timing] %s: %.3f s after launch\n", what, now - atof(getenv("BQC_T0")));
    };
    since_launch("main entered");
    if (S) { // one option for every job, a genome per directory: "{dir}" in the reference's path stands for the directory of the job's input
        const size_t slash = opt.bamFile.rfind('/');
        const std::string dir = slash == std::string::npos ? "." : slash == 0 ? "/" : opt.bamFile.substr(0, slash);
        for (size_t at; (at = opt.referenceFile.find("{dir}")) != std::string::npos;) opt.referenceFile.replace(at, 5, dir);
    }
    auto note_rc = [S](int r) { if (S && r == BQC_ERR_DEVICE) S->ended = true; }; // a HIP error ends a session (the job fails as a single run does)
    setenv("GPU_MAX_HW_QUEUES", "8", 0); // (before the runtime starts: the batch pipeline, the reader and its producer each keep a hardware queue of their own)
    // the HIP runtime starts (~0.1 s) while the inputs are opened; from then on the reader's runs are inflated on the card
    const char* gi_env = getenv("BQC_GPU_INFLATE");
    const bool gpu_inflate = gi_env && atoi(gi_env) != 0;
    std::thread warm([dev = opt.device, gpu_inflate] {
        if (bqc_warmup(dev) != 0 || !gpu_inflate) return;
        bqc_raw_vector_free_hook = pin_free_hook; // the reader page-locks the buffers the card copies into
        bqc_raw_vector_pin_hook = pin_hook;
        bgzf_gpu_inflate_device(dev);
    });
    struct InflateOff { ~InflateOff() { bgzf_gpu_inflate_device(-1); bqc_raw_vector_pin_hook = nullptr; } } inflate_off; // (destroyed after the joiner below has joined the thread that sets it)
    struct Joiner { std::thread& t; ~Joiner() { if (t.joinable()) t.join(); } } warm_joiner{warm};
    // The input becomes a reader (InputOpener; DESIGN section 4.5d, "which reader takes it").  The reference opens every path as BAM
    // (bamqualcheck.cpp:252-262: a .sam path fails to open there).  A stream is held by this thread while the runtime starts beside it; a
    // BAM file the card takes may still end this pass before anything has been reported (GpuBamReader::kUnsupported), and the program
    // starts over with the host reader (host_reader_only).
    InputOpener in(S ? &S->gpu_rd : nullptr);
    std::string err;
    // a failure before the hook is reached must still reach it: the other processes wait for this one
    auto shard_abort = [&]() { if (shard) { bqc_shard_info si{}; si.status = 1; bqc_shard_result sr{}; (void)shard->hook(shard->user, &si, &sr); } return 1; };
    bqc_route_facts facts{};
    facts.caller = CALLER_PROGRAM; facts.host_reader_only = host_reader_only; facts.shard = shard != nullptr;
    uint64_t shard_lo = 0, shard_hi = UINT64_MAX; // this process's part of the compressed file
    if (shard) {
        const uint64_t size = bqc_file_size(opt.bamFile.c_str());
        shard_lo = size / shard->count * shard->index;
        if (shard->index + 1 != shard->count) shard_hi = size / shard->count * (shard->index + 1);
    }
    const bool opened = in.open(opt.bamFile.c_str(), facts, shard_lo, shard_hi, err);
    const bqc_route& rt = in.route();
    if (rt.refuse) { fprintf(stderr, "ERROR: %s\n", err.c_str()); return shard_abort(); } // (SAM text: the front end of --gpus N says so before it forks)
    since_launch("input opened");
    if (!opened) {
        fprintf(stderr, "ERROR: Could not open %s for reading.\n", opt.bamFile.c_str()); // bamqualcheck.cpp:265
        return shard_abort();
    }
    GpuBamReader& gpu_rd = in.gpu();
    GpuSamReader& gsam_rd = in.gsam();
    const bool bam_on_card = rt.reader == RD_GPU_BAM;
    if (bam_on_card) { bqc_raw_vector_free_hook = pin_free_hook; bqc_raw_vector_pin_hook = pin_hook; } // (the reader page-locks the buffers the card copies into)
    RecordReader& rd = in.reader();
    if (rd.header().lane_count > 256) { // the lane column is a byte and bqc_create takes 256 at the most: said here in the input's terms, before the output file is opened
        fprintf(stderr, "ERROR: %s: the header has %u @RG lines; at most 256 read groups are supported\n", opt.bamFile.c_str(), rd.header().lane_count);
        return shard_abort();
    }
    std::vector<int32_t> wdp_lens; // --window-depth: the contigs' lengths as this header gives them (every worker of --gpus N takes them from its own copy)
    if (mod.window_depth) {
        uint64_t NW = 0;
        for (const uint32_t len : rd.header().ref_lens) {
            wdp_lens.push_back((int32_t)std::min<uint32_t>(len, 0x7FFFFFFFu));
            NW += ((uint64_t)len + mod.window_depth_size - 1) / mod.window_depth_size;
        }
        const uint64_t lanes = std::max(1u, rd.header().lane_count);
        if (lanes * (4 + 3 * NW) > 1ull << 28) { // said here in the option's terms, before the output file is opened
            fprintf(stderr, "ERROR: %s: %llu windows of %u bases x 3 planes x %llu read groups are more than 268435456 (2^28) words; --window-depth-size wants a larger window for this header\n",
                    opt.bamFile.c_str(), (unsigned long long)NW, (uint32_t)mod.window_depth_size, (unsigned long long)lanes);
            return shard_abort();
        }
    }
    if (!shard || shard->index == 0) {
        FILE* of = fopen(opt.outputFile.c_str(), "wb"); // opened (truncated) before the scan, :278-283
        if (!of) { fprintf(stderr, "ERROR: Could not open output file %s\n", opt.outputFile.c_str()); return shard_abort(); }
        fclose(of);
    }
    const BamHeader& H = rd.header();
    const uint32_t n_refs = (uint32_t)H.ref_names.size();
    // initChroms (:106-123): names that are not BAM references are silently dropped
    std::vector<uint8_t> main_chrom(std::max(1u, n_refs), 0);
    {
        size_t p = 0;
        while (p <= opt.chroms.size()) {
            size_t e = opt.chroms.find(',', p);
            if (e == std::string::npos) e = opt.chroms.size();
            const std::string name = opt.chroms.substr(p, e - p);
            for (uint32_t r = 0; r < n_refs; ++r) if (H.ref_names[r] == name) { main_chrom[r] = 1; break; }
            p = e + 1;
        }
    }
    rd.set_main_chrom(main_chrom);
    since_launch("input opened, header read");
    // --site-alleles: the sites as this header numbers the contigs (every worker of --gpus N loads the list itself)
    std::vector<int32_t> site_rid, site_pos;
    if (!opt.site_alleles.empty()) {
        if (S && S->sites_loaded && S->sites_names == H.ref_names && S->sites_lens == H.ref_lens) { site_rid = S->sites_rid; site_pos = S->sites_pos; }
        else {
            std::vector<const char*> names;
            for (const auto& nm : H.ref_names) names.push_back(nm.c_str());
            uint32_t n_sites = 0;
            int32_t *sr = nullptr, *sp = nullptr;
            uint64_t given = 0, unnamed = 0;
            char serr[1024];
            if (bqc_sites_load(opt.site_alleles.c_str(), names.data(), H.ref_lens.data(), n_refs, &n_sites, &sr, &sp, &given, &unnamed, serr, sizeof serr)) {
                fprintf(stderr, "ERROR: %s\n", serr);
                return shard_abort();
            }
            site_rid.assign(sr, sr + n_sites);
            site_pos.assign(sp, sp + n_sites);
            bqc_sites_free(sr, sp);
            if (unnamed && !host_reader_only && (!shard || shard->index == 0))
                fprintf(stderr, "bamqualcheck: %llu of %llu sites of %s lie on contigs the header does not name\n", (unsigned long long)unnamed, (unsigned long long)given, opt.site_alleles.c_str());
            if (S) { S->sites_loaded = true; S->sites_names = H.ref_names; S->sites_lens = H.ref_lens; S->sites_rid = site_rid; S->sites_pos = site_pos; }
        }
    }
    // --regions: the regions as this header numbers the contigs (every worker of --gpus N loads the list itself)
    std::vector<int32_t> region_rid, region_start, region_end;
    if (!opt.regions.empty()) {
        if (S && S->regions_loaded && S->regions_names == H.ref_names && S->regions_lens == H.ref_lens) { region_rid = S->regions_rid; region_start = S->regions_start; region_end = S->regions_end; }
        else {
            std::vector<const char*> names;
            for (const auto& nm : H.ref_names) names.push_back(nm.c_str());
            uint32_t n_regions = 0;
            int32_t *rr = nullptr, *rs = nullptr, *re = nullptr;
            uint64_t given = 0, unnamed = 0, merged = 0;
            char rerr[1024];
            if (bqc_regions_load(opt.regions.c_str(), names.data(), H.ref_lens.data(), n_refs, &n_regions, &rr, &rs, &re, &given, &unnamed, &merged, rerr, sizeof rerr)) {
                fprintf(stderr, "ERROR: %s\n", rerr);
                return shard_abort();
            }
            region_rid.assign(rr, rr + n_regions);
            region_start.assign(rs, rs + n_regions);
            region_end.assign(re, re + n_regions);
            bqc_regions_free(rr, rs, re);
            if (!host_reader_only && (!shard || shard->index == 0)) {
                if (unnamed) fprintf(stderr, "bamqualcheck: %llu of %llu regions of %s lie on contigs the header does not name\n", (unsigned long long)unnamed, (unsigned long long)given, opt.regions.c_str());
                if (merged) fprintf(stderr, "bamqualcheck: %llu regions of %s overlap or abut their predecessor and were merged with it: %u regions are left\n", (unsigned long long)merged, opt.regions.c_str(), n_regions);
            }
            if (S) { S->regions_loaded = true; S->regions_names = H.ref_names; S->regions_lens = H.ref_lens; S->regions_rid = region_rid; S->regions_start = region_start; S->regions_end = region_end; }
        }
    }
    const auto t_begin = std::chrono::steady_clock::now(); // (BQC_TIMING=1 also reports the phases around the record loop)
    auto secs = [](clk::time_point a, clk::time_point b) { return std::chrono::duration<double>(b - a).count(); };
    double t_wait = 0, t_submit = 0, t_decode = 0;
    uint64_t n_total = 0;
    // decode thread feeds batches; this thread submits them.  It starts right away: the first batches are inflated and
    // decoded while the FASTA file is read and the device is set up.
    BatchQueue Q;
    // a session's batch objects: taken here, given back on every way out (their device buffers return to the readers' pool, where the
    // next file's reader counts them)
    struct SpareLoan {
        BatchQueue& Q; Session* S; bool given = false;
        void give()
        {
            if (!S || given) return;
            given = true;
            std::lock_guard<std::mutex> lk(Q.m);
            for (auto& hb : Q.spare) {
                if (hb->dev_mem && hb->dev_free) { hb->dev_free(hb->dev_mem); hb->dev_mem = nullptr; hb->dev_cap = 0; }
                if (S->spare.size() < 8) S->spare.push_back(std::move(hb));
            }
            Q.spare.clear();
        }
        ~SpareLoan() { give(); }
    } spare_loan{Q, S};
    size_t n_spare_kept = 0;
    if (S) { n_spare_kept = S->spare.size(); Q.spare = std::move(S->spare); S->spare.clear(); }
    struct ReaderEnd { GpuBamReader& r; bool on; ~ReaderEnd() { if (on) r.end_file(); } } reader_end{gpu_rd, S && bam_on_card}; // (the file is over on every way out)
    std::atomic<bool> gpu_reader_opened{false};
    std::thread dec;
    auto stop_decoder = [&]() {
        if (!dec.joinable()) return;
        { std::lock_guard<std::mutex> lk(Q.m); Q.stop = true; }
        Q.cv.notify_all();
        dec.join();
    };
    if (H.lane_count != 0) dec = std::thread([&]() {
        if (route_on_card(rt)) { // the device side of the reader opens here, beside the FASTA file and the context
            std::string e;
            int code = 0;
            const bool ok = in.start_card(opt.device, opt.batch_reads, 256ull << 20, e, code);
            gpu_reader_opened = true; // (the context is created after this: see there)
            if (!ok) {
                std::lock_guard<std::mutex> lk(Q.m);
                Q.err = e; Q.err_code = code; Q.done = true; Q.cv.notify_all();
                return;
            }
            rd.set_main_chrom(main_chrom);
        }
        for (;;) {
            std::unique_ptr<HostBatch> hb;
            {
                std::lock_guard<std::mutex> lk(Q.m);
                if (!Q.spare.empty()) { hb = std::move(Q.spare.back()); Q.spare.pop_back(); }
            }
            if (!hb) hb = std::make_unique<HostBatch>();
            int code = 0;
            std::string e;
            const auto d0 = clk::now();
            const int r = rd.next_batch(*hb, opt.batch_reads, 256ull << 20, e, code);
            t_decode += secs(d0, clk::now());
            std::unique_lock<std::mutex> lk(Q.m);
            if (r < 0) { Q.err = e; Q.err_code = code; Q.done = true; Q.cv.notify_all(); return; }
            if (r == 0) { Q.done = true; Q.cv.notify_all(); return; }
            Q.cv.wait(lk, [&] { return Q.q.size() < 3 || Q.stop; });
            if (Q.stop) return;
            Q.q.push_back(std::move(hb));
            Q.cv.notify_all();
        }
    });
    if (H.lane_count == 0) { // no @RG: counts is empty; any record is an error, none means an empty output file
        std::vector<FastaRecord> fa0;
        std::string ferr0;
        if (!load_fasta(opt.referenceFile.c_str(), &H.ref_names, fa0, ferr0)) fprintf(stderr, "%s\n", ferr0.c_str()); // return value ignored (:291)
        HostBatch hb;
        int code = 0;
        const int rc = rd.next_batch(hb, 1, 1 << 20, err, code);
        if (rc != 0) { fprintf(stderr, "%s\n", rc < 0 ? err.c_str() : "ERROR: records present but the header has no @RG line"); return shard_abort(); }
        if (shard) { bqc_shard_info si{}; bqc_shard_result sr{}; (void)shard->hook(shard->user, &si, &sr); } // (nothing to merge: no counters at all)
        return 0;
    }
    // the context is created (device memory, streams, sketch tables: ~0.1 s) by a thread of its own while this one reads the FASTA file
    bqc_options bo;
    memset(&bo, 0, sizeof bo);
    bo.struct_size = sizeof bo;
    bo.n_lanes = H.lane_count; bo.n_refs = n_refs; bo.isize = opt.isize;
    bo.max_read_len = opt.max_read_len; bo.hist_cap = opt.hist_cap;
    bo.main_chrom = main_chrom.data(); bo.fasta_index = nullptr; bo.device = opt.device; // (FASTA order: bqc_set_fasta_index below)
    bo.shard_tail = shard && shard->index > 0 ? 1u : 0u;
    bo.qual_by_cycle = (uint32_t)mod.qual_by_cycle;
    bo.mismatch_by_cycle = (uint32_t)mod.mismatch_by_cycle;
    if (!opt.no_sketch) {
        bo.sketch.n_k = (uint32_t)opt.klist.size(); bo.sketch.klist = opt.klist.data();
        bo.sketch.n_q = (uint32_t)opt.q_cutoff.size(); bo.sketch.qlist = opt.q_cutoff.data();
        bo.sketch.e = opt.e; bo.sketch.seed = opt.seed;
    }
    // the modules beside bqc_options (bqc_create_ex): adapter content by cycle
    std::vector<bqc_adapter> adp_set;
    for (const auto& ad : opt.adapters) adp_set.push_back(bqc_adapter{ad.first.c_str(), ad.second.c_str()});
    bqc_modules bm;
    memset(&bm, 0, sizeof bm);
    bm.struct_size = sizeof bm;
    bm.adapter_by_cycle = (uint32_t)mod.adapter_by_cycle;
    bm.n_adapters = (uint32_t)adp_set.size(); bm.adapters = adp_set.empty() ? nullptr : adp_set.data();
    bqc_ctx* ctx = nullptr;
    int rc = 0;
    std::string create_err;
    double t_create_s = 0, t_c_warm = 0, t_c_reader = 0, t_c_create = 0;
    // A session: the contigs on the card stay when this job names the same genome (same FASTA file, same @SQ lines); the context stays
    // — bqc_reset — when the options that size it are the same as well; another context over the same genome takes the contigs over
    // (bqc_move_references).  Another genome: the old context goes first, with its contigs, and everything is as in a single run.
    RefKey ref_key;
    CtxKey ctx_key;
    bool refs_kept = false, ctx_kept = false;
    if (S) {
        ref_key = make_ref_key(opt.referenceFile, H);
        ctx_key.mod = settings_in_use(mod, !site_rid.empty(), !region_rid.empty());
        ctx_key.adapters = opt.adapters;
        ctx_key.site_rid = site_rid; ctx_key.site_pos = site_pos; ctx_key.region_rid = region_rid; ctx_key.region_start = region_start; ctx_key.region_end = region_end; // (empty where the module is off)
        ctx_key.window_depth_lens = wdp_lens; ctx_key.main_chrom = main_chrom;
        ctx_key.n_lanes = bo.n_lanes; ctx_key.n_refs = bo.n_refs; ctx_key.max_read_len = bo.max_read_len; ctx_key.hist_cap = bo.hist_cap; ctx_key.isize = bo.isize; ctx_key.device = bo.device;
        ctx_key.sketch = !opt.no_sketch;
        if (!opt.no_sketch) { ctx_key.klist = opt.klist; ctx_key.qlist = opt.q_cutoff; ctx_key.e = opt.e; ctx_key.seed = opt.seed; }
        refs_kept = S->ctx && ref_key == S->ref_key;
        ctx_kept = refs_kept && ctx_key == S->ctx_key;
    }
    const uint32_t contigs_before = refs_kept ? S->contigs_on_card : 0;
    std::thread creator([&] {
        if (ctx_kept) {
            const auto c0 = clk::now();
            ctx = S->ctx; S->ctx = nullptr;
            rc = bqc_reset(ctx);
            if (rc) create_err = bqc_last_error(ctx);
            t_create_s = t_c_create = secs(c0, clk::now());
            return;
        }
        bqc_ctx* old = nullptr;
        if (S) {
            old = S->ctx; S->ctx = nullptr;
            if (old && !refs_kept) { bqc_destroy(old); old = nullptr; S->ref_key = RefKey(); S->contigs_on_card = 0; }
        }
        const auto c0 = clk::now();
        // Who sets up when (round 4): the warm-up thread starts the runtime (~60 ms) and then makes the program's four streams one after the
        // other (20 + 3 x 8-10 ms: hardware queues, serial whoever asks); the reader allocates its buffers as soon as the runtime is up
        // and takes the SECOND stream; the context is created here as soon as the FIRST stream exists — a few milliseconds of allocations
        // and memsets, behind the reader's allocations by then (side by side the two were measured to hold each other up at the runtime's
        // locks in round 3, when each also made its own streams and the reader page-locked 96 MB with hipHostMalloc) — and the references
        // go to the card while the reader still waits for its stream.
        const auto c1 = clk::now();
        const auto c2 = clk::now();
        rc = mod.adapter_by_cycle ? bqc_create_ex(&bo, &bm, &ctx) : bqc_create(&bo, &ctx);
        if (rc) create_err = bqc_last_error(nullptr);
        else { // the modules that are switched on right behind the creation, to the first that fails
            const auto u32 = [](uint64_t x) { return (uint32_t)x; }; // (the parser's bounds keep every such word below 2^32)
            if (mod.gc_bias) rc = bqc_enable_gc_bias(ctx, u32(mod.gc_bias));
            if (!rc && mod.indel_by_cycle) rc = bqc_enable_indel_by_cycle(ctx, u32(mod.indel_by_cycle));
            if (!rc && mod.substitutions) rc = bqc_enable_substitutions(ctx, u32(mod.substitutions), u32(mod.subst_min_qual), u32(mod.subst_min_mapq));
            if (!rc && !site_rid.empty()) rc = bqc_enable_site_alleles(ctx, (uint32_t)site_rid.size(), site_rid.data(), site_pos.data(), u32(mod.site_min_qual), u32(mod.site_min_mapq));
            if (!rc && !region_rid.empty())
                rc = bqc_enable_region_coverage(ctx, (uint32_t)region_rid.size(), region_rid.data(), region_start.data(), region_end.data(), u32(mod.regions_min_mapq),
                                                u32(mod.n_regions_thresholds), mod.regions_thresholds, u32(mod.regions_depth_cap));
            if (!rc && mod.duplicate_sets) rc = bqc_enable_duplicate_sets(ctx, mod.duplicate_sets_capacity);
            if (!rc && mod.overrepresented) rc = bqc_enable_overrepresented(ctx, u32(mod.overrepresented_len), u32(mod.overrepresented_ppm), mod.overrepresented_capacity);
            if (!rc && mod.window_depth) rc = bqc_enable_window_depth(ctx, u32(mod.window_depth_size), wdp_lens.data(), u32(mod.window_depth_min_mapq));
            if (rc) create_err = bqc_last_error(ctx);
        }
        if (!rc && old) { // the same genome under another context: its contigs change owner, nothing is uploaded
            rc = bqc_move_references(old, ctx);
            if (rc) create_err = bqc_last_error(ctx);
        }
        else if (!rc && !shard) { // one allocation for the contigs, sized from the BAM header, while nothing runs on the card yet (an allocation beside running kernels waits for them)
            uint64_t total = 0;
            for (uint32_t r = 0; r < n_refs; ++r) total += H.ref_lens[r];
            (void)bqc_reserve_references(ctx, total, n_refs);
        }
        if (old) { bqc_destroy(old); if (rc) { S->ref_key = RefKey(); S->contigs_on_card = 0; } }
        t_create_s = secs(c0, clk::now());
        t_c_warm = secs(c0, c1); t_c_reader = secs(c1, c2); t_c_create = secs(c2, clk::now());
    });
    // reference genome: all contigs that are BAM references, FASTA order kept for the cursor rule
    // One of several processes over a file needs the contigs ITS records lie on, not the genome: the FASTA file is only indexed
    // here (where its records are), and a contig is encoded and uploaded when the first batch with a read on it arrives
    // (ensure_refs below) — eight workers parsing 3 GB of text each on shared host cores would cost more than their record loops.
    std::vector<FastaRecord> fa;
    std::string ferr;
    MappedFasta lazy_fa;
    const bool lazy_refs = shard && !(getenv("BQC_EAGER_REFS") && getenv("BQC_EAGER_REFS")[0] == '1') && lazy_fa.open(opt.referenceFile.c_str()) == 1;
    if (lazy_refs) { for (const auto& r : lazy_fa.recs) fa.push_back(FastaRecord{r.name, {}}); }
    else if (refs_kept) {} // (a session: the contigs are on the card, the file is neither parsed nor uploaded again)
    else if (!load_fasta(opt.referenceFile.c_str(), &H.ref_names, fa, ferr)) fprintf(stderr, "%s\n", ferr.c_str()); // return value ignored (:291)
    std::vector<int32_t> fasta_index(std::max(1u, n_refs), -1);
    if (refs_kept) fasta_index = S->fasta_index;
    else for (uint32_t r = 0; r < n_refs; ++r)
        for (size_t i = 0; i < fa.size(); ++i) if (fa[i].name == H.ref_names[r]) { fasta_index[r] = (int32_t)i; break; }
    const auto t_fasta = clk::now();
    creator.join();
    // The reader may launch its first inflate kernel once the context exists AND its own set-up is done (it is still waiting for its
    // stream at this point, as a rule): a thread of its own says so, this one goes on to the references.
    std::thread allow_thr;
    struct AllowJoiner { std::thread& t; ~AllowJoiner() { if (t.joinable()) t.join(); } } allow_joiner{allow_thr};
    if (route_on_card(rt)) allow_thr = std::thread([&gpu_reader_opened, &in, ctx, rc] {
        while (!gpu_reader_opened.load()) std::this_thread::sleep_for(std::chrono::microseconds(100));
        in.allow(rc ? nullptr : ctx); // (the context exists: the card may get busy)
    });
    const auto t_create = clk::now();
    // where a context goes on every way out: back to the session (the next job resets it, or takes its contigs, or destroys it)
    auto give_ctx = [&]() { if (!ctx) return; if (S) { S->ctx = ctx; S->ctx_key = ctx_key; } else bqc_destroy(ctx); ctx = nullptr; };
    if (rc) { note_rc(rc); fprintf(stderr, "ERROR: %s\n", create_err.c_str()); stop_decoder(); give_ctx(); return shard_abort(); }
    if (!ctx_kept && (rc = bqc_set_fasta_index(ctx, fasta_index.data()))) { note_rc(rc); fprintf(stderr, "ERROR: %s\n", bqc_last_error(ctx)); stop_decoder(); give_ctx(); return shard_abort(); }
    // The references go to the card BEHIND the start of the record loop: a thread of its own uploads the contigs in the BAM header's order
    // (a human genome is 3.1 GB: 0.35-0.45 s that the loop used to wait for) and the submitting thread only waits when a batch holds a
    // read on a contig that is not there yet — the first one, as a rule.  (bqc_set_reference may be called beside bqc_submit* for contigs
    // no submitted batch refers to: include/bamqc.h.)
    std::vector<uint8_t> ref_loaded(std::max(1u, n_refs), 0); // lazy_refs: 1 loaded; background upload: see ref_state
    std::unique_ptr<std::atomic<uint8_t>[]> ref_state(new std::atomic<uint8_t>[std::max(1u, n_refs)]); // 0 on its way, 1 on the card, 2 failed
    for (uint32_t r = 0; r < std::max(1u, n_refs); ++r) ref_state[r] = 0;
    std::mutex ref_m;
    std::condition_variable ref_cv;
    std::string ref_err;
    std::atomic<bool> ref_stop{false};
    std::thread ref_loader;
    const bool bg_refs = !lazy_refs;
    // BQC_BG_REFS=1: the uploader runs BESIDE the record loop (which then starts 0.35 s earlier).  Measured on a 100 M-read file over a
    // human-sized genome: the loop itself becomes 0.5-0.6 s longer (1.45-1.55 s against 0.9), from pageable and from page-locked memory
    // alike — page-locking and large copies beside running inflate kernels hold up the other threads' calls into the runtime — so by
    // default the uploader is waited for before the loop starts; what is kept of it: one allocation for all contigs, made with the context.
    const bool refs_beside_loop = bg_refs && getenv("BQC_BG_REFS") && getenv("BQC_BG_REFS")[0] == '1';
    std::atomic<bool> ref_skipped{false}; // the uploader was stopped before a contig of the FASTA file: the genome on the card is not whole
    auto upload_all = [&] {
        for (uint32_t r = 0; r < n_refs; ++r) {
            uint8_t st = 1;
            if (fasta_index[r] >= 0 && ref_stop.load()) ref_skipped = true;
            if (fasta_index[r] >= 0 && !ref_stop.load()) {
                auto& c = fa[fasta_index[r]].codes;
                // (from pageable memory: page-locking the 3.1 GB first — hipHostRegister — and copying at the link's speed measured SLOWER
                // for the whole genome, 0.63-0.82 s against 0.35-0.46 s)
                const int src = bqc_set_reference(ctx, (int32_t)r, c.data(), c.size());
                if (src) { note_rc(src); std::lock_guard<std::mutex> lk(ref_m); if (ref_err.empty()) ref_err = bqc_last_error(ctx); st = 2; }
                // (the host copy is NOT given back here: returning a human genome's 3.1 GB to the kernel costs 0.35-0.4 s — measured:
                // "references" 0.57 s with the contigs freed one by one, 0.20 s without — and the program's exit does it for nothing)
            }
            { std::lock_guard<std::mutex> lk(ref_m); ref_state[r] = st; }
            ref_cv.notify_all();
        }
    };
    if (refs_kept) { for (uint32_t r = 0; r < n_refs; ++r) ref_state[r] = 1; } // (a session: they are there)
    else if (bg_refs && refs_beside_loop) ref_loader = std::thread(upload_all);
    else if (bg_refs) upload_all(); // (in this thread, before the loop: the default)
    auto note_refs = [&]() { // a session remembers which genome its context holds, once every contig of it has arrived
        if (!S || refs_kept || !bg_refs) return;
        std::lock_guard<std::mutex> lk(ref_m);
        if (!ref_err.empty() || !ref_key.valid || ref_skipped.load()) return; // (BQC_BG_REFS=1: contigs no read asked for may have been left out)
        for (uint32_t r = 0; r < n_refs; ++r) if (ref_state[r].load() != 1) return;
        S->ref_key = ref_key; S->fasta_index = fasta_index; S->contigs_on_card = 0;
        for (uint32_t r = 0; r < n_refs; ++r) S->contigs_on_card += fasta_index[r] >= 0;
    };
    auto destroy_ctx = [&]() { // (every way out: the uploader first, it uses the context)
        ref_stop = true;
        if (ref_loader.joinable()) ref_loader.join();
        note_refs();
        give_ctx();
    };
    std::vector<raw_vector<uint8_t>> uploaded_codes; // (lazy_refs) host copies of contigs that are on the card: kept, see above
    double t_lazy_refs = 0;
    uint32_t n_lazy_refs = 0;
    double t_wait_refs = 0;
    std::vector<int32_t> rid_range; // (a batch whose columns stayed on the card names the range of its reference ids)
    auto ensure_refs = [&](const HostBatch& hb) -> int { // the contigs this batch's reads lie on are on the card before it is submitted
        const int32_t* rid_begin = hb.rid.data();
        const int32_t* rid_end = hb.rid.data() + hb.rid.size();
        if (hb.anchored) {
            rid_range.clear();
            for (int32_t r = hb.rid_min; r <= hb.rid_max; ++r) rid_range.push_back(r);
            rid_begin = rid_range.data(); rid_end = rid_range.data() + rid_range.size();
        }
        if (bg_refs) { // wait for the uploader where it has not got to yet
            int32_t last = -1;
            for (const int32_t* q = rid_begin; q != rid_end; ++q) {
                const int32_t rid = *q;
                if (rid == last || rid < 0 || (uint32_t)rid >= n_refs) continue;
                last = rid;
                if (ref_state[rid].load() == 1) continue;
                const auto w0 = clk::now();
                std::unique_lock<std::mutex> lk(ref_m);
                ref_cv.wait(lk, [&] { return ref_state[rid].load() != 0; });
                t_wait_refs += secs(w0, clk::now());
                if (ref_state[rid].load() == 2) { fprintf(stderr, "ERROR: %s\n", ref_err.c_str()); return 1; }
            }
            return 0;
        }
        std::vector<size_t> which;
        std::vector<uint32_t> rids;
        int32_t last = -1;
        for (const int32_t* q = rid_begin; q != rid_end; ++q) {
            const int32_t rid = *q;
            if (rid == last || rid < 0 || (uint32_t)rid >= n_refs) continue;
            last = rid;
            if (ref_loaded[rid] || fasta_index[rid] < 0) continue;
            ref_loaded[rid] = 1;
            which.push_back((size_t)fasta_index[rid]);
            rids.push_back((uint32_t)rid);
        }
        if (which.empty()) return 0;
        const auto l0 = clk::now();
        std::vector<raw_vector<uint8_t>> codes(which.size());
        std::vector<raw_vector<uint8_t>*> dst;
        for (auto& c : codes) dst.push_back(&c);
        if (!lazy_fa.encode(which, dst)) { fprintf(stderr, "ERROR: out of memory while loading %s\n", opt.referenceFile.c_str()); return 1; }
        for (size_t k = 0; k < rids.size(); ++k)
            if (bqc_set_reference(ctx, (int32_t)rids[k], codes[k].data(), codes[k].size())) { fprintf(stderr, "ERROR: %s\n", bqc_last_error(ctx)); return 1; }
        for (auto& c : codes) uploaded_codes.push_back(std::move(c));
        t_lazy_refs += secs(l0, clk::now());
        n_lazy_refs += (uint32_t)rids.size();
        return 0;
    };
    const auto t_setup = clk::now();
    since_launch("record loop starts");

    int status = 0;
    uint64_t n_noqual_deferred = 0;
    const bool pinned = !(getenv("BQC_NO_PINNED") && getenv("BQC_NO_PINNED")[0] == '1'); // (1: the staging path of bqc_submit, for comparison)
    if (pinned) bqc_raw_vector_free_hook = pin_free_hook;
    struct InFlight { uint64_t ticket; std::unique_ptr<HostBatch> hb; };
    std::deque<InFlight> inflight; // batches whose columns the device may still be reading
    auto recycle = [&](bool wait_all) {
        while (!inflight.empty()) {
            const int up = bqc_batch_uploaded(ctx, inflight.front().ticket, wait_all || inflight.size() > 3 ? 1 : 0);
            if (up == 0) break;
            std::lock_guard<std::mutex> lk(Q.m);
            if (Q.spare.size() < 8) Q.spare.push_back(std::move(inflight.front().hb));
            inflight.pop_front();
        }
    };
    for (;;) {
        std::unique_ptr<HostBatch> hb;
        const auto w0 = clk::now();
        {
            std::unique_lock<std::mutex> lk(Q.m);
            Q.cv.wait(lk, [&] { return !Q.q.empty() || Q.done; });
            if (Q.q.empty()) break;
            hb = std::move(Q.q.front());
            Q.q.pop_front();
            Q.cv.notify_all();
        }
        if (status) continue; // drain
        { // check_read_len (QualityCheck.hpp:70-79, called at bamqualcheck.cpp:357,378; return value ignored): one line per primary
          // record with a first / last flag whose quality string is empty while its sequence is not
            size_t n_noqual = hb->anchored ? hb->n_noqual : 0; // (a batch whose columns stayed on the card: counted there)
            for (uint16_t f : hb->flag) n_noqual += (f & BQC_FLAG_NO_QUAL) && !(f & 0x900) && (f & 0xC0);
            // (the reader on the card: printed once the pass is known to be the one that counts — it may still hand the file over to the host
            // reader, which then prints them itself — i.e. behind the loop and in front of a record error: the lines of the batches BEFORE
            // a failing record all come first, where the reference interleaves them with nothing either; the failing batch's own lines
            // are the host decoder's to print)
            if (bam_on_card) { n_noqual_deferred += n_noqual; n_noqual = 0; }
            if (n_noqual) {
                static const char msg[] = "ERROR: length of sequence and quality is not the same\n";
                std::string out;
                out.reserve(std::min<size_t>(n_noqual, 4096) * (sizeof msg - 1));
                for (size_t k = 0; k < n_noqual; ++k) {
                    out.append(msg, sizeof msg - 1);
                    if (out.size() >= 4096 * (sizeof msg - 1)) { fwrite(out.data(), 1, out.size(), stderr); out.clear(); }
                }
                fwrite(out.data(), 1, out.size(), stderr);
            }
        }
        if (ensure_refs(*hb)) { status = 1; continue; }
        const bqc_batch v = hb->view();
        const auto s0 = clk::now();
        t_wait += secs(w0, s0);
        n_total += v.n_reads;
        if (pinned || hb->d_seq) { // (BQC_NO_PINNED=1 is about host columns: a payload that lives on the card can only be taken from there)
            if (!hb->d_seq) pin_batch(*hb); // (a batch decoded on the card: its payload is there already, its small fixed columns are copied staged)
            uint64_t ticket = 0;
            if (hb->anchored) { rc = bqc_submit_anchored(ctx, &v, (bqc_anchored*)hb->anchored, &ticket); hb->anchored = nullptr; }
            else rc = bqc_submit_async(ctx, &v, &ticket);
            if (rc) { note_rc(rc); fprintf(stderr, "%s\n", bqc_last_error(ctx)); status = 1; }
            inflight.push_back(InFlight{ticket, std::move(hb)});
            recycle(false);
        } else {
            if ((rc = bqc_submit(ctx, &v))) { note_rc(rc); fprintf(stderr, "%s\n", bqc_last_error(ctx)); status = 1; }
            std::lock_guard<std::mutex> lk(Q.m); // (bqc_submit has staged the batch)
            if (Q.spare.size() < 4) Q.spare.push_back(std::move(hb));
        }
        t_submit += secs(s0, clk::now());
    }
    recycle(true);
    ref_stop = true; // (contigs no read has asked for are not waited for)
    if (ref_loader.joinable()) ref_loader.join();
    if (!status && (rc = bqc_sync(ctx))) { note_rc(rc); fprintf(stderr, "%s\n", bqc_last_error(ctx)); status = 1; } // what the device found in the last batches
    dec.join();
    if (S && bam_on_card) gpu_rd.end_file(); // (its threads are gone and its streams idle: what it holds can be told, and the next file may open it)
    note_rc(Q.err_code);
    if (timing) fprintf(stderr, "[timing] records decoded %s\n", bam_on_card ? "on the GPU (csrc/gpu_bam.hip)" : rt.reader == RD_GPU_SAM_BGZF ? "on the GPU (csrc/gpu_inflate.hip + csrc/gpu_sam.hip)" : rt.reader == RD_GPU_SAM ? "on the GPU (csrc/gpu_sam.hip)" : "on the host");
    if (timing) { // (every buffer of the run exists at this point: what is in use now is the run's peak)
        size_t free_b = 0, total_b = 0, pinned = 0;
        { std::lock_guard<std::mutex> lk(g_pins.m); for (auto& kv : g_pins.blocks) pinned += kv.second; }
        if (hipMemGetInfo(&free_b, &total_b) == hipSuccess)
            fprintf(stderr, "[timing] device memory in use at the end of the record loop: %.2f GB of %.0f GB; page-locked decode buffers %.2f GB\n", (total_b - free_b) / 1e9, total_b / 1e9, pinned / 1e9);
    }
    if (timing && refs_beside_loop) fprintf(stderr, "[timing] references uploaded beside the record loop; the submitting thread waited %.3f s for them\n", t_wait_refs);
    if (timing && lazy_refs) fprintf(stderr, "[timing] %u of %u contigs loaded, when their first reads arrived: %.3f s\n", n_lazy_refs, n_refs, t_lazy_refs);
    if (timing && bam_on_card) fprintf(stderr, "[timing] %llu batches anchored on the card (fixed columns never on the host) of %llu batches\n", (unsigned long long)gpu_rd.batches_anchored(), (unsigned long long)gpu_rd.batches());
    if (timing && bam_on_card)
        fprintf(stderr, rt.stream ? "[timing] reader on the card: a stream, read() and waiting for it %.2f s in its one reader thread, the producer waited %.2f s for chunks, the decode thread waited %.2f s for inflated runs\n"
                                   : "[timing] reader on the card: pread %.2f s summed over its reader threads, the producer waited %.2f s for them, the decode thread waited %.2f s for inflated runs\n",
                gpu_rd.seconds_reading(), gpu_rd.seconds_producer_waiting_for_chunks(), gpu_rd.seconds_waiting_for_runs());
    if (timing && rt.reader == RD_GPU_SAM_BGZF)
        fprintf(stderr, "[sam reader] text inflated on the card: %s %.2f s in the producer's reader thread%s, the producer waited %.2f s for chunks, the decode thread waited %.2f s for inflated runs\n",
                rt.stream ? "a stream, read() and waiting for it" : "pread", gsam_rd.seconds_producer_reading(), rt.stream ? "" : "s (summed)", gsam_rd.seconds_producer_waiting_for_chunks(), gsam_rd.seconds_waiting_for_runs());
    if (timing && route_any_gsam(rt)) {
        fprintf(stderr, "[sam reader] %llu batches on the card, %llu handed over, %llu anchored\n", (unsigned long long)gsam_rd.batches(), (unsigned long long)gsam_rd.batches_handed_over(),
                (unsigned long long)gsam_rd.batches_anchored());
        fprintf(stderr, "[sam reader] read() %.3f s in the reader thread; the decode thread waited %.3f s for input, copied text for %.3f s, ran kernels for %.3f s\n", gsam_rd.seconds_reading(),
                gsam_rd.seconds_waiting_for_input(), gsam_rd.seconds_copying(), gsam_rd.seconds_in_kernels());
    }
    if (timing && bam_on_card && gpu_rd.batches_handed_over()) fprintf(stderr, "[timing] %llu batches held records the card does not decode and went through the host decoder\n", (unsigned long long)gpu_rd.batches_handed_over());
    if (timing)
        fprintf(stderr, "[timing] %llu records: decode thread busy %.2f s, submit thread (host pass + enqueue; page-locking %.2f s) %.2f s, waiting for the decoder %.2f s, loop %.2f s\n",
                (unsigned long long)n_total, t_decode, g_pins.t_register, t_submit, t_wait, secs(t_setup, clk::now()));
    if (Q.err_code == GpuBamReader::kUnsupported && rt.stream) { // (cannot happen: the reader decides a stream's records itself — and there is no second pass over a stream)
        fprintf(stderr, "ERROR: internal error: the reader on the card gave up a stream (%s)\n", Q.err.c_str());
        Q.err_code = 0; status = 1;
    }
    if (Q.err_code == GpuBamReader::kUnsupported && status) Q.err_code = 0; // (an error of the records before it has been reported: that is the run's result)
    if (Q.err_code == GpuBamReader::kUnsupported) { // nothing has been reported yet: the same file again, through the host reader
        if (timing) fprintf(stderr, "[timing] %s\n", Q.err.c_str());
        destroy_ctx();
        if (!S) g_pins.release_all();
        spare_loan.give();
        if (S && !S->started_over) { S->started_over = true; S->first_ctx_kept = ctx_kept; S->first_contigs = contigs_before; }
        return run_program(argc, argv, shard, true, S); // (a session: inside the job, with what the session holds)
    }
    if (timing && S) // what this job found in place: facts, told when everything it needed exists
        fprintf(stderr, "[timing] job %u of %u: context %s, %u of %u contigs already on the card, reader buffers %s\n", S->job, std::max(S->job, S->n_jobs), (S->started_over ? S->first_ctx_kept : ctx_kept) ? "kept" : "created",
                S->started_over ? S->first_contigs : contigs_before, n_refs, bam_on_card ? gpu_rd.buffers_report() : n_spare_kept ? "kept" : "new");
    for (uint64_t k = 0; k < n_noqual_deferred; ++k) fputs("ERROR: length of sequence and quality is not the same\n", stderr);
    if (!status && Q.err_code) {
        if (Q.err_code == BQC_ERR_IO) fprintf(stderr, "ERROR: Could not read record from BAM File %s\n", opt.bamFile.c_str()); // :308
        else fprintf(Q.err == "Read does not have Z" ? stdout : stderr, "%s\n", Q.err.c_str());
        status = 1;
    }
    // writeOutput iterates laneNames (std::map: lexicographic), including IDs inserted by getLane
    std::vector<const char*> names;
    std::vector<uint32_t> idx;
    for (auto& kv : rd.header().lane_names) { names.push_back(kv.first.c_str()); idx.push_back(kv.second); }
    if (shard) { // what needs the other processes: split check, coverage hand-over, sum of the state vectors, lane names
        bqc_shard_info si{};
        si.ctx = ctx; si.status = status;
        si.begin_block = in.range_begin_block(); si.end_block = in.range_end_block(); si.first = in.range_first(); si.over = in.range_over();
        si.sample_id = rd.header().sample_id.c_str();
        si.n_lane_names = (uint32_t)names.size(); si.lane_names = names.data(); si.lane_index = idx.data();
        bqc_shard_result sr{};
        const int verdict = shard->hook(shard->user, &si, &sr);
        if (verdict == BQC_SHARD_FALLBACK) { // the split could not be verified: the whole file again, in this process alone
            destroy_ctx();
            g_pins.release_all();
            return run_program(argc, argv, nullptr);
        }
        if (verdict != BQC_SHARD_WRITE) { destroy_ctx(); g_pins.release_all(); return verdict == BQC_SHARD_DONE && !status ? 0 : 1; }
        names.assign(sr.lane_names, sr.lane_names + sr.n_lane_names);
        idx.assign(sr.lane_index, sr.lane_index + sr.n_lane_names);
    }
    if (status) { destroy_ctx(); return 1; }
    const bqc_counts* counts = nullptr;
    const auto t_loop_end = clk::now();
    since_launch("record loop and its checks over");
    if ((rc = bqc_finalize(ctx, &counts))) { note_rc(rc); fprintf(stderr, "ERROR: %s\n", bqc_last_error(ctx)); destroy_ctx(); return 1; }
    const auto t_final = clk::now();
    bqc_header_info hi;
    hi.sample_id = rd.header().sample_id.c_str();
    hi.n_names = (uint32_t)names.size();
    hi.lane_names = names.data();
    hi.lane_index = idx.data();
    rc = bqc_write_bamqc(counts, &hi, opt.outputFile.c_str());
    // the modules' tables, each in a file of its own beside the .bamqc (the context still exists), in this order, to the first that fails
    std::vector<const char*> sac_names;
    for (const auto& nm : H.ref_names) sac_names.push_back(nm.c_str());
    struct ModuleFile { bool on; const char* suffix; std::function<int(const char*)> write; };
    const ModuleFile module_files[] = {
        {mod.qual_by_cycle != 0, ".qbc", [&](const char* p) { return bqc_write_qual_by_cycle(ctx, &hi, p); }},
        {mod.mismatch_by_cycle != 0, ".mbc", [&](const char* p) { return bqc_write_mismatch_by_cycle(ctx, &hi, p); }},
        {mod.adapter_by_cycle != 0, ".adp", [&](const char* p) { return bqc_write_adapter_by_cycle(ctx, &hi, p); }},
        {mod.gc_bias != 0, ".gcb", [&](const char* p) { return bqc_write_gc_bias(ctx, &hi, p); }},
        {mod.indel_by_cycle != 0, ".ibc", [&](const char* p) { return bqc_write_indel_by_cycle(ctx, &hi, p); }},
        {mod.substitutions != 0, ".sbc", [&](const char* p) { return bqc_write_substitutions(ctx, &hi, p); }},
        {!site_rid.empty(), ".sac", [&](const char* p) { return bqc_write_site_alleles(ctx, &hi, sac_names.data(), n_refs, p); }},
        {!region_rid.empty(), ".rcv", [&](const char* p) { return bqc_write_region_coverage(ctx, &hi, sac_names.data(), n_refs, p); }},
        {mod.duplicate_sets != 0, ".dup", [&](const char* p) { return bqc_write_duplicate_sets(ctx, &hi, p); }},
        {mod.window_depth != 0, ".wdp", [&](const char* p) { return bqc_write_window_depth(ctx, &hi, sac_names.data(), n_refs, p); }},
        {mod.overrepresented != 0, ".ovr", [&](const char* p) { return bqc_write_overrepresented(ctx, &hi, p); }},
    };
    std::string path = opt.outputFile; // the file last written: where rc, the one that failed
    for (const ModuleFile& f : module_files) {
        if (rc) break;
        if (!f.on) continue;
        path = opt.outputFile + f.suffix;
        rc = f.write(path.c_str());
    }
    const auto t_write = clk::now();
    // the program proper (tools/bamqualcheck.cpp sets BQC_FAST_EXIT) leaves without the static destructors of the HIP runtime:
    // the output file is complete and closed, the process is about to end anyway
    const bool fast_exit = !S && !rc && getenv("BQC_FAST_EXIT") && getenv("BQC_FAST_EXIT")[0] == '1'; // (a session: its owner leaves, behind the last job)
    const char* done_fd = fast_exit ? getenv("BQC_DONE_FD") : nullptr; // the front end (tools/bamqualcheck.cpp) waits for a byte there
    auto teardown = [&]() { // (device memory and page locks are released explicitly: left to the kernel's process teardown they cost 0.2 s more)
        destroy_ctx();
        if (!S) g_pins.release_all();
    };
    if (!done_fd) teardown();
    if (timing) {
        fprintf(stderr, "[timing] start-up: waiting for the HIP runtime %.3f s, then for the GPU reader's set-up %.3f s, bqc_create %.3f s\n", t_c_warm, t_c_reader, t_c_create);
        fprintf(stderr, "[timing] phases: FASTA %.2f s (context created meanwhile in %.2f s), context %.2f s, references %.2f s, record loop %.2f s, finalize %.2f s, write %.2f s, destroy %.2f s%s\n",
                secs(t_begin, t_fasta), t_create_s, secs(t_fasta, t_create), secs(t_create, t_setup), secs(t_setup, t_loop_end), secs(t_loop_end, t_final), secs(t_final, t_write),
                secs(t_write, clk::now()), done_fd ? " (the context is released after the run has been reported complete)" : "");
    }
    if (rc) { fprintf(stderr, "ERROR: Could not write output file %s\n", path.c_str()); return 1; }
    since_launch("done");
    if (fast_exit) { // the program proper leaves without the static destructors of the HIP runtime: the output file is complete and closed
        fflush(stdout); fflush(stderr);
        if (done_fd) { // nothing is printed from here on: the run is reported complete, then this process cleans up on its own
            const int fd = atoi(done_fd);
            const unsigned char st = 0;
            (void)prctl(PR_SET_PDEATHSIG, 0); // (the front end leaves now; this process still hands its memory back)
            if (write(fd, &st, 1) == 1) {
                close(fd);
                const int nul = open("/dev/null", O_WRONLY);
                if (nul >= 0) { dup2(nul, 1); dup2(nul, 2); }
            }
            teardown();
        }
        _exit(0);
    }
    return 0;
}

// ---------------------------------------------------------------------------------------------------
// one process, many files
// ---------------------------------------------------------------------------------------------------
extern "C" int bqc_session_open(int argc, const char** argv, bqc_session** out)
{
    if (!out || argc < 1 || !argv) return 1;
    *out = nullptr;
    ProgramOptions opt;
    std::string perr;
    const int pr = parse_args(argc, argv, opt, perr, true);
    if (pr == 1) fprintf(stderr, "%s\n", perr.c_str());
    if (pr != 0) return 1; // (help and version are the program's to answer, not a session's)
    bqc_session* S = new bqc_session();
    S->args.assign(argv, argv + argc);
    *out = S;
    return 0;
}

// The job's exit status, as the single run's; 2: not run — the session has ended on a HIP error (in an earlier job: the job that met
// the error is a failed one, 1).  The rule is enforced here and nowhere else: run_program only notes the error (note_rc).
extern "C" int bqc_session_run(bqc_session* S, const char* input, const char* output)
{
    if (!S || !input || !output) return 1;
    if (S->ended.load()) return 2;
    if (strcmp(input, "-") == 0) { fprintf(stderr, "bamqualcheck: a stream on stdin is not a job\n"); return 1; }
    ++S->job;
    S->started_over = false;
    std::vector<const char*> av;
    for (const std::string& a : S->args) av.push_back(a.c_str());
    av.push_back("-o"); av.push_back(output);
    const std::string in = input[0] == '-' ? std::string("./") + input : std::string(input); // (a path, whatever it starts with)
    av.push_back(in.c_str());
    return run_program((int)av.size(), av.data(), nullptr, false, S);
}

extern "C" void bqc_session_close(bqc_session* S)
{
    if (!S) return;
    delete S; // the context with its contigs, the reader's buffers, the batch objects
    g_pins.release_all();
}

// --manifest LIST: a loop over the three calls above.  The front end's early-exit byte (BQC_DONE_FD) goes out behind the LAST job, and
// the one teardown happens behind that byte.
static int run_manifest(int argc, const char** argv)
{
    ProgramOptions opt;
    std::string perr;
    const int pr = parse_args(argc, argv, opt, perr);
    if (pr == 2) return 0;
    if (pr == 1) { fprintf(stderr, "%s\n", perr.c_str()); return 1; }
    std::vector<const char*> av;
    for (int i = 0; i < argc; ++i) { // the session's options: everything but the list
        if (i > 0 && strcmp(argv[i], "--manifest") == 0) { ++i; continue; }
        if (i > 0 && strncmp(argv[i], "--manifest=", 11) == 0) continue;
        av.push_back(argv[i]);
    }
    bqc_session* S = nullptr;
    if (bqc_session_open((int)av.size(), av.data(), &S) != 0) return 1;
    S->n_jobs = (uint32_t)opt.jobs.size();
    const bool timing = getenv("BQC_TIMING") && getenv("BQC_TIMING")[0] == '1';
    int status = 0;
    for (size_t k = 0; k < opt.jobs.size(); ++k) {
        const int rc = bqc_session_run(S, opt.jobs[k].first.c_str(), opt.jobs[k].second.c_str());
        if (rc == 0) continue;
        status = 1;
        fflush(stdout);
        fprintf(stderr, "bamqualcheck: job %zu (%s): %s\n", k + 1, opt.jobs[k].first.c_str(), rc == 2 ? "not run" : "failed");
    }
    if (timing) { // what the session holds behind its last job
        size_t free_b = 0, total_b = 0, pinned = 0, rd_dev = 0, rd_pinned = 0;
        { std::lock_guard<std::mutex> lk(g_pins.m); for (auto& kv : g_pins.blocks) pinned += kv.second; }
        S->gpu_rd.memory_held(rd_dev, rd_pinned);
        if (!S->ended.load() && hipMemGetInfo(&free_b, &total_b) == hipSuccess)
            fprintf(stderr, "[timing] session after %zu jobs: device memory in use %.2f GB of %.0f GB (the reader and its batch pool %.2f GB of it); page-locked: decode buffers %.2f GB, the reader's ring and tables %.2f GB\n",
                    opt.jobs.size(), (total_b - free_b) / 1e9, total_b / 1e9, rd_dev / 1e9, pinned / 1e9, rd_pinned / 1e9);
    }
    const bool fast_exit = getenv("BQC_FAST_EXIT") && getenv("BQC_FAST_EXIT")[0] == '1';
    const char* done_fd = fast_exit ? getenv("BQC_DONE_FD") : nullptr;
    fflush(stdout); fflush(stderr);
    if (done_fd) { // nothing is printed from here on: the list is reported complete, then this process cleans up on its own
        const int fd = atoi(done_fd);
        const unsigned char st = (unsigned char)status;
        (void)prctl(PR_SET_PDEATHSIG, 0);
        if (write(fd, &st, 1) == 1) {
            close(fd);
            const int nul = open("/dev/null", O_WRONLY);
            if (nul >= 0) { dup2(nul, 1); dup2(nul, 2); }
        }
    }
    bqc_session_close(S);
    if (fast_exit) _exit(status); // (without the static destructors of the HIP runtime, as the single run)
    return status;
}

extern "C" int bqc_main(int argc, const char** argv)
{
    for (int i = 1; i < argc; ++i)
        if (strcmp(argv[i], "--manifest") == 0 || strncmp(argv[i], "--manifest=", 11) == 0) return run_manifest(argc, argv);
    return run_program(argc, argv, nullptr);
}

// The front end of `--gpus N` checks the command line ONCE, before it forks (a usage error is then printed once, and no worker
// starts RCCL for it), and learns the input path the workers will use from the same parser they use.
extern "C" int bqc_program_args(int argc, const char** argv, char* input_path, uint64_t cap)
{
    ProgramOptions opt;
    std::string perr;
    const int pr = parse_args(argc, argv, opt, perr);
    if (pr == 1) fprintf(stderr, "%s\n", perr.c_str());
    if (pr == 0 && input_path && cap) snprintf(input_path, (size_t)cap, "%s", opt.bamFile.c_str());
    return pr;
}

extern "C" int bqc_main_shard(int argc, const char** argv, uint32_t shard_index, uint32_t shard_count, bqc_shard_hook hook, void* user)
{
    if (!hook || shard_count == 0 || shard_index >= shard_count) return 1;
    const ShardArgs sa{shard_index, shard_count, hook, user};
    return run_program(argc, argv, &sa);
}
