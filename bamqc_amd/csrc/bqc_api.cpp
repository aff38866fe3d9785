// bqc_api.cpp — host side of libbamqc_gpu.so: context, host pre-pass, device batches, launches,
// finalisation.  Implements include/bamqc.h.  There is NO CPU fallback in this library: without a
// working HIP device bqc_create fails with BQC_ERR_DEVICE.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdarg>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <chrono>
#include <condition_variable>
#include <mutex>
#include <thread>
#include <vector>

#include "bqc_ctx.h"
#include "adapter_rule.h"
#include "../host/parallel.h"

extern "C" {
void bqc_launch_cov_final(const StateLayout&, uint64_t*, const uint32_t* carry, const uint32_t* parity, const uint8_t* started, const uint8_t* sel, uint32_t count_start, hipStream_t);
void bqc_launch_ref_nibbles(const uint8_t* dna5, uint64_t len, uint32_t* out, uint64_t n_dwords, hipStream_t);
uint32_t bqc_long_slots_cap(uint32_t max_read_len, uint32_t n_cu);
uint64_t bqc_qcyc_words(uint32_t n_lanes, uint32_t N);
uint64_t bqc_mbc_words(uint32_t n_lanes, uint32_t N);
uint64_t bqc_adp_words(uint32_t n_lanes, uint32_t N);
uint64_t bqc_gcb_words(uint32_t n_lanes);
uint64_t bqc_ibc_words(uint32_t n_lanes, uint32_t N);
uint64_t bqc_sbc_words(uint32_t n_lanes, uint32_t N);
uint64_t bqc_sac_words(uint32_t n_lanes, uint32_t S);
uint64_t bqc_rcv_words(uint32_t n_lanes, uint64_t B, uint32_t R);
uint64_t bqc_wdp_words(uint32_t n_lanes, uint64_t NW);
uint32_t bqc_rcv_tiles(uint64_t B, uint32_t R);
uint64_t bqc_rcv_out_words(uint32_t n_lanes, uint32_t R, uint32_t n_thr, uint32_t D);
void bqc_launch_rcv_final(const uint64_t* state, const RcvRegions& rg, const RcvFinal& fp, uint32_t n_lanes, uint64_t* tsum, uint64_t* out, hipStream_t s);
uint64_t bqc_dup_slots(uint64_t capacity);
uint64_t bqc_dup_out_words(void);
void bqc_launch_dup_clear(const DupTable& T, uint64_t* sums, uint32_t n_lanes, uint32_t n_cu, hipStream_t s);
void bqc_launch_dup_final(const DupTable& T, uint64_t* out, uint32_t n_cu, hipStream_t s);
uint64_t bqc_ovr_out_words(uint64_t list_cap);
void bqc_launch_ovr_clear(const DupTable& T, uint64_t* sums, uint32_t n_lanes, uint32_t n_cu, hipStream_t s);
void bqc_launch_ovr_final(const DupTable& T, const uint64_t* thr, uint64_t* out, uint64_t list_cap, uint32_t* err, uint32_t n_cu, hipStream_t s);
uint32_t bqc_gcb_share(void);
void bqc_launch_gcb_genome(const GcbContig* tab, uint32_t n_contigs, uint64_t n_shares, uint32_t W, const GcbDiv& D, uint64_t* G, uint32_t n_cu, hipStream_t s);
hipError_t bqc_long_init();
hipError_t bqc_short_init();
}

static thread_local char g_create_err[512];

int bqc_fail(bqc_ctx* c, int code, const char* fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (c) c->err = buf;
    else snprintf(g_create_err, sizeof g_create_err, "%s", buf);
    return code;
}
#define fail bqc_fail

extern "C" int bqc_abi_version(void) { return BQC_ABI_VERSION; }
extern "C" const char* bqc_last_error(const bqc_ctx* c) { return c ? c->err.c_str() : g_create_err; }

static int upload_ref_tables(bqc_ctx* c)
{
    HIPCHK(c, hipMemcpyAsync(c->d_ref_ptrs, c->d_ref.data(), sizeof(uint8_t*) * c->d_ref.size(), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->d_ref_len, c->ref_len.data(), sizeof(uint64_t) * c->ref_len.size(), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->d_refn_ptrs, c->d_refn.data(), sizeof(uint32_t*) * c->d_refn.size(), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
}

// the records that follow the stream of batches: merged error record (none), FASTA cursor (-1: before the first contig)
static int reset_stream_records(bqc_ctx* c)
{
    ErrRec e{};
    e.first_key = BQC_ERRKEY_NONE;
    const int32_t cur[2] = {-1, -1}; // last / first FASTA position of the stream's triplet-eligible reads
    HIPCHK(c, hipMemcpyAsync(c->d_err0, &e, sizeof e, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->d_cursor, cur, 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream)); // (the sources are on this function's stack)
    return 0;
}

// The adapter set of bqc_modules, checked (include/bamqc.h: bqc_create_ex) and copied: names, sequences and the kernel's patterns.
// n_adapters = 0: the built-in set.  Returns 0, or BQC_ERR_ARG with the message set.
static int adapter_set(const bqc_modules* mod, std::vector<std::string>& names, std::vector<std::string>& seqs, AdpPatterns& P)
{
    uint32_t n_builtin;
    const bqc_adapter* builtin = bqc_builtin_adapters(&n_builtin);
    const bqc_adapter* set = mod->n_adapters ? mod->adapters : builtin;
    const uint32_t n = mod->n_adapters ? mod->n_adapters : n_builtin;
    if (n > BQC_ADP_MAX) return fail(nullptr, BQC_ERR_ARG, "bqc_create_ex: %u adapters given, at most %d are taken", n, BQC_ADP_MAX);
    if (!set) return fail(nullptr, BQC_ERR_ARG, "bqc_create_ex: n_adapters is %u and adapters is null", n);
    memset(&P, 0, sizeof P);
    P.n = n;
    for (uint32_t a = 0; a < n; ++a) {
        const char* nm = set[a].name;
        const char* sq = set[a].seq;
        const std::string fault = bqc_adapter_fault(nm, sq);
        if (!fault.empty()) return fail(nullptr, BQC_ERR_ARG, "bqc_create_ex: adapter %u: %s", a, fault.c_str());
        for (uint32_t b = 0; b < a; ++b)
            if (names[b] == nm) return fail(nullptr, BQC_ERR_ARG, "bqc_create_ex: the adapter name '%s' is given twice", nm);
        const size_t m = strlen(sq);
        uint32_t fwd = 0, rc = 0;
        for (size_t i = 0; i < m; ++i) {
            const uint32_t code = (uint32_t)(strchr("ACGT", sq[i]) - "ACGT");
            fwd |= code << (2 * i);
            rc |= (3u - code) << (2 * (m - 1 - i)); // (the complement of letter i is letter m-1-i of the reverse complement)
        }
        names.push_back(nm);
        seqs.push_back(sq);
        P.len[a] = (uint32_t)m; P.fwd[a] = fwd; P.rc[a] = rc;
        P.cmask[a] = (uint32_t)((1ull << (2 * m)) - 1); // (64-bit: m = 16 would be a 32-bit shift by 32)
        P.vmask[a] = (1u << m) - 1u;
    }
    return 0;
}

// bqc_create_ex's device calls: a failure destroys the half-made context
#define CCHK(call)                                                                                            \
    do {                                                                                                      \
        hipError_t e_ = (call);                                                                               \
        if (e_ != hipSuccess) {                                                                               \
            fail(nullptr, BQC_ERR_DEVICE, "bqc_create: %s failed: %s", #call, hipGetErrorString(e_));         \
            bqc_destroy(c);                                                                                   \
            return BQC_ERR_DEVICE;                                                                            \
        }                                                                                                     \
    } while (0)

// A module's table of the creation (qual_by_cycle, mismatch_by_cycle, adapter_by_cycle; `option`: the call and the option's name, `shape`:
// the table's dimensions) becomes segment `s`: refused before allocating when it does not fit, as the sketch's tables are (1 GiB stays
// for the rest of the context).  A failure destroys the context, as CCHK does.
static int create_segment(bqc_ctx* c, int s, uint64_t words, const char* option, uint32_t n, const char* shape)
{
    size_t free_b = 0, total_b = 0;
    CCHK(hipMemGetInfo(&free_b, &total_b));
    if (words * 8 + (1ull << 30) > free_b) {
        fail(nullptr, BQC_ERR_ARG, "%s %u needs %llu bytes of tables (%s), the device has %zu bytes free (%llu kept for the rest of the context)",
             option, n, (unsigned long long)(words * 8), shape, free_b, 1ull << 30);
        bqc_destroy(c);
        return BQC_ERR_ARG;
    }
    c->seg[s].words = words;
    CCHK(hipMalloc(&c->seg[s].d, words * 8));
    CCHK(hipMemsetAsync(c->seg[s].d, 0, words * 8, c->stream));
    CCHK(hipStreamSynchronize(c->stream));
    return 0;
}

extern "C" int bqc_create(const bqc_options* opt, bqc_ctx** out) { return bqc_create_ex(opt, nullptr, out); }

extern "C" int bqc_create_ex(const bqc_options* opt, const bqc_modules* mod, bqc_ctx** out)
{
    if (!opt || !out) return fail(nullptr, BQC_ERR_ARG, "bqc_create: null argument");
    // (with qual_by_cycle, which lies in the former tail padding, or cut off in front of it: the module is off then)
    // (and with mismatch_by_cycle behind it, or as it was before that field: that module is off then)
    if (opt->struct_size != sizeof(bqc_options) && opt->struct_size != offsetof(bqc_options, mismatch_by_cycle) && opt->struct_size != offsetof(bqc_options, qual_by_cycle))
        return fail(nullptr, BQC_ERR_ARG, "bqc_create: struct_size mismatch");
    const uint32_t qbc_n = opt->struct_size > offsetof(bqc_options, qual_by_cycle) ? opt->qual_by_cycle : 0u;
    const uint32_t mbc_n = opt->struct_size > offsetof(bqc_options, mismatch_by_cycle) ? opt->mismatch_by_cycle : 0u;
    if (opt->n_lanes == 0 || opt->n_lanes > 256) return fail(nullptr, BQC_ERR_ARG, "bqc_create: n_lanes must be 1..256");
    if (opt->isize < 0) return fail(nullptr, BQC_ERR_ARG, "bqc_create: negative insert size");
    if (opt->max_read_len == 0 || opt->hist_cap == 0) return fail(nullptr, BQC_ERR_ARG, "bqc_create: zero capacity");
    if (opt->n_refs && !opt->main_chrom) return fail(nullptr, BQC_ERR_ARG, "bqc_create: main_chrom missing");
    if (qbc_n > opt->max_read_len || qbc_n >= 1u << 30) return fail(nullptr, BQC_ERR_ARG, "bqc_create: qual_by_cycle %u exceeds max_read_len %u", qbc_n, opt->max_read_len);
    if (mbc_n > opt->max_read_len || mbc_n >= 1u << 30) return fail(nullptr, BQC_ERR_ARG, "bqc_create: mismatch_by_cycle %u exceeds max_read_len %u", mbc_n, opt->max_read_len);
    uint32_t adp_n = 0;
    std::vector<std::string> adp_names, adp_seqs;
    AdpPatterns adp_pat{};
    if (mod) {
        if (mod->struct_size != sizeof(bqc_modules)) return fail(nullptr, BQC_ERR_ARG, "bqc_create_ex: bqc_modules.struct_size is %u, not %zu", mod->struct_size, sizeof(bqc_modules));
        adp_n = mod->adapter_by_cycle;
        if (!adp_n && mod->n_adapters) return fail(nullptr, BQC_ERR_ARG, "bqc_create_ex: %u adapters given with adapter_by_cycle 0", mod->n_adapters);
        if (adp_n > opt->max_read_len || adp_n >= 1u << 30) return fail(nullptr, BQC_ERR_ARG, "bqc_create_ex: adapter_by_cycle %u exceeds max_read_len %u", adp_n, opt->max_read_len);
        if (adp_n) {
            const int rc = adapter_set(mod, adp_names, adp_seqs, adp_pat);
            if (rc) return rc;
        }
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(nullptr, BQC_ERR_DEVICE, "bqc_create: no HIP device available (this library has no CPU fallback)");
    if (opt->device < 0 || opt->device >= ndev) return fail(nullptr, BQC_ERR_DEVICE, "bqc_create: device %d out of range", opt->device);
    bqc_ctx* c = new bqc_ctx();
    c->adp_n = adp_n;
    c->adp_names = std::move(adp_names);
    c->adp_seqs = std::move(adp_seqs);
    c->adp_pat = adp_pat;
    for (size_t a = 0; a < c->adp_names.size(); ++a) c->adp_set.push_back(bqc_adapter{c->adp_names[a].c_str(), c->adp_seqs[a].c_str()});
    memset(&c->opt, 0, sizeof(bqc_options));
    memcpy(&c->opt, opt, std::min<size_t>(opt->struct_size, sizeof(bqc_options)));
    c->opt.qual_by_cycle = qbc_n;
    c->opt.mismatch_by_cycle = mbc_n;
    c->opt.pad_tail = 0;
    c->device = opt->device;
    uint32_t nr = opt->n_refs ? opt->n_refs : 1;
    c->main_chrom.assign(nr, 0);
    if (opt->n_refs) memcpy(c->main_chrom.data(), opt->main_chrom, opt->n_refs);
    if (opt->fasta_index) c->fasta_index.assign(opt->fasta_index, opt->fasta_index + opt->n_refs);
    c->opt.main_chrom = c->main_chrom.data();
    c->opt.fasta_index = c->fasta_index.empty() ? nullptr : c->fasta_index.data();
    c->sl = make_state_layout(opt->n_lanes, opt->max_read_len, opt->hist_cap, (uint32_t)opt->isize + 1);
    c->cov.assign(opt->n_lanes, LaneCov());
    c->shard.tail = opt->shard_tail != 0;
    c->shard.pending.assign(opt->n_lanes, c->shard.tail ? 1 : 0);
    c->shard.has_prev.assign(opt->n_lanes, 0);
    c->shard.prev_rid.assign(opt->n_lanes, 0);
    c->shard.prev_bp.assign(opt->n_lanes, 0);
    c->d_ref.assign(nr, nullptr);
    c->d_refn.assign(nr, nullptr);
    c->ref_len.assign(nr, 0);
    const char* v = getenv("BQC_NO_FAST");
    c->no_fast = v && v[0] == '1';
    const char* cs = getenv("BQC_COV_STREAM");
    c->cov_side = !(cs && cs[0] == '0');
    const bool ctiming = getenv("BQC_TIMING") && getenv("BQC_TIMING")[0] == '1';
    const auto ct0 = std::chrono::steady_clock::now();
    double cts[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    auto cstamp = [&](int k) { cts[k] = std::chrono::duration<double>(std::chrono::steady_clock::now() - ct0).count() * 1e3; };
    CCHK(hipSetDevice(c->device));
    hipDeviceProp_t prop;
    CCHK(hipGetDeviceProperties(&prop, c->device));
    c->n_cu = prop.multiProcessorCount > 0 ? (uint32_t)prop.multiProcessorCount : 256;
    // (the kernels' attributes — hipFuncSetAttribute for k_short's and k_long's LDS — are set at their first launch: the first such call
    // loads the code object, 40-60 ms that sat between the runtime's start and the first copy of a run here)
    cstamp(0);
    c->stream = bqc_pool_stream(c->device, 0); // (made ahead by bqc_warmup, or now; the copy stream: at the first submit, bqc_copy_stream)
    if (!c->stream) { fail(nullptr, BQC_ERR_DEVICE, "bqc_create: hipStreamCreate failed"); bqc_destroy(c); return BQC_ERR_DEVICE; }
    cstamp(1);
    CCHK(hipMalloc(&c->d_state, c->sl.words * 8));
    CCHK(hipMalloc(&c->d_err0, sizeof(ErrRec)));
    CCHK(hipMalloc(&c->d_cursor, 8));
    cstamp(6);
    if (!c->fasta_index.empty()) {
        CCHK(hipMalloc(&c->d_fasta_index, 4 * c->fasta_index.size()));
        CCHK(hipMemcpy(c->d_fasta_index, c->fasta_index.data(), 4 * c->fasta_index.size(), hipMemcpyHostToDevice));
    }
    cstamp(7);
    // k_long's scratch: a slot per workgroup it can launch — n_cu, or one per KL_ROW cycles of the longest read accepted
    c->kl_slots_cap = bqc_long_slots_cap(opt->max_read_len, c->n_cu);
    c->t8_slots_cap = std::max(std::max(1024u, 4u * c->n_cu), c->kl_slots_cap);
    CCHK(hipMalloc(&c->d_t8rows, (size_t)c->t8_slots_cap * BQC_T8_SPW * 65536));
    CCHK(hipMalloc(&c->d_t8used, (size_t)c->t8_slots_cap * BQC_T8_USED * 4));
    cstamp(8);
    CCHK(hipMalloc(&c->d_kl_cyc, (size_t)c->kl_slots_cap * 2 * 6 * 1024 * 4));
    CCHK(hipMalloc(&c->d_kl_cyc_used, (size_t)c->kl_slots_cap * 4));
    CCHK(hipMalloc(&c->d_carry, (size_t)opt->n_lanes * 2 * 2000 * 4));
    CCHK(hipMalloc(&c->d_parity, ((size_t)opt->n_lanes + 1) * 4));
    CCHK(hipMalloc(&c->d_started, opt->n_lanes));
    CCHK(hipMalloc(&c->d_ref_ptrs, sizeof(uint8_t*) * nr));
    CCHK(hipMalloc(&c->d_ref_len, sizeof(uint64_t) * nr));
    CCHK(hipMalloc(&c->d_refn_ptrs, sizeof(uint32_t*) * nr));
    CCHK(hipMalloc(&c->d_main, nr));
    cstamp(9);
    CCHK(hipMemcpy(c->d_main, c->main_chrom.data(), nr, hipMemcpyHostToDevice));
    cstamp(2);
    CCHK(hipMemsetAsync(c->d_state, 0, c->sl.words * 8, c->stream));
    if (reset_stream_records(c)) { snprintf(g_create_err, sizeof g_create_err, "%s", c->err.c_str()); bqc_destroy(c); return BQC_ERR_DEVICE; }
    CCHK(hipMemsetAsync(c->d_carry, 0, (size_t)opt->n_lanes * 2 * 2000 * 4, c->stream));
    CCHK(hipMemsetAsync(c->d_parity, 0, ((size_t)opt->n_lanes + 1) * 4, c->stream));
    CCHK(hipMemsetAsync(c->d_started, 0, opt->n_lanes, c->stream));
    CCHK(hipStreamSynchronize(c->stream));
    if (upload_ref_tables(c)) { snprintf(g_create_err, sizeof g_create_err, "%s", c->err.c_str()); bqc_destroy(c); return BQC_ERR_DEVICE; }
    cstamp(3);
    if (opt->sketch.n_k && opt->sketch.n_q) {
        std::string e;
        c->sketch = sketch_create(opt->sketch, opt->n_lanes, c->stream, e);
        if (!c->sketch) { fail(nullptr, BQC_ERR_ARG, "bqc_create: sketch: %s", e.c_str()); bqc_destroy(c); return BQC_ERR_ARG; }
    }
    char shape[128];
    if (qbc_n) {
        snprintf(shape, sizeof shape, "%u read groups x 2 x %u cycles x 224 qualities x 8 bytes", opt->n_lanes, qbc_n);
        if (int rc = create_segment(c, SEG_QCYC, bqc_qcyc_words(opt->n_lanes, qbc_n), "bqc_create: qual_by_cycle", qbc_n, shape)) return rc;
    }
    if (mbc_n) {
        snprintf(shape, sizeof shape, "%u read groups x 2 x 2 x %u cycles x 224 qualities x 8 bytes", opt->n_lanes, mbc_n);
        if (int rc = create_segment(c, SEG_MBC, bqc_mbc_words(opt->n_lanes, mbc_n), "bqc_create: mismatch_by_cycle", mbc_n, shape)) return rc;
    }
    if (adp_n) {
        snprintf(shape, sizeof shape, "%u read groups x 2 x 9 x %u cycles x 8 bytes", opt->n_lanes, adp_n);
        if (int rc = create_segment(c, SEG_ADP, bqc_adp_words(opt->n_lanes, adp_n), "bqc_create_ex: adapter_by_cycle", adp_n, shape)) return rc;
    }
    cstamp(4);
    for (int i = 0; i < 16; ++i) {
        hipEvent_t e;
        CCHK(hipEventCreate(&e));
        c->ev.push_back(e);
    }
    cstamp(5);
    if (ctiming) fprintf(stderr, "[timing] bqc_create: kernel attributes (code object load) at %.1f ms, compute stream %.1f, allocations %.1f (first three %.1f, FASTA index copied %.1f, 8-mer rows %.1f, the rest %.1f, then a copy), memsets + tables %.1f, sketch %.1f, events %.1f\n", cts[0], cts[1], cts[2], cts[6], cts[7], cts[8], cts[9], cts[3], cts[4], cts[5]);
    *out = c;
    return 0;
}

// Streams made ahead.  On this card a process's first stream costs 20-25 ms and each of the next three 8-10 (a hardware queue each:
// tools/micro/startup_probe.cpp, profiles/r4_startup_probe.txt), one after the other whichever threads ask — 45-50 ms that the program's
// reader (two streams) and the context (two) used to pay in turn, between the runtime's start and the first kernel.  bqc_warmup makes
// them in ITS thread right behind the runtime's start, while the caller's other threads allocate, page-lock and parse; whoever needs
// a stream takes one from here (waiting for the warm-up if it is still at it), or creates it when there is none.
namespace {
struct StreamPool {
    std::mutex m;
    std::condition_variable cv;
    static const int kAhead = 4;
    hipStream_t made[kAhead] = {nullptr, nullptr, nullptr, nullptr};
    bool taken[kAhead] = {false, false, false, false};
    int device = -1;
    int n_made = 0;
    bool making = false; // the warm-up thread is still at it
};
StreamPool g_streams;
}
// `rank`: the order in which the program needs its streams — 0 the context's compute stream (its creation, the references), 1 the
// reader's producer (first copy, first inflate), 2 the reader's consumer (first walk), 3 the context's copy stream (first submit):
// a caller waits for the stream of ITS rank, not for whichever comes next.
hipStream_t bqc_pool_stream(int device, int rank)
{
    {
        std::unique_lock<std::mutex> lk(g_streams.m);
        if (g_streams.device == device && rank >= 0 && rank < StreamPool::kAhead) {
            g_streams.cv.wait(lk, [&] { return g_streams.n_made > rank || !g_streams.making; });
            if (g_streams.n_made > rank && !g_streams.taken[rank]) { g_streams.taken[rank] = true; return g_streams.made[rank]; }
        }
    }
    hipStream_t s = nullptr;
    if (rank == BQC_STREAM_RANK_COV) { // the context's coverage stream: it must not take the card from the compute stream's next kernel
        int least = 0, greatest = 0;
        if (hipDeviceGetStreamPriorityRange(&least, &greatest) != hipSuccess) { (void)hipGetLastError(); least = 0; }
        if (hipStreamCreateWithPriority(&s, hipStreamNonBlocking, least) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
        return s;
    }
    if (hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    return s;
}

extern "C" int bqc_warmup(int32_t device)
{
    {
        std::lock_guard<std::mutex> lk(g_streams.m);
        if (g_streams.device != -1) return g_streams.device == device ? 0 : BQC_ERR_ARG; // (once per process)
        g_streams.device = device;
        g_streams.making = true;
    }
    auto done = [](int rc) { { std::lock_guard<std::mutex> lk(g_streams.m); g_streams.making = false; } g_streams.cv.notify_all(); return rc; };
    if (hipSetDevice(device) != hipSuccess || hipFree(nullptr) != hipSuccess) return done(BQC_ERR_DEVICE);
    // (Tried in round 4: the first copy from pageable memory — ~50 ms of runtime set-up that bqc_create pays behind its compute stream,
    // `[timing] bqc_create` — made here by a thread of its own beside the streams: the record loop starts at 0.19 s either way,
    // gpurun_out/r9d; the runtime serialises the two.)
    for (int k = 0; k < StreamPool::kAhead; ++k) {
        hipStream_t s = nullptr;
        if (hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess) { (void)hipGetLastError(); return done(BQC_ERR_DEVICE); }
        { std::lock_guard<std::mutex> lk(g_streams.m); g_streams.made[k] = s; g_streams.n_made = k + 1; }
        g_streams.cv.notify_all();
    }
    return done(0);
}

extern "C" int bqc_set_fasta_index(bqc_ctx* c, const int32_t* idx)
{
    if (!c || !idx) return BQC_ERR_ARG;
    if (c->upload_counter) return bqc_fail(c, BQC_ERR_STATE, "bqc_set_fasta_index after the first batch");
    HIPCHK(c, hipSetDevice(c->device));
    const size_t n = c->opt.n_refs ? c->opt.n_refs : 1;
    c->fasta_index.assign(n, -1);
    for (uint32_t r = 0; r < c->opt.n_refs; ++r) c->fasta_index[r] = idx[r];
    c->opt.fasta_index = c->fasta_index.data();
    if (!c->d_fasta_index) HIPCHK(c, hipMalloc(&c->d_fasta_index, 4 * n));
    HIPCHK(c, hipMemcpy(c->d_fasta_index, c->fasta_index.data(), 4 * n, hipMemcpyHostToDevice));
    return 0;
}

extern "C" void bqc_destroy(bqc_ctx* c)
{
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->copy_stream) (void)hipStreamSynchronize(c->copy_stream);
    if (c->cov_stream) (void)hipStreamSynchronize(c->cov_stream);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    bqc_pipeline_destroy(c);
    bqc_anchor_destroy(c);
    auto in_arena = [&](const void* p) { return c->ref_arena && (const uint8_t*)p >= c->ref_arena && (const uint8_t*)p < c->ref_arena + c->ref_arena_cap; };
    for (auto p : c->d_ref) if (p && !in_arena(p)) (void)hipFree(p);
    for (auto p : c->d_refn) if (p && !in_arena(p)) (void)hipFree(p);
    if (c->ref_arena) (void)hipFree(c->ref_arena);

    (void)hipFree(c->d_refn_ptrs);
    if (c->sketch) sketch_destroy(c->sketch);
    for (const StateSeg& s : c->seg) if (s.d) (void)hipFree(s.d);
    if (c->d_sac_tab) (void)hipFree(c->d_sac_tab);
    if (c->d_wdp_tab) (void)hipFree(c->d_wdp_tab);
    if (c->d_rcv_tab) (void)hipFree(c->d_rcv_tab);
    if (c->d_rcv_out) (void)hipFree(c->d_rcv_out);
    if (c->d_dup) (void)hipFree(c->d_dup);
    if (c->d_ovr) (void)hipFree(c->d_ovr);
    if (c->d_gcb_g) (void)hipFree(c->d_gcb_g);
    if (c->d_gcb_tab) (void)hipFree(c->d_gcb_tab);
    (void)hipFree(c->d_state); (void)hipFree(c->d_err0); (void)hipFree(c->d_cursor); (void)hipFree(c->d_fasta_index); (void)hipFree(c->d_t8rows); (void)hipFree(c->d_t8used); (void)hipFree(c->d_kl_cyc); (void)hipFree(c->d_kl_cyc_used); (void)hipFree(c->d_carry); (void)hipFree(c->d_parity);
    (void)hipFree(c->d_started); (void)hipFree(c->d_ref_ptrs); (void)hipFree(c->d_ref_len); (void)hipFree(c->d_main);
    for (auto e : c->ev) (void)hipEventDestroy(e);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    if (c->copy_stream) (void)hipStreamDestroy(c->copy_stream);
    if (c->cov_stream) (void)hipStreamDestroy(c->cov_stream);
    if (c->ev_cov_fork) (void)hipEventDestroy(c->ev_cov_fork);
    if (c->ev_cov_join) (void)hipEventDestroy(c->ev_cov_join);
    delete c;
}

extern "C" int bqc_reserve_references(bqc_ctx* c, uint64_t total_bases, uint32_t n_contigs)
{
    if (!c) return BQC_ERR_ARG;
    if (c->ref_arena) return 0;
    HIPCHK(c, hipSetDevice(c->device));
    // per contig: len bytes of codes + (len / 8 + pads) dwords of nibbles, each rounded up to 256 bytes
    const size_t cap = (size_t)total_bases + (size_t)total_bases / 2 + (size_t)n_contigs * (8 * BQC_FAST_NH + 1024) + 4096;
    if (hipMalloc((void**)&c->ref_arena, cap) != hipSuccess) { (void)hipGetLastError(); c->ref_arena = nullptr; return 0; } // (not fatal: the contigs are then allocated one by one)
    c->ref_arena_cap = cap;
    c->ref_arena_used = 0;
    return 0;
}

extern "C" int bqc_set_reference(bqc_ctx* c, int32_t rid, const uint8_t* dna5, uint64_t len)
{
    if (!c || rid < 0 || (uint32_t)rid >= c->opt.n_refs || (!dna5 && len)) return fail(c, BQC_ERR_ARG, "bqc_set_reference: bad argument");
    HIPCHK(c, hipSetDevice(c->device));
    auto in_arena = [&](const void* p) { return c->ref_arena && (const uint8_t*)p >= c->ref_arena && (const uint8_t*)p < c->ref_arena + c->ref_arena_cap; };
    if (c->d_ref[rid]) { if (!in_arena(c->d_ref[rid])) HIPCHK(c, hipFree(c->d_ref[rid])); c->d_ref[rid] = nullptr; }
    if (c->d_refn[rid]) { if (!in_arena(c->d_refn[rid])) HIPCHK(c, hipFree(c->d_refn[rid])); c->d_refn[rid] = nullptr; }
    const uint64_t nd8 = (len + 7) / 8; // nibble table of the fast path: BQC_FAST_NH pad dwords + nd8 + BQC_FAST_NH pad dwords
    const size_t b1 = ((len ? len : 1) + 255) & ~(size_t)255, b2 = ((nd8 + 2 * BQC_FAST_NH) * 4 + 255) & ~(size_t)255;
    uint8_t* p = nullptr;
    uint32_t* pn = nullptr;
    if (c->ref_arena && c->ref_arena_used + b1 + b2 <= c->ref_arena_cap) {
        p = c->ref_arena + c->ref_arena_used;
        pn = (uint32_t*)(p + b1);
        c->ref_arena_used += b1 + b2;
    } else {
        HIPCHK(c, hipMalloc(&p, len ? len : 1));
        HIPCHK(c, hipMalloc(&pn, (nd8 + 2 * BQC_FAST_NH) * 4));
    }
    // (a plain synchronous copy from the caller's pageable memory: 8.9 GB/s for a human genome's 3.1 GB — measured in round 3 against
    // hipMemcpyAsync on a stream of its own, 4.8 GB/s, and against page-locking the contigs first, 4-5 GB/s all told)
    HIPCHK(c, hipMemcpy(p, dna5, len, hipMemcpyHostToDevice));
    bqc_launch_ref_nibbles(p, len, pn, nd8, c->stream);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->d_ref[rid] = p;
    c->d_refn[rid] = pn;
    c->ref_len[rid] = len;
    return upload_ref_tables(c);
}

// The contigs of `from` become those of `to` without another upload: the device allocations (and the bqc_reserve_references block they
// may lie in) change owner.  Same device, same n_refs, `to` has none yet; `from` is only good for bqc_destroy afterwards.
extern "C" int bqc_move_references(bqc_ctx* from, bqc_ctx* to)
{
    if (!from || !to || from == to) return BQC_ERR_ARG;
    if (from->device != to->device || from->opt.n_refs != to->opt.n_refs) return fail(to, BQC_ERR_ARG, "bqc_move_references: another device or another number of contigs");
    if (to->ref_arena) return fail(to, BQC_ERR_STATE, "bqc_move_references: the receiving context has references of its own");
    for (size_t r = 0; r < to->d_ref.size(); ++r) if (to->d_ref[r] || to->d_refn[r]) return fail(to, BQC_ERR_STATE, "bqc_move_references: the receiving context has references of its own");
    HIPCHK(to, hipSetDevice(to->device));
    (void)bqc_drain(from); // (nothing of the giving context may still be reading them)
    HIPCHK(to, hipStreamSynchronize(from->stream));
    to->d_ref = from->d_ref; to->d_refn = from->d_refn; to->ref_len = from->ref_len;
    to->ref_arena = from->ref_arena; to->ref_arena_cap = from->ref_arena_cap; to->ref_arena_used = from->ref_arena_used;
    from->d_ref.assign(from->d_ref.size(), nullptr); from->d_refn.assign(from->d_refn.size(), nullptr); from->ref_len.assign(from->ref_len.size(), 0);
    from->ref_arena = nullptr; from->ref_arena_cap = from->ref_arena_used = 0;
    from->poisoned = true; from->poison_code = BQC_ERR_STATE; from->err = "its references were moved to another context";
    const int rc = upload_ref_tables(to);
    if (rc) return rc;
    HIPCHK(to, hipStreamSynchronize(to->stream));
    return 0;
}

// Wait for everything submitted and report the first error of the stream (as the reference would have met it): batches of the
// submit pipeline through their own records, resident batches (bqc_process) through the context's merged record.
static int sync_and_check(bqc_ctx* c)
{
    HIPCHK(c, hipSetDevice(c->device));
    if (c->poisoned) return bqc_fail(c, BQC_ERR_STATE, "context is in an error state: %s", c->err.c_str());
    int rc = bqc_drain(c);
    if (rc) return rc;
    ErrRec e;
    HIPCHK(c, hipMemcpyAsync(&e, c->d_err0, sizeof e, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    rc = bqc_report_errors(c, e);
    if (rc) { c->poisoned = true; c->poison_code = rc; }
    return rc;
}

extern "C" int bqc_sync(bqc_ctx* c)
{
    if (!c) return BQC_ERR_ARG;
    return sync_and_check(c);
}

extern "C" int bqc_reset(bqc_ctx* c)
{
    if (!c) return BQC_ERR_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    (void)bqc_drain(c); // (whatever the batches in flight found is forgotten with the counters)
    bqc_state_ready(c);
    HIPCHK(c, hipMemsetAsync(c->d_state, 0, c->sl.words * 8, c->stream));
    if (reset_stream_records(c)) return BQC_ERR_DEVICE;
    HIPCHK(c, hipMemsetAsync(c->d_carry, 0, (size_t)c->opt.n_lanes * 2 * 2000 * 4, c->stream));
    HIPCHK(c, hipMemsetAsync(c->d_parity, 0, ((size_t)c->opt.n_lanes + 1) * 4, c->stream));
    HIPCHK(c, hipMemsetAsync(c->d_started, 0, c->opt.n_lanes, c->stream));
    if (c->sketch) sketch_reset(c->sketch, c->stream);
    for (const StateSeg& s : c->seg) // (the modules' words; their side tables — sites, regions, contigs — stay, the genome table is bqc_finalize's)
        if (s.d) HIPCHK(c, hipMemsetAsync(s.d, 0, s.words * 8, c->stream));
    if (c->d_dup) { // (the table and the sums go back to empty; the allocation stays)
        bqc_launch_dup_clear(c->dup_tab, c->d_dup_sums, c->opt.n_lanes, c->n_cu, c->stream);
        HIPCHK(c, hipGetLastError());
    }
    if (c->d_ovr) { // (the same for the table of the overrepresented sequences)
        bqc_launch_ovr_clear(c->ovr_tab, c->d_ovr_sums, c->opt.n_lanes, c->n_cu, c->stream);
        HIPCHK(c, hipGetLastError());
    }
    for (bool& f : c->finalised) f = false;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->cov.assign(c->opt.n_lanes, LaneCov());
    if (c->anchor.d_state) HIPCHK(c, bqc_anchor_fresh_state(c)); // (anchors made on the card: every read group's state starts over as well)
    c->anchor.mode = 0;
    c->state_seq = 0;
    c->flushed = false;
    c->poisoned = false;
    c->poison_code = 0;
    return 0;
}

extern "C" int bqc_set_timing(bqc_ctx* c, int enable)
{
    if (!c) return BQC_ERR_ARG;
    c->timing = enable != 0;
    return 0;
}

extern "C" int bqc_last_timing(bqc_ctx* c, uint32_t* n, const char* const** names, const float** ms)
{
    if (!c || !n || !names || !ms) return BQC_ERR_ARG;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->tms.assign(c->n_timed, 0.f);
    for (int i = 0; i < c->n_timed; ++i) (void)hipEventElapsedTime(&c->tms[i], c->ev[i], c->ev[i + 1]);
    *n = (uint32_t)c->n_timed;
    *names = c->tnames.data();
    *ms = c->tms.data();
    return 0;
}

extern "C" int bqc_flush(bqc_ctx* c)
{
    if (!c) return BQC_ERR_ARG;
    if (c->poisoned) return fail(c, BQC_ERR_STATE, "context is in an error state: %s", c->err.c_str());
    if (c->flushed) return 0;
    HIPCHK(c, hipSetDevice(c->device));
    int rc = sync_and_check(c);
    if (rc) return rc;
    bqc_state_ready(c);
    bqc_launch_cov_final(c->sl, c->d_state, c->d_carry, c->d_parity, c->d_started, nullptr, 1, c->stream);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->flushed = true;
    return 0;
}

// where segment `s` begins in the flat vector (s = N_SEG: the vector's length): behind sl.words, the sketch's words and the segments in front of it
static uint64_t seg_start(const bqc_ctx* c, int s)
{
    uint64_t off = c->sl.words + (c->sketch ? sketch_state_words(c->sketch) : 0);
    for (int k = 0; k < s; ++k) off += c->seg[k].words;
    return off;
}
extern "C" uint64_t bqc_state_words(const bqc_ctx* c) { return c ? seg_start(c, N_SEG) : 0; }

// The four exchange calls: the whole vector between the context and `buf` (only read when `incoming`), which lies in device memory — copies
// on the compute stream — or, `host`, in host memory: blocking copies, the sketch's words through a staging buffer on the card.
static int state_transfer(bqc_ctx* c, uint64_t* buf, bool incoming, bool host)
{
    c->modules_closed = true;
    if (incoming) {
        HIPCHK(c, hipSetDevice(c->device));
        (void)bqc_drain(c);
    } else {
        const int rc = bqc_flush(c);
        if (rc) return rc;
    }
    bqc_state_ready(c);
    if (host) HIPCHK(c, hipStreamSynchronize(c->stream));
    const hipMemcpyKind kind = !host ? hipMemcpyDeviceToDevice : incoming ? hipMemcpyHostToDevice : hipMemcpyDeviceToHost;
    auto copy_words = [&](uint64_t* dev, uint64_t off, uint64_t words) {
        void* dst = incoming ? dev : buf + off;
        const void* src = incoming ? buf + off : dev;
        return host ? hipMemcpy(dst, src, words * 8, kind) : hipMemcpyAsync(dst, src, words * 8, kind, c->stream);
    };
    HIPCHK(c, copy_words(c->d_state, 0, c->sl.words));
    if (c->sketch) {
        uint64_t *sk = buf + c->sl.words, *tmp = nullptr;
        const uint64_t w = sketch_state_words(c->sketch);
        if (host) {
            HIPCHK(c, hipMalloc(&tmp, w * 8));
            if (incoming) HIPCHK(c, hipMemcpy(tmp, sk, w * 8, hipMemcpyHostToDevice));
        }
        if (incoming) sketch_state_import(c->sketch, host ? tmp : sk, c->stream);
        else sketch_state_export(c->sketch, host ? tmp : sk, c->stream);
        if (host) {
            HIPCHK(c, hipStreamSynchronize(c->stream));
            if (!incoming) HIPCHK(c, hipMemcpy(sk, tmp, w * 8, hipMemcpyDeviceToHost));
            HIPCHK(c, hipFree(tmp));
        }
    }
    for (int s = 0; s < N_SEG; ++s)
        if (c->seg[s].d) HIPCHK(c, copy_words(c->seg[s].d, seg_start(c, s), c->seg[s].words));
    if (!host) HIPCHK(c, hipStreamSynchronize(c->stream));
    if (incoming) c->flushed = true; // an imported vector is already flushed
    return 0;
}
extern "C" int bqc_state_export(bqc_ctx* c, void* dst) { return c && dst ? state_transfer(c, (uint64_t*)dst, false, false) : BQC_ERR_ARG; }
extern "C" int bqc_state_import(bqc_ctx* c, const void* src) { return c && src ? state_transfer(c, (uint64_t*)src, true, false) : BQC_ERR_ARG; }
extern "C" int bqc_state_export_host(bqc_ctx* c, uint64_t* dst) { return c && dst ? state_transfer(c, dst, false, true) : BQC_ERR_ARG; }
extern "C" int bqc_state_import_host(bqc_ctx* c, const uint64_t* src) { return c && src ? state_transfer(c, (uint64_t*)src, true, true) : BQC_ERR_ARG; }

// ---------------------------------------------------------------------------------------------------
// finalize
// ---------------------------------------------------------------------------------------------------
static uint32_t last_nonzero_len(const uint64_t* p, uint32_t n)
{
    while (n > 0 && p[n - 1] == 0) --n;
    return n;
}

// A kernel of bqc_finalize (k_gcb_genome, k_rcv_final, k_dup_final, k_ovr_final).  With timing on, bqc_last_timing shows it afterwards, as it shows a
// batch's kernels, which are over; `shown`: of several in one bqc_finalize the GC bias's comes first, then the regions', then the sets', then the sequences'.
template <class Launch> static void timed_launch(bqc_ctx* c, bool shown, const char* name, Launch&& launch)
{
    const bool timed = shown && c->timing && c->ev.size() >= 2;
    if (timed) { c->n_timed = 0; c->tnames.clear(); (void)hipEventRecord(c->ev[0], c->stream); }
    launch();
    if (timed) { (void)hipEventRecord(c->ev[1], c->stream); c->tnames.push_back(name); c->n_timed = 1; }
}

// bqc_finalize's copy of a module's words
static int fetch_segment(bqc_ctx* c, int s, std::vector<uint64_t>& h)
{
    h.resize(c->seg[s].words);
    HIPCHK(c, hipMemcpy(h.data(), c->seg[s].d, h.size() * 8, hipMemcpyDeviceToHost));
    return 0;
}

// The genome table G of the GC bias (include/bamqc.h) from the contigs the context holds now: k_gcb_genome on the compute stream, into
// d_gcb_g, and from there into h_gcb_g.
static int gcb_genome_table(bqc_ctx* c)
{
    std::vector<GcbContig> tab;
    uint64_t n_shares = 0;
    const uint64_t share = bqc_gcb_share();
    for (size_t r = 0; r < c->d_ref.size(); ++r) {
        if (!c->d_ref[r] || c->ref_len[r] < c->gcb_w) continue; // (not given, or shorter than a window)
        const uint64_t nstarts = c->ref_len[r] - c->gcb_w + 1;
        tab.push_back(GcbContig{c->d_ref[r], nstarts, n_shares});
        n_shares += (nstarts + share - 1) / share;
    }
    HIPCHK(c, hipMemsetAsync(c->d_gcb_g, 0, BQC_GCB_BINS * 8, c->stream));
    if (!tab.empty()) {
        HIPCHK(c, hipMemcpyAsync(c->d_gcb_tab, tab.data(), tab.size() * sizeof(GcbContig), hipMemcpyHostToDevice, c->stream));
        timed_launch(c, true, "k_gcb_genome", [&] { bqc_launch_gcb_genome(c->d_gcb_tab, (uint32_t)tab.size(), n_shares, c->gcb_w, c->gcb_div, c->d_gcb_g, c->n_cu, c->stream); });
        HIPCHK(c, hipGetLastError());
    }
    c->h_gcb_g.resize(BQC_GCB_BINS);
    HIPCHK(c, hipMemcpyAsync(c->h_gcb_g.data(), c->d_gcb_g, BQC_GCB_BINS * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream)); // (also: `tab` is read to here)
    return 0;
}

// The bqc_enable_* calls belong right behind bqc_create: `fn` comes too late (BQC_ERR_STATE) once the context has done anything else.
static int too_late(bqc_ctx* c, const char* fn)
{
    if (c->upload_counter || c->next_ticket > 1 || c->anchor.mode.load() == 1 || c->modules_closed)
        return fail(c, BQC_ERR_STATE, "%s: the context has taken a batch, exchanged state or been finalised (the call belongs right behind bqc_create)", fn);
    return 0;
}

// `words` words of device memory, cleared on the compute stream and waited for: a module's segment in the making (nullptr: not to be
// had, and nothing stays allocated).  The caller registers it in bqc_ctx::seg once its side tables exist as well.
static uint64_t* zeroed_words(bqc_ctx* c, uint64_t words)
{
    uint64_t* d = nullptr;
    if (hipMalloc(&d, words * 8) == hipSuccess && hipMemsetAsync(d, 0, words * 8, c->stream) == hipSuccess && hipStreamSynchronize(c->stream) == hipSuccess) return d;
    (void)hipGetLastError();
    (void)hipFree(d);
    return nullptr;
}

extern "C" int bqc_enable_gc_bias(bqc_ctx* c, uint32_t window)
{
    if (!c) return BQC_ERR_ARG;
    if (window < BQC_GCB_WMIN || window > BQC_GCB_WMAX) return fail(c, BQC_ERR_ARG, "bqc_enable_gc_bias: window %u is outside %d ... %d", window, BQC_GCB_WMIN, BQC_GCB_WMAX);
    if (c->seg[SEG_GCB].d) return fail(c, BQC_ERR_STATE, "bqc_enable_gc_bias: the module is on already (window %u)", c->gcb_w);
    if (int rc = too_late(c, __func__)) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    const uint64_t words = bqc_gcb_words(c->opt.n_lanes);
    uint64_t *d = zeroed_words(c, words), *g = zeroed_words(c, BQC_GCB_BINS);
    GcbContig* tab = nullptr;
    if (!d || !g || hipMalloc(&tab, std::max<size_t>(1, c->opt.n_refs) * sizeof(GcbContig)) != hipSuccess) {
        (void)hipGetLastError();
        (void)hipFree(d); (void)hipFree(g); (void)hipFree(tab);
        return fail(c, BQC_ERR_DEVICE, "bqc_enable_gc_bias: the tables could not be allocated");
    }
    for (uint32_t n = 0; n < 5; ++n) c->gcb_div.m[n] = (uint32_t)(((1ull << 32) + (window - n) - 1) / (window - n)); // ceil(2^32 / (W - n))
    c->gcb_w = window;
    c->seg[SEG_GCB] = {d, words};
    c->d_gcb_g = g; c->d_gcb_tab = tab;
    return 0;
}

extern "C" int bqc_enable_indel_by_cycle(bqc_ctx* c, uint32_t n_cycles)
{
    if (!c) return BQC_ERR_ARG;
    if (!n_cycles || n_cycles > c->opt.max_read_len || n_cycles >= 1u << 30)
        return fail(c, BQC_ERR_ARG, "bqc_enable_indel_by_cycle: capacity %u is outside 1 ... max_read_len %u", n_cycles, c->opt.max_read_len);
    if (c->seg[SEG_IBC].d) return fail(c, BQC_ERR_STATE, "bqc_enable_indel_by_cycle: the module is on already (capacity %u)", c->ibc_n);
    if (int rc = too_late(c, __func__)) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    const uint64_t words = bqc_ibc_words(c->opt.n_lanes, n_cycles);
    uint64_t* d = zeroed_words(c, words);
    if (!d) return fail(c, BQC_ERR_DEVICE, "bqc_enable_indel_by_cycle: the tables (%llu bytes) could not be allocated", (unsigned long long)(words * 8));
    c->ibc_n = n_cycles;
    c->seg[SEG_IBC] = {d, words};
    return 0;
}

extern "C" int bqc_enable_substitutions(bqc_ctx* c, uint32_t n_cycles, uint32_t min_base_qual, uint32_t min_mapq)
{
    if (!c) return BQC_ERR_ARG;
    if (!n_cycles || n_cycles > c->opt.max_read_len || n_cycles >= 1u << 27)
        return fail(c, BQC_ERR_ARG, "bqc_enable_substitutions: capacity %u is outside 1 ... max_read_len %u", n_cycles, c->opt.max_read_len);
    if (min_base_qual > 222) return fail(c, BQC_ERR_ARG, "bqc_enable_substitutions: minimum base quality %u is outside 0 ... 222", min_base_qual);
    if (min_mapq > 255) return fail(c, BQC_ERR_ARG, "bqc_enable_substitutions: minimum mapping quality %u is outside 0 ... 255", min_mapq);
    if (c->seg[SEG_SBC].d) return fail(c, BQC_ERR_STATE, "bqc_enable_substitutions: the module is on already (capacity %u)", c->sbc_n);
    if (int rc = too_late(c, __func__)) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    const uint64_t words = bqc_sbc_words(c->opt.n_lanes, n_cycles);
    uint64_t* d = zeroed_words(c, words);
    if (!d) return fail(c, BQC_ERR_DEVICE, "bqc_enable_substitutions: the tables (%llu bytes) could not be allocated", (unsigned long long)(words * 8));
    c->sbc_n = n_cycles; c->sbc_q = min_base_qual; c->sbc_mq = min_mapq;
    c->seg[SEG_SBC] = {d, words};
    return 0;
}

// The site tables of k_sac.hip (device_types.h: SacSites) from the checked list: one allocation, [pos S][first n_refs + 1][bkt_off
// n_refs + 1][bkt].  The index comes from the sites alone: the library does not know contig lengths.
extern "C" int bqc_enable_site_alleles(bqc_ctx* c, uint32_t n_sites, const int32_t* rid, const int32_t* pos, uint32_t min_base_qual, uint32_t min_mapq)
{
    if (!c) return BQC_ERR_ARG;
    if (!n_sites) return fail(c, BQC_ERR_ARG, "bqc_enable_site_alleles: the list holds 0 sites");
    if ((uint64_t)c->opt.n_lanes * n_sites > 1ull << 24)
        return fail(c, BQC_ERR_ARG, "bqc_enable_site_alleles: %u sites x %u read groups are more than 16777216 (2^24) rows of counters", n_sites, c->opt.n_lanes);
    if (!rid || !pos) return fail(c, BQC_ERR_ARG, "bqc_enable_site_alleles: the list of %u sites is a null pointer", n_sites);
    if (min_base_qual > 222) return fail(c, BQC_ERR_ARG, "bqc_enable_site_alleles: minimum base quality %u is outside 0 ... 222", min_base_qual);
    if (min_mapq > 255) return fail(c, BQC_ERR_ARG, "bqc_enable_site_alleles: minimum mapping quality %u is outside 0 ... 255", min_mapq);
    const uint32_t n_refs = c->opt.n_refs;
    for (uint32_t i = 0; i < n_sites; ++i) {
        if (rid[i] < 0 || (uint32_t)rid[i] >= n_refs) return fail(c, BQC_ERR_ARG, "bqc_enable_site_alleles: site %u: contig %d is outside 0 ... %u", i, rid[i], n_refs - 1);
        if (pos[i] < 0 || pos[i] > 0x7FFFFFFE) return fail(c, BQC_ERR_ARG, "bqc_enable_site_alleles: site %u: position %d is outside 0 ... 2147483646", i, pos[i]);
        if (i && (rid[i] < rid[i - 1] || (rid[i] == rid[i - 1] && pos[i] <= pos[i - 1])))
            return fail(c, BQC_ERR_ARG, "bqc_enable_site_alleles: site %u: (contig %d, position %d) does not lie behind its predecessor (%d, %d)", i, rid[i], pos[i], rid[i - 1], pos[i - 1]);
    }
    if (c->seg[SEG_SAC].d) return fail(c, BQC_ERR_STATE, "bqc_enable_site_alleles: the module is on already (%u sites)", c->sac_s);
    if (int rc = too_late(c, __func__)) return rc;
    std::vector<uint32_t> first(n_refs + 1, 0), bkt_off(n_refs + 1, 0);
    for (uint32_t i = 0; i < n_sites; ++i) ++first[rid[i] + 1];
    for (uint32_t r = 0; r < n_refs; ++r) first[r + 1] += first[r];
    uint64_t n_bkt = 0;
    for (uint32_t r = 0; r < n_refs; ++r) {
        bkt_off[r] = (uint32_t)n_bkt;
        if (first[r + 1] > first[r]) n_bkt += ((uint64_t)pos[first[r + 1] - 1] >> 12) + 2;
        if (n_bkt > 0xFFFFFFFFull) return fail(c, BQC_ERR_ARG, "bqc_enable_site_alleles: the index of the sites needs more than 2^32 buckets of 4096 bases");
    }
    bkt_off[n_refs] = (uint32_t)n_bkt;
    std::vector<uint32_t> tab; // everything behind the positions
    tab.reserve(2 * (size_t)(n_refs + 1) + n_bkt);
    tab.insert(tab.end(), first.begin(), first.end());
    tab.insert(tab.end(), bkt_off.begin(), bkt_off.end());
    for (uint32_t r = 0; r < n_refs; ++r) {
        const uint64_t nb = bkt_off[r + 1] - bkt_off[r];
        uint32_t s = first[r];
        for (uint64_t k = 0; k < nb; ++k) { // (the entry behind the last bucket: every site lies below its start, so it is first[r + 1])
            while (s < first[r + 1] && (uint64_t)pos[s] < k << 12) ++s;
            tab.push_back(s);
        }
    }
    HIPCHK(c, hipSetDevice(c->device));
    const uint64_t words = bqc_sac_words(c->opt.n_lanes, n_sites);
    const uint64_t tab_bytes = ((uint64_t)n_sites + tab.size()) * 4;
    uint64_t* d = zeroed_words(c, words);
    void* t = nullptr;
    if (!d || hipMalloc(&t, tab_bytes) != hipSuccess || hipMemcpy(t, pos, (uint64_t)n_sites * 4, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy((uint32_t*)t + n_sites, tab.data(), tab.size() * 4, hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipGetLastError();
        (void)hipFree(d);
        (void)hipFree(t);
        return fail(c, BQC_ERR_DEVICE, "bqc_enable_site_alleles: the table (%llu bytes) and the sites (%llu bytes) could not be allocated", (unsigned long long)(words * 8), (unsigned long long)tab_bytes);
    }
    c->sac_sites.pos = (const int32_t*)t;
    c->sac_sites.first = (const uint32_t*)t + n_sites;
    c->sac_sites.bkt_off = c->sac_sites.first + n_refs + 1;
    c->sac_sites.bkt = c->sac_sites.bkt_off + n_refs + 1;
    c->sac_sites.S = n_sites;
    c->sac_sites.n_refs = n_refs;
    c->sac_rid.assign(rid, rid + n_sites);
    c->sac_pos.assign(pos, pos + n_sites);
    c->sac_s = n_sites; c->sac_q = min_base_qual; c->sac_mq = min_mapq;
    c->d_sac_tab = t;
    c->seg[SEG_SAC] = {d, words};
    return 0;
}

// The region tables of k_rcv.hip (device_types.h: RcvRegions) from the checked list: one allocation, [start R][end R][off R + 1][first
// n_refs + 1][bkt_off n_refs + 1][bkt].  The index is over the regions' ends and comes from the list alone.
extern "C" int bqc_enable_region_coverage(bqc_ctx* c, uint32_t n_regions, const int32_t* rid, const int32_t* start, const int32_t* end, uint32_t min_mapq,
                                          uint32_t n_thresholds, const uint64_t* thresholds, uint32_t depth_cap)
{
    if (!c) return BQC_ERR_ARG;
    static const uint64_t default_thr[6] = {1, 10, 20, 30, 50, 100};
    if (!n_regions) return fail(c, BQC_ERR_ARG, "bqc_enable_region_coverage: the list holds 0 regions");
    if (!rid || !start || !end) return fail(c, BQC_ERR_ARG, "bqc_enable_region_coverage: the list of %u regions is a null pointer", n_regions);
    if (min_mapq > 255) return fail(c, BQC_ERR_ARG, "bqc_enable_region_coverage: minimum mapping quality %u is outside 0 ... 255", min_mapq);
    if (n_thresholds > BQC_RCV_MAX_THRESHOLDS) return fail(c, BQC_ERR_ARG, "bqc_enable_region_coverage: %u depth thresholds are more than %d", n_thresholds, BQC_RCV_MAX_THRESHOLDS);
    if (n_thresholds && !thresholds) return fail(c, BQC_ERR_ARG, "bqc_enable_region_coverage: the list of %u depth thresholds is a null pointer", n_thresholds);
    if (!n_thresholds) { thresholds = default_thr; n_thresholds = 6; }
    for (uint32_t t = 0; t < n_thresholds; ++t) {
        if (thresholds[t] < 1 || thresholds[t] > 0xFFFFFFFFull)
            return fail(c, BQC_ERR_ARG, "bqc_enable_region_coverage: depth threshold %u: %llu is outside 1 ... 4294967295", t, (unsigned long long)thresholds[t]);
        if (t && thresholds[t] <= thresholds[t - 1])
            return fail(c, BQC_ERR_ARG, "bqc_enable_region_coverage: depth threshold %u: %llu is not above its predecessor %llu", t, (unsigned long long)thresholds[t], (unsigned long long)thresholds[t - 1]);
    }
    if (depth_cap < 1 || depth_cap > 16383) return fail(c, BQC_ERR_ARG, "bqc_enable_region_coverage: histogram cap %u is outside 1 ... 16383", depth_cap);
    const uint32_t n_refs = c->opt.n_refs;
    uint64_t B = 0;
    for (uint32_t i = 0; i < n_regions; ++i) {
        if (rid[i] < 0 || (uint32_t)rid[i] >= n_refs) return fail(c, BQC_ERR_ARG, "bqc_enable_region_coverage: region %u: contig %d is outside 0 ... %u", i, rid[i], n_refs - 1);
        if (start[i] < 0) return fail(c, BQC_ERR_ARG, "bqc_enable_region_coverage: region %u: start %d is outside 0 ... 2147483646", i, start[i]);
        if (end[i] <= start[i]) return fail(c, BQC_ERR_ARG, "bqc_enable_region_coverage: region %u: end %d does not lie behind start %d", i, end[i], start[i]);
        if (i && (rid[i] < rid[i - 1] || (rid[i] == rid[i - 1] && start[i] < end[i - 1])))
            return fail(c, BQC_ERR_ARG, "bqc_enable_region_coverage: region %u: (contig %d, start %d) does not lie at or behind its predecessor's end (%d, %d)", i, rid[i], start[i], rid[i - 1], end[i - 1]);
        B += (uint64_t)((int64_t)end[i] - start[i]);
    }
    if ((uint64_t)c->opt.n_lanes * (B + n_regions + 4) > 1ull << 28)
        return fail(c, BQC_ERR_ARG, "bqc_enable_region_coverage: %llu bases in %u regions x %u read groups are more than 268435456 (2^28) words", (unsigned long long)B, n_regions, c->opt.n_lanes);
    if (c->seg[SEG_RCV].d) return fail(c, BQC_ERR_STATE, "bqc_enable_region_coverage: the module is on already (%u regions)", c->rcv_r);
    if (int rc = too_late(c, __func__)) return rc;
    std::vector<uint32_t> off(n_regions + 1, 0), first(n_refs + 1, 0), bkt_off(n_refs + 1, 0);
    for (uint32_t i = 0; i < n_regions; ++i) {
        off[i + 1] = off[i] + (uint32_t)(end[i] - start[i]) + 1u;
        ++first[rid[i] + 1];
    }
    for (uint32_t r = 0; r < n_refs; ++r) first[r + 1] += first[r];
    uint64_t n_bkt = 0;
    for (uint32_t r = 0; r < n_refs; ++r) {
        bkt_off[r] = (uint32_t)n_bkt;
        if (first[r + 1] > first[r]) n_bkt += ((uint64_t)end[first[r + 1] - 1] >> 12) + 2;
        if (n_bkt > 0xFFFFFFFFull) return fail(c, BQC_ERR_ARG, "bqc_enable_region_coverage: the index of the regions needs more than 2^32 buckets of 4096 bases");
    }
    bkt_off[n_refs] = (uint32_t)n_bkt;
    std::vector<uint32_t> tab; // everything behind the starts and ends
    tab.reserve((size_t)n_regions + 1 + 2 * (size_t)(n_refs + 1) + n_bkt);
    tab.insert(tab.end(), off.begin(), off.end());
    tab.insert(tab.end(), first.begin(), first.end());
    tab.insert(tab.end(), bkt_off.begin(), bkt_off.end());
    for (uint32_t r = 0; r < n_refs; ++r) {
        const uint64_t nb = bkt_off[r + 1] - bkt_off[r];
        uint32_t s = first[r];
        for (uint64_t k = 0; k < nb; ++k) { // entry k: the first region with end > 4096 k (behind the last bucket: none, first[r + 1])
            while (s < first[r + 1] && (uint64_t)end[s] <= k << 12) ++s;
            tab.push_back(s);
        }
    }
    HIPCHK(c, hipSetDevice(c->device));
    const uint64_t words = bqc_rcv_words(c->opt.n_lanes, B, n_regions);
    const uint64_t tab_bytes = (2 * (uint64_t)n_regions + tab.size()) * 4;
    const uint64_t out_words = bqc_rcv_out_words(c->opt.n_lanes, n_regions, n_thresholds, depth_cap);
    const uint64_t out_all = out_words + (uint64_t)c->opt.n_lanes * bqc_rcv_tiles(B, n_regions);
    uint64_t *d = zeroed_words(c, words), *o = nullptr;
    void* t = nullptr;
    if (!d || hipMalloc(&t, tab_bytes) != hipSuccess || hipMalloc(&o, out_all * 8) != hipSuccess ||
        hipMemcpy(t, start, (uint64_t)n_regions * 4, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy((uint32_t*)t + n_regions, end, (uint64_t)n_regions * 4, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy((uint32_t*)t + 2 * (uint64_t)n_regions, tab.data(), tab.size() * 4, hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipGetLastError();
        (void)hipFree(d);
        (void)hipFree(t);
        (void)hipFree(o);
        return fail(c, BQC_ERR_DEVICE, "bqc_enable_region_coverage: the words (%llu bytes), the regions (%llu bytes) and the products (%llu bytes) could not be allocated", (unsigned long long)(words * 8), (unsigned long long)tab_bytes, (unsigned long long)(out_all * 8));
    }
    RcvRegions& rg = c->rcv_regions;
    rg.start = (const int32_t*)t;
    rg.end = rg.start + n_regions;
    rg.off = (const uint32_t*)(rg.end + n_regions);
    rg.first = rg.off + n_regions + 1;
    rg.bkt_off = rg.first + n_refs + 1;
    rg.bkt = rg.bkt_off + n_refs + 1;
    rg.R = n_regions;
    rg.n_refs = n_refs;
    rg.lane_words = 4 + B + n_regions;
    c->rcv_fp.n_thr = n_thresholds;
    c->rcv_fp.D = depth_cap;
    for (uint32_t k = 0; k < BQC_RCV_MAX_THRESHOLDS; ++k) c->rcv_fp.thr[k] = k < n_thresholds ? (uint32_t)thresholds[k] : 0xFFFFFFFFu;
    c->rcv_thr.assign(thresholds, thresholds + n_thresholds);
    c->rcv_rid.assign(rid, rid + n_regions);
    c->rcv_start.assign(start, start + n_regions);
    c->rcv_end.assign(end, end + n_regions);
    c->rcv_r = n_regions; c->rcv_mq = min_mapq; c->rcv_b = B;
    c->rcv_out_words = out_words;
    c->d_rcv_tab = t;
    c->d_rcv_out = o;
    c->seg[SEG_RCV] = {d, words};
    return 0;
}

// The tables of k_wdp.hip (device_types.h: WdpTab) from the contigs' lengths: one allocation, [len n_refs][woff n_refs + 1], and the
// reciprocal of the window size.
extern "C" int bqc_enable_window_depth(bqc_ctx* c, uint32_t window, const int32_t* ref_len, uint32_t min_mapq)
{
    if (!c) return BQC_ERR_ARG;
    const uint32_t n_refs = c->opt.n_refs, n_lanes = c->opt.n_lanes;
    if (window < 100 || window > 1u << 24) return fail(c, BQC_ERR_ARG, "bqc_enable_window_depth: window size %u is outside 100 ... 16777216 (2^24)", window);
    if (min_mapq > 255) return fail(c, BQC_ERR_ARG, "bqc_enable_window_depth: minimum mapping quality %u is outside 0 ... 255", min_mapq);
    if (!ref_len && n_refs) return fail(c, BQC_ERR_ARG, "bqc_enable_window_depth: the list of %u contig lengths is a null pointer", n_refs);
    std::vector<uint32_t> tab(2 * (size_t)n_refs + 1, 0); // the lengths, then woff
    uint64_t NW = 0;
    for (uint32_t r = 0; r < n_refs; ++r) {
        if (ref_len[r] < 0) return fail(c, BQC_ERR_ARG, "bqc_enable_window_depth: contig %u: length %d is negative", r, ref_len[r]);
        tab[r] = (uint32_t)ref_len[r];
        tab[n_refs + r] = (uint32_t)std::min<uint64_t>(NW, 0xFFFFFFFFull);
        NW += ((uint64_t)ref_len[r] + window - 1) / window;
    }
    if ((uint64_t)n_lanes * (4 + 3 * NW) > 1ull << 28)
        return fail(c, BQC_ERR_ARG, "bqc_enable_window_depth: %llu windows of %u bases x 3 planes x %u read groups are more than 268435456 (2^28) words", (unsigned long long)NW, window, n_lanes);
    tab[2 * (size_t)n_refs] = (uint32_t)NW;
    if (c->seg[SEG_WDP].d) return fail(c, BQC_ERR_STATE, "bqc_enable_window_depth: the module is on already (windows of %u bases)", c->wdp_tab.W);
    if (int rc = too_late(c, __func__)) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    const uint64_t words = bqc_wdp_words(n_lanes, NW);
    uint64_t* d = zeroed_words(c, words);
    void* t = nullptr;
    if (!d || hipMalloc(&t, tab.size() * 4) != hipSuccess || hipMemcpy(t, tab.data(), tab.size() * 4, hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipGetLastError();
        (void)hipFree(d);
        (void)hipFree(t);
        return fail(c, BQC_ERR_DEVICE, "bqc_enable_window_depth: the words (%llu bytes) and the contigs' tables (%llu bytes) could not be allocated", (unsigned long long)(words * 8), (unsigned long long)(tab.size() * 4));
    }
    uint32_t l = 0; // ceil(log2 W)
    while ((1u << l) < window) ++l;
    WdpTab& T = c->wdp_tab;
    T.len = (const uint32_t*)t;
    T.woff = T.len + n_refs;
    T.n_refs = n_refs;
    T.NW = (uint32_t)NW;
    T.W = window;
    T.shift = 31 + l;
    T.mul = (uint32_t)(((1ull << T.shift) + window - 1) / window); // (2^31 for a power of two, otherwise between 2^31 and 2^32)
    T.lane_words = (uint32_t)(4 + 3 * NW);
    c->wdp_len.assign(tab.begin(), tab.begin() + n_refs);
    c->wdp_woff.assign(tab.begin() + n_refs, tab.end());
    c->wdp_mq = min_mapq;
    c->d_wdp_tab = t;
    c->seg[SEG_WDP] = {d, words};
    return 0;
}

// The table of k_dup.hip: one allocation, [C slots][the counter of sets, 7 spare words][n_lanes][5 sums][k_dup_final's products].  The
// clear is left on the compute stream, in front of the first batch.
extern "C" int bqc_enable_duplicate_sets(bqc_ctx* c, uint64_t capacity)
{
    if (!c) return BQC_ERR_ARG;
    if (capacity < 16 || capacity > 1ull << 31)
        return fail(c, BQC_ERR_ARG, "bqc_enable_duplicate_sets: capacity %llu is outside 16 ... 2147483648 (2^31) signatures", (unsigned long long)capacity);
    if (c->d_dup) return fail(c, BQC_ERR_STATE, "bqc_enable_duplicate_sets: the module is on already (capacity %llu)", (unsigned long long)c->dup_tab.capacity);
    if (int rc = too_late(c, __func__)) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    const uint64_t C = bqc_dup_slots(capacity);
    const uint64_t bytes = C * sizeof(DupSlot) + (8 + (uint64_t)c->opt.n_lanes * 5 + bqc_dup_out_words()) * 8;
    void* d = nullptr;
    if (hipMalloc(&d, bytes) != hipSuccess) {
        (void)hipGetLastError();
        return fail(c, BQC_ERR_DEVICE, "bqc_enable_duplicate_sets: the table of %llu slots for a capacity of %llu signatures (%llu bytes) could not be allocated", (unsigned long long)C, (unsigned long long)capacity, (unsigned long long)bytes);
    }
    DupTable& T = c->dup_tab;
    T.slots = (DupSlot*)d;
    T.n_sets = (uint64_t*)(T.slots + C);
    T.mask = C - 1;
    T.capacity = capacity;
    c->d_dup_sums = T.n_sets + 8;
    c->d_dup_out = c->d_dup_sums + (uint64_t)c->opt.n_lanes * 5;
    bqc_launch_dup_clear(T, c->d_dup_sums, c->opt.n_lanes, c->n_cu, c->stream);
    if (hipGetLastError() != hipSuccess) {
        (void)hipFree(d);
        T = DupTable{};
        c->d_dup_sums = c->d_dup_out = nullptr;
        return fail(c, BQC_ERR_DEVICE, "bqc_enable_duplicate_sets: the table could not be cleared");
    }
    c->d_dup = d;
    return 0;
}

// The table of k_ovr.hip: one allocation, [C slots][the counter of sets, 7 spare words][n_lanes][4 sums][k_ovr_final's products: the
// head and a list of 2 floor(10^6 / ppm) sets].  The clear is left on the compute stream, in front of the first batch.
extern "C" int bqc_enable_overrepresented(bqc_ctx* c, uint32_t K, uint32_t ppm, uint64_t capacity)
{
    if (!c) return BQC_ERR_ARG;
    if (K < BQC_OVR_KMIN || K > BQC_OVR_KMAX) return fail(c, BQC_ERR_ARG, "bqc_enable_overrepresented: prefix length %u is outside %d ... %d bases", K, BQC_OVR_KMIN, BQC_OVR_KMAX);
    if (ppm < 10 || ppm > 1000000) return fail(c, BQC_ERR_ARG, "bqc_enable_overrepresented: threshold %u is outside 10 ... 1000000 reads per million", ppm);
    if (capacity < 16 || capacity > 1ull << 31)
        return fail(c, BQC_ERR_ARG, "bqc_enable_overrepresented: capacity %llu is outside 16 ... 2147483648 (2^31) sequences", (unsigned long long)capacity);
    if (c->d_ovr) return fail(c, BQC_ERR_STATE, "bqc_enable_overrepresented: the module is on already (prefix length %u, capacity %llu)", c->ovr_k, (unsigned long long)c->ovr_tab.capacity);
    if (int rc = too_late(c, __func__)) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    const uint64_t C = bqc_dup_slots(capacity), list_cap = 2ull * (1000000u / ppm);
    const uint64_t bytes = C * sizeof(DupSlot) + (8 + (uint64_t)c->opt.n_lanes * 4 + bqc_ovr_out_words(list_cap)) * 8;
    void* d = nullptr;
    if (hipMalloc(&d, bytes) != hipSuccess) {
        (void)hipGetLastError();
        return fail(c, BQC_ERR_DEVICE, "bqc_enable_overrepresented: the table of %llu slots for a capacity of %llu sequences (%llu bytes) could not be allocated", (unsigned long long)C, (unsigned long long)capacity, (unsigned long long)bytes);
    }
    DupTable& T = c->ovr_tab;
    T.slots = (DupSlot*)d;
    T.n_sets = (uint64_t*)(T.slots + C);
    T.mask = C - 1;
    T.capacity = capacity;
    c->d_ovr_sums = T.n_sets + 8;
    c->d_ovr_out = c->d_ovr_sums + (uint64_t)c->opt.n_lanes * 4;
    bqc_launch_ovr_clear(T, c->d_ovr_sums, c->opt.n_lanes, c->n_cu, c->stream);
    if (hipGetLastError() != hipSuccess) {
        (void)hipFree(d);
        T = DupTable{};
        c->d_ovr_sums = c->d_ovr_out = nullptr;
        return fail(c, BQC_ERR_DEVICE, "bqc_enable_overrepresented: the table could not be cleared");
    }
    c->d_ovr = d;
    c->ovr_k = K;
    c->ovr_ppm = ppm;
    c->ovr_list_cap = list_cap;
    return 0;
}

// The view's list from k_ovr_final's (c->h_ovr_out): letters, possible source, and the order — mate, count descending, sequence ascending.
static void ovr_make_list(bqc_ctx* c, uint64_t n_sets)
{
    struct Item { std::string seq; uint64_t count; uint32_t mate; };
    std::vector<Item> items(n_sets);
    for (uint64_t e = 0; e < n_sets; ++e) {
        const uint64_t* w = c->h_ovr_out.data() + BQC_OVR_HEAD + 3 * e;
        const uint32_t n = (uint32_t)(w[0] >> 56) & 63u;
        Item& it = items[e];
        it.mate = (uint32_t)(w[0] >> 62) & 1u;
        it.count = w[2];
        it.seq.resize(n);
        for (uint32_t i = 0; i < n; ++i) it.seq[i] = "ACGT"[(i < 28 ? w[0] >> (2 * i) : w[1] >> (2 * (i - 28))) & 3u];
    }
    std::sort(items.begin(), items.end(), [](const Item& a, const Item& b) {
        if (a.mate != b.mate) return a.mate < b.mate;
        if (a.count != b.count) return a.count > b.count;
        return a.seq < b.seq;
    });
    c->ovr_text.resize(n_sets);
    c->ovr_listed.resize(n_sets);
    c->ovr_n_listed[0] = c->ovr_n_listed[1] = 0;
    for (uint64_t e = 0; e < n_sets; ++e) {
        c->ovr_text[e].swap(items[e].seq);
        c->ovr_listed[e] = bqc_ovr_seq{c->ovr_text[e].c_str(), items[e].count, bqc_possible_source(c->ovr_text[e].c_str())};
        ++c->ovr_n_listed[items[e].mate];
    }
}

// Picard's estimateLibrarySize: the library size x with c = x (1 - exp(-n / x)) for n read pairs of which c are unique, by bisection
static uint64_t dup_library_size(uint64_t n_reads, uint64_t n_unique)
{
    if (!n_unique || n_unique >= n_reads) return 0;
    const double n = (double)n_reads, c = (double)n_unique;
    auto f = [&](double x) { return c / x - 1 + exp(-n / x); };
    double m = 1, M = 100;
    while (f(M * c) > 0) M *= 10;
    for (int i = 0; i < 40; ++i) {
        const double r = (m + M) / 2, u = f(r * c);
        if (u == 0) break;
        if (u > 0) m = r;
        else M = r;
    }
    return (uint64_t)(c * (m + M) / 2);
}

extern "C" int bqc_finalize(bqc_ctx* c, const bqc_counts** out)
{
    if (!c || !out) return BQC_ERR_ARG;
    c->modules_closed = true;
    int rc = bqc_flush(c);
    if (rc) return rc;
    const StateLayout& sl = c->sl;
    c->h_state.resize(sl.words);
    HIPCHK(c, hipMemcpy(c->h_state.data(), c->d_state, sl.words * 8, hipMemcpyDeviceToHost));
    c->arrays.clear();
    c->lanes.assign(sl.n_lanes, bqc_lane_counts{});
    c->sk_out.assign(sl.n_lanes, {});
    auto keep = [&](std::vector<uint64_t>&& v) -> const uint64_t* {
        c->arrays.push_back(std::move(v));
        return c->arrays.back().data();
    };
    auto u32copy = [&](const uint64_t* p, uint32_t n) { // reference type `unsigned`: value mod 2^32
        std::vector<uint64_t> v(n ? n : 1);
        for (uint32_t i = 0; i < n; ++i) v[i] = p[i] & 0xFFFFFFFFull;
        return v;
    };
    c->arrays.reserve(sl.n_lanes * 64);
    for (uint32_t l = 0; l < sl.n_lanes; ++l) {
        const uint64_t* S = c->h_state.data() + sl.lane_base(l);
        bqc_lane_counts& L = c->lanes[l];
        for (int i = 0; i < BQC_N_SCALARS; ++i)
            L.scalars[i] = i == BQC_S_TOTALBPS ? S[sl.o_scalars + i] : (S[sl.o_scalars + i] & 0xFFFFFFFFull);
        for (int i = 0; i <= BQC_COVSIZE; ++i) L.poscov[i] = S[sl.o_poscov + i];
        if (S[sl.o_covstart] == 0) L.poscov[0] += 2 * BQC_VSIZE; // lane never saw coverage(): final flush of two empty windows
        for (int i = 0; i <= BQC_COVSIZE; ++i) L.poscov[i] &= 0xFFFFFFFFull;
        L.eightmer = S + sl.o_eightmer;
        L.triplet = S + sl.o_triplet;
        for (uint32_t m = 0; m < 2; ++m) {
            const uint64_t* Mq = S + sl.o_mate[m];
            bqc_mate_counts& mc = L.mate[m];
            const uint32_t n_rl = last_nonzero_len(Mq + sl.m_readlen, sl.lcap + 1); // maxL + 1, or 0 when no read
            const uint32_t ncyc = n_rl ? n_rl - 1 : 0;
            mc.n_cycles = ncyc;
            for (int j = 0; j < 5; ++j) mc.dnacount[j] = Mq + sl.m_dnacount + (uint64_t)j * sl.lcap;
            mc.qualcount = Mq + sl.m_qualcount;
            mc.qualcount_readnr = Mq[sl.m_readnr] & 0xFFFFFFFFull;
            { // sc5[j] = #reads whose leading clip exceeds j (suffix sum of the clip-length histogram)
                std::vector<uint64_t> v(ncyc ? ncyc : 1, 0);
                uint64_t run = 0;
                for (uint32_t j = sl.lcap + 1; j-- > 0;) {
                    if (j < ncyc) v[j] = run & 0xFFFFFFFFull; // run = sum_{n > j} H[n]
                    run += Mq[sl.m_sc5hist + j];
                }
                // v[j] = sum_{n > j} H[n]
                mc.sc5 = keep(std::move(v));
            }
            { // sc3 = prefix sum of the difference array
                std::vector<uint64_t> v(ncyc ? ncyc : 1, 0);
                uint64_t run = 0;
                for (uint32_t j = 0; j < ncyc; ++j) { run += Mq[sl.m_sc3diff + j]; v[j] = run & 0xFFFFFFFFull; }
                mc.sc3 = keep(std::move(v));
            }
            mc.n_Ncount = n_rl; mc.Ncount = keep(u32copy(Mq + sl.m_ncount, n_rl));
            mc.n_GCcount = n_rl; mc.GCcount = Mq + sl.m_gccount;
            mc.n_averageQual = last_nonzero_len(Mq + sl.m_avgceil, 256);
            mc.averageQual = keep(u32copy(Mq + sl.m_avgqual, mc.n_averageQual));
            mc.n_insertSize = sl.icap; mc.insertSize = keep(u32copy(Mq + sl.m_insert, sl.icap));
            mc.n_mapQ = last_nonzero_len(Mq + sl.m_mapq, 256); mc.mapQ = keep(u32copy(Mq + sl.m_mapq, mc.n_mapQ));
            mc.n_readLength = n_rl; mc.readLength = keep(u32copy(Mq + sl.m_readlen, n_rl));
            mc.n_mismatch = last_nonzero_len(Mq + sl.m_mismatch, sl.hcap); mc.mismatch = keep(u32copy(Mq + sl.m_mismatch, mc.n_mismatch));
            mc.n_delhist = last_nonzero_len(Mq + sl.m_delhist, sl.hcap); mc.delhist = keep(u32copy(Mq + sl.m_delhist, mc.n_delhist));
            mc.n_inshist = last_nonzero_len(Mq + sl.m_inshist, sl.hcap); mc.inshist = keep(u32copy(Mq + sl.m_inshist, mc.n_inshist));
        }
        if (c->sketch) {
            std::string e;
            if (!sketch_finalize(c->sketch, l, c->sk_out[l], c->stream, e)) return fail(c, BQC_ERR_DEVICE, "sketch finalize: %s", e.c_str());
            L.n_sketch = (uint32_t)c->sk_out[l].size();
            L.sketch = c->sk_out[l].data();
        }
    }
    if (c->seg[SEG_QCYC].d) { // the printed sizes follow from the sums: cycles from the mate's read lengths, qualities from the table itself
        const uint32_t N = c->opt.qual_by_cycle;
        if ((rc = fetch_segment(c, SEG_QCYC, c->h_qcyc))) return rc;
        c->qcyc_ncyc.assign((size_t)sl.n_lanes * 2, 0);
        c->qcyc_nq.assign((size_t)sl.n_lanes * 2, 0);
        for (uint32_t l = 0; l < sl.n_lanes; ++l)
            for (uint32_t m = 0; m < 2; ++m) {
                const uint64_t* H = c->h_qcyc.data() + ((uint64_t)l * 2 + m) * N * 224;
                uint32_t nq = 0;
                for (uint32_t cy = 0; cy < N; ++cy) nq = std::max(nq, last_nonzero_len(H + (uint64_t)cy * 224, 224));
                c->qcyc_ncyc[l * 2 + m] = std::min(N, c->lanes[l].mate[m].n_cycles);
                c->qcyc_nq[l * 2 + m] = nq;
            }
        c->finalised[SEG_QCYC] = true;
    }
    if (c->seg[SEG_MBC].d) { // the same for the two tables of a lane and mate: the quality range is that of A (M <= A cell by cell)
        const uint32_t N = c->opt.mismatch_by_cycle;
        if ((rc = fetch_segment(c, SEG_MBC, c->h_mbc))) return rc;
        c->mbc_ncyc.assign((size_t)sl.n_lanes * 2, 0);
        c->mbc_nq.assign((size_t)sl.n_lanes * 2, 0);
        for (uint32_t l = 0; l < sl.n_lanes; ++l)
            for (uint32_t m = 0; m < 2; ++m) {
                const uint64_t* A = c->h_mbc.data() + ((uint64_t)l * 2 + m) * 2 * N * 224;
                uint32_t nq = 0;
                for (uint32_t cy = 0; cy < N; ++cy) nq = std::max(nq, last_nonzero_len(A + (uint64_t)cy * 224, 224));
                c->mbc_ncyc[l * 2 + m] = std::min(N, c->lanes[l].mate[m].n_cycles);
                c->mbc_nq[l * 2 + m] = nq;
            }
        c->finalised[SEG_MBC] = true;
    }
    if (c->seg[SEG_ADP].d) { // the printed length follows from the module's own sums: the longest examined read of the lane and mate, cut at N
        const uint32_t N = c->adp_n;
        if ((rc = fetch_segment(c, SEG_ADP, c->h_adp))) return rc;
        c->adp_ncyc.assign((size_t)sl.n_lanes * 2, 0);
        for (uint32_t l = 0; l < sl.n_lanes; ++l)
            for (uint32_t m = 0; m < 2; ++m)
                c->adp_ncyc[l * 2 + m] = last_nonzero_len(c->h_adp.data() + (((uint64_t)l * 2 + m) * BQC_ADP_ROWS + BQC_ADP_MAX) * N, N);
        c->finalised[SEG_ADP] = true;
    }
    if (c->seg[SEG_RCV].d) { // k_rcv_final: the depths from the difference words, which it leaves as they are
        const uint32_t n_lanes = c->opt.n_lanes, R = c->rcv_r;
        c->finalised[SEG_RCV] = false;
        timed_launch(c, !c->seg[SEG_GCB].d, "k_rcv_final", [&] { bqc_launch_rcv_final(c->seg[SEG_RCV].d, c->rcv_regions, c->rcv_fp, n_lanes, c->d_rcv_out + c->rcv_out_words, c->d_rcv_out, c->stream); });
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipStreamSynchronize(c->stream));
        c->h_rcv_out.resize(c->rcv_out_words);
        HIPCHK(c, hipMemcpy(c->h_rcv_out.data(), c->d_rcv_out, c->rcv_out_words * 8, hipMemcpyDeviceToHost));
        c->h_rcv_eta.assign((size_t)n_lanes * 4, 0);
        HIPCHK(c, hipMemcpy2D(c->h_rcv_eta.data(), 32, c->seg[SEG_RCV].d, c->rcv_regions.lane_words * 8, 32, n_lanes, hipMemcpyDeviceToHost));
        const uint64_t bad = c->h_rcv_out[c->rcv_out_words - 1];
        if (bad != ~0ull)
            return fail(c, BQC_ERR_STATE, "bqc_finalize: region coverage: the words are not a difference array of this list of regions: region %llu (contig %d, %d ... %d) does not close at depth 0 (state imported from a context with another list?)",
                        (unsigned long long)bad, c->rcv_rid[bad], c->rcv_start[bad], c->rcv_end[bad]);
        const uint32_t C = 3 + c->rcv_fp.n_thr;
        const uint64_t lane_out = (uint64_t)R * C + c->rcv_fp.D + 1;
        for (uint32_t l = 0; l < n_lanes; ++l) { // (word 3 of a read group's header is 0 in the state; the view's copy holds the bases on target)
            uint64_t on = 0;
            for (uint32_t k = 0; k < R; ++k) on += c->h_rcv_out[l * lane_out + (uint64_t)k * C];
            c->h_rcv_eta[(size_t)l * 4 + 3] = on;
        }
        c->finalised[SEG_RCV] = true;
    }
    if (c->d_dup) { // k_dup_final: the sets by class and size from the table, which it leaves as it is
        c->finalised[MOD_DUP] = false;
        timed_launch(c, !c->seg[SEG_GCB].d && !c->seg[SEG_RCV].d, "k_dup_final", [&] { bqc_launch_dup_final(c->dup_tab, c->d_dup_out, c->n_cu, c->stream); });
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipStreamSynchronize(c->stream));
        c->h_dup_out.resize(bqc_dup_out_words());
        c->h_dup_sums.resize((size_t)c->opt.n_lanes * 5);
        HIPCHK(c, hipMemcpy(c->h_dup_out.data(), c->d_dup_out, c->h_dup_out.size() * 8, hipMemcpyDeviceToHost));
        HIPCHK(c, hipMemcpy(c->h_dup_sums.data(), c->d_dup_sums, c->h_dup_sums.size() * 8, hipMemcpyDeviceToHost));
        uint64_t pairs = 0;
        for (uint32_t k = 0; k < 2; ++k) {
            c->dup_sets[k] = 0;
            for (uint32_t i = 0; i < BQC_DUP_BINS; ++i) c->dup_sets[k] += c->h_dup_out[(size_t)k * BQC_DUP_BINS + i];
        }
        for (uint32_t l = 0; l < c->opt.n_lanes; ++l) pairs += c->h_dup_sums[(size_t)l * 5 + 1];
        c->dup_estimate = dup_library_size(pairs, c->dup_sets[1]);
        c->finalised[MOD_DUP] = true;
    }
    if (c->d_ovr) { // k_ovr_final: the sets by mate and size and the list from the table, which it leaves as it is; the thresholds come from the sums
        const uint32_t n_lanes = c->opt.n_lanes;
        c->finalised[MOD_OVR] = false;
        HIPCHK(c, hipStreamSynchronize(c->stream));
        c->h_ovr_sums.resize((size_t)n_lanes * 4);
        HIPCHK(c, hipMemcpy(c->h_ovr_sums.data(), c->d_ovr_sums, c->h_ovr_sums.size() * 8, hipMemcpyDeviceToHost));
        for (uint32_t m = 0; m < 2; ++m) {
            uint64_t entered = 0;
            for (uint32_t l = 0; l < n_lanes; ++l) entered += c->h_ovr_sums[(size_t)l * 4 + m] - c->h_ovr_sums[(size_t)l * 4 + 2 + m];
            c->ovr_threshold[m] = std::max<uint64_t>(2, (entered * c->ovr_ppm + 999999) / 1000000); // (entered < 2^40 reads: the product stays below 2^60)
        }
        timed_launch(c, !c->seg[SEG_GCB].d && !c->seg[SEG_RCV].d && !c->d_dup, "k_ovr_final", [&] { bqc_launch_ovr_final(c->ovr_tab, c->ovr_threshold, c->d_ovr_out, c->ovr_list_cap, &c->d_err0->flags, c->n_cu, c->stream); });
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipStreamSynchronize(c->stream));
        c->h_ovr_out.resize(BQC_OVR_HEAD);
        HIPCHK(c, hipMemcpy(c->h_ovr_out.data(), c->d_ovr_out, BQC_OVR_HEAD * 8, hipMemcpyDeviceToHost));
        const uint64_t n_sets = c->h_ovr_out[BQC_OVR_HEAD - 2];
        if (n_sets > c->ovr_list_cap)
            return fail(c, BQC_ERR_DEVICE, "internal error: overrepresented sequences: %llu sets reach the thresholds, the list holds %llu", (unsigned long long)n_sets, (unsigned long long)c->ovr_list_cap);
        c->h_ovr_out.resize(bqc_ovr_out_words(n_sets));
        if (n_sets) HIPCHK(c, hipMemcpy(c->h_ovr_out.data() + BQC_OVR_HEAD, c->d_ovr_out + BQC_OVR_HEAD, n_sets * 24, hipMemcpyDeviceToHost));
        for (uint32_t m = 0; m < 2; ++m) {
            c->ovr_distinct[m] = 0;
            for (uint32_t i = 0; i < BQC_DUP_BINS; ++i) c->ovr_distinct[m] += c->h_ovr_out[(size_t)m * BQC_DUP_BINS + i];
        }
        ovr_make_list(c, n_sets);
        c->finalised[MOD_OVR] = true;
    }
    if (c->seg[SEG_WDP].d) { // the sums by contig and the histogram over the main contigs' windows: one pass over a copy of the words, no kernel
        const uint32_t n_lanes = c->opt.n_lanes, n_refs = c->opt.n_refs, W = c->wdp_tab.W;
        const uint64_t NW = c->wdp_tab.NW, LW = c->wdp_tab.lane_words;
        c->finalised[SEG_WDP] = false;
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if ((rc = fetch_segment(c, SEG_WDP, c->h_wdp))) return rc;
        c->h_wdp_contigs.assign((size_t)n_lanes * n_refs * 3, 0);
        c->h_wdp_hist.assign((size_t)n_lanes * BQC_WDP_HIST_BINS, 0);
        for (uint32_t l = 0; l < n_lanes; ++l) {
            const uint64_t* reads = c->h_wdp.data() + l * LW + 4;
            const uint64_t *bases = reads + NW, *low = bases + NW;
            uint64_t* hist = c->h_wdp_hist.data() + (size_t)l * BQC_WDP_HIST_BINS;
            for (uint32_t r = 0; r < n_refs; ++r) {
                uint64_t* sum = c->h_wdp_contigs.data() + ((size_t)l * n_refs + r) * 3;
                const bool main = r < c->main_chrom.size() && c->main_chrom[r] == 1;
                for (uint32_t w = c->wdp_woff[r]; w < c->wdp_woff[r + 1]; ++w) {
                    sum[0] += reads[w]; sum[1] += bases[w]; sum[2] += low[w];
                    if (main) {
                        const uint64_t k = w - c->wdp_woff[r], from = k * W, len = std::min<uint64_t>(from + W, c->wdp_len[r]) - from; // (>= 1)
                        const uint64_t depth = bases[w] / len;
                        ++hist[depth < BQC_WDP_HIST_BINS - 1 ? depth : BQC_WDP_HIST_BINS - 1];
                    }
                }
            }
        }
        c->finalised[SEG_WDP] = true;
    }
    if (c->seg[SEG_SAC].d) {
        if ((rc = fetch_segment(c, SEG_SAC, c->h_sac))) return rc;
        c->finalised[SEG_SAC] = true;
    }
    if (c->seg[SEG_SBC].d) {
        if ((rc = fetch_segment(c, SEG_SBC, c->h_sbc))) return rc;
        const uint32_t N = c->sbc_n;
        c->sbc_ncyc.assign((size_t)sl.n_lanes * 2, 0);
        for (uint32_t l = 0; l < sl.n_lanes; ++l)
            for (int m = 0; m < 2; ++m) // (Y of a (lane, mate): 16 words a cycle)
                c->sbc_ncyc[l * 2 + m] = (last_nonzero_len(c->h_sbc.data() + ((uint64_t)l * 2 + m) * BQC_SBC_MATE_WORDS(N) + BQC_SBC_X_WORDS, 16 * N) + 15) / 16;
        c->finalised[SEG_SBC] = true;
    }
    if (c->seg[SEG_IBC].d) {
        if ((rc = fetch_segment(c, SEG_IBC, c->h_ibc))) return rc;
        const uint32_t N = c->ibc_n;
        c->ibc_ncyc.assign((size_t)sl.n_lanes * 2, 0);
        for (uint32_t l = 0; l < sl.n_lanes; ++l)
            for (int m = 0; m < 2; ++m) // (row 0 of a (lane, mate): E)
                c->ibc_ncyc[l * 2 + m] = last_nonzero_len(c->h_ibc.data() + ((uint64_t)l * 2 + m) * BQC_IBC_MATE_WORDS(N), N);
        c->finalised[SEG_IBC] = true;
    }
    if (c->seg[SEG_GCB].d) {
        rc = gcb_genome_table(c);
        if (rc) return rc;
        if ((rc = fetch_segment(c, SEG_GCB, c->h_gcb))) return rc;
        c->finalised[SEG_GCB] = true;
    }
    c->counts.n_lanes = sl.n_lanes;
    c->counts.lanes = c->lanes.data();
    *out = &c->counts;
    return 0;
}

extern "C" int bqc_qual_by_cycle(bqc_ctx* c, uint32_t lane, uint32_t mate, bqc_qbc_view* out)
{
    if (!c || !out) return BQC_ERR_ARG;
    if (!c->seg[SEG_QCYC].d) return fail(c, BQC_ERR_STATE, "bqc_qual_by_cycle: the context was created without qual_by_cycle");
    if (!c->finalised[SEG_QCYC]) return fail(c, BQC_ERR_STATE, "bqc_qual_by_cycle: nothing has been finalised");
    if (lane >= c->opt.n_lanes || mate > 1) return fail(c, BQC_ERR_ARG, "bqc_qual_by_cycle: lane %u / mate %u out of range", lane, mate);
    out->n_cycles = c->qcyc_ncyc[lane * 2 + mate];
    out->n_q = c->qcyc_nq[lane * 2 + mate];
    out->stride = 224;
    out->hist = c->h_qcyc.data() + ((uint64_t)lane * 2 + mate) * c->opt.qual_by_cycle * 224;
    return 0;
}

extern "C" int bqc_mismatch_by_cycle(bqc_ctx* c, uint32_t lane, uint32_t mate, bqc_mbc_view* out)
{
    if (!c || !out) return BQC_ERR_ARG;
    if (!c->seg[SEG_MBC].d) return fail(c, BQC_ERR_STATE, "bqc_mismatch_by_cycle: the context was created without mismatch_by_cycle");
    if (!c->finalised[SEG_MBC]) return fail(c, BQC_ERR_STATE, "bqc_mismatch_by_cycle: nothing has been finalised");
    if (lane >= c->opt.n_lanes || mate > 1) return fail(c, BQC_ERR_ARG, "bqc_mismatch_by_cycle: lane %u / mate %u out of range", lane, mate);
    const uint64_t tbl = (uint64_t)c->opt.mismatch_by_cycle * 224;
    out->n_cycles = c->mbc_ncyc[lane * 2 + mate];
    out->n_q = c->mbc_nq[lane * 2 + mate];
    out->stride = 224;
    out->aligned = c->h_mbc.data() + ((uint64_t)lane * 2 + mate) * 2 * tbl;
    out->mismatch = out->aligned + tbl;
    return 0;
}

extern "C" int bqc_adapter_by_cycle(bqc_ctx* c, uint32_t lane, uint32_t mate, bqc_adp_view* out)
{
    if (!c || !out) return BQC_ERR_ARG;
    if (!c->seg[SEG_ADP].d) return fail(c, BQC_ERR_STATE, "bqc_adapter_by_cycle: the context was created without adapter_by_cycle");
    if (!c->finalised[SEG_ADP]) return fail(c, BQC_ERR_STATE, "bqc_adapter_by_cycle: nothing has been finalised");
    if (lane >= c->opt.n_lanes || mate > 1) return fail(c, BQC_ERR_ARG, "bqc_adapter_by_cycle: lane %u / mate %u out of range", lane, mate);
    out->n_cycles = c->adp_ncyc[lane * 2 + mate];
    out->n_adapters = (uint32_t)c->adp_set.size();
    out->stride = c->adp_n;
    out->first_hit = c->h_adp.data() + ((uint64_t)lane * 2 + mate) * BQC_ADP_ROWS * c->adp_n;
    out->reads_by_length = out->first_hit + (uint64_t)BQC_ADP_MAX * c->adp_n;
    out->adapters = c->adp_set.data();
    return 0;
}

extern "C" int bqc_gc_bias(bqc_ctx* c, uint32_t lane, bqc_gcb_view* out)
{
    if (!c || !out) return BQC_ERR_ARG;
    if (!c->seg[SEG_GCB].d) return fail(c, BQC_ERR_STATE, "bqc_gc_bias: bqc_enable_gc_bias has not been called for the context");
    if (!c->finalised[SEG_GCB]) return fail(c, BQC_ERR_STATE, "bqc_gc_bias: nothing has been finalised");
    if (lane >= c->opt.n_lanes) return fail(c, BQC_ERR_ARG, "bqc_gc_bias: lane %u out of range", lane);
    out->window = c->gcb_w;
    out->n_bins = BQC_GCB_BINS;
    out->genome_windows = c->h_gcb_g.data();
    out->read_starts = c->h_gcb.data() + (uint64_t)lane * BQC_GCB_ROWS * BQC_GCB_BINS;
    out->bases = out->read_starts + BQC_GCB_BINS;
    out->qual_sum = out->bases + BQC_GCB_BINS;
    return 0;
}

extern "C" int bqc_indel_by_cycle(bqc_ctx* c, uint32_t lane, uint32_t mate, bqc_ibc_view* out)
{
    if (!c || !out) return BQC_ERR_ARG;
    if (!c->seg[SEG_IBC].d) return fail(c, BQC_ERR_STATE, "bqc_indel_by_cycle: bqc_enable_indel_by_cycle has not been called for the context");
    if (!c->finalised[SEG_IBC]) return fail(c, BQC_ERR_STATE, "bqc_indel_by_cycle: nothing has been finalised");
    if (lane >= c->opt.n_lanes || mate > 1) return fail(c, BQC_ERR_ARG, "bqc_indel_by_cycle: lane %u / mate %u out of range", lane, mate);
    const uint32_t N = c->ibc_n;
    out->n_cycles = c->ibc_ncyc[lane * 2 + mate];
    out->n_len = BQC_IBC_K;
    out->reads_by_length = c->h_ibc.data() + ((uint64_t)lane * 2 + mate) * BQC_IBC_MATE_WORDS(N);
    out->insertions = out->reads_by_length + N;
    out->deletions = out->insertions + N;
    out->insertion_lengths = out->deletions + N;
    out->deletion_lengths = out->insertion_lengths + BQC_IBC_K;
    return 0;
}

extern "C" int bqc_substitutions(bqc_ctx* c, uint32_t lane, uint32_t mate, bqc_sbc_view* out)
{
    if (!c || !out) return BQC_ERR_ARG;
    if (!c->seg[SEG_SBC].d) return fail(c, BQC_ERR_STATE, "bqc_substitutions: bqc_enable_substitutions has not been called for the context");
    if (!c->finalised[SEG_SBC]) return fail(c, BQC_ERR_STATE, "bqc_substitutions: nothing has been finalised");
    if (lane >= c->opt.n_lanes || mate > 1) return fail(c, BQC_ERR_ARG, "bqc_substitutions: lane %u / mate %u out of range", lane, mate);
    out->n_cycles = c->sbc_ncyc[lane * 2 + mate];
    out->min_base_qual = c->sbc_q;
    out->min_mapq = c->sbc_mq;
    out->by_context = c->h_sbc.data() + ((uint64_t)lane * 2 + mate) * BQC_SBC_MATE_WORDS(c->sbc_n);
    out->by_cycle = out->by_context + BQC_SBC_X_WORDS;
    return 0;
}

extern "C" int bqc_site_alleles(bqc_ctx* c, uint32_t lane, bqc_sac_view* out)
{
    if (!c || !out) return BQC_ERR_ARG;
    if (!c->seg[SEG_SAC].d) return fail(c, BQC_ERR_STATE, "bqc_site_alleles: bqc_enable_site_alleles has not been called for the context");
    if (!c->finalised[SEG_SAC]) return fail(c, BQC_ERR_STATE, "bqc_site_alleles: nothing has been finalised");
    if (lane >= c->opt.n_lanes) return fail(c, BQC_ERR_ARG, "bqc_site_alleles: lane %u out of range", lane);
    out->n_sites = c->sac_s;
    out->min_base_qual = c->sac_q;
    out->min_mapq = c->sac_mq;
    out->rid = c->sac_rid.data();
    out->pos = c->sac_pos.data();
    out->counts = c->h_sac.data() + (uint64_t)lane * c->sac_s * 8;
    return 0;
}

extern "C" int bqc_region_coverage(bqc_ctx* c, uint32_t lane, bqc_rcv_view* out)
{
    if (!c || !out) return BQC_ERR_ARG;
    if (!c->seg[SEG_RCV].d) return fail(c, BQC_ERR_STATE, "bqc_region_coverage: bqc_enable_region_coverage has not been called for the context");
    if (!c->finalised[SEG_RCV]) return fail(c, BQC_ERR_STATE, "bqc_region_coverage: nothing has been finalised");
    if (lane >= c->opt.n_lanes) return fail(c, BQC_ERR_ARG, "bqc_region_coverage: lane %u out of range", lane);
    const uint32_t C = 3 + c->rcv_fp.n_thr;
    const uint64_t lane_out = (uint64_t)c->rcv_r * C + c->rcv_fp.D + 1;
    const uint64_t* eta = c->h_rcv_eta.data() + (size_t)lane * 4;
    out->n_regions = c->rcv_r;
    out->min_mapq = c->rcv_mq;
    out->n_thresholds = c->rcv_fp.n_thr;
    out->depth_cap = c->rcv_fp.D;
    out->rid = c->rcv_rid.data();
    out->start = c->rcv_start.data();
    out->end = c->rcv_end.data();
    out->reads_examined = eta[0];
    out->reads_on_target = eta[1];
    out->aligned_bases = eta[2];
    out->bases_on_target = eta[3];
    out->target_bases = c->rcv_b;
    out->thresholds = c->rcv_thr.data();
    out->regions = c->h_rcv_out.data() + lane * lane_out;
    out->hist = out->regions + (uint64_t)c->rcv_r * C;
    return 0;
}

extern "C" int bqc_duplicate_sets(bqc_ctx* c, bqc_dup_view* out)
{
    if (!c || !out) return BQC_ERR_ARG;
    if (!c->d_dup) return fail(c, BQC_ERR_STATE, "bqc_duplicate_sets: bqc_enable_duplicate_sets has not been called for the context");
    if (!c->finalised[MOD_DUP]) return fail(c, BQC_ERR_STATE, "bqc_duplicate_sets: nothing has been finalised");
    out->capacity = c->dup_tab.capacity;
    out->n_lanes = c->opt.n_lanes;
    for (uint32_t k = 0; k < 2; ++k) {
        out->sets[k] = c->dup_sets[k];
        out->largest[k] = c->h_dup_out[2 * BQC_DUP_BINS + k];
        out->hist[k] = c->h_dup_out.data() + (size_t)k * BQC_DUP_BINS;
    }
    out->estimated_library_size = c->dup_estimate;
    out->lanes = c->h_dup_sums.data();
    return 0;
}

extern "C" int bqc_overrepresented(bqc_ctx* c, bqc_ovr_view* out)
{
    if (!c || !out) return BQC_ERR_ARG;
    if (!c->d_ovr) return fail(c, BQC_ERR_STATE, "bqc_overrepresented: bqc_enable_overrepresented has not been called for the context");
    if (!c->finalised[MOD_OVR]) return fail(c, BQC_ERR_STATE, "bqc_overrepresented: nothing has been finalised");
    out->prefix_len = c->ovr_k;
    out->ppm = c->ovr_ppm;
    out->capacity = c->ovr_tab.capacity;
    out->n_lanes = c->opt.n_lanes;
    out->pad = 0;
    out->lanes = c->h_ovr_sums.data();
    for (uint32_t m = 0; m < 2; ++m) {
        out->distinct[m] = c->ovr_distinct[m];
        out->largest[m] = c->h_ovr_out[2 * BQC_DUP_BINS + m];
        out->hist[m] = c->h_ovr_out.data() + (size_t)m * BQC_DUP_BINS;
        out->threshold[m] = c->ovr_threshold[m];
        out->n_listed[m] = c->ovr_n_listed[m];
    }
    out->listed[0] = c->ovr_listed.data();
    out->listed[1] = c->ovr_listed.data() + c->ovr_n_listed[0];
    return 0;
}

extern "C" int bqc_window_depth(bqc_ctx* c, uint32_t lane, bqc_wdp_view* out)
{
    if (!c || !out) return BQC_ERR_ARG;
    if (!c->seg[SEG_WDP].d) return fail(c, BQC_ERR_STATE, "bqc_window_depth: bqc_enable_window_depth has not been called for the context");
    if (!c->finalised[SEG_WDP]) return fail(c, BQC_ERR_STATE, "bqc_window_depth: nothing has been finalised");
    if (lane >= c->opt.n_lanes) return fail(c, BQC_ERR_ARG, "bqc_window_depth: lane %u out of range", lane);
    const uint64_t* w = c->h_wdp.data() + (uint64_t)lane * c->wdp_tab.lane_words;
    out->window = c->wdp_tab.W;
    out->min_mapq = c->wdp_mq;
    out->n_windows = c->wdp_tab.NW;
    out->n_refs = c->opt.n_refs;
    out->woff = c->wdp_woff.data();
    out->ref_len = c->wdp_len.data();
    out->reads_examined = w[0];
    out->reads_low_mapq = w[1];
    out->bases_outside = w[2];
    out->reads = w + 4;
    out->bases = out->reads + c->wdp_tab.NW;
    out->bases_low = out->bases + c->wdp_tab.NW;
    out->contigs = c->h_wdp_contigs.data() + (size_t)lane * c->opt.n_refs * 3;
    out->hist = c->h_wdp_hist.data() + (size_t)lane * BQC_WDP_HIST_BINS;
    return 0;
}
