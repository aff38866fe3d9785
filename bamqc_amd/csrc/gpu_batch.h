// gpu_batch.h — the device-resident batch the readers on the card produce (gpu_bam.hip: BAM files, gpu_sam.hip: SAM text), and the tail of
// their next_batch, stated once: the batch's buffer [seq][qual][cigar][fixed columns][cov] from the pool, the coverage anchors on the
// card (include/bamqc.h: bqc_anchor_*) or the fixed columns to the host, and the status word of the decode kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <string>

#include "../../include/bamqc.h"
#include "../host/bam_io.h"

struct GbCols { // device copies of the fixed columns + per-record payload placement
    uint16_t* flag; uint8_t* mapq; uint8_t* lane; int32_t* rid; int32_t* pos; int32_t* tlen; int32_t* nm; int32_t* as; uint32_t* l_seq; uint16_t* n_cigar;
    uint32_t* rec_off; uint64_t* so; uint64_t* qo; uint64_t* co;
};
struct GbLanes { const uint8_t* blob; const uint32_t* off; const uint32_t* len; const uint32_t* index; uint32_t n, lane_count; };

template <typename T> struct DevBuf { // grows, never shrinks
    T* p = nullptr;
    size_t cap = 0;
    bool need(size_t n, bool exact = false)
    {
        if (cap >= n) return true;
        if (p) (void)hipFree(p);
        p = nullptr; cap = 0;
        const size_t c = exact ? n : n + n / 4 + 64;
        if (hipMalloc((void**)&p, c * sizeof(T)) != hipSuccess) { p = nullptr; return false; }
        cap = c;
        return true;
    }
    ~DevBuf() { if (p) (void)hipFree(p); }
};
template <typename T> struct PinBuf {
    T* p = nullptr;
    size_t cap = 0;
    bool need(size_t n)
    {
        if (cap >= n) return true;
        if (p) (void)hipHostFree(p);
        p = nullptr; cap = 0;
        const size_t c = n + n / 4 + 64;
        if (hipHostMalloc((void**)&p, c * sizeof(T), hipHostMallocDefault) != hipSuccess) { p = nullptr; return false; }
        cap = c;
        return true;
    }
    ~PinBuf() { if (p) (void)hipHostFree(p); }
};

// the pool of the batches' payload buffers (gpu_bam.hip): one for both readers
void gb_pool_fill(size_t bytes, int n);
void* gb_pool_take(size_t need, size_t& cap); // nullptr: larger than the pool's buffers, or none left
void gb_pool_give(void* p);                   // (HostBatch::dev_free of every batch of the readers)

struct GbBatch { // where a batch's columns lie in its device buffer
    GbCols C;
    uint8_t *seq, *qual, *cigar, *cov;
    size_t N;
    bqc_batch dv; // the device view
};

// The batch's own buffer on the device: [seq][qual][cigar] (512 spare bytes behind each: the kernels' vector loads), then the fixed
// columns [rid pos tlen nm as l_seq](4 B) [flag n_cigar](2 B) [mapq lane](1 B) and 8 bytes per read for the coverage anchors — a
// batch that is anchored on the card (bqc_anchor_*) is submitted from here without its columns ever visiting the host.  d_cols: the
// scratch columns of the payload kernels, [so qo co](8 B) [rec_off](4 B) per record; `slack`: records a batch may exceed max_reads by.
// nullptr, or what failed.
inline const char* gb_batch_layout(HostBatch& o, DevBuf<uint8_t>& d_cols, size_t N, size_t max_reads, size_t slack, uint64_t so, uint64_t qo, uint64_t co, GbBatch& L)
{
    const size_t Np = (N + 63) & ~(size_t)63, Np_cap = std::max(Np, (std::min<size_t>(max_reads, 1u << 22) + 63 + slack) & ~(size_t)63);
    if (!d_cols.need(Np_cap * (3 * 8 + 4) + 256)) return "out of device memory";
    const size_t o_seq = 512, o_qual = (o_seq + so + 512 + 255) & ~(size_t)255, o_cig = o_qual + ((qo + 512 + 255) & ~(size_t)255),
                 o_fix = (o_cig + 4 * co + 512 + 255) & ~(size_t)255, o_cov = o_fix + Np * (6 * 4 + 2 * 2 + 2), total = o_cov + 8 * Np + 256;
    if (o.dev_cap < total) {
        if (o.dev_mem) gb_pool_give(o.dev_mem);
        size_t cap = 0;
        o.dev_mem = gb_pool_take(total, cap);
        o.dev_cap = o.dev_mem ? cap : 0;
        if (!o.dev_mem) { // larger than the pool's buffers (or the pool is empty): its own allocation
            const size_t own = total + total / 8 + 4096;
            if (hipMalloc(&o.dev_mem, own) != hipSuccess) { o.dev_mem = nullptr; return "out of device memory"; }
            o.dev_cap = own;
        }
        o.dev_free = gb_pool_give;
    }
    uint8_t* pay = (uint8_t*)o.dev_mem;
    GbCols& C = L.C;
    uint8_t* q = d_cols.p;
    C.so = (uint64_t*)q; q += Np * 8; C.qo = (uint64_t*)q; q += Np * 8; C.co = (uint64_t*)q; q += Np * 8; C.rec_off = (uint32_t*)q;
    q = pay + o_fix;
    C.rid = (int32_t*)q; q += Np * 4; C.pos = (int32_t*)q; q += Np * 4; C.tlen = (int32_t*)q; q += Np * 4; C.nm = (int32_t*)q; q += Np * 4;
    C.as = (int32_t*)q; q += Np * 4; C.l_seq = (uint32_t*)q; q += Np * 4;
    C.flag = (uint16_t*)q; q += Np * 2; C.n_cigar = (uint16_t*)q; q += Np * 2;
    C.mapq = q; q += Np; C.lane = q;
    L.seq = pay + o_seq; L.qual = pay + o_qual; L.cigar = pay + o_cig; L.cov = pay + o_cov; L.N = N;
    bqc_batch& dv = L.dv;
    memset(&dv, 0, sizeof dv);
    dv.n_reads = (uint32_t)N; dv.flag = C.flag; dv.mapq = C.mapq; dv.lane = C.lane; dv.rid = C.rid; dv.pos = C.pos; dv.tlen = C.tlen; dv.nm = C.nm; dv.as = C.as;
    dv.l_seq = C.l_seq; dv.n_cigar = C.n_cigar; dv.seq = L.seq; dv.qual = L.qual; dv.cigar = (const uint32_t*)L.cigar;
    return nullptr;
}

// Behind the decode kernels on stream s: the anchors of the coverage statistic on the card (k_anchor.hip), when the program has handed
// its context over and the stream allows it — the fixed columns then stay here, and a summary comes back instead of 26 bytes per
// read — or the fixed columns to the host; then the kernels' status word (*h_status: page-locked).  When that word is set the batch is
// the host decoder's: its anchors are dropped, the host keeps the window state from this batch on, and `o` holds nothing yet.
// nullptr, or what failed.
inline const char* gb_batch_finish(HostBatch& o, const GbBatch& L, bqc_ctx* actx, bool& anchors_ok, uint64_t& n_anchored, hipStream_t s, hipEvent_t ev,
                                   const uint32_t* d_status, uint32_t* h_status, std::string& anchor_err)
{
    const GbCols& C = L.C;
    const size_t N = L.N;
    auto sync = [&] { return hipEventRecord(ev, s) == hipSuccess && hipEventSynchronize(ev) == hipSuccess; };
    bqc_anchored* ah = nullptr;
    if (actx && anchors_ok) {
        const int arc = bqc_anchor_enqueue(actx, &L.dv, L.cov, s, &ah);
        if (arc < 0) { anchor_err = bqc_anchor_error(actx); return anchor_err.c_str(); }
        if (arc > 0) { anchors_ok = false; ah = nullptr; } // (the host has kept the state so far, or the context is a resolved shard)
    }
    auto columns_to_host = [&]() -> hipError_t {
        o.flag.resize(N); o.mapq.resize(N); o.lane.resize(N); o.rid.resize(N); o.pos.resize(N); o.tlen.resize(N);
        o.nm.resize(N); o.as.resize(N); o.l_seq.resize(N); o.n_cigar.resize(N);
        hipError_t e = hipMemcpyAsync(o.flag.data(), C.flag, N * 2, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipMemcpyAsync(o.n_cigar.data(), C.n_cigar, N * 2, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipMemcpyAsync(o.mapq.data(), C.mapq, N, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipMemcpyAsync(o.lane.data(), C.lane, N, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipMemcpyAsync(o.rid.data(), C.rid, N * 4, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipMemcpyAsync(o.pos.data(), C.pos, N * 4, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipMemcpyAsync(o.tlen.data(), C.tlen, N * 4, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipMemcpyAsync(o.nm.data(), C.nm, N * 4, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipMemcpyAsync(o.as.data(), C.as, N * 4, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipMemcpyAsync(o.l_seq.data(), C.l_seq, N * 4, hipMemcpyDeviceToHost, s);
        return e;
    };
    hipError_t he = ah ? hipSuccess : columns_to_host();
    if (he == hipSuccess) he = hipMemcpyAsync(h_status, d_status, 4, hipMemcpyDeviceToHost, s);
    if (he != hipSuccess || !sync()) return "decode failed";
    if (ah) {
        bqc_anchor_info info{};
        // a batch the host decoder takes, or one with more breaks than the card's chain walks: the host keeps the window
        // state from this batch on (it is current there: every anchored batch before this one is submitted before it)
        const int arc = *h_status ? 1 : bqc_anchor_complete(actx, ah, &info);
        if (*h_status) bqc_anchor_discard(actx, ah);
        if (arc < 0) { anchor_err = bqc_anchor_error(actx); return anchor_err.c_str(); }
        if (arc > 0) {
            anchors_ok = false; ah = nullptr;
            if (!*h_status && (columns_to_host() != hipSuccess || !sync())) return "decode failed";
        } else { o.anchored = ah; o.dev = L.dv; o.n_noqual = info.n_noqual; o.rid_min = info.rid_min; o.rid_max = info.rid_max; ++n_anchored; }
    }
    if (!*h_status) { o.d_seq = L.seq; o.d_qual = L.qual; o.d_cigar = (const uint32_t*)L.cigar; }
    return nullptr;
}
