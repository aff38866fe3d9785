// gpu_sam.hip — SAM text decoded on the GPU (row N4 of the scope table: see gpu_sam.h).
//
//   stream --read(), one thread--> ring of page-locked chunks --H2D--> the text, in a device window
//        --> k_gs_lines: where the lines and their first 11 fields are   --> k_gs_decode: the fixed columns
//        --> k_gs_payload: bases / qualities / CIGARs into packed columns (device)   --> the batch's tail (gpu_batch.h)
//
// The window is cut into 16 KiB segments; a line belongs to the segment in which it starts (nothing to guess: a line starts behind a
// '\n'), and whole segments are taken while the batch has room, as the reader of BAM files does from its record walk.  The card
// decodes the forms listed in DESIGN section 4.5b; a line of any other form sets the batch's exception word, and THAT batch is parsed
// by the host's line parser (host/bam_io.h: SamLineParser) from the window's bytes — it alone words the errors — and the run goes on
// from the card with the next batch.  A stream cannot be started over, so there is no hand-over of the whole input.
//
// A second source: SAM text inside BGZF.  The text then arrives ON the card — the runs of the BGZF producer of gpu_bam.hip
// (GpuBamReader::open_runs / next_run) — and the window is pointed at a run's inflated bytes instead of a buffer of its own; a run's
// unfinished last line goes in front of the next run's bytes (the producer's copy, as for a BAM record).  Everything from k_gs_lines
// on is the one code path of both sources.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <errno.h>
#include <poll.h>
#include <unistd.h>

#include <algorithm>
#include <chrono>
#include <condition_variable>
#include <mutex>
#include <thread>

#include "../../include/bamqc.h"
#include "gpu_sam.h"
#include "gpu_batch.h"

hipStream_t bqc_pool_stream(int device, int rank); // bqc_api.cpp

#define GS_SEG 16384u
#define GS_MAXR (GS_SEG / 22u + 2u) // (a line of 11 fields is 21 bytes and its '\n')
#define GS_SLACK 512u               // bytes in front of and behind the text on the card: 16-byte loads may over-read

enum { GS_INCOMPLETE = 1, GS_EXCEPTION = 2 };

struct GsSeg { uint32_t exit, count, flags, seq_bytes, qual_bytes, cigar_words, pad0, pad1; }; // exit: behind the last line that starts here (0: none does)
struct GsLine { uint32_t start, end, ntabs, n_cig, l_seq, fe[11]; };                           // offsets into the window; fe[k]: the end of field k
struct GsPre { uint32_t so, qo, co, pad; };                                                    // payload prefix inside the segment
struct GsBase { uint64_t so, qo, co; uint32_t rec, take; };
struct GsPay { uint32_t seq_at, qual_at, cig_at, cig_len; };                                   // qual_at 0xFFFFFFFF: no qualities
struct GsNames { const uint8_t* blob; const uint32_t* off; const uint32_t* len; const int32_t* rid; uint32_t n; };

typedef uint32_t __attribute__((aligned(1))) gs_u32_u;
typedef uint64_t __attribute__((aligned(1))) gs_u64_u;
typedef uint32_t gs_u32x4 __attribute__((ext_vector_type(4)));
typedef gs_u32x4 __attribute__((aligned(1))) gs_u32x4_u;

namespace {
__device__ __forceinline__ uint64_t gs_below(uint32_t lane) { return lane ? (~0ull >> (64u - lane)) : 0ull; }   // bits of the lanes below
__device__ __forceinline__ uint64_t gs_from(uint32_t lane) { return lane >= 64u ? 0ull : (~0ull << lane); }       // bits of this lane and above
__device__ __forceinline__ uint32_t gs_msb(uint64_t m) { return 63u - (uint32_t)__clzll((long long)m); }
} // namespace

// A wave per segment.  The segment comes into LDS with one round of 16-byte loads; then 64 bytes at a time, a byte per lane: the
// newline and tab bytes are two ballots, and every lane knows from the two masks which line it is in, whether that line is a record
// of this segment, and how many tabs lie between the line's start and itself — so the lane that holds the k-th tab of a record line
// writes fe[k], and the lane that holds its '\n' the line's end: no loop over a line's bytes.  The last line is followed past the
// segment's end, from memory.  A second pass (a lane per record) turns field ends into l_seq / n_cigar and the payload prefix.
__global__ __launch_bounds__(64) void k_gs_lines(const uint8_t* __restrict__ base, uint32_t avail, uint32_t tail_ok, GsSeg* __restrict__ segs, GsLine* __restrict__ lines,
                                                  GsPre* __restrict__ pres)
{
    __shared__ uint32_t buf[GS_SEG / 4 + 4];
    const uint32_t s = blockIdx.x, lane = threadIdx.x;
    const uint32_t a = s * GS_SEG, b = min(avail, a + GS_SEG);
    const uint32_t staged = (b - a) & ~3u;
    {
        constexpr uint32_t kSteps = GS_SEG / 1024u;
        gs_u32x4 v[kSteps];
#pragma unroll
        for (uint32_t k = 0; k < kSteps; ++k) {
            const uint32_t off = lane * 16u + 1024u * k;
            v[k] = gs_u32x4{0, 0, 0, 0};
            if (off + 16u <= staged) v[k] = *(const gs_u32x4_u*)(base + a + off);
        }
#pragma unroll
        for (uint32_t k = 0; k < kSteps; ++k) {
            const uint32_t off = lane * 16u + 1024u * k;
            if (off + 16u <= staged) { buf[off / 4] = v[k].x; buf[off / 4 + 1] = v[k].y; buf[off / 4 + 2] = v[k].z; buf[off / 4 + 3] = v[k].w; }
            else if (off < staged) for (uint32_t q = off; q < staged; q += 4u) buf[q / 4] = *(const gs_u32_u*)(base + a + q);
        }
    }
    __syncthreads();
    auto getb = [&](uint32_t p) -> uint32_t { return p - a < staged ? (buf[(p - a) >> 2] >> (8u * (p & 3u))) & 255u : (uint32_t)base[p]; }; // (a is a multiple of 4)
    GsLine* const L = lines + (size_t)s * GS_MAXR;
    uint32_t flags = 0, exit = 0, nrec = 0;
    // the line that is open at the window's first byte: its start (none: 0xFFFFFFFF), whether it is a record line, its tabs and CIGAR letters so far
    uint32_t line_start = 0xFFFFFFFFu, tab_carry = 0, ops_carry = 0;
    bool open_rec = false;
    uint32_t last_c = a ? (uint32_t)base[a - 1] : (uint32_t)'\n';
    uint32_t w = a;
    for (; w < avail; w += 64u) {
        if (last_c == '\n') { // a line starts at this window's first byte (uniform): one of this segment's only in front of its end
            line_start = 0xFFFFFFFFu; open_rec = false; tab_carry = ops_carry = 0;
            if (w < b) {
                const uint32_t c0 = getb(w), c1 = w + 1 < avail ? getb(w + 1) : 255u;
                line_start = w;
                open_rec = !(c0 == '\n' || (c0 == '\r' && c1 == '\n') || c0 == '@');
                nrec += open_rec ? 1u : 0u;
            }
        }
        if (line_start == 0xFFFFFFFFu && w >= b) break;
        const uint32_t p = w + lane;
        const bool in = p < avail;
        const uint32_t c = in ? getb(p) : 255u;
        uint32_t prevc = (uint32_t)__shfl_up((int)c, 1);
        if (lane == 0) prevc = last_c;
        const bool is_nl = in && c == '\n', is_tab = in && c == '\t';
        const bool is_start = lane != 0 && in && prevc == '\n' && p < b;
        bool start_rec = false;
        if (is_start) {
            const uint32_t c1 = p + 1 < avail ? getb(p + 1) : 255u;
            start_rec = !(c == '\n' || (c == '\r' && c1 == '\n') || c == '@');
        }
        const uint64_t nlm = __ballot(is_nl), tbm = __ballot(is_tab), startm = __ballot(is_start), recm = __ballot(start_rec);
        const uint64_t below = gs_below(lane), nl_before = nlm & below;
        const bool has_nl = nl_before != 0;
        const uint32_t Ls = has_nl ? gs_msb(nl_before) + 1u : 0u; // the lane at which my line starts (when it starts in this window)
        const bool owned = has_nl ? ((startm >> Ls) & 1u) != 0 : line_start != 0xFFFFFFFFu;
        const bool rec_line = has_nl ? ((recm >> Ls) & 1u) != 0 : open_rec;
        const uint32_t idx = (has_nl ? nrec + (uint32_t)__popcll(recm & ~gs_from(Ls + 1u)) : nrec) - 1u;
        const uint32_t tabs = has_nl ? (uint32_t)__popcll(tbm & below & gs_from(Ls)) : tab_carry + (uint32_t)__popcll(tbm & below);
        const bool digit = c - '0' < 10u;
        const uint64_t opm = __ballot(in && rec_line && tabs == 5u && !is_tab && !is_nl && !digit);
        const bool live = rec_line && idx < GS_MAXR;
        if (in && owned && c == 0) flags |= GS_EXCEPTION; // (a NUL byte: DESIGN section 2)
        if (is_tab && live) {
            if (tabs < 11u) L[idx].fe[tabs] = p;
            if (tabs == 5u) L[idx].n_cig = (has_nl ? 0u : ops_carry) + (uint32_t)__popcll(opm & below & (has_nl ? gs_from(Ls) : ~0ull));
        }
        if (is_nl && live) {
            const uint32_t e = p - (prevc == '\r' && p > (has_nl ? w + Ls : line_start) ? 1u : 0u);
            L[idx].start = has_nl ? w + Ls : line_start;
            L[idx].end = e;
            L[idx].ntabs = tabs;
            if (tabs == 10u) L[idx].fe[10] = e;
            if (tabs < 10u) flags |= GS_EXCEPTION; // fewer than 11 fields
        }
        const uint64_t donem = __ballot(is_nl && owned);
        if (donem) exit = w + gs_msb(donem) + 1u;
        // the line that is open behind this window
        nrec += (uint32_t)__popcll(recm);
        if (nlm) {
            const uint32_t Lx = gs_msb(nlm) + 1u;
            if (Lx < 64u) {
                const bool st = ((startm >> Lx) & 1u) != 0;
                line_start = st ? w + Lx : 0xFFFFFFFFu;
                open_rec = ((recm >> Lx) & 1u) != 0;
                tab_carry = (uint32_t)__popcll(tbm & gs_from(Lx));
                ops_carry = (uint32_t)__popcll(opm & gs_from(Lx));
            } else { line_start = 0xFFFFFFFFu; open_rec = false; }
        } else { tab_carry += (uint32_t)__popcll(tbm); ops_carry += (uint32_t)__popcll(opm); }
        last_c = (uint32_t)__shfl((int)c, 63);
    }
    flags = __ballot(flags != 0) ? GS_EXCEPTION : 0u;
    if (line_start != 0xFFFFFFFFu && w >= avail && last_c != '\n') { // the data at hand ends inside a line of this segment
        if (tail_ok) { // the stream's last line, without its '\n' (no '\r' is stripped from it, as on the host)
            if (open_rec && nrec - 1u < GS_MAXR && lane == 0) {
                GsLine& X = L[nrec - 1u];
                X.start = line_start; X.end = avail; X.ntabs = tab_carry;
                if (tab_carry == 10u) X.fe[10] = avail;
            }
            if (open_rec && tab_carry < 10u) flags |= GS_EXCEPTION;
            exit = avail;
        } else {
            if (open_rec) --nrec;
            flags |= GS_INCOMPLETE;
            exit = line_start;
        }
    }
    if (nrec > GS_MAXR) { nrec = GS_MAXR; flags |= GS_EXCEPTION; } // (more short lines than a segment of records can hold: none of them is a record)
    __threadfence_block();
    __syncthreads();
    // a lane per record: l_seq, n_cigar, and where its payload goes inside the segment
    uint32_t so = 0, qo = 0, co = 0;
    for (uint32_t r0 = 0; r0 < nrec; r0 += 64u) {
        const uint32_t r = r0 + lane;
        uint32_t ls = 0, nc = 0;
        if (r < nrec && L[r].ntabs >= 10u) {
            const uint32_t f4 = L[r].fe[4], f5 = L[r].fe[5], f8 = L[r].fe[8], f9 = L[r].fe[9], f10 = L[r].fe[10];
            const uint32_t slen = f9 - f8 - 1u, qlen = f10 - f9 - 1u, clen = f5 - f4 - 1u;
            ls = slen == 1u && base[f8 + 1u] == '*' ? 0u : slen;
            const bool qstar = qlen == 1u && base[f9 + 1u] == '*';
            nc = clen == 1u && base[f4 + 1u] == '*' ? 0u : L[r].n_cig;
            if ((!qstar && qlen != ls) || nc > 65535u) { flags |= GS_EXCEPTION; nc = min(nc, 65535u); }
            L[r].l_seq = ls; L[r].n_cig = nc;
        } else if (r < nrec) { L[r].l_seq = 0; L[r].n_cig = 0; }
        uint32_t xs = (ls + 1u) / 2u, xq = ls, xc = nc; // inclusive scans over the wave
#pragma unroll
        for (uint32_t d = 1; d < 64u; d <<= 1) {
            const uint32_t ys = (uint32_t)__shfl_up((int)xs, d), yq = (uint32_t)__shfl_up((int)xq, d), yc = (uint32_t)__shfl_up((int)xc, d);
            if (lane >= d) { xs += ys; xq += yq; xc += yc; }
        }
        if (r < nrec) pres[(size_t)s * GS_MAXR + r] = GsPre{so + xs - (ls + 1u) / 2u, qo + xq - ls, co + xc - nc, 0};
        so += (uint32_t)__shfl((int)xs, 63); qo += (uint32_t)__shfl((int)xq, 63); co += (uint32_t)__shfl((int)xc, 63);
    }
    flags = (flags & GS_INCOMPLETE) | (__ballot((flags & GS_EXCEPTION) != 0) ? GS_EXCEPTION : 0u);
    if (lane == 0) segs[s] = GsSeg{exit, nrec, flags, so, qo, co, 0, 0};
}

// workgroup per taken segment, thread per record: the fixed columns from the text, by the rules of DESIGN section 4.5b — each equals the
// host parser's on the forms it lists, anything else sets the exception word.  The fields FLAG .. TLEN and the first optional fields
// are walked byte by byte; their first GSD_STAGE bytes come into LDS with 16-byte loads issued together (as k_gb_decode's).
#define GSD_STAGE 64u
namespace {
struct GsdBytes { // a byte source over the window: two staged stretches from LDS, the rest from memory
    const uint32_t *fb, *tb;
    uint32_t f0, t0;
    const uint8_t* base;
    __device__ __forceinline__ uint32_t u8(uint32_t p) const
    {
        if (p - f0 < GSD_STAGE) return (fb[(p - f0) >> 2] >> (8u * ((p - f0) & 3u))) & 255u;
        if (p - t0 < GSD_STAGE) return (tb[(p - t0) >> 2] >> (8u * ((p - t0) & 3u))) & 255u;
        return base[p];
    }
};
// -?[0-9]{1,10} in [lo, hi): the value in 64 bits; anything else: ok = false
__device__ __forceinline__ int64_t gs_number(const GsdBytes& B, uint32_t lo, uint32_t hi, bool sign, bool& ok)
{
    bool neg = false;
    if (sign && lo < hi && B.u8(lo) == '-') { neg = true; ++lo; }
    const uint32_t n = hi - lo;
    if (n < 1u || n > 10u) { ok = false; return 0; }
    int64_t v = 0;
    for (uint32_t k = lo; k < hi; ++k) {
        const uint32_t d = B.u8(k) - '0';
        if (d > 9u) ok = false;
        v = v * 10 + (int64_t)d;
    }
    return neg ? -v : v;
}
// a reference name -> its id: binary search in the table sorted as the host's map (bytes, then length); "*" and unknown names: -1
__device__ int32_t gs_ref(const GsdBytes& B, uint32_t lo, uint32_t hi, const GsNames& T)
{
    const uint32_t n = hi - lo;
    if (n == 1u && B.u8(lo) == '*') return -1;
    uint32_t x = 0, y = T.n;
    while (x < y) {
        const uint32_t m = (x + y) >> 1;
        const uint8_t* nm = T.blob + T.off[m];
        const uint32_t ln = T.len[m], k_end = min(ln, n);
        int cmp = 0;
        for (uint32_t k = 0; k < k_end && !cmp; ++k) { const uint32_t q = B.u8(lo + k), t = nm[k]; cmp = q < t ? -1 : q > t ? 1 : 0; }
        if (!cmp) cmp = n < ln ? -1 : n > ln ? 1 : 0;
        if (!cmp) return T.rid[m];
        if (cmp < 0) y = m; else x = m + 1u;
    }
    return -1;
}
} // namespace

__global__ __launch_bounds__(64) void k_gs_decode(const uint8_t* __restrict__ base, const GsSeg* __restrict__ segs, const GsLine* __restrict__ lines, const GsPre* __restrict__ pres,
                                                   const GsBase* __restrict__ bases, GbCols C, GsPay* __restrict__ pays, GbLanes LN, GsNames RN, const uint8_t* __restrict__ main_chrom,
                                                   uint32_t n_main, uint32_t* __restrict__ status)
{
    __shared__ uint32_t fbuf[64][GSD_STAGE / 4 + 1], tbuf[64][GSD_STAGE / 4 + 1]; // (an odd stride: the lanes' words in different banks)
    const uint32_t s = blockIdx.x;
    const GsBase B = bases[s];
    if (!B.take) return;
    const uint32_t count = segs[s].count;
    uint32_t exc = 0;
    for (uint32_t slot = threadIdx.x; slot < count; slot += 64) {
        const GsLine Ln = lines[(size_t)s * GS_MAXR + slot];
        const GsPre P = pres[(size_t)s * GS_MAXR + slot];
        const uint32_t i = B.rec + slot;
        // (a line of fewer than 11 fields never gets here: k_gs_lines has marked its segment, and next_batch launches nothing for a marked batch)
        const uint32_t* fe = Ln.fe;
        const uint32_t f0 = fe[0] + 1u, t0 = fe[10] + 1u;
        uint32_t* const fb = fbuf[threadIdx.x];
        uint32_t* const tb = tbuf[threadIdx.x];
        {
            gs_u32x4 vf[GSD_STAGE / 16], vt[GSD_STAGE / 16];
#pragma unroll
            for (uint32_t k = 0; k < GSD_STAGE / 16; ++k) vf[k] = f0 + 16u * k < Ln.end ? *(const gs_u32x4_u*)(base + f0 + 16u * k) : gs_u32x4{0, 0, 0, 0};
#pragma unroll
            for (uint32_t k = 0; k < GSD_STAGE / 16; ++k) vt[k] = t0 + 16u * k < Ln.end ? *(const gs_u32x4_u*)(base + t0 + 16u * k) : gs_u32x4{0, 0, 0, 0};
#pragma unroll
            for (uint32_t k = 0; k < GSD_STAGE / 16; ++k) { fb[4 * k] = vf[k].x; fb[4 * k + 1] = vf[k].y; fb[4 * k + 2] = vf[k].z; fb[4 * k + 3] = vf[k].w; }
#pragma unroll
            for (uint32_t k = 0; k < GSD_STAGE / 16; ++k) { tb[4 * k] = vt[k].x; tb[4 * k + 1] = vt[k].y; tb[4 * k + 2] = vt[k].z; tb[4 * k + 3] = vt[k].w; }
        }
        const GsdBytes T{fb, tb, f0, t0, base};
        bool ok = true;
        const uint32_t flag = (uint32_t)gs_number(T, fe[0] + 1u, fe[1], false, ok) & 0x0FFFu;
        const int32_t rid = gs_ref(T, fe[1] + 1u, fe[2], RN);
        const int32_t pos = (int32_t)((uint32_t)gs_number(T, fe[2] + 1u, fe[3], true, ok) - 1u);
        const uint32_t mapq = (uint32_t)gs_number(T, fe[3] + 1u, fe[4], false, ok) & 255u;
        const int32_t rnext = fe[6] - fe[5] == 2u && T.u8(fe[5] + 1u) == '=' ? rid : gs_ref(T, fe[5] + 1u, fe[6], RN);
        const int32_t tlen = (int32_t)(uint32_t)gs_number(T, fe[7] + 1u, fe[8], true, ok);
        const bool qstar = fe[10] - fe[9] == 2u && base[fe[9] + 1u] == '*';
        // the optional fields: RG -> lane, NM:i, the first AS
        int lane = -1;
        bool rg_seen = false, nm_seen = false, as_seen = false;
        int32_t nm = BQC_NM_ABSENT, as = BQC_AS_ABSENT;
        for (uint32_t p = fe[10]; p < Ln.end;) {
            const uint32_t fs = p + 1u;
            uint32_t fz = fs;
            while (fz < Ln.end && T.u8(fz) != '\t') ++fz;
            p = fz;
            if (fz - fs < 5u || T.u8(fs + 2u) != ':' || T.u8(fs + 4u) != ':') continue;
            const uint32_t k0 = T.u8(fs), k1 = T.u8(fs + 1u), ty = T.u8(fs + 3u), v = fs + 5u, vl = fz - v;
            if (k0 == 'R' && k1 == 'G' && !rg_seen) {
                rg_seen = true;
                if (ty != 'Z') { ok = false; continue; }
                for (uint32_t l = 0; l < LN.n && lane < 0; ++l) {
                    if (LN.len[l] != vl) continue;
                    const uint8_t* id = LN.blob + LN.off[l];
                    uint32_t k = 0;
                    while (k < vl && id[k] == T.u8(v + k)) ++k;
                    if (k == vl) lane = (int)LN.index[l];
                }
                if (lane < 0 || (uint32_t)lane >= LN.lane_count) { ok = false; lane = 0; }
            } else if (k0 == 'N' && k1 == 'M' && ty == 'i') {
                const uint32_t x = (uint32_t)gs_number(T, v, fz, true, ok);
                if (nm_seen || x == 0xFFFFFFFFu) ok = false;
                nm = (int32_t)x; nm_seen = true;
            } else if (k0 == 'A' && k1 == 'S' && !as_seen) {
                as_seen = true;
                if (ty == 'i') as = (int32_t)(uint32_t)gs_number(T, v, fz, true, ok);
                else if (ty == 'A') { const uint32_t ch = vl ? T.u8(v) : 255u; if (ch < 128u) as = (int32_t)ch; else ok = false; }
                else if (ty == 'f') ok = false;
            }
        }
        if (!rg_seen) ok = false;
        if (!ok) exc |= 1u;
        uint32_t fl = flag;
        if (rnext >= 0 && (uint32_t)rnext < n_main && main_chrom[rnext]) fl |= BQC_FLAG_MATE_MAIN;
        if (Ln.l_seq > 0 && qstar) fl |= BQC_FLAG_NO_QUAL;
        C.flag[i] = (uint16_t)fl; C.mapq[i] = (uint8_t)mapq; C.lane[i] = (uint8_t)(lane < 0 ? 0 : lane); C.rid[i] = rid; C.pos[i] = pos;
        C.tlen[i] = tlen; C.nm[i] = nm; C.as[i] = as; C.l_seq[i] = Ln.l_seq; C.n_cigar[i] = (uint16_t)Ln.n_cig;
        C.so[i] = B.so + P.so; C.qo[i] = B.qo + P.qo; C.co[i] = B.co + P.co;
        const uint32_t clen = fe[5] - fe[4] - 1u;
        const bool cstar = clen == 1u && T.u8(fe[4] + 1u) == '*';
        pays[i] = GsPay{fe[8] + 1u, qstar ? 0xFFFFFFFFu : fe[9] + 1u, fe[4] + 1u, cstar ? 0u : clen}; // (a field without a letter is looked at too: it is none the host takes)
    }
    if (exc) atomicOr(status, exc);
}

// Bases, qualities and CIGARs of the text into the batch's packed columns: 16 lanes per record, 16 characters per lane and step (long
// reads: the 16 lanes stride).  Qualities: minus 33 in every byte (SWAR), or 0xFF.  Bases: two characters -> a byte of 4-bit codes
// through the 256-entry table (LDS).  A last piece shorter than a step is done as the array's last full step (it overlaps the piece
// before it: the same bytes twice); an array shorter than one step byte by byte.  CIGAR: every lane looks at 16 characters of the
// field; a letter ends an operation, its index is the number of letters in front of it (a count over the 16 lanes), its count the <= 9
// digits in front of it, which the lane reads from the 16 characters before its own — no walk over the field.  The field must end in a letter.
namespace {
__device__ __forceinline__ uint64_t gs_sub33(uint64_t x) // every byte minus 33, modulo 256
{
    const uint64_t H = 0x8080808080808080ull, y = 0x2121212121212121ull;
    return ((x | H) - y) ^ ((x ^ ~y) & H);
}
__device__ __forceinline__ uint32_t gs_byte(uint64_t a0, uint64_t a1, uint64_t a2, uint64_t a3, uint32_t k) // byte k of 32
{
    const uint64_t wd = k < 16u ? (k < 8u ? a0 : a1) : (k < 24u ? a2 : a3);
    return (uint32_t)(wd >> (8u * (k & 7u))) & 255u;
}
__device__ __forceinline__ uint64_t gs_pack16(uint64_t lo, uint64_t hi, const uint8_t* lut, uint32_t n_valid) // 16 characters -> 8 bytes of codes
{
    uint64_t out = 0;
#pragma unroll
    for (uint32_t t = 0; t < 8u; ++t) {
        const uint64_t src = t < 4u ? lo : hi;
        const uint32_t c0 = (uint32_t)(src >> (16u * (t & 3u))) & 255u, c1 = (uint32_t)(src >> (16u * (t & 3u) + 8u)) & 255u;
        const uint32_t n0 = 2u * t < n_valid ? lut[c0] : 0u, n1 = 2u * t + 1u < n_valid ? lut[c1] : 0u;
        out |= (uint64_t)((n0 << 4) | n1) << (8u * t);
    }
    return out;
}
} // namespace

__global__ __launch_bounds__(256) void k_gs_payload(const uint8_t* __restrict__ base, GbCols C, const GsPay* __restrict__ pays, uint32_t n, const uint8_t* __restrict__ lut_g,
                                                     uint8_t* __restrict__ seq, uint8_t* __restrict__ qual, uint32_t* __restrict__ cigar, uint32_t* __restrict__ status)
{
    __shared__ uint8_t lut[256];
    lut[threadIdx.x] = lut_g[threadIdx.x];
    __syncthreads();
    const uint32_t i = blockIdx.x * 16 + (threadIdx.x >> 4), gl = threadIdx.x & 15u;
    if (i >= n) return;
    const GsPay P = pays[i];
    const uint32_t l_seq = C.l_seq[i];
    uint8_t* const ds = seq + C.so[i];
    uint8_t* const dq = qual + C.qo[i];
    uint32_t* const dc = cigar + C.co[i];
    // qualities
    const uint32_t nq = l_seq, pq = (nq + 15u) >> 4;
    for (uint32_t k = gl; k < pq; k += 16u) {
        if (nq >= 16u) {
            const uint32_t at = min(16u * k, nq - 16u);
            uint64_t lo = ~0ull, hi = ~0ull;
            if (P.qual_at != 0xFFFFFFFFu) { lo = gs_sub33(*(const gs_u64_u*)(base + P.qual_at + at)); hi = gs_sub33(*(const gs_u64_u*)(base + P.qual_at + at + 8u)); }
            *(gs_u64_u*)(dq + at) = lo; *(gs_u64_u*)(dq + at + 8u) = hi;
        } else for (uint32_t b_ = 0; b_ < nq; ++b_) dq[b_] = P.qual_at != 0xFFFFFFFFu ? (uint8_t)(base[P.qual_at + b_] - 33u) : (uint8_t)0xFF;
    }
    // bases
    const uint32_t ns = (l_seq + 1u) / 2u, ps = (ns + 7u) >> 3;
    for (uint32_t k = gl; k < ps; k += 16u) {
        const uint32_t at = ns >= 8u ? min(8u * k, ns - 8u) : 0u; // (in bytes of codes: two characters each)
        const uint64_t lo = *(const gs_u64_u*)(base + P.seq_at + 2u * at), hi = *(const gs_u64_u*)(base + P.seq_at + 2u * at + 8u);
        const uint64_t out = gs_pack16(lo, hi, lut, l_seq - 2u * at);
        if (ns >= 8u) *(gs_u64_u*)(ds + at) = out;
        else for (uint32_t b_ = 0; b_ < ns; ++b_) ds[b_] = (uint8_t)(out >> (8u * b_));
    }
    // CIGAR (every lane of the record's 16 takes part in every round: the counts go from lane to lane)
    uint32_t exc = 0, opbase = 0;
    if (gl == 0 && P.cig_len && base[P.cig_at + P.cig_len - 1u] - '0' < 10u) exc = 1u; // digits behind the last letter (or nothing but digits): no operation ends them
    for (uint32_t c0 = 0; c0 < P.cig_len; c0 += 256u) {
        const uint32_t mine = c0 + 16u * gl;
        uint64_t a0 = 0, a1 = 0, a2 = 0, a3 = 0; // the 16 characters in front of mine, and mine
        if (mine < P.cig_len) {
            const uint8_t* q = base + P.cig_at + mine;
            a0 = *(const gs_u64_u*)(q - 16); a1 = *(const gs_u64_u*)(q - 8); a2 = *(const gs_u64_u*)q; a3 = *(const gs_u64_u*)(q + 8);
        }
        uint32_t m = 0; // my letters
        for (uint32_t j = 0; j < 16u; ++j) {
            const uint32_t ch = gs_byte(a0, a1, a2, a3, 16u + j);
            if (mine + j < P.cig_len && ch - '0' >= 10u) m |= 1u << j;
        }
        uint32_t incl = (uint32_t)__popc(m);
        const uint32_t cnt = incl;
#pragma unroll
        for (uint32_t d = 1; d < 16u; d <<= 1) { const uint32_t y = (uint32_t)__shfl_up((int)incl, d, 16); if (gl >= d) incl += y; }
        uint32_t at = opbase + incl - cnt;
        opbase += (uint32_t)__shfl((int)incl, 15, 16);
        while (m) {
            const uint32_t j = (uint32_t)__ffs((int)m) - 1u;
            m &= m - 1u;
            const uint32_t ch = gs_byte(a0, a1, a2, a3, 16u + j);
            const uint32_t op = ch == 'M' ? 0u : ch == 'I' ? 1u : ch == 'D' ? 2u : ch == 'N' ? 3u : ch == 'S' ? 4u : ch == 'H' ? 5u : ch == 'P' ? 6u : ch == '=' ? 7u : ch == 'X' ? 8u : 15u;
            uint32_t val = 0, mul = 1, nd = 0;
            for (uint32_t k = 1; k <= 10u && k <= mine + j; ++k) { // (k <= mine + j: not in front of the field)
                const uint32_t d = gs_byte(a0, a1, a2, a3, 16u + j - k) - '0';
                if (d > 9u) break;
                if (k == 10u) { nd = 10u; break; }
                val += d * mul; mul *= 10u; ++nd;
            }
            if (op == 15u || nd == 0u || nd > 9u || val >= (1u << 28)) exc = 1u;
            dc[at++] = (val << 4) | (op & 15u);
        }
    }
    if (exc) atomicOr(status, exc);
}

// ---------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------
namespace {
double gs_now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
} // namespace

struct GpuSamReader::Impl {
    int device = 0, fd = -1;
    hipStream_t s = nullptr;
    hipEvent_t ev = nullptr;
    // the ring: one thread read()s the stream into page-locked chunks, next_batch copies them to the card in order
    struct Slot { uint8_t* p = nullptr; size_t len = 0; };
    static const int kSlots = 4;
    Slot slots[kSlots];
    size_t chunk_bytes = 8u << 20; // (BQC_GS_CHUNK_KB: tests)
    std::thread reader;
    std::mutex m;
    std::condition_variable cv;
    uint64_t filled = 0, released = 0; // chunk k lives in slots[k % kSlots]
    bool eof = false, stop = false, io_error = false;
    double t_read = 0;
    bool kernels_ok = false;
    // the window: text[cur, end) of the current buffer (GS_SLACK spare bytes in front and behind); the other buffer takes what is left
    // when the current one is full
    DevBuf<uint8_t> d_win[2];
    int wi = 0;
    size_t cur = GS_SLACK, end = GS_SLACK;
    bool all_in = false; // the stream's last byte is in the window
    // the second source: the window is [cur, end) of bg_win, a run of inflated text in the producer's buffer (its spare bytes around it)
    GpuBamReader* bg = nullptr;
    const uint8_t* bg_win = nullptr;
    bool need_run = false; // the window holds no whole line: the next run's bytes behind it
    bool own_stream = true; // (false: the producer's consumer stream)
    uint32_t *d_status = nullptr, *h_status = nullptr;
    DevBuf<GsSeg> d_seg; PinBuf<GsSeg> h_seg;
    DevBuf<GsLine> d_line; DevBuf<GsPre> d_pre; DevBuf<GsPay> d_pay;
    DevBuf<GsBase> d_base; PinBuf<GsBase> h_base;
    DevBuf<uint8_t> d_cols;
    DevBuf<uint8_t> d_lane_blob; DevBuf<uint32_t> d_lane_tab; uint32_t n_lane_ids = 0, lane_count = 0;
    DevBuf<uint8_t> d_name_blob; DevBuf<uint32_t> d_name_tab; uint32_t n_names = 0;
    DevBuf<uint8_t> d_main; uint32_t n_main = 0; bool main_set = false;
    DevBuf<uint8_t> d_lut;
    double avg_line_bytes = 0, avg_line_bases = 0;
    uint64_t grow = 0;
    std::vector<char> handover;
    bool timing = false;

    ~Impl()
    {
        { std::lock_guard<std::mutex> lk(m); stop = true; }
        cv.notify_all();
        if (reader.joinable()) reader.join(); // (it looks at `stop` between two waits for input)
        (void)hipSetDevice(device);
        if (s) { (void)hipStreamSynchronize(s); if (own_stream) (void)hipStreamDestroy(s); }
        if (ev) (void)hipEventDestroy(ev);
        for (Slot& C : slots) if (C.p) (void)hipHostFree(C.p);
        if (d_status) (void)hipFree(d_status);
        if (h_status) (void)hipHostFree(h_status);
    }
    bool sync() { return hipEventRecord(ev, s) == hipSuccess && hipEventSynchronize(ev) == hipSuccess; }
    uint8_t* win() { return bg ? const_cast<uint8_t*>(bg_win) : d_win[wi].p; }
    void read_loop()
    {
        for (;;) {
            Slot* C;
            {
                std::unique_lock<std::mutex> lk(m);
                cv.wait(lk, [&] { return stop || filled - released < (uint64_t)kSlots; });
                if (stop) return;
                C = &slots[filled % kSlots];
            }
            size_t n = 0;
            bool end_ = false, bad = false;
            const double t0 = gs_now();
            while (n < chunk_bytes) {
                struct pollfd pf{fd, POLLIN, 0};
                if (poll(&pf, 1, 100) == 0) { // nothing yet (a pipe): is the reader still wanted?
                    std::lock_guard<std::mutex> lk(m);
                    if (stop) return;
                    continue;
                }
                const ssize_t r = ::read(fd, C->p + n, chunk_bytes - n);
                if (r < 0) { if (errno == EINTR) continue; bad = true; break; }
                if (r == 0) { end_ = true; break; }
                n += (size_t)r;
            }
            const double t1 = gs_now();
            {
                std::lock_guard<std::mutex> lk(m);
                C->len = n;
                ++filled;
                t_read += t1 - t0;
                if (end_ || bad) eof = true;
                if (bad) io_error = true;
            }
            cv.notify_all();
            if (end_ || bad) return;
        }
    }
    bool upload_lanes(const BamHeader& hdr)
    {
        std::vector<uint8_t> blob;
        n_lane_ids = (uint32_t)hdr.lane_names.size();
        lane_count = hdr.lane_count;
        std::vector<uint32_t> cols(3 * (size_t)n_lane_ids + 1);
        uint32_t l = 0;
        for (const auto& kv : hdr.lane_names) {
            cols[l] = (uint32_t)blob.size(); cols[n_lane_ids + l] = (uint32_t)kv.first.size(); cols[2 * n_lane_ids + l] = kv.second;
            blob.insert(blob.end(), kv.first.begin(), kv.first.end());
            ++l;
        }
        if (!d_lane_blob.need(blob.size() + 1) || !d_lane_tab.need(cols.size())) return false;
        if (!blob.empty() && hipMemcpy(d_lane_blob.p, blob.data(), blob.size(), hipMemcpyHostToDevice) != hipSuccess) return false;
        return hipMemcpy(d_lane_tab.p, cols.data(), cols.size() * 4, hipMemcpyHostToDevice) == hipSuccess;
    }
    bool upload_names(const std::map<std::string, int32_t>& ref_index) // in the map's order: the table the kernel searches
    {
        std::vector<uint8_t> blob;
        n_names = (uint32_t)ref_index.size();
        std::vector<uint32_t> cols(3 * (size_t)n_names + 1);
        uint32_t l = 0;
        for (const auto& kv : ref_index) {
            cols[l] = (uint32_t)blob.size(); cols[n_names + l] = (uint32_t)kv.first.size(); cols[2 * n_names + l] = (uint32_t)kv.second;
            blob.insert(blob.end(), kv.first.begin(), kv.first.end());
            ++l;
        }
        if (!d_name_blob.need(blob.size() + 1) || !d_name_tab.need(cols.size())) return false;
        if (!blob.empty() && hipMemcpy(d_name_blob.p, blob.data(), blob.size(), hipMemcpyHostToDevice) != hipSuccess) return false;
        return hipMemcpy(d_name_tab.p, cols.data(), cols.size() * 4, hipMemcpyHostToDevice) == hipSuccess;
    }
    // room for `more` bytes behind the window's end: what is left moves to the other buffer when this one is full
    bool make_room(size_t more)
    {
        if (end + more + GS_SLACK <= d_win[wi].cap) return true;
        const size_t left = end - cur;
        DevBuf<uint8_t>& O = d_win[wi ^ 1];
        if (!O.need(std::max(d_win[wi].cap, 2 * GS_SLACK + left + more + left / 2))) return false;
        if (left && hipMemcpyAsync(O.p + GS_SLACK, win() + cur, left, hipMemcpyDeviceToDevice, s) != hipSuccess) return false;
        if (!sync()) return false;
        wi ^= 1;
        cur = GS_SLACK; end = GS_SLACK + left;
        return true;
    }
};

GpuSamReader::GpuSamReader() {}
GpuSamReader::~GpuSamReader()
{
    delete p_;
    if (fd_ > 0) close(fd_);
}
double GpuSamReader::seconds_producer_reading() const { return bg_ ? bg_->seconds_reading() : 0; }
double GpuSamReader::seconds_producer_waiting_for_chunks() const { return bg_ ? bg_->seconds_producer_waiting_for_chunks() : 0; }
double GpuSamReader::seconds_waiting_for_runs() const { return bg_ ? bg_->seconds_waiting_for_runs() : 0; }

void GpuSamReader::start_bgzf(const BamHeader& hdr, const std::map<std::string, int32_t>& ref_index, uint64_t first_record_u, const char* path)
{
    hdr_ = hdr;
    ref_index_ = ref_index;
    bg_skip_ = first_record_u;
    bg_path_ = path ? path : "";
    bg_.reset(new GpuBamReader());
}

void GpuSamReader::allow_kernels()
{
    if (!p_) return;
    if (bg_) bg_->allow_kernels();
    { std::lock_guard<std::mutex> lk(p_->m); p_->kernels_ok = true; }
    p_->cv.notify_all();
}

bool GpuSamReader::start(int fd, size_t hold_bytes, std::string& err)
{
    fd_ = fd;
    if (fd < 0) { err = "no input stream"; return false; }
    size_t scan = 0;
    bool header_done = false;
    std::string line;
    auto scan_header = [&](bool at_end) {
        while (!header_done && scan < pre_.size()) {
            const char* p = pre_.data() + scan;
            const char* e = (const char*)memchr(p, '\n', pre_.size() - scan);
            if (!e && !at_end) return;
            const size_t n = e ? (size_t)(e - p) : pre_.size() - scan;
            sam_take_line(p, n, e != nullptr, line);
            if (!line.empty() && line[0] != '@') { header_done = true; return; } // (the first record line: scan stays at its start)
            if (!line.empty()) sam_header_line(line, hdr_, ref_index_);
            scan += n + (e ? 1 : 0);
        }
    };
    // (... and the first record line is whole: a header without @RG lines makes the caller ask for one record before any reader thread exists)
    while (!pre_eof_ && !(header_done && pre_.size() >= hold_bytes && memchr(pre_.data() + scan, '\n', pre_.size() - scan))) {
        const size_t at = pre_.size(), want = 1u << 20;
        pre_.resize(at + want);
        ssize_t r;
        do r = ::read(fd, pre_.data() + at, want); while (r < 0 && errno == EINTR);
        if (r < 0) { pre_.resize(at); err = "could not read the input stream"; return false; }
        pre_.resize(at + (size_t)r);
        if (r == 0) pre_eof_ = true;
        scan_header(pre_eof_);
    }
    pre_at_ = scan;
    parse_read_groups(hdr_);
    return true;
}

bool GpuSamReader::open(int device, size_t batch_reads, size_t batch_bases, std::string& err)
{
    delete p_;
    p_ = new Impl();
    Impl& I = *p_;
    I.device = device; I.fd = fd_;
    I.timing = getenv("BQC_GB_TIMING") != nullptr;
    if (const char* e = getenv("BQC_GS_CHUNK_KB")) I.chunk_bytes = (size_t)std::max(4, atoi(e)) << 10;
    auto fail = [&](const char* what) { err = std::string("GPU reader: ") + what; return false; };
    if (hipSetDevice(device) != hipSuccess) return fail("no device");
    const size_t reads = std::min<size_t>(std::max<size_t>(batch_reads, 1), 1u << 22);
    const size_t typical_text = std::min<size_t>(reads * 440, batch_bases * 3) + (8u << 20);
    const size_t seg_cap = typical_text / GS_SEG + 2;
    // (the second source: the producer reads its first run while the buffers below are made; no window and no ring of this reader's own)
    if (bg_ && !bg_->open_runs(bg_path_.c_str(), device, bg_skip_, GS_SLACK, err)) return false;
    I.bg = bg_.get();
    if (I.bg) I.cur = I.end = 0;
    bool ok = (I.bg || I.d_win[0].need(2 * GS_SLACK + typical_text + 2 * I.chunk_bytes)) && I.d_seg.need(seg_cap) && I.h_seg.need(seg_cap) && I.d_line.need(seg_cap * GS_MAXR, true) &&
              I.d_pre.need(seg_cap * GS_MAXR, true) && I.d_base.need(seg_cap) && I.h_base.need(seg_cap) && I.d_pay.need(reads + GS_MAXR + 64) && I.d_lut.need(256);
    for (int k = 0; ok && !I.bg && k < Impl::kSlots; ++k) ok = hipHostMalloc((void**)&I.slots[k].p, I.chunk_bytes, hipHostMallocDefault) == hipSuccess;
    if (!ok) return fail("out of memory");
    gb_pool_fill(std::min<size_t>(reads * 400, batch_bases / 2 * 3 + reads * 40 + (64u << 20)) + (1u << 20), 10);
    if (I.bg) { I.s = I.bg->consumer_stream(); I.own_stream = false; } // (one stream: the producer's hand-over of a run and this reader's kernels are in order)
    else I.s = bqc_pool_stream(device, 2);
    if (!I.s) return fail("no stream");
    if (hipEventCreateWithFlags(&I.ev, hipEventBlockingSync | hipEventDisableTiming) != hipSuccess || hipMalloc((void**)&I.d_status, 64) != hipSuccess ||
        hipHostMalloc((void**)&I.h_status, 64, hipHostMallocDefault) != hipSuccess || hipMemset(I.d_status, 0, 64) != hipSuccess)
        return fail("out of memory");
    uint8_t lut[256];
    for (int c = 0; c < 256; ++c) lut[c] = (uint8_t)sam_base_code((unsigned char)c); // (the host's expression: host/bam_io.h)
    if (hipMemcpy(I.d_lut.p, lut, 256, hipMemcpyHostToDevice) != hipSuccess || !I.upload_lanes(hdr_) || !I.upload_names(ref_index_)) return fail("out of device memory");
    I.eof = pre_eof_ || I.bg != nullptr;
    if (!pre_eof_ && !I.bg) I.reader = std::thread([&I] { I.read_loop(); });
    return true;
}

int GpuSamReader::host_lines(const char* text, size_t n, bool last_line_open, HostBatch& o, size_t max_reads, size_t max_bases, size_t& used, std::string& err, int& err_code)
{
    SamLineParser P{hdr_, ref_index_, main_, nrec_};
    std::string line;
    size_t at = 0, bases = 0;
    while (at < n && o.n() < max_reads && bases < max_bases) {
        const char* p = text + at;
        const char* e = (const char*)memchr(p, '\n', n - at);
        if (!e && !last_line_open) break;
        const size_t len = e ? (size_t)(e - p) : n - at;
        sam_take_line(p, len, e != nullptr, line);
        const size_t s0 = o.seq.size(), q0 = o.qual.size(), c0 = o.cigar.size(), x0 = o.nm_extra_read.size();
        const int r = P.parse(line, o, err, err_code);
        if (r < 0) { // the records in front of this line are delivered first; the error is the next call's answer
            o.seq.resize(s0); o.qual.resize(q0); o.cigar.resize(c0); o.nm_extra_read.resize(x0); o.nm_extra_val.resize(x0);
            used = n;
            if (o.n() == 0) return -1;
            pending_err_ = err; pending_code_ = err_code; err.clear(); err_code = 0;
            return 1;
        }
        if (r) bases += o.l_seq.back();
        at += len + (e ? 1 : 0);
    }
    used = at;
    return o.n() ? 1 : 0;
}

int GpuSamReader::next_batch(HostBatch& o, size_t max_reads, size_t max_bases, std::string& err, int& err_code)
{
    o.clear();
    err_code = 0;
    if (!pending_err_.empty()) { err = pending_err_; err_code = pending_code_; return -1; }
    if (!p_) { // the whole stream is in memory and no device reader was set up: the host's parser
        size_t used = 0;
        const int rc = host_lines(pre_.data() + pre_at_, pre_.size() - pre_at_, true, o, max_reads, max_bases, used, err, err_code);
        pre_at_ += used;
        return rc;
    }
    Impl& I = *p_;
    auto fail_dev = [&](const char* what) { err = std::string("GPU reader: ") + what; err_code = BQC_ERR_DEVICE; return -1; };
    if (hipSetDevice(I.device) != hipSuccess) return fail_dev("device lost");
    {
        std::unique_lock<std::mutex> lk(I.m);
        I.cv.wait(lk, [&] { return I.kernels_ok; });
    }
    if (!I.main_set) {
        I.n_main = (uint32_t)main_.size();
        if (!I.d_main.need(main_.size() + 1)) return fail_dev("out of device memory");
        if (!main_.empty() && hipMemcpy(I.d_main.p, main_.data(), main_.size(), hipMemcpyHostToDevice) != hipSuccess) return fail_dev("copy failed");
        I.main_set = true;
    }
    const double t0 = gs_now();
    for (;;) {
        // the text a batch is expected to need, in the window
        uint64_t want;
        {
            const double per = I.avg_line_bytes > 0 ? I.avg_line_bytes : 440.0;
            double w = (double)std::min<size_t>(max_reads, 1u << 22) * per;
            if (I.avg_line_bases > 0) w = std::min(w, ((double)max_bases / I.avg_line_bases + 1.0) * per);
            want = (uint64_t)(w * 1.1) + (1u << 20) + I.grow;
            want = std::min<uint64_t>(want, 0x7FFF0000u);
        }
        if (I.bg && (I.end == I.cur || I.need_run) && !I.all_in) { // the text arrives on the card: the next run joins what is left of the window
            const double tw = gs_now();
            const uint8_t* w = nullptr;
            size_t n_ = 0;
            bool last = false;
            const int rc = I.bg->next_run(I.cur, w, n_, last, err, err_code);
            t_wait_in_ += gs_now() - tw;
            if (rc < 0) { pending_err_ = err; pending_code_ = err_code; return -1; } // the BGZF layer's words, as the host reader's (BQC_ERR_IO), or the device's — and every later call's answer: what is left in the window is no line
            I.need_run = false;
            if (rc > 0) { I.bg_win = w; I.cur = 0; I.end = n_; }
            if (rc == 0 || last) I.all_in = true;
        }
        while (!I.bg && I.end - I.cur < want && !I.all_in) {
            const uint8_t* src;
            size_t len;
            bool from_ring = false;
            if (pre_at_ < pre_.size()) { src = (const uint8_t*)pre_.data() + pre_at_; len = std::min<size_t>(pre_.size() - pre_at_, 64u << 20); }
            else {
                const double tw = gs_now();
                std::unique_lock<std::mutex> lk(I.m);
                I.cv.wait(lk, [&] { return I.filled > I.released || I.eof; });
                t_wait_in_ += gs_now() - tw;
                if (I.filled == I.released) { I.all_in = true; break; }
                src = I.slots[I.released % Impl::kSlots].p; len = I.slots[I.released % Impl::kSlots].len;
                from_ring = true;
            }
            const double tc = gs_now();
            if (!I.make_room(len)) return fail_dev("out of device memory");
            if (len && (hipMemcpyAsync(I.win() + I.end, src, len, hipMemcpyHostToDevice, I.s) != hipSuccess || !I.sync())) return fail_dev("copy failed");
            t_copy_ += gs_now() - tc;
            I.end += len;
            if (from_ring) {
                { std::lock_guard<std::mutex> lk(I.m); ++I.released; if (I.eof && I.filled == I.released) I.all_in = true; }
                I.cv.notify_all();
            } else {
                pre_at_ += len;
                if (pre_at_ == pre_.size()) { std::vector<char>().swap(pre_); pre_at_ = 0; if (pre_eof_) I.all_in = true; }
            }
        }
        { std::lock_guard<std::mutex> lk(I.m); t_read_ = I.t_read; if (I.io_error) { err = "could not read the input stream"; err_code = BQC_ERR_IO; return -1; } }
        const size_t have = I.end - I.cur;
        if (!have) { if (!I.all_in) continue; return 0; } // (an empty run: the next one)
        const uint32_t avail = (uint32_t)std::min<uint64_t>(have, want);
        const bool tail_ok = I.all_in && avail == have;
        const uint8_t* base = I.win() + I.cur;
        const uint32_t nseg = (avail + GS_SEG - 1) / GS_SEG;
        if (!I.d_seg.need(nseg) || !I.h_seg.need(nseg) || !I.d_line.need((size_t)nseg * GS_MAXR) || !I.d_pre.need((size_t)nseg * GS_MAXR) || !I.d_base.need(nseg) || !I.h_base.need(nseg))
            return fail_dev("out of device memory");
        const double tk = gs_now();
        hipLaunchKernelGGL(k_gs_lines, dim3(nseg), dim3(64), 0, I.s, base, avail, tail_ok ? 1u : 0u, I.d_seg.p, I.d_line.p, I.d_pre.p);
        if (hipMemcpyAsync(I.h_seg.p, I.d_seg.p, (size_t)nseg * sizeof(GsSeg), hipMemcpyDeviceToHost, I.s) != hipSuccess || !I.sync()) return fail_dev("line scan failed");
        // whole segments are taken while the batch has room
        uint64_t pos = 0, n = 0, bases = 0, so = 0, qo = 0, co = 0;
        uint32_t last_taken = 0, flags = 0;
        for (uint32_t s = 0; s < nseg; ++s) {
            GsBase& B = I.h_base.p[s];
            B = GsBase{so, qo, co, (uint32_t)n, 0};
            const GsSeg& S = I.h_seg.p[s];
            if (n && (n + S.count > max_reads || bases >= max_bases)) break;
            B.take = 1;
            last_taken = s + 1;
            flags |= S.flags;
            n += S.count; bases += S.qual_bytes; so += S.seq_bytes; qo += S.qual_bytes; co += S.cigar_words;
            if (S.exit > pos) pos = S.exit;
            if (S.flags & GS_INCOMPLETE) break;
        }
        if (n == 0) {
            if (pos) { I.cur += pos; continue; } // (lines that are no records)
            if (tail_ok) return 0;               // (cannot happen: the stream's last line is complete as it is)
            if (I.bg && avail == have) { I.need_run = true; continue; } // a line that goes on in the next run
            I.grow += 2ull * avail + (4u << 20); // a line longer than the window looked at
            if (I.grow > 0x7FFF0000u) { err = "corrupt SAM record (a line of more than 2 GB)"; err_code = BQC_ERR_IO; return -1; }
            continue;
        }
        I.grow = 0;
        ++n_batches_;
        const size_t N = (size_t)n;
        bool exception = (flags & GS_EXCEPTION) != 0;
        if (!exception) {
            GbBatch L;
            if (const char* what = gb_batch_layout(o, I.d_cols, N, max_reads, GS_MAXR, so, qo, co, L)) return fail_dev(what);
            if (!I.d_pay.need(N + 64)) return fail_dev("out of device memory");
            GbLanes LN{I.d_lane_blob.p, I.d_lane_tab.p, I.d_lane_tab.p + I.n_lane_ids, I.d_lane_tab.p + 2 * (size_t)I.n_lane_ids, I.n_lane_ids, I.lane_count};
            GsNames RN{I.d_name_blob.p, I.d_name_tab.p, I.d_name_tab.p + I.n_names, (const int32_t*)(I.d_name_tab.p + 2 * (size_t)I.n_names), I.n_names};
            if (hipMemcpyAsync(I.d_base.p, I.h_base.p, (size_t)last_taken * sizeof(GsBase), hipMemcpyHostToDevice, I.s) != hipSuccess) return fail_dev("copy failed");
            hipLaunchKernelGGL(k_gs_decode, dim3(last_taken), dim3(64), 0, I.s, base, I.d_seg.p, I.d_line.p, I.d_pre.p, I.d_base.p, L.C, I.d_pay.p, LN, RN, I.d_main.p, I.n_main, I.d_status);
            hipLaunchKernelGGL(k_gs_payload, dim3((uint32_t)((N + 15) / 16)), dim3(256), 0, I.s, base, L.C, I.d_pay.p, (uint32_t)N, I.d_lut.p, L.seq, L.qual, (uint32_t*)L.cigar, I.d_status);
            std::string aerr;
            if (const char* what = gb_batch_finish(o, L, anchor_ctx_.load(), anchors_ok_, n_anchored_, I.s, I.ev, I.d_status, I.h_status, aerr)) return fail_dev(what);
            exception = *I.h_status != 0;
            if (exception && hipMemsetAsync(I.d_status, 0, 4, I.s) != hipSuccess) return fail_dev("memset failed");
        } else anchors_ok_ = false; // (the host keeps the window state from this batch on, as after any batch handed over)
        t_kern_ += gs_now() - tk;
        if (exception) {
            // A line the card has no rule for: THIS batch is parsed by the host's line parser from the window's bytes, which decides what
            // is an error and learns read groups that are not in the header; the run goes on from the card with the next batch.
            o.clear();
            try { I.handover.resize((size_t)pos); } catch (const std::bad_alloc&) { err = "no host memory for a batch handed over"; err_code = BQC_ERR_IO; return -1; }
            if (hipMemcpy(I.handover.data(), base, (size_t)pos, hipMemcpyDeviceToHost) != hipSuccess) return fail_dev("copy failed");
            size_t used = 0;
            const int rc = host_lines(I.handover.data(), (size_t)pos, tail_ok && pos == avail, o, SIZE_MAX, SIZE_MAX, used, err, err_code);
            ++n_handed_over_;
            if (hdr_.lane_names.size() != I.n_lane_ids && !I.upload_lanes(hdr_)) return fail_dev("out of device memory");
            I.cur += pos;
            if (I.timing) fprintf(stderr, "[sam reader] batch of %zu lines handed over to the host parser (%.1f ms)\n", N, (gs_now() - t0) * 1e3);
            if (rc == 0) continue; // (no record among them after all)
            return rc;
        }
        I.cur += pos;
        nrec_ += n;
        I.avg_line_bytes = (double)pos / (double)n;
        I.avg_line_bases = (double)bases / (double)n;
        if (I.timing) fprintf(stderr, "[sam reader] batch of %zu records (%.1f MB of text): %.1f ms\n", N, pos / 1e6, (gs_now() - t0) * 1e3);
        return 1;
    }
}
