// bqc_writer.cpp — `.bamqc` text emission (drop-in for writeOutput, reference
// src/bamqualcheck.cpp:156-233; printString :130-139; ten_most_abundant_kmers
// OverallNumbers.hpp:170-216; avgQualPerPos QualityCheck.hpp:273-279; writeTripletCounts
// TripletCounting.hpp:271-301).  Host-only code, part of libbamqc_gpu.so.
#include <algorithm>
#include <charconv>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/bamqc.h"

namespace {
struct Out {
    std::string s;
    void str(const char* p) { s.append(p); }
    void u64(uint64_t v)
    {
        char b[24];
        auto r = std::to_chars(b, b + sizeof b, v);
        s.append(b, r.ptr);
    }
    void line_u64(const char* key, uint64_t v) { str(key); s.push_back(' '); u64(v); s.push_back('\n'); }
    void array(const char* key, const uint64_t* v, size_t n) // `key` + " " + value ... ; empty array prints the bare key
    {
        str(key);
        for (size_t i = 0; i < n; ++i) { s.push_back(' '); u64(v[i]); }
        s.push_back('\n');
    }
    void dbl(double d) // default ostream formatting: 6 significant digits, %g style
    {
        char b[40];
        int n = snprintf(b, sizeof b, "%g", d);
        s.append(b, (size_t)n);
    }
};

// Ten largest counts, then for each the lowest index holding it that has not been used yet.
// The reference selects with std::greater<int> (values truncated to int, OverallNumbers.hpp:177).
void top_kmers(Out& o, const uint64_t* em)
{
    std::vector<uint64_t> v(em, em + BQC_N_8MER);
    std::partial_sort(v.begin(), v.begin() + 10, v.end(), [](uint64_t a, uint64_t b) { return (int)a > (int)b; });
    uint64_t top[10];
    std::copy(v.begin(), v.begin() + 10, top);
    std::sort(top, top + 10, [](uint64_t a, uint64_t b) { return a > b; });
    int used[10];
    for (int i = 0; i < 10; ++i) {
        int pos = 0;
        for (; pos < BQC_N_8MER; ++pos) {
            if (em[pos] != top[i]) continue;
            bool seen = false;
            for (int k = 0; k < i; ++k) seen |= used[k] == pos;
            if (!seen) break;
        }
        used[i] = pos;
        char kmer[9];
        for (int k = 0; k < 8; ++k) kmer[k] = "ACGT"[(pos >> (2 * (7 - k))) & 3];
        kmer[8] = 0;
        o.str("nr_"); o.u64((uint64_t)i + 1); o.str("_most_abundant_8mer "); o.str(kmer); o.s.push_back(' '); o.u64(top[i]); o.s.push_back('\n');
    }
}

void avgqual(Out& o, const char* key, const bqc_mate_counts& m)
{
    o.str(key);
    const double nr = (double)(uint32_t)m.qualcount_readnr;
    for (uint32_t i = 0; i < m.n_cycles; ++i) { o.s.push_back(' '); o.dbl((double)m.qualcount[i] / nr); }
    o.s.push_back('\n');
}
int write_file(const Out& o, const char* path)
{
    FILE* f = fopen(path, "wb");
    if (!f) return BQC_ERR_IO;
    size_t w = fwrite(o.s.data(), 1, o.s.size(), f);
    int rc = fclose(f);
    return (w == o.s.size() && rc == 0) ? 0 : BQC_ERR_IO;
}
} // namespace

extern "C" int bqc_write_bamqc(const bqc_counts* counts, const bqc_header_info* hdr, const char* path)
{
    if (!counts || !hdr || !path) return BQC_ERR_ARG;
    Out o;
    o.s.reserve(1 << 20);
    for (uint32_t n = 0; n < hdr->n_names; ++n) {
        if (hdr->lane_index[n] >= counts->n_lanes) return BQC_ERR_ARG;
        const bqc_lane_counts& L = counts->lanes[hdr->lane_index[n]];
        const bqc_mate_counts &a = L.mate[0], &b = L.mate[1];
        o.str("sample_id "); o.str(hdr->sample_id ? hdr->sample_id : ""); o.s.push_back('\n');
        o.str("lane "); o.str(hdr->lane_names[n]); o.s.push_back('\n');
        o.line_u64("total_read_pairs", (uint32_t)L.scalars[BQC_S_READCOUNT] / 2);
        o.line_u64("total_bps", L.scalars[BQC_S_TOTALBPS]);
        o.line_u64("supplementary_alignments", L.scalars[BQC_S_SUPPLEMENTARY]);
        o.line_u64("marked_duplicate", L.scalars[BQC_S_DUPLICATES]);
        o.line_u64("QC_failed", L.scalars[BQC_S_QCFAILED]);
        o.line_u64("not_primary_alignment", L.scalars[BQC_S_NOT_PRIMARY]);
        o.line_u64("both_reads_unmapped", L.scalars[BQC_S_BOTHUNMAPPED]);
        o.line_u64("first_read_unmapped", L.scalars[BQC_S_FIRSTUNMAPPED]);
        o.line_u64("second_read_unmapped", L.scalars[BQC_S_SECONDUNMAPPED]);
        o.line_u64("first_and_or_second_read_mapped", L.scalars[BQC_S_FIRST_AND_OR_SECOND_MAPPED]);
        o.line_u64("FF_RR_oriented_pairs", L.scalars[BQC_S_FF_RR]);
        o.line_u64("total_proper_pairs", L.scalars[BQC_S_PROPERPAIR]);
        o.line_u64("total_proper_pairs_autosome", L.scalars[BQC_S_AUTO_PROPERPAIR]);
        o.array("genome_coverage_histogram", L.poscov, BQC_COVSIZE + 1);
        o.array("insert_size_histogram", a.insertSize, a.n_insertSize);
        struct { const char* key; const uint64_t* bqc_mate_counts::*arr; uint32_t bqc_mate_counts::*len; } hists[] = {
            {"read_length_histogram", &bqc_mate_counts::readLength, &bqc_mate_counts::n_readLength},
            {"N_count_histogram", &bqc_mate_counts::Ncount, &bqc_mate_counts::n_Ncount},
            {"GC_content_histogram", &bqc_mate_counts::GCcount, &bqc_mate_counts::n_GCcount},
            {"average_base_qual_histogram", &bqc_mate_counts::averageQual, &bqc_mate_counts::n_averageQual},
            {"mapping_qual_histogram", &bqc_mate_counts::mapQ, &bqc_mate_counts::n_mapQ},
            {"mismatch_count_histogram", &bqc_mate_counts::mismatch, &bqc_mate_counts::n_mismatch},
            {"deletion_count_histogram", &bqc_mate_counts::delhist, &bqc_mate_counts::n_delhist},
            {"insertion_count_histogram", &bqc_mate_counts::inshist, &bqc_mate_counts::n_inshist},
        };
        for (auto& h : hists) {
            std::string k1 = std::string(h.key) + "_first", k2 = std::string(h.key) + "_second";
            o.array(k1.c_str(), a.*(h.arr), a.*(h.len));
            o.array(k2.c_str(), b.*(h.arr), b.*(h.len));
        }
        static const int order[5] = {4, 0, 1, 2, 3}; // N A C G T
        static const char* bn[5] = {"Ns", "As", "Cs", "Gs", "Ts"};
        for (int k = 0; k < 5; ++k) {
            std::string k1 = std::string(bn[k]) + "_by_position_first", k2 = std::string(bn[k]) + "_by_position_second";
            o.array(k1.c_str(), a.dnacount[order[k]], a.n_cycles);
            o.array(k2.c_str(), b.dnacount[order[k]], b.n_cycles);
        }
        avgqual(o, "average_base_qual_by_position_first", a);
        avgqual(o, "average_base_qual_by_position_second", b);
        o.array("soft_clipping_5_prime_by_position_first", a.sc5, a.n_cycles);
        o.array("soft_clipping_3_prime_by_position_first", a.sc3, a.n_cycles);
        o.array("soft_clipping_5_prime_by_position_second", b.sc5, b.n_cycles);
        o.array("soft_clipping_3_prime_by_position_second", b.sc3, b.n_cycles);
        top_kmers(o, L.eightmer);
        o.array("8mer_count", L.eightmer, BQC_N_8MER);
        for (uint32_t s = 0; s < L.n_sketch; ++s) { // bamqualcheck.cpp:221-230
            const bqc_sketch_counts& k = L.sketch[s];
            std::string ks = std::to_string(k.k), qs = std::to_string(k.q);
            o.line_u64((ks + "mer_count_after_qual_clipping_" + qs).c_str(), k.sumCount);
            o.line_u64(("distinct_" + ks + "mer_count_after_qual_clipping_" + qs).c_str(), k.F0);
            o.line_u64(("unique_" + ks + "mer_count_after_qual_clipping_" + qs).c_str(), k.f1);
            o.line_u64((ks + "mer_F2_after_qual_clipping_" + qs).c_str(), k.F2);
        }
        static const char* grp[4] = {"1st_FW", "1st_RC", "2nd_FW", "2nd_RC"};
        static const int gidx[4] = {0, 2, 1, 3}; // state order: fwd1st, fwd2nd, rev1st, rev2nd
        std::vector<uint64_t> row(64);
        for (int bi = 0; bi < 4; ++bi)
            for (int g = 0; g < 4; ++g) {
                for (int x = 0; x < 64; ++x) row[x] = L.triplet[x * 16 + gidx[g] * 4 + bi];
                std::string key = std::string("triplet_counts_") + "ACGT"[bi] + "_" + grp[g];
                o.array(key.c_str(), row.data(), 64);
            }
    }
    return write_file(o, path);
}

// The per-cycle base quality histograms as text (include/bamqc.h): per lane and mate a key line with the table's sizes, then one line
// of n_q counts per cycle.
extern "C" int bqc_write_qual_by_cycle(bqc_ctx* ctx, const bqc_header_info* hdr, const char* path)
{
    if (!ctx || !hdr || !path) return BQC_ERR_ARG;
    Out o;
    o.s.reserve(1 << 16);
    static const char* keys[2] = {"base_qual_histogram_by_position_first", "base_qual_histogram_by_position_second"};
    for (uint32_t n = 0; n < hdr->n_names; ++n) {
        o.str("sample_id "); o.str(hdr->sample_id ? hdr->sample_id : ""); o.s.push_back('\n');
        o.str("lane "); o.str(hdr->lane_names[n]); o.s.push_back('\n');
        for (uint32_t m = 0; m < 2; ++m) {
            bqc_qbc_view v;
            const int rc = bqc_qual_by_cycle(ctx, hdr->lane_index[n], m, &v);
            if (rc) return rc;
            o.str(keys[m]); o.s.push_back(' '); o.u64(v.n_cycles); o.s.push_back(' '); o.u64(v.n_q); o.s.push_back('\n');
            if (!v.n_q) continue; // no counted base: no rows
            for (uint32_t c = 0; c < v.n_cycles; ++c) {
                const uint64_t* row = v.hist + (uint64_t)c * v.stride;
                for (uint32_t q = 0; q < v.n_q; ++q) { if (q) o.s.push_back(' '); o.u64(row[q]); }
                o.s.push_back('\n');
            }
        }
    }
    return write_file(o, path);
}

// The mismatches by cycle and base quality as text (include/bamqc.h): per lane and mate the table of compared bases, then the table of
// mismatches, each a key line with the sizes and one line of n_q counts per cycle.
extern "C" int bqc_write_mismatch_by_cycle(bqc_ctx* ctx, const bqc_header_info* hdr, const char* path)
{
    if (!ctx || !hdr || !path) return BQC_ERR_ARG;
    Out o;
    o.s.reserve(1 << 16);
    static const char* keys[2][2] = {{"aligned_bases_by_position_and_qual_first", "mismatches_by_position_and_qual_first"},
                                     {"aligned_bases_by_position_and_qual_second", "mismatches_by_position_and_qual_second"}};
    for (uint32_t n = 0; n < hdr->n_names; ++n) {
        o.str("sample_id "); o.str(hdr->sample_id ? hdr->sample_id : ""); o.s.push_back('\n');
        o.str("lane "); o.str(hdr->lane_names[n]); o.s.push_back('\n');
        for (uint32_t m = 0; m < 2; ++m) {
            bqc_mbc_view v;
            const int rc = bqc_mismatch_by_cycle(ctx, hdr->lane_index[n], m, &v);
            if (rc) return rc;
            for (uint32_t t = 0; t < 2; ++t) {
                const uint64_t* tbl = t ? v.mismatch : v.aligned;
                o.str(keys[m][t]); o.s.push_back(' '); o.u64(v.n_cycles); o.s.push_back(' '); o.u64(v.n_q); o.s.push_back('\n');
                if (!v.n_q) continue; // no compared base: no rows
                for (uint32_t c = 0; c < v.n_cycles; ++c) {
                    const uint64_t* row = tbl + (uint64_t)c * v.stride;
                    for (uint32_t q = 0; q < v.n_q; ++q) { if (q) o.s.push_back(' '); o.u64(row[q]); }
                    o.s.push_back('\n');
                }
            }
        }
    }
    return write_file(o, path);
}

// The adapter content by cycle as text (include/bamqc.h): per lane and mate the reads by length, then one line of first hits per adapter
// of the set, key-then-values lines as in the `.bamqc`.
extern "C" int bqc_write_adapter_by_cycle(bqc_ctx* ctx, const bqc_header_info* hdr, const char* path)
{
    if (!ctx || !hdr || !path) return BQC_ERR_ARG;
    Out o;
    o.s.reserve(1 << 16);
    static const char* keys[2][2] = {{"adapter_reads_by_length_first", "adapter_first_hit_by_position_first"},
                                     {"adapter_reads_by_length_second", "adapter_first_hit_by_position_second"}};
    for (uint32_t n = 0; n < hdr->n_names; ++n) {
        o.str("sample_id "); o.str(hdr->sample_id ? hdr->sample_id : ""); o.s.push_back('\n');
        o.str("lane "); o.str(hdr->lane_names[n]); o.s.push_back('\n');
        for (uint32_t m = 0; m < 2; ++m) {
            bqc_adp_view v;
            const int rc = bqc_adapter_by_cycle(ctx, hdr->lane_index[n], m, &v);
            if (rc) return rc;
            o.array(keys[m][0], v.reads_by_length, v.n_cycles);
            for (uint32_t a = 0; a < v.n_adapters; ++a) {
                const std::string key = std::string(keys[m][1]) + " " + v.adapters[a].name + " " + v.adapters[a].seq;
                o.array(key.c_str(), v.first_hit + (uint64_t)a * v.stride, v.n_cycles);
            }
        }
    }
    return write_file(o, path);
}

// The GC bias tables as text (include/bamqc.h): per lane the window length, the genome's windows by GC bin (the same line for every
// lane: the table belongs to the genome) and the lane's three read tables, key-then-values lines as in the `.bamqc`.
extern "C" int bqc_write_gc_bias(bqc_ctx* ctx, const bqc_header_info* hdr, const char* path)
{
    if (!ctx || !hdr || !path) return BQC_ERR_ARG;
    Out o;
    o.s.reserve(1 << 14);
    for (uint32_t n = 0; n < hdr->n_names; ++n) {
        bqc_gcb_view v;
        const int rc = bqc_gc_bias(ctx, hdr->lane_index[n], &v);
        if (rc) return rc;
        o.str("sample_id "); o.str(hdr->sample_id ? hdr->sample_id : ""); o.s.push_back('\n');
        o.str("lane "); o.str(hdr->lane_names[n]); o.s.push_back('\n');
        o.line_u64("gc_bias_window", v.window);
        o.array("genome_windows_by_gc", v.genome_windows, v.n_bins);
        o.array("read_starts_by_gc", v.read_starts, v.n_bins);
        o.array("bases_by_gc", v.bases, v.n_bins);
        o.array("base_qual_sum_by_gc", v.qual_sum, v.n_bins);
    }
    return write_file(o, path);
}

// The indel tables as text (include/bamqc.h): per lane and mate the reads by length, the insertions and the deletions by cycle and
// the two length histograms, key-then-values lines as in the `.bamqc`.
extern "C" int bqc_write_indel_by_cycle(bqc_ctx* ctx, const bqc_header_info* hdr, const char* path)
{
    if (!ctx || !hdr || !path) return BQC_ERR_ARG;
    Out o;
    o.s.reserve(1 << 14);
    static const char* const mates[2] = {"first", "second"};
    for (uint32_t n = 0; n < hdr->n_names; ++n) {
        o.str("sample_id "); o.str(hdr->sample_id ? hdr->sample_id : ""); o.s.push_back('\n');
        o.str("lane "); o.str(hdr->lane_names[n]); o.s.push_back('\n');
        for (uint32_t m = 0; m < 2; ++m) {
            bqc_ibc_view v;
            const int rc = bqc_indel_by_cycle(ctx, hdr->lane_index[n], m, &v);
            if (rc) return rc;
            const std::string sfx = std::string("_") + mates[m];
            o.array(("indel_reads_by_length" + sfx).c_str(), v.reads_by_length, v.n_cycles);
            o.array(("insertions_by_position" + sfx).c_str(), v.insertions, v.n_cycles);
            o.array(("deletions_by_position" + sfx).c_str(), v.deletions, v.n_cycles);
            o.array(("insertion_length_histogram" + sfx).c_str(), v.insertion_lengths, v.n_len);
            o.array(("deletion_length_histogram" + sfx).c_str(), v.deletion_lengths, v.n_len);
        }
    }
    return write_file(o, path);
}

// The substitution tables as text (include/bamqc.h): per lane the two thresholds, then per mate the contexts of the reads on the
// forward and on the reverse strand, one line a context, and the base pairs by cycle, one line a cycle.
extern "C" int bqc_write_substitutions(bqc_ctx* ctx, const bqc_header_info* hdr, const char* path)
{
    if (!ctx || !hdr || !path) return BQC_ERR_ARG;
    Out o;
    o.s.reserve(1 << 16);
    static const char* const mates[2] = {"first", "second"};
    static const char* const strands[2] = {"forward", "reverse"};
    for (uint32_t n = 0; n < hdr->n_names; ++n) {
        o.str("sample_id "); o.str(hdr->sample_id ? hdr->sample_id : ""); o.s.push_back('\n');
        o.str("lane "); o.str(hdr->lane_names[n]); o.s.push_back('\n');
        for (uint32_t m = 0; m < 2; ++m) {
            bqc_sbc_view v;
            const int rc = bqc_substitutions(ctx, hdr->lane_index[n], m, &v);
            if (rc) return rc;
            if (m == 0) {
                o.line_u64("substitution_min_base_qual", v.min_base_qual);
                o.line_u64("substitution_min_mapq", v.min_mapq);
            }
            for (uint32_t s = 0; s < 2; ++s)
                for (uint32_t x = 0; x < 64; ++x) {
                    const char name[4] = {"ACGT"[x >> 4], "ACGT"[(x >> 2) & 3], "ACGT"[x & 3], 0};
                    o.array((std::string("substitutions_by_context_") + mates[m] + "_" + strands[s] + " " + name).c_str(), v.by_context + (s * 64 + x) * 4, 4);
                }
            o.str((std::string("substitutions_by_position_") + mates[m]).c_str()); o.s.push_back(' '); o.u64(v.n_cycles); o.str(" 16\n");
            for (uint32_t c = 0; c < v.n_cycles; ++c) {
                for (uint32_t k = 0; k < 16; ++k) { if (k) o.s.push_back(' '); o.u64(v.by_cycle[c * 16 + k]); }
                o.s.push_back('\n');
            }
        }
    }
    return write_file(o, path);
}

// The allele counts at the given sites as text (include/bamqc.h): per lane the two thresholds and the number of sites, then one line a
// site, in the table's order: the contig's name, the position counted from 1 and the eight counts, forward A C G T then reverse.
extern "C" int bqc_write_site_alleles(bqc_ctx* ctx, const bqc_header_info* hdr, const char* const* ref_names, uint32_t n_refs, const char* path)
{
    if (!ctx || !hdr || !path || (!ref_names && n_refs)) return BQC_ERR_ARG;
    Out o;
    o.s.reserve(1 << 16);
    for (uint32_t n = 0; n < hdr->n_names; ++n) {
        bqc_sac_view v;
        const int rc = bqc_site_alleles(ctx, hdr->lane_index[n], &v);
        if (rc) return rc;
        o.str("sample_id "); o.str(hdr->sample_id ? hdr->sample_id : ""); o.s.push_back('\n');
        o.str("lane "); o.str(hdr->lane_names[n]); o.s.push_back('\n');
        o.line_u64("site_allele_min_base_qual", v.min_base_qual);
        o.line_u64("site_allele_min_mapq", v.min_mapq);
        o.line_u64("site_alleles", v.n_sites);
        for (uint32_t s = 0; s < v.n_sites; ++s) {
            if ((uint32_t)v.rid[s] >= n_refs || !ref_names[v.rid[s]]) return BQC_ERR_ARG; // (a site's contig has no name)
            o.str(ref_names[v.rid[s]]); o.s.push_back(' '); o.u64((uint64_t)v.pos[s] + 1);
            for (uint32_t k = 0; k < 8; ++k) { o.s.push_back(' '); o.u64(v.counts[(uint64_t)s * 8 + k]); }
            o.s.push_back('\n');
        }
    }
    return write_file(o, path);
}

// The depth over the given regions as text (include/bamqc.h): per lane the scalars, the thresholds and the histogram (its length
// first), then one line a region, in the list's order: the contig's name, start and end as a BED file gives them, the depth's sum, min
// and max and the positions at or above each threshold.
extern "C" int bqc_write_region_coverage(bqc_ctx* ctx, const bqc_header_info* hdr, const char* const* ref_names, uint32_t n_refs, const char* path)
{
    if (!ctx || !hdr || !path || (!ref_names && n_refs)) return BQC_ERR_ARG;
    Out o;
    o.s.reserve(1 << 16);
    for (uint32_t n = 0; n < hdr->n_names; ++n) {
        bqc_rcv_view v;
        const int rc = bqc_region_coverage(ctx, hdr->lane_index[n], &v);
        if (rc) return rc;
        const uint32_t C = 3 + v.n_thresholds;
        o.str("sample_id "); o.str(hdr->sample_id ? hdr->sample_id : ""); o.s.push_back('\n');
        o.str("lane "); o.str(hdr->lane_names[n]); o.s.push_back('\n');
        o.line_u64("region_min_mapq", v.min_mapq);
        o.line_u64("region_reads_examined", v.reads_examined);
        o.line_u64("region_reads_on_target", v.reads_on_target);
        o.line_u64("region_aligned_bases", v.aligned_bases);
        o.line_u64("region_bases_on_target", v.bases_on_target);
        o.line_u64("region_target_bases", v.target_bases);
        o.array("region_depth_thresholds", v.thresholds, v.n_thresholds);
        o.str("region_depth_histogram "); o.u64((uint64_t)v.depth_cap + 1);
        for (uint32_t d = 0; d <= v.depth_cap; ++d) { o.s.push_back(' '); o.u64(v.hist[d]); }
        o.s.push_back('\n');
        o.line_u64("regions", v.n_regions);
        for (uint32_t k = 0; k < v.n_regions; ++k) {
            if ((uint32_t)v.rid[k] >= n_refs || !ref_names[v.rid[k]]) return BQC_ERR_ARG; // (a region's contig has no name)
            o.str(ref_names[v.rid[k]]); o.s.push_back(' '); o.u64((uint64_t)v.start[k]); o.s.push_back(' '); o.u64((uint64_t)v.end[k]);
            for (uint32_t q = 0; q < C; ++q) { o.s.push_back(' '); o.u64(v.regions[(uint64_t)k * C + q]); }
            o.s.push_back('\n');
        }
    }
    return write_file(o, path);
}

// The duplicate sets as text (include/bamqc.h): the capacity, per lane of `hdr` the five sums, then the sets over all read groups.
extern "C" int bqc_write_duplicate_sets(bqc_ctx* ctx, const bqc_header_info* hdr, const char* path)
{
    if (!ctx || !hdr || !path) return BQC_ERR_ARG;
    bqc_dup_view v;
    const int rc = bqc_duplicate_sets(ctx, &v);
    if (rc) return rc;
    Out o;
    o.s.reserve(1 << 14);
    o.str("sample_id "); o.str(hdr->sample_id ? hdr->sample_id : ""); o.s.push_back('\n');
    o.line_u64("duplicate_sets_capacity", v.capacity);
    for (uint32_t n = 0; n < hdr->n_names; ++n) {
        if (hdr->lane_index[n] >= v.n_lanes) return BQC_ERR_ARG;
        const uint64_t* s = v.lanes + (uint64_t)hdr->lane_index[n] * 5;
        o.str("lane "); o.str(hdr->lane_names[n]); o.s.push_back('\n');
        o.line_u64("duplicate_reads_examined_single", s[0]);
        o.line_u64("duplicate_reads_examined_pair", s[1]);
        o.line_u64("duplicate_reads_flagged_single", s[2]);
        o.line_u64("duplicate_reads_flagged_pair", s[3]);
        o.line_u64("duplicate_reads_second_end", s[4]);
    }
    o.str("all_lanes\n");
    o.line_u64("duplicate_sets_single", v.sets[0]);
    o.line_u64("duplicate_sets_pair", v.sets[1]);
    o.line_u64("duplicate_set_largest_single", v.largest[0]);
    o.line_u64("duplicate_set_largest_pair", v.largest[1]);
    o.array("duplicate_set_size_histogram_single", v.hist[0], 256);
    o.array("duplicate_set_size_histogram_pair", v.hist[1], 256);
    o.line_u64("duplicate_estimated_library_size", v.estimated_library_size);
    return write_file(o, path);
}

// The overrepresented sequences as text (include/bamqc.h): the parameters, per lane of `hdr` the four sums, then per mate the sets over
// all read groups and the list.
extern "C" int bqc_write_overrepresented(bqc_ctx* ctx, const bqc_header_info* hdr, const char* path)
{
    if (!ctx || !hdr || !path) return BQC_ERR_ARG;
    bqc_ovr_view v;
    const int rc = bqc_overrepresented(ctx, &v);
    if (rc) return rc;
    Out o;
    o.s.reserve(1 << 14);
    o.str("sample_id "); o.str(hdr->sample_id ? hdr->sample_id : ""); o.s.push_back('\n');
    o.line_u64("overrepresented_len", v.prefix_len);
    o.line_u64("overrepresented_ppm", v.ppm);
    o.line_u64("overrepresented_capacity", v.capacity);
    for (uint32_t n = 0; n < hdr->n_names; ++n) {
        if (hdr->lane_index[n] >= v.n_lanes) return BQC_ERR_ARG;
        const uint64_t* s = v.lanes + (uint64_t)hdr->lane_index[n] * 4;
        o.str("lane "); o.str(hdr->lane_names[n]); o.s.push_back('\n');
        o.line_u64("sequence_reads_examined_first", s[0]);
        o.line_u64("sequence_reads_examined_second", s[1]);
        o.line_u64("sequence_reads_skipped_first", s[2]);
        o.line_u64("sequence_reads_skipped_second", s[3]);
    }
    o.str("all_lanes\n");
    for (uint32_t m = 0; m < 2; ++m) {
        const std::string mate = m ? "_second" : "_first";
        o.line_u64(("sequences_distinct" + mate).c_str(), v.distinct[m]);
        o.line_u64(("sequence_set_largest" + mate).c_str(), v.largest[m]);
        o.array(("sequence_set_size_histogram" + mate).c_str(), v.hist[m], 256);
        o.line_u64(("overrepresented_threshold" + mate).c_str(), v.threshold[m]);
        o.line_u64(("overrepresented_sequences" + mate).c_str(), v.n_listed[m]);
        for (uint32_t e = 0; e < v.n_listed[m]; ++e) {
            const bqc_ovr_seq& q = v.listed[m][e];
            o.str(q.seq); o.s.push_back(' '); o.u64(q.count); o.s.push_back(' '); o.str(q.source); o.s.push_back('\n');
        }
    }
    return write_file(o, path);
}

// The depth in fixed genome windows as text (include/bamqc.h): per lane the scalars and the histogram (its length first), one line a
// contig in the header's order — name, length, windows and the three sums — then one line for every window with a word that is not 0,
// in order: the contig's name, the window's start and end, its reads, bases and bases of low mapping quality.
extern "C" int bqc_write_window_depth(bqc_ctx* ctx, const bqc_header_info* hdr, const char* const* ref_names, uint32_t n_refs, const char* path)
{
    if (!ctx || !hdr || !path || (!ref_names && n_refs)) return BQC_ERR_ARG;
    Out o;
    o.s.reserve(1 << 16);
    for (uint32_t n = 0; n < hdr->n_names; ++n) {
        bqc_wdp_view v;
        const int rc = bqc_window_depth(ctx, hdr->lane_index[n], &v);
        if (rc) return rc;
        if (v.n_refs != n_refs) return BQC_ERR_ARG; // (a name for every contig of the context)
        o.str("sample_id "); o.str(hdr->sample_id ? hdr->sample_id : ""); o.s.push_back('\n');
        o.str("lane "); o.str(hdr->lane_names[n]); o.s.push_back('\n');
        o.line_u64("window_depth_window", v.window);
        o.line_u64("window_depth_min_mapq", v.min_mapq);
        o.line_u64("window_depth_reads_examined", v.reads_examined);
        o.line_u64("window_depth_reads_low_mapq", v.reads_low_mapq);
        o.line_u64("window_depth_bases_outside_contigs", v.bases_outside);
        o.str("window_depth_histogram "); o.u64(BQC_WDP_HIST_BINS);
        for (uint32_t d = 0; d < BQC_WDP_HIST_BINS; ++d) { o.s.push_back(' '); o.u64(v.hist[d]); }
        o.s.push_back('\n');
        o.line_u64("contigs", n_refs);
        uint64_t lines = 0;
        for (uint32_t r = 0; r < n_refs; ++r) {
            if (!ref_names[r]) return BQC_ERR_ARG;
            o.str(ref_names[r]); o.s.push_back(' '); o.u64(v.ref_len[r]); o.s.push_back(' '); o.u64(v.woff[r + 1] - v.woff[r]);
            for (uint32_t q = 0; q < 3; ++q) { o.s.push_back(' '); o.u64(v.contigs[(size_t)r * 3 + q]); }
            o.s.push_back('\n');
        }
        for (uint32_t w = 0; w < v.n_windows; ++w) lines += (v.reads[w] | v.bases[w] | v.bases_low[w]) != 0;
        o.str("windows "); o.u64(lines); o.s.push_back(' '); o.u64(v.n_windows); o.s.push_back('\n');
        for (uint32_t r = 0; r < n_refs; ++r)
            for (uint32_t w = v.woff[r]; w < v.woff[r + 1]; ++w) {
                if (!(v.reads[w] | v.bases[w] | v.bases_low[w])) continue;
                const uint64_t from = (uint64_t)(w - v.woff[r]) * v.window, to = from + v.window < v.ref_len[r] ? from + v.window : v.ref_len[r];
                o.str(ref_names[r]); o.s.push_back(' '); o.u64(from); o.s.push_back(' '); o.u64(to);
                o.s.push_back(' '); o.u64(v.reads[w]); o.s.push_back(' '); o.u64(v.bases[w]); o.s.push_back(' '); o.u64(v.bases_low[w]);
                o.s.push_back('\n');
            }
    }
    return write_file(o, path);
}
