// program_options.h — the `bamqualcheck` command line (CommandLineParser.hpp:43-149, and the options of the modules the reference does
// not have): one table of options states each one's names, kind, bounds, messages, module and help paragraph; the parser, usage() and
// the rule "not with --gpus" read it.  Host only: no HIP header, no context, no device call — bqc_program_args answers from here.
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

namespace bqc_cli {
// Every number an optional module is configured with.  The first word of a module says whether it runs (0: off) — for most of them it
// is a parameter at once (cycles, a window length).  All words are of one type, so that an option row names its word with one kind of
// member pointer and two sets of settings compare as memory: no term of the comparison can be forgotten.
struct ModuleSettings {
    uint64_t qual_by_cycle = 0;     // --qual-by-cycle[-len N]: cycles, into <output>.qbc
    uint64_t mismatch_by_cycle = 0; // --mismatch-by-cycle[-len N]: cycles, into <output>.mbc
    uint64_t adapter_by_cycle = 0;  // --adapter-by-cycle[-len N], --adapter NAME=SEQ (ProgramOptions::adapters): cycles, into <output>.adp
    uint64_t gc_bias = 0;           // --gc-bias, --gc-bias-window W: the window length, into <output>.gcb
    uint64_t indel_by_cycle = 0;    // --indel-by-cycle[-len N]: cycles, into <output>.ibc
    uint64_t substitutions = 0, subst_min_qual = 20, subst_min_mapq = 30; // --substitutions[-len N], -min-qual Q, -min-mapq MQ: cycles, into <output>.sbc
    uint64_t site_alleles = 0, site_min_qual = 20, site_min_mapq = 20;    // --site-alleles FILE (1: given), -min-qual Q, -min-mapq MQ, into <output>.sac
    uint64_t regions = 0, regions_min_mapq = 20, regions_depth_cap = 1000; // --regions FILE (1: given), -min-mapq MQ, -depth-cap D, -thresholds LIST, into <output>.rcv
    uint64_t n_regions_thresholds = 6, regions_thresholds[8] = {1, 10, 20, 30, 50, 100, 0, 0}; // (words behind the n-th stay 0)
    uint64_t duplicate_sets = 0, duplicate_sets_capacity = 1ull << 26;    // --duplicate-sets, -capacity N (3 GiB of slots), into <output>.dup
    uint64_t overrepresented = 0, overrepresented_len = 50, overrepresented_ppm = 1000, overrepresented_capacity = 1ull << 26; // --overrepresented, -len K, -ppm P, -capacity N, into <output>.ovr
    uint64_t window_depth = 0, window_depth_size = 1000, window_depth_min_mapq = 20; // --window-depth, -size W, -min-mapq MQ, into <output>.wdp
    bool operator==(const ModuleSettings& o) const;
};
static_assert(std::has_unique_object_representations<ModuleSettings>::value, "ModuleSettings: words of one type, no padding (it is compared as memory)");

struct ProgramOptions {
    std::string bamFile, referenceFile = "genome.fa", outputFile;
    std::string chroms = "chr1,chr2,chr3,chr4,chr5,chr6,chr7,chr8,chr9,chr10,chr11,chr12,chr13,chr14,chr15,chr16,chr17,chr18,chr19,chr20,chr21,chr22";
    std::string kmer_sizes = "32", quality_cutoffs = "17"; // -k, -q as given; as numbers below
    std::vector<int32_t> klist;
    std::vector<uint32_t> q_cutoff;
    double e = 0.01;
    int seed = 1;
    int isize = 1000;
    // extensions (not in the reference)
    uint32_t max_read_len = 65536, hist_cap = 65536;
    int device = 0;
    uint32_t batch_reads = [] { const char* e = getenv("BQC_BATCH_READS"); return e && atoi(e) > 0 ? (uint32_t)atoi(e) : 1u << 20; }(); // (the variable: experiments; --batch-reads)
    bool no_sketch = false;
    ModuleSettings mod;
    std::vector<std::pair<std::string, std::string>> adapters; // --adapter NAME=SEQ (empty: the built-in set)
    std::string site_alleles, regions;                         // --site-alleles FILE, --regions FILE (empty: off)
    // --manifest LIST: many files through one resident worker (INPUT<TAB>OUTPUT per line); bamFile and outputFile stay empty
    std::string manifest;
    std::vector<std::pair<std::string, std::string>> jobs;
};

void usage(FILE* f);
// returns 0 = ok, 1 = parse error (err), 2 = help/version printed (exit 0)
// session_form: the options of a session (bqc_session_open) — the program's without an input, -o and --manifest
int parse_args(int argc, const char* const* argv, ProgramOptions& o, std::string& err, bool session_form = false);
// the positional rule (valid values: "- bam sam" by file extension, CommandLineParser.hpp:59-60), for a path that is not "-"
bool input_extension_ok(const std::string& path, std::string& err);
// --manifest LIST: one job per line; everything that is wrong with the list is found here, before any job runs
bool read_manifest(const std::string& path, std::vector<std::pair<std::string, std::string>>& jobs, std::string& err);

// Not with --gpus (no worker holds the whole genome; a set may have members in two workers' shards): the message about the first module
// of the table's order that cannot run so — the one an argument asks for, or the one that is switched on in `m` — or "" if there is none.
std::string gpus_conflict(int argc, const char* const* argv);
std::string gpus_conflict(const ModuleSettings& m);
// A module that is off contributes nothing to what identifies a context: its parameters as nobody had given them.  sites, regions:
// whether the file named any on this job's header (a list that maps to nothing switches the module off).
ModuleSettings settings_in_use(ModuleSettings m, bool sites, bool regions);
} // namespace bqc_cli
