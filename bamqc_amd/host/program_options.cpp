// program_options.cpp — the table of the program's options, and what reads it: the parser, the help text, "not with --gpus" and the
// settings a context is identified by.  Adding an option is adding a row.
#include "program_options.h"

#include <algorithm>
#include <cstring>
#include <set>

#include "input_route.h"
#include "../csrc/adapter_rule.h"

namespace bqc_cli {
namespace {
const char* kVersion = "dev"; // src/version.h:12

// ---- the optional modules, in the order their files are written
enum Module : uint8_t { M_NONE, M_QBC, M_MBC, M_ADP, M_GCB, M_IBC, M_SBC, M_SAC, M_RCV, M_DUP, M_OVR, M_WDP, N_MODULES };
using Word = uint64_t ModuleSettings::*;
struct ModuleRow {
    const char* option;                // the module's own option
    Word on;                           // the word that says whether it runs,
    uint64_t on_default;               // and what the module's option alone sets it to (an option that writes the word itself comes first)
    std::string ProgramOptions::* file; // or: it runs when this FILE was named
    const char* needs;                 // what an option that needs the module is told it needs
    // not with --gpus: why, and the spelling the module's parameter options begin with (an argument that is the module's option, or
    // begins like this, asks for the module)
    const char *not_with_gpus, *gpus_prefix;
};
using MS = ModuleSettings;
const ModuleRow kModules[N_MODULES] = {
    {},
    {"--qual-by-cycle", &MS::qual_by_cycle, 1024, nullptr, nullptr, nullptr, nullptr},
    {"--mismatch-by-cycle", &MS::mismatch_by_cycle, 1024, nullptr, nullptr, nullptr, nullptr},
    {"--adapter-by-cycle", &MS::adapter_by_cycle, 1024, nullptr, nullptr, nullptr, nullptr},
    {"--gc-bias", &MS::gc_bias, 100, nullptr, nullptr, "no worker holds the whole genome (run one process)", "--gc-bias-window"},
    {"--indel-by-cycle", &MS::indel_by_cycle, 1024, nullptr, nullptr, nullptr, nullptr},
    {"--substitutions", &MS::substitutions, 1024, nullptr, nullptr, nullptr, nullptr},
    {"--site-alleles", &MS::site_alleles, 1, &ProgramOptions::site_alleles, "--site-alleles FILE (the sites it applies to)", nullptr, nullptr},
    {"--regions", &MS::regions, 1, &ProgramOptions::regions, "--regions FILE (the regions it applies to)", nullptr, nullptr},
    {"--duplicate-sets", &MS::duplicate_sets, 1, nullptr, "--duplicate-sets (the table it sizes)", "a set may have members in two workers' shards (run one process)", "--duplicate-sets-capacity"},
    {"--overrepresented", &MS::overrepresented, 1, nullptr, nullptr, "a set may have members in two workers' shards (run one process)", "--overrepresented"},
    {"--window-depth", &MS::window_depth, 1, nullptr, nullptr, nullptr, nullptr},
};

// ---- the options
enum Kind : uint8_t { FLAG, NUMBER, TEXT, CUSTOM };
enum Dep : uint8_t { ALONE, IMPLIES, NEEDS }; // giving the option switches its module on / is an error unless the module's own option is given
typedef bool (*CustomParser)(ProgramOptions& o, const std::string& v, std::string& err); // false: err
struct OptionRow {
    const char *name, *alias; // (alias: the reference's one-letter form)
    Kind kind;
    Module module;
    Dep dep;
    bool ProgramOptions::* flag;        // FLAG: set (none: the option is its module's own, which IMPLIES the module)
    std::string ProgramOptions::* text; // TEXT: the value as given
    CustomParser custom;                // CUSTOM
    // NUMBER: lo <= value <= hi in at most max_chars characters (0: any number of them — the older options take leading zeros without
    // end), or "the given value 'V' is not <noun> (<name> wants <range>)"
    Word number;
    uint64_t lo, hi;
    unsigned max_chars;
    const char *noun, *range;
    const char* help; // the option's paragraph of the help text (none: it is named in the text's fixed head)
};
OptionRow flag_row(const char* name, Module m, bool ProgramOptions::* f, const char* help) { return OptionRow{name, nullptr, FLAG, m, m ? IMPLIES : ALONE, f,nullptr, nullptr, nullptr, 0, 0, 0, nullptr, nullptr, help}; }
OptionRow text_row(const char* name, const char* alias, Module m, std::string ProgramOptions::* t, const char* help) { return OptionRow{name, alias, TEXT, m, ALONE, nullptr, t, nullptr, nullptr, 0, 0, 0, nullptr, nullptr, help}; }
OptionRow custom_row(const char* name, const char* alias, Module m, Dep dep, CustomParser p, const char* help) { return OptionRow{name, alias, CUSTOM, m, dep, nullptr, nullptr, p, nullptr, 0, 0, 0, nullptr, nullptr, help}; }
OptionRow number_row(const char* name, Module m, Dep dep, Word w, uint64_t lo, uint64_t hi, unsigned max_chars, const char* noun, const char* range, const char* help) { return OptionRow{name, nullptr, NUMBER, m, dep, nullptr, nullptr, nullptr, w, lo, hi, max_chars, noun, range, help}; }

// The one rule of a bounded number: decimal digits from the first character on, nothing behind them, within the bounds (a number too
// large for 64 bits is beyond every bound).
bool bounded_number(const std::string& v, uint64_t lo, uint64_t hi, unsigned max_chars, uint64_t& x)
{
    if (v.empty() || v[0] < '0' || v[0] > '9' || (max_chars && v.size() > max_chars)) return false;
    char* end = nullptr;
    const unsigned long long y = strtoull(v.c_str(), &end, 10);
    if (*end || y < lo || y > hi) return false;
    x = y;
    return true;
}

// the options with rules of their own
bool parse_insert_size(ProgramOptions& o, const std::string& v, std::string& err)
{
    char* end = nullptr;
    const long x = strtol(v.c_str(), &end, 10);
    if (!end || *end || v.empty()) { err = "bamqualcheck: the given value '" + v + "' cannot be casted to integer"; return false; }
    o.isize = (int)x;
    return true;
}
bool parse_error_rate(ProgramOptions& o, const std::string& v, std::string& err)
{
    char* end = nullptr;
    o.e = strtod(v.c_str(), &end);
    if (!end || *end || v.empty()) { err = "bamqualcheck: the given value '" + v + "' cannot be casted to double"; return false; }
    if (o.e < 0) { err = "bamqualcheck: the given value '" + v + "' is smaller than the minimum value of 0"; return false; }
    return true;
}
template <int ProgramOptions::* F> bool parse_atoi(ProgramOptions& o, const std::string& v, std::string&) { o.*F = atoi(v.c_str()); return true; } // (whatever it makes of the value)
template <uint32_t ProgramOptions::* F> bool parse_strtoul(ProgramOptions& o, const std::string& v, std::string&) { o.*F = (uint32_t)strtoul(v.c_str(), nullptr, 10); return true; }
bool parse_adapter(ProgramOptions& o, const std::string& v, std::string& err)
{
    const size_t eq = v.find('=');
    if (eq == std::string::npos) { err = "bamqualcheck: the given value '" + v + "' is not an adapter (--adapter wants NAME=SEQ)"; return false; }
    const std::string nm = v.substr(0, eq), sq = v.substr(eq + 1);
    const std::string fault = bqc_adapter_fault(nm.c_str(), sq.c_str());
    if (!fault.empty()) { err = "bamqualcheck: --adapter " + v + ": " + fault; return false; }
    for (const auto& ad : o.adapters)
        if (ad.first == nm) { err = "bamqualcheck: --adapter " + v + ": the adapter name '" + nm + "' is given twice"; return false; }
    if (o.adapters.size() == 8) { err = "bamqualcheck: --adapter " + v + ": at most 8 adapters are taken"; return false; }
    o.adapters.emplace_back(nm, sq);
    return true;
}
bool parse_regions_thresholds(ProgramOptions& o, const std::string& v, std::string& err)
{
    uint64_t t[8] = {}, n = 0;
    bool ok = !v.empty();
    for (size_t at = 0; ok && at <= v.size();) {
        const size_t comma = std::min(v.find(',', at), v.size());
        uint64_t x = 0;
        ok = n < 8 && bounded_number(v.substr(at, comma - at), 1, 0xFFFFFFFFull, 10, x) && (n == 0 || x > t[n - 1]);
        if (ok) t[n++] = x;
        at = comma + 1;
    }
    if (!ok) {
        err = "bamqualcheck: the given value '" + v + "' is not a list of depths (--regions-thresholds wants up to 8 increasing numbers of 1 to 4294967295, separated by commas)";
        return false;
    }
    o.mod.n_regions_thresholds = n;
    std::copy(t, t + 8, o.mod.regions_thresholds);
    return true;
}

const char* const kCycles = "a number of cycles";
const char* const kBaseQual = "a base quality";
const char* const kMapq = "a mapping quality";
const OptionRow kOptions[] = {
    // the reference's options, and the extensions that size the run: named in the head of the help text
    text_row("--reference", "-r", M_NONE, &ProgramOptions::referenceFile, nullptr),
    text_row("--output-file", "-o", M_NONE, &ProgramOptions::outputFile, nullptr),
    text_row("--chromosomes", "-c", M_NONE, &ProgramOptions::chroms, nullptr),
    custom_row("--insert-size", "-i", M_NONE, ALONE, parse_insert_size, nullptr),
    text_row("--kmer-size", "-k", M_NONE, &ProgramOptions::kmer_sizes, nullptr),
    text_row("--quality-cutoff", "-q", M_NONE, &ProgramOptions::quality_cutoffs, nullptr),
    custom_row("--error-rate", "-e", M_NONE, ALONE, parse_error_rate, nullptr),
    custom_row("--seed", "-s", M_NONE, ALONE, parse_atoi<&ProgramOptions::seed>, nullptr),
    custom_row("--device", nullptr, M_NONE, ALONE, parse_atoi<&ProgramOptions::device>, nullptr),
    custom_row("--max-read-len", nullptr, M_NONE, ALONE, parse_strtoul<&ProgramOptions::max_read_len>, nullptr),
    custom_row("--hist-cap", nullptr, M_NONE, ALONE, parse_strtoul<&ProgramOptions::hist_cap>, nullptr),
    custom_row("--batch-reads", nullptr, M_NONE, ALONE, parse_strtoul<&ProgramOptions::batch_reads>, nullptr),
    flag_row("--no-sketch", M_NONE, &ProgramOptions::no_sketch, nullptr),
    // the modules
    flag_row("--qual-by-cycle", M_QBC, nullptr, "    --qual-by-cycle\n          Per-cycle base quality histograms (read group x mate x cycle x Phred value) into OUT.qbc,\n"
             "          for the first 1024 cycles of every read.\n"),
    number_row("--qual-by-cycle-len", M_QBC, IMPLIES, &MS::qual_by_cycle, 1, 0x3FFFFFFF, 0, kCycles, "1 or more", "    --qual-by-cycle-len INT\n          The same for the first INT cycles (at least 1, at most --max-read-len).\n"),
    flag_row("--mismatch-by-cycle", M_MBC, nullptr, "    --mismatch-by-cycle\n          Bases compared with the reference genome, and those that differ from it (read group x mate x\n"
             "          cycle x Phred value), into OUT.mbc, for the first 1024 cycles of every read.\n"),
    number_row("--mismatch-by-cycle-len", M_MBC, IMPLIES, &MS::mismatch_by_cycle, 1, 0x3FFFFFFF, 0, kCycles, "1 or more", "    --mismatch-by-cycle-len INT\n          The same for the first INT cycles (at least 1, at most --max-read-len).\n"),
    flag_row("--adapter-by-cycle", M_ADP, nullptr, "    --adapter-by-cycle\n          Adapter content by cycle: per read group, mate and adapter the reads whose first occurrence of the\n"
             "          adapter starts at each cycle, and the reads by length, into OUT.adp, for the first 1024 cycles.\n"),
    number_row("--adapter-by-cycle-len", M_ADP, IMPLIES, &MS::adapter_by_cycle, 1, 0x3FFFFFFF, 0, kCycles, "1 or more", "    --adapter-by-cycle-len INT\n          The same for the first INT cycles (at least 1, at most --max-read-len).\n"),
    custom_row("--adapter", nullptr, M_ADP, IMPLIES, parse_adapter, "    --adapter NAME=SEQ\n          An adapter to look for (repeatable, at most 8; the first one replaces the built-in set): NAME is 1 to 31\n"
               "          characters of [A-Za-z0-9_.-], SEQ 8 to 16 letters of ACGT.  Implies --adapter-by-cycle.\n"),
    flag_row("--gc-bias", M_GCB, nullptr, "    --gc-bias\n          GC bias: the genome's windows of 100 bases by GC bin, and per read group the reads that start in a\n"
             "          window of each bin, their bases and the sum of their base qualities, into OUT.gcb.  Not with --gpus.\n"),
    number_row("--gc-bias-window", M_GCB, IMPLIES, &MS::gc_bias, 20, 1000, 0, "a window length", "20 to 1000", "    --gc-bias-window INT\n          The same for windows of INT bases (at least 20, at most 1000).  Implies --gc-bias.\n"),
    flag_row("--indel-by-cycle", M_IBC, nullptr, "    --indel-by-cycle\n          Insertions and deletions by cycle (read group x mate x the first 1024 cycles) and by length (1 to 64\n"
             "          and more), with the reads by length they are rates of, into OUT.ibc.\n"),
    number_row("--indel-by-cycle-len", M_IBC, IMPLIES, &MS::indel_by_cycle, 1, 0x3FFFFFFF, 0, kCycles, "1 or more", "    --indel-by-cycle-len INT\n          The same for the first INT cycles (at least 1, at most --max-read-len).  Implies --indel-by-cycle.\n"),
    flag_row("--substitutions", M_SBC, nullptr, "    --substitutions\n          Substitutions as sequenced: the pairs (genome base, read base) by trinucleotide context, per read group,\n"
             "          mate and strand, and by cycle (the first 1024), over bases of quality 20 and more in reads of mapping\n"
             "          quality 30 and more, into OUT.sbc (oxidation, deamination and strand artefacts are folds of it).\n"),
    number_row("--substitutions-len", M_SBC, IMPLIES, &MS::substitutions, 1, 0x7FFFFFF, 0, kCycles, "1 or more", // (its table's cycle axis is narrower)
               "    --substitutions-len INT\n          The same for the first INT cycles (at least 1, at most --max-read-len).  Implies --substitutions.\n"),
    number_row("--substitutions-min-qual", M_SBC, IMPLIES, &MS::subst_min_qual, 0, 222, 0, kBaseQual, "0 to 222", "    --substitutions-min-qual INT\n          The same over bases of quality INT and more (0 to 222).  Implies --substitutions.\n"),
    number_row("--substitutions-min-mapq", M_SBC, IMPLIES, &MS::subst_min_mapq, 0, 255, 0, kMapq, "0 to 255", "    --substitutions-min-mapq INT\n          The same over reads of mapping quality INT and more (0 to 255).  Implies --substitutions.\n"),
    text_row("--site-alleles", nullptr, M_SAC, &ProgramOptions::site_alleles, "    --site-alleles FILE\n          Allele counts at given sites: per read group and site of FILE (lines CONTIG<TAB>POS, POS counted from 1,\n"
             "          as the body lines of a VCF are), the reads that show A, C, G and T there, by strand, over bases of quality\n"
             "          20 and more in reads of mapping quality 20 and more, into OUT.sac (fingerprint, lane swap and\n"
             "          contamination checks are folds of it).\n"),
    number_row("--site-alleles-min-qual", M_SAC, NEEDS, &MS::site_min_qual, 0, 222, 0, kBaseQual, "0 to 222", "    --site-alleles-min-qual INT\n          The same over bases of quality INT and more (0 to 222).  Needs --site-alleles.\n"),
    number_row("--site-alleles-min-mapq", M_SAC, NEEDS, &MS::site_min_mapq, 0, 255, 0, kMapq, "0 to 255", "    --site-alleles-min-mapq INT\n          The same over reads of mapping quality INT and more (0 to 255).  Needs --site-alleles.\n"),
    text_row("--regions", nullptr, M_RCV, &ProgramOptions::regions, "    --regions FILE\n          Depth over given regions: FILE is a BED file (lines CONTIG<TAB>START<TAB>END, START counted from 0, END\n"
             "          exclusive; regions that overlap or abut are merged).  Per read group the reads and aligned bases on the\n"
             "          regions, a histogram of the depth over their bases and per region the depth's sum, minimum and maximum\n"
             "          and the bases at depth 1, 10, 20, 30, 50 and 100 or more, over reads of mapping quality 20 and more,\n"
             "          into OUT.rcv (on-target rate, mean target depth, fold-80 and the list of gaps are folds of it).\n"),
    number_row("--regions-min-mapq", M_RCV, NEEDS, &MS::regions_min_mapq, 0, 255, 0, kMapq, "0 to 255", "    --regions-min-mapq INT\n          The same over reads of mapping quality INT and more (0 to 255).  Needs --regions.\n"),
    custom_row("--regions-thresholds", nullptr, M_RCV, NEEDS, parse_regions_thresholds, "    --regions-thresholds LIST\n          The same with the depths of LIST: up to 8 numbers of 1 to 4294967295, increasing, separated by\n"
               "          commas.  Needs --regions.\n"),
    number_row("--regions-depth-cap", M_RCV, NEEDS, &MS::regions_depth_cap, 1, 16383, 0, "a histogram cap", "1 to 16383", "    --regions-depth-cap INT\n          The histogram's last bin: depth INT and more (1 to 16383, default 1000).  Needs --regions.\n"),
    flag_row("--duplicate-sets", M_DUP, nullptr, "    --duplicate-sets\n          Duplicate sets: reads of equal alignment signature (class, strands, contig, unclipped 5' position and\n"
             "          template length) are one set.  Per read group the examined and the flagged (0x400) reads, over all read\n"
             "          groups the sets, the largest set, the sets by size and the estimated library size, into OUT.dup (the\n"
             "          duplication rate and observed against flagged duplicates are folds of it).  Not with --gpus.\n"),
    number_row("--duplicate-sets-capacity", M_DUP, NEEDS, &MS::duplicate_sets_capacity, 16, 1ull << 31, 10, "a number of signatures", "16 to 2147483648", "    --duplicate-sets-capacity INT\n          The different signatures the table takes (16 to 2147483648, default 67108864: 3 GiB on the card).\n"
               "          Needs --duplicate-sets.\n"),
    flag_row("--overrepresented", M_OVR, nullptr, "    --overrepresented\n          Overrepresented sequences: reads whose first 50 bases as sequenced (a reverse read's last stored bases,\n"
             "          reverse-complemented) are equal, of the same mate, are one set; unmapped reads count, reads with a base\n"
             "          other than A, C, G, T among them are skipped.  Per read group the examined and the skipped reads, per mate\n"
             "          over all read groups the sets, the largest set, the sets by size and every sequence that makes up 1000 reads\n"
             "          per million or more (at least 2 reads) with its count and the built-in adapter it contains, into OUT.ovr\n"
             "          (duplication by sequence and contaminant spotting are folds of it).  Not with --gpus.\n"),
    number_row("--overrepresented-len", M_OVR, IMPLIES, &MS::overrepresented_len, 20, 56, 10, "a prefix length", "20 to 56", "    --overrepresented-len INT\n          The same for the first INT bases (20 to 56).  Implies --overrepresented.\n"),
    number_row("--overrepresented-ppm", M_OVR, IMPLIES, &MS::overrepresented_ppm, 10, 1000000, 10, "a number of reads per million", "10 to 1000000", "    --overrepresented-ppm INT\n          The same listing sequences of INT reads per million or more (10 to 1000000).  Implies --overrepresented.\n"),
    number_row("--overrepresented-capacity", M_OVR, IMPLIES, &MS::overrepresented_capacity, 16, 1ull << 31, 10, "a number of sequences", "16 to 2147483648", "    --overrepresented-capacity INT\n          The different sequences the table takes (16 to 2147483648, default 67108864: 3 GiB on the card).\n"
               "          Implies --overrepresented.\n"),
    flag_row("--window-depth", M_WDP, nullptr, "    --window-depth\n          Depth in fixed genome windows of 1000 bases over every contig of the header: per read group and window\n"
             "          the reads that begin in it and the covered bases of reads of mapping quality 20 and more, the covered bases\n"
             "          of the reads below it, the same summed by contig, and a histogram of the main contigs' window depths, into\n"
             "          OUT.wdp (sex and aneuploidy checks, the share of reads off the main contigs and coverage evenness are\n"
             "          folds of it).\n"),
    number_row("--window-depth-size", M_WDP, IMPLIES, &MS::window_depth_size, 100, 1ull << 24, 10, "a window size", "100 to 16777216", "    --window-depth-size INT\n          The same in windows of INT bases (100 to 16777216).  Implies --window-depth.\n"),
    number_row("--window-depth-min-mapq", M_WDP, IMPLIES, &MS::window_depth_min_mapq, 0, 255, 10, kMapq, "0 to 255", "    --window-depth-min-mapq INT\n          The same with mapping quality INT as the border between the two classes (0 to 255).  Implies\n"
               "          --window-depth.\n"),
    text_row("--manifest", nullptr, M_NONE, &ProgramOptions::manifest, "    --manifest LIST\n          Many files, one resident worker: LIST holds INPUT<TAB>OUTPUT per line (instead of BAMFILE and -o).\n"
             "          With a list (only then), \"{dir}\" in the reference's filename stands for the directory of each\n"
             "          job's input; in a single run the filename is taken as it is.\n"),
};
const size_t kOptionCount = sizeof kOptions / sizeof kOptions[0];

// the row `key` names (kOptionCount for an unknown key)
size_t find_option(const std::string& key) { return std::find_if(kOptions, kOptions + kOptionCount, [&](const OptionRow& r) { return key == r.name || (r.alias && key == r.alias); }) - kOptions; }
} // namespace

bool ModuleSettings::operator==(const ModuleSettings& o) const { return memcmp(this, &o, sizeof o) == 0; }

void usage(FILE* f)
{
    fputs("bamqualcheck - String Modifier\n==============================\n\nSYNOPSIS\n    bamqualcheck [OPTIONS] BAMFILE\n\n"
          "DESCRIPTION\n    Program for bam quality checks. The program can read from bamfile or stdin(sam format)\n\n"
          "    -h, --help\n          Displays this help message.\n    --version\n          Display version information\n\n"
          "  General options:\n    -r, --reference FILENAME\n          Reference genome filename. Default: genome.fa.\n"
          "    -i, --insert-size INT\n          Upper bound for the insert size in insert size histogram. Default: 1000.\n"
          "    -c, --chromosomes STRING\n          Comma separated list of the main chromosome names.\n"
          "    -o, --output-file OUT\n          Output filename.\n\n"
          "  Kmerstream options:\n    -k, --kmer-size STRING\n          Comma-separated list of k-mer sizes. Default: 32.\n"
          "    -q, --quality-cutoff STRING\n          Comma-separated list of PHRED quality thresholds. Default: 17.\n"
          "    -e, --error-rate DOUBLE\n          Error rate guaranteed. Default: 0.01.\n"
          "    -s, --seed INT\n          Seed value for the randomness. Default: 1.\n\n"
          "  MI355X options (not in the reference):\n    --device INT, --max-read-len INT, --hist-cap INT, --batch-reads INT, --no-sketch\n",
          f);
    for (const OptionRow& row : kOptions)
        if (row.help) fputs(row.help, f);
    fprintf(f, "\nVERSION\n    bamqualcheck version: %s\n    Last update August 2019\n", kVersion);
}

bool input_extension_ok(const std::string& path, std::string& err)
{
    // (input_kind: ".sam.gz" is two extensions, and a pipe has no name to speak of — /dev/stdin, /dev/fd/N, a process substitution)
    const InputKind k = input_kind(path.c_str());
    if (k == IN_OTHER || k == IN_STDIN) { err = "bamqualcheck: the given path '" + path + "' does not have one of the valid file extensions [*.-, *.bam, *.sam, *.sam.gz]"; return false; }
    return true;
}

// --manifest LIST: one job per line, INPUT<TAB>OUTPUT; empty lines and lines that start with '#' are skipped, a '\r' in front of the
// '\n' is dropped.  Everything that is wrong with the list is found here, before any job runs or any output file is touched.
bool read_manifest(const std::string& path, std::vector<std::pair<std::string, std::string>>& jobs, std::string& err)
{
    std::string text;
    {
        FILE* f = fopen(path.c_str(), "rb");
        if (!f) { err = "bamqualcheck: the manifest '" + path + "' cannot be read"; return false; }
        char buf[1 << 16];
        size_t n;
        while ((n = fread(buf, 1, sizeof buf, f)) > 0) text.append(buf, n);
        const bool bad = ferror(f) != 0;
        fclose(f);
        if (bad) { err = "bamqualcheck: the manifest '" + path + "' cannot be read"; return false; }
    }
    std::set<std::string> outputs;
    size_t line_no = 0;
    for (size_t p = 0; p < text.size();) {
        size_t e = text.find('\n', p);
        if (e == std::string::npos) e = text.size();
        std::string line = text.substr(p, e - p);
        p = e + 1;
        ++line_no;
        if (!line.empty() && line.back() == '\r') line.pop_back();
        if (line.empty() || line[0] == '#') continue;
        const std::string where = "bamqualcheck: manifest '" + path + "' line " + std::to_string(line_no) + ": ";
        const size_t tab = line.find('\t');
        if (tab == std::string::npos || line.find('\t', tab + 1) != std::string::npos || tab == 0 || tab + 1 == line.size()) { err = where + "expected INPUT<TAB>OUTPUT"; return false; }
        const std::string in = line.substr(0, tab), out = line.substr(tab + 1);
        if (in == "-") { err = where + "a stream on stdin is not a job"; return false; }
        std::string xerr;
        if (!input_extension_ok(in, xerr)) { err = where + xerr.substr(strlen("bamqualcheck: ")); return false; }
        if (!outputs.insert(out).second) { err = where + "the output '" + out + "' is named twice"; return false; }
        jobs.emplace_back(in, out);
    }
    if (jobs.empty()) { err = "bamqualcheck: the manifest '" + path + "' names no job"; return false; }
    return true;
}

static std::string gpus_message(const ModuleRow& m) { return std::string("bamqualcheck: ") + m.option + " with --gpus is not supported: " + m.not_with_gpus; }
std::string gpus_conflict(int argc, const char* const* argv)
{
    for (const ModuleRow& m : kModules) {
        if (!m.not_with_gpus) continue;
        for (int k = 1; k < argc; ++k)
            if (strcmp(argv[k], m.option) == 0 || strncmp(argv[k], m.gpus_prefix, strlen(m.gpus_prefix)) == 0) return gpus_message(m);
    }
    return std::string();
}
std::string gpus_conflict(const ModuleSettings& s)
{
    for (const ModuleRow& m : kModules)
        if (m.not_with_gpus && s.*(m.on)) return gpus_message(m);
    return std::string();
}

ModuleSettings settings_in_use(ModuleSettings s, bool sites, bool regions)
{
    const ModuleSettings unset;
    s.site_alleles = sites;
    s.regions = regions;
    for (const OptionRow& row : kOptions)
        if (row.kind == NUMBER && !(s.*(kModules[row.module].on))) s.*(row.number) = unset.*(row.number);
    if (!s.regions) { s.n_regions_thresholds = unset.n_regions_thresholds; std::copy(unset.regions_thresholds, unset.regions_thresholds + 8, s.regions_thresholds); }
    return s;
}

int parse_args(int argc, const char* const* argv, ProgramOptions& o, std::string& err, bool session_form)
{
    bool given[kOptionCount] = {}; // by row
    bool wanted[N_MODULES] = {};   // the module's own option, or one that implies it
    std::string needing[N_MODULES]; // the last option given that needs the module
    std::vector<std::string> pos;
    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        if (a == "-") { pos.push_back(a); continue; }
        if (a == "-h" || a == "--help") { usage(stdout); return 2; }
        if (a == "--version") { printf("bamqualcheck version: %s\nLast update August 2019\n", kVersion); return 2; }
        const char* inl = nullptr;
        std::string key = a;
        if (a.rfind("--", 0) == 0) {
            size_t eq = a.find('=');
            if (eq != std::string::npos) { key = a.substr(0, eq); inl = argv[i] + eq + 1; }
        } else if (a.size() > 2 && a[0] == '-') { // -ovalue
            key = a.substr(0, 2);
            inl = argv[i] + 2;
        }
        const size_t r = find_option(key);
        if (r == kOptionCount) {
            // (--gpus N is the front end's and never reaches this parser from it; given here, it is an illegal option — said in the
            // module's own terms where one is asked for as well that no worker of --gpus could compute)
            if (key == "--gpus" && !(err = gpus_conflict(argc, argv)).empty()) return 1;
            if (a[0] == '-') { err = "bamqualcheck: illegal option -- " + a.substr(a.rfind("--", 0) == 0 ? 2 : 1); return 1; }
            pos.push_back(a);
            continue;
        }
        const OptionRow& row = kOptions[r];
        given[r] = true;
        if (row.kind != FLAG && !inl && i + 1 >= argc) { err = "bamqualcheck: option requires an argument -- " + key; return 1; }
        const std::string v = row.kind == FLAG ? "" : inl ? inl : argv[++i];
        if (row.kind == FLAG) { if (row.flag) o.*(row.flag) = true; }
        else if (row.kind == TEXT) o.*(row.text) = v;
        else if (row.kind == CUSTOM) { if (!row.custom(o, v, err)) return 1; }
        else if (!bounded_number(v, row.lo, row.hi, row.max_chars, o.mod.*(row.number))) { err = "bamqualcheck: the given value '" + v + "' is not " + row.noun + " (" + row.name + " wants " + row.range + ")"; return 1; }
        if (row.dep == IMPLIES) wanted[row.module] = true;
        if (row.dep == NEEDS) needing[row.module] = key;
    }
    // the modules, once: which ones run, at their defaults unless an option has said otherwise; then what an option needed
    for (int m = M_NONE + 1; m < N_MODULES; ++m) {
        uint64_t& on = o.mod.*(kModules[m].on);
        if (kModules[m].file) on = !(o.*(kModules[m].file)).empty();
        else if (wanted[m] && !on) on = kModules[m].on_default;
    }
    for (int m = M_NONE + 1; m < N_MODULES; ++m)
        if (!needing[m].empty() && !(o.mod.*(kModules[m].on))) { err = "bamqualcheck: option " + needing[m] + " needs " + kModules[m].needs; return 1; }
    const bool have_r = given[find_option("-r")], have_o = given[find_option("-o")], have_m = given[find_option("--manifest")];
    if (!have_r) { err = "bamqualcheck: option requires an argument -- r (required option -r/--reference missing)"; return 1; }
    if (session_form) {
        if (have_o || have_m || !pos.empty()) { err = "bamqualcheck: a session takes the program's options without an input, -o and --manifest"; return 1; }
    } else if (have_m) {
        if (have_o) { err = "bamqualcheck: --manifest names every job's output: -o cannot be given with it"; return 1; }
        if (!pos.empty()) { err = "bamqualcheck: --manifest names every job's input: no BAMFILE can be given with it"; return 1; }
        if (!read_manifest(o.manifest, o.jobs, err)) return 1;
    } else {
        if (!have_o) { err = "bamqualcheck: option requires an argument -- o (required option -o/--output-file missing)"; return 1; }
        if (pos.size() != 1) { err = pos.empty() ? "bamqualcheck: Not enough arguments were provided." : "bamqualcheck: Too many arguments were provided!"; return 1; }
        o.bamFile = pos[0];
        if (o.bamFile != "-" && !input_extension_ok(o.bamFile, err)) return 1;
    }
    // comma separated lists, parsed like the reference's stringstream loops (:121-143)
    auto split_nums = [](const std::string& s, auto& out) {
        size_t p = 0;
        while (p < s.size()) {
            char* end = nullptr;
            long v = strtol(s.c_str() + p, &end, 10);
            if (end == s.c_str() + p) break;
            out.push_back((typename std::remove_reference<decltype(out)>::type::value_type)v);
            p = (size_t)(end - s.c_str());
            if (p < s.size() && s[p] == ',') ++p;
        }
    };
    split_nums(o.kmer_sizes, o.klist);
    split_nums(o.quality_cutoffs, o.q_cutoff);
    return 0;
}
} // namespace bqc_cli
