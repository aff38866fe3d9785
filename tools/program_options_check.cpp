// program_options_check.cpp — the command line's parser under the host sanitizers: a stand-alone program (no HIP, no Python) that feeds
// bamqc_amd/host/program_options.cpp the recorded matrix of tests/golden/program_options/cases.json and compares what the parser
// answers — return code, input path, message — with the recording.  Built by hand, run on the host, from the repository's root:
//
//   c++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -o /tmp/program_options_check \
//       tools/program_options_check.cpp bamqc_amd/host/program_options.cpp bamqc_amd/host/input_route.cpp
//   /tmp/program_options_check tests/golden/program_options/cases.json
//
// Exit status 0: every case answered as recorded and the sanitizers found nothing.
#include <unistd.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "../bamqc_amd/host/program_options.h"

// the JSON the recording uses: strings of ASCII with \" \\ \n \t \r, lists of strings, integers
static std::string json_string(const std::string& s, size_t& at)
{
    std::string out;
    for (++at; at < s.size() && s[at] != '"'; ++at) {
        if (s[at] != '\\') { out += s[at]; continue; }
        const char c = s[++at];
        out += c == 'n' ? '\n' : c == 't' ? '\t' : c == 'r' ? '\r' : c;
    }
    ++at;
    return out;
}
static size_t value_of(const std::string& line, const char* key)
{
    const size_t at = line.find(std::string("\"") + key + "\": ");
    if (at == std::string::npos) { fprintf(stderr, "no %s in: %s\n", key, line.c_str()); exit(2); }
    return at + strlen(key) + 4;
}

int main(int argc, char** argv)
{
    if (argc != 2) { fprintf(stderr, "usage: %s tests/golden/program_options/cases.json\n", argv[0]); return 2; }
    std::ifstream in(argv[1]);
    if (!in) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    char dir[] = "/tmp/program_options_check.XXXXXX"; // the lists of the --manifest cases, by relative name
    if (!mkdtemp(dir) || chdir(dir) != 0) { perror(dir); return 2; }
    std::vector<std::string> made;
    if (!freopen("/dev/null", "w", stdout)) return 2; // (help and version, which the parser prints itself)
    size_t n = 0, wrong = 0;
    for (std::string line; std::getline(in, line);) {
        if (line.compare(0, 10, "{\"files\": ") == 0) {
            for (size_t at = line.find('{', 1) + 1; line[at] == '"';) {
                const std::string name = json_string(line, at);
                at += 2; // ": "
                const std::string text = json_string(line, at);
                std::ofstream(name) << text;
                made.push_back(name);
                if (line[at] == ',') at += 2;
            }
            continue;
        }
        if (line.find("{\"entry\": ") == std::string::npos) continue;
        size_t at = value_of(line, "entry");
        const bool session = json_string(line, at) == "session";
        std::vector<std::string> args{"bamqualcheck"};
        for (at = value_of(line, "args") + 1; line[at] == '"';) {
            args.push_back(json_string(line, at));
            if (line[at] == ',') at += 2;
        }
        const int want_rc = atoi(line.c_str() + value_of(line, "rc"));
        at = value_of(line, "path");
        const std::string want_path = json_string(line, at);
        at = value_of(line, "stderr");
        const std::string want_err = json_string(line, at);
        std::vector<const char*> av;
        for (const std::string& a : args) av.push_back(a.c_str());
        bqc_cli::ProgramOptions o;
        std::string err;
        const int pr = bqc_cli::parse_args((int)av.size(), av.data(), o, err, session);
        // (what bqc_program_args and bqc_session_open make of the parser's answer)
        const int rc = session ? pr != 0 : pr;
        const std::string path = session ? "" : pr == 0 ? o.bamFile : "untouched", said = pr == 1 ? err + "\n" : "";
        (void)bqc_cli::gpus_conflict((int)av.size(), av.data());
        (void)bqc_cli::gpus_conflict(o.mod);
        (void)(bqc_cli::settings_in_use(o.mod, false, true) == bqc_cli::settings_in_use(o.mod, true, false));
        ++n;
        if (rc != want_rc || path != want_path || said != want_err) {
            if (++wrong <= 5) fprintf(stderr, "differs: %s\n  got  %d '%s' %s  want %d '%s' %s", line.c_str(), rc, path.c_str(), said.c_str(), want_rc, want_path.c_str(), want_err.c_str());
        }
    }
    bqc_cli::usage(stdout);
    // what the recording cannot show: the settings an accepted command line ends at, whatever the order of its options
    auto mod = [](std::vector<const char*> extra) {
        std::vector<const char*> av{"bamqualcheck", "-r", "g.fa", "-o", "x", "in.bam"};
        av.insert(av.end(), extra.begin(), extra.end());
        bqc_cli::ProgramOptions o;
        std::string err;
        if (bqc_cli::parse_args((int)av.size(), av.data(), o, err) != 0) { fprintf(stderr, "refused: %s\n", err.c_str()); exit(1); }
        return o.mod;
    };
    const bqc_cli::ModuleSettings off;
    auto expect = [&](bool ok, const char* what) { if (!ok) { fprintf(stderr, "settings: %s\n", what); ++wrong; } };
    expect(mod({}) == off && off.qual_by_cycle == 0 && off.regions == 0, "nothing given: every module off");
    expect(mod({"--qual-by-cycle"}).qual_by_cycle == 1024 && mod({"--qual-by-cycle-len", "300"}).qual_by_cycle == 300, "--qual-by-cycle, -len alone");
    expect(mod({"--qual-by-cycle-len", "300", "--qual-by-cycle"}) == mod({"--qual-by-cycle", "--qual-by-cycle-len=300"}) && mod({"--qual-by-cycle-len", "300", "--qual-by-cycle"}).qual_by_cycle == 300, "-len in front of the flag");
    expect(mod({"--adapter", "a=ACGTACGT"}).adapter_by_cycle == 1024 && mod({"--adapter", "a=ACGTACGT", "--adapter-by-cycle-len", "7"}).adapter_by_cycle == 7, "--adapter implies");
    expect(mod({"--gc-bias"}).gc_bias == 100 && mod({"--gc-bias-window", "50", "--gc-bias"}).gc_bias == 50, "--gc-bias");
    const bqc_cli::ModuleSettings sbc = mod({"--substitutions-min-qual", "5"});
    expect(sbc.substitutions == 1024 && sbc.subst_min_qual == 5 && sbc.subst_min_mapq == 30 && mod({"--substitutions-min-mapq=0", "--substitutions-len", "9"}).substitutions == 9, "--substitutions-min-* imply");
    const bqc_cli::ModuleSettings ovr = mod({"--overrepresented-capacity", "2147483648"});
    expect(ovr.overrepresented == 1 && ovr.overrepresented_capacity == 1ull << 31 && ovr.overrepresented_len == 50 && ovr.overrepresented_ppm == 1000, "--overrepresented-capacity implies");
    expect(mod({"--window-depth-min-mapq", "0"}).window_depth == 1 && mod({"--window-depth"}).window_depth_size == 1000 && mod({"--duplicate-sets", "--duplicate-sets-capacity=16"}).duplicate_sets_capacity == 16, "--window-depth, --duplicate-sets");
    const bqc_cli::ModuleSettings rcv = mod({"--regions-thresholds", "2,9", "--regions", "r.bed", "--regions-depth-cap", "7", "--site-alleles", "s.tsv", "--site-alleles-min-qual", "1"});
    expect(rcv.regions == 1 && rcv.n_regions_thresholds == 2 && rcv.regions_thresholds[1] == 9 && rcv.regions_thresholds[2] == 0 && rcv.regions_depth_cap == 7 && rcv.site_alleles == 1 && rcv.site_min_qual == 1, "--regions, --site-alleles");
    // a module that is off adds nothing to what identifies a context
    expect(bqc_cli::settings_in_use(rcv, false, false) == off, "lists that map to nothing: both modules off");
    expect(bqc_cli::settings_in_use(rcv, true, false).site_min_qual == 1 && bqc_cli::settings_in_use(rcv, true, false).regions_depth_cap == 1000 && bqc_cli::settings_in_use(rcv, false, true).n_regions_thresholds == 2, "one of the two off");
    expect(bqc_cli::settings_in_use(sbc, false, false) == sbc && !(sbc == off), "a module that is on keeps its settings");
    for (const std::string& name : made) unlink(name.c_str());
    if (chdir("/") == 0) rmdir(dir);
    fprintf(stderr, "%zu cases, %zu differ\n", n, wrong);
    return wrong || n == 0 ? 1 : 0;
}
