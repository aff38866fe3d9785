// Reads SAM text files through the host's code twice — SamReader on a FILE*, and from memory the way GpuSamReader does it for a short
// stream on stdin and for a batch handed over by the card (lines split at '\n' by sam_take_line, '@' lines to sam_header_line, record
// lines to SamLineParser::parse) — and prints records and result per file.  Built with -fsanitize=address,undefined by
// tools/asan_sam_text.sh, run on the files of tests/sam_sweeps.py and damaged copies of the wild one.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../bamqc_amd/host/bam_io.h"

static long from_file(FILE* f, std::string& err, int& code)
{
    SamReader rd;
    if (!rd.open(f, err)) return -1;
    HostBatch hb;
    long n = 0;
    for (;;) {
        const int rc = rd.next_batch(hb, 777, 1 << 20, err, code);
        if (rc < 0) return -1 - n;
        if (rc == 0) return n;
        n += (long)hb.n();
    }
}

static long from_memory(const std::vector<char>& text, std::string& err, int& code)
{
    BamHeader hdr;
    std::map<std::string, int32_t> ref_index;
    std::vector<uint8_t> main_chrom;
    uint64_t nrec = 0;
    std::string line;
    size_t at = 0;
    bool in_header = true;
    HostBatch hb;
    long n = 0;
    SamLineParser P{hdr, ref_index, main_chrom, nrec};
    while (at < text.size()) {
        const char* p = text.data() + at;
        const char* e = (const char*)memchr(p, '\n', text.size() - at);
        const size_t len = e ? (size_t)(e - p) : text.size() - at;
        at += len + (e ? 1 : 0);
        sam_take_line(p, len, e != nullptr, line);
        if (in_header && !line.empty() && line[0] == '@') { sam_header_line(line, hdr, ref_index); continue; }
        if (in_header && !line.empty()) { in_header = false; parse_read_groups(hdr); }
        if (hb.n() >= 777) { n += (long)hb.n(); hb.clear(); } // (batches as the reader's: an error drops the failing batch's records)
        if (P.parse(line, hb, err, code) < 0) return -1 - n;
    }
    return n + (long)hb.n();
}

int main(int argc, char** argv)
{
    int differ = 0;
    for (int a = 1; a < argc; ++a) {
        FILE* f = fopen(argv[a], "rb");
        if (!f) { printf("%s: cannot open\n", argv[a]); continue; }
        std::vector<char> text;
        char buf[1 << 16];
        for (size_t n; (n = fread(buf, 1, sizeof buf, f)) > 0;) text.insert(text.end(), buf, buf + n);
        rewind(f);
        std::string e1, e2;
        int c1 = 0, c2 = 0;
        const long n1 = from_file(f, e1, c1), n2 = from_memory(text, e2, c2);
        fclose(f);
        // (a NUL byte ends what fgets + strlen take of a line; from memory a line is what lies between two '\n': such files may differ)
        const bool has_nul = memchr(text.data(), 0, text.size()) != nullptr;
        if (!has_nul && (n1 != n2 || c1 != c2 || e1 != e2)) { ++differ; printf("%s: FILE* and memory differ: %ld / %ld, %s / %s\n", argv[a], n1, n2, e1.c_str(), e2.c_str()); }
        printf("%s: %ld records rc %d %s\n", argv[a], n1 < 0 ? -1 - n1 : n1, n1 < 0 ? c1 : 0, e1.c_str());
    }
    return differ ? 1 : 0;
}
