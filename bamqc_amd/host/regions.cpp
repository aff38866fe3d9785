// regions.cpp — the BED file of --regions (include/bamqc_host.h: bqc_regions_load): text lines CONTIG<TAB>START<TAB>END[<TAB>anything],
// START counted from 0 and END exclusive.  Host code, no GPU.
#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/bamqc.h"
#include "../../include/bamqc_host.h"

namespace {
int regions_fail(char* err, uint64_t cap, const char* fmt, ...)
{
    if (err && cap) {
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(err, (size_t)cap, fmt, ap);
        va_end(ap);
    }
    return BQC_ERR_IO;
}
struct Region {
    int32_t rid, start, end;
};
// a number of digits alone up to the next tab or the line's end (false: none); values past 2^40 stay past it
bool number(const char* p, uint64_t& v, const char*& behind)
{
    const char* q = p;
    v = 0;
    for (; *q >= '0' && *q <= '9'; ++q)
        if (v < 1ull << 40) v = v * 10 + (uint64_t)(*q - '0');
    behind = q;
    return q != p && (!*q || *q == '\t');
}
} // namespace

extern "C" int bqc_regions_load(const char* path, const char* const* ref_names, const uint32_t* ref_lens, uint32_t n_refs, uint32_t* n_regions, int32_t** rid,
                                int32_t** start, int32_t** end, uint64_t* n_given, uint64_t* n_unnamed, uint64_t* n_merged, char* err, uint64_t err_cap)
{
    if (err && err_cap) err[0] = 0;
    if (!path || (!ref_names && n_refs) || (!ref_lens && n_refs) || !n_regions || !rid || !start || !end) return BQC_ERR_ARG;
    *n_regions = 0; *rid = nullptr; *start = nullptr; *end = nullptr;
    if (n_given) *n_given = 0;
    if (n_unnamed) *n_unnamed = 0;
    if (n_merged) *n_merged = 0;
    FILE* f = fopen(path, "rb");
    if (!f) return regions_fail(err, err_cap, "%s: the file could not be opened", path);
    std::unordered_map<std::string, uint32_t> index;
    for (uint32_t r = 0; r < n_refs; ++r) index.emplace(ref_names[r] ? ref_names[r] : "", r); // (a name given twice: the first contig of that name)
    std::vector<Region> regs;
    uint64_t given = 0, unnamed = 0, line_no = 0;
    char* line = nullptr;
    size_t cap = 0;
    ssize_t len;
    int rc = 0;
    while ((len = getline(&line, &cap, f)) >= 0) {
        ++line_no;
        while (len && (line[len - 1] == '\n' || line[len - 1] == '\r')) --len;
        line[len] = 0;
        if (!len || line[0] == '#') continue;
        if ((!strncmp(line, "track", 5) && (!line[5] || line[5] == ' ' || line[5] == '\t')) || (!strncmp(line, "browser", 7) && (!line[7] || line[7] == ' ' || line[7] == '\t'))) continue;
        char* tab = (char*)memchr(line, '\t', (size_t)len);
        if (!tab) { rc = regions_fail(err, err_cap, "%s: line %llu: no tab between the contig and the start", path, (unsigned long long)line_no); break; }
        uint64_t s = 0, e = 0;
        const char *p = tab + 1, *q = nullptr;
        if (!number(p, s, q)) {
            const std::string field(p, strcspn(p, "\t"));
            rc = regions_fail(err, err_cap, "%s: line %llu: the start '%s' is not a number", path, (unsigned long long)line_no, field.c_str());
            break;
        }
        if (*q != '\t') { rc = regions_fail(err, err_cap, "%s: line %llu: no tab between the start and the end", path, (unsigned long long)line_no); break; }
        p = q + 1;
        if (!number(p, e, q)) {
            const std::string field(p, strcspn(p, "\t"));
            rc = regions_fail(err, err_cap, "%s: line %llu: the end '%s' is not a number", path, (unsigned long long)line_no, field.c_str());
            break;
        }
        if (e <= s) {
            rc = regions_fail(err, err_cap, "%s: line %llu: the end %llu does not lie behind the start %llu", path, (unsigned long long)line_no, (unsigned long long)e, (unsigned long long)s);
            break;
        }
        ++given;
        const auto it = index.find(std::string(line, (size_t)(tab - line)));
        if (it == index.end()) { ++unnamed; continue; }
        if (e > ref_lens[it->second]) {
            rc = regions_fail(err, err_cap, "%s: line %llu: end %llu lies behind the end of contig %s (%u bases)", path, (unsigned long long)line_no, (unsigned long long)e,
                              ref_names[it->second], ref_lens[it->second]);
            break;
        }
        if (e > 0x7FFFFFFFull) {
            rc = regions_fail(err, err_cap, "%s: line %llu: end %llu is more than 2147483647", path, (unsigned long long)line_no, (unsigned long long)e);
            break;
        }
        regs.push_back(Region{(int32_t)it->second, (int32_t)s, (int32_t)e});
    }
    free(line);
    const bool read_error = ferror(f) != 0;
    fclose(f);
    if (rc) return rc;
    if (read_error) return regions_fail(err, err_cap, "%s: the file could not be read", path);
    std::sort(regs.begin(), regs.end(), [](const Region& a, const Region& b) { return a.rid != b.rid ? a.rid < b.rid : a.start != b.start ? a.start < b.start : a.end < b.end; });
    uint64_t merged = 0;
    size_t n = 0;
    for (size_t i = 0; i < regs.size(); ++i) { // regions of one contig that overlap or abut become one
        if (n && regs[n - 1].rid == regs[i].rid && regs[i].start <= regs[n - 1].end) {
            regs[n - 1].end = std::max(regs[n - 1].end, regs[i].end);
            ++merged;
        } else regs[n++] = regs[i];
    }
    regs.resize(n);
    if (n_given) *n_given = given;
    if (n_unnamed) *n_unnamed = unnamed;
    if (n_merged) *n_merged = merged;
    if (regs.empty()) {
        if (given) return regions_fail(err, err_cap, "%s: line %llu: no region left: all %llu regions lie on contigs the header does not name", path, (unsigned long long)line_no, (unsigned long long)given);
        return regions_fail(err, err_cap, "%s: line %llu: no region left: the file holds none", path, (unsigned long long)line_no);
    }
    if (regs.size() > 0xFFFFFFFFull) return regions_fail(err, err_cap, "%s: more than 4294967295 regions", path);
    int32_t* r = (int32_t*)malloc(n * sizeof(int32_t));
    int32_t* s = (int32_t*)malloc(n * sizeof(int32_t));
    int32_t* e = (int32_t*)malloc(n * sizeof(int32_t));
    if (!r || !s || !e) { free(r); free(s); free(e); return regions_fail(err, err_cap, "%s: out of memory for %llu regions", path, (unsigned long long)n); }
    for (size_t i = 0; i < n; ++i) { r[i] = regs[i].rid; s[i] = regs[i].start; e[i] = regs[i].end; }
    *n_regions = (uint32_t)n;
    *rid = r;
    *start = s;
    *end = e;
    return 0;
}

extern "C" void bqc_regions_free(int32_t* rid, int32_t* start, int32_t* end)
{
    free(rid);
    free(start);
    free(end);
}
