// sites.cpp — the sites file of --site-alleles (include/bamqc_host.h: bqc_sites_load): text lines CONTIG<TAB>POS[<TAB>anything], POS
// counted from 1, so the body lines of a VCF are such lines.  Host code, no GPU.
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
int sites_fail(char* err, uint64_t cap, const char* fmt, ...)
{
    if (err && cap) {
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(err, (size_t)cap, fmt, ap);
        va_end(ap);
    }
    return BQC_ERR_IO;
}
struct Site {
    int32_t rid, pos;
    uint64_t line;
};
} // namespace

extern "C" int bqc_sites_load(const char* path, const char* const* ref_names, const uint32_t* ref_lens, uint32_t n_refs, uint32_t* n_sites, int32_t** rid,
                              int32_t** pos, uint64_t* n_given, uint64_t* n_unnamed, char* err, uint64_t err_cap)
{
    if (err && err_cap) err[0] = 0;
    if (!path || (!ref_names && n_refs) || (!ref_lens && n_refs) || !n_sites || !rid || !pos) return BQC_ERR_ARG;
    *n_sites = 0; *rid = nullptr; *pos = nullptr;
    if (n_given) *n_given = 0;
    if (n_unnamed) *n_unnamed = 0;
    FILE* f = fopen(path, "rb");
    if (!f) return sites_fail(err, err_cap, "%s: the file could not be opened", path);
    std::unordered_map<std::string, uint32_t> index;
    for (uint32_t r = 0; r < n_refs; ++r) index.emplace(ref_names[r] ? ref_names[r] : "", r); // (a name given twice: the first contig of that name)
    std::vector<Site> sites;
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
        char* tab = (char*)memchr(line, '\t', (size_t)len);
        if (!tab) { rc = sites_fail(err, err_cap, "%s: line %llu: no tab between the contig and the position", path, (unsigned long long)line_no); break; }
        const char* p = tab + 1;
        uint64_t v = 0;
        const char* q = p;
        for (; *q >= '0' && *q <= '9'; ++q)
            if (v < 1ull << 40) v = v * 10 + (uint64_t)(*q - '0'); // (more digits: behind every contig's end all the same)
        if (q == p || (*q && *q != '\t') || v < 1) {
            const std::string field(p, strcspn(p, "\t"));
            rc = sites_fail(err, err_cap, "%s: line %llu: the position '%s' is not a number of 1 or more", path, (unsigned long long)line_no, field.c_str());
            break;
        }
        ++given;
        const auto it = index.find(std::string(line, (size_t)(tab - line)));
        if (it == index.end()) { ++unnamed; continue; }
        if (v > ref_lens[it->second]) {
            rc = sites_fail(err, err_cap, "%s: line %llu: position %llu lies behind the end of contig %s (%u bases)", path, (unsigned long long)line_no, (unsigned long long)v,
                            ref_names[it->second], ref_lens[it->second]);
            break;
        }
        if (v > 0x7FFFFFFFull) { // (pos counted from 0 must stay at or below 2^31 - 2)
            rc = sites_fail(err, err_cap, "%s: line %llu: position %llu is more than 2147483647", path, (unsigned long long)line_no, (unsigned long long)v);
            break;
        }
        sites.push_back(Site{(int32_t)it->second, (int32_t)(v - 1), line_no});
    }
    free(line);
    const bool read_error = ferror(f) != 0;
    fclose(f);
    if (rc) return rc;
    if (read_error) return sites_fail(err, err_cap, "%s: the file could not be read", path);
    std::stable_sort(sites.begin(), sites.end(), [](const Site& a, const Site& b) { return a.rid != b.rid ? a.rid < b.rid : a.pos < b.pos; });
    for (size_t i = 1; i < sites.size(); ++i)
        if (sites[i].rid == sites[i - 1].rid && sites[i].pos == sites[i - 1].pos)
            return sites_fail(err, err_cap, "%s: line %llu: the site %s:%d is given twice (first on line %llu)", path, (unsigned long long)sites[i].line,
                              ref_names[sites[i].rid], sites[i].pos + 1, (unsigned long long)sites[i - 1].line);
    if (n_given) *n_given = given;
    if (n_unnamed) *n_unnamed = unnamed;
    if (sites.empty()) {
        if (given) return sites_fail(err, err_cap, "%s: line %llu: no site left: all %llu sites lie on contigs the header does not name", path, (unsigned long long)line_no, (unsigned long long)given);
        return sites_fail(err, err_cap, "%s: line %llu: no site left: the file holds none", path, (unsigned long long)line_no);
    }
    if (sites.size() > 0xFFFFFFFFull) return sites_fail(err, err_cap, "%s: more than 4294967295 sites", path);
    int32_t* r = (int32_t*)malloc(sites.size() * sizeof(int32_t));
    int32_t* q = (int32_t*)malloc(sites.size() * sizeof(int32_t));
    if (!r || !q) { free(r); free(q); return sites_fail(err, err_cap, "%s: out of memory for %llu sites", path, (unsigned long long)sites.size()); }
    for (size_t i = 0; i < sites.size(); ++i) { r[i] = sites[i].rid; q[i] = sites[i].pos; }
    *n_sites = (uint32_t)sites.size();
    *rid = r;
    *pos = q;
    return 0;
}

extern "C" void bqc_sites_free(int32_t* rid, int32_t* pos)
{
    free(rid);
    free(pos);
}
