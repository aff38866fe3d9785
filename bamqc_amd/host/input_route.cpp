// input_route.cpp — see input_route.h.  The table this function states is DESIGN section 4.5d, "which reader takes it".
#include "input_route.h"

#include <sys/stat.h>

#include <cstdlib>
#include <cstring>

#include "host_tools.h"

InputKind input_kind(const char* path, bool* regular, uint64_t* size)
{
    const size_t n = strlen(path);
    auto ends = [&](const char* sfx) { const size_t k = strlen(sfx); return n >= k && strcmp(path + n - k, sfx) == 0; };
    struct stat st;
    const bool known = strcmp(path, "-") != 0 && stat(path, &st) == 0;
    if (regular) *regular = known && S_ISREG(st.st_mode);
    if (size) *size = known && S_ISREG(st.st_mode) ? (uint64_t)st.st_size : 0;
    if (strcmp(path, "-") == 0) return IN_STDIN;
    if (ends(".sam.gz")) return IN_SAM_BGZF;
    if (ends(".sam")) return IN_SAM;
    if (known && !S_ISREG(st.st_mode) && !S_ISDIR(st.st_mode)) return IN_STREAM;
    return ends(".bam") ? IN_BAM : IN_OTHER;
}
bool bqc_input_is_sam_text(const char* path) { const InputKind k = input_kind(path); return k == IN_SAM || k == IN_SAM_BGZF; } // (host_tools.h: the front end of --gpus N)

GpuDecode gpu_decode_env()
{
    const char* e = getenv("BQC_GPU_DECODE");
    return !e ? GD_UNSET : atoi(e) == 0 ? GD_OFF : GD_ON;
}

extern "C" void bqc_input_route(const bqc_route_facts* facts, bqc_route* route)
{
    const bqc_route_facts& f = *facts;
    bqc_route& r = *route;
    r = bqc_route{};
    const bool program = f.caller == CALLER_PROGRAM, lib_card = f.caller == CALLER_LIB_CARD, lib_host = f.caller == CALLER_LIB_HOST;
    const bool off = f.gpu_decode == GD_OFF, on = f.gpu_decode == GD_ON, unset = f.gpu_decode == GD_UNSET;
    const bool card_allowed = lib_card || (program && !f.host_reader_only); // (before the variable, the size and the header have their say)
    // A BGZF stream the card may take (either caller): the variable steers it, a header without @RG is the host reader's, and with the variable
    // unset the stream is held up to `from` bytes and goes to the card if it has not ended by then.
    auto stream_rule = [&](uint64_t from, int card_reader, int host_reader) {
        bool card = card_allowed && !off && f.has_rg;
        if (card && unset) { r.hold = from; card = !f.ended; }
        r.reader = card ? card_reader : host_reader;
    };
    if (f.shard) { // one process's part of a BAM file; a path that is no regular file too: never the stream branch
        if (f.kind == IN_STDIN && program) r.refuse = REFUSE_STDIN_SHARD;
        else if (f.kind == IN_SAM || f.kind == IN_SAM_BGZF || (f.kind == IN_STDIN && lib_card)) r.refuse = REFUSE_SAM_SHARD;
        if (r.refuse) return;
        r.header_by = HDR_BAM; r.reader = RD_BAM; r.source = SRC_RANGE;
        if (lib_host) return;
        r.find_blocks = lib_card || (!f.host_reader_only && !off && f.regular);
        if (lib_card && !f.shard_found) r.refuse = REFUSE_EMPTY_SHARD;
        // (an empty part, or a small one, is the host reader's: the GPU reader's set-up costs ~50 ms)
        r.header_first = lib_card || (r.find_blocks && f.shard_found && (on || f.shard_bytes >= kBamStreamCardFrom));
        if (r.header_first && (lib_card || f.has_rg)) r.reader = RD_GPU_BAM; // (no @RG line: the host reader, over its range, decides what that means)
        return;
    }
    if (f.kind == IN_STDIN) r.sniff = lib_host || (program && off) ? SNIFF_STDIO : SNIFF_FD; // (the host's SAM parser reads stdin through stdio)
    r.stream = f.kind == IN_STDIN ? f.dash_bgzf != 0 : f.kind == IN_STREAM || (f.kind == IN_SAM_BGZF && !f.regular && !lib_host);
    r.source = r.stream ? SRC_STREAM : SRC_FILE;
    if ((f.kind == IN_STDIN && !r.stream) || f.kind == IN_SAM) { // plain SAM text: no second pass exists here, host_reader_only has no say
        const bool by_size = f.kind == IN_SAM && f.regular;
        if (lib_card) { r.header_by = HDR_GSAM; r.reader = RD_GPU_SAM; }
        else if (program && !off && (!by_size || on || f.size >= kSamCardFrom)) {
            r.header_by = HDR_GSAM;
            r.hold = on || by_size ? 0 : kSamCardFrom; // (a regular file: by its size instead of holding bytes)
            r.reader = f.has_rg && (on || !f.ended) ? RD_GPU_SAM : RD_GSAM_MEMORY;
        }
        else { r.header_by = HDR_SAM_STDIO; r.reader = RD_SAM_STDIO; }
    }
    else if (f.kind == IN_SAM_BGZF || (r.stream && f.carries == CARRIES_SAM_TEXT)) { // SAM text inside BGZF
        r.header_by = HDR_SAM_BGZF;
        if (r.stream) stream_rule(kSamBgzfCardFrom, RD_GPU_SAM_BGZF, RD_SAM_BGZF);
        else r.reader = lib_card || (card_allowed && !off && f.regular && (on || f.size >= kSamBgzfCardFrom) && f.has_rg) ? RD_GPU_SAM_BGZF : RD_SAM_BGZF;
    }
    else if (r.stream) { r.header_by = HDR_BAM; stream_rule(kBamStreamCardFrom, RD_GPU_BAM, RD_BAM); } // a BAM stream
    else { // a BAM file read as a whole
        r.header_by = HDR_BAM;
        r.header_first = lib_card || (card_allowed && !off && f.regular && (on || f.size >= kBamStreamCardFrom));
        r.reader = r.header_first && (lib_card || f.has_rg) ? RD_GPU_BAM : RD_BAM;
    }
}
