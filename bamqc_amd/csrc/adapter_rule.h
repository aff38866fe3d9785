// adapter_rule.h — what a single adapter of the adapter-by-cycle module may look like (include/bamqc.h: the adapter set), stated once
// for bqc_create_ex (bqc_api.cpp) and for the program's --adapter NAME=SEQ (host/driver.cpp).  Host-only code.
#pragma once
#include <cstring>
#include <string>
#include "../../include/bamqc.h"

// The built-in adapter set (include/bamqc.h), in the set's order: bqc_create_ex's when none is given, and what the overrepresented
// sequences' possible source is looked up in.
inline const bqc_adapter* bqc_builtin_adapters(uint32_t* n)
{
    static const bqc_adapter builtin[] = {{"Illumina_Universal", "AGATCGGAAGAG"}, {"Illumina_SmallRNA_3p", "TGGAATTCTCGG"}, {"Illumina_SmallRNA_5p", "GATCGTCGGACT"},
                                          {"Nextera_Transposase", "CTGTCTCTTATA"}, {"PolyA", "AAAAAAAAAAAA"}, {"PolyG", "GGGGGGGGGGGG"}};
    *n = (uint32_t)(sizeof builtin / sizeof builtin[0]);
    return builtin;
}
// the name of the first built-in adapter that occurs letter for letter in `seq`, else "-"
inline const char* bqc_possible_source(const char* seq)
{
    uint32_t n;
    const bqc_adapter* set = bqc_builtin_adapters(&n);
    for (uint32_t a = 0; a < n; ++a)
        if (strstr(seq, set[a].seq)) return set[a].name;
    return "-";
}

// "" when the adapter is good, else what is wrong with it, naming the offending thing
inline std::string bqc_adapter_fault(const char* name, const char* seq)
{
    if (!name || !seq) return "an adapter has a null name or sequence";
    const size_t ln = strnlen(name, 32), m = strnlen(seq, 17);
    bool good = ln >= 1 && ln <= 31;
    for (size_t i = 0; good && i < ln; ++i) {
        const char ch = name[i];
        good = (ch >= 'A' && ch <= 'Z') || (ch >= 'a' && ch <= 'z') || (ch >= '0' && ch <= '9') || ch == '_' || ch == '.' || ch == '-';
    }
    if (!good) return "the adapter name '" + std::string(name, ln) + "' is not 1 to 31 characters of [A-Za-z0-9_.-]";
    if (m < 8 || m > 16) return "adapter '" + std::string(name) + "': the sequence '" + std::string(seq, m) + "' is not 8 to 16 letters long";
    for (size_t i = 0; i < m; ++i)
        if (!seq[i] || !strchr("ACGT", seq[i])) return "adapter '" + std::string(name) + "': the letter '" + std::string(1, seq[i]) + "' of the sequence '" + seq + "' is not one of ACGT";
    return "";
}
