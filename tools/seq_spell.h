// seq_spell.h - the text a list of segments spells over the texts of a set's literals, for the check programs that hold the host
// plans to the texts (tools/planner_check.cpp, tools/seqset_check.cpp): a slice of a parent per segment, reversed and complemented
// where the segment says so (invert_base's pairs; every other character stays), the whole upper-cased on request.
#pragma once

#include "vapor_planner.h"

#include <string>
#include <vector>

namespace seq_spell {

inline char comp(char c)
{
    switch (c) {
    case 'A': return 'T'; case 'T': return 'A'; case 'C': return 'G'; case 'G': return 'C';
    case 'a': return 't'; case 't': return 'a'; case 'c': return 'g'; case 'g': return 'c';
    default: return c;
    }
}
inline std::string revcomp(const std::string& s)
{
    std::string r(s.rbegin(), s.rend());
    for (char& c : r) c = comp(c);
    return r;
}
inline std::string upper(std::string s)
{
    for (char& c : s) if (c >= 'a' && c <= 'z') c = (char)(c - 32);
    return s;
}

// `out`: what `segs` spell over text[0 .. n_lit).  false, with `why`, when a segment is empty, lies outside its parent or does not
// begin where the one before it ends.
inline bool spell(const std::vector<std::string>& text, int32_t n_lit, const std::vector<vapor::HSeg>& segs, bool up, std::string& out, std::string& why)
{
    out.clear();
    for (const vapor::HSeg& x : segs) {
        if (!(x.parent >= 0 && x.parent < n_lit && x.off >= 0 && x.len > 0 && (size_t)x.off + (size_t)x.len <= text[(size_t)x.parent].size())) {
            why = "segment " + std::to_string(x.off) + "+" + std::to_string(x.len) + " outside literal " + std::to_string(x.parent);
            return false;
        }
        if (x.dst != (int32_t)out.size()) {
            why = "segment at " + std::to_string(x.dst) + ", " + std::to_string(out.size()) + " symbols before it";
            return false;
        }
        const std::string cut = text[(size_t)x.parent].substr((size_t)x.off, (size_t)x.len);
        out += x.rc ? revcomp(cut) : cut;
    }
    if (up) out = upper(out);
    return true;
}

}  // namespace seq_spell
