// tools/sa_check.cpp - vapor_amd/csrc/vapor_sa.h (the SA:Z grammar of `--links`; host code) held to direct
// statements of the grammar, for a sanitizer build:
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -Ivapor_amd/csrc tools/sa_check.cpp -o /tmp/sa_check
//   ASAN_OPTIONS=detect_leaks=0 /tmp/sa_check
// parse_piece against the regular expression of the rule (std::regex) with the three range rules beside it, on designed pieces
// and on seeded ones drawn from an alphabet that is mostly grammar; for_each_piece against a cut written here; find_sa against
// aux areas built field by field, whole and cut short at every byte.  Every buffer is a heap copy of its exact size, so that a
// read past a piece, a value or a record is the sanitizer's to report.  Prints one line per part and "sa_check: all equal".
#include "vapor_sa.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>
#include <regex>
#include <string>
#include <vector>

using namespace vapor_sa;

static std::mt19937_64 rng(20211);
static int rnd(int lo, int hi) { return lo + (int)(rng() % (uint64_t)(hi - lo + 1)); }

#define CHECK(cond, ...) do { if (!(cond)) { fprintf(stderr, "sa_check: " __VA_ARGS__); fprintf(stderr, "\n"); exit(1); } } while (0)

struct Want {
    bool ok = false;
    std::string name;
    int64_t a = 0, b = 0;
    bool minus = false;
    uint32_t mapq = 0;
};

// the rule, stated directly: the regular expression, then pos in 1 .. 2^31 - 1, mapq at most 255, every length at most 2^28 - 1
static Want by_the_rule(const std::string& piece)
{
    static const std::regex whole("([^,;]+),([0-9]{1,10}),([+-]),((?:[0-9]{1,9}[MIDNSHP=X])+),([0-9]{1,3}),([0-9]+)");
    static const std::regex op("([0-9]{1,9})([MIDNSHP=X])");
    Want w;
    std::smatch m;
    if (!std::regex_match(piece, m, whole)) return w;
    const long long pos = atoll(m[2].str().c_str()), mapq = atoll(m[5].str().c_str());
    if (pos < 1 || pos > 2147483647LL || mapq > 255) return w;
    const std::string cg = m[4].str();
    long long span = 0;
    for (std::sregex_iterator it(cg.begin(), cg.end(), op), end; it != end; ++it) {
        const long long n = atoll((*it)[1].str().c_str());
        if (n > 268435455LL) return w;
        const char c = (*it)[2].str()[0];
        if (c == 'M' || c == 'D' || c == 'N' || c == '=' || c == 'X') span += n;
    }
    w.ok = true;
    w.name = m[1].str();
    w.a = pos - 1;
    w.b = pos - 1 + span;
    w.minus = m[3].str() == "-";
    w.mapq = (uint32_t)mapq;
    return w;
}

static bool same(const Want& w, bool ok, const Entry& e)
{
    if (w.ok != ok) return false;
    if (!ok) return true;
    return w.name == std::string((const char*)e.name, e.name_len) && w.a == e.a && w.b == e.b && w.minus == e.minus && w.mapq == e.mapq;
}

static void one_piece(const std::string& piece)
{
    if (piece.find(';') != std::string::npos) {
        // a ';' never stands inside a piece: parse_piece refuses one that is handed over anyway
        std::unique_ptr<uint8_t[]> buf(new uint8_t[piece.size()]);
        memcpy(buf.get(), piece.data(), piece.size());
        Entry e;
        CHECK(!parse_piece(buf.get(), buf.get() + piece.size(), &e), "a piece with ';' passes: %s", piece.c_str());
        return;
    }
    std::unique_ptr<uint8_t[]> buf(new uint8_t[piece.size() ? piece.size() : 1]);
    memcpy(buf.get(), piece.data(), piece.size());
    Entry e;
    const bool ok = parse_piece(buf.get(), buf.get() + piece.size(), &e);
    CHECK(same(by_the_rule(piece), ok, e), "parse_piece and the rule differ on: %s", piece.c_str());
}

static long check_designed()
{
    struct D { const char* text; bool ok; int64_t a, b; };
    const D designed[] = {
        {"chr1,100,+,50M,60,0", true, 99, 149},
        {"chr1,100,-,10S50M5D20M3I7N2=4X9H1P,0,12", true, 99, 99 + 50 + 5 + 20 + 7 + 2 + 4},
        {"c,0,+,5M,60,0", false, 0, 0},
        {"c,2147483647,+,5M,60,0", true, 2147483646LL, 2147483651LL},
        {"c,2147483648,+,5M,60,0", false, 0, 0},
        {"c,0000000100,+,5M,60,0", true, 99, 104},
        {"c,00000000100,+,5M,60,0", false, 0, 0},
        {"c,100,+,268435455M,60,0", true, 99, 99 + 268435455LL},
        {"c,100,+,268435456M,60,0", false, 0, 0},
        {"c,100,+,0000000005M,60,0", false, 0, 0},
        {"c,100,+,000000005M,60,0", true, 99, 104},
        {"c,100,+,5M7,60,0", false, 0, 0},
        {"c,100,+,,60,0", false, 0, 0},
        {"c,100,+,*,60,0", false, 0, 0},
        {"c,100,+,M,60,0", false, 0, 0},
        {"c,100,+,5M5,60,0", false, 0, 0},
        {"c,100,+,5Q,60,0", false, 0, 0},
        {"c,100,.,5M,60,0", false, 0, 0},
        {"c,100,,5M,60,0", false, 0, 0},
        {"c,100,+-,5M,60,0", false, 0, 0},
        {"c,100,+,5M,255,0", true, 99, 104},
        {"c,100,+,5M,256,0", false, 0, 0},
        {"c,100,+,5M,0060,0", false, 0, 0},
        {"c,100,+,5M,,0", false, 0, 0},
        {"c,100,+,5M,60,", false, 0, 0},
        {"c,100,+,5M,60,x", false, 0, 0},
        {"c,100,+,5M,60,1x", false, 0, 0},
        {"c,100,+,5M,60,00000000000000000000000000000000001", true, 99, 104},
        {"c,100,+,5M,60", false, 0, 0},
        {"c,100,+,5M,60,0,7", false, 0, 0},
        {",100,+,5M,60,0", false, 0, 0},
        {"c", false, 0, 0},
        {",,,,,", false, 0, 0},
        {" c d,100,+,5M,60,0", true, 99, 104},
        {"c, 100,+,5M,60,0", false, 0, 0},
        {"c,1e2,+,5M,60,0", false, 0, 0},
        {"c,-100,+,5M,60,0", false, 0, 0},
        {"c,100,+,5M,60,0;", false, 0, 0},
    };
    long n = 0;
    for (const D& d : designed) {
        const std::string piece(d.text);
        if (piece.find(';') == std::string::npos) {
            const Want w = by_the_rule(piece);
            CHECK(w.ok == d.ok && (!d.ok || (w.a == d.a && w.b == d.b)), "the rule itself is misstated on: %s", d.text);
        }
        one_piece(piece);
        ++n;
    }
    // the sums are 64-bit: sixty operations of the longest length
    std::string big = "c,2147483647,+,";
    for (int k = 0; k < 60; ++k) big += "268435455N";
    big += ",1,1";
    const Want w = by_the_rule(big);
    CHECK(w.ok && w.b == 2147483646LL + 60 * 268435455LL, "the 64-bit sum");
    one_piece(big);
    return n + 1;
}

static std::string seeded_piece()
{
    // a well-formed piece, then a few edits: most seeded pieces are near the grammar's edges, not noise
    static const char letters[] = "MIDNSHP=X";
    static const char noise[] = "0123456789,;+-MIDNSHP=X*. abz";
    std::string s;
    for (int k = rnd(1, 6); k > 0; --k) s += (char)rnd('a', 'z');
    s += ',';
    for (int k = rnd(1, 10); k > 0; --k) s += (char)rnd('0', '9');
    s += ',';
    s += rnd(0, 1) ? '+' : '-';
    s += ',';
    for (int k = rnd(1, 5); k > 0; --k) {
        for (int d = rnd(1, 9); d > 0; --d) s += (char)rnd('0', '9');
        s += letters[rnd(0, 8)];
    }
    s += ',';
    for (int k = rnd(1, 3); k > 0; --k) s += (char)rnd('0', '9');
    s += ',';
    for (int k = rnd(1, 4); k > 0; --k) s += (char)rnd('0', '9');
    for (int edits = rnd(0, 3); edits > 0; --edits) {
        const int how = rnd(0, 2);
        const size_t at = (size_t)rnd(0, (int)s.size() - 1);
        const char c = noise[rnd(0, (int)sizeof noise - 2)];
        if (how == 0) s[at] = c;
        else if (how == 1) s.insert(at, 1, c);
        else if (s.size() > 1) s.erase(at, 1);
    }
    return s;
}

static long check_seeded()
{
    long n_ok = 0;
    for (int it = 0; it < 20000; ++it) {
        const std::string p = seeded_piece();
        if (p.find(';') == std::string::npos && by_the_rule(p).ok) ++n_ok;
        one_piece(p);
    }
    CHECK(n_ok > 2000 && n_ok < 18000, "the seeded pieces are all of one kind (%ld well-formed)", n_ok);
    return n_ok;
}

static long check_values()
{
    long n_values = 0;
    for (int it = 0; it < 4000; ++it) {
        // a value: pieces and separators as they come - ";;" and a last piece without ';' among them
        std::string v;
        for (int k = rnd(0, 5); k > 0; --k) {
            if (rnd(0, 5) == 0) v += ';';
            else {
                std::string p = seeded_piece();
                v += p;
                if (k > 1 || rnd(0, 1)) v += ';';
            }
        }
        // the cut, written here: at every ';', empty pieces dropped
        std::vector<std::string> pieces;
        std::string cur;
        for (char c : v) {
            if (c == ';') { if (!cur.empty()) pieces.push_back(cur); cur.clear(); }
            else cur += c;
        }
        if (!cur.empty()) pieces.push_back(cur);
        std::unique_ptr<uint8_t[]> buf(new uint8_t[v.size() ? v.size() : 1]);
        memcpy(buf.get(), v.data(), v.size());
        size_t at = 0;
        for_each_piece(buf.get(), v.size(), [&](bool ok, const Entry& e) {
            CHECK(at < pieces.size(), "more pieces than the cut has in: %s", v.c_str());
            CHECK(same(by_the_rule(pieces[at]), ok, e), "piece %zu of: %s", at, v.c_str());
            ++at;
            return false;
        });
        CHECK(at == pieces.size(), "%zu pieces of %zu in: %s", at, pieces.size(), v.c_str());
        // the walk ends where the caller says so
        if (!pieces.empty()) {
            const size_t stop_at = (size_t)rnd(0, (int)pieces.size() - 1);
            size_t seen = 0;
            for_each_piece(buf.get(), v.size(), [&](bool, const Entry&) { return seen++ == stop_at; });
            CHECK(seen == stop_at + 1, "the walk goes on behind its end");
        }
        ++n_values;
    }
    // an empty value has no piece
    uint8_t none = 0;
    for_each_piece(&none, 0, [&](bool, const Entry&) { CHECK(false, "an empty value has a piece"); return true; });
    return n_values;
}

static void put32(std::string& s, int32_t v) { for (int k = 0; k < 4; ++k) s += (char)((uint32_t)v >> (8 * k)); }

static long check_find()
{
    long n = 0;
    for (int it = 0; it < 3000; ++it) {
        // an aux area field by field; the first field named SA decides
        std::string area;
        int want = FIND_NONE;
        std::string want_value;
        for (int k = rnd(0, 6); k > 0; --k) {
            const bool sa = rnd(0, 2) == 0;
            std::string tag = sa ? "SA" : std::string(1, (char)rnd('A', 'Z')) + (char)rnd('0', '9');
            const int ty = rnd(0, 6);
            std::string f = tag;
            std::string value;
            if (ty == 0) { f += 'A'; f += 'x'; }
            else if (ty == 1) { f += 'c'; f += (char)rnd(0, 255); }
            else if (ty == 2) { f += 'S'; f += (char)rnd(0, 255); f += (char)rnd(0, 255); }
            else if (ty == 3) { f += 'i'; put32(f, rnd(-1000, 1000)); }
            else if (ty == 4) { f += 'B'; f += 'I'; const int cnt = rnd(0, 5); put32(f, cnt); for (int j = 0; j < cnt; ++j) put32(f, rnd(0, 1 << 20)); }
            else {
                f += (ty == 5 ? 'Z' : 'H');
                for (int j = rnd(0, 150); j > 0; --j) value += (char)rnd(33, 126);
                f += value; f += '\0';
            }
            area += f;
            if (sa) {
                if (ty == 5) { want = FIND_VALUE; want_value = value; }
                // (what follows the first SA is not looked at, whatever its type: garbage may stand there)
                if (rnd(0, 1)) area += "??";
                break;
            }
        }
        auto run = [&](size_t len, const uint8_t** value, size_t* vlen) {
            std::unique_ptr<uint8_t[]> buf(new uint8_t[len ? len : 1]);
            memcpy(buf.get(), area.data(), len);
            const int got = find_sa(buf.get(), buf.get() + len, value, vlen);
            std::string out;
            if (got == FIND_VALUE) out.assign((const char*)*value, *vlen);
            return std::make_pair(got, out);
        };
        const uint8_t* value = nullptr;
        size_t vlen = 0;
        const auto whole = run(area.size(), &value, &vlen);
        CHECK(whole.first == want && whole.second == want_value, "find_sa on a whole area: %d, not %d", whole.first, want);
        // cut short at every byte: a status, never a read past the end; a value only when its NUL is inside
        for (size_t len = 0; len < area.size(); ++len) {
            const auto part = run(len, &value, &vlen);
            CHECK(part.first == FIND_NONE || part.first == FIND_MALFORMED || (part.first == FIND_VALUE && part.second == want_value), "find_sa on a cut area");
        }
        ++n;
    }
    // designed: two SA fields - the first decides; an SA of type A; an unknown type; an SA:Z without its NUL
    const uint8_t* value = nullptr;
    size_t vlen = 0;
    const std::string two = std::string("SAZfirst") + '\0' + "SAZsecond" + '\0';
    CHECK(find_sa((const uint8_t*)two.data(), (const uint8_t*)two.data() + two.size(), &value, &vlen) == FIND_VALUE && std::string((const char*)value, vlen) == "first", "two SA fields");
    const std::string typed_a = std::string("SAAx") + "SAZsecond" + '\0';
    CHECK(find_sa((const uint8_t*)typed_a.data(), (const uint8_t*)typed_a.data() + typed_a.size(), &value, &vlen) == FIND_NONE && value == nullptr, "an SA of type A");
    const std::string unknown = std::string("XYq1") + "SAZv" + '\0';
    CHECK(find_sa((const uint8_t*)unknown.data(), (const uint8_t*)unknown.data() + unknown.size(), &value, &vlen) == FIND_MALFORMED, "an unknown type");
    const std::string open = "SAZchr1,1,+,5M,1,1;";
    CHECK(find_sa((const uint8_t*)open.data(), (const uint8_t*)open.data() + open.size(), &value, &vlen) == FIND_MALFORMED, "an SA:Z without its NUL");
    return n + 4;
}

int main()
{
    printf("designed pieces: %ld equal the rule\n", check_designed());
    printf("seeded pieces: 20000 equal the rule (%ld well-formed)\n", check_seeded());
    printf("values: %ld cut and parsed as the rule cuts and parses them\n", check_values());
    printf("aux areas: %ld found as built, whole and cut short at every byte\n", check_find());
    printf("sa_check: all equal\n");
    return 0;
}
