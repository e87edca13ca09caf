// polish_call_time.cpp - what the host plan of one vapor_realign_polish / vapor_realign_revote call costs
// (vapor_amd/csrc/vapor_polish_call.h): the plan of a call of `loci` loci, each `reads` pairs and `votes` vote pairs of reads of
// read_len symbols on an allele of allele_len columns, built twenty times - the polish alone, and the re-vote with its spelt output
// and the dealing of allele_len bytes a locus.  No HIP, no device: the share of a call's wall time is this against the call's.
//   g++ -O3 -std=c++17 -Iinclude -Ivapor_amd/csrc tools/polish_call_time.cpp -o polish_call_time
//   ./polish_call_time [loci] [reads] [votes] [read_len] [allele_len] [band]
#include "vapor_polish_call.h"

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <vector>

namespace pc = vapor_polish_call;
namespace vr = vapor_revote;

int main(int argc, char** argv)
{
    const auto arg = [&](int k, int64_t d) { return argc > k ? (int64_t)std::atoll(argv[k]) : d; };
    const int64_t n_loci = arg(1, 480), reads = arg(2, 8), voters = arg(3, 12), read_len = arg(4, 4000), allele_len = arg(5, 6000), band = arg(6, 256);
    std::vector<vapor_pair> pairs, votes;
    std::vector<int64_t> first{0}, col_off{0}, vfirst{0}, spelt_off{0};
    for (int64_t g = 0; g < n_loci; ++g) {                          // (sequence 0 .. n_loci - 1: the alleles; then one read a pair)
        for (int64_t k = 0; k < reads; ++k) pairs.push_back({(int32_t)(n_loci + g * (reads + voters) + k), (int32_t)g, (int32_t)(k * 97 % (allele_len / 2 + 1)), 0, 0});
        for (int64_t k = 0; k < voters; ++k)
            votes.push_back({(int32_t)(n_loci + g * (reads + voters) + reads + k), (int32_t)g, (int32_t)(k * 61 % (allele_len / 2 + 1)), 0, 0});
        first.push_back((int64_t)pairs.size());
        vfirst.push_back((int64_t)votes.size());
        col_off.push_back(col_off.back() + allele_len);
        spelt_off.push_back(spelt_off.back() + vr::spelt_cap(allele_len));
    }
    const auto set = pc::seqs((int32_t)(n_loci * (1 + reads + voters)), [&](int32_t s) { return s < n_loci ? allele_len : read_len; },
                              [&](int32_t s) { return (uint32_t)(s * ((allele_len + 31) / 32)); });
    std::vector<int32_t> lout((size_t)(vr::LOUT * n_loci), 0), vout((size_t)(vr::VOUT * votes.size()) + 1), stats(1), sites(1);
    std::vector<uint8_t> calls(1), ins(1), spelt((size_t)spelt_off.back());
    for (int64_t g = 0; g < n_loci; ++g) lout[(size_t)(vr::LOUT * g + vr::L_PLEN)] = (int32_t)allele_len;
    const pc::RevoteArgs rv{(int64_t)votes.size(), votes.data(), vfirst.data(), vout.data(), lout.data(), spelt_off.data(), spelt.data()};
    pc::Call c{true, (int64_t)pairs.size(), pairs.data(), (int32_t)band, n_loci, first.data(), col_off.data(), stats.data(), calls.data(), sites.data(),
               ins.data(), nullptr, nullptr};
    const auto us = [](auto&& f) {
        std::vector<double> t;
        for (int k = 0; k < 20; ++k) {
            const auto t0 = std::chrono::steady_clock::now();
            f();
            t.push_back(std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count());
        }
        std::sort(t.begin(), t.end());
        return std::make_pair(t[0], t[t.size() / 2]);
    };
    size_t sink = 0;
    bool nothing = false;
    const auto polish = us([&] {
        if (pc::check_args(c, nothing)) std::abort();
        sink += pc::Plan(c, set, vapor_trace::BUDGET_DEFAULT).image.size();
    });
    c.rv = &rv;
    const pc::Plan p(c, set, vapor_trace::BUDGET_DEFAULT);
    const std::vector<uint32_t> staged((size_t)p.staged_words, 0x01010101u);
    const auto revote = us([&] {
        if (pc::check_args(c, nothing)) std::abort();
        sink += pc::Plan(c, set, vapor_trace::BUDGET_DEFAULT).image.size();
    });
    const auto deal = us([&] { p.deal_spelt(staged.data(), lout.data(), spelt_off.data(), spelt.data()); });
    std::printf("%lld loci, %lld pairs and %lld vote pairs of %lld on %lld columns, band %lld: %zu groups, image %zu bytes, %zu staged\n", (long long)n_loci,
                (long long)pairs.size(), (long long)votes.size(), (long long)read_len, (long long)allele_len, (long long)band, p.groups.size(), p.image.size(),
                4 * staged.size());
    std::printf("host plan, us (best, median of 20): polish %.1f %.1f   re-vote %.1f %.1f   deal_spelt %.1f %.1f   (%zu)\n", polish.first, polish.second,
                revote.first, revote.second, deal.first, deal.second, sink % 10);
    return 0;
}
