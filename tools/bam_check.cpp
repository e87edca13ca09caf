// tools/bam_check.cpp - the native BAM reader (vapor_amd/csrc/vapor_bam.cpp, host code) for a sanitizer build: walks every
// record of a file through vapor_bam_chop - one index chunk from the given virtual offset to the end of the file, a window
// per call - and prints the status of each call.  A damaged file must end in a status, never in a report of the sanitizer.
//   g++ -O1 -g -fsanitize=address,undefined -Iinclude -Ivapor_amd/csrc -o /tmp/bam_check tools/bam_check.cpp -lz -lpthread
//   ASAN_OPTIONS=detect_leaks=0 /tmp/bam_check file.bam <first virtual offset> <tid> <start> <end> <flank> [threads [min_mapq exclude_flags]]
// With min_mapq and exclude_flags (decimal or 0x hex) the handle carries that read filter (vapor_bam_set_filter), and
// the right-anchored and the tagged reader walk the file behind the plain one; without them nothing changes.
// A last argument `depth` adds a depth pass (vapor_bam_depth) over every record of the file behind the others:
// the intervals [0, start) [start, end) [end, 2^31 - 1) of the contig, under the handle's filter.
// A last argument `sig` adds, in place of the depth pass, a signature pass (vapor_bam_signature) over every record: a
// region per contig from 0 to the one behind `tid`, its window [0, 2^31 - 1), the targets start and end, tolerance 50, minimum
// clip 30, every length and every event kind, under the handle's filter.
// A last argument `links` adds, in place of the depth pass, a links pass (vapor_bam_links) over every record: per
// contig from 0 to the one behind `tid` the eight regions ev x pend x rel, the window [0, 2^31 - 1), the local target start, the
// partner target end, tolerance 50, minimum clip 30, the partner's name the bytes "c1" of a three-name blob, under the handle's
// filter.
// A last argument `sup` adds, in place of the depth pass, a support pass (vapor_bam_support) over every record: a
// region per contig from 0 to the one behind `tid`, the signature pass's nine fields with the mask 255, the flank 51 and the
// blocking length 30, under the handle's filter.
// tests/test_bamio.py builds it and runs it over the damaged files of its other tests and a few hundred randomly damaged ones.
#include "vapor_bam.cpp"
#include <cstdio>
#include <sys/stat.h>

int main(int argc, char** argv)
{
    const bool depth = argc > 7 && !strcmp(argv[argc - 1], "depth");
    const bool sig = argc > 7 && !strcmp(argv[argc - 1], "sig");
    const bool lnk = argc > 7 && !strcmp(argv[argc - 1], "links");
    const bool sup = argc > 7 && !strcmp(argv[argc - 1], "sup");
    if (depth || sig || lnk || sup) --argc;
    if (argc < 7) { fprintf(stderr, "usage: bam_check file.bam first_voffset tid start end flank [threads [min_mapq exclude_flags]] [depth | sig | links | sup]\n"); return 2; }
    vapor_bam* b = nullptr;
    if (vapor_bam_open(argv[1], &b) != 0) { printf("open: %s\n", vapor_bam_last_error()); return 0; }
    if (argc > 7) vapor_bam_set_threads(b, atoi(argv[7]));
    const bool filtered = argc > 9;
    if (filtered) {
        const int frc = vapor_bam_set_filter(b, (int32_t)strtol(argv[8], nullptr, 0), (uint32_t)strtoul(argv[9], nullptr, 0));
        printf("filter: rc %d %s\n", frc, frc ? vapor_bam_last_error() : "");
    }
    struct stat st;
    if (stat(argv[1], &st) != 0) return 2;
    const uint64_t chunk[2] = {strtoull(argv[2], nullptr, 10), (uint64_t)st.st_size << 16};
    const int32_t tid = atoi(argv[3]);
    const int64_t start = atoll(argv[4]), end = atoll(argv[5]), flank = atoll(argv[6]);
    // small buffers first (the overflow answer and its sizes), then as asked for
    std::vector<uint8_t> seq(64);
    std::vector<char> names(8);
    std::vector<int64_t> meta(4);
    int32_t n = 0;
    int64_t need[3] = {0, 0, 0};
    int rc = vapor_bam_chop(b, tid, start, end, flank, 1, chunk, seq.data(), (int64_t)seq.size(), names.data(), (int64_t)names.size(),
                            meta.data(), 1, &n, need);
    printf("small buffers: rc %d reads %d need %lld %lld %lld %s\n", rc, n, (long long)need[0], (long long)need[1], (long long)need[2],
           rc ? vapor_bam_last_error() : "");
    if (rc == VAPOR_E_OVERFLOW) {
        seq.resize((size_t)need[0] + 16); names.resize((size_t)need[1] + 16); meta.resize(4 * ((size_t)need[2] + 1));
        rc = vapor_bam_chop(b, tid, start, end, flank, 1, chunk, seq.data(), (int64_t)seq.size(), names.data(), (int64_t)names.size(),
                            meta.data(), (int32_t)need[2] + 1, &n, need);
        long long bases = 0;
        for (int32_t r = 0; r < n && rc == 0; ++r) bases += meta[4 * r + 1];
        printf("sized buffers: rc %d reads %d bases %lld %s\n", rc, n, bases, rc ? vapor_bam_last_error() : "");
    }
    if (filtered) {
        // the other flavours of the reader under the same filter, their buffers sized by a first call each
        for (int flavour = 0; flavour < 2; ++flavour) {
            const int w = flavour ? 6 : 4;
            auto call = [&](int32_t max_reads) {
                return flavour ? vapor_bam_chop_tagged(b, tid, start, end, flank, 1, chunk, seq.data(), (int64_t)seq.size(), names.data(),
                                                       (int64_t)names.size(), meta.data(), max_reads, &n, need)
                               : vapor_bam_chop_right(b, tid, start, end, flank, 1, chunk, seq.data(), (int64_t)seq.size(), names.data(),
                                                      (int64_t)names.size(), meta.data(), max_reads, &n, need);
            };
            meta.resize((size_t)w * std::max<size_t>(meta.size() / 4, 1));
            rc = call((int32_t)(meta.size() / (size_t)w));
            if (rc == VAPOR_E_OVERFLOW) {
                seq.resize((size_t)need[0] + 16); names.resize((size_t)need[1] + 16); meta.resize((size_t)w * ((size_t)need[2] + 1));
                rc = call((int32_t)need[2] + 1);
            }
            long long bases = 0;
            for (int32_t r = 0; r < n && rc == 0; ++r) bases += meta[(size_t)w * r + 1];
            printf("%s: rc %d reads %d bases %lld %s\n", flavour ? "tagged" : "right", rc, n, bases, rc ? vapor_bam_last_error() : "");
        }
    }
    if (depth) {
        const int64_t s = std::max<int64_t>(start, 0), e = std::max(end, s);
        const int64_t bounds[4] = {0, s, e, std::max<int64_t>(e, ((int64_t)1 << 31) - 1)};
        uint64_t cov[3] = {0, 0, 0};
        rc = vapor_bam_depth(b, tid, bounds, 1, chunk, cov);
        printf("depth: rc %d cov %llu %llu %llu %s\n", rc, (unsigned long long)cov[0], (unsigned long long)cov[1], (unsigned long long)cov[2],
               rc ? vapor_bam_last_error() : "");
    }
    if (sig) {
        for (int32_t t = 0; t <= std::max(tid, 0) + 1; ++t) {
            const int64_t fields[9] = {0, ((int64_t)1 << 31) - 1, start, std::max(end, start), 50, 30, 0, (int64_t)1 << 28, 63};
            int64_t out[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
            rc = vapor_bam_signature(b, t, fields, 1, chunk, out);
            printf("sig: contig %d rc %d counts %lld %lld %lld %lld %lld %lld modes %lld %lld %lld %lld %s\n", t, rc, (long long)out[0], (long long)out[1],
                   (long long)out[2], (long long)out[3], (long long)out[4], (long long)out[5], (long long)out[6], (long long)out[7], (long long)out[8],
                   (long long)out[9], rc ? vapor_bam_last_error() : "");
        }
    }
    if (lnk) {
        const uint8_t blob[] = {'c', '0', 'c', '1', 'c', '1', '0'};
        for (int32_t t = 0; t <= std::max(tid, 0) + 1; ++t)
            for (int q = 0; q < 8; ++q) {
                const int64_t fields[11] = {0, ((int64_t)1 << 31) - 1, start, end, 50, 30, q & 1, (q >> 1) & 1, (q >> 2) & 1, 2, 2};
                int64_t out[5] = {0, 0, 0, 0, 0};
                rc = vapor_bam_links(b, t, fields, blob, (int64_t)sizeof blob, 1, chunk, out);
                printf("links: contig %d ev %d pend %d rel %d rc %d words %lld %lld %lld %lld %lld %s\n", t, q & 1, (q >> 1) & 1, (q >> 2) & 1, rc, (long long)out[0],
                       (long long)out[1], (long long)out[2], (long long)out[3], (long long)out[4], rc ? vapor_bam_last_error() : "");
            }
    }
    if (sup) {
        for (int32_t t = 0; t <= std::max(tid, 0) + 1; ++t) {
            const int64_t fields[11] = {0, ((int64_t)1 << 31) - 1, start, std::max(end, start), 50, 30, 0, (int64_t)1 << 28, 255, 51, 30};
            int64_t out[7] = {0, 0, 0, 0, 0, 0, 0};
            rc = vapor_bam_support(b, t, fields, 1, chunk, out);
            printf("sup: contig %d rc %d words %lld %lld %lld %lld %lld %lld %lld %s\n", t, rc, (long long)out[0], (long long)out[1], (long long)out[2],
                   (long long)out[3], (long long)out[4], (long long)out[5], (long long)out[6], rc ? vapor_bam_last_error() : "");
        }
    }
    vapor_bam_close(b);
    return 0;
}
