// dsm_count -- occurrence counts of given patterns in every sample (FMIndex::Search, FMIndex.cpp:360-382, batched on the GPU).
//   dsm_count [--device D] [-f fmin] [--all] [-k K] [--times] a.fmi b.fmi ... < patterns
// Input: one pattern per line, the line's first whitespace-separated token (a reference or dsm_node tuple file can be fed in as it
// is); blank lines are skipped.  Output, one line per pattern in input order: "pattern id:count id:count ...", sample ids in
// argument order (as dsm_node numbers them); only samples with count >= fmin (default 1) unless --all.  -k: the counter's k-mer
// table length (default 10, 0 = none).  --times: host parse, device wait and format seconds on stderr.
// The input is read and counted in batches: batch i+1 is read while batch i is on the card.
#include <getopt.h>
#include <unistd.h>

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "../../include/dsmhip.h"
#include "../csrc/count_input.h"

static const char* USAGE = "usage: dsm_count [--device D] [-f fmin] [--all] [-k K] [--times] a.fmi b.fmi ... < patterns";

static bool parse_u64(const char* s, unsigned long long& v) {
    if (!s || !*s || *s == '-') return false;
    char* end = nullptr;
    v = strtoull(s, &end, 10);
    return end && !*end;
}

int main(int argc, char** argv) {
    int device = 0, kmer = -1;
    unsigned long long fmin = 1;
    bool all = false, times = false;
    static option long_options[] = {{"device", required_argument, 0, 256}, {"all", no_argument, 0, 257}, {"times", no_argument, 0, 258},
                                    {"fmin", required_argument, 0, 'f'},   {0, 0, 0, 0}};
    int c, oi = 0;
    opterr = 0;
    while ((c = getopt_long(argc, argv, "f:k:", long_options, &oi)) != -1) {
        unsigned long long v = 0;
        switch (c) {
            case 'f':
                if (!parse_u64(optarg, v)) { fprintf(stderr, "%s\n", USAGE); return 1; }
                fmin = v;
                break;
            case 'k':
                if (!parse_u64(optarg, v) || v > 12) { fprintf(stderr, "%s\n", USAGE); return 1; }
                kmer = (int)v;
                break;
            case 256:
                if (!parse_u64(optarg, v) || v > 1024) { fprintf(stderr, "%s\n", USAGE); return 1; }
                device = (int)v;
                break;
            case 257: all = true; break;
            case 258: times = true; break;
            default: fprintf(stderr, "%s\n", USAGE); return 1;
        }
    }
    if (optind >= argc) { fprintf(stderr, "%s\n", USAGE); return 1; }

    std::vector<dsm_index*> idx;
    auto close_all = [&]() { for (dsm_index* x : idx) dsm_index_close(x); };
    for (int a = optind; a < argc; ++a) {
        dsm_index* x = nullptr;
        if (dsm_index_open(argv[a], device, &x) != 0) {
            fprintf(stderr, "dsm_count: %s: %s\n", argv[a], dsm_last_error());
            close_all();
            return 1;
        }
        idx.push_back(x);
    }
    const size_t nidx = idx.size();
    dsm_counter* ctr = nullptr;
    if (dsm_counter_create(idx.data(), (int)nidx, kmer, &ctr) != 0) {
        fprintf(stderr, "dsm_count: %s\n", dsm_last_error());
        close_all();
        return 1;
    }

    const size_t MAX_PAT = (size_t)1 << 20, MAX_BYTES = (size_t)64 << 20;
    dsm::PatternReader reader([](char* b, size_t n) -> long { return (long)read(0, b, n); });
    dsm::PatternBatch cur, nxt;
    std::vector<uint64_t> counts;
    std::string out;
    double t_parse = 0, t_wait = 0, t_format = 0;
    typedef std::chrono::steady_clock clk;
    auto secs = [](clk::time_point a, clk::time_point b) { return std::chrono::duration<double>(b - a).count(); };
    int rc = 0;
    auto t0 = clk::now();
    bool have = reader.next(cur, MAX_PAT, MAX_BYTES);
    t_parse += secs(t0, clk::now());
    while (have && rc == 0) {
        counts.resize(cur.size() * nidx);
        int crc = 0;
        std::thread gpu([&]() { crc = dsm_counter_count(ctr, cur.bytes.data(), cur.offsets.data(), cur.size(), counts.data(), nullptr); });
        t0 = clk::now();
        const bool more = reader.next(nxt, MAX_PAT, MAX_BYTES);  // batch i+1 while batch i is on the card
        auto t1 = clk::now();
        gpu.join();
        auto t2 = clk::now();
        t_parse += secs(t0, t1);
        t_wait += secs(t1, t2);
        if (crc != 0) {
            fprintf(stderr, "dsm_count: %s\n", dsm_last_error());
            rc = 1;
            break;
        }
        out.clear();
        char num[48];
        for (size_t p = 0; p < cur.size(); ++p) {
            out.append((const char*)cur.bytes.data() + cur.offsets[p], cur.offsets[p + 1] - cur.offsets[p]);
            for (size_t i = 0; i < nidx; ++i) {
                const uint64_t v = counts[p * nidx + i];
                if (!all && v < fmin) continue;
                const int k = snprintf(num, sizeof num, " %zu:%llu", i, (unsigned long long)v);
                out.append(num, (size_t)k);
            }
            out.push_back('\n');
        }
        if (fwrite(out.data(), 1, out.size(), stdout) != out.size()) {
            fprintf(stderr, "dsm_count: write failed\n");
            rc = 1;
            break;
        }
        t_format += secs(t2, clk::now());
        std::swap(cur, nxt);
        have = more;
    }
    if (rc == 0 && reader.error()) {
        fprintf(stderr, "dsm_count: reading the patterns failed\n");
        rc = 1;
    }
    if (fflush(stdout) != 0) rc = 1;
    if (times) fprintf(stderr, "dsm_count: parse %.3f s, device wait %.3f s, format %.3f s\n", t_parse, t_wait, t_format);
    dsm_counter_destroy(ctr);
    close_all();
    return rc;
}
