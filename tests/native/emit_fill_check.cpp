// CPU check of csrc/emit_fill.h: the host pass that gives one sample's chunk its entropies (and, from four-byte frequencies, its
// eight-byte ones), split over any number of callers, against a direct restatement of the exact one-reader entropy
// (metaserver.cpp:366-389 with one pair: log(1 + f) / log(2) - ((f + 1) * log(f + 1) / log(2)) / (1 + f), evaluated inline with libm).
// Also csrc/emit_runs.h with no pair array: only the path offsets of a run are rebased.  usage: emit_fill_check <cases> <seed>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../../dsm-framework_amd/csrc/emit_fill.h"
#include "../../dsm-framework_amd/csrc/emit_runs.h"

static const double LN2 = 0x1.62e42fefa39efp-1;  // the reference's log(2)
static const uint32_t TERM_TAB = 1u << 16, LOGN_TAB = 1u << 20;
static const uint8_t EV_DROP = 0, EV_KEEP = 1, EV_HOST = 2;

static double direct(uint64_t f) {
    const uint64_t sumN = 1 + f;
    double sumNlogN = 0;
    sumNlogN += (double)(f + 1) * log((double)(f + 1)) / LN2;
    return log((double)sumN) / LN2 - sumNlogN / (double)sumN;
}

int main(int argc, char** argv) {
    const int cases = argc > 1 ? atoi(argv[1]) : 300;
    std::mt19937_64 rng(argc > 2 ? atoll(argv[2]) : 1);
    // the tables exactly as the library builds them (entropy_tables.h); no slack behind them: a read past an end is the sanitizer's to see
    std::vector<double> terms(TERM_TAB), logn(LOGN_TAB);
    for (uint32_t f = 0; f < TERM_TAB; ++f) terms[f] = (double)((uint64_t)f + 1) * log((double)((uint64_t)f + 1)) / LN2;
    logn[0] = 0;
    for (uint32_t n = 1; n < LOGN_TAB; ++n) logn[n] = log((double)n) / LN2;
    const uint64_t edges[] = {1, 2, 511, 512, 65534, 65535, 0, 3, 255, 256, 4095, 4096, 32767, 32768};
    const double poison = -12345.678;
    long checked = 0;
    for (int it = 0; it < cases; ++it) {
        const uint32_t nt = it == 0 ? 64 : 1 + (uint32_t)(rng() % (it % 7 == 0 ? 5 : 5000));  // (case 0 holds every edge frequency)
        const bool narrow = it % 2 == 0;
        std::vector<uint64_t> f(nt), freqs(nt);
        std::vector<uint32_t> staged(nt);
        std::vector<uint8_t> keep(nt);
        std::vector<double> ent(nt, poison);
        for (uint32_t r = 0; r < nt; ++r) {
            const unsigned kind = (unsigned)(rng() % 8);
            if (kind == 0) f[r] = edges[rng() % (sizeof edges / sizeof edges[0])];
            else if (kind == 1) f[r] = TERM_TAB + rng() % (narrow ? 0xFFFF0000ull : (1ull << 40));  // beyond the tables: the host's libm path
            else f[r] = rng() % TERM_TAB;
            if (it == 0 && r < sizeof edges / sizeof edges[0]) f[r] = edges[r];
            keep[r] = f[r] >= TERM_TAB ? EV_HOST : (rng() % 9 == 0 ? EV_DROP : EV_KEEP);
            staged[r] = (uint32_t)f[r];
            freqs[r] = narrow ? 0xDEADBEEFDEADBEEFull : f[r];
        }
        const std::vector<uint8_t> keep0 = keep;
        // callers: nth ranges of `per` tuples as emit_job cuts them, in shuffled order
        const unsigned nth = 1 + (unsigned)(rng() % 17);
        const uint32_t per = (nt + nth - 1) / nth;
        std::vector<unsigned> order(nth);
        for (unsigned t = 0; t < nth; ++t) order[t] = t;
        for (unsigned t = nth; t > 1; --t) std::swap(order[t - 1], order[rng() % t]);
        for (unsigned k = 0; k < nth; ++k) {
            const unsigned t = order[k];
            const uint32_t lo = t * per < nt ? t * per : nt, hi = lo + per < nt ? lo + per : nt;
            dsm::fill_from_freqs(narrow ? staged.data() : nullptr, freqs.data(), ent.data(), keep.data(), EV_HOST, terms.data(), logn.data(), lo, hi);
        }
        for (uint32_t r = 0; r < nt; ++r) {
            if (freqs[r] != f[r]) { printf("frequency, case %d tuple %u: %llu want %llu\n", it, r, (unsigned long long)freqs[r], (unsigned long long)f[r]); return 1; }
            if (keep[r] != keep0[r]) { printf("verdict touched, case %d tuple %u\n", it, r); return 1; }
            if (keep0[r] == EV_HOST) {
                if (memcmp(&ent[r], &poison, 8) != 0) { printf("EV_HOST entry written, case %d tuple %u\n", it, r); return 1; }
                continue;
            }
            const double want = direct(f[r]);
            if (memcmp(&ent[r], &want, 8) != 0) { printf("entropy, case %d tuple %u f %llu: %a want %a\n", it, r, (unsigned long long)f[r], ent[r], want); return 1; }
            ++checked;
        }
    }
    // runs of kept tuples with one pair per tuple: the path offsets are rebased, no pair array is there to touch
    for (int it = 0; it < cases; ++it) {
        const uint32_t nt = 1 + (uint32_t)(rng() % 2000);
        std::vector<uint8_t> keep(nt);
        std::vector<uint32_t> plen(nt), rel_path(nt + 1);
        for (uint32_t r = 0; r < nt; ++r) { keep[r] = rng() % 40 == 0 ? EV_DROP : EV_KEEP; plen[r] = 1 + (uint32_t)(rng() % 40); }
        rel_path[0] = 0;
        for (uint32_t r = 0; r < nt; ++r) rel_path[r + 1] = rel_path[r] + plen[r];
        std::vector<uint32_t> seg;
        dsm::kept_runs(keep.data(), nt, EV_DROP, seg);
        const size_t ns = seg.size() / 2;
        std::vector<uint32_t> bp(ns), bq(ns);
        for (size_t i = 0; i < ns; ++i) { bp[i] = rel_path[seg[2 * i]]; bq[i] = seg[2 * i]; }
        const unsigned nth = 1 + (unsigned)(rng() % 17);
        const uint32_t per = (nt + nth - 1) / nth;
        for (unsigned t = nth; t-- > 0;) {
            const uint32_t lo = t * per < nt ? t * per : nt, hi = t + 1 == nth ? nt + 1 : (lo + per < nt ? lo + per : nt);
            dsm::rebase_runs(rel_path.data(), nullptr, seg, bp, bq, lo, hi);
        }
        for (size_t i = 0; i < ns; ++i) {
            uint32_t p = 0;
            for (uint32_t r = seg[2 * i]; r < seg[2 * i + 1]; ++r) {
                if (rel_path[r] != p) { printf("run offset, case %d run %zu tuple %u\n", it, i, r); return 1; }
                p += plen[r];
            }
            if (rel_path[seg[2 * i + 1]] != p) { printf("run closing entry, case %d run %zu\n", it, i); return 1; }
        }
    }
    printf("ok %d cases %ld entropies\n", cases, checked);
    return 0;
}
