// emit_fill.h -- what a chunk of one sample's tuples does not carry over the bus (engine.hip, emit_job).  Every tuple has one pair, so
// its exact entropy (metaserver.cpp:366-389) is a function of its frequency f alone: logn[1 + f] - terms[f] / (double)(1 + f), the
// table entries of entropy_tables.h, one division and one subtraction in IEEE double -- the very double the fill kernel compared with
// emin / emax.  With 32-bit positions the frequency itself arrives as four bytes and is widened here.  Host code, no device types: the
// arithmetic is checked on the CPU (tests/native/emit_fill_check.cpp).
#pragma once
#include <cstdint>

namespace dsm {

// Tuples lo .. hi - 1 of a chunk.  staged: the frequencies as they crossed the bus, widened into freqs (null: freqs holds them already).
// ent[r] is written unless keep[r] == host: such a tuple's frequency lies beyond the tables (terms has term_tab entries, logn more than
// term_tab), its entropy is libm's to compute.  Ranges of different callers may be disjoint pieces of the chunk in any order.
inline void fill_from_freqs(const uint32_t* staged, uint64_t* freqs, double* ent, const uint8_t* keep, uint8_t host, const double* terms,
                            const double* logn, uint32_t lo, uint32_t hi) {
    for (uint32_t r = lo; r < hi; ++r) {
        const uint64_t f = staged ? (uint64_t)staged[r] : freqs[r];
        if (staged) freqs[r] = f;
        if (keep[r] != host) ent[r] = logn[1 + f] - terms[f] / (double)(1 + f);
    }
}

}  // namespace dsm
