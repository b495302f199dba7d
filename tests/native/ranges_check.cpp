// CPU check of csrc/ranges.h: how the tiles of a level are dealt to the workgroups and waves of the range sweep.  For every number of
// tiles 2..5000 and every cap on the ranges in {1, 3, 7, 1024}: R = min(cap, ceil(nbp / 4)), T = 4 * ceil(nbp / (4 * R)); the waves'
// intervals, taken in the order (range, wave), are disjoint, ordered and cover [0, nbp) exactly; no interval is longer than T / 4; what
// lies behind the level is empty.  usage: ranges_check [max_tiles]
#include <cstdio>
#include <cstdlib>

#include "../../dsm-framework_amd/csrc/ranges.h"

int main(int argc, char** argv) {
    const uint32_t max_tiles = argc > 1 ? (uint32_t)atol(argv[1]) : 5000;
    const uint32_t caps[] = {1, 3, 7, 1024};
    long checked = 0;
    for (uint32_t cap : caps) {
        for (uint32_t nbp = 2; nbp <= max_tiles; ++nbp) {
            const dsm::RangeGeo g = dsm::range_geometry(nbp, cap);
            const uint32_t quads = (nbp + 3) / 4;
            const uint32_t wantR = cap < quads ? cap : quads;
            uint32_t wantT = 0;
            while ((uint64_t)wantT * wantR < nbp) wantT += 4;   // the smallest multiple of 4 with R * T >= nbp
            if (g.R != wantR || g.T != wantT || g.R < 1 || g.R > cap || g.T % 4 != 0) {
                printf("geometry: nbp %u cap %u -> R %u T %u, expected R %u T %u\n", nbp, cap, g.R, g.T, wantR, wantT);
                return 1;
            }
            uint32_t next = 0;
            bool short_seen = false;   // once a wave's interval was clipped, every later one is empty
            for (uint32_t b = 0; b < g.R; ++b) {
                for (uint32_t w = 0; w < dsm::RANGE_WAVES; ++w) {
                    uint32_t t0 = ~0u, t1 = ~0u;
                    dsm::range_wave_tiles(g.T, nbp, b, w, &t0, &t1);
                    const bool empty = t0 == t1;
                    if (t0 > t1 || t1 > nbp || t1 - t0 > g.T / 4 || (!empty && t0 != next) || (empty && next != nbp && t0 != next) ||
                        (short_seen && !empty)) {
                        printf("interval: nbp %u cap %u range %u wave %u -> [%u, %u), expected to start at %u\n", nbp, cap, b, w, t0, t1, next);
                        return 1;
                    }
                    if (t1 - t0 < g.T / 4) short_seen = true;
                    if (!empty) next = t1;
                    ++checked;
                }
            }
            if (next != nbp) {
                printf("cover: nbp %u cap %u: the intervals end at %u\n", nbp, cap, next);
                return 1;
            }
        }
    }
    printf("ok %ld intervals\n", checked);
    return 0;
}
