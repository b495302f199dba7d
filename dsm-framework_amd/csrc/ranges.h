// ranges.h -- how the tiles of a mined level are dealt to the workgroups of the range sweep (engine.hip: range_sums_kernel,
// advance_single_kernel).  A level of nbp tiles is cut into R ranges of T consecutive tiles, T a multiple of 4; one workgroup takes
// a range, each of its four waves a quarter of it, front to back.  Plain integer arithmetic for host and device; checked on the CPU
// by tests/native/ranges_check.cpp.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DSM_RANGES_HD __host__ __device__ __forceinline__
#else
#define DSM_RANGES_HD inline
#endif

namespace dsm {

constexpr uint32_t RANGE_WAVES = 4;  // waves of a workgroup: sub-ranges of a range

struct RangeGeo {
    uint32_t R;  // workgroups launched; ranges at the end may own no tile
    uint32_t T;  // tiles per range
};

// nbp >= 1, rmax >= 1:  R = min(rmax, ceil(nbp / 4)),  T = 4 * ceil(nbp / (4 * R))
DSM_RANGES_HD RangeGeo range_geometry(uint32_t nbp, uint32_t rmax) {
    const uint32_t quads = (nbp + 3) / 4;
    RangeGeo g;
    g.R = rmax < quads ? rmax : quads;
    g.T = 4 * ((quads + g.R - 1) / g.R);
    return g;
}

// tiles [*t0, *t1) of wave w (0..3) of range b, clipped to the level (empty: *t0 == *t1)
DSM_RANGES_HD void range_wave_tiles(uint32_t T, uint32_t nbp, uint32_t b, uint32_t w, uint32_t* t0, uint32_t* t1) {
    const uint64_t first = (uint64_t)b * T + (uint64_t)w * (T / RANGE_WAVES), last = first + T / RANGE_WAVES;
    *t0 = (uint32_t)(first < nbp ? first : nbp);
    *t1 = (uint32_t)(last < nbp ? last : nbp);
}

}  // namespace dsm
