// count.hip -- occurrence counts of given patterns in every index of a counter: batched backward search on the plane
// layout (gfx950).  FMIndex::Search (FMIndex.cpp:360-382) and the step of Query.h:37-45, for many (pattern, sample) pairs
// in one launch.
//
// A pattern's bytes are pushed left to right from the root interval.  The interval is kept half open, [sp, e):
//   sp' = C[c] + occ(c, sp),  e' = C[c] + occ(c, e)        (occ(c, x) = occurrences of c in BWT[0, x))
// which is sp' = LF(c, sp - 1), ep' = LF(c, ep) - 1 with e = ep + 1.  When sp and e fall in one 128-symbol block, one 64-byte
// load answers both ranks.
//
// Work: the items (pattern p, index i) = p * nidx + i.  The grid is persistent (sized to the card's resident waves); each wave
// takes items GRAB at a time from a global counter, and a lane that finishes its item takes the next one from the wave's
// range before the next step, so patterns of mixed lengths do not leave lanes idle until the longest one ends.
//
// The k-mer table of an index holds (sp, count) of every ACGT string of length 1..k, level j computed from level j-1 by one
// step per entry.  A pattern whose first min(k, len) bytes are bases starts from it: the first, widest steps (the ones whose
// two ranks lie in different blocks) are never taken.
#include <cstring>
#include <memory>
#include <vector>

#include "common.h"

namespace dsm {

constexpr int COUNT_KMAX = 12;        // 4^13 / 3 entries of 16 bytes = 358 MB per index at most
constexpr int COUNT_KDEFAULT = 10;    // 1.4e6 entries = 22 MB per index
constexpr int COUNT_T = 256;          // threads per block
constexpr u32 COUNT_GRAB = 64;        // items a wave takes from the global counter at once

struct CountIdx {      // one index as the count kernel sees it
    const Blk* blk;
    const u64* sbase;  // C[] of the bases folded in
    const u64* rare;
    const u64* tab;    // k-mer table [(4^(k+1) - 4) / 3][2] = {sp, count}, or null
    u64 n;
    u64 Crare[4];      // C[] of codes 4..7
    u32 rare_bytes;    // code2byte[4 + j] in bits 8j..8j+7
    u32 nrare;         // codes in use beyond the four bases
};

// statistics words after the work counter (dsm_count_stats order)
enum { W_NEXT = 0, W_LF_STEPS, W_BLOCK_LOADS, W_WAVE_STEPS, W_LANE_STEPS, W_TABLE_STARTS, W_RARE_BLOCKS, W_WORDS };

__device__ __forceinline__ int count_code(u32 rare_bytes, u32 nrare, u32 b) {
    switch (b) {
        case 'A': return 0;
        case 'C': return 1;
        case 'G': return 2;
        case 'T': return 3;
    }
    for (u32 j = 0; j < nrare; ++j)
        if (((rare_bytes >> (8 * j)) & 0xFF) == b) return 4 + (int)j;
    return -1;  // the index does not contain the byte
}

// occurrences of base `code` (0..3) among the first `off` symbols of a block in registers
__device__ __forceinline__ u32 blk_count1(const Blk16& r, u32 off, u32 code) {
    u64 ma = off >= 64 ? ~0ull : ((1ull << off) - 1);
    u64 mb = off > 64 ? ((1ull << (off - 64)) - 1) : 0ull;
    u64 a = ma & ~r.p2a & ((code & 1) ? r.p0a : ~r.p0a) & ((code & 2) ? r.p1a : ~r.p1a);
    u64 b = mb & ~r.p2b & ((code & 1) ? r.p0b : ~r.p0b) & ((code & 2) ? r.p1b : ~r.p1b);
    u32 c = code == 0 ? r.cnt[0] : code == 1 ? r.cnt[1] : code == 2 ? r.cnt[2] : r.cnt[3];  // (no runtime-indexed array)
    return c + (u32)__popcll(a) + (u32)__popcll(b);
}

// occurrences of code 4..7 in BWT[0, x): the sampled absolute count and the blocks since the sample (planes_count's rare path)
__device__ __forceinline__ u64 rare_occ(const Blk* __restrict__ blk, const u64* __restrict__ rare, u32 code, u64 pos, u64& blocks) {
    const u64 bi = pos >> BLK_SHIFT;
    const u32 off = (u32)(pos & (BLK_SYMS - 1));
    const u64 s = bi >> RARE_SAMPLE_SHIFT;
    u64 cnt = rare[s * 4 + (code - 4)];
    for (u64 b = s << RARE_SAMPLE_SHIFT; b <= bi; ++b) {
        const Blk& k = blk[b];
        const u32 lim = b == bi ? off : BLK_SYMS;
#pragma unroll
        for (int w = 0; w < 2; ++w) {
            const u32 lo = w * 64;
            const u64 mask = lim >= lo + 64 ? ~0ull : (lim > lo ? ((1ull << (lim - lo)) - 1) : 0ull);
            u64 m = mask & k.pl[2][w];
            m &= (code & 1) ? k.pl[0][w] : ~k.pl[0][w];
            m &= (code & 2) ? k.pl[1][w] : ~k.pl[1][w];
            cnt += __popcll(m);
        }
        ++blocks;
    }
    return cnt;
}

// One push of code c on [sp, e).  Returns the number of 64-byte block loads of the base path (1 or 2).  The rare-code path reads
// its fields from *rx; the base path needs only the blocks and the superblock bases, kept in registers by the caller.
__device__ __forceinline__ u32 count_step(const Blk* __restrict__ blk, const u64* __restrict__ sbase, const CountIdx* __restrict__ rx, int c,
                                         u64& sp, u64& e, u64& rare_blocks) {
    if (c >= 4) {
        const u64 Cc = rx->Crare[c - 4];
        const u64* rare = rx->rare;
        const u64 a = rare_occ(blk, rare, (u32)c, sp, rare_blocks), b = rare_occ(blk, rare, (u32)c, e, rare_blocks);
        sp = Cc + a;
        e = Cc + b;
        return 0;
    }
    const u64 b1 = sp >> BLK_SHIFT, b2 = e >> BLK_SHIFT;
    const bool two = b1 != b2;
    Blk16 r1, r2;
    load_blk(blk, b1, r1);
    if (two) load_blk(blk, b2, r2);
    const u64 s1 = sbase[(sp >> SB_SHIFT) * 4 + c];
    const u64 s2 = (sp >> SB_SHIFT) == (e >> SB_SHIFT) ? s1 : sbase[(e >> SB_SHIFT) * 4 + c];
    const u32 o1 = blk_count1(r1, (u32)(sp & (BLK_SYMS - 1)), (u32)c);
    const u32 o2 = two ? blk_count1(r2, (u32)(e & (BLK_SYMS - 1)), (u32)c) : blk_count1(r1, (u32)(e & (BLK_SYMS - 1)), (u32)c);
    sp = s1 + o1;
    e = s2 + o2;
    return two ? 2u : 1u;
}

// level j of the k-mer table from level j - 1 (level 0 = the root): entry v of level j is the string whose base-4 digits,
// first byte most significant, are v
__global__ __launch_bounds__(256) void kmer_level_kernel(const CountIdx* __restrict__ ixp, int j) {
    const u64 nj = 1ull << (2 * j);
    const u64 v = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= nj) return;
    const Blk* blk = ixp->blk;
    const u64* sbase = ixp->sbase;
    u64* tab = const_cast<u64*>(ixp->tab);
    const u64 lvl = ((1ull << (2 * j)) - 4) / 3, plvl = j > 1 ? ((1ull << (2 * (j - 1))) - 4) / 3 : 0;
    u64 sp = 0, e = ixp->n;
    if (j > 1) {
        sp = tab[2 * (plvl + (v >> 2))];
        e = sp + tab[2 * (plvl + (v >> 2)) + 1];
    }
    if (e > sp) {
        u64 rb = 0;
        count_step(blk, sbase, ixp, (int)(v & 3), sp, e, rb);
    }
    tab[2 * (lvl + v)] = e > sp ? sp : 0;
    tab[2 * (lvl + v) + 1] = e > sp ? e - sp : 0;
}

__global__ __launch_bounds__(COUNT_T) void count_kernel(const CountIdx* __restrict__ ixs, u32 nidx, const u8* __restrict__ bytes,
                                                        const u64* __restrict__ offsets, u64 obase, u64 npat, int kmer,
                                                        u64* __restrict__ counts, u64* __restrict__ sps, u64* __restrict__ work) {
    const u64 total = npat * nidx;
    const u32 lane = threadIdx.x & 63;
    const u64 lt = (1ull << lane) - 1;
    u64 q_next = 0, q_end = 0;  // the wave's range of items (wave-uniform)
    bool drained = false;
    bool active = false;
    u64 item = 0, pb = 0, len = 0, pos = 0, sp = 0, e = 0;
    u32 nb = 0;  // the pattern's byte at pos, fetched a step ahead
    const Blk* blk = nullptr;
    const u64* sbase = nullptr;
    const CountIdx* rx = nullptr;
    u32 rare_bytes = 0, nrare = 0;
    u64 wave_steps = 0, lane_steps = 0, loads = 0, steps = 0, tstarts = 0, rare_blocks = 0;
    for (;;) {
        // idle lanes take the next items of the wave's range; the range is refilled GRAB items at a time
        for (u64 idle = __ballot(!active); idle && !drained; idle = __ballot(!active)) {
            if (q_next >= q_end) {
                u64 g = 0;
                if (lane == (u32)__ffsll((long long)idle) - 1) g = atomicAdd((unsigned long long*)&work[W_NEXT], (unsigned long long)COUNT_GRAB);
                g = __shfl(g, __ffsll((long long)idle) - 1);
                if (g >= total) { drained = true; break; }
                q_next = g;
                q_end = g + COUNT_GRAB < total ? g + COUNT_GRAB : total;
            }
            const u64 avail = q_end - q_next;
            const u32 rank = (u32)__popcll(idle & lt);
            if (!active && rank < avail) {
                item = q_next + rank;
                const u64 p = item / nidx;
                rx = ixs + (item - p * nidx);
                const CountIdx x = *rx;
                blk = x.blk;
                sbase = x.sbase;
                rare_bytes = x.rare_bytes;
                nrare = x.nrare;
                pb = offsets[p] - obase;
                len = offsets[p + 1] - obase - pb;
                sp = 0;
                e = x.n;
                pos = 0;
                if (kmer > 0 && len > 0 && x.tab) {
                    const u32 m = len < (u64)kmer ? (u32)len : (u32)kmer;
                    u64 v = 0;
                    bool bases = true;
#pragma unroll
                    for (int j = 0; j < COUNT_KMAX; ++j) {
                        if ((u32)j < m) {
                            const u32 b = bytes[pb + j];
                            const int c = b == 'A' ? 0 : b == 'C' ? 1 : b == 'G' ? 2 : b == 'T' ? 3 : -1;
                            bases &= c >= 0;
                            v = (v << 2) | (u64)(c & 3);
                        }
                    }
                    if (bases) {
                        const u64 at = ((1ull << (2 * m)) - 4) / 3 + v;
                        sp = x.tab[2 * at];
                        e = sp + x.tab[2 * at + 1];
                        pos = m;
                        ++tstarts;
                    }
                }
                if (pos < len && e > sp) {
                    nb = bytes[pb + pos];
                    active = true;
                } else {  // done before the first step: the empty pattern, a table hit that covers it, or an empty interval
                    counts[item] = e - sp;
                    if (sps) sps[item] = sp;
                }
            }
            q_next += avail < (u64)__popcll(idle) ? avail : (u64)__popcll(idle);
        }
        const u64 act = __ballot(active);
        if (!act) break;
        ++wave_steps;
        lane_steps += (u64)__popcll(act);
        if (active) {
            const int c = count_code(rare_bytes, nrare, nb);
            ++pos;
            if (pos < len) nb = bytes[pb + pos];  // issued ahead of the block loads: it does not wait for them
            if (c < 0) {
                e = sp;  // a byte the index does not contain
            } else {
                loads += count_step(blk, sbase, rx, c, sp, e, rare_blocks);
                ++steps;
            }
            if (pos >= len || e <= sp) {
                counts[item] = e > sp ? e - sp : 0;
                if (sps) sps[item] = sp;
                active = false;
            }
        }
    }
    // statistics: lane sums reduced over the wave, one atomic per word and wave
    for (int s = 32; s > 0; s >>= 1) {
        loads += __shfl_xor(loads, s);
        steps += __shfl_xor(steps, s);
        tstarts += __shfl_xor(tstarts, s);
        rare_blocks += __shfl_xor(rare_blocks, s);
    }
    if (lane == 0 && wave_steps) {
        atomicAdd((unsigned long long*)&work[W_LF_STEPS], (unsigned long long)steps);
        atomicAdd((unsigned long long*)&work[W_BLOCK_LOADS], (unsigned long long)loads);
        atomicAdd((unsigned long long*)&work[W_WAVE_STEPS], (unsigned long long)wave_steps);
        atomicAdd((unsigned long long*)&work[W_LANE_STEPS], (unsigned long long)lane_steps);
        atomicAdd((unsigned long long*)&work[W_TABLE_STARTS], (unsigned long long)tstarts);
        atomicAdd((unsigned long long*)&work[W_RARE_BLOCKS], (unsigned long long)rare_blocks);
    } else if (lane == 0 && tstarts) {
        atomicAdd((unsigned long long*)&work[W_TABLE_STARTS], (unsigned long long)tstarts);
    }
}

}  // namespace dsm

using namespace dsm;

struct dsm_counter {
    std::vector<const dsm_index*> idx;
    int device = 0;
    int kmer = 0;
    std::vector<void*> tabs;          // one k-mer table per index
    std::vector<CountIdx> host_ix;    // what d_ix holds (the block pointers change when an index is offloaded and reloaded)
    CountIdx* d_ix = nullptr;
    u64* d_work = nullptr;            // [W_WORDS]: statistics accumulate until dsm_counter_stats resets them
    int grid = 0;                     // resident blocks of count_kernel
    u64 patterns = 0, items = 0;      // host-side statistics
    // host call: device and pinned buffers, grown on demand
    hipStream_t st = nullptr;
    u8* d_bytes = nullptr; u64* d_off = nullptr; u64* d_cnt = nullptr; u64* d_sp = nullptr;
    u8* h_bytes = nullptr; u64* h_off = nullptr; u64* h_cnt = nullptr; u64* h_sp = nullptr;
    size_t cap_bytes = 0, cap_pat = 0;
    ~dsm_counter() {
        (void)hipSetDevice(device);
        for (void* t : tabs) if (t) (void)hipFree(t);
        if (d_ix) (void)hipFree(d_ix);
        if (d_work) (void)hipFree(d_work);
        for (void* p : {(void*)d_bytes, (void*)d_off, (void*)d_cnt, (void*)d_sp}) if (p) (void)hipFree(p);
        for (void* p : {(void*)h_bytes, (void*)h_off, (void*)h_cnt, (void*)h_sp}) if (p) (void)hipHostFree(p);
        if (st) (void)hipStreamDestroy(st);
    }
};

namespace {

constexpr size_t HOST_CHUNK_BYTES = 32u << 20;   // pattern bytes per chunk of the host call
constexpr size_t HOST_CHUNK_ITEMS = 4u << 20;    // (pattern, index) pairs per chunk of the host call

CountIdx make_count_idx(const dsm_index* ix, const void* tab) {
    CountIdx c;
    memset(&c, 0, sizeof c);
    c.blk = ix->dev.blk;
    c.sbase = ix->dev.sbase;
    c.rare = ix->dev.rare;
    c.tab = (const u64*)tab;
    c.n = ix->meta.n;
    c.nrare = (u32)(ix->meta.ncodes - 4);
    for (u32 j = 0; j < c.nrare; ++j) {
        c.Crare[j] = ix->meta.C[ix->meta.code2byte[4 + j]];
        c.rare_bytes |= (u32)ix->meta.code2byte[4 + j] << (8 * j);
    }
    return c;
}

int check_resident(dsm_counter* k) {
    bool changed = false;
    for (size_t i = 0; i < k->idx.size(); ++i) {
        if (!k->idx[i]->dev.blk) return fail(DSM_E_INVAL, "dsm_counter: an index is offloaded: dsm_index_reload first");
        if (k->host_ix[i].blk != k->idx[i]->dev.blk) { k->host_ix[i].blk = k->idx[i]->dev.blk; changed = true; }
    }
    if (changed) DSM_HIP(hipMemcpy(k->d_ix, k->host_ix.data(), k->host_ix.size() * sizeof(CountIdx), hipMemcpyHostToDevice));
    return 0;
}

int count_dev(dsm_counter* k, const u8* d_bytes, const u64* d_off, u64 obase, size_t npat, u64* d_counts, u64* d_sp, hipStream_t st) {
    if (npat == 0) return DSM_OK;
    if (int rc = check_resident(k)) return rc;
    const u64 total = (u64)npat * k->idx.size();
    const u64 waves = (total + COUNT_GRAB - 1) / COUNT_GRAB;
    const u64 blocks = (waves + COUNT_T / 64 - 1) / (COUNT_T / 64);
    const unsigned grid = (unsigned)(blocks < (u64)k->grid ? blocks : (u64)k->grid);
    DSM_HIP(hipMemsetAsync(k->d_work, 0, sizeof(u64), st));  // the work counter; the statistics words accumulate
    hipLaunchKernelGGL(count_kernel, dim3(grid), dim3(COUNT_T), 0, st, k->d_ix, (u32)k->idx.size(), d_bytes, d_off, obase, (u64)npat,
                       k->kmer, d_counts, d_sp, k->d_work);
    DSM_HIP(hipGetLastError());
    k->patterns += npat;
    k->items += total;
    return DSM_OK;
}

template <class T>
int grow_dev(T*& p, size_t n) {
    if (p) (void)hipFree(p);
    p = nullptr;
    if (hipMalloc((void**)&p, (n ? n : 1) * sizeof(T)) != hipSuccess) { p = nullptr; return fail(DSM_E_NOMEM, "dsm_counter: hipMalloc failed"); }
    return 0;
}
template <class T>
int grow_host(T*& p, size_t n) {
    if (p) (void)hipHostFree(p);
    p = nullptr;
    if (hipHostMalloc((void**)&p, (n ? n : 1) * sizeof(T)) != hipSuccess) { p = nullptr; return fail(DSM_E_NOMEM, "dsm_counter: hipHostMalloc failed"); }
    return 0;
}

}  // namespace

extern "C" {

int dsm_counter_create(dsm_index* const* idx, int nidx, int kmer, dsm_counter** out) {
    if (!out) return fail(DSM_E_INVAL, "dsm_counter_create: null argument");
    *out = nullptr;
    if (!idx || nidx <= 0) return fail(DSM_E_INVAL, "dsm_counter_create: no index");
    if (kmer < -1 || kmer > COUNT_KMAX) return fail(DSM_E_INVAL, "dsm_counter_create: kmer must be -1 (default), 0 (off) or 1..12");
    for (int i = 0; i < nidx; ++i) {
        if (!idx[i]) return fail(DSM_E_INVAL, "dsm_counter_create: null index");
        if (idx[i]->device != idx[0]->device) return fail(DSM_E_INVAL, "dsm_counter_create: the indexes are on different devices");
        if (!idx[i]->dev.blk) return fail(DSM_E_INVAL, "dsm_counter_create: an index is offloaded: dsm_index_reload first");
    }
    std::unique_ptr<dsm_counter> k(new dsm_counter());
    k->device = idx[0]->device;
    k->kmer = kmer < 0 ? COUNT_KDEFAULT : kmer;
    DSM_HIP(hipSetDevice(k->device));
    DSM_HIP(hipStreamCreateWithFlags(&k->st, hipStreamNonBlocking));
    for (int i = 0; i < nidx; ++i) k->idx.push_back(idx[i]);
    k->tabs.assign(nidx, nullptr);
    DSM_HIP(hipMalloc((void**)&k->d_work, W_WORDS * sizeof(u64)));
    DSM_HIP(hipMemsetAsync(k->d_work, 0, W_WORDS * sizeof(u64), k->st));
    for (int i = 0; i < nidx; ++i) {
        void* tab = nullptr;
        if (k->kmer > 0) {
            const u64 entries = ((1ull << (2 * (k->kmer + 1))) - 4) / 3;
            if (hipMalloc(&tab, entries * 16) != hipSuccess) return fail(DSM_E_NOMEM, "dsm_counter_create: hipMalloc (k-mer table) failed");
            k->tabs[i] = tab;
        }
        k->host_ix.push_back(make_count_idx(idx[i], tab));
    }
    DSM_HIP(hipMalloc((void**)&k->d_ix, nidx * sizeof(CountIdx)));
    DSM_HIP(hipMemcpyAsync(k->d_ix, k->host_ix.data(), nidx * sizeof(CountIdx), hipMemcpyHostToDevice, k->st));
    for (int i = 0; i < nidx; ++i)
        for (int j = 1; j <= k->kmer; ++j) {
            const u64 nj = 1ull << (2 * j);
            hipLaunchKernelGGL(kmer_level_kernel, dim3((unsigned)((nj + 255) / 256)), dim3(256), 0, k->st, (const CountIdx*)(k->d_ix + i), j);
        }
    DSM_HIP(hipGetLastError());
    DSM_HIP(hipStreamSynchronize(k->st));
    int per_cu = 0, cus = 0;
    DSM_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, count_kernel, COUNT_T, 0));
    DSM_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, k->device));
    k->grid = (per_cu > 0 ? per_cu : 1) * (cus > 0 ? cus : 1);
    *out = k.release();
    return DSM_OK;
}

int dsm_counter_count_dev(dsm_counter* k, const uint8_t* d_bytes, const uint64_t* d_offsets, size_t npat, uint64_t* d_counts,
                          uint64_t* d_sp, void* stream) {
    if (!k) return fail(DSM_E_INVAL, "dsm_counter_count_dev: null counter");
    if (npat && (!d_bytes || !d_offsets || !d_counts)) return fail(DSM_E_INVAL, "dsm_counter_count_dev: null argument");
    DSM_HIP(hipSetDevice(k->device));
    return count_dev(k, d_bytes, d_offsets, 0, npat, d_counts, d_sp, (hipStream_t)stream);
}

int dsm_counter_count(dsm_counter* k, const uint8_t* bytes, const uint64_t* offsets, size_t npat, uint64_t* counts, uint64_t* sp) {
    if (!k) return fail(DSM_E_INVAL, "dsm_counter_count: null counter");
    if (npat && (!offsets || !counts)) return fail(DSM_E_INVAL, "dsm_counter_count: null argument");
    if (npat && offsets[npat] > offsets[0] && !bytes) return fail(DSM_E_INVAL, "dsm_counter_count: null bytes");
    DSM_HIP(hipSetDevice(k->device));
    const size_t nidx = k->idx.size();
    const size_t max_pat = HOST_CHUNK_ITEMS / nidx > 0 ? HOST_CHUNK_ITEMS / nidx : 1;
    for (size_t p0 = 0; p0 < npat;) {
        if (offsets[p0 + 1] < offsets[p0]) return fail(DSM_E_INVAL, "dsm_counter_count: offsets decrease");
        // the chunk: at most max_pat patterns and HOST_CHUNK_BYTES bytes (a longer single pattern goes alone)
        size_t p1 = p0 + 1;
        while (p1 < npat && p1 - p0 < max_pat && offsets[p1 + 1] >= offsets[p1] && offsets[p1 + 1] - offsets[p0] <= HOST_CHUNK_BYTES) ++p1;
        const size_t np = p1 - p0;
        const u64 nb = offsets[p1] - offsets[p0];
        if (nb > k->cap_bytes) {
            if (int rc = grow_dev(k->d_bytes, nb)) return rc;
            if (int rc = grow_host(k->h_bytes, nb)) return rc;
            k->cap_bytes = nb;
        }
        if (np > k->cap_pat) {
            const size_t c = max_pat;
            if (int rc = grow_dev(k->d_off, c + 1)) return rc;
            if (int rc = grow_dev(k->d_cnt, c * nidx)) return rc;
            if (int rc = grow_dev(k->d_sp, c * nidx)) return rc;
            if (int rc = grow_host(k->h_off, c + 1)) return rc;
            if (int rc = grow_host(k->h_cnt, c * nidx)) return rc;
            if (int rc = grow_host(k->h_sp, c * nidx)) return rc;
            k->cap_pat = c;
        }
        if (nb) memcpy(k->h_bytes, bytes + offsets[p0], nb);
        memcpy(k->h_off, offsets + p0, (np + 1) * sizeof(u64));
        if (nb) DSM_HIP(hipMemcpyAsync(k->d_bytes, k->h_bytes, nb, hipMemcpyHostToDevice, k->st));
        DSM_HIP(hipMemcpyAsync(k->d_off, k->h_off, (np + 1) * sizeof(u64), hipMemcpyHostToDevice, k->st));
        if (int rc = count_dev(k, k->d_bytes, k->d_off, offsets[p0], np, k->d_cnt, sp ? k->d_sp : nullptr, k->st)) return rc;
        DSM_HIP(hipMemcpyAsync(k->h_cnt, k->d_cnt, np * nidx * sizeof(u64), hipMemcpyDeviceToHost, k->st));
        if (sp) DSM_HIP(hipMemcpyAsync(k->h_sp, k->d_sp, np * nidx * sizeof(u64), hipMemcpyDeviceToHost, k->st));
        DSM_HIP(hipStreamSynchronize(k->st));
        memcpy(counts + p0 * nidx, k->h_cnt, np * nidx * sizeof(u64));
        if (sp) memcpy(sp + p0 * nidx, k->h_sp, np * nidx * sizeof(u64));
        p0 = p1;
    }
    return DSM_OK;
}

int dsm_counter_stats(dsm_counter* k, dsm_count_stats* out, int reset) {
    if (!k || !out) return fail(DSM_E_INVAL, "dsm_counter_stats: null argument");
    DSM_HIP(hipSetDevice(k->device));
    u64 w[W_WORDS];
    DSM_HIP(hipDeviceSynchronize());  // calls enqueued on any stream have finished
    DSM_HIP(hipMemcpy(w, k->d_work, sizeof w, hipMemcpyDeviceToHost));
    memset(out, 0, sizeof *out);
    out->patterns = k->patterns;
    out->items = k->items;
    out->lf_steps = w[W_LF_STEPS];
    out->block_loads = w[W_BLOCK_LOADS];
    out->wave_steps = w[W_WAVE_STEPS];
    out->lane_steps = w[W_LANE_STEPS];
    out->table_starts = w[W_TABLE_STARTS];
    out->rare_blocks = w[W_RARE_BLOCKS];
    out->kmer = (uint32_t)k->kmer;
    out->table_bytes = k->kmer > 0 ? (((1ull << (2 * (k->kmer + 1))) - 4) / 3) * 16 * k->idx.size() : 0;
    if (reset) {
        DSM_HIP(hipMemset(k->d_work, 0, sizeof w));
        k->patterns = k->items = 0;
    }
    return DSM_OK;
}

void dsm_counter_destroy(dsm_counter* k) { delete k; }

}  // extern "C"
