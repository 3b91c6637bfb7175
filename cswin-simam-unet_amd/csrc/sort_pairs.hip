// Stable segmented LSD radix sort of (u32 key, u32 value) pairs on the device: the descending order of the
// per-pixel errors that the Lovasz-Softmax loss needs (csu_seg_lovasz_*, csrc/seg_ce.hip).  The reference has no
// counterpart.
//   `segments` contiguous runs of `len` pairs are sorted independently, ascending by the low key_bits bits of the
//   key, 8 bits per pass from the bottom; equal keys keep their order.  A tile is TILE = 2048 consecutive pairs of
//   one segment (the last one of a segment may be ragged), one workgroup ranks one tile at a time; tiles beyond
//   the grid are walked grid-stride.  Per pass, three launches:
//   sp_hist     the digit histogram of every tile in LDS counters -> hist[segment][digit][tile].  Every entry is
//               written, so nothing is cleared and there are no atomics on global memory.
//   sp_scan     one workgroup per (segment, digit): the exclusive scan of that row over the tiles, in place, and
//               the row's total -> tot[segment][digit].
//   sp_scatter  the exclusive scan of the segment's 256 totals (every workgroup forms it again), then the rank of
//               each pair among the pairs of its digit in the tile, in the tile's order: wave w owns the pairs
//               [512 w, 512 w + 512) and takes them 64 at a time; the lanes of one digit find each other with
//               eight ballots, a lane's rank is the digit's running count of the wave (an LDS counter only the
//               digit's first lane updates) plus the lanes of its digit below it.  The counts of the waves before
//               it and the two scans give the destination.
// Integer arithmetic only: the result is a function of the input alone and bitwise repeatable.  Every loop runs to
// a bound passed from the host.  A pass whose digit lies wholly above key_bits does not run; an odd number of
// passes ends with a copy from the scratch buffers.
#include "common.hpp"

#include <utility>

namespace csu {
namespace {

constexpr int NT = 256;
constexpr int BINS = 256;
constexpr int EPT = 8;                  // pairs per thread
constexpr int TILE = NT * EPT;          // 2048
constexpr int WCHUNK = TILE / (NT / 64);   // a wave's consecutive pairs
constexpr int SP_BLOCKS = 1 << 18;
typedef unsigned u32;
typedef unsigned long long u64;

struct SpArgs {
    long len, ntiles, items;   // items = segments * ntiles
    u32 kmask;
    int shift;
};

__device__ __forceinline__ u32 sp_digit(u32 key, const SpArgs& a) { return ((key & a.kmask) >> a.shift) & (BINS - 1); }

__global__ __launch_bounds__(NT) void sp_hist(const u32* __restrict__ keys, SpArgs a, u32* __restrict__ hist) {
    __shared__ u32 lh[BINS];
    const int tid = threadIdx.x;
    for (long it = blockIdx.x; it < a.items; it += gridDim.x) {
        const long seg = it / a.ntiles, tile = it - seg * a.ntiles;
        const long first = tile * TILE;
        const int n = (int)min((long)TILE, a.len - first);
        const u32* k = keys + seg * a.len + first;
        lh[tid] = 0;
        __syncthreads();
        for (int i = tid; i < n; i += NT) atomicAdd(&lh[sp_digit(k[i], a)], 1u);
        __syncthreads();
        hist[(seg * BINS + tid) * a.ntiles + tile] = lh[tid];
        __syncthreads();
    }
}

// rows = segments * BINS rows of ntiles counts
__global__ __launch_bounds__(NT) void sp_scan(u32* __restrict__ hist, u32* __restrict__ tot, long rows, long ntiles) {
    __shared__ u32 wsum[NT / 64];
    for (long r = blockIdx.x; r < rows; r += gridDim.x) {
        u32* row = hist + r * ntiles;
        u32 carry = 0;
        for (long c0 = 0; c0 < ntiles; c0 += NT) {
            const long i = c0 + threadIdx.x;
            const u32 v = i < ntiles ? row[i] : 0u;
            u32 total;
            const u32 inc = block_scan<NT>(v, wsum, total);
            if (i < ntiles) row[i] = carry + inc - v;
            carry += total;
        }
        if (threadIdx.x == 0) tot[r] = carry;
    }
}

__global__ __launch_bounds__(NT) void sp_scatter(const u32* __restrict__ keys, const u32* __restrict__ vals, SpArgs a,
                                                 const u32* __restrict__ hist, const u32* __restrict__ tot,
                                                 u32* __restrict__ okeys, u32* __restrict__ ovals) {
    __shared__ u32 run[NT / 64][BINS];
    __shared__ u32 wsum[NT / 64];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    for (long it = blockIdx.x; it < a.items; it += gridDim.x) {
        const long seg = it / a.ntiles, tile = it - seg * a.ntiles;
        const long first = tile * TILE;
        const int n = (int)min((long)TILE, a.len - first);
        const u32* k = keys + seg * a.len + first;
        const u32* v = vals + seg * a.len + first;
        // where digit tid of this tile starts in the segment: the digits below it, then the tiles before this one
        const u32 dt = tot[seg * BINS + tid];
        u32 total;
        const u32 dbase = block_scan<NT>(dt, wsum, total) - dt + hist[(seg * BINS + tid) * a.ntiles + tile];
#pragma unroll
        for (int j = 0; j < NT / 64; ++j) run[j][tid] = 0;
        __syncthreads();
        volatile u32* rw = run[w];
        u32 key[EPT], val[EPT], rank[EPT];
#pragma unroll
        for (int r = 0; r < EPT; ++r) {
            const int i = w * WCHUNK + r * 64 + lane;
            const bool valid = i < n;
            key[r] = valid ? k[i] : 0u;
            val[r] = valid ? v[i] : 0u;
            const u32 d = sp_digit(key[r], a);
            u64 m = __ballot(valid);
#pragma unroll
            for (int b = 0; b < 8; ++b) {
                const bool bit = (d >> b) & 1u;
                const u64 bal = __ballot(bit);
                m &= bit ? bal : ~bal;
            }
            const u32 below = (u32)__popcll(m & ((1ull << lane) - 1ull));
            const u32 prev = rw[d];
            rank[r] = prev + below;
            if (valid && below == 0) rw[d] = prev + (u32)__popcll(m);   // the digit's first lane: one writer per counter
        }
        __syncthreads();
        {   // run[w][d]: the wave's count of digit d -> where the wave's first pair of digit d goes
            u32 at = dbase;
#pragma unroll
            for (int j = 0; j < NT / 64; ++j) {
                const u32 c = run[j][tid];
                run[j][tid] = at;
                at += c;
            }
        }
        __syncthreads();
        u32* ok = okeys + seg * a.len;
        u32* ov = ovals + seg * a.len;
#pragma unroll
        for (int r = 0; r < EPT; ++r) {
            const int i = w * WCHUNK + r * 64 + lane;
            const long pos = (long)run[w][sp_digit(key[r], a)] + rank[r];
            if (i < n && pos < a.len) {   // pos < len by construction; the guard keeps a wrong count inside the segment
                ok[pos] = key[r];
                ov[pos] = val[r];
            }
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(NT) void sp_copy(const u32* __restrict__ sk, const u32* __restrict__ sv, u32* __restrict__ dk,
                                              u32* __restrict__ dv, long n) {
    for (long i = (long)blockIdx.x * NT + threadIdx.x; i < n; i += (long)gridDim.x * NT) {
        dk[i] = sk[i];
        dv[i] = sv[i];
    }
}

inline long sp_ntiles(long len) { return (len + TILE - 1) / TILE; }
inline int sp_grid(long want) { return (int)(want < SP_BLOCKS ? want : SP_BLOCKS); }

}  // namespace
}  // namespace csu

using namespace csu;

extern "C" int csu_sort_pairs_tile(void) { return TILE; }

extern "C" size_t csu_sort_pairs_workspace(int segments, long len) {
    if (segments < 1 || len < 1 || (long)segments * len >= (1L << 31)) return 0;
    return ((size_t)segments * BINS * (size_t)sp_ntiles(len) + (size_t)segments * BINS) * sizeof(u32);
}

extern "C" int csu_sort_pairs(int segments, long len, int key_bits, uint32_t* keys, uint32_t* vals, uint32_t* keys_alt,
                              uint32_t* vals_alt, void* workspace, size_t ws_bytes, void* stream) {
    if (segments < 1 || len < 1 || (long)segments * len >= (1L << 31))
        return fail(CSU_E_ARG, "sort_pairs: segments >= 1, len >= 1 and segments * len < 2^31");
    if (key_bits < 1 || key_bits > 32) return fail(CSU_E_ARG, "sort_pairs: 1 <= key_bits <= 32");
    if (!keys || !vals || !keys_alt || !vals_alt) return fail(CSU_E_ARG, "sort_pairs: null keys, vals or scratch buffers");
    if (((uintptr_t)keys | (uintptr_t)vals | (uintptr_t)keys_alt | (uintptr_t)vals_alt) & 3)
        return fail(CSU_E_ARG, "sort_pairs: keys, vals or scratch buffers misaligned");
    if (!workspace || ((uintptr_t)workspace & 3) || ws_bytes < csu_sort_pairs_workspace(segments, len))
        return fail(CSU_E_WORKSPACE, "sort_pairs: workspace (4-byte aligned)");
    hipStream_t st = as_stream(stream);
    SpArgs a;
    a.len = len;
    a.ntiles = sp_ntiles(len);
    a.items = (long)segments * a.ntiles;
    a.kmask = key_bits == 32 ? 0xFFFFFFFFu : (1u << key_bits) - 1u;
    u32* hist = (u32*)workspace;
    u32* tot = hist + (size_t)segments * BINS * (size_t)a.ntiles;
    const long rows = (long)segments * BINS;
    const int passes = (key_bits + 7) / 8;
    u32 *sk = keys, *sv = vals, *dk = keys_alt, *dv = vals_alt;
    for (int p = 0; p < passes; ++p) {
        a.shift = 8 * p;
        sp_hist<<<sp_grid(a.items), NT, 0, st>>>(sk, a, hist);
        sp_scan<<<sp_grid(rows), NT, 0, st>>>(hist, tot, rows, a.ntiles);
        sp_scatter<<<sp_grid(a.items), NT, 0, st>>>(sk, sv, a, hist, tot, dk, dv);
        std::swap(sk, dk);
        std::swap(sv, dv);
    }
    if (sk != keys) {
        const long n = (long)segments * len;
        sp_copy<<<sp_grid((n + NT - 1) / NT), NT, 0, st>>>(sk, sv, keys, vals, n);
    }
    return check_launch("sort_pairs");
}
