// Chunk geometry of a csu_adamw_item table (csu.h), shared by the kernels that walk one: the
// optimizer step (adamw.hip), the gradient-norm / clipping passes (grad_norm.hip) and the weight EMA
// update / swap (ema.hip).  One
// workgroup of NT threads per chunk; a flat chunk is CH consecutive elements, a tile chunk one
// 64 x 64 tile of a rows x cols matrix.
#pragma once
#include "common.hpp"

namespace csu {
namespace adamw_items {

constexpr int NT = 256;
constexpr int PER = 16;                  // elements per thread
constexpr long CH = (long)NT * PER;      // elements per chunk (workgroup)

// index of the item that owns chunk b: the last item with chunk0 <= b
__device__ __forceinline__ int find_item(const csu_adamw_item* __restrict__ items, int count, long b) {
    int lo = 0, hi = count - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (items[mid].chunk0 <= b) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// a tile item: 64 x 64 tiles of a rows x cols matrix (W and W^T shadows)
__device__ __forceinline__ bool is_tiled(const csu_adamw_item& it) { return it.shadow && it.shadow_t && it.taps == 0; }

// n (<= 4) elements at index i: one 16-B vector when vec (n == 4, 16-B aligned), else scalars
__device__ __forceinline__ void ld4n(const float* p, long i, int n, bool vec, float* v) {
    if (vec) load4(p + i, v);
    else {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = j < n ? p[i + j] : 0.f;
    }
}
template <typename T> __device__ __forceinline__ void st4n(T* p, long i, int n, bool vec, const float* v) {
    if (vec) store4(p + i, v);
    else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (j < n) p[i + j] = from_f<T>(v[j]);
    }
}

// LDS stage of a tile item's W^T shadow (+ 2 columns: the column reads spread over the banks)
using ShadowTile = bf16[64][64 + 2];

// Walks chunk b of item `it` as the optimizer step does (tile items: 4 row segments of a 64 x 64 tile
// per thread; flat items: PER / 4 groups of 4 consecutive elements) and writes every bf16 shadow
// layout the item names (csu.h) from the values f leaves behind: f(index of the first element,
// count n, vec, pv) updates the fp32 tensors and returns the now-live parameter values in pv[0..n).
// Shared by the step (adamw.hip) and the parameter <-> EMA swap (ema.hip).  Every thread of the
// workgroup must call it (the tile path has a barrier).  SHADOWS = false: the same walk with no
// shadow written, no LDS and no barrier (the stand-alone EMA update; tile may be null).
template <bool SHADOWS, typename F>
__device__ __forceinline__ void walk_chunk(const csu_adamw_item& it, long b, ShadowTile* tile, F f) {
    bf16* sh = SHADOWS ? (bf16*)it.shadow : nullptr;
    bf16* sht = (bf16*)it.shadow_t;
    if (is_tiled(it)) {   // 64 x 64 tile of a rows x cols matrix: W and W^T shadows
        const int tk = (it.cols + 63) / 64;
        const long t = b - it.chunk0;
        const int r0 = (int)(t / tk) * 64, c0 = (int)(t % tk) * 64;
        const int cq = (threadIdx.x & 15) * 4, rr = threadIdx.x >> 4;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int r = r0 + rr + 16 * i, c = c0 + cq;
            float pv[4] = {0.f, 0.f, 0.f, 0.f};
            if (r < it.rows && c < it.cols) {
                const int n = min(4, it.cols - c);
                const bool vec = (it.cols & 3) == 0;   // then n == 4 and the row segment is 16-B aligned
                const long e = (long)r * it.cols + c;
                f(e, n, vec, pv);
                if constexpr (SHADOWS) st4n(sh, e, n, vec, pv);
            }
            if constexpr (SHADOWS) {
#pragma unroll
                for (int j = 0; j < 4; ++j) (*tile)[rr + 16 * i][cq + j] = (bf16)pv[j];
            }
        }
        if constexpr (!SHADOWS) return;
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 4; ++i) {   // W^T rows c0.. (cols rows): thread -> (column c, 4 rows)
            const int c = c0 + rr + 16 * i;
            if (c >= it.cols) continue;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int r = r0 + cq + j;
                if (r < it.rows) sht[(long)c * it.rows + r] = (*tile)[cq + j][rr + 16 * i];
            }
        }
        return;
    }
    const long base = (b - it.chunk0) * CH;
    const bool vec = (it.numel & 3) == 0;
#pragma unroll
    for (int q = 0; q < PER / 4; ++q) {
        const long i = base + ((long)q * NT + threadIdx.x) * 4;   // 4 consecutive elements, coalesced per q
        if (i >= it.numel) break;
        const int n = vec ? 4 : (int)(it.numel - i < 4 ? it.numel - i : 4);
        float pv[4];
        f(i, n, vec, pv);
        if (!sh) continue;
        if (it.taps > 0) {   // conv weight [n][c][tap] -> OHWI [n][tap][c] (stride cols_pad), IHWO [c][tap][n]
            const unsigned TP = it.taps, CT = (unsigned)it.cols * TP;
            const unsigned CP = it.cols_pad > it.cols ? it.cols_pad : it.cols;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (j >= n) break;
                const unsigned e = (unsigned)(i + j), o = e / CT, rem = e - o * CT, c = rem / TP, t = rem - c * TP;
                const bf16 w = (bf16)pv[j];
                sh[(o * TP + t) * CP + c] = w;
                if (sht) sht[(c * TP + t) * (unsigned)it.rows + o] = w;
            }
        } else {
            st4n(sh, i, n, vec, pv);
        }
    }
}

// Weight of the new value in one EMA update, w = 1 - d: d = decay, or with warmup min(decay, n / (n + 9))
// where n counts the EMA updates including this one ((1 + t) / (10 + t) for t = n - 1).
__device__ __forceinline__ float ema_weight(const float* n_dev, float decay, int warmup) {
    float d = decay;
    if (warmup) {
        const float n = *n_dev;
        d = fminf(decay, n / (n + 9.f));
    }
    return 1.f - d;
}

// e <- e + w (p - e) on 4 elements: ONE definition, so the fused step and the stand-alone update agree
// bit for bit
__device__ __forceinline__ void ema4(float w, const float* pv, float* ev) {
#pragma unroll
    for (int j = 0; j < 4; ++j) ev[j] = fmaf(w, pv[j] - ev[j], ev[j]);
}

}  // namespace adamw_items
}  // namespace csu
