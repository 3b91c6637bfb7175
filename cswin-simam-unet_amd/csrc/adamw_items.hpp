// Chunk geometry of a csu_adamw_item table (csu.h), shared by the kernels that walk one: the
// optimizer step (adamw.hip) and the gradient-norm / clipping passes (grad_norm.hip).  One
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

}  // namespace adamw_items
}  // namespace csu
