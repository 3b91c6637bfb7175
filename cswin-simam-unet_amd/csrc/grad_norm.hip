// Global L2 norm of all gradients and its clip coefficient for gfx950, over the optimizer's own
// csu_adamw_item table (adamw.hip): torch.nn.utils.clip_grad_norm_ without its ~2 small torch
// kernels per tensor and without a host sync, so it can live in the captured training step.
//   1  grad_sumsq_kernel: one workgroup per chunk of the table (the chunk numbering of adamw_kernel:
//      flat chunks of 4096 elements, 64 x 64 tiles of a matrix with a transposed shadow), 16-B loads
//      where the step uses them; every element goes to fp64 BEFORE it is squared (an fp32 square
//      underflows below 1e-19 and overflows above 1.8e19), fixed order per thread, xor-shuffle tree
//      per wave, LDS across the four waves -> partial[chunk].  No atomics.
//   2  grad_norm_finish_kernel (one workgroup): fixed-order strided sum of the partials in fp64 ->
//      ctl = {norm, coef = min(1, max_norm / (norm + 1e-6)), finite, 0}.
//   3  the step multiplies g by ctl[1] in registers (adamw_kernel<.., CLIP>), or, for another
//      optimizer, grad_scale_kernel scales the gradients in place.
// Streaming: 4 B per parameter read (+ 4 B written by the in-place scale).  Equal gradients give
// bitwise equal norms: the summation order depends on the table alone.
#include "adamw_items.hpp"

namespace csu {
namespace {

using namespace adamw_items;

constexpr int FT = 1024;   // threads of the finish workgroup

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__device__ __forceinline__ bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// Walks the in-bounds elements of chunk b of item `it` in groups of up to 4 consecutive ones:
// f(index of the first, count n, vec) -- vec: n == 4 and the group is 16-B aligned.  The masks are
// those of adamw_kernel (tile: r < rows, c < cols, scalar path when cols % 4 != 0; flat: ragged tail
// when numel % 4 != 0), plus a scalar path for a gradient buffer that is itself off a 16-B boundary.
template <typename F> __device__ __forceinline__ void for_chunk(const csu_adamw_item& it, long b, F f) {
    const bool al = aligned16(it.grad);
    if (is_tiled(it)) {
        const int tk = (it.cols + 63) / 64;
        const long t = b - it.chunk0;
        const int r0 = (int)(t / tk) * 64, c0 = (int)(t % tk) * 64;
        const int cq = (threadIdx.x & 15) * 4, rr = threadIdx.x >> 4;
        const bool vec = al && (it.cols & 3) == 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int r = r0 + rr + 16 * i, c = c0 + cq;
            if (r < it.rows && c < it.cols) f((long)r * it.cols + c, min(4, it.cols - c), vec);
        }
        return;
    }
    const long base = (b - it.chunk0) * CH;
    const bool vec = al && (it.numel & 3) == 0;
#pragma unroll
    for (int q = 0; q < PER / 4; ++q) {
        const long i = base + ((long)q * NT + threadIdx.x) * 4;
        if (i >= it.numel) break;
        f(i, (int)(it.numel - i < 4 ? it.numel - i : 4), vec);
    }
}

__global__ __launch_bounds__(NT) void grad_sumsq_kernel(const csu_adamw_item* __restrict__ items, int count,
                                                        double* __restrict__ partial) {
    __shared__ double red[NT / 64];
    const long b = blockIdx.x;
    const csu_adamw_item it = items[find_item(items, count, b)];
    const float* g = it.grad;
    double s = 0.;
    for_chunk(it, b, [&](long i, int n, bool vec) {
        float gv[4];
        ld4n(g, i, n, vec, gv);   // elements past n read as 0
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const double d = (double)gv[j];
            s = fma(d, d, s);
        }
    });
    s = wave_sum_d(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) partial[b] = (red[0] + red[1]) + (red[2] + red[3]);
}

__global__ __launch_bounds__(FT) void grad_norm_finish_kernel(const double* __restrict__ partial, long n, float max_norm,
                                                              float* __restrict__ ctl) {
    __shared__ double red[FT / 64];
    double s0 = 0., s1 = 0., s2 = 0., s3 = 0.;   // four loads in flight; fixed association
    long j = threadIdx.x;
    for (; j + 3 * FT < n; j += 4 * FT) {
        s0 += partial[j];
        s1 += partial[j + FT];
        s2 += partial[j + 2 * FT];
        s3 += partial[j + 3 * FT];
    }
    for (; j < n; j += FT) s0 += partial[j];
    const double s = wave_sum_d((s0 + s1) + (s2 + s3));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        double tot = 0.;
#pragma unroll
        for (int w = 0; w < FT / 64; ++w) tot += red[w];
        const float norm = (float)sqrt(tot);
        float coef = 1.f;
        if (max_norm > 0.f && max_norm <= 3.402823466e38f) {
            // torch: clamp(max_norm / (total_norm + 1e-6), max=1.0) in fp32; a NaN norm stays NaN
            const float q = max_norm / (norm + 1e-6f);
            coef = q < 1.f ? q : (q != q ? q : 1.f);
        }
        ctl[0] = norm;
        ctl[1] = coef;
        ctl[2] = isfinite(tot) ? 1.f : 0.f;
        ctl[3] = 0.f;
    }
}

__global__ __launch_bounds__(NT) void grad_scale_kernel(const csu_adamw_item* __restrict__ items, int count,
                                                        const float* __restrict__ coef_dev) {
    const float c = *coef_dev;
    if (c == 1.f) return;   // nothing clipped: g * 1 is g
    const long b = blockIdx.x;
    const csu_adamw_item it = items[find_item(items, count, b)];
    float* g = const_cast<float*>(it.grad);
    for_chunk(it, b, [&](long i, int n, bool vec) {
        float gv[4];
        ld4n(g, i, n, vec, gv);
#pragma unroll
        for (int j = 0; j < 4; ++j) gv[j] *= c;
        st4n(g, i, n, vec, gv);
    });
}

}  // namespace
}  // namespace csu

using namespace csu;

extern "C" size_t csu_grad_norm_workspace(long total_chunks) {
    return total_chunks < 1 ? 0 : (size_t)total_chunks * sizeof(double);
}

extern "C" int csu_grad_sumsq(const csu_adamw_item* items, int count, long total_chunks, double* partial, void* stream) {
    if (!items || count < 1 || total_chunks < 1) return fail(CSU_E_ARG, "grad_sumsq: empty item table");
    if (!partial || ((uintptr_t)partial & 7)) return fail(CSU_E_ARG, "grad_sumsq: partial must be an 8-B aligned buffer");
    grad_sumsq_kernel<<<(unsigned)total_chunks, NT, 0, as_stream(stream)>>>(items, count, partial);
    return check_launch("grad_sumsq");
}

extern "C" int csu_grad_norm_finish(const double* partial, long n, float max_norm, float* ctl, void* stream) {
    if (!partial || n < 1) return fail(CSU_E_ARG, "grad_norm_finish: no partial sums");
    if (!ctl) return fail(CSU_E_ARG, "grad_norm_finish: null ctl");
    if (max_norm != max_norm) return fail(CSU_E_ARG, "grad_norm_finish: max_norm is NaN");
    grad_norm_finish_kernel<<<1, FT, 0, as_stream(stream)>>>(partial, n, max_norm, ctl);
    return check_launch("grad_norm_finish");
}

extern "C" int csu_grad_scale(const csu_adamw_item* items, int count, long total_chunks, const float* coef_dev,
                              void* stream) {
    if (!items || count < 1 || total_chunks < 1) return fail(CSU_E_ARG, "grad_scale: empty item table");
    if (!coef_dev) return fail(CSU_E_ARG, "grad_scale: null coefficient");
    grad_scale_kernel<<<(unsigned)total_chunks, NT, 0, as_stream(stream)>>>(items, count, coef_dev);
    return check_launch("grad_scale");
}
