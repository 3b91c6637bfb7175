// Patch pool for gfx950 (include/csu.h, "Patch pool"): the row index of a pool of full-size cases, and the draw
// of patch origins with forced foreground centres.  The reference has no counterpart.  None of this is a hot
// path (the index is built once per pool, the draw is one wave per batch slot); the warp that cuts the patches
// is patch_warp_kernel in augment_warp.hip.
//
//   patch_count_kernel    one wave per label row: per class, the popcount of __ballot(class == c) over the row's
//                         64-label chunks, lane c keeping class c's count -> rows[i][c][y + 1]
//   patch_scan_kernel     one wave per (image, class): an inclusive wave scan over 64 rows at a time with a
//                         carry turns the counts into the exclusive prefix, in place
//   patch_draw_kernel     one wave per slot: 2 Philox calls -> image, class, pixel rank, origin; locate()
//   patch_locate_kernel   one wave per query: locate()
// Integers only: every result is exact and independent of the launch shape.
#include "common.hpp"
#include "rng.hpp"

namespace csu {
namespace {

constexpr int NT = 256, WAVES = NT / 64;

__device__ __forceinline__ int classes_of(int K) { return K == 1 ? 2 : K; }
// the class of a label byte; a label >= K (K >= 2) equals no class c < K
__device__ __forceinline__ int class_of(int label, int K) { return K == 1 ? (int)(label > 0) : label; }
__device__ __forceinline__ int pick(uint32_t w, int n) { return (int)__umulhi(w, (uint32_t)n); }   // (uint64(w) n) >> 32

struct Case {
    const uint8_t* lab;
    const int* rows;
    int H, W;
};
__device__ __forceinline__ Case load_case(const uint8_t* labels, const long long* meta, const int* rows, int n) {
    const long long* m = meta + (long)n * 4;
    return {labels + m[0], rows + m[3], (int)m[1], (int)m[2]};
}

// (y, x) of the r-th pixel of class c in raster order, 0 <= r < count.  Called by a whole wave with uniform
// arguments; the result is uniform.
__device__ __forceinline__ int2 locate(const Case& cs, int K, int c, int r, int lane) {
    const int* t = cs.rows + (long)c * (cs.H + 1);
    int lo = 0, hi = cs.H;                    // t[lo] <= r < t[hi]: row lo holds the pixel when hi = lo + 1
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (t[mid] <= r) lo = mid; else hi = mid;
    }
    int rem = r - t[lo], x = -1;
    const uint8_t* row = cs.lab + (long)lo * cs.W;
    for (int x0 = 0; x0 < cs.W; x0 += 64) {
        const int xx = x0 + lane;
        const bool hit = xx < cs.W && class_of(row[min(xx, cs.W - 1)], K) == c;
        const unsigned long long m = __ballot(hit);
        const int pc = __popcll(m);
        if (rem < pc) {                       // the chunk that crosses the rank: the lane with `rem` hits before it
            const unsigned long long sel = __ballot(hit && __popcll(m & ((1ull << lane) - 1ull)) == rem);
            x = x0 + __ffsll((long long)sel) - 1;
            break;
        }
        rem -= pc;
    }
    return make_int2(lo, x);
}

__global__ __launch_bounds__(NT) void patch_count_kernel(int N, int K, const uint8_t* __restrict__ labels,
                                                         const long long* __restrict__ meta, int* __restrict__ rows) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, Kc = classes_of(K);
    for (int n = blockIdx.y; n < N; n += gridDim.y) {
        const long long* m = meta + (long)n * 4;
        const uint8_t* lab = labels + m[0];
        const int H = (int)m[1], W = (int)m[2];
        int* t = rows + m[3];
        for (int y = blockIdx.x * WAVES + wave; y < H; y += gridDim.x * WAVES) {
            const uint8_t* row = lab + (long)y * W;
            int cnt = 0;                      // lane c: the pixels of class c in this row
            for (int x0 = 0; x0 < W; x0 += 64) {
                const int xx = x0 + lane;
                const int cl = xx < W ? class_of(row[xx], K) : -1;
                for (int c = 0; c < Kc; ++c) {
                    const int pc = __popcll(__ballot(cl == c));
                    if (lane == c) cnt += pc;
                }
            }
            if (lane < Kc) t[(long)lane * (H + 1) + y + 1] = cnt;
        }
    }
}

__global__ __launch_bounds__(64) void patch_scan_kernel(int N, int K, const long long* __restrict__ meta, int* __restrict__ rows) {
    const int lane = threadIdx.x, Kc = classes_of(K);
    const long total = (long)N * Kc;
    for (long q = blockIdx.x; q < total; q += gridDim.x) {
        const int n = (int)(q / Kc), c = (int)(q - (long)n * Kc);
        const int H = (int)meta[(long)n * 4 + 1];
        int* t = rows + meta[(long)n * 4 + 3] + (long)c * (H + 1);
        if (lane == 0) t[0] = 0;
        int carry = 0;
        for (int y0 = 0; y0 < H; y0 += 64) {      // each lane reads and writes its own entry only
            const int y = y0 + lane;
            int v = y < H ? t[y + 1] : 0;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const int u = __shfl_up(v, o, 64);
                if (lane >= o) v += u;
            }
            if (y < H) t[y + 1] = carry + v;
            carry += __shfl(v, 63, 64);
        }
    }
}

struct DrawArgs {
    int N, K, Ph, Pw, B, fg_slots;
    uint32_t class_mask, site;
    float p_fg;
};

// the origin along one axis: L the image's extent, P the patch's, c the centre of a foreground slot
__device__ __forceinline__ int origin(int L, int P, bool fg, int c, uint32_t w) {
    if (L < P) return -((P - L) / 2);
    return fg ? min(max(c - P / 2, 0), L - P) : pick(w, L - P + 1);
}

__global__ __launch_bounds__(NT) void patch_draw_kernel(DrawArgs a, const uint8_t* __restrict__ labels,
                                                        const long long* __restrict__ meta, const int* __restrict__ rows,
                                                        const int* __restrict__ indices, const uint64_t* __restrict__ rng,
                                                        int* __restrict__ record) {
    const int lane = threadIdx.x & 63, b = blockIdx.x * WAVES + (threadIdx.x >> 6);
    if (b >= a.B) return;                     // whole waves leave; no barrier below
    const Snap s = load_snap(rng);
    const uint4 v0 = draw4(s, 0u, b, a.site), v1 = draw4(s, 1u, b, a.site);
    const uint32_t w[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
    const int n = indices ? min(max(indices[b], 0), a.N - 1) : pick(w[0], a.N);
    const Case cs = load_case(labels, meta, rows, n);
    bool fg = b < a.fg_slots || u01(w[1]) < a.p_fg;
    int cls = -1, cy = -1, cx = -1, count = 0;
    if (fg) {
        // lane c: the count of class c if it is eligible
        const bool elig = lane < classes_of(a.K) && ((a.class_mask >> lane) & 1u);
        const int cnt = elig ? cs.rows[(long)lane * (cs.H + 1) + cs.H] : 0;
        const unsigned long long present = __ballot(cnt > 0);
        const int m = __popcll(present);
        if (m > 0) {
            const int j = pick(w[2], m);
            const unsigned long long sel = __ballot(cnt > 0 && __popcll(present & ((1ull << lane) - 1ull)) == j);
            cls = __ffsll((long long)sel) - 1;
            count = __shfl(cnt, cls, 64);
            const int2 p = locate(cs, a.K, cls, pick(w[3], count), lane);
            cy = p.x; cx = p.y;
        } else {
            fg = false;
        }
    }
    const int oy = origin(cs.H, a.Ph, fg, cy, w[4]), ox = origin(cs.W, a.Pw, fg, cx, w[5]);
    if (lane == 0) {
        int4* out = reinterpret_cast<int4*>(record + (long)b * CSU_PATCH_RECORD);
        out[0] = make_int4(n, cls, cy, cx);
        out[1] = make_int4(oy, ox, (int)fg, count);
        out[2] = make_int4((int)w[0], (int)w[1], (int)w[2], (int)w[3]);
        out[3] = make_int4((int)w[4], (int)w[5], (int)w[6], (int)w[7]);
    }
}

__global__ __launch_bounds__(NT) void patch_locate_kernel(int N, int K, int M, const uint8_t* __restrict__ labels,
                                                          const long long* __restrict__ meta, const int* __restrict__ rows,
                                                          const int* __restrict__ qn, const int* __restrict__ qc,
                                                          const int* __restrict__ qr, int* __restrict__ yx) {
    const int lane = threadIdx.x & 63;
    for (long i = (long)blockIdx.x * WAVES + (threadIdx.x >> 6); i < M; i += (long)gridDim.x * WAVES) {
        const int n = qn[i], c = qc[i], r = qr[i];
        int2 p = make_int2(-1, -1);
        if (n >= 0 && n < N && c >= 0 && c < classes_of(K) && r >= 0) {
            const Case cs = load_case(labels, meta, rows, n);
            if (r < cs.rows[(long)c * (cs.H + 1) + cs.H]) p = locate(cs, K, c, r, lane);
        }
        if (lane == 0) { yx[2 * i] = p.x; yx[2 * i + 1] = p.y; }
    }
}

bool pool_ok(const void* labels, const int64_t* meta, const int32_t* rows, int N, int K) {
    return labels && meta && rows && N >= 1 && N <= (1 << 20) && K >= 1 && K <= 32;
}

}  // namespace
}  // namespace csu

using namespace csu;

extern "C" int csu_patch_index(int N, int K, int max_h, const void* labels, const int64_t* meta, int32_t* rows, void* stream) {
    if (!pool_ok(labels, meta, rows, N, K) || max_h < 1) return fail(CSU_E_ARG, "patch_index: bad args");
    hipStream_t st = as_stream(stream);
    const int gx = (max_h + WAVES - 1) / WAVES;
    patch_count_kernel<<<dim3((unsigned)(gx > 1024 ? 1024 : gx), (unsigned)(N > 4096 ? 4096 : N)), NT, 0, st>>>(
        N, K, (const uint8_t*)labels, (const long long*)meta, rows);
    const long q = (long)N * (K == 1 ? 2 : K);
    patch_scan_kernel<<<(unsigned)(q > 65536 ? 65536 : q), 64, 0, st>>>(N, K, (const long long*)meta, rows);
    return check_launch("patch_index");
}

extern "C" int csu_patch_draw(const void* labels, const int64_t* meta, const int32_t* rows, int N, int K, unsigned class_mask,
                              int Ph, int Pw, int B, int fg_slots, float p_fg, const int32_t* indices, const uint64_t* rng,
                              unsigned site, int32_t* record, void* stream) {
    if (!pool_ok(labels, meta, rows, N, K) || Ph < 1 || Pw < 1 || B < 1 || B > (1 << 20) || fg_slots < 0 ||
        !(p_fg >= 0.f && p_fg <= 1.f) || !rng || site >= 4096u || !record)
        return fail(CSU_E_ARG, "patch_draw: bad args");
    DrawArgs a;
    a.N = N; a.K = K; a.Ph = Ph; a.Pw = Pw; a.B = B; a.fg_slots = fg_slots;
    a.class_mask = class_mask; a.site = site; a.p_fg = p_fg;
    patch_draw_kernel<<<(B + WAVES - 1) / WAVES, NT, 0, as_stream(stream)>>>(a, (const uint8_t*)labels, (const long long*)meta,
                                                                            rows, indices, rng, record);
    return check_launch("patch_draw");
}

extern "C" int csu_patch_locate(const void* labels, const int64_t* meta, const int32_t* rows, int N, int K, int M,
                                const int32_t* n, const int32_t* cls, const int32_t* r, int32_t* yx, void* stream) {
    if (!pool_ok(labels, meta, rows, N, K) || M < 1 || !n || !cls || !r || !yx) return fail(CSU_E_ARG, "patch_locate: bad args");
    const int g = (M + WAVES - 1) / WAVES;
    patch_locate_kernel<<<g > 16384 ? 16384 : g, NT, 0, as_stream(stream)>>>(N, K, M, (const uint8_t*)labels,
                                                                            (const long long*)meta, rows, n, cls, r, yx);
    return check_launch("patch_locate");
}
