// Sliding-window (tiled) whole-image inference for gfx950: the traffic between an image of any size
// and the network's fixed S x S input, with test-time augmentation.  The reference has no prediction
// path beyond evaluate_model (cswin:712-747), so nothing here is a port.
//   tile table  int32 (B, 6) on the device, one record per batch slot: y0, x0, hflip, vflip, rot
//               (clockwise quarter turns after the flips, flipmap.hpp), active.  active = 0: a padding
//               slot of a ragged last batch.
//   gather      out[b, c, y, x] = image pixel (y0, x0) + src_of(y, x), coordinates clamped to the image
//               (replicate), uint8 / 255 (an IEEE division, as augment.hip) or fp32 as is.  A padding
//               slot shows slot 0's tile, so the forward never reads uninitialised memory.
//   blend       canvas[k, y0 + ty, x0 + tx] += w1[ty] w1[tx] p_k(b, y, x), (ty, tx) = src_of(y, x): the
//               same mapping, which undoes the transform.  p = the model output itself (PROB), its
//               sigmoid (K = 1 logits) or its softmax over k (max-subtracted, fp32 registers).
//   finish      prob = canvas / (ry[y] rx[x] n_tta); label = prob > 0.5 (K = 1) or the first argmax.
// Blend, deterministic without atomics: one workgroup owns a patch of the canvas in LDS (patch_w x
// patch_h; initialised from the canvas, so launches chain) and walks the batch's slots in table order; for a
// slot that touches the patch, the patch's part of the tile is a rectangle of the model output, whose
// rows the threads read in units on vector boundaries (the access modes of seg_ce.hip: class-last 16-B
// loads per pixel, NCHW V pixels per class, per element otherwise), one thread per pixel and a barrier
// per slot.  Every canvas pixel therefore receives its contributions one at a time in table order,
// starting from the canvas value: the result does not depend on how the tile list is cut into batches.
// Every model output element is read once, every covered canvas element read and written once per launch.
#include "common.hpp"
#include "flipmap.hpp"

namespace csu {
namespace {

constexpr int NT = 256;
constexpr int KMAX = 32;
constexpr int BMAX = 128;   // slots per launch (the table is staged in LDS)
constexpr int REC = 6;
constexpr int NTB = 256;    // blend workgroup
enum { MODE_CL = 0, MODE_NCHW = 1, MODE_GEN = 2 };

struct Rec {
    int y0, x0, hf, vf, rot, on;
};
__device__ __forceinline__ Rec load_rec(const int* t) {
    Rec r;
    r.y0 = t[0]; r.x0 = t[1];
    r.hf = t[2] != 0; r.vf = t[3] != 0; r.rot = t[4] & 3; r.on = t[5] != 0;
    return r;
}

template <bool U8>
__global__ __launch_bounds__(NT) void gather_kernel(int B, int S, int H, int W, const void* __restrict__ img,
                                                    const int* __restrict__ table, float* __restrict__ out) {
    const long ss = (long)S * S, n = (long)B * ss;
    for (long q = (long)blockIdx.x * NT + threadIdx.x; q < n; q += (long)gridDim.x * NT) {
        const int b = (int)(q / ss);
        const int r = (int)(q - (long)b * ss), y = r / S, x = r - y * S;
        Rec rc = load_rec(table + REC * b);
        if (!rc.on) rc = load_rec(table);
        int ty, tx;
        src_of(S, rc.hf, rc.vf, rc.rot, y, x, &ty, &tx);
        long sy = (long)rc.y0 + ty, sx = (long)rc.x0 + tx;
        sy = sy < 0 ? 0 : sy > H - 1 ? H - 1 : sy;
        sx = sx < 0 ? 0 : sx > W - 1 ? W - 1 : sx;
        float v[3];
        if constexpr (U8) {
            const uint8_t* p = (const uint8_t*)img + (sy * W + sx) * 3;
#pragma unroll
            for (int c = 0; c < 3; ++c) v[c] = (float)p[c] / 255.f;
        } else {
#pragma unroll
            for (int c = 0; c < 3; ++c) v[c] = ((const float*)img)[((long)c * H + sy) * W + sx];
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) out[((long)b * 3 + c) * ss + r] = v[c];
    }
}

struct BlendArgs {
    int B, S, H, W, K, prob;
    int by0, bx0;   // first patch row / column of the launch
    long s_b, s_k, s_pix;
    const void* z;
    const int* table;
    const float* w1;
    float* canvas;
};

inline int blend_bucket(int K) { return K == 1 ? 1 : K <= 4 ? 4 : K <= 8 ? 8 : K <= 16 ? 16 : 32; }
// The canvas patch of a workgroup.  One pixel per thread and round (class-last, per element): 16 x 16, a
// thread per patch pixel.  V pixels per thread (NCHW): 32 wide, as high as 34 KiB of LDS allow.  Measured
// at 2048 x 2048, tile 512, 16 slots: class-last K = 5 with eight variants 45 us per launch at 16 x 16
// against 83 at 32 x 32; K = 1 planes with one variant 23 us at 32 x 32 against 47 at 16 x 16.
constexpr int patch_w(int mode) { return mode == MODE_NCHW ? 32 : 16; }
constexpr int patch_h(int KB, int mode) { return mode != MODE_NCHW ? 16 : KB <= 8 ? 32 : KB == 16 ? 16 : 8; }
constexpr int blend_vec(int KB, int mode) { return mode != MODE_NCHW ? 1 : KB <= 8 ? 4 : KB == 16 ? 2 : 1; }

template <int V, typename T> __device__ __forceinline__ void ldv(const T* p, float* v) {
    if constexpr (V == 1) {
        v[0] = (float)p[0];
    } else {
        typedef T vec __attribute__((ext_vector_type(V)));
        const vec x = *reinterpret_cast<const vec*>(p);
#pragma unroll
        for (int j = 0; j < V; ++j) v[j] = (float)x[j];
    }
}
// widest access of a class-last pixel's KB elements: 16 B, or all of it when that is less
template <typename T, int KB> constexpr int cl_vec() { return KB * (int)sizeof(T) >= 16 ? 16 / (int)sizeof(T) : KB; }

// model output -> probabilities in place (z[k >= K] = -inf on entry)
template <int KB> __device__ __forceinline__ void to_prob(float (&z)[KB], bool prob) {
    if constexpr (KB == 1) {
        if (!prob) {
            const float e = exp_neg(-fabsf(z[0])), d = 1.f / (1.f + e);
            z[0] = z[0] >= 0.f ? d : e * d;
        }
    } else {
        float m = z[0];
#pragma unroll
        for (int k = 1; k < KB; ++k) m = z[k] > m ? z[k] : m;
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < KB; ++k) {
            z[k] = exp_neg(z[k] - m);
            s += z[k];
        }
        const float inv = 1.f / s;
#pragma unroll
        for (int k = 0; k < KB; ++k) z[k] *= inv;
    }
}

// the part of slot r's tile inside the patch [py0, py0 + ph) x [px0, px0 + pw), as canvas coordinates
__device__ __forceinline__ bool clip(const Rec& r, int S, int py0, int px0, int ph, int pw, int* cy0, int* cy1, int* cx0,
                                     int* cx1) {
    const long ylo = max((long)py0, (long)r.y0), yhi = min((long)py0 + ph, (long)r.y0 + S);
    const long xlo = max((long)px0, (long)r.x0), xhi = min((long)px0 + pw, (long)r.x0 + S);
    *cy0 = (int)ylo; *cy1 = (int)yhi; *cx0 = (int)xlo; *cx1 = (int)xhi;
    return r.on && ylo < yhi && xlo < xhi;
}

template <typename T, int KB, int MODE>
__global__ __launch_bounds__(NTB) void blend_kernel(BlendArgs a, int vec_ok) {
    constexpr int PW = patch_w(MODE), PH = patch_h(KB, MODE), PITCH = PW + 1, PP = PH * PITCH, V = blend_vec(KB, MODE);
    constexpr int UPR = PW / V + (V > 1 ? 1 : 0);   // units of a rectangle row (<= PW pixels as PH <= PW, any phase)
    __shared__ float acc[KB * PP];
    __shared__ int tab[BMAX * REC];
    const int K = a.K, S = a.S, H = a.H, W = a.W;
    const int py0 = (a.by0 + blockIdx.y) * PH, px0 = (a.bx0 + blockIdx.x) * PW;
    const int ph = min(PH, H - py0), pw = min(PW, W - px0);
    // the first slot that touches this patch, straight from the table (workgroup-uniform reads): a patch
    // none touches costs no LDS traffic and no barrier
    int first = -1, cy0, cy1, cx0, cx1;
    for (int b = 0; b < a.B && first < 0; ++b)
        if (clip(load_rec(a.table + REC * b), S, py0, px0, ph, pw, &cy0, &cy1, &cx0, &cx1)) first = b;
    if (first < 0) return;
    for (int i = threadIdx.x; i < a.B * REC; i += NTB) tab[i] = a.table[i];
    for (int i = threadIdx.x; i < K * PH * PW; i += NTB) {
        const int k = i / (PH * PW), r = i - k * (PH * PW), y = r / PW, x = r - y * PW;
        if (y < ph && x < pw) acc[k * PP + y * PITCH + x] = a.canvas[((long)k * H + py0 + y) * W + px0 + x];
    }
    __syncthreads();
    for (int b = first; b < a.B; ++b) {
        const Rec rc = load_rec(tab + REC * b);
        if (!clip(rc, S, py0, px0, ph, pw, &cy0, &cy1, &cx0, &cx1)) continue;   // block-uniform
        // the clipped tile as a rectangle of the model output (inclusive corners)
        int ya, xa, yb, xb;
        dst_of(S, rc.hf, rc.vf, rc.rot, cy0 - rc.y0, cx0 - rc.x0, &ya, &xa);
        dst_of(S, rc.hf, rc.vf, rc.rot, cy1 - 1 - rc.y0, cx1 - 1 - rc.x0, &yb, &xb);
        const int my0 = min(ya, yb), my1 = max(ya, yb), mx0 = min(xa, xb), mx1 = max(xa, xb);
        const int rows = my1 - my0 + 1;
        const T* zb = (const T*)a.z + (long)b * a.s_b;
        for (int u = threadIdx.x; u < rows * UPR; u += NTB) {
            const int row = u / UPR, j = u - row * UPR, y = my0 + row;
            int pre = 0;
            if (V > 1 && vec_ok)
                pre = (int)(((unsigned long)((uintptr_t)a.z / sizeof(T)) + (unsigned long)((long)b * a.s_b + (long)y * S + mx0)) % V);
            const int xs = mx0 - pre + j * V;   // the unit's first pixel: on a vector boundary when vec_ok
            if (xs > mx1) continue;
            const bool full = vec_ok && xs >= mx0 && xs + V - 1 <= mx1;
            float z[V][KB];
#pragma unroll
            for (int i = 0; i < V; ++i)
#pragma unroll
                for (int k = 0; k < KB; ++k) z[i][k] = k < K ? 0.f : -INFINITY;
            const long pix = (long)y * S + xs;
            if constexpr (MODE == MODE_CL) {
                constexpr int WV = cl_vec<T, KB>();
                float v[KB];
#pragma unroll
                for (int k = 0; k < KB; k += WV) ldv<WV>(zb + pix * a.s_pix + k, v + k);
#pragma unroll
                for (int k = 0; k < KB; ++k)
                    if (k < K) z[0][k] = v[k];
            } else if constexpr (MODE == MODE_NCHW) {
#pragma unroll
                for (int k = 0; k < KB; ++k) {
                    if (k < K) {
                        const T* q = zb + k * a.s_k + pix;
                        if (full) {
                            float v[V];
                            ldv<V>(q, v);
#pragma unroll
                            for (int i = 0; i < V; ++i) z[i][k] = v[i];
                        } else {
#pragma unroll
                            for (int i = 0; i < V; ++i)
                                if (xs + i >= mx0 && xs + i <= mx1) z[i][k] = (float)q[i];
                        }
                    }
                }
            } else {
#pragma unroll
                for (int k = 0; k < KB; ++k)
                    if (k < K) z[0][k] = (float)zb[pix * a.s_pix + k * a.s_k];
            }
#pragma unroll
            for (int i = 0; i < V; ++i) {
                const int x = xs + i;
                if (x < mx0 || x > mx1) continue;
                to_prob<KB>(z[i], a.prob != 0);
                int ty, tx;
                src_of(S, rc.hf, rc.vf, rc.rot, y, x, &ty, &tx);
                const float w = a.w1[ty] * a.w1[tx];
                float* c = acc + (rc.y0 + ty - py0) * PITCH + (rc.x0 + tx - px0);
#pragma unroll
                for (int k = 0; k < KB; ++k)
                    if (k < K) c[k * PP] += w * z[i][k];
            }
        }
        __syncthreads();
    }
    for (int i = threadIdx.x; i < K * PH * PW; i += NTB) {
        const int k = i / (PH * PW), r = i - k * (PH * PW), y = r / PW, x = r - y * PW;
        if (y < ph && x < pw) a.canvas[((long)k * H + py0 + y) * W + px0 + x] = acc[k * PP + y * PITCH + x];
    }
}

__global__ __launch_bounds__(NT) void finish_kernel(int K, int H, int W, const float* __restrict__ canvas,
                                                    const float* __restrict__ ry, const float* __restrict__ rx, float n_tta,
                                                    float* __restrict__ prob, uint8_t* __restrict__ labels) {
    const long hw = (long)H * W;
    for (long q = (long)blockIdx.x * NT + threadIdx.x; q < hw; q += (long)gridDim.x * NT) {
        const int y = (int)(q / W), x = (int)(q - (long)y * W);
        const float den = ry[y] * rx[x] * n_tta;
        float best = canvas[q] / den;
        int arg = 0;
        if (prob) prob[q] = best;
        for (int k = 1; k < K; ++k) {
            const float p = canvas[k * hw + q] / den;
            if (prob) prob[k * hw + q] = p;
            if (p > best) {
                best = p;
                arg = k;
            }
        }
        if (labels) labels[q] = (uint8_t)(K == 1 ? (best > 0.5f ? 1 : 0) : arg);
    }
}

// the access mode of a model output and whether its vector form applies (seg_ce.hip's rules)
template <typename T> int blend_mode(int K, int KB, const void* z, long s_b, long s_k, long s_pix, int pad_ok, int* vec_ok) {
    *vec_ok = 0;
    const uintptr_t za = (uintptr_t)z;
    // one class with unit pixel stride is a plane whatever s_k says: the V-pixel form, not 1-element "class vectors"
    if (s_k == 1 && s_pix >= KB && (K == KB || pad_ok) && !(K == 1 && s_pix == 1)) {
        const long WV = KB * (long)sizeof(T) >= 16 ? 16 / (long)sizeof(T) : KB;
        if (za % ((uintptr_t)WV * sizeof(T)) == 0 && s_pix % WV == 0 && s_b % WV == 0) return MODE_CL;
    }
    if (s_pix == 1) {
        const long V = blend_vec(KB, MODE_NCHW);
        *vec_ok = V > 1 && (K == 1 || s_k % V == 0) && s_b % V == 0 && za % sizeof(T) == 0;
        return MODE_NCHW;
    }
    return MODE_GEN;
}

template <class F> void with_bucket(int KB, F&& f) {
    switch (KB) {
        case 1: f(iconst<1>{}); break;
        case 4: f(iconst<4>{}); break;
        case 8: f(iconst<8>{}); break;
        case 16: f(iconst<16>{}); break;
        default: f(iconst<32>{}); break;
    }
}
template <class F> void with_mode(int mode, F&& f) {
    switch (mode) {
        case MODE_CL: f(iconst<MODE_CL>{}); break;
        case MODE_NCHW: f(iconst<MODE_NCHW>{}); break;
        default: f(iconst<MODE_GEN>{}); break;
    }
}

inline unsigned grid_1d(long n) {
    const long g = (n + NT - 1) / NT;
    return (unsigned)(g > 65536 ? 65536 : g);
}

}  // namespace
}  // namespace csu

using namespace csu;

extern "C" int csu_tile_gather(int B, int S, int H, int W, int src_kind, const void* image, const int* table, float* out,
                               void* stream) {
    if (B < 1 || S < 1 || H < 1 || W < 1) return fail(CSU_E_ARG, "tile_gather: B, S, H and W must be >= 1");
    if (src_kind != CSU_TILE_SRC_U8_HWC && src_kind != CSU_TILE_SRC_F32_CHW)
        return fail(CSU_E_ARG, "tile_gather: src_kind must be CSU_TILE_SRC_U8_HWC or CSU_TILE_SRC_F32_CHW");
    if (!image || !table || !out) return fail(CSU_E_ARG, "tile_gather: null image, table or out");
    const unsigned g = grid_1d((long)B * S * S);
    if (src_kind == CSU_TILE_SRC_U8_HWC)
        gather_kernel<true><<<g, NT, 0, as_stream(stream)>>>(B, S, H, W, image, table, out);
    else
        gather_kernel<false><<<g, NT, 0, as_stream(stream)>>>(B, S, H, W, image, table, out);
    return check_launch("tile_gather");
}

extern "C" int csu_tile_blend(int B, int S, int H, int W, int K, int form, int dtype, const void* z, long s_b, long s_k,
                              long s_pix, int pad_ok, const int* table, const float* w1, float* canvas, int ry0, int rx0,
                              int ry1, int rx1, void* stream) {
    if (B < 1 || B > BMAX) return fail(CSU_E_ARG, "tile_blend: 1 <= B <= 128 slots per launch");
    if (S < 1 || H < 1 || W < 1) return fail(CSU_E_ARG, "tile_blend: S, H and W must be >= 1");
    if (K < 1 || K > KMAX) return fail(CSU_E_ARG, "tile_blend: 1 <= K <= 32 classes");
    if (form != CSU_TILE_PROB && form != CSU_TILE_LOGITS) return fail(CSU_E_ARG, "tile_blend: form must be CSU_TILE_PROB or CSU_TILE_LOGITS");
    if (dtype != CSU_F32 && dtype != CSU_BF16) return fail(CSU_E_ARG, "tile_blend: dtype must be f32 or bf16");
    if (form == CSU_TILE_PROB && (K != 1 || dtype != CSU_F32)) return fail(CSU_E_ARG, "tile_blend: PROB is fp32 with K = 1");
    if (s_k < 1 || s_pix < 1 || s_b < 0) return fail(CSU_E_ARG, "tile_blend: strides must be positive");
    if (!z || !table || !w1 || !canvas) return fail(CSU_E_ARG, "tile_blend: null z, table, w1 or canvas");
    if (ry0 < 0 || rx0 < 0 || ry1 > H || rx1 > W || ry0 >= ry1 || rx0 >= rx1)
        return fail(CSU_E_ARG, "tile_blend: region must be a non-empty rectangle inside the canvas");
    const int KB = blend_bucket(K);
    int vec_ok = 0;
    const int mode = dtype == CSU_F32 ? blend_mode<float>(K, KB, z, s_b, s_k, s_pix, pad_ok, &vec_ok)
                                      : blend_mode<bf16>(K, KB, z, s_b, s_k, s_pix, pad_ok, &vec_ok);
    const int PH = patch_h(KB, mode), PW = patch_w(mode);
    const int by0 = ry0 / PH, bx0 = rx0 / PW;
    const long gy = (ry1 + PH - 1) / PH - by0, gx = (rx1 + PW - 1) / PW - bx0;
    if (gy > 65535) return fail(CSU_E_ARG, "tile_blend: region too tall for one launch");
    BlendArgs a;
    a.B = B; a.S = S; a.H = H; a.W = W; a.K = K; a.prob = form == CSU_TILE_PROB;
    a.by0 = by0; a.bx0 = bx0;
    a.s_b = s_b; a.s_k = s_k; a.s_pix = s_pix;
    a.z = z; a.table = table; a.w1 = w1; a.canvas = canvas;
    const dim3 grid((unsigned)gx, (unsigned)gy);
    hipStream_t st = as_stream(stream);
    with_flag(dtype == CSU_F32, [&](auto f32) {
        using T = std::conditional_t<decltype(f32)::value, float, bf16>;
        with_bucket(KB, [&](auto kb) {
            with_mode(mode, [&](auto md) {
                blend_kernel<T, decltype(kb)::value, decltype(md)::value><<<grid, NTB, 0, st>>>(a, vec_ok);
            });
        });
    });
    return check_launch("tile_blend");
}

extern "C" int csu_tile_finish(int K, int H, int W, const float* canvas, const float* ry, const float* rx, float n_tta,
                               float* prob, void* labels, void* stream) {
    if (K < 1 || K > KMAX) return fail(CSU_E_ARG, "tile_finish: 1 <= K <= 32 classes");
    if (H < 1 || W < 1) return fail(CSU_E_ARG, "tile_finish: H and W must be >= 1");
    if (!(n_tta > 0.f)) return fail(CSU_E_ARG, "tile_finish: n_tta must be > 0");
    if (!canvas || !ry || !rx) return fail(CSU_E_ARG, "tile_finish: null canvas, ry or rx");
    if (!prob && !labels) return fail(CSU_E_ARG, "tile_finish: no output (prob and labels both null)");
    finish_kernel<<<grid_1d((long)H * W), NT, 0, as_stream(stream)>>>(K, H, W, canvas, ry, rx, n_tta, prob, (uint8_t*)labels);
    return check_launch("tile_finish");
}
