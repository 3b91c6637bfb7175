// Fused multi-class segmentation loss  w_ce * CE + w_tversky * mean_r mean_{c in C}(1 - TI_rc)  on
// K-class logits z (fp32 or bf16, upcast in registers) and integer labels t (uint8 or int64), with
// the hard (argmax) per-class sums of the training loop's Dice / IoU from the same pass.  The
// reference trains one class only (num_classes=1, cswin:924) and has no counterpart.
//   p = softmax_k(z) (max-subtracted, fp32);  pixels with t == ignore_index contribute to no sum
//   CE    = sum_pix w[t] (logsumexp(z) - z_t) / sum_pix w[t]                      (whole batch)
//   TP_rc = sum p_c [t = c],  P_rc = sum p_c,  T_rc = sum [t = c]                 (row r: batch or image)
//   D = (1 - a - b) TP + a P + b T + smooth,  TI = (TP + smooth) / D
//   hard: pred = argmax_k z (lowest index wins a tie);  I_c = sum [pred = c][t = c],  Pr_c = sum [pred = c]
//
// Work split (seg_loss.hip's): an image's HW pixels are cut into cpi chunks of clen pixels
// (clen % 4 == 0); one workgroup reduces one (image, chunk) item at a time, items beyond the grid
// are walked grid-stride.  A row of the Tversky term is one image (rows = B) or all of them (rows = 1).
//   forward 1  ce_partial: 2 + 5 K sums per item (CE numerator, sum w, and per class TP, P, T, I, Pr)
//              -> workspace[item][2 + 5 K].  A thread keeps p_c and p_c [t = c] sums per class in a
//              fixed pixel order; the three counts are wave ballots (integers: exact in any order);
//              then a fixed shuffle + LDS tree.  No atomics.
//   forward 2  ce_finish (one workgroup, fp64): wave w sums the items of the (row, class) pairs w,
//              w + 4, ...; writes loss, stats (3, K) fp64 [I; Pr; T], per (row, class) the backward
//              coefficients A = (D - (TP + smooth)(1 - a - b)) / D^2, C = a (TP + smooth) / D^2 (zero for
//              an excluded background), and 1 / sum w (0 when every pixel is ignored: CE and its
//              gradient are then 0, not NaN).
//   backward   ce_backward: recomputes the softmax and writes, in the logits' dtype and strides,
//              dz_k = g [w_ce w[t] (p_k - [k = t]) / sum w - (w_tv / (R |C|)) p_k (G_k - sum_c G_c p_c)],
//              G_c = A_rc [t = c] - C_rc.
// Logits are addressed by element strides (s_b, s_k, s_pix).  Three access modes:
//   class-last vector  s_k = 1, every pixel's K logits start on a vector boundary and the bucket
//              KB >= K is readable per pixel (K == KB, or a padded pitch: the token GEMM's n8):
//              one thread per pixel, 16-B loads.
//   NCHW       s_pix = 1: a thread owns V = 4 / 2 / 1 (KB <= 8 / 16 / 32) consecutive pixels of every
//              class, V-wide loads on units that lie inside the chunk on a vector boundary; the
//              first / last unit of a chunk that starts off a boundary are read per element.
//   strided    anything else (dense class-last with K != KB): per-element loads.
// Boundary term (csu_seg_bd_*, template flag BD; off in csu_seg_ce_*, whose arithmetic it leaves alone):
//   + w_bd[0] BD,  BD = sum over live pixels and c in Cb of p_c phi_c / (n |Cb|),  n = sum_c T_c,  Cb = 1 .. K-1 or all;
//   phi dense fp32 (B, K, HW) read per class plane; one more partial sum per item (index 2 + 5 K); ce_finish leaves
//   1 / (n |Cb|) behind 1 / sum w; backward adds g w_bd / (n |Cb|) p_k (phi_k [k in Cb] - sum_{c in Cb} phi_c p_c).
// Hard-example CE (csu_seg_hard_*, template flag HD; off in the other two families, whose arithmetic it leaves alone):
//   l = w[t] u^gamma L per live pixel, u = sum_{k != t} p_k, L = log(sum) + (max - z_t), in the place of w[t] L.  Without
//   a selection nothing else changes.  With one (rho on the device), ce_partial also stores every l as an fp32 key,
//   csu_kth_largest (kth_largest.hip) finds tau = the k-th largest, hd_msum sums l and w[t] above tau and w[t] at tau per
//   item in a fixed order, ce_finish forms HCE = (S_gt + (k - n_gt) tau) / (W_gt + f W_eq), f = (k - n_gt) / n_eq, in
//   fp64 and leaves 1 / W, tau, f in coef; backward scales the CE part by m (u^gamma + gamma q u^(gamma - 1) L) with
//   m = 1, f, 0 from the stored key against tau.
// No label ever indexes memory (class weight and z_t are selected by comparison), so a label
// outside [0, K) cannot fault; it matches no class.  The summation order is a function of the
// shape, the strides and the address mod 16 only.
#include "common.hpp"

namespace csu {
namespace {

constexpr int NT = 256;
constexpr int CE_BLOCKS = 1024;
constexpr int KMAX = 32;

enum { MODE_CL = 0, MODE_NCHW = 1, MODE_GEN = 2 };

struct CePlan {
    long clen, items;
    int cpi;
};

CePlan ce_plan(int B, long HW) {
    CePlan s;
    const long maxc = B < CE_BLOCKS ? CE_BLOCKS / B : 1;
    long cpi = (HW + 4 * NT - 1) / (4 * NT);
    cpi = cpi < 1 ? 1 : cpi > maxc ? maxc : cpi;
    s.clen = ((HW + cpi - 1) / cpi + 3) & ~3L;
    s.cpi = (int)((HW + s.clen - 1) / s.clen);
    s.items = (long)B * s.cpi;
    return s;
}

inline int ce_nsum(int K) { return 2 + 5 * K; }
inline int ce_bucket(int K) { return K <= 4 ? 4 : K <= 8 ? 8 : K <= 16 ? 16 : 32; }
constexpr int ce_vec(int KB, int mode) { return mode != MODE_NCHW ? 1 : KB <= 8 ? 4 : KB == 16 ? 2 : 1; }

struct CeArgs {
    int B, K, cpi, lab64;
    long HW, clen, items, s_b, s_k, s_pix, ignore;
    const void* z;
    const void* t;
    const float* cw;
};

// The boundary term (csu_seg_bd_*): BD = sum over live pixels and c in Cb of p_c phi_c / (n |Cb|), n = the live
// pixels whose label is a class, Cb = classes 1 .. K-1 or all of them (bg).  phi is dense fp32 (B, K, HW).
struct BdArgs {
    const float* phi;
    const float* w_bd;   // one float on the device
    int bg;
};

// The hard-example CE term (csu_seg_hard_*): l = w[t] u^gamma L per live pixel, u = sum_{k != t} p_k, L = the pixel's
// CE.  keys == nullptr: HCE = sum l / sum w.  Otherwise the forward leaves every l in keys (a dead pixel: HD_DEAD,
// sign bit set), csu_kth_largest leaves (tau, n_gt, n_eq, k, n) in sel, and the pixels above tau count in full,
// those equal to it with f = (k - n_gt) / n_eq.  Keys are compared as bit patterns, which order non-negative floats.
struct HdArgs {
    float gamma;
    float* keys;         // (B, HW) fp32, or nullptr
    const double* sel;   // csu_kth_largest's five values
    float* msum;         // per item: sum of l above tau, sum of w above tau, sum of w at tau
};
constexpr float HD_DEAD = -1.f;

// The Lovasz-Softmax term (csu_seg_lovasz_*): for the classes of mask (C), in the order of their bits m = 0 .. |C|-1,
// the forward leaves every pixel's key and value in keys / vals (|C|, B, HW) for csu_sort_pairs:
//   e = fminf(t == c ? sum_{k != c} p_k : p_c, 1) (a NaN counts as 1),  key = 0x3F800000 - bits(e), in [0, 0x3F800000]:
//   ascending keys are descending e; a dead pixel has e = 0 and bit 30 set, which puts it behind every live one;
//   value = (fg << 31) | the pixel's flat index in its segment (b HW + pix, or pix with per_image).
// The backward reads the planes psi (|C|, B, HW) through BdArgs (phi = psi, w_bd = w_lv, bg = mask): load_phi<LV>.
struct LvArgs {
    unsigned* keys;
    unsigned* vals;
    unsigned mask;
    int per_image;
};
constexpr unsigned LV_ONE = 0x3F800000u, LV_DEAD = 1u << 30;

// u^gamma; 1 when gamma = 0, also at u = 0.  gamma is uniform: the usual exponents 1 and 2 skip powf, which
// measured 75 us of the 200 us of forward + backward at B 16, K 5, 512 x 512 (profiles/hard_example_loss_timing.txt)
__device__ __forceinline__ float hd_pow(float u, float gamma) {
    return gamma == 0.f ? 1.f : gamma == 1.f ? u : gamma == 2.f ? u * u : powf(u, gamma);
}
// l of one pixel, >= +0 (a NaN stays one): L = log(sum) + (max - z_t) >= 0 by construction (in that association it
// keeps its precision next to logits of 1e4, which the gradient, unlike plain CE's, needs), and -0 is flushed
__device__ __forceinline__ float hd_term(float wt, float u, float L, float gamma) {
    const float l = wt * hd_pow(u, gamma) * L;
    return l == 0.f ? 0.f : l;
}
// d l / d L at fixed weights of the softmax: u^gamma + gamma q u^(gamma - 1) L, the second summand 0 at gamma = 0,
// u = 0 or L = 0 (where u^(gamma - 1) may be infinite)
__device__ __forceinline__ float hd_factor(float q, float u, float L, float gamma) {
    const float second = gamma != 0.f && u > 0.f && L > 0.f ? gamma * q * hd_pow(u, gamma - 1.f) * L : 0.f;
    return hd_pow(u, gamma) + second;
}
// the weight m of a pixel's key in the selection
__device__ __forceinline__ float hd_select(float key, float tau, float f) {
    const unsigned kb = __float_as_uint(key), tb = __float_as_uint(tau);
    return (int)kb < 0 || kb < tb ? 0.f : kb > tb ? 1.f : f;
}

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

template <int V, typename T> __device__ __forceinline__ void loadv(const T* p, float* v) {
    if constexpr (V == 1) {
        v[0] = (float)p[0];
    } else {
        typedef T vec __attribute__((ext_vector_type(V)));
        const vec x = *reinterpret_cast<const vec*>(p);
#pragma unroll
        for (int j = 0; j < V; ++j) v[j] = (float)x[j];
    }
}
template <int V, typename T> __device__ __forceinline__ void storev(T* p, const float* v) {
    if constexpr (V == 1) {
        p[0] = (T)v[0];
    } else {
        typedef T vec __attribute__((ext_vector_type(V)));
        vec x;
#pragma unroll
        for (int j = 0; j < V; ++j) x[j] = (T)v[j];
        *reinterpret_cast<vec*>(p) = x;
    }
}
// widest access of a class-last pixel's KB elements: 16 B, or all of it when that is less
template <typename T, int KB> constexpr int cl_vec() { return KB * (int)sizeof(T) >= 16 ? 16 / (int)sizeof(T) : KB; }

// f[j][k] = phi of pixel e0 + j and class k for the classes that carry the term, else 0; only pixels inside
// [lo, hi) are read.  A unit that is whole and whose plane address is on a vector boundary takes one V-wide load.
// LV: the planes are psi (|C|, B, HW) of the Lovasz term, class k's plane the one of its place among the bits of bd.bg
template <int KB, int V, bool LV = false>
__device__ __forceinline__ void load_phi(const CeArgs& a, const BdArgs& bd, long b, long e0, long lo, long hi, bool full,
                                         float (&f)[V][KB]) {
#pragma unroll
    for (int k = 0; k < KB; ++k) {
#pragma unroll
        for (int j = 0; j < V; ++j) f[j][k] = 0.f;
        if (k < a.K && (LV ? (((unsigned)bd.bg >> k) & 1u) != 0 : (bd.bg || k > 0))) {
            const long plane = LV ? (long)__popc((unsigned)bd.bg & ((1u << k) - 1u)) * a.B + b : b * a.K + k;
            const float* q = bd.phi + plane * a.HW + e0;
            if (V > 1 && full && ((uintptr_t)q % (V * sizeof(float))) == 0) {
                float v[V];
                loadv<V>(q, v);
#pragma unroll
                for (int j = 0; j < V; ++j) f[j][k] = v[j];
            } else {
#pragma unroll
                for (int j = 0; j < V; ++j)
                    if (e0 + j >= lo && e0 + j < hi) f[j][k] = q[j];
            }
        }
    }
}

// One unit = V pixels e0 .. e0 + V - 1 of image base zb; pixels outside [lo, hi) are dead.
// z[j][k] = logit of pixel j, class k; 0 for a dead pixel, -inf for k >= K.
template <typename T, int KB, int MODE, int V>
__device__ __forceinline__ void load_unit(const CeArgs& a, const T* zb, long e0, long lo, long hi, bool full,
                                          float (&z)[V][KB]) {
#pragma unroll
    for (int j = 0; j < V; ++j)
#pragma unroll
        for (int k = 0; k < KB; ++k) z[j][k] = k < a.K ? 0.f : -INFINITY;
    if constexpr (MODE == MODE_CL) {
        if (e0 >= lo && e0 < hi) {
            constexpr int W = cl_vec<T, KB>();
            float v[KB];
#pragma unroll
            for (int k = 0; k < KB; k += W) loadv<W>(zb + e0 * a.s_pix + k, v + k);
#pragma unroll
            for (int k = 0; k < KB; ++k)
                if (k < a.K) z[0][k] = v[k];
        }
    } else if constexpr (MODE == MODE_NCHW) {
#pragma unroll
        for (int k = 0; k < KB; ++k) {
            if (k < a.K) {
                const T* q = zb + k * a.s_k + e0;
                if (full) {
                    float v[V];
                    loadv<V>(q, v);
#pragma unroll
                    for (int j = 0; j < V; ++j) z[j][k] = v[j];
                } else {
#pragma unroll
                    for (int j = 0; j < V; ++j)
                        if (e0 + j >= lo && e0 + j < hi) z[j][k] = (float)q[j];
                }
            }
        }
    } else {
        if (e0 >= lo && e0 < hi) {
#pragma unroll
            for (int k = 0; k < KB; ++k)
                if (k < a.K) z[0][k] = (float)zb[e0 * a.s_pix + k * a.s_k];
        }
    }
}

// label of pixel e of image b as a class index, -1 when the pixel is dead, ignored or out of range
__device__ __forceinline__ int load_label(const CeArgs& a, long b, long e, long lo, long hi, bool& live) {
    live = false;
    if (e < lo || e >= hi) return -1;
    const long i = b * a.HW + e;
    const long v = a.lab64 ? ((const long*)a.t)[i] : (long)((const unsigned char*)a.t)[i];
    live = v != a.ignore;
    return live && v >= 0 && v < a.K ? (int)v : -1;
}

// softmax of one pixel in place (z -> p), returns max and sum of exp; arg = first maximum
template <int KB> __device__ __forceinline__ void softmax_px(float (&z)[KB], float& m, float& s, int& arg) {
    m = z[0];
    arg = 0;
#pragma unroll
    for (int k = 1; k < KB; ++k)
        if (z[k] > m) {
            m = z[k];
            arg = k;
        }
    s = 0.f;
#pragma unroll
    for (int k = 0; k < KB; ++k) {
        z[k] = exp_neg(z[k] - m);
        s += z[k];
    }
    const float inv = 1.f / s;
#pragma unroll
    for (int k = 0; k < KB; ++k) z[k] *= inv;
}

// the units of item `it`: image b, pixels [lo, hi), first unit at e_first (<= lo, on a V boundary of
// the logits' address when the vector form applies), nu units
template <typename T, int V>
__device__ __forceinline__ void item_range(const CeArgs& a, long it, bool vec_ok, long& b, long& lo, long& hi,
                                           long& e_first, long& nu) {
    b = it / a.cpi;
    lo = (it - b * a.cpi) * a.clen;
    hi = min(lo + a.clen, a.HW);
    long pre = 0;
    if (V > 1 && vec_ok) pre = (long)((((uintptr_t)a.z / sizeof(T)) + (unsigned long)(b * a.s_b + lo)) % V);
    e_first = lo - pre;
    nu = (hi - e_first + V - 1) / V;
}

// BD: one more sum per item, the boundary term's sum of p_c phi_c, at index 2 + 5 K
// HD: the CE numerator is the sum of l = w[t] u^gamma L, and with hd.keys every pixel's l goes there as its key
// LV: every pixel's Lovasz key and value go to lv.keys / lv.vals for the classes of lv.mask; the sums are unchanged
template <typename T, int KB, int MODE, bool BD, bool HD, bool LV = false>
__global__ __launch_bounds__(NT) void ce_partial(CeArgs a, BdArgs bd, HdArgs hd, int vec_ok, float* __restrict__ partial,
                                                 LvArgs lv = LvArgs{nullptr, nullptr, 0u, 0}) {
    constexpr int V = ce_vec(KB, MODE);
    constexpr bool LANE_CNT = KB >= 16;
    constexpr int NC = LANE_CNT ? 1 : KB;
    __shared__ float red[NT / 64][2 + 5 * KB + (BD ? 1 : 0)];
    const int K = a.K, ns = 2 + 5 * K + (BD ? 1 : 0);
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    float cw[KB];
#pragma unroll
    for (int k = 0; k < KB; ++k) cw[k] = (a.cw && k < K) ? a.cw[k] : 1.f;
    for (long it = blockIdx.x; it < a.items; it += gridDim.x) {
        long b, lo, hi, e_first, nu;
        item_range<T, V>(a, it, vec_ok, b, lo, hi, e_first, nu);
        const T* zb = (const T*)a.z + b * a.s_b;
        float ce = 0.f, sw = 0.f, bsum = 0.f, tp[KB], ps[KB];
        // counts: wave-uniform ballot sums, one scalar per class (small buckets) or held by lane k for
        // class k (KB >= 16: 3 registers instead of 3 KB)
        int ct[NC], ci[NC], cp[NC];
#pragma unroll
        for (int k = 0; k < KB; ++k) tp[k] = ps[k] = 0.f;
#pragma unroll
        for (int k = 0; k < NC; ++k) ct[k] = ci[k] = cp[k] = 0;
        auto count = [&](int (&c)[NC], int k, bool pred) {
            const int n = __popcll(__ballot(pred));
            if constexpr (LANE_CNT) c[0] += lane == k ? n : 0; else c[k] += n;
        };
        for (long ub = 0; ub < nu; ub += NT) {   // the same trip count in every lane: ballots see whole waves
            const long u = ub + threadIdx.x;
            const long e0 = e_first + u * V;
            const bool full = vec_ok && e0 >= lo && e0 + V <= hi;
            float z[V][KB];
            load_unit<T, KB, MODE, V>(a, zb, e0, lo, hi, full, z);
            float f[BD ? V : 1][BD ? KB : 1];
            if constexpr (BD) load_phi<KB, V>(a, bd, b, e0, lo, hi, e0 >= lo && e0 + V <= hi, f);
#pragma unroll
            for (int j = 0; j < V; ++j) {
                bool live;
                const int t = load_label(a, b, e0 + j, lo, hi, live);
                float zt = 0.f, wt = 0.f;
#pragma unroll
                for (int k = 0; k < KB; ++k) {
                    zt = t == k ? z[j][k] : zt;
                    wt = t == k ? cw[k] : wt;
                }
                float m, s;
                int arg;
                softmax_px<KB>(z[j], m, s, arg);
                if constexpr (HD) {
                    float u = 0.f;
#pragma unroll
                    for (int k = 0; k < KB; ++k) u += t == k ? 0.f : z[j][k];
                    const float l = hd_term(wt, u, logf(s) + (m - zt), hd.gamma);
                    ce += t >= 0 ? l : 0.f;
                    if (hd.keys && e0 + j >= lo && e0 + j < hi) hd.keys[b * a.HW + e0 + j] = t >= 0 ? l : HD_DEAD;
                } else {
                    ce += live ? wt * ((logf(s) + m) - zt) : 0.f;
                }
                if constexpr (LV) {
                    const long pix = e0 + j;
                    if (pix >= lo && pix < hi) {
                        float u = 0.f;   // the foreground error, formed as the hard-example term forms its u
#pragma unroll
                        for (int k = 0; k < KB; ++k) u += t == k ? 0.f : z[j][k];
                        const unsigned flat = (unsigned)(lv.per_image ? pix : b * a.HW + pix);
#pragma unroll
                        for (int k = 0; k < KB; ++k) {
                            if (k < K && ((lv.mask >> k) & 1u)) {
                                const bool fg = t == k;
                                const float e = fminf(fg ? u : z[j][k], 1.f);
                                const long at = ((long)__popc(lv.mask & ((1u << k) - 1u)) * a.B + b) * a.HW + pix;
                                lv.keys[at] = live ? LV_ONE - __float_as_uint(e) : LV_DEAD | LV_ONE;
                                lv.vals[at] = (fg ? 0x80000000u : 0u) | flat;
                            }
                        }
                    }
                }
                sw += wt;
                const int pred = live ? arg : -1;
#pragma unroll
                for (int k = 0; k < KB; ++k) {
                    const float pk = live ? z[j][k] : 0.f;
                    ps[k] += pk;
                    tp[k] += t == k ? pk : 0.f;
                    count(ct, k, t == k);
                    count(cp, k, pred == k);
                    count(ci, k, pred == k && t == k);
                }
                if constexpr (BD) {
                    float pf = 0.f;
#pragma unroll
                    for (int k = 0; k < KB; ++k) pf = __builtin_fmaf(z[j][k], f[j][k], pf);
                    bsum += live ? pf : 0.f;
                }
            }
        }
        ce = wave_sum(ce);
        sw = wave_sum(sw);
        if (lane == 0) {
            red[wv][0] = ce;
            red[wv][1] = sw;
        }
        if constexpr (BD) {
            bsum = wave_sum(bsum);
            if (lane == 0) red[wv][2 + 5 * K] = bsum;
        }
#pragma unroll
        for (int k = 0; k < KB; ++k) {
            const float wtp = wave_sum(tp[k]), wps = wave_sum(ps[k]);
            if (lane == 0 && k < K) {
                red[wv][2 + k] = wtp;
                red[wv][2 + K + k] = wps;
                if constexpr (!LANE_CNT) {
                    red[wv][2 + 2 * K + k] = (float)ct[k];
                    red[wv][2 + 3 * K + k] = (float)ci[k];
                    red[wv][2 + 4 * K + k] = (float)cp[k];
                }
            }
        }
        if constexpr (LANE_CNT) {
            if (lane < K) {
                red[wv][2 + 2 * K + lane] = (float)ct[0];
                red[wv][2 + 3 * K + lane] = (float)ci[0];
                red[wv][2 + 4 * K + lane] = (float)cp[0];
            }
        }
        __syncthreads();
        for (int i = threadIdx.x; i < ns; i += NT)
            partial[it * ns + i] = (red[0][i] + red[1][i]) + (red[2][i] + red[3][i]);
        __syncthreads();
    }
}

// coef: rows x K x 2 floats (A, C), then 1 / sum w; BD: then 1 / (n |Cb|), and terms = {the loss without the
// boundary term, BD}.  HD: HCE in the place of CE; coef: (A, C), then 1 / W (W = HCE's denominator), tau, f (0, 1
// without a selection), and hterms = fp64 {HCE, the Tversky term, tau, k} (k = n without a selection)
template <bool BD, bool HD>
__global__ __launch_bounds__(NT) void ce_finish(int B, int K, int cpi, int rows, const float* __restrict__ partial,
                                                float w_ce, float w_tv, float alpha, float beta, float smooth, int bg,
                                                BdArgs bd, HdArgs hd, float* __restrict__ terms, double* __restrict__ hterms,
                                                float* __restrict__ loss, double* __restrict__ stats,
                                                float* __restrict__ coef) {
    __shared__ double red[HD ? 7 : BD ? 5 : 3][NT / 64];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int ns = 2 + 5 * K + (BD ? 1 : 0);
    const long items = (long)B * cpi;
    const long ipr = rows == 1 ? items : cpi;   // items per row
    const double a = alpha, b = beta, g = 1.0 - a - b, sm = smooth;
    double atv = 0.;
    for (long pr = w; pr < (long)rows * K; pr += NT / 64) {
        const long r = pr / K;
        const int c = (int)(pr - r * K);
        double TP = 0., P = 0., T = 0.;
        for (long i = lane; i < ipr; i += 64) {
            const float* q = partial + (r * ipr + i) * ns + 2 + c;
            TP += (double)q[0];
            P += (double)q[K];
            T += (double)q[2 * K];
        }
        TP = wave_sum_d(TP);
        P = wave_sum_d(P);
        T = wave_sum_d(T);
        const bool on = bg || c > 0;
        const double num = TP + sm, D = g * TP + a * P + b * T + sm, inv = 1.0 / D;
        if (lane == 0) {
            coef[2 * pr] = on ? (float)((D - num * g) * inv * inv) : 0.f;
            coef[2 * pr + 1] = on ? (float)(a * num * inv * inv) : 0.f;
        }
        if (on) atv += (a * (P - TP) + b * (T - TP)) * inv;   // 1 - TI without the cancellation of 1 - num / D
    }
    if (stats)
        for (int c = w; c < K; c += NT / 64) {
            double I = 0., Pr = 0., T = 0.;
            for (long i = lane; i < items; i += 64) {
                const float* q = partial + i * ns + 2 + 2 * K + c;
                T += (double)q[0];
                I += (double)q[K];
                Pr += (double)q[2 * K];
            }
            I = wave_sum_d(I);
            Pr = wave_sum_d(Pr);
            T = wave_sum_d(T);
            if (lane == 0) {
                stats[c] = I;
                stats[K + c] = Pr;
                stats[2 * K + c] = T;
            }
        }
    double ce = 0., sw = 0.;
    for (long i = threadIdx.x; i < items; i += NT) {
        ce += (double)partial[i * ns];
        sw += (double)partial[i * ns + 1];
    }
    ce = wave_sum_d(ce);
    sw = wave_sum_d(sw);
    if (lane == 0) {
        red[0][w] = atv;
        red[1][w] = ce;
        red[2][w] = sw;
    }
    if constexpr (BD) {
        double n = 0., bs = 0.;   // n: the counts T_c of every class and item (integers: exact in any order)
        for (long i = threadIdx.x; i < items; i += NT) {
            const float* q = partial + i * ns + 2 + 2 * K;
            for (int c = 0; c < K; ++c) n += (double)q[c];
            bs += (double)partial[i * ns + 2 + 5 * K];
        }
        n = wave_sum_d(n);
        bs = wave_sum_d(bs);
        if (lane == 0) {
            red[3][w] = n;
            red[4][w] = bs;
        }
    }
    if constexpr (HD) {
        double sg = 0., wg = 0., we = 0., n = 0.;   // n: as for BD
        for (long i = threadIdx.x; i < items; i += NT) {
            const float* q = partial + i * ns + 2 + 2 * K;
            for (int c = 0; c < K; ++c) n += (double)q[c];
            if (hd.keys) {
                sg += (double)hd.msum[3 * i];
                wg += (double)hd.msum[3 * i + 1];
                we += (double)hd.msum[3 * i + 2];
            }
        }
        sg = wave_sum_d(sg);
        wg = wave_sum_d(wg);
        we = wave_sum_d(we);
        n = wave_sum_d(n);
        if (lane == 0) {
            red[3][w] = sg;
            red[4][w] = wg;
            red[5][w] = we;
            red[6][w] = n;
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double tot[HD ? 7 : BD ? 5 : 3];
#pragma unroll
        for (int k = 0; k < (HD ? 7 : BD ? 5 : 3); ++k) tot[k] = (red[k][0] + red[k][1]) + (red[k][2] + red[k][3]);
        const int nc = bg ? K : K - 1;
        if constexpr (HD) {
            double num = tot[1], W = tot[2], tau = 0., f = 1., k = tot[6];
            if (hd.keys) {   // sum m l = sum above tau + (k - n_gt) tau;  sum m w = sum above tau + f (sum at tau)
                tau = hd.sel[0];
                k = hd.sel[3];
                const double rest = k - hd.sel[1];
                f = hd.sel[2] > 0. ? rest / hd.sel[2] : 0.;
                num = tot[3] + (rest > 0. ? rest * tau : 0.);
                W = tot[4] + f * tot[5];
            }
            const double iw = W > 0. ? 1.0 / W : 0., hce = W > 0. ? num * iw : 0.;
            const double tv = tot[0] / ((double)rows * nc);
            coef[2 * (long)rows * K] = (float)iw;
            coef[2 * (long)rows * K + 1] = (float)tau;
            coef[2 * (long)rows * K + 2] = (float)f;
            hterms[0] = hce;
            hterms[1] = tv;
            hterms[2] = tau;
            hterms[3] = k;
            loss[0] = (float)((double)w_ce * hce + (double)w_tv * tv);
            return;
        }
        const double isw = tot[2] > 0. ? 1.0 / tot[2] : 0.;
        const double base = (double)w_ce * tot[1] * isw + (double)w_tv * tot[0] / ((double)rows * nc);
        coef[2 * (long)rows * K] = (float)isw;
        if constexpr (BD) {
            const double inb = tot[3] > 0. ? 1.0 / (tot[3] * (double)(bd.bg ? K : K - 1)) : 0.;
            const double term = tot[4] * inb;
            terms[0] = (float)base;
            terms[1] = (float)term;
            loss[0] = (float)(base + (double)bd.w_bd[0] * term);
            coef[2 * (long)rows * K + 1] = (float)inb;
        } else {
            loss[0] = (float)base;
        }
    }
}

// BD: dz_k += g w_bd / (n |Cb|) p_k (f_k - sum_c f_c p_c), f = phi on the classes that carry the term
// csu_seg_bd_bwd launches both instantiations with bd.w_bd set and exactly one of them works: the one without the
// term when it is switched off (w_bd[0] = 0, or a zero upstream gradient), so that phi is not read and the
// gradient is csu_seg_ce_bwd's bit for bit.  One kernel with the term in the same expression does not give that:
// the compiler contracts and packs the multiplies and adds of the whole expression as it sees fit.
// HD: the CE part of dz_k becomes g w_ce m w[t] (p_k - [k = t]) (u^gamma + gamma q u^(gamma - 1) L) / W.  m comes from
// the pixel's stored key against tau, never from l formed again here: this kernel's l need not round as the
// forward's did, and a key that moved across tau would move the gradient by a whole pixel's worth.
// LV (csu_seg_lovasz_bwd, with BD): the planes are the forward's psi, which carry their own scale (the coefficient
// behind 1 / sum w is 1), f = psi on the classes of the mask in bd.bg; the same gated pair.
template <typename T, int KB, int MODE, bool BD, bool HD, bool LV = false>
__global__ __launch_bounds__(NT) void ce_backward(CeArgs a, BdArgs bd, HdArgs hd, int vec_ok, int rows,
                                                  const float* __restrict__ dloss, const float* __restrict__ coef, float w_ce,
                                                  float tv_scale, T* __restrict__ dz) {
    static_assert(!LV || BD, "the Lovasz term takes the boundary term's place in the expression");
    constexpr int V = ce_vec(KB, MODE);
    const int K = a.K;
    if (bd.w_bd != nullptr) {
        const bool off = dloss[0] * bd.w_bd[0] * coef[2 * (long)rows * K + 1] == 0.f;
        if (off == BD) return;
    }
    const float g = dloss[0], g1 = g * w_ce * coef[2 * (long)rows * K], g2 = g * tv_scale;
    float g3 = 0.f;
    if constexpr (BD) g3 = g * bd.w_bd[0] * coef[2 * (long)rows * K + 1];
    float tau = 0.f, ftie = 1.f;
    if constexpr (HD) {
        tau = coef[2 * (long)rows * K + 1];
        ftie = coef[2 * (long)rows * K + 2];
    }
    float cw[KB];
#pragma unroll
    for (int k = 0; k < KB; ++k) cw[k] = (a.cw && k < K) ? a.cw[k] : 1.f;
    for (long it = blockIdx.x; it < a.items; it += gridDim.x) {
        long b, lo, hi, e_first, nu;
        item_range<T, V>(a, it, vec_ok, b, lo, hi, e_first, nu);
        const T* zb = (const T*)a.z + b * a.s_b;
        T* db = dz + b * a.s_b;
        const float* cf = coef + 2 * (rows == 1 ? 0 : b) * K;
        float A[KB], C[KB];
#pragma unroll
        for (int k = 0; k < KB; ++k) {
            A[k] = k < K ? cf[2 * k] : 0.f;
            C[k] = k < K ? cf[2 * k + 1] : 0.f;
        }
        for (long ub = 0; ub < nu; ub += NT) {
            const long u = ub + threadIdx.x;
            const long e0 = e_first + u * V;
            const bool full = vec_ok && e0 >= lo && e0 + V <= hi;
            float z[V][KB];
            load_unit<T, KB, MODE, V>(a, zb, e0, lo, hi, full, z);
            float f[BD ? V : 1][BD ? KB : 1];
            if constexpr (BD) load_phi<KB, V, LV>(a, bd, b, e0, lo, hi, e0 >= lo && e0 + V <= hi, f);
#pragma unroll
            for (int j = 0; j < V; ++j) {
                bool live;
                const int t = load_label(a, b, e0 + j, lo, hi, live);
                float wt = 0.f;
#pragma unroll
                for (int k = 0; k < KB; ++k) wt = t == k ? cw[k] : wt;
                float zt = 0.f;
                if constexpr (HD) {
#pragma unroll
                    for (int k = 0; k < KB; ++k) zt = t == k ? z[j][k] : zt;
                }
                float m, s;
                int arg;
                softmax_px<KB>(z[j], m, s, arg);
                float dot = 0.f;
#pragma unroll
                for (int k = 0; k < KB; ++k) dot += ((t == k ? A[k] : 0.f) - C[k]) * z[j][k];
                float hf = 1.f;
                if constexpr (HD) {
                    float q = 0.f, u = 0.f;
#pragma unroll
                    for (int k = 0; k < KB; ++k) {
                        q = t == k ? z[j][k] : q;
                        u += t == k ? 0.f : z[j][k];
                    }
                    hf = hd_factor(q, u, logf(s) + (m - zt), hd.gamma);
                    if (hd.keys) hf *= t >= 0 ? hd_select(hd.keys[b * a.HW + e0 + j], tau, ftie) : 0.f;
                }
                const float c1 = HD ? g1 * wt * hf : g1 * wt;
                float fdot = 0.f;
                if constexpr (BD) {
#pragma unroll
                    for (int k = 0; k < KB; ++k) fdot = __builtin_fmaf(f[j][k], z[j][k], fdot);
                }
#pragma unroll
                for (int k = 0; k < KB; ++k) {
                    const float pk = z[j][k], G = (t == k ? A[k] : 0.f) - C[k];
                    float d = c1 * (pk - (t == k ? 1.f : 0.f)) - g2 * pk * (G - dot);
                    if constexpr (BD) d = __builtin_fmaf(g3, pk * (f[j][k] - fdot), d);
                    z[j][k] = live ? d : 0.f;
                }
            }
            if constexpr (MODE == MODE_CL) {
                if (e0 >= lo && e0 < hi) {
                    constexpr int W = cl_vec<T, KB>();
#pragma unroll
                    for (int k = 0; k < KB; ++k)
                        if (k >= K) z[0][k] = 0.f;
#pragma unroll
                    for (int k = 0; k < KB; k += W) storev<W>(db + e0 * a.s_pix + k, &z[0][k]);
                }
            } else if constexpr (MODE == MODE_NCHW) {
#pragma unroll
                for (int k = 0; k < KB; ++k) {
                    if (k < K) {
                        T* q = db + k * a.s_k + e0;
                        if (full) {
                            float v[V];
#pragma unroll
                            for (int j = 0; j < V; ++j) v[j] = z[j][k];
                            storev<V>(q, v);
                        } else {
#pragma unroll
                            for (int j = 0; j < V; ++j)
                                if (e0 + j >= lo && e0 + j < hi) q[j] = (T)z[j][k];
                        }
                    }
                }
            } else {
                if (e0 >= lo && e0 < hi) {
#pragma unroll
                    for (int k = 0; k < KB; ++k)
                        if (k < K) db[e0 * a.s_pix + k * a.s_k] = (T)z[0][k];
                }
            }
        }
    }
}

// The selected sums of the hard-example term, per item in a fixed order: over the item's keys above tau the sum of
// l and of w[t], over those equal to tau the sum of w[t].  Reads the keys, and the labels only when there are class
// weights (without them w = 1 on every live key).
__global__ __launch_bounds__(NT) void hd_msum(CeArgs a, HdArgs hd) {
    __shared__ float red[NT / 64][3];
    const int K = a.K, wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const unsigned tb = __float_as_uint((float)hd.sel[0]);
    float cw[KMAX];
#pragma unroll
    for (int k = 0; k < KMAX; ++k) cw[k] = (a.cw && k < K) ? a.cw[k] : 1.f;
    for (long it = blockIdx.x; it < a.items; it += gridDim.x) {
        const long b = it / a.cpi, lo = (it - b * a.cpi) * a.clen, hi = min(lo + a.clen, a.HW);
        float sg = 0.f, wg = 0.f, we = 0.f;
        for (long e = lo + threadIdx.x; e < hi; e += NT) {
            const float l = hd.keys[b * a.HW + e];
            const unsigned kb = __float_as_uint(l);
            float wt = 1.f;
            if (a.cw) {
                bool live;
                const int t = load_label(a, b, e, lo, hi, live);
                wt = 0.f;
#pragma unroll
                for (int k = 0; k < KMAX; ++k) wt = t == k ? cw[k] : wt;
            }
            const bool on = (int)kb >= 0;
            sg += on && kb > tb ? l : 0.f;
            wg += on && kb > tb ? wt : 0.f;
            we += on && kb == tb ? wt : 0.f;
        }
        sg = wave_sum(sg);
        wg = wave_sum(wg);
        we = wave_sum(we);
        if (lane == 0) {
            red[wv][0] = sg;
            red[wv][1] = wg;
            red[wv][2] = we;
        }
        __syncthreads();
        if (threadIdx.x < 3)
            hd.msum[3 * it + threadIdx.x] = (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
        __syncthreads();
    }
}

// the access mode of a logits tensor and whether its vector form applies; dz (bwd) shares the strides
template <typename T> int ce_mode(int K, int KB, const void* z, const void* dz, long s_b, long s_k, long s_pix, int pad_ok,
                                  int* vec_ok) {
    *vec_ok = 0;
    const uintptr_t za = (uintptr_t)z, da = dz ? (uintptr_t)dz : za;
    if (s_k == 1 && s_pix >= KB && (K == KB || pad_ok)) {
        const long W = KB * (long)sizeof(T) >= 16 ? 16 / (long)sizeof(T) : KB;
        const uintptr_t wb = (uintptr_t)W * sizeof(T);
        if (za % wb == 0 && da % wb == 0 && s_pix % W == 0 && s_b % W == 0) return MODE_CL;
    }
    if (s_pix == 1) {
        const long V = ce_vec(KB, MODE_NCHW);
        // every class plane and image starts at the same offset within a vector; dz at the logits' offset
        *vec_ok = V > 1 && s_k % V == 0 && s_b % V == 0 && za % sizeof(T) == 0 &&
                  (za / sizeof(T)) % V == (da / sizeof(T)) % V && da % sizeof(T) == 0;
        return MODE_NCHW;
    }
    return MODE_GEN;
}

template <class F> void with_bucket(int KB, F&& f) {
    switch (KB) {
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

int ce_args(const char* what, int B, int K, long HW, int rows, int dtype, long s_b, long s_k, long s_pix, int label_dtype,
            float w_ce, float w_tv, bool both_zero_ok = false) {
    const std::string w(what);
    if (B < 1 || HW < 1) return fail(CSU_E_ARG, w + ": B and HW must be >= 1");
    if (K < 2 || K > KMAX) return fail(CSU_E_ARG, w + ": 2 <= K <= 32 classes (more: the caller's torch composition)");
    if (rows != 1 && rows != B) return fail(CSU_E_ARG, w + ": rows must be 1 or B");
    if (dtype != CSU_F32 && dtype != CSU_BF16) return fail(CSU_E_ARG, w + ": logits dtype must be f32 or bf16");
    if (label_dtype != 0 && label_dtype != 1) return fail(CSU_E_ARG, w + ": label_dtype must be 0 (uint8) or 1 (int64)");
    if (s_k < 1 || s_pix < 1 || s_b < 0) return fail(CSU_E_ARG, w + ": strides must be positive");
    if (!(w_ce >= 0.f) || !(w_tv >= 0.f)) return fail(CSU_E_ARG, w + ": w_ce and w_tversky must be >= 0");
    if (w_ce == 0.f && w_tv == 0.f && !both_zero_ok) return fail(CSU_E_ARG, w + ": w_ce and w_tversky are both zero");
    return 0;
}

CeArgs ce_pack(int B, int K, long HW, const void* z, long s_b, long s_k, long s_pix, int label_dtype, const void* t,
               long ignore, const float* cw) {
    const CePlan s = ce_plan(B, HW);
    CeArgs a;
    a.B = B; a.K = K; a.cpi = s.cpi; a.lab64 = label_dtype;
    a.HW = HW; a.clen = s.clen; a.items = s.items; a.s_b = s_b; a.s_k = s_k; a.s_pix = s_pix; a.ignore = ignore;
    a.z = z; a.t = t; a.cw = cw;
    return a;
}

// what the host needs for the selection of the hard-example term (hd.keys set): rho, and csu_kth_largest's workspace
struct HdSelect {
    const float* rho;
    double* hterms;
    void* kth_ws;
    size_t kth_bytes;
};

// the two forward launches and the backward launch, shared by csu_seg_ce_* (BD = false), csu_seg_bd_* and
// csu_seg_hard_* (HD; with keys the selection and its sums run between the two)
// LV: csu_seg_lovasz_fwd's first two launches; the sort and the term's own kernels follow them there
template <bool BD, bool HD = false, bool LV = false>
int ce_forward(const char* what, const CeArgs& a, const BdArgs& bd, int rows, int dtype, int pad_ok, float w_ce, float w_tv,
               float alpha, float beta, float smooth, int include_background, float* terms, float* loss, double* stats,
               float* coef, void* workspace, void* stream, const HdArgs& hd = HdArgs{0.f, nullptr, nullptr, nullptr},
               const HdSelect& hs = HdSelect{nullptr, nullptr, nullptr, 0}, const LvArgs& lv = LvArgs{nullptr, nullptr, 0u, 0}) {
    const int K = a.K, KB = ce_bucket(K);
    const int nb = (int)(a.items < CE_BLOCKS ? a.items : CE_BLOCKS);
    hipStream_t st = as_stream(stream);
    int vec_ok = 0;
    const int mode = dtype == CSU_F32 ? ce_mode<float>(K, KB, a.z, nullptr, a.s_b, a.s_k, a.s_pix, pad_ok, &vec_ok)
                                            : ce_mode<bf16>(K, KB, a.z, nullptr, a.s_b, a.s_k, a.s_pix, pad_ok, &vec_ok);
    with_flag(dtype == CSU_F32, [&](auto f32) {
        using T = std::conditional_t<decltype(f32)::value, float, bf16>;
        with_bucket(KB, [&](auto kb) {
            with_mode(mode, [&](auto md) {
                ce_partial<T, decltype(kb)::value, decltype(md)::value, BD, HD, LV>
                    <<<nb, NT, 0, st>>>(a, bd, hd, vec_ok, (float*)workspace, lv);
            });
        });
    });
    if (int e = check_launch(what)) return e;
    if constexpr (HD) {
        if (hd.keys) {
            if (int e = csu_kth_largest((long)a.B * a.HW, hd.keys, hs.rho, const_cast<double*>(hd.sel), hs.kth_ws, hs.kth_bytes,
                                        stream))
                return e;
            hd_msum<<<nb, NT, 0, st>>>(a, hd);
            if (int e = check_launch(what)) return e;
        }
    }
    ce_finish<BD, HD><<<1, NT, 0, st>>>(a.B, K, a.cpi, rows, (const float*)workspace, w_ce, w_tv, alpha, beta, smooth,
                                        include_background != 0, bd, hd, terms, hs.hterms, loss, stats, coef);
    return check_launch(what);
}

template <bool BD, bool HD = false, bool LV = false>
int ce_backward_launch(const char* what, const CeArgs& a, const BdArgs& bd, int rows, int dtype, int pad_ok, float w_ce,
                       float w_tv, int include_background, const float* dloss, const float* coef, void* dz, void* stream,
                       const HdArgs& hd = HdArgs{0.f, nullptr, nullptr, nullptr}) {
    const int K = a.K, KB = ce_bucket(K);
    const int nb = (int)(a.items < CE_BLOCKS ? a.items : CE_BLOCKS);
    hipStream_t st = as_stream(stream);
    int vec_ok = 0;
    const int mode = dtype == CSU_F32 ? ce_mode<float>(K, KB, a.z, dz, a.s_b, a.s_k, a.s_pix, pad_ok, &vec_ok)
                                            : ce_mode<bf16>(K, KB, a.z, dz, a.s_b, a.s_k, a.s_pix, pad_ok, &vec_ok);
    const float tv_scale = w_tv / ((float)rows * (float)(include_background ? K : K - 1));
    with_flag(dtype == CSU_F32, [&](auto f32) {
        using T = std::conditional_t<decltype(f32)::value, float, bf16>;
        with_bucket(KB, [&](auto kb) {
            with_mode(mode, [&](auto md) {
                if constexpr (BD)   // the gated pair: see ce_backward
                    ce_backward<T, decltype(kb)::value, decltype(md)::value, false, false>
                        <<<nb, NT, 0, st>>>(a, bd, hd, vec_ok, rows, dloss, coef, w_ce, tv_scale, (T*)dz);
                ce_backward<T, decltype(kb)::value, decltype(md)::value, BD, HD, LV>
                    <<<nb, NT, 0, st>>>(a, bd, hd, vec_ok, rows, dloss, coef, w_ce, tv_scale, (T*)dz);
            });
        });
    });
    return check_launch(what);
}

}  // namespace
}  // namespace csu

using namespace csu;

extern "C" size_t csu_seg_ce_workspace(int B, int K, long HW) {
    if (B < 1 || HW < 1 || K < 2 || K > KMAX) return 0;
    return (size_t)ce_plan(B, HW).items * ce_nsum(K) * sizeof(float);
}

extern "C" int csu_seg_ce_fwd(int B, int K, long HW, int rows, int dtype, const void* z, long s_b, long s_k, long s_pix,
                              int pad_ok, int label_dtype, const void* t, long ignore_index, const float* class_weight,
                              float w_ce, float w_tversky, float alpha, float beta, float smooth, int include_background,
                              float* loss, double* stats, float* coef, void* workspace, size_t ws_bytes, void* stream) {
    if (int e = ce_args("seg_ce_fwd", B, K, HW, rows, dtype, s_b, s_k, s_pix, label_dtype, w_ce, w_tversky)) return e;
    if (!(alpha >= 0.f) || !(beta >= 0.f)) return fail(CSU_E_ARG, "seg_ce_fwd: alpha and beta must be >= 0");
    if (!(smooth > 0.f)) return fail(CSU_E_ARG, "seg_ce_fwd: smooth must be > 0");
    if (!z || !t || !loss || !coef) return fail(CSU_E_ARG, "seg_ce_fwd: null z, t, loss or coef");
    if (!workspace || ws_bytes < csu_seg_ce_workspace(B, K, HW)) return fail(CSU_E_WORKSPACE, "seg_ce_fwd: workspace");
    const CeArgs a = ce_pack(B, K, HW, z, s_b, s_k, s_pix, label_dtype, t, ignore_index, class_weight);
    return ce_forward<false>("seg_ce_fwd", a, BdArgs{nullptr, nullptr, 0}, rows, dtype, pad_ok, w_ce, w_tversky, alpha, beta,
                             smooth, include_background, nullptr, loss, stats, coef, workspace, stream);
}

extern "C" int csu_seg_ce_bwd(int B, int K, long HW, int rows, int dtype, const void* z, long s_b, long s_k, long s_pix,
                              int pad_ok, int label_dtype, const void* t, long ignore_index, const float* class_weight,
                              const float* dloss, const float* coef, float w_ce, float w_tversky, int include_background,
                              void* dz, void* stream) {
    if (int e = ce_args("seg_ce_bwd", B, K, HW, rows, dtype, s_b, s_k, s_pix, label_dtype, w_ce, w_tversky)) return e;
    if (!z || !t || !dloss || !coef || !dz) return fail(CSU_E_ARG, "seg_ce_bwd: null z, t, dloss, coef or dz");
    const CeArgs a = ce_pack(B, K, HW, z, s_b, s_k, s_pix, label_dtype, t, ignore_index, class_weight);
    return ce_backward_launch<false>("seg_ce_bwd", a, BdArgs{nullptr, nullptr, 0}, rows, dtype, pad_ok, w_ce, w_tversky,
                                     include_background, dloss, coef, dz, stream);
}

// ---- the same loss with the boundary term: + w_bd[0] BD ---------------------------------------------
extern "C" size_t csu_seg_bd_workspace(int B, int K, long HW) {
    if (B < 1 || HW < 1 || K < 2 || K > KMAX) return 0;
    return (size_t)ce_plan(B, HW).items * (ce_nsum(K) + 1) * sizeof(float);
}

extern "C" int csu_seg_bd_fwd(int B, int K, long HW, int rows, int dtype, const void* z, long s_b, long s_k, long s_pix,
                              int pad_ok, int label_dtype, const void* t, long ignore_index, const float* class_weight,
                              float w_ce, float w_tversky, float alpha, float beta, float smooth, int include_background,
                              const float* phi, const float* w_bd, int bd_background, float* loss, float* terms,
                              double* stats, float* coef, void* workspace, size_t ws_bytes, void* stream) {
    if (int e = ce_args("seg_bd_fwd", B, K, HW, rows, dtype, s_b, s_k, s_pix, label_dtype, w_ce, w_tversky, true)) return e;
    if (!(alpha >= 0.f) || !(beta >= 0.f)) return fail(CSU_E_ARG, "seg_bd_fwd: alpha and beta must be >= 0");
    if (!(smooth > 0.f)) return fail(CSU_E_ARG, "seg_bd_fwd: smooth must be > 0");
    if (!z || !t || !loss || !coef || !terms) return fail(CSU_E_ARG, "seg_bd_fwd: null z, t, loss, terms or coef");
    if (!phi || !w_bd) return fail(CSU_E_ARG, "seg_bd_fwd: null phi or w_bd");
    if (!workspace || ws_bytes < csu_seg_bd_workspace(B, K, HW)) return fail(CSU_E_WORKSPACE, "seg_bd_fwd: workspace");
    const CeArgs a = ce_pack(B, K, HW, z, s_b, s_k, s_pix, label_dtype, t, ignore_index, class_weight);
    return ce_forward<true>("seg_bd_fwd", a, BdArgs{phi, w_bd, bd_background != 0}, rows, dtype, pad_ok, w_ce, w_tversky, alpha,
                            beta, smooth, include_background, terms, loss, stats, coef, workspace, stream);
}

extern "C" int csu_seg_bd_bwd(int B, int K, long HW, int rows, int dtype, const void* z, long s_b, long s_k, long s_pix,
                              int pad_ok, int label_dtype, const void* t, long ignore_index, const float* class_weight,
                              const float* dloss, const float* coef, float w_ce, float w_tversky, int include_background,
                              const float* phi, const float* w_bd, int bd_background, void* dz, void* stream) {
    if (int e = ce_args("seg_bd_bwd", B, K, HW, rows, dtype, s_b, s_k, s_pix, label_dtype, w_ce, w_tversky, true)) return e;
    if (!z || !t || !dloss || !coef || !dz) return fail(CSU_E_ARG, "seg_bd_bwd: null z, t, dloss, coef or dz");
    if (!phi || !w_bd) return fail(CSU_E_ARG, "seg_bd_bwd: null phi or w_bd");
    const CeArgs a = ce_pack(B, K, HW, z, s_b, s_k, s_pix, label_dtype, t, ignore_index, class_weight);
    return ce_backward_launch<true>("seg_bd_bwd", a, BdArgs{phi, w_bd, bd_background != 0}, rows, dtype, pad_ok, w_ce, w_tversky,
                                    include_background, dloss, coef, dz, stream);
}

// ---- the same loss with the hard-example CE term: focal weighting and / or a top-k selection --------
namespace csu {
namespace {
// workspace: csu_kth_largest's, its five doubles, then the (2 + 5 K) partial sums and the 3 selected sums per item
struct HdLayout {
    size_t kth, sel, partial, msum, total;
};
HdLayout hd_layout(int B, int K, long HW) {
    HdLayout l;
    const size_t items = (size_t)ce_plan(B, HW).items;
    l.kth = csu_kth_largest_workspace((long)B * HW);
    l.sel = l.kth;
    l.partial = l.sel + 6 * sizeof(double);
    l.msum = l.partial + items * ce_nsum(K) * sizeof(float);
    l.total = (l.msum + items * 3 * sizeof(float) + 7) & ~(size_t)7;
    return l;
}
}  // namespace
}  // namespace csu

extern "C" size_t csu_seg_hard_workspace(int B, int K, long HW) {
    if (B < 1 || HW < 1 || K < 2 || K > KMAX) return 0;
    return hd_layout(B, K, HW).total;
}

extern "C" int csu_seg_hard_fwd(int B, int K, long HW, int rows, int dtype, const void* z, long s_b, long s_k, long s_pix,
                                int pad_ok, int label_dtype, const void* t, long ignore_index, const float* class_weight,
                                float w_ce, float w_tversky, float alpha, float beta, float smooth, int include_background,
                                float gamma, const float* rho, float* keys, float* loss, double* terms, double* stats,
                                float* coef, void* workspace, size_t ws_bytes, void* stream) {
    if (int e = ce_args("seg_hard_fwd", B, K, HW, rows, dtype, s_b, s_k, s_pix, label_dtype, w_ce, w_tversky)) return e;
    if (!(alpha >= 0.f) || !(beta >= 0.f)) return fail(CSU_E_ARG, "seg_hard_fwd: alpha and beta must be >= 0");
    if (!(smooth > 0.f)) return fail(CSU_E_ARG, "seg_hard_fwd: smooth must be > 0");
    if (!(gamma >= 0.f) || gamma == INFINITY) return fail(CSU_E_ARG, "seg_hard_fwd: gamma must be finite and >= 0");
    if (!z || !t || !loss || !coef || !terms) return fail(CSU_E_ARG, "seg_hard_fwd: null z, t, loss, terms or coef");
    if ((rho != nullptr) != (keys != nullptr)) return fail(CSU_E_ARG, "seg_hard_fwd: rho and keys go together");
    if (!workspace || ((uintptr_t)workspace & 7) || ws_bytes < csu_seg_hard_workspace(B, K, HW))
        return fail(CSU_E_WORKSPACE, "seg_hard_fwd: workspace (8-byte aligned)");
    const CeArgs a = ce_pack(B, K, HW, z, s_b, s_k, s_pix, label_dtype, t, ignore_index, class_weight);
    const HdLayout l = hd_layout(B, K, HW);
    char* ws = (char*)workspace;
    const HdArgs hd{gamma, keys, (const double*)(ws + l.sel), (float*)(ws + l.msum)};
    return ce_forward<false, true>("seg_hard_fwd", a, BdArgs{nullptr, nullptr, 0}, rows, dtype, pad_ok, w_ce, w_tversky, alpha,
                                   beta, smooth, include_background, nullptr, loss, stats, coef, ws + l.partial, stream, hd,
                                   HdSelect{rho, terms, ws, l.kth});
}

extern "C" int csu_seg_hard_bwd(int B, int K, long HW, int rows, int dtype, const void* z, long s_b, long s_k, long s_pix,
                                int pad_ok, int label_dtype, const void* t, long ignore_index, const float* class_weight,
                                const float* dloss, const float* coef, float w_ce, float w_tversky, int include_background,
                                float gamma, const float* keys, void* dz, void* stream) {
    if (int e = ce_args("seg_hard_bwd", B, K, HW, rows, dtype, s_b, s_k, s_pix, label_dtype, w_ce, w_tversky)) return e;
    if (!(gamma >= 0.f) || gamma == INFINITY) return fail(CSU_E_ARG, "seg_hard_bwd: gamma must be finite and >= 0");
    if (!z || !t || !dloss || !coef || !dz) return fail(CSU_E_ARG, "seg_hard_bwd: null z, t, dloss, coef or dz");
    const CeArgs a = ce_pack(B, K, HW, z, s_b, s_k, s_pix, label_dtype, t, ignore_index, class_weight);
    return ce_backward_launch<false, true>("seg_hard_bwd", a, BdArgs{nullptr, nullptr, 0}, rows, dtype, pad_ok, w_ce, w_tversky,
                                           include_background, dloss, coef, dz, stream,
                                           HdArgs{gamma, const_cast<float*>(keys), nullptr, nullptr});
}

// ---- the same loss with the Lovasz-Softmax term: + w_lv[0] LS --------------------------------------
// After ce_partial<LV> has left the keys and values and csu_sort_pairs has put every segment in descending e:
//   lv_count   the foreground pixels of every tile of LT sorted pairs -> cnt[segment][tile]
//   lv_scan    one workgroup per segment: the exclusive scan of its row of cnt in place, G[segment] = the total
//   lv_coef    per tile: the scan within the tile on top of the tile's prefix gives F of every pair; from the integers
//              I = G - F, U = I + (j - 1) the increment g in fp64, psi = -/+ g scale rounded once to fp32 and stored
//              at the pair's pixel, and the tile's sum of e g in fp64 (a thread's 8 pairs in order, then a fixed
//              tree) -> lsum[segment][tile].  A dead pair (bit 30 of the key) gets psi = 0 and adds nothing.
//   lv_finish  one workgroup: LS = sum over segments of scale (sum over tiles of lsum), in a fixed order; terms,
//              loss[0] += w_lv[0] LS on top of ce_finish's, and the 1 behind 1 / sum w in coef.
namespace csu {
namespace {

constexpr int LV_EPT = 8;
constexpr int LT = NT * LV_EPT;   // 2048 pairs per tile
constexpr int LV_BLOCKS = 1 << 18;

struct LvPlan {
    long len, ntl, items, segs;   // a segment's pairs, its tiles, segs * ntl
    int B, nc, per_image, present_only;
};

LvPlan lv_plan(int B, long HW, unsigned mask, int per_image, int present_only) {
    LvPlan p;
    p.B = B;
    p.nc = __builtin_popcount(mask);
    p.per_image = per_image != 0;
    p.present_only = present_only != 0;
    p.segs = p.per_image ? (long)p.nc * B : p.nc;
    p.len = p.per_image ? HW : (long)B * HW;
    p.ntl = (p.len + LT - 1) / LT;
    p.items = p.segs * p.ntl;
    return p;
}

// scale of a segment: [it counts] / (number counted x (B if per_image else 1)); counted within the segment's image
__device__ __forceinline__ double lv_scale(const LvPlan& p, const unsigned* __restrict__ G, long seg) {
    const long b = p.per_image ? seg % p.B : 0, stride = p.per_image ? p.B : 1;
    int present = 0;
    for (int m = 0; m < p.nc; ++m) present += G[m * stride + b] > 0u ? 1 : 0;
    const int counted = p.present_only ? present : p.nc;
    const bool on = !p.present_only || G[seg] > 0u;
    return on ? 1.0 / ((double)(counted > 1 ? counted : 1) * (double)(p.per_image ? p.B : 1)) : 0.0;
}

__global__ __launch_bounds__(NT) void lv_count(const unsigned* __restrict__ vals, LvPlan p, unsigned* __restrict__ cnt) {
    __shared__ unsigned wsum[NT / 64];
    for (long it = blockIdx.x; it < p.items; it += gridDim.x) {
        const long seg = it / p.ntl, tile = it - seg * p.ntl, first = tile * LT;
        const int n = (int)min((long)LT, p.len - first);
        const unsigned* v = vals + seg * p.len + first;
        unsigned c = 0;
        for (int i = threadIdx.x; i < n; i += NT) c += v[i] >> 31;
        unsigned total;
        block_scan<NT>(c, wsum, total);
        if (threadIdx.x == 0) cnt[it] = total;
    }
}

__global__ __launch_bounds__(NT) void lv_scan(unsigned* __restrict__ cnt, unsigned* __restrict__ G, LvPlan p) {
    __shared__ unsigned wsum[NT / 64];
    for (long seg = blockIdx.x; seg < p.segs; seg += gridDim.x) {
        unsigned* row = cnt + seg * p.ntl;
        unsigned carry = 0;
        for (long c0 = 0; c0 < p.ntl; c0 += NT) {
            const long i = c0 + threadIdx.x;
            const unsigned v = i < p.ntl ? row[i] : 0u;
            unsigned total;
            const unsigned inc = block_scan<NT>(v, wsum, total);
            if (i < p.ntl) row[i] = carry + inc - v;
            carry += total;
        }
        if (threadIdx.x == 0) G[seg] = carry;
    }
}

__global__ __launch_bounds__(NT) void lv_coef(const unsigned* __restrict__ keys, const unsigned* __restrict__ vals, LvPlan p,
                                              const unsigned* __restrict__ cnt, const unsigned* __restrict__ G,
                                              float* __restrict__ psi, double* __restrict__ lsum) {
    __shared__ unsigned wsum[NT / 64];
    __shared__ double red[NT / 64];
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (long it = blockIdx.x; it < p.items; it += gridDim.x) {
        const long seg = it / p.ntl, tile = it - seg * p.ntl, first = tile * LT;
        const int n = (int)min((long)LT, p.len - first);
        const unsigned* k = keys + seg * p.len + first;
        const unsigned* v = vals + seg * p.len + first;
        float* out = psi + seg * p.len;
        const double scale = lv_scale(p, G, seg);
        const long Gs = G[seg];
        unsigned key[LV_EPT], val[LV_EPT], mine = 0;
        const int i0 = threadIdx.x * LV_EPT;
#pragma unroll
        for (int r = 0; r < LV_EPT; ++r) {
            const bool valid = i0 + r < n;
            key[r] = valid ? k[i0 + r] : LV_DEAD;
            val[r] = valid ? v[i0 + r] : 0u;
            mine += val[r] >> 31;
        }
        unsigned total;
        long F = (long)cnt[it] + (block_scan<NT>(mine, wsum, total) - mine);   // the foreground pairs before this thread's
        double acc = 0.0;
#pragma unroll
        for (int r = 0; r < LV_EPT; ++r) {
            const bool fg = (val[r] >> 31) != 0, live = (key[r] & LV_DEAD) == 0;
            const long I = Gs - F, U = I + (first + i0 + r);   // j - 1 = the pair's place in the segment
            const double g = fg ? 1.0 / (double)U : U == 0 ? 1.0 : (double)I / ((double)U * (double)(U + 1));
            const float e = __uint_as_float(LV_ONE - key[r]);
            acc += live ? (double)e * g : 0.0;
            const long at = val[r] & 0x7FFFFFFFu;
            if (i0 + r < n && at < p.len) out[at] = live ? (float)((fg ? -g : g) * scale) : 0.f;
            F += fg ? 1 : 0;
        }
        acc = wave_sum_d(acc);
        if (lane == 0) red[wv] = acc;
        __syncthreads();
        if (threadIdx.x == 0) lsum[it] = (red[0] + red[1]) + (red[2] + red[3]);
        __syncthreads();
    }
}

__global__ __launch_bounds__(NT) void lv_finish(const double* __restrict__ lsum, const unsigned* __restrict__ G, LvPlan p,
                                                const float* __restrict__ w_lv, float* __restrict__ loss,
                                                float* __restrict__ terms, float* __restrict__ coef_one) {
    __shared__ double red[NT / 64];
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    double ls = 0.0;
    for (long seg = wv; seg < p.segs; seg += NT / 64) {
        double s = 0.0;
        for (long i = lane; i < p.ntl; i += 64) s += lsum[seg * p.ntl + i];
        ls += wave_sum_d(s) * lv_scale(p, G, seg);
    }
    if (lane == 0) red[wv] = ls;
    __syncthreads();
    if (threadIdx.x == 0) {
        const double LS = (red[0] + red[1]) + (red[2] + red[3]);
        const float base = loss[0];
        terms[0] = base;
        terms[1] = (float)LS;
        loss[0] = (float)((double)base + (double)w_lv[0] * LS);
        coef_one[0] = 1.f;
    }
}

// workspace: the (2 + 5 K) partial sums per item, the tile sums (fp64), the sort's scratch pairs and workspace, the
// tile counts and the segment totals
struct LvLayout {
    size_t partial, lsum, kalt, valt, sort, sort_bytes, cnt, G, total;
};
LvLayout lv_layout(int B, int K, long HW, const LvPlan& p) {
    LvLayout l;
    const size_t N = (size_t)p.nc * B * HW;
    l.partial = 0;
    l.lsum = ((size_t)ce_plan(B, HW).items * ce_nsum(K) * sizeof(float) + 7) & ~(size_t)7;
    l.kalt = l.lsum + (size_t)p.items * sizeof(double);
    l.valt = l.kalt + N * sizeof(unsigned);
    l.sort = l.valt + N * sizeof(unsigned);
    l.sort_bytes = csu_sort_pairs_workspace((int)p.segs, p.len);
    l.cnt = l.sort + l.sort_bytes;
    l.G = l.cnt + (size_t)p.items * sizeof(unsigned);
    l.total = (l.G + (size_t)p.segs * sizeof(unsigned) + 7) & ~(size_t)7;
    return l;
}

bool lv_mask_ok(int B, int K, long HW, unsigned mask) {
    if (mask == 0 || (K < 32 && (mask >> K) != 0)) return false;
    return (long)__builtin_popcount(mask) * B * HW < (1L << 31);
}

}  // namespace
}  // namespace csu

extern "C" size_t csu_seg_lovasz_workspace(int B, int K, long HW, uint32_t class_mask, int per_image) {
    if (B < 1 || HW < 1 || K < 2 || K > KMAX || HW >= (1L << 31) || !lv_mask_ok(B, K, HW, class_mask)) return 0;
    return lv_layout(B, K, HW, lv_plan(B, HW, class_mask, per_image, 0)).total;
}

extern "C" int csu_seg_lovasz_fwd(int B, int K, long HW, int rows, int dtype, const void* z, long s_b, long s_k, long s_pix,
                                  int pad_ok, int label_dtype, const void* t, long ignore_index, const float* class_weight,
                                  float w_ce, float w_tversky, float alpha, float beta, float smooth, int include_background,
                                  uint32_t class_mask, int present_only, int per_image, const float* w_lv,
                                  uint32_t* sorted_keys, uint32_t* sorted_vals, float* psi, float* loss, float* terms,
                                  double* stats, float* coef, void* workspace, size_t ws_bytes, void* stream) {
    if (int e = ce_args("seg_lovasz_fwd", B, K, HW, rows, dtype, s_b, s_k, s_pix, label_dtype, w_ce, w_tversky, true)) return e;
    if (!(alpha >= 0.f) || !(beta >= 0.f)) return fail(CSU_E_ARG, "seg_lovasz_fwd: alpha and beta must be >= 0");
    if (!(smooth > 0.f)) return fail(CSU_E_ARG, "seg_lovasz_fwd: smooth must be > 0");
    if (HW >= (1L << 31) || !lv_mask_ok(B, K, HW, class_mask))
        return fail(CSU_E_ARG, "seg_lovasz_fwd: class_mask needs a bit, none at or above K, and |C| B HW < 2^31");
    if (!z || !t || !loss || !coef || !terms) return fail(CSU_E_ARG, "seg_lovasz_fwd: null z, t, loss, terms or coef");
    if (!w_lv || !sorted_keys || !sorted_vals || !psi)
        return fail(CSU_E_ARG, "seg_lovasz_fwd: null w_lv, sorted_keys, sorted_vals or psi");
    if (((uintptr_t)sorted_keys | (uintptr_t)sorted_vals | (uintptr_t)psi) & 3)
        return fail(CSU_E_ARG, "seg_lovasz_fwd: sorted_keys, sorted_vals or psi misaligned");
    if (!workspace || ((uintptr_t)workspace & 7) || ws_bytes < csu_seg_lovasz_workspace(B, K, HW, class_mask, per_image))
        return fail(CSU_E_WORKSPACE, "seg_lovasz_fwd: workspace (8-byte aligned)");
    const CeArgs a = ce_pack(B, K, HW, z, s_b, s_k, s_pix, label_dtype, t, ignore_index, class_weight);
    const LvPlan p = lv_plan(B, HW, class_mask, per_image, present_only);
    const LvLayout l = lv_layout(B, K, HW, p);
    char* ws = (char*)workspace;
    if (int e = ce_forward<false, false, true>("seg_lovasz_fwd", a, BdArgs{nullptr, nullptr, 0}, rows, dtype, pad_ok, w_ce,
                                               w_tversky, alpha, beta, smooth, include_background, nullptr, loss, stats, coef,
                                               ws + l.partial, stream, HdArgs{0.f, nullptr, nullptr, nullptr},
                                               HdSelect{nullptr, nullptr, nullptr, 0},
                                               LvArgs{sorted_keys, sorted_vals, class_mask, p.per_image}))
        return e;
    if (int e = csu_sort_pairs((int)p.segs, p.len, 31, sorted_keys, sorted_vals, (uint32_t*)(ws + l.kalt),
                               (uint32_t*)(ws + l.valt), ws + l.sort, l.sort_bytes, stream))
        return e;
    hipStream_t st = as_stream(stream);
    const int nb = (int)(p.items < LV_BLOCKS ? p.items : LV_BLOCKS);
    const int nsb = (int)(p.segs < LV_BLOCKS ? p.segs : LV_BLOCKS);
    unsigned* cnt = (unsigned*)(ws + l.cnt);
    unsigned* G = (unsigned*)(ws + l.G);
    double* lsum = (double*)(ws + l.lsum);
    lv_count<<<nb, NT, 0, st>>>(sorted_vals, p, cnt);
    lv_scan<<<nsb, NT, 0, st>>>(cnt, G, p);
    lv_coef<<<nb, NT, 0, st>>>(sorted_keys, sorted_vals, p, cnt, G, psi, lsum);
    lv_finish<<<1, NT, 0, st>>>(lsum, G, p, w_lv, loss, terms, coef + 2 * (long)rows * K + 1);
    return check_launch("seg_lovasz_fwd");
}

extern "C" int csu_seg_lovasz_bwd(int B, int K, long HW, int rows, int dtype, const void* z, long s_b, long s_k, long s_pix,
                                  int pad_ok, int label_dtype, const void* t, long ignore_index, const float* class_weight,
                                  const float* dloss, const float* coef, float w_ce, float w_tversky, int include_background,
                                  uint32_t class_mask, const float* psi, const float* w_lv, void* dz, void* stream) {
    if (int e = ce_args("seg_lovasz_bwd", B, K, HW, rows, dtype, s_b, s_k, s_pix, label_dtype, w_ce, w_tversky, true)) return e;
    if (HW >= (1L << 31) || !lv_mask_ok(B, K, HW, class_mask))
        return fail(CSU_E_ARG, "seg_lovasz_bwd: class_mask needs a bit, none at or above K, and |C| B HW < 2^31");
    if (!z || !t || !dloss || !coef || !dz) return fail(CSU_E_ARG, "seg_lovasz_bwd: null z, t, dloss, coef or dz");
    if (!psi || !w_lv) return fail(CSU_E_ARG, "seg_lovasz_bwd: null psi or w_lv");
    const CeArgs a = ce_pack(B, K, HW, z, s_b, s_k, s_pix, label_dtype, t, ignore_index, class_weight);
    return ce_backward_launch<true, false, true>("seg_lovasz_bwd", a, BdArgs{psi, w_lv, (int)class_mask}, rows, dtype, pad_ok,
                                                 w_ce, w_tversky, include_background, dloss, coef, dz, stream);
}
