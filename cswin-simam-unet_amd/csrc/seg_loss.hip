// Fused segmentation training loss  w_bce * BCE + w_tversky * mean_r(1 - Tversky_r)  on fp32
// probabilities p and targets t viewed as rows x L (rows = 1: batch-flattened, the form of the
// reference's Dice metric cswin:692-698; rows = B: per image), with the reference loop's
// thresholded Dice / IoU sums (cswin:789-795) from the same pass.  Per row r:
//   TP = sum p t, P = sum p, T = sum t, D = (1 - a - b) TP + a P + b T + smooth, TI = (TP + smooth) / D
//   BCE = (1 / n) sum -(pos_weight t max(log p, -100) + (1 - t) max(log1p(-p), -100))
// Dice is a = b = 0.5 with smooth = s / 2.
//
// Work split: every row is cut into cpr chunks of clen elements (clen % 4 == 0); one workgroup
// reduces one (row, chunk) item at a time, so the row -- and in backward its two coefficients -- is
// uniform per workgroup and no per-element division by L is needed.  Items beyond the grid are
// walked grid-stride (rows above the grid size), a long row gets up to SEG_BLOCKS / rows chunks
// (rows below it).
//   forward 1  seg_partial: 6 sums per item (BCE, TP, P, T and the hard sums sum[p > .5] t,
//              sum[p > .5]) -> workspace[item][6]; per thread a fixed element order, then a fixed
//              shuffle + LDS tree.  No atomics.
//   forward 2  seg_finish (one workgroup): wave w sums the chunks of rows w, w + 4, ... (lanes
//              stride the chunks, xor-shuffle tree), in fp64; writes loss, stats and per row
//              coef = (A, C), A = (D - (TP + smooth)(1 - a - b)) / D^2, C = a (TP + smooth) / D^2.
//   backward   seg_backward: dp = dloss (w_bce (p (1 - t) - pos_weight t (1 - p)) / max(p (1 - p), 1e-12) / n
//                                       - (w_tversky / rows) (t A_r - C_r)).
// Alignment: a chunk starts at element r L + c clen, which is off a 16-B boundary whenever L % 4 != 0
// (or the tensors are views).  Each chunk is walked as  scalar head (up to the first 16-B boundary
// of p) | 16-B vectors | scalar tail;  when p, t (and dp) do not share their offset within 16 B
// the whole chunk takes the scalar path.  The summation order is a function of (n, rows, address
// mod 16) only: equal inputs in equally aligned buffers give bitwise equal results.
#include "common.hpp"

namespace csu {
namespace {

constexpr int NT = 256;
constexpr int SEG_BLOCKS = 1024;
constexpr int NSUM = 6;   // BCE, TP, P, T, hard TP, hard P

struct SegPlan {
    long L, clen, items;
    int cpr;
};

SegPlan seg_plan(long n, int rows) {
    SegPlan s;
    s.L = n / rows;
    const long maxc = rows < SEG_BLOCKS ? SEG_BLOCKS / rows : 1;
    long cpr = (s.L + 4 * NT - 1) / (4 * NT);
    cpr = cpr < 1 ? 1 : cpr > maxc ? maxc : cpr;
    s.clen = ((s.L + cpr - 1) / cpr + 3) & ~3L;
    s.cpr = (int)((s.L + s.clen - 1) / s.clen);
    s.items = (long)rows * s.cpr;
    return s;
}

// elements in front of the first 16-B boundary at or after a
__device__ __forceinline__ long head_of(const void* a) { return (long)(((16 - ((uintptr_t)a & 15)) & 15) >> 2); }

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__global__ __launch_bounds__(NT) void seg_partial(long L, long clen, int cpr, long items, const float* __restrict__ p,
                                                  const float* __restrict__ t, int bce, float pw,
                                                  float* __restrict__ partial) {
    __shared__ float red[NSUM][NT / 64];
    for (long it = blockIdx.x; it < items; it += gridDim.x) {
        const long r = it / cpr, c0 = (it - r * cpr) * clen;
        const long len = min(clen, L - c0);
        const float* pp = p + r * L + c0;
        const float* tt = t + r * L + c0;
        float s = 0.f, tp = 0.f, sp = 0.f, st = 0.f, hi = 0.f, hp = 0.f;
        auto acc = [&](float pv, float tv) {
            if (bce) {   // ATen's binary_cross_entropy clamps and log1p (glue.hip bce_term), target term weighted
                const float lp = fmaxf(logf(pv), -100.f), lq = fmaxf(log1pf(-pv), -100.f);
                s += (tv - 1.f) * lq - (pw * tv) * lp;
            }
            tp += pv * tv;
            sp += pv;
            st += tv;
            const float pr = pv > 0.5f ? 1.f : 0.f;
            hi += pr * tv;
            hp += pr;
        };
        const bool vec = ((((uintptr_t)pp) ^ ((uintptr_t)tt)) & 15) == 0;
        const long head = vec ? min(head_of(pp), len) : len;
        const long nv = (len - head) >> 2;
        for (long e = threadIdx.x; e < head; e += NT) acc(pp[e], tt[e]);
        for (long v = threadIdx.x; v < nv; v += NT) {
            float pv[4], tv[4];
            load4(pp + head + 4 * v, pv);
            load4(tt + head + 4 * v, tv);
#pragma unroll
            for (int j = 0; j < 4; ++j) acc(pv[j], tv[j]);
        }
        for (long e = head + 4 * nv + threadIdx.x; e < len; e += NT) acc(pp[e], tt[e]);
        const float v[NSUM] = {s, tp, sp, st, hi, hp};
#pragma unroll
        for (int k = 0; k < NSUM; ++k) {
            const float w = wave_sum(v[k]);
            if ((threadIdx.x & 63) == 0) red[k][threadIdx.x >> 6] = w;
        }
        __syncthreads();
        if (threadIdx.x < NSUM) {
            const int k = threadIdx.x;
            partial[it * NSUM + k] = (red[k][0] + red[k][1]) + (red[k][2] + red[k][3]);
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(NT) void seg_finish(int rows, int cpr, long n, const float* __restrict__ partial, float w_bce,
                                                 float w_tv, float alpha, float beta, float smooth,
                                                 float* __restrict__ loss, float* __restrict__ stats,
                                                 float* __restrict__ coef) {
    __shared__ double red[5][NT / 64];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const double a = alpha, b = beta, g = 1.0 - a - b;
    double abce = 0., atv = 0., ahi = 0., ahp = 0., at = 0.;   // identical in every lane of a wave
    for (int r = w; r < rows; r += NT / 64) {
        double s[NSUM] = {0., 0., 0., 0., 0., 0.};
        for (int c = lane; c < cpr; c += 64) {
            const float* q = partial + ((long)r * cpr + c) * NSUM;
#pragma unroll
            for (int k = 0; k < NSUM; ++k) s[k] += (double)q[k];
        }
#pragma unroll
        for (int k = 0; k < NSUM; ++k) s[k] = wave_sum_d(s[k]);
        const double TP = s[1], P = s[2], T = s[3];
        const double num = TP + (double)smooth, D = g * TP + a * P + b * T + (double)smooth, inv = 1.0 / D;
        if (lane == 0) {
            coef[2 * (long)r] = (float)((D - num * g) * inv * inv);
            coef[2 * (long)r + 1] = (float)(a * num * inv * inv);
        }
        abce += s[0];
        atv += (a * (P - TP) + b * (T - TP)) * inv;   // 1 - TI without the cancellation of 1 - num / D
        ahi += s[4];
        ahp += s[5];
        at += T;
    }
    if (lane == 0) {
        red[0][w] = abce;
        red[1][w] = atv;
        red[2][w] = ahi;
        red[3][w] = ahp;
        red[4][w] = at;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double tot[5];
#pragma unroll
        for (int k = 0; k < 5; ++k) tot[k] = (red[k][0] + red[k][1]) + (red[k][2] + red[k][3]);
        loss[0] = (float)((double)w_bce * tot[0] / (double)n + (double)w_tv * tot[1] / (double)rows);
        if (stats) {
            stats[0] = (float)tot[2];
            stats[1] = (float)tot[3];
            stats[2] = (float)tot[4];
        }
    }
}

__global__ __launch_bounds__(NT) void seg_backward(long L, long clen, int cpr, long items, const float* __restrict__ p,
                                                   const float* __restrict__ t, const float* __restrict__ dloss,
                                                   const float* __restrict__ coef, float w_bce, float pw, float w_tv_rows,
                                                   float inv_n, float* __restrict__ dp) {
    const float g = dloss[0], gb = g * w_bce, gt = g * w_tv_rows;
    for (long it = blockIdx.x; it < items; it += gridDim.x) {
        const long r = it / cpr, c0 = (it - r * cpr) * clen;
        const long len = min(clen, L - c0);
        const float* pp = p + r * L + c0;
        const float* tt = t + r * L + c0;
        float* dd = dp + r * L + c0;
        const float A = coef[2 * r], C = coef[2 * r + 1];
        auto grad = [&](float pv, float tv) {
            float o = 0.f;
            // at pos_weight 1 and t in {0, 1} the numerator is bce_backward's p - t (glue.hip), same clamp
            if (w_bce != 0.f)
                o = (gb * (pv * (1.f - tv) - (pw * tv) * (1.f - pv)) / fmaxf((1.f - pv) * pv, 1e-12f)) * inv_n;
            return o - gt * (tv * A - C);
        };
        const bool vec = (((((uintptr_t)pp) ^ ((uintptr_t)tt)) | (((uintptr_t)pp) ^ ((uintptr_t)dd))) & 15) == 0;
        const long head = vec ? min(head_of(pp), len) : len;
        const long nv = (len - head) >> 2;
        for (long e = threadIdx.x; e < head; e += NT) dd[e] = grad(pp[e], tt[e]);
        for (long v = threadIdx.x; v < nv; v += NT) {
            float pv[4], tv[4], o[4];
            load4(pp + head + 4 * v, pv);
            load4(tt + head + 4 * v, tv);
#pragma unroll
            for (int j = 0; j < 4; ++j) o[j] = grad(pv[j], tv[j]);
            store4(dd + head + 4 * v, o);
        }
        for (long e = head + 4 * nv + threadIdx.x; e < len; e += NT) dd[e] = grad(pp[e], tt[e]);
    }
}

int seg_args(const char* what, long n, int rows, float w_bce, float pos_weight, float w_tversky) {
    const std::string w(what);
    if (n < 1 || rows < 1) return fail(CSU_E_ARG, w + ": n and rows must be >= 1");
    if (n % rows) return fail(CSU_E_ARG, w + ": n must be a multiple of rows");
    if (!(w_bce >= 0.f) || !(w_tversky >= 0.f) || !(pos_weight >= 0.f))
        return fail(CSU_E_ARG, w + ": w_bce, w_tversky and pos_weight must be >= 0");
    if (w_bce == 0.f && w_tversky == 0.f) return fail(CSU_E_ARG, w + ": w_bce and w_tversky are both zero");
    return 0;
}

}  // namespace
}  // namespace csu

using namespace csu;

extern "C" size_t csu_seg_loss_workspace(long n, int rows) {
    if (n < 1 || rows < 1 || n % rows) return 0;
    return (size_t)seg_plan(n, rows).items * NSUM * sizeof(float);
}

extern "C" int csu_seg_loss_fwd(long n, int rows, const float* p, const float* t, float w_bce, float pos_weight,
                                float w_tversky, float alpha, float beta, float smooth, float* loss, float* stats,
                                float* coef, void* workspace, size_t ws_bytes, void* stream) {
    if (int e = seg_args("seg_loss_fwd", n, rows, w_bce, pos_weight, w_tversky)) return e;
    if (!(alpha >= 0.f) || !(beta >= 0.f)) return fail(CSU_E_ARG, "seg_loss_fwd: alpha and beta must be >= 0");
    if (!(smooth > 0.f)) return fail(CSU_E_ARG, "seg_loss_fwd: smooth must be > 0");
    if (!p || !t || !loss || !coef) return fail(CSU_E_ARG, "seg_loss_fwd: null p, t, loss or coef");
    if (!workspace || ws_bytes < csu_seg_loss_workspace(n, rows)) return fail(CSU_E_WORKSPACE, "seg_loss_fwd: workspace");
    const SegPlan s = seg_plan(n, rows);
    const int nb = (int)(s.items < SEG_BLOCKS ? s.items : SEG_BLOCKS);
    hipStream_t st = as_stream(stream);
    seg_partial<<<nb, NT, 0, st>>>(s.L, s.clen, s.cpr, s.items, p, t, w_bce != 0.f, pos_weight, (float*)workspace);
    if (int e = check_launch("seg_loss_fwd")) return e;
    seg_finish<<<1, NT, 0, st>>>(rows, s.cpr, n, (const float*)workspace, w_bce, w_tversky, alpha, beta, smooth, loss, stats,
                                 coef);
    return check_launch("seg_loss_fwd");
}

extern "C" int csu_seg_loss_bwd(long n, int rows, const float* p, const float* t, const float* dloss, const float* coef,
                                float w_bce, float pos_weight, float w_tversky, float* dp, void* stream) {
    if (int e = seg_args("seg_loss_bwd", n, rows, w_bce, pos_weight, w_tversky)) return e;
    if (!p || !t || !dloss || !coef || !dp) return fail(CSU_E_ARG, "seg_loss_bwd: null p, t, dloss, coef or dp");
    const SegPlan s = seg_plan(n, rows);
    const int nb = (int)(s.items < SEG_BLOCKS ? s.items : SEG_BLOCKS);
    seg_backward<<<nb, NT, 0, as_stream(stream)>>>(s.L, s.clen, s.cpr, s.items, p, t, dloss, coef, w_bce, pos_weight,
                                                   w_tversky / (float)rows, 1.f / (float)n, dp);
    return check_launch("seg_loss_bwd");
}
