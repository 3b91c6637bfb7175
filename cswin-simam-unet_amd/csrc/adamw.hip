// Fused multi-tensor AdamW for gfx950 (fp32 params / grads / moments).
//
// The optimizer of the reference training step (torch.optim.AdamW(lr 1e-4, betas (0.9, 0.999),
// eps 1e-8, weight_decay 1e-4), cswin:937-941) over all 463 parameter tensors in ONE launch:
// a device table of (param, grad, exp_avg, exp_avg_sq, numel, first chunk) items, one workgroup per
// 4096-element chunk (items found by binary search), 16-B vector loads/stores; the update is
// torch's AdamW arithmetic operation for operation (decoupled decay, lerp first moment,
// sqrt(v)/sqrt(bc2) + eps denominator).  lr and step may live on the device (HIP-graph capture:
// the scheduler updates the lr tensor between replays, a graph node increments the step).
// Streaming kernel: 28 B per parameter (read p, g, m, v; write p, m, v), HBM-bound; + 2 B per bf16
// shadow layout written (the forward's weight copies, csu.h), which replaces a separate cast pass
// re-reading every fp32 weight (4 B + the same 2 B per layout).
//
// Gradient clipping (csu_adamw_step_ex): the CLIP instantiations multiply every gradient element by
// the device coefficient ctl[1] that csu_grad_norm_finish wrote (grad_norm.hip) while the element is
// in registers -- no extra traffic -- and may skip the whole step when ctl[2] says the gradient
// norm was not finite.
//
// Weight EMA (csu_adamw_step_ema): the EMA instantiations also update an exponential moving average
// of every parameter from the updated value in registers -- + 8 B per parameter (read and write the
// EMA value), no extra launch, against 12 B for a separate pass (ema.hip, the stand-alone form the
// fused one matches bit for bit).
#include "adamw_items.hpp"

namespace csu {
namespace {

using namespace adamw_items;

struct AdamConst {
    float beta1, beta2, eps, wd, step_size, bc2s, decay;
    float coef;   // CLIP: the clip coefficient every gradient element is multiplied by first
};

// g * c rounded on its own: never contracted into the fmaf / subtraction that consumes it, so a
// clipped step is bitwise "scale the gradient, then run the plain step" (__fmul_rn is a plain
// product in HIP, which the compiler may fuse)
__device__ __forceinline__ float mul_rn(float a, float b) {
#pragma clang fp contract(off)
    return a * b;
}

template <bool L2, bool CLIP>
__device__ __forceinline__ void adam4(const AdamConst& k, float* pv, const float* gv0, float* mv, float* vv) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        float g = gv0[j];
        if constexpr (CLIP) g = mul_rn(g, k.coef);
        if constexpr (L2) g = fmaf(k.wd, pv[j], g);
        else pv[j] *= k.decay;
        mv[j] = fmaf(1.f - k.beta1, g - mv[j], mv[j]);   // lerp(m, g, 1 - beta1)
        vv[j] = fmaf(1.f - k.beta2, g * g, vv[j] * k.beta2);
        const float denom = sqrtf(vv[j]) / k.bc2s + k.eps;
        pv[j] = fmaf(-k.step_size, mv[j] / denom, pv[j]);
    }
}

// ev: EMA only, the four EMA values (loaded beside the others, stored with the same 16-B stores); e == null:
// no EMA for this item
template <bool L2, bool CLIP, bool EMA>
__device__ __forceinline__ void update(const AdamConst& k, float* p, const float* g, float* m, float* v, float* e, float ew,
                                       long i, int n, bool vec, float* pv) {
    float gv[4], mv[4], vv[4], ev[4];
    ld4n(p, i, n, vec, pv);
    ld4n(g, i, n, vec, gv);
    ld4n(m, i, n, vec, mv);
    ld4n(v, i, n, vec, vv);
    if constexpr (EMA) {
        if (e) ld4n(e, i, n, vec, ev);
    }
    adam4<L2, CLIP>(k, pv, gv, mv, vv);
    st4n(p, i, n, vec, pv);
    st4n(m, i, n, vec, mv);
    st4n(v, i, n, vec, vv);
    if constexpr (EMA) {
        if (e) {   // while pv holds the updated parameter: + one read and one write of the EMA value
            ema4(ew, pv, ev);
            st4n(e, i, n, vec, ev);
        }
    }
}

// L2 = false: AdamW (decoupled decay, cswin:937-941); L2 = true: Adam with L2 weight decay, the
// plain UNet's optim.Adam(weight_decay) (unet:486-490): g += wd * param before the moments.
// Shadow modes (csu.h): tile items update a 64 x 64 tile and write W and, through LDS, W^T in
// bf16; flat items write the bf16 copy at the same index, conv items scatter the OHWI / IHWO
// layouts (the csu_cast_bf16_batch layouts, now made from the updated fp32 value in registers;
// walk_chunk, adamw_items.hpp).
// CLIP (csu_adamw_step_ex): ctl = the device scalars of csu_grad_norm_finish; g <- g * ctl[1] before
// anything else (the L2 term included), and with skip != 0 and ctl[2] == 0 (non-finite gradient
// norm) every workgroup returns before it loads or stores anything else.  ctl and skip are unused
// without CLIP.
// EMA (csu_adamw_step_ema): ema[item] <- ema + w (param - ema) from the updated parameter, w = 1 - d
// once per workgroup (ema_weight); a skipped step leaves the EMA alone.  The ema_* arguments are
// unused without EMA.
template <bool L2, bool CLIP = false, bool EMA = false>
__global__ __launch_bounds__(NT) void adamw_kernel(const csu_adamw_item* __restrict__ items, int count, const float* lr_dev,
                                                   float lr_host, float beta1, float beta2, float eps, float wd,
                                                   const float* step_dev, float step_host, const float* ctl, int skip,
                                                   float* const* __restrict__ ema, const float* ema_n_dev, float ema_decay,
                                                   int ema_warmup) {
    __shared__ ShadowTile tile;
    if constexpr (CLIP) {
        if (skip && ctl[2] == 0.f) return;
    }
    const long b = blockIdx.x;
    const int idx = find_item(items, count, b);
    const csu_adamw_item it = items[idx];
    const float lr = lr_dev ? *lr_dev : lr_host;
    const float step = step_dev ? *step_dev : step_host;
    float coef = 1.f;
    if constexpr (CLIP) coef = ctl[1];   // read beside lr / step: its latency hides behind theirs
    float* e = nullptr;
    float ew = 0.f;
    if constexpr (EMA) {
        e = ema[idx];
        ew = ema_weight(ema_n_dev, ema_decay, ema_warmup);
    }
    const float bc1 = 1.f - powf(beta1, step), bc2 = 1.f - powf(beta2, step);
    const AdamConst k{beta1, beta2, eps, wd, lr / bc1, sqrtf(bc2), L2 ? 1.f : 1.f - lr * wd, coef};
    float* p = it.param;
    const float* g = it.grad;
    float* m = it.exp_avg;
    float* v = it.exp_avg_sq;
    walk_chunk<true>(it, b, &tile, [&](long i, int n, bool vec, float* pv) {
        update<L2, CLIP, EMA>(k, p, g, m, v, e, ew, i, n, vec, pv);
    });
}

template <bool L2, bool CLIP, bool EMA>
void launch_adamw(const csu_adamw_item* items, int count, long total_chunks, const float* lr_dev, float lr, float beta1,
                  float beta2, float eps, float wd, const float* step_dev, float step, const float* ctl, int skip,
                  float* const* ema, const float* ema_n_dev, float ema_decay, int ema_warmup, hipStream_t st) {
    adamw_kernel<L2, CLIP, EMA><<<(unsigned)total_chunks, NT, 0, st>>>(items, count, lr_dev, lr, beta1, beta2, eps, wd,
                                                                       step_dev, step, ctl, skip, ema, ema_n_dev, ema_decay,
                                                                       ema_warmup);
}

}  // namespace
}  // namespace csu

using namespace csu;

extern "C" long csu_adamw_chunk_elems(void) { return CH; }

extern "C" int csu_adamw_step(const csu_adamw_item* items, int count, long total_chunks, const float* lr_dev, float lr,
                              float beta1, float beta2, float eps, float weight_decay, const float* step_dev, float step,
                              void* stream) {
    if (!items || count < 1 || total_chunks < 1) return fail(CSU_E_ARG, "adamw: empty item table");
    launch_adamw<false, false, false>(items, count, total_chunks, lr_dev, lr, beta1, beta2, eps, weight_decay, step_dev,
                                      step, nullptr, 0, nullptr, nullptr, 0.f, 0, as_stream(stream));
    return check_launch("adamw");
}

extern "C" int csu_adam_l2_step(const csu_adamw_item* items, int count, long total_chunks, const float* lr_dev, float lr,
                                float beta1, float beta2, float eps, float weight_decay, const float* step_dev, float step,
                                void* stream) {
    if (!items || count < 1 || total_chunks < 1) return fail(CSU_E_ARG, "adam_l2: empty item table");
    launch_adamw<true, false, false>(items, count, total_chunks, lr_dev, lr, beta1, beta2, eps, weight_decay, step_dev,
                                     step, nullptr, 0, nullptr, nullptr, 0.f, 0, as_stream(stream));
    return check_launch("adam_l2");
}

extern "C" int csu_adamw_step_ex(const csu_adamw_item* items, int count, long total_chunks, const float* lr_dev, float lr,
                                 float beta1, float beta2, float eps, float weight_decay, const float* step_dev, float step,
                                 const float* ctl, int skip_nonfinite, int l2, void* stream) {
    if (!items || count < 1 || total_chunks < 1) return fail(CSU_E_ARG, "adamw_step_ex: empty item table");
    if (!ctl) return fail(CSU_E_ARG, "adamw_step_ex: null ctl (csu_grad_norm_finish writes it)");
    hipStream_t st = as_stream(stream);
    if (l2)
        launch_adamw<true, true, false>(items, count, total_chunks, lr_dev, lr, beta1, beta2, eps, weight_decay, step_dev,
                                        step, ctl, skip_nonfinite, nullptr, nullptr, 0.f, 0, st);
    else
        launch_adamw<false, true, false>(items, count, total_chunks, lr_dev, lr, beta1, beta2, eps, weight_decay, step_dev,
                                         step, ctl, skip_nonfinite, nullptr, nullptr, 0.f, 0, st);
    return check_launch("adamw_step_ex");
}

extern "C" int csu_adamw_step_ema(const csu_adamw_item* items, int count, long total_chunks, const float* lr_dev, float lr,
                                  float beta1, float beta2, float eps, float weight_decay, const float* step_dev, float step,
                                  const float* ctl, int skip_nonfinite, int l2, float* const* ema,
                                  const float* ema_updates_dev, float ema_decay, int ema_warmup, void* stream) {
    if (!items || count < 1 || total_chunks < 1) return fail(CSU_E_ARG, "adamw_step_ema: empty item table");
    if (!ema) return fail(CSU_E_ARG, "adamw_step_ema: null EMA pointer array");
    if (ema_warmup && !ema_updates_dev) return fail(CSU_E_ARG, "adamw_step_ema: warmup needs the device update count");
    if (!(ema_decay >= 0.f && ema_decay <= 1.f)) return fail(CSU_E_ARG, "adamw_step_ema: decay outside [0, 1]");
    hipStream_t st = as_stream(stream);
    auto go = [&](auto fn) {
        fn(items, count, total_chunks, lr_dev, lr, beta1, beta2, eps, weight_decay, step_dev, step, ctl, skip_nonfinite,
           ema, ema_updates_dev, ema_decay, ema_warmup, st);
    };
    if (ctl) {   // null ctl: no clipping
        if (l2) go(launch_adamw<true, true, true>);
        else go(launch_adamw<false, true, true>);
    } else {
        if (l2) go(launch_adamw<true, false, true>);
        else go(launch_adamw<false, false, true>);
    }
    return check_launch("adamw_step_ema");
}
