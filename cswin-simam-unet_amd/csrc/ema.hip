// Exponential moving average (EMA) of the weights for gfx950, over the optimizer's csu_adamw_item
// table (adamw.hip) and a parallel array of EMA pointers, one fp32 tensor per item.
//   ema_update_kernel: ema <- ema + w (param - ema), w = 1 - d, the stand-alone form of the update the
//     EMA instantiations of adamw_kernel do in registers (same ema_weight / ema4, adamw_items.hpp: bit
//     for bit the same result).  Streaming: 12 B per parameter (read p, e; write e).
//   ema_swap_kernel: param <-> ema for every element, and every bf16 shadow layout of the item
//     re-made from the value now in param (walk_chunk, the step's own shadow tail), so the
//     forward's weight copies are current and every captured pointer stays valid.  16 B per
//     parameter + 2 B per shadow layout.  Swapping twice is the identity, bit for bit.
// Both walk the table with the step's chunk numbering, one workgroup per chunk, 16-B vector loads /
// stores, no atomics: results are bitwise repeatable.
#include "adamw_items.hpp"

namespace csu {
namespace {

using namespace adamw_items;

__global__ __launch_bounds__(NT) void ema_update_kernel(const csu_adamw_item* __restrict__ items,
                                                        float* const* __restrict__ ema, int count, const float* n_dev,
                                                        float decay, int warmup) {
    const long b = blockIdx.x;
    const int idx = find_item(items, count, b);
    const csu_adamw_item it = items[idx];
    float* e = ema[idx];
    if (!e) return;   // no EMA for this item
    const float w = ema_weight(n_dev, decay, warmup);
    const float* p = it.param;
    walk_chunk<false>(it, b, nullptr, [&](long i, int n, bool vec, float* pv) {
        float ev[4];
        ld4n(p, i, n, vec, pv);
        ld4n(e, i, n, vec, ev);
        ema4(w, pv, ev);
        st4n(e, i, n, vec, ev);
    });
}

__global__ __launch_bounds__(NT) void ema_swap_kernel(const csu_adamw_item* __restrict__ items,
                                                      float* const* __restrict__ ema, int count) {
    __shared__ ShadowTile tile;
    const long b = blockIdx.x;
    const int idx = find_item(items, count, b);
    const csu_adamw_item it = items[idx];
    float* e = ema[idx];
    if (!e) return;   // the whole workgroup: before the walk's barrier
    float* p = it.param;
    walk_chunk<true>(it, b, &tile, [&](long i, int n, bool vec, float* pv) {
        float ov[4];
        ld4n(p, i, n, vec, ov);
        ld4n(e, i, n, vec, pv);
        st4n(p, i, n, vec, pv);   // pv: the value now in param, the one the shadows are made from
        st4n(e, i, n, vec, ov);
    });
}

}  // namespace
}  // namespace csu

using namespace csu;

extern "C" int csu_ema_update(const csu_adamw_item* items, float* const* ema, int count, long total_chunks,
                              const float* ema_updates_dev, float decay, int warmup, void* stream) {
    if (!items || !ema || count < 1 || total_chunks < 1) return fail(CSU_E_ARG, "ema_update: empty item table");
    if (warmup && !ema_updates_dev) return fail(CSU_E_ARG, "ema_update: warmup needs the device update count");
    if (!(decay >= 0.f && decay <= 1.f)) return fail(CSU_E_ARG, "ema_update: decay outside [0, 1]");
    ema_update_kernel<<<(unsigned)total_chunks, NT, 0, as_stream(stream)>>>(items, ema, count, ema_updates_dev, decay,
                                                                            warmup);
    return check_launch("ema_update");
}

extern "C" int csu_ema_swap(const csu_adamw_item* items, float* const* ema, int count, long total_chunks, void* stream) {
    if (!items || !ema || count < 1 || total_chunks < 1) return fail(CSU_E_ARG, "ema_swap: empty item table");
    ema_swap_kernel<<<(unsigned)total_chunks, NT, 0, as_stream(stream)>>>(items, ema, count);
    return check_launch("ema_swap");
}
