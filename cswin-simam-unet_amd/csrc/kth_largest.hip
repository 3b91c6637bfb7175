// The k-th largest of cap fp32 keys on the device, k = a fraction rho of the live keys: the threshold of the top-k
// cross-entropy (csu_seg_hard_*, csrc/seg_ce.hip).  The reference has no counterpart.
//   A key with the sign bit set is skipped.  The bit patterns of the others (+0, denormals, normals, +inf, and NaNs
//   above them) are ordered as unsigned integers exactly as the values are, so the selection is a 4 x 8-bit radix
//   select from the top byte down (surface.hip's for HD95, for one rank and with the rank formed here):
//   pass p  kth_hist<p>: a histogram of byte 3 - p of the keys whose higher bytes equal the prefix chosen so far;
//           LDS counters per workgroup, then one 64-bit integer atomic per non-empty bin.  Integer sums: exact in
//           any order, so the result is a function of the multiset of keys alone.
//   pick    at the start of the next pass every workgroup forms the new prefix again from the finished histogram:
//           the bin b with (keys above b) < rank <= (keys above b) + hist[b]; rank -= keys above b, n_gt += them.
//           After pass 0 the histogram's total is n, the live keys, and rank = k = max(1, floor(double(rho) n))
//           (at most n; 0 when n = 0).  Workgroup 0 stores the state for the pass after.
//   finish  kth_finish: the last pick; out = fp64 {tau, n_gt, n_eq, k, n}.  n = 0: all zero.
// Every loop runs to cap, the grid or the 256 bins, never to a value read from memory.  No floating-point
// arithmetic touches a key, so NaN keys are patterns like any other.
#include "common.hpp"

namespace csu {
namespace {

constexpr int NT = 256;
constexpr int BINS = 256;
constexpr int PASSES = 4;
constexpr int KTH_BLOCKS = 1024;
typedef unsigned long long u64;

struct KthState {
    u64 rank;   // 1-based from the top among the keys that match the prefix; 0: nothing to select
    u64 ngt;    // keys known to be above every key that matches the prefix
    unsigned prefix, pad;
};
struct KthWs {
    u64 hist[PASSES][BINS];
    KthState state[PASSES];   // state[p]: after the pick that follows pass p
    u64 n, k;
};

__device__ __forceinline__ u64 kth_rank(float rho, u64 n) {
    if (n == 0) return 0;
    const double v = floor((double)rho * (double)n);
    return v >= (double)n ? n : v >= 1.0 ? (u64)v : 1;   // a NaN rho: 1
}

struct KthShared {
    u64 h[BINS];
    u64 tot;
    KthState cur;
};

// the state after pass p, left in sh.cur (and sh.tot = the keys pass p counted); all NT = BINS threads call it
__device__ __forceinline__ void kth_pick(int p, const KthWs* __restrict__ ws, const float* __restrict__ rho, KthShared& sh) {
    const int tid = threadIdx.x;
    sh.h[tid] = ws->hist[p][tid];
    __syncthreads();
    u64 above = 0;
    for (int j = tid + 1; j < BINS; ++j) above += sh.h[j];
    if (tid == 0) sh.tot = above + sh.h[0];
    __syncthreads();
    KthState prev;
    if (p == 0) {
        prev.rank = kth_rank(rho[0], sh.tot);
        prev.ngt = 0;
        prev.prefix = 0;
    } else {
        prev = ws->state[p - 1];
    }
    const bool mine = prev.rank > above && prev.rank <= above + sh.h[tid];   // true in at most one thread
    const bool none = prev.rank == 0 || prev.rank > sh.tot;                  // no live key (or histograms that disagree)
    if (mine) sh.cur = KthState{prev.rank - above, prev.ngt + above, (prev.prefix << 8) | (unsigned)tid, 0u};
    if (none && tid == 0) sh.cur = KthState{0, prev.ngt, prev.prefix << 8, 0u};
    __syncthreads();
}

// The workspace is cleared by a kernel, not a memset: as a memset node of a captured graph with parallel branches
// (a whole training step) the clearing did not precede the first pass.
__global__ __launch_bounds__(NT) void kth_clear(u64* __restrict__ ws, int n) {
    const int i = blockIdx.x * NT + threadIdx.x;
    if (i < n) ws[i] = 0;
}

template <int P>
__global__ __launch_bounds__(NT) void kth_hist(const unsigned* __restrict__ keys, long cap, const float* __restrict__ rho,
                                               KthWs* __restrict__ ws) {
    __shared__ unsigned lh[BINS];
    __shared__ KthShared sh;
    const int tid = threadIdx.x;
    unsigned prefix = 0;
    if constexpr (P > 0) {
        kth_pick(P - 1, ws, rho, sh);
        prefix = sh.cur.prefix;
        if (blockIdx.x == 0 && tid == 0) {
            ws->state[P - 1] = sh.cur;
            if (P == 1) {
                ws->n = sh.tot;
                ws->k = sh.cur.rank + sh.cur.ngt;
            }
        }
    }
    lh[tid] = 0;
    __syncthreads();
    constexpr int shift = 24 - 8 * P;
    // Plain LDS atomics, also in pass 0 where loss values share a handful of top bytes: one add per distinct bin of
    // a wave (ballots) measured 10 % slower for the whole selection than the contended counter it avoids.
    auto count = [&](unsigned key) {
        if ((int)key < 0) return;
        if (P == 0 || (key >> ((shift + 8) & 31)) == prefix) atomicAdd(&lh[(key >> shift) & (BINS - 1)], 1u);
    };
    // 16-B loads where the buffer allows them; the last cap % 4 keys by workgroup 0
    const bool vec = ((uintptr_t)keys & 15) == 0;
    const long nv = vec ? cap / 4 : 0;
    const uint4* kv = reinterpret_cast<const uint4*>(keys);
    for (long i = (long)blockIdx.x * NT + tid; i < nv; i += (long)gridDim.x * NT) {
        const uint4 q = kv[i];
        count(q.x);
        count(q.y);
        count(q.z);
        count(q.w);
    }
    for (long i = nv * 4 + (long)blockIdx.x * NT + tid; i < cap; i += (long)gridDim.x * NT) count(keys[i]);
    __syncthreads();
    if (lh[tid]) atomicAdd(&ws->hist[P][tid], (u64)lh[tid]);
}

__global__ __launch_bounds__(NT) void kth_finish(const float* __restrict__ rho, const KthWs* __restrict__ ws,
                                                 double* __restrict__ out) {
    __shared__ KthShared sh;
    kth_pick(PASSES - 1, ws, rho, sh);
    if (threadIdx.x == 0) {
        const bool any = sh.cur.rank > 0;
        out[0] = any ? (double)__uint_as_float(sh.cur.prefix) : 0.0;
        out[1] = (double)sh.cur.ngt;
        out[2] = any ? (double)sh.h[sh.cur.prefix & (BINS - 1)] : 0.0;
        out[3] = (double)ws->k;
        out[4] = (double)ws->n;
    }
}

}  // namespace
}  // namespace csu

using namespace csu;

extern "C" size_t csu_kth_largest_workspace(long cap) {
    if (cap < 1) return 0;
    return sizeof(KthWs);
}

extern "C" int csu_kth_largest(long cap, const float* keys, const float* rho, double* out, void* workspace, size_t ws_bytes,
                               void* stream) {
    if (cap < 1 || cap > (1L << 40)) return fail(CSU_E_ARG, "kth_largest: 1 <= cap <= 2^40 keys");
    if (!keys || !rho || !out) return fail(CSU_E_ARG, "kth_largest: null keys, rho or out");
    if (((uintptr_t)keys & 3) || ((uintptr_t)out & 7)) return fail(CSU_E_ARG, "kth_largest: keys or out misaligned");
    if (!workspace || ((uintptr_t)workspace & 7) || ws_bytes < csu_kth_largest_workspace(cap))
        return fail(CSU_E_WORKSPACE, "kth_largest: workspace (8-byte aligned)");
    hipStream_t st = as_stream(stream);
    KthWs* ws = (KthWs*)workspace;
    constexpr int nw = (int)(sizeof(KthWs) / sizeof(u64));
    static_assert(sizeof(KthWs) % sizeof(u64) == 0, "KthWs is cleared in 8-byte words");
    kth_clear<<<(nw + NT - 1) / NT, NT, 0, st>>>((u64*)ws, nw);
    const long want = (cap + 4L * NT - 1) / (4L * NT);
    const int nb = (int)(want < KTH_BLOCKS ? want : KTH_BLOCKS);
    const unsigned* kb = (const unsigned*)keys;
    kth_hist<0><<<nb, NT, 0, st>>>(kb, cap, rho, ws);
    kth_hist<1><<<nb, NT, 0, st>>>(kb, cap, rho, ws);
    kth_hist<2><<<nb, NT, 0, st>>>(kb, cap, rho, ws);
    kth_hist<3><<<nb, NT, 0, st>>>(kb, cap, rho, ws);
    kth_finish<<<1, NT, 0, st>>>(rho, ws, out);
    return check_launch("kth_largest");
}
