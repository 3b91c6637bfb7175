// Connected-component labelling of label maps and the component rules of segmentation post-processing
// (fill holes, remove small, keep largest) for gfx950.  The reference has no counterpart: nothing here is a port.
//   component  maximal set of pixels of one value joined by adjacency: `connectivity` 4 or 8 for the non-zero
//              values, always 4 for value 0, so the background components come out of the same pass.
//   root       the component's smallest per-image pixel index y W + x = its first pixel in raster order.  Roots
//              are unique by definition, so every result below is bitwise repeatable and independent of B.
//   parent     P (B, H, W) int32: a union-find forest over pixel indices with P[i] <= i at every moment
//              (parents only ever decrease), P[r] == r exactly at the roots once flatten has run.
//   acc        A (B, H, W) int32, meaningful at roots: bits 0..29 the pixel count (H W < 2^30), bit 30 "value
//              is non-zero", bit 31 "touches the image border".
// Launches (plain ones, no workgroup ever waits for another):
//   tile     one workgroup per 64 x 64 tile: a wave owns a row, __ballot gives the row runs, the runs are merged
//            with the row above by union-find in LDS; writes P = index of the tile-local root, A = the
//            tile-local count and bits at the local roots and 0 elsewhere (every element of both is written).
//   seam     one thread per pixel of a tile's first row / first column: unions across the tile borders in
//            global memory (agent-scope atomics only), the diagonals and the four-tile corners included.
//   flatten  P[i] <- root; the local roots add their count and bits to the root's A (at most one integer
//            atomic per tile-local component); counts the non-zero roots of each 4096-pixel chunk.
//   scan     one workgroup per image: exclusive scan of the chunk counts, and `count`.
//   number   the rank of every non-zero root in raster order -> N at the roots.
//   relabel  comp = N[P], area = A[P] & mask.
//   filter   fill (holes take the value left of their root), best (64-bit atomicMax of (area, ~root) per
//            image and class), apply (size and largest rules per pixel).
#include <algorithm>

#include "common.hpp"

namespace csu {
namespace {

constexpr int T = 64;                 // tile edge: a wave is a tile row
constexpr int NT = 256;
constexpr int TNT = 256;              // threads of a tile workgroup (512 and 1024 measured within 5 % of it)
constexpr int ROWS = T / (TNT / 64);  // tile rows per wave
constexpr int CHUNK = 4096;           // pixels per workgroup of the linear passes (16 x 64 per wave)
constexpr int WCH = CHUNK / (NT / 64);
constexpr int DMAX = 32767;
constexpr int KMAX = 32;
constexpr unsigned AREA = 0x3FFFFFFFu, FG = 0x40000000u, BORDER = 0x80000000u;
constexpr long GRID_MAX = 1L << 23;   // workgroups per launch: 2^23 x 256 threads < 2^32

inline size_t up256(size_t n) { return (n + 255) & ~(size_t)255; }

#define CC_RLX __ATOMIC_RELAXED
#define CC_AGENT __HIP_MEMORY_SCOPE_AGENT
#define CC_WG __HIP_MEMORY_SCOPE_WORKGROUP

// ---- union-find ------------------------------------------------------------------------------
// find: follows P[i] < i until P[i] == i.  Every step strictly decreases i and i >= 0, so the walk ends
// after at most i steps whatever other workgroups do meanwhile (they only lower parents, which keeps
// P[j] <= j).  SCOPE: agent for the forest in global memory, workgroup for the one in LDS.
template <int SCOPE> __device__ __forceinline__ int uf_find(int* p, int i) {
    for (;;) {
        const int j = __hip_atomic_load(p + i, CC_RLX, SCOPE);
        if (j == i) return i;
        i = j;
    }
}
// union: hangs the larger root under the smaller with atomicMin.  A lost race returns old < hi (somebody
// gave hi a smaller parent first); the pair to join is then (old, lo), and max(old, lo) < hi: the larger
// index of the pair strictly decreases with every retry and is bounded below by 0, so the loop ends.
template <int SCOPE> __device__ __forceinline__ void uf_union(int* p, int a, int b) {
    for (;;) {
        a = uf_find<SCOPE>(p, a);
        b = uf_find<SCOPE>(p, b);
        if (a == b) return;
        const int hi = max(a, b), lo = min(a, b);
        const int old = __hip_atomic_fetch_min(p + hi, lo, CC_RLX, SCOPE);
        if (old == hi) return;
        a = old;
        b = lo;
    }
}

// ---- tile ------------------------------------------------------------------------------------
// grid (ceil(W / T), ceil(H / T), B), TNT threads; wave w owns tile rows w, w + 4, ...
template <typename V>
__global__ __launch_bounds__(TNT) void tile_kernel(int H, int W, int conn8, const V* __restrict__ labels, int* __restrict__ P,
                                                  unsigned* __restrict__ A) {
    __shared__ int lpar[T * T];
    __shared__ unsigned lacc[T * T];
    const int lx = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int x = blockIdx.x * T + lx, ty0 = blockIdx.y * T;
    const long base = (long)blockIdx.z * H * W;
    const V* img = labels + base;
    const bool xin = x < W;
    unsigned long long need = 0;   // 4 bits a row: unions with up / up-left / up-right still to make
#pragma unroll
    for (int k = 0; k < ROWS; ++k) {
        const int ly = w + k * (TNT / 64), y = ty0 + ly;
        const bool in = xin && y < H, upin = in && ly > 0;
        // out-of-image lanes hold 0 and are masked by `in` wherever they could pair with a pixel
        const V v = in ? img[(long)y * W + x] : (V)0;
        const V vu = upin ? img[(long)(y - 1) * W + x] : (V)0;
        const V vl = __shfl_up(v, 1, 64), vul = __shfl_up(vu, 1, 64), vur = __shfl_down(vu, 1, 64);
        const bool L = in && lx > 0 && vl == v;
        const bool U = upin && vu == v;
        const bool Lu = upin && lx > 0 && vul == vu;
        const bool diag = conn8 && upin && v != (V)0;
        const bool UL = diag && lx > 0 && vul == v;
        const bool UR = diag && lx < T - 1 && x + 1 < W && vur == v;
        // U with L and Lu: the left neighbour makes the same union (its U holds); a diagonal beside U: the two
        // upper pixels share a run
        const unsigned f = (U && !(L && Lu) ? 1u : 0u) | (UL && !U ? 2u : 0u) | (UR && !U ? 4u : 0u);
        need |= (unsigned long long)f << (4 * k);
        const unsigned long long heads = ~__ballot(L);                 // bit 0 is always a head
        const int start = 63 - __clzll(heads & (~0ull >> (63 - lx)));  // the run's first lane
        const int idx = ly * T + lx;
        lpar[idx] = ly * T + start;
        unsigned a = 0;
        if (in && !L) {
            const unsigned long long above = lx < 63 ? heads >> (lx + 1) : 0ull;
            const int len = above ? __ffsll((long long)above) : 64 - lx;   // out-of-image lanes are heads: runs stop at W
            a = (unsigned)len | (v != (V)0 ? FG : 0u);
            if (y == 0 || y == H - 1 || x == 0 || x + len == W) a |= BORDER;
        }
        lacc[idx] = a;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < ROWS; ++k) {
        const unsigned f = (unsigned)(need >> (4 * k)) & 7u;
        const int idx = (w + k * (TNT / 64)) * T + lx;
        if (f & 1u) uf_union<CC_WG>(lpar, idx, idx - T);
        if (f & 2u) uf_union<CC_WG>(lpar, idx, idx - T - 1);
        if (f & 4u) uf_union<CC_WG>(lpar, idx, idx - T + 1);
    }
    __syncthreads();
    // the forest is final: lpar is only read from here on.  Run heads that are not the local root hand their
    // count to the root; the root's own word is only added to, a non-root's only read
    int root[ROWS];
#pragma unroll
    for (int k = 0; k < ROWS; ++k) {
        const int idx = (w + k * (TNT / 64)) * T + lx;
        const int r = uf_find<CC_WG>(lpar, idx);
        root[k] = r;
        const unsigned a = lacc[idx];
        if (r != idx && a) {
            atomicAdd(&lacc[r], a & AREA);
            if (a & BORDER) atomicOr(&lacc[r], BORDER);
        }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < ROWS; ++k) {
        const int ly = w + k * (TNT / 64), y = ty0 + ly;
        if (!xin || y >= H) continue;
        const int idx = ly * T + lx, r = root[k];
        const long g = base + (long)y * W + x;
        P[g] = (ty0 + (r >> 6)) * W + blockIdx.x * T + (r & 63);
        A[g] = r == idx ? lacc[idx] : 0u;
    }
}

// ---- seam ------------------------------------------------------------------------------------
// grid (ceil(n / NT), B), n = nsr W + nsc H: the pixels of the nsr first rows and nsc first columns of tiles.
// Other workgroups, on other XCDs, change P during this launch: agent-scope atomics only.
template <typename V>
__global__ __launch_bounds__(NT) void seam_kernel(int H, int W, int conn8, int nsr, const V* __restrict__ labels, int* P) {
    const long base = (long)blockIdx.y * H * W;
    const V* img = labels + base;
    int* p = P + base;
    int t = blockIdx.x * NT + threadIdx.x;
    // An edge is left out where others imply it, so that a seam through a uniform region costs one union per tile
    // and not 64 on one address.  What an omitted edge leans on: edges inside a tile (made by tile_kernel), the
    // same kind of edge one pixel earlier on the same seam (never omitted at a tile's first pixel), and, for the
    // diagonals, the straight seam edges -- no circle.
    if (t < nsr * W) {   // a tile's first row: up, and the two diagonals (they cross the corners too)
        const int y = (t / W + 1) * T, x = t % W;
        const int i = y * W + x;
        const V v = img[i];
        const bool U = img[i - W] == v;
        // (y, x - 1) -- (y - 1, x - 1) is the same union when both row neighbours lie in the same tiles and match
        if (U && !(x % T != 0 && img[i - 1] == v && img[i - W - 1] == v)) uf_union<CC_AGENT>(p, i, i - W);
        if (conn8 && v != (V)0 && !U) {   // with U the upper diagonal pixel joins (y - 1, x) along its row
            if (x > 0 && img[i - W - 1] == v) uf_union<CC_AGENT>(p, i, i - W - 1);
            if (x + 1 < W && img[i - W + 1] == v) uf_union<CC_AGENT>(p, i, i - W + 1);
        }
        return;
    }
    t -= nsr * W;
    const int nsc = (W - 1) / T;
    if (t >= nsc * H) return;
    // a tile's first column: left, up-left, and the anti-diagonal (y, x - 1) -- (y - 1, x)
    const int x = (t / H + 1) * T, y = t % H;
    const int i = y * W + x;
    const V v = img[i], l = img[i - 1];
    const bool Lf = l == v;
    if (Lf && !(y % T != 0 && img[i - W] == v && img[i - W - 1] == v)) uf_union<CC_AGENT>(p, i, i - 1);
    if (conn8 && y > 0 && !Lf) {   // with Lf both diagonals close a triangle of straight edges
        if (v != (V)0 && img[i - W - 1] == v) uf_union<CC_AGENT>(p, i, i - W - 1);
        if (l != (V)0 && img[i - W] == l) uf_union<CC_AGENT>(p, i - 1, i - W);
    }
}

// ---- flatten, scan, number, relabel ----------------------------------------------------------------
// The linear passes: grid (ceil(H W / CHUNK), B), NT threads; wave w owns pixels [w WCH, (w + 1) WCH) of the
// chunk, 64 consecutive ones at a time, so a __ballot is 64 raster-ordered flags.
__global__ __launch_bounds__(NT) void flatten_kernel(int HW, int nchunk, int* P, unsigned* A, int* __restrict__ bsum) {
    __shared__ int wsum[NT / 64];
    const long base = (long)blockIdx.y * HW;
    int* p = P + base;
    unsigned* acc = A + base;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int i0 = blockIdx.x * CHUNK + w * WCH;
    int n = 0;
    for (int k = 0; k < WCH / 64; ++k) {
        const int i = i0 + k * 64 + lane;   // < 2^30 + CHUNK
        bool rootfg = false;
        if (i < HW) {
            // P[j] of other pixels is rewritten by their owners during this launch, always to an ancestor of j:
            // whichever value the walk sees, it still ends at the root
            const int j = __hip_atomic_load(p + i, CC_RLX, CC_AGENT);
            const int r = j == i ? i : uf_find<CC_AGENT>(p, j);
            const unsigned a = acc[i];   // a non-root's word is never written here; a root's FG bit neither
            if (r != i) {
                if (r != j) __hip_atomic_store(p + i, r, CC_RLX, CC_AGENT);
                if (a) {   // a tile-local root: one atomic per local component
                    atomicAdd(acc + r, a & AREA);
                    if (a & BORDER) atomicOr(acc + r, BORDER);
                }
            } else {
                rootfg = (a & FG) != 0;
            }
        }
        n += __popcll(__ballot(rootfg));
    }
    if (bsum == nullptr) return;
    if (lane == 0) wsum[w] = n;
    __syncthreads();
    if (threadIdx.x == 0) bsum[(long)blockIdx.y * nchunk + blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

// grid (B), NT threads: bsum -> its exclusive scan, count[b] = the total
__global__ __launch_bounds__(NT) void scan_kernel(int nchunk, int* __restrict__ bsum, int* __restrict__ count) {
    __shared__ int sh[NT];
    int* s = bsum + (long)blockIdx.x * nchunk;
    int carry = 0;
    for (int c0 = 0; c0 < nchunk; c0 += NT) {
        const int c = c0 + threadIdx.x;
        const int v = c < nchunk ? s[c] : 0;
        sh[threadIdx.x] = v;
        __syncthreads();
        for (int o = 1; o < NT; o <<= 1) {   // Hillis-Steele inclusive scan
            const int add = threadIdx.x >= o ? sh[threadIdx.x - o] : 0;
            __syncthreads();
            sh[threadIdx.x] += add;
            __syncthreads();
        }
        if (c < nchunk) s[c] = carry + sh[threadIdx.x] - v;
        carry += sh[NT - 1];
        __syncthreads();
    }
    if (threadIdx.x == 0 && count) count[blockIdx.x] = carry;
}

__global__ __launch_bounds__(NT) void number_kernel(int HW, int nchunk, const int* __restrict__ P, const unsigned* __restrict__ A,
                                                    const int* __restrict__ bsum, int* __restrict__ N) {
    __shared__ int wsum[NT / 64];
    const long base = (long)blockIdx.y * HW;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int i0 = blockIdx.x * CHUNK + w * WCH;
    unsigned long long flags[WCH / 64];
    int n = 0;
#pragma unroll
    for (int k = 0; k < WCH / 64; ++k) {
        const int i = i0 + k * 64 + lane;
        const bool rootfg = i < HW && P[base + i] == i && (A[base + i] & FG);
        flags[k] = __ballot(rootfg);
        n += __popcll(flags[k]);
    }
    if (lane == 0) wsum[w] = n;
    __syncthreads();
    int rank = bsum[(long)blockIdx.y * nchunk + blockIdx.x];
    for (int j = 0; j < w; ++j) rank += wsum[j];
#pragma unroll
    for (int k = 0; k < WCH / 64; ++k) {
        const unsigned long long below = flags[k] & ((1ull << lane) - 1ull);
        if ((flags[k] >> lane) & 1ull) N[base + i0 + k * 64 + lane] = rank + __popcll(below) + 1;
        rank += __popcll(flags[k]);
    }
}

// grid (ceil(H W / NT), B)
__global__ __launch_bounds__(NT) void relabel_kernel(int HW, const int* __restrict__ P, const unsigned* __restrict__ A,
                                                     const int* __restrict__ N, int* __restrict__ comp, int* __restrict__ area) {
    const int i = blockIdx.x * NT + threadIdx.x;
    if (i >= HW) return;
    const long base = (long)blockIdx.y * HW;
    const int r = P[base + i];
    const unsigned a = A[base + r];
    if (comp) comp[base + i] = (a & FG) ? N[base + r] : 0;
    if (area) area[base + i] = (int)(a & AREA);
}

// ---- the rules -----------------------------------------------------------------------------------
struct Rules {
    int K;
    unsigned keep;            // bit c: keep only the largest component of class c
    int max_hole;             // < 0: any size
    int min_size[KMAX];
};

// a class the size and largest rules apply to: 1 .. K - 1, and 1 alone for K = 1
template <typename V> __device__ __forceinline__ bool ruled(V v, int K) { return v >= (V)1 && (long)v < (long)(K == 1 ? 2 : K); }

// grid (ceil(H W / NT), B): a zero pixel whose component misses the border (and is small enough) takes the value
// left of the component's root, which lies in the same row (x > 0: the component misses the border) and is not 0
// (a zero there would belong to the component and precede its first pixel).  out == in is safe: only zero
// pixels change, only non-zero ones are read besides a thread's own.
template <typename V>
__global__ __launch_bounds__(NT) void fill_kernel(int HW, Rules ru, const V* in, const int* __restrict__ P,
                                                  const unsigned* __restrict__ A, V* out) {
    const int i = blockIdx.x * NT + threadIdx.x;
    if (i >= HW) return;
    const long base = (long)blockIdx.y * HW;
    V v = in[base + i];
    if (v == (V)0) {
        const int r = P[base + i];
        const unsigned a = A[base + r];
        if (!(a & BORDER) && (ru.max_hole < 0 || (int)(a & AREA) <= ru.max_hole)) {
            const V f = in[base + r - 1];
            if (f > (V)0 && (long)f < (long)(ru.K == 1 ? 2 : ru.K)) v = f;
        }
    }
    out[base + i] = v;
}

__device__ __forceinline__ unsigned long long best_key(unsigned a, int r) {
    return ((unsigned long long)(a & AREA) << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)r);   // ties: the lowest root
}

// grid (ceil(H W / NT), B): the roots of kept-largest classes that pass the size rule bid for their class
template <typename V>
__global__ __launch_bounds__(NT) void best_kernel(int HW, Rules ru, const V* __restrict__ in, const int* __restrict__ P,
                                                  const unsigned* __restrict__ A, unsigned long long* best) {
    const int i = blockIdx.x * NT + threadIdx.x;
    if (i >= HW) return;
    const long base = (long)blockIdx.y * HW;
    if (P[base + i] != i) return;
    const V v = in[base + i];
    if (!ruled(v, ru.K) || !((ru.keep >> (int)v) & 1u)) return;
    const unsigned a = A[base + i];
    if ((int)(a & AREA) < ru.min_size[(int)v]) return;
    unsigned long long* slot = best + (long)blockIdx.y * KMAX + (int)v;
    const unsigned long long key = best_key(a, i);
    if (__hip_atomic_load(slot, CC_RLX, CC_AGENT) < key) atomicMax(slot, key);   // the load only spares atomics
}

// out == in is safe: a thread reads and writes its own pixel only
template <typename V>
__global__ __launch_bounds__(NT) void apply_kernel(int HW, Rules ru, const V* in, const int* __restrict__ P,
                                                   const unsigned* __restrict__ A, const unsigned long long* __restrict__ best,
                                                   V* out) {
    const int i = blockIdx.x * NT + threadIdx.x;
    if (i >= HW) return;
    const long base = (long)blockIdx.y * HW;
    V v = in[base + i];
    if (ruled(v, ru.K)) {
        const int c = (int)v, r = P[base + i];
        const unsigned a = A[base + r];
        if ((int)(a & AREA) < ru.min_size[c]) v = (V)0;
        else if (((ru.keep >> c) & 1u) && best[(long)blockIdx.y * KMAX + c] != best_key(a, r)) v = (V)0;
    }
    out[base + i] = v;
}

// ---- launchers ---------------------------------------------------------------------------------
struct Layout {
    size_t P, A, N, bsum, best, end;
};
Layout layout(long B, long H, long W, bool number, bool best) {
    const size_t px = (size_t)B * H * W, nchunk = ((size_t)H * W + CHUNK - 1) / CHUNK;
    Layout l;
    size_t o = 0;
    auto take = [&](size_t bytes) { const size_t at = o; o += up256(bytes); return at; };
    l.P = take(px * 4);
    l.A = take(px * 4);
    l.N = number ? take(px * 4) : 0;
    l.bsum = number ? take((size_t)B * nchunk * 4) : 0;
    l.best = best ? take((size_t)B * KMAX * 8) : 0;
    l.end = o;
    return l;
}

const char* check_dims(int B, int H, int W) {
    if (B < 1 || H < 1 || W < 1) return "B, H and W must be >= 1";
    if (H > DMAX || W > DMAX) return "H, W <= 32767";
    if (B > 65535) return "B <= 65535 images per call";
    if ((long)B * ((H + T - 1) / T) * ((W + T - 1) / T) > GRID_MAX) return "B ceil(H / 64) ceil(W / 64) must be <= 2^23 per call";
    return nullptr;
}
inline bool dtype_ok(int d) { return d == CSU_SURFACE_U8 || d == CSU_SURFACE_I64; }

// P and A of the map `labels`; with bsum the chunk counts of the non-zero roots too
template <typename V>
void label(int B, int H, int W, int conn8, const V* labels, int* P, unsigned* A, int* bsum, hipStream_t st) {
    const int HW = H * W, nchunk = (HW + CHUNK - 1) / CHUNK;
    tile_kernel<V><<<dim3((unsigned)((W + T - 1) / T), (unsigned)((H + T - 1) / T), (unsigned)B), TNT, 0, st>>>(H, W, conn8, labels,
                                                                                                                 P, A);
    const int nsr = (H - 1) / T, nsc = (W - 1) / T;
    const long n = (long)nsr * W + (long)nsc * H;   // < 2 * 512 * 32767
    if (n > 0) seam_kernel<V><<<dim3((unsigned)((n + NT - 1) / NT), (unsigned)B), NT, 0, st>>>(H, W, conn8, nsr, labels, P);
    flatten_kernel<<<dim3((unsigned)nchunk, (unsigned)B), NT, 0, st>>>(HW, nchunk, P, A, bsum);
}

template <typename V>
void filter(int B, int H, int W, int conn8, const Rules& ru, bool fill, const V* in, V* out, char* ws, const Layout& l,
            hipStream_t st) {
    const int HW = H * W;
    int* P = (int*)(ws + l.P);
    unsigned* A = (unsigned*)(ws + l.A);
    unsigned long long* best = (unsigned long long*)(ws + l.best);
    const dim3 grid((unsigned)((HW + NT - 1) / NT), (unsigned)B);
    bool sized = ru.keep != 0;
    for (int c = 0; c < KMAX; ++c) sized |= ru.min_size[c] > 0;
    const V* map = in;
    if (fill) {
        label<V>(B, H, W, conn8, in, P, A, nullptr, st);
        fill_kernel<V><<<grid, NT, 0, st>>>(HW, ru, in, P, A, out);
        map = out;
    }
    if (!sized) {
        if (!fill && (const void*)in != (void*)out)
            (void)hipMemcpyAsync(out, in, (size_t)B * HW * sizeof(V), hipMemcpyDeviceToDevice, st);
        return;
    }
    label<V>(B, H, W, conn8, map, P, A, nullptr, st);   // of the filled map: filling can join components
    if (ru.keep) {
        (void)hipMemsetAsync(best, 0, (size_t)B * KMAX * 8, st);   // an error shows in check_launch
        best_kernel<V><<<grid, NT, 0, st>>>(HW, ru, map, P, A, best);
    }
    apply_kernel<V><<<grid, NT, 0, st>>>(HW, ru, map, P, A, best, out);
}

}  // namespace
}  // namespace csu

using namespace csu;

extern "C" size_t csu_ccl_workspace(int B, int H, int W) {
    if (check_dims(B, H, W)) return 0;
    return layout(B, H, W, true, false).end;
}

extern "C" int csu_ccl(int B, int H, int W, int dtype, const void* labels, int connectivity, void* workspace, size_t ws_bytes,
                       int* comp, int* area, int* count, void* stream) {
    if (const char* e = check_dims(B, H, W)) return fail(CSU_E_ARG, std::string("ccl: ") + e);
    if (connectivity != CSU_CC_4 && connectivity != CSU_CC_8) return fail(CSU_E_ARG, "ccl: connectivity must be 4 or 8");
    if (!dtype_ok(dtype)) return fail(CSU_E_ARG, "ccl: the label map must be CSU_SURFACE_U8 or CSU_SURFACE_I64");
    if (!labels || !workspace) return fail(CSU_E_ARG, "ccl: null labels or workspace");
    if (!comp && !area && !count) return fail(CSU_E_ARG, "ccl: comp, area and count are all null");
    const Layout l = layout(B, H, W, true, false);
    if (ws_bytes < l.end) return fail(CSU_E_WORKSPACE, "ccl: workspace smaller than csu_ccl_workspace(B, H, W)");
    hipStream_t st = as_stream(stream);
    char* ws = (char*)workspace;
    int* P = (int*)(ws + l.P);
    unsigned* A = (unsigned*)(ws + l.A);
    int* N = (int*)(ws + l.N);
    int* bsum = (int*)(ws + l.bsum);
    const bool number = comp || count;
    const int conn8 = connectivity == CSU_CC_8;
    if (dtype == CSU_SURFACE_U8)
        label<uint8_t>(B, H, W, conn8, (const uint8_t*)labels, P, A, number ? bsum : nullptr, st);
    else
        label<int64_t>(B, H, W, conn8, (const int64_t*)labels, P, A, number ? bsum : nullptr, st);
    const int HW = H * W, nchunk = (HW + CHUNK - 1) / CHUNK;
    if (number) scan_kernel<<<B, NT, 0, st>>>(nchunk, bsum, count);
    if (comp) number_kernel<<<dim3((unsigned)nchunk, (unsigned)B), NT, 0, st>>>(HW, nchunk, P, A, bsum, N);
    if (comp || area)
        relabel_kernel<<<dim3((unsigned)((HW + NT - 1) / NT), (unsigned)B), NT, 0, st>>>(HW, P, A, N, comp, area);
    return check_launch("ccl");
}

extern "C" size_t csu_cc_filter_workspace(int B, int H, int W) {
    if (check_dims(B, H, W)) return 0;
    return layout(B, H, W, false, true).end;
}

extern "C" int csu_cc_filter(int B, int H, int W, int dtype, const void* labels, int connectivity, int num_classes,
                             const int* min_size, unsigned keep_largest, int fill_holes, int max_hole_size, void* workspace,
                             size_t ws_bytes, void* out, void* stream) {
    if (const char* e = check_dims(B, H, W)) return fail(CSU_E_ARG, std::string("cc_filter: ") + e);
    if (connectivity != CSU_CC_4 && connectivity != CSU_CC_8) return fail(CSU_E_ARG, "cc_filter: connectivity must be 4 or 8");
    if (!dtype_ok(dtype)) return fail(CSU_E_ARG, "cc_filter: the label map must be CSU_SURFACE_U8 or CSU_SURFACE_I64");
    if (num_classes < 1 || num_classes > KMAX) return fail(CSU_E_ARG, "cc_filter: 1 <= num_classes <= 32");
    if (max_hole_size < -1) return fail(CSU_E_ARG, "cc_filter: max_hole_size must be >= 0, or -1 for any size");
    Rules ru = {};
    ru.K = num_classes;
    ru.max_hole = max_hole_size;
    // the tables are indexed by class; num_classes = 1: entry 0 / bit 0 is the rule of the foreground value 1
    for (int c = 0; c < num_classes && min_size; ++c) {
        if (min_size[c] < 0) return fail(CSU_E_ARG, "cc_filter: min_size must be >= 0");
        if (num_classes == 1) ru.min_size[1] = min_size[0];
        else if (c >= 1) ru.min_size[c] = min_size[c];
    }
    if (num_classes == 1) ru.keep = (keep_largest & 1u) << 1;
    else ru.keep = keep_largest & (num_classes >= 32 ? 0xFFFFFFFEu : ((1u << num_classes) - 1u) & ~1u);
    if (!labels || !workspace || !out) return fail(CSU_E_ARG, "cc_filter: null labels, workspace or out");
    const Layout l = layout(B, H, W, false, true);
    if (ws_bytes < l.end) return fail(CSU_E_WORKSPACE, "cc_filter: workspace smaller than csu_cc_filter_workspace(B, H, W)");
    hipStream_t st = as_stream(stream);
    const int conn8 = connectivity == CSU_CC_8;
    if (dtype == CSU_SURFACE_U8)
        filter<uint8_t>(B, H, W, conn8, ru, fill_holes != 0, (const uint8_t*)labels, (uint8_t*)out, (char*)workspace, l, st);
    else
        filter<int64_t>(B, H, W, conn8, ru, fill_holes != 0, (const int64_t*)labels, (int64_t*)out, (char*)workspace, l, st);
    return check_launch("cc_filter");
}
