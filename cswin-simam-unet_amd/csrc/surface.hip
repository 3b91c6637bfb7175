// Surface-distance metrics (HD, HD95, ASSD, NSD; medpy's definitions) and an exact Euclidean distance
// transform for gfx950.  The reference scores with Dice / IoU only, so nothing here is a port.
//   field    one (image, class, side) binary border map of H x W, side 0 = prediction, 1 = target:
//            field = (b C + c) 2 + side; (b, c) is a "pair".  The transform has one field per image.
//   site     a border pixel of the field's mask (a mask pixel with one of its four edge neighbours outside
//            the mask; everything beyond the image is outside), decided from the label map itself.  For the
//            transform: a zero pixel of the mask.
//   column   g[field, y, x] = rows from (y, x) to the nearest site of column x (uint16; NONE = no site in
//            the column), so g == 0 marks the sites themselves and no border bitmap exists.
//   row      for every pixel that needs a value, d2 = min over x' of sy^2 g(y, x')^2 + sx^2 (x - x')^2 with g of
//            the OTHER side's field (the transform: its own), the row of g staged in LDS (2 W bytes <= 64 KiB).
//            The search goes outwards from x and stops once sx^2 k^2 alone reaches the best value: every
//            candidate at distance >= k is at least that, so the minimum is exact.  Equal spacing: int32 on
//            index distances (exact for every legal size: 2 * 32766^2 < 2^31), scaled by s^2 in fp64 at the
//            end; otherwise fp32.  Either way the non-negative 32-bit pattern of d2 orders as an unsigned key.
//   sums     per (field, row) partials {sum of d (fp64), max key, count, count <= tau} -> per field in a
//            fixed tree order: no floating-point atomics, bitwise repeatable, independent of the batching.
//   select   the keys of a pair's two sides are pooled in a list (slots from an integer atomic cursor: the
//            SET of keys is what matters) and the floor(h)-th and (floor(h)+1)-th order statistics,
//            h = (n - 1) q / 100, found by a 4 x 8-bit radix select: a histogram of the next byte among the
//            keys that match the prefix so far (integer atomics), the bin picked at the start of the next
//            launch by every workgroup alike.  Ranks come from the device-side counts.
//   finish   fp64 (hd, hd95, assd, nsd, |dP|, |dT|) per pair; NaN in the first four where a mask is empty.
// Signed distance maps (csu_signed_distance, the boundary loss's phi) reuse the column pass with two more site
// modes -- every pixel on the class, every pixel off it -- as the two fields of a pair, and one row pass that
// stages the row of both (4 W bytes of LDS) and searches, per pixel, the field of the other side.
#include <algorithm>

#include "common.hpp"

namespace csu {
namespace {

constexpr int CMAX = 32;
constexpr int DMAX = 32767;          // H, W: g fits uint16 below NONE, 2 W bytes of LDS fit 64 KiB
constexpr int SDMAX = 16383;         // signed distance maps: the rows of two fields share the 64 KiB
constexpr unsigned short NONE = 0xFFFF;
constexpr unsigned NOKEY_I = 0x7FFFFFFFu;   // no site at all (int path); above every legal 2 * 32766^2
constexpr int NT = 256;
constexpr int COLS = 64;             // columns per column-pass workgroup: one wave reads consecutive columns
constexpr int SEGMAX = 16;           // row segments of a column, one thread each
constexpr int PASSES = 4, BINS = 256;
constexpr int HBMAX = 64;            // histogram workgroups per pair
enum { SITE_CLASS = 0, SITE_BINARY = 1, SITE_ZERO = 2, SITE_EQ = 3, SITE_NE = 4 };
// SITE_CLASS / SITE_BINARY: the sites are a mask's border pixels; the others take every pixel that is zero, that
// holds the class (SITE_EQ), or that does not (SITE_NE), as a site
constexpr bool site_is_border(int mode) { return mode == SITE_CLASS || mode == SITE_BINARY; }

inline size_t up256(size_t n) { return (n + 255) & ~(size_t)255; }

// ---- column pass ------------------------------------------------------------------------------
template <typename T, int MODE>
__device__ __forceinline__ bool in_mask(const T* __restrict__ img, int H, int W, int y, int x, int cls) {
    if (y < 0 || y >= H || x < 0 || x >= W) return false;
    const T v = img[(long)y * W + x];
    return MODE == SITE_CLASS ? (long)v == (long)cls : v > (T)0;
}

// grid (ceil(W / COLS), pairs), block (COLS, nseg): thread (tx, s) owns rows [s seg, (s + 1) seg) of one column
template <typename T, int MODE>
__global__ __launch_bounds__(COLS* SEGMAX) void column_kernel(int C, int H, int W, int seg, int nside, int side, int class0,
                                                              const T* __restrict__ labels, unsigned short* __restrict__ g) {
    __shared__ int s_first[SEGMAX][COLS], s_last[SEGMAX][COLS];
    const int tx = threadIdx.x, s = threadIdx.y, nseg = blockDim.y;
    const int x = blockIdx.x * COLS + tx, pair = blockIdx.y;
    const int b = pair / C, cls = class0 + pair % C;
    const bool on = x < W;
    const T* img = labels + (long)b * H * W;
    unsigned short* gc = g + ((long)pair * nside + side) * H * W + x;
    const int y0 = min(H, s * seg), y1 = min(H, y0 + seg);
    // 1: sites of the segment, and the distance down from the nearest site above inside the segment
    int first = -1, last = -1;
    if (on) {
        bool up = false, cur = false;
        if (site_is_border(MODE) && y0 < y1) {
            up = in_mask<T, MODE>(img, H, W, y0 - 1, x, cls);
            cur = in_mask<T, MODE>(img, H, W, y0, x, cls);
        }
#pragma unroll 4
        for (int y = y0; y < y1; ++y) {
            bool site;
            if (MODE == SITE_ZERO) {
                site = img[(long)y * W + x] == (T)0;
            } else if (MODE == SITE_EQ || MODE == SITE_NE) {
                site = ((long)img[(long)y * W + x] == (long)cls) == (MODE == SITE_EQ);
            } else {
                const bool dn = in_mask<T, MODE>(img, H, W, y + 1, x, cls);
                const bool lf = in_mask<T, MODE>(img, H, W, y, x - 1, cls), rt = in_mask<T, MODE>(img, H, W, y, x + 1, cls);
                site = cur && !(up && dn && lf && rt);
                up = cur;
                cur = dn;
            }
            if (site) {
                if (first < 0) first = y;
                last = y;
            }
            gc[(long)y * W] = last < 0 ? NONE : (unsigned short)(y - last);
        }
    }
    s_first[s][tx] = first;
    s_last[s][tx] = last;
    __syncthreads();
    if (!on) return;
    int above = -1, below = -1;
    for (int j = 0; j < s; ++j)
        if (s_last[j][tx] >= 0) above = s_last[j][tx];
    for (int j = nseg - 1; j > s; --j)
        if (s_first[j][tx] >= 0) below = s_first[j][tx];
    // 2: the rows before the segment's first site take the carry from the segments above
    if (above >= 0) {
        const int ye = first < 0 ? y1 : first;
        for (int y = y0; y < ye; ++y) gc[(long)y * W] = (unsigned short)(y - above);
    }
    // 3: up the column
    int next = below;
#pragma unroll 4
    for (int y = y1 - 1; y >= y0; --y) {
        const unsigned short v = gc[(long)y * W];
        if (v == 0) next = y;
        const unsigned short c = next < 0 ? NONE : (unsigned short)(next - y);
        if (c < v) gc[(long)y * W] = c;
    }
}

// ---- row pass ---------------------------------------------------------------------------------
struct RowArgs {
    int H, W;
    float sy2, sx2;       // fp32 path
    double s2, tau;       // int path: s^2; tau for both
    const unsigned short* g;
    unsigned* keys;       // (pairs, cap)
    unsigned* cursor;     // (pairs)
    long cap;
    double* psum;         // (fields, H) partials
    unsigned *pmax, *pcnt, *ptau;
    float* edt;           // the transform's output (fields, H, W)
};

template <bool ISO> __device__ __forceinline__ double key_dist(unsigned key, double s2) {
    if (ISO) return key == NOKEY_I ? (double)INFINITY : sqrt((double)key * s2);
    return sqrt((double)__uint_as_float(key));
}

// min over x' of the squared distance from (y, x) through column x' (row = g of the row, LDS)
template <bool ISO>
__device__ __forceinline__ unsigned row_search(const unsigned short* row, int W, int x, float sy2, float sx2) {
    if (ISO) {
        int best = (int)NOKEY_I;
        const int g0 = row[x];
        if (g0 != NONE) best = g0 * g0;
        for (int k = 1; x - k >= 0 || x + k < W; ++k) {
            const int k2 = k * k;
            if (k2 >= best) break;
            if (x - k >= 0) {
                const int gv = row[x - k];
                if (gv != NONE) best = min(best, gv * gv + k2);
            }
            if (x + k < W) {
                const int gv = row[x + k];
                if (gv != NONE) best = min(best, gv * gv + k2);
            }
        }
        return (unsigned)best;
    } else {
        float best = INFINITY;
        const int g0 = row[x];
        if (g0 != NONE) best = sy2 * (float)(g0 * g0);
        for (int k = 1; x - k >= 0 || x + k < W; ++k) {
            const float kk = sx2 * (float)(k * k);
            if (kk >= best) break;
            if (x - k >= 0) {
                const int gv = row[x - k];
                if (gv != NONE) best = fminf(best, sy2 * (float)(gv * gv) + kk);
            }
            if (x + k < W) {
                const int gv = row[x + k];
                if (gv != NONE) best = fminf(best, sy2 * (float)(gv * gv) + kk);
            }
        }
        return __float_as_uint(best);
    }
}

struct Part {
    double sum;
    unsigned mx, cnt, tau;
};
__device__ __forceinline__ Part part_add(const Part& a, const Part& b) {
    Part r;
    r.sum = a.sum + b.sum;
    r.mx = max(a.mx, b.mx);
    r.cnt = a.cnt + b.cnt;
    r.tau = a.tau + b.tau;
    return r;
}
// the workgroup's total in thread 0, in a fixed order: xor butterfly inside a wave, then the waves in turn
__device__ __forceinline__ Part block_part(Part p, Part* sh) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        Part q;
        q.sum = __shfl_xor(p.sum, o, 64);
        q.mx = __shfl_xor(p.mx, o, 64);
        q.cnt = __shfl_xor(p.cnt, o, 64);
        q.tau = __shfl_xor(p.tau, o, 64);
        p = part_add(p, q);
    }
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) sh[w] = p;
    __syncthreads();
    if (threadIdx.x == 0)
        for (int j = 1; j < NT / 64; ++j) p = part_add(p, sh[j]);
    return p;
}

// grid (H, fields), NT threads, dynamic LDS max(2 W rounded up to 16, 128) bytes
template <bool ISO, bool EDT>
__global__ __launch_bounds__(NT) void row_kernel(RowArgs a) {
    extern __shared__ __align__(16) unsigned char smem[];
    unsigned short* row = reinterpret_cast<unsigned short*>(smem);
    const int W = a.W, y = blockIdx.x, f = blockIdx.y;
    const unsigned short* own = a.g + ((long)f * a.H + y) * W;
    const unsigned short* other = EDT ? own : a.g + ((long)(f ^ 1) * a.H + y) * W;
    int any = 0;
    for (int x = threadIdx.x; x < W; x += NT) {
        const unsigned short v = other[x];
        row[x] = v;
        any |= v != NONE;
    }
    any = __syncthreads_or(any);   // no site in any column of this row: the field has none at all
    const unsigned nokey = ISO ? NOKEY_I : __float_as_uint(INFINITY);
    Part p = {0.0, 0u, 0u, 0u};
    for (int x = threadIdx.x; x < W; x += NT) {
        if (!EDT && own[x] != 0) continue;
        const unsigned key = any ? row_search<ISO>(row, W, x, a.sy2, a.sx2) : nokey;
        const double d = key_dist<ISO>(key, a.s2);
        if (EDT) {
            a.edt[((long)f * a.H + y) * W + x] = (float)d;
        } else {
            p.sum += d;
            p.mx = max(p.mx, key);
            p.cnt += 1;
            p.tau += (ISO ? (key != NOKEY_I && (double)key * a.s2 <= a.tau * a.tau) : d <= a.tau) ? 1u : 0u;
            const unsigned slot = atomicAdd(a.cursor + (f >> 1), 1u);   // < cap = 2 H W: one slot per border pixel
            a.keys[(long)(f >> 1) * a.cap + slot] = key;
        }
    }
    if (!EDT) {
        __syncthreads();   // the row is done with: its LDS holds the waves' partials
        p = block_part(p, reinterpret_cast<Part*>(smem));
        if (threadIdx.x == 0) {
            const long i = (long)f * a.H + y;
            a.psum[i] = p.sum;
            a.pmax[i] = p.mx;
            a.pcnt[i] = p.cnt;
            a.ptau[i] = p.tau;
        }
    }
}

// ---- signed distance maps ---------------------------------------------------------------------------
// row_search with the outward walk cut at kmax columns (kmax >= W: no cut).  With a clip the caller passes the
// first k whose columns lie beyond the clip radius: what the cut leaves out cannot bring the result under it.
template <bool ISO>
__device__ __forceinline__ unsigned row_search_cut(const unsigned short* row, int W, int x, int kmax, float sy2, float sx2) {
    if (ISO) {
        int best = (int)NOKEY_I;
        const int g0 = row[x];
        if (g0 != NONE) best = g0 * g0;
        for (int k = 1; k < kmax && (x - k >= 0 || x + k < W); ++k) {
            const int k2 = k * k;
            if (k2 >= best) break;
            if (x - k >= 0) {
                const int gv = row[x - k];
                if (gv != NONE) best = min(best, gv * gv + k2);
            }
            if (x + k < W) {
                const int gv = row[x + k];
                if (gv != NONE) best = min(best, gv * gv + k2);
            }
        }
        return (unsigned)best;
    } else {
        float best = INFINITY;
        const int g0 = row[x];
        if (g0 != NONE) best = sy2 * (float)(g0 * g0);
        for (int k = 1; k < kmax && (x - k >= 0 || x + k < W); ++k) {
            const float kk = sx2 * (float)(k * k);
            if (kk >= best) break;
            if (x - k >= 0) {
                const int gv = row[x - k];
                if (gv != NONE) best = fminf(best, sy2 * (float)(gv * gv) + kk);
            }
            if (x + k < W) {
                const int gv = row[x + k];
                if (gv != NONE) best = fminf(best, sy2 * (float)(gv * gv) + kk);
            }
        }
        return __float_as_uint(best);
    }
}

struct SignedArgs {
    int H, W, C, out_classes, out_c0, kmax;
    float sy2, sx2;
    double s2, step, clip;      // step = min(sy, sx); clip <= 0: none
    const unsigned short* g;    // (pairs, 2, H, W): field 0 has its sites on the class, field 1 off it
    float* out;                 // (B, out_classes, H, W)
};

// grid (H, pairs), NT threads, dynamic LDS 4 W bytes rounded up to 16: the row of both fields.  A pixel on the class
// (g of field 0 is 0 there) searches field 1, any other pixel field 0.  A field without a site in this row's columns
// has none at all (g != NONE says "this column has a site"): the class is absent or fills the image, phi = 0.
template <bool ISO>
__global__ __launch_bounds__(NT) void signed_row_kernel(SignedArgs a) {
    extern __shared__ __align__(16) unsigned char smem[];
    unsigned short* on = reinterpret_cast<unsigned short*>(smem);
    const int W = a.W, y = blockIdx.x, pair = blockIdx.y;
    unsigned short* off = on + ((W + 7) & ~7);
    const unsigned short* g_on = a.g + (((long)pair * 2) * a.H + y) * W;
    const unsigned short* g_off = a.g + (((long)pair * 2 + 1) * a.H + y) * W;
    int any = 0;
    for (int x = threadIdx.x; x < W; x += NT) {
        const unsigned short u = g_on[x], v = g_off[x];
        on[x] = u;
        off[x] = v;
        any |= (u != NONE ? 1 : 0) | (v != NONE ? 2 : 0);
    }
    const int any_on = __syncthreads_or(any & 1), any_off = __syncthreads_or(any & 2);
    const bool both = any_on && any_off;
    const int b = pair / a.C, c = pair % a.C;
    float* o = a.out + (((long)b * a.out_classes + a.out_c0 + c) * a.H + y) * W;
    const unsigned step_key = __float_as_uint(fminf(a.sy2, a.sx2));
    for (int x = threadIdx.x; x < W; x += NT) {
        double phi = 0.0;
        if (both) {
            const bool inside = on[x] == 0;
            const unsigned key = row_search_cut<ISO>(inside ? off : on, W, x, a.kmax, a.sy2, a.sx2);
            const double d = key_dist<ISO>(key, a.s2);
            // the fp32 path: one step along the finer axis is the distance `step` itself, so that an inner border
            // pixel is 0 and not the rounding of sqrt(fp32(step^2)) - step
            phi = !inside ? d : (!ISO && key == step_key) ? 0.0 : a.step - d;
            if (a.clip > 0.0) phi = fmin(fmax(phi, -a.clip), a.clip);
        }
        o[x] = (float)phi;
    }
}

// ---- per-field totals and the ranks --------------------------------------------------------------
struct Sel {
    unsigned prefix, rank;
};
struct Tot {
    double* sum;          // (fields)
    unsigned *mx, *cnt, *tau;
    double* h;            // (pairs) the fractional rank (n - 1) q / 100
    Sel* state;           // (PASSES, pairs, 2)
    unsigned* hist;       // (PASSES, pairs, 2, BINS)
};

// grid (pairs), NT threads
__global__ __launch_bounds__(NT) void total_kernel(int H, int pairs, double q, RowArgs a, Tot t) {
    __shared__ Part sh[NT / 64];
    const int pair = blockIdx.x;
    unsigned n = 0;
    for (int side = 0; side < 2; ++side) {
        const long f = (long)pair * 2 + side;
        Part p = {0.0, 0u, 0u, 0u};
        for (int y = threadIdx.x; y < H; y += NT) {
            const Part r = {a.psum[f * H + y], a.pmax[f * H + y], a.pcnt[f * H + y], a.ptau[f * H + y]};
            p = part_add(p, r);
        }
        p = block_part(p, sh);
        if (threadIdx.x == 0) {
            t.sum[f] = p.sum;
            t.mx[f] = p.mx;
            t.cnt[f] = p.cnt;
            t.tau[f] = p.tau;
            n += p.cnt;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const double h = n ? (double)(n - 1) * q / 100.0 : 0.0;
        const unsigned r0 = (unsigned)floor(h);
        t.h[pair] = h;
        t.state[pair * 2 + 0] = {0u, r0};
        t.state[pair * 2 + 1] = {0u, n && r0 + 1 < n ? r0 + 1 : r0};
    }
}

// the selection after pass k - 1: the bin that holds the rank, appended to the prefix
__device__ __forceinline__ Sel pick(Sel s, const unsigned* __restrict__ hist) {
    unsigned cum = 0;
    int bin = 0;
    for (; bin < BINS - 1; ++bin) {
        const unsigned c = hist[bin];
        if (cum + c > s.rank) break;
        cum += c;
    }
    return {(s.prefix << 8) | (unsigned)bin, s.rank - cum};
}

// pass k: grid (hb, pairs), NT = BINS threads
__global__ __launch_bounds__(NT) void hist_kernel(int k, int pairs, const unsigned* __restrict__ keys, long cap,
                                                  const unsigned* __restrict__ cursor, Tot t) {
    __shared__ unsigned lh[2][BINS];
    __shared__ Sel sel[2];
    const int pair = blockIdx.y, tid = threadIdx.x;
    if (tid < 2) {
        Sel s = t.state[((long)(k > 0 ? k - 1 : 0) * pairs + pair) * 2 + tid];
        if (k > 0) {
            s = pick(s, t.hist + (((long)(k - 1) * pairs + pair) * 2 + tid) * BINS);
            if (blockIdx.x == 0) t.state[((long)k * pairs + pair) * 2 + tid] = s;
        }
        sel[tid] = s;
    }
    lh[0][tid] = 0;
    lh[1][tid] = 0;
    __syncthreads();
    const unsigned n = cursor[pair];
    const int shift = 24 - 8 * k;
    const unsigned p0 = sel[0].prefix, p1 = sel[1].prefix;
    const unsigned* kp = keys + (long)pair * cap;
    for (unsigned i = blockIdx.x * NT + tid; i < n; i += gridDim.x * NT) {
        const unsigned key = kp[i];
        const unsigned hi = k == 0 ? 0u : key >> (shift + 8), bin = (key >> shift) & (BINS - 1);
        if (hi == p0) atomicAdd(&lh[0][bin], 1u);
        if (hi == p1) atomicAdd(&lh[1][bin], 1u);
    }
    __syncthreads();
    unsigned* gh = t.hist + (((long)k * pairs + pair) * 2) * BINS;
    if (lh[0][tid]) atomicAdd(gh + tid, lh[0][tid]);
    if (lh[1][tid]) atomicAdd(gh + BINS + tid, lh[1][tid]);
}

// one thread per pair
template <bool ISO>
__global__ __launch_bounds__(64) void finish_kernel(int pairs, int C, int out_classes, int out_c0, double s2, Tot t,
                                                    double* __restrict__ out) {
    const int pair = blockIdx.x * 64 + threadIdx.x;
    if (pair >= pairs) return;
    const long f = (long)pair * 2;
    const unsigned cp = t.cnt[f], ct = t.cnt[f + 1];
    double* o = out + ((long)(pair / C) * out_classes + out_c0 + pair % C) * 6;
    o[4] = (double)cp;
    o[5] = (double)ct;
    if (cp == 0 || ct == 0) {
        o[0] = o[1] = o[2] = o[3] = (double)NAN;
        return;
    }
    double v[2];
    for (int j = 0; j < 2; ++j) {
        const long i = ((long)(PASSES - 1) * pairs + pair) * 2 + j;
        v[j] = key_dist<ISO>(pick(t.state[i], t.hist + i * BINS).prefix, s2);
    }
    const double h = t.h[pair];
    o[0] = key_dist<ISO>(max(t.mx[f], t.mx[f + 1]), s2);
    o[1] = v[0] + (h - floor(h)) * (v[1] - v[0]);
    o[2] = (t.sum[f] / (double)cp + t.sum[f + 1] / (double)ct) * 0.5;
    o[3] = ((double)t.tau[f] + (double)t.tau[f + 1]) / ((double)cp + (double)ct);
}

// ---- launchers ----------------------------------------------------------------------------------
template <int MODE>
void launch_columns(int dtype, int pairs, int C, int H, int W, int nside, int side, int class0, const void* labels,
                    unsigned short* g, hipStream_t st) {
    const int nseg = min(SEGMAX, (H + 63) / 64), seg = (H + nseg - 1) / nseg;
    const dim3 grid((unsigned)((W + COLS - 1) / COLS), (unsigned)pairs), block(COLS, nseg);
    if (dtype == CSU_SURFACE_U8)
        column_kernel<uint8_t, MODE><<<grid, block, 0, st>>>(C, H, W, seg, nside, side, class0, (const uint8_t*)labels, g);
    else
        column_kernel<int64_t, MODE><<<grid, block, 0, st>>>(C, H, W, seg, nside, side, class0, (const int64_t*)labels, g);
}

inline size_t row_lds(int W) { return std::max<size_t>(((size_t)W * 2 + 15) & ~(size_t)15, 128); }

template <bool ISO, bool EDT> void launch_rows(dim3 grid, int W, const RowArgs& a, hipStream_t st) {
    const size_t lds = row_lds(W);
    // the longest rows fill 64 KiB, and __syncthreads_or keeps a few words of its own: ask for more than the default
    // limit (a CU has 160 KiB).  A host-side attribute of the function, not a stream operation: legal under capture
    if (lds + 1024 > 65536)
        (void)hipFuncSetAttribute((const void*)row_kernel<ISO, EDT>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    row_kernel<ISO, EDT><<<grid, NT, lds, st>>>(a);
}

struct Layout {
    size_t g, keys, psum, pmax, pcnt, ptau, tsum, tmx, tcnt, ttau, h, state, zero, cursor, hist, end;
};
Layout layout(long pairs, long H, long W) {
    const size_t N = (size_t)pairs * 2, hw = (size_t)H * W;
    Layout l;
    size_t o = 0;
    auto take = [&](size_t bytes) { const size_t at = o; o += up256(bytes); return at; };
    l.g = take(N * hw * 2);
    l.keys = take((size_t)pairs * 2 * hw * 4);
    l.psum = take(N * H * 8);
    l.pmax = take(N * H * 4);
    l.pcnt = take(N * H * 4);
    l.ptau = take(N * H * 4);
    l.tsum = take(N * 8);
    l.tmx = take(N * 4);
    l.tcnt = take(N * 4);
    l.ttau = take(N * 4);
    l.h = take((size_t)pairs * 8);
    l.state = take((size_t)PASSES * pairs * 2 * sizeof(Sel));
    l.zero = o;   // cursor and histograms: cleared by every call
    l.cursor = take((size_t)pairs * 4);
    l.hist = take((size_t)PASSES * pairs * 2 * BINS * 4);
    l.end = o;
    return l;
}

const char* check_dims(int B, int C, int H, int W) {
    if (B < 1 || H < 1 || W < 1) return "B, H and W must be >= 1";
    if (H > DMAX || W > DMAX) return "H, W <= 32767";
    if (C < 1 || C > CMAX) return "1 <= C <= 32 classes per call";
    if ((long)B * C * 2 > 65535) return "B * C * 2 fields must be <= 65535 per call";
    return nullptr;
}
inline bool dtype_ok(int d) { return d == CSU_SURFACE_U8 || d == CSU_SURFACE_I64; }

}  // namespace
}  // namespace csu

using namespace csu;

extern "C" size_t csu_surface_workspace(int B, int C, int H, int W) {
    if (check_dims(B, C, H, W)) return 0;
    return layout((long)B * C, H, W).end;
}

extern "C" int csu_surface_metrics(int B, int C, int H, int W, int mode, int class0, int pred_dtype, const void* pred,
                                   int target_dtype, const void* target, double sy, double sx, double tolerance,
                                   double percentile, void* workspace, size_t ws_bytes, double* out, int out_classes,
                                   int out_c0, void* stream) {
    if (const char* e = check_dims(B, C, H, W)) return fail(CSU_E_ARG, std::string("surface_metrics: ") + e);
    if (mode != CSU_SURFACE_LABELS && mode != CSU_SURFACE_BINARY)
        return fail(CSU_E_ARG, "surface_metrics: mode must be CSU_SURFACE_LABELS or CSU_SURFACE_BINARY");
    if (mode == CSU_SURFACE_BINARY && C != 1) return fail(CSU_E_ARG, "surface_metrics: the binary form has C = 1");
    if (!dtype_ok(pred_dtype) || !dtype_ok(target_dtype))
        return fail(CSU_E_ARG, "surface_metrics: label maps must be CSU_SURFACE_U8 or CSU_SURFACE_I64");
    if (!(sy > 0.0) || !(sx > 0.0) || !(sy < INFINITY) || !(sx < INFINITY))
        return fail(CSU_E_ARG, "surface_metrics: spacing must be positive and finite");
    if (!(tolerance >= 0.0)) return fail(CSU_E_ARG, "surface_metrics: tolerance must be >= 0");
    if (!(percentile >= 0.0 && percentile <= 100.0)) return fail(CSU_E_ARG, "surface_metrics: 0 <= percentile <= 100");
    if (out_classes < C || out_c0 < 0 || out_c0 + C > out_classes)
        return fail(CSU_E_ARG, "surface_metrics: the C classes must lie inside the out_classes rows of out");
    if (!pred || !target || !workspace || !out) return fail(CSU_E_ARG, "surface_metrics: null pred, target, workspace or out");
    const int pairs = B * C;
    const Layout l = layout(pairs, H, W);
    if (ws_bytes < l.end) return fail(CSU_E_WORKSPACE, "surface_metrics: workspace smaller than csu_surface_workspace(B, C, H, W)");
    hipStream_t st = as_stream(stream);
    char* ws = (char*)workspace;
    (void)hipMemsetAsync(ws + l.zero, 0, l.end - l.zero, st);   // an error shows in check_launch below
    unsigned short* g = (unsigned short*)(ws + l.g);
    if (mode == CSU_SURFACE_LABELS) {
        launch_columns<SITE_CLASS>(pred_dtype, pairs, C, H, W, 2, 0, class0, pred, g, st);
        launch_columns<SITE_CLASS>(target_dtype, pairs, C, H, W, 2, 1, class0, target, g, st);
    } else {
        launch_columns<SITE_BINARY>(pred_dtype, pairs, C, H, W, 2, 0, 0, pred, g, st);
        launch_columns<SITE_BINARY>(target_dtype, pairs, C, H, W, 2, 1, 0, target, g, st);
    }
    RowArgs a;
    a.H = H; a.W = W;
    a.sy2 = (float)(sy * sy); a.sx2 = (float)(sx * sx);
    a.s2 = sy * sy; a.tau = tolerance;
    a.g = g;
    a.keys = (unsigned*)(ws + l.keys);
    a.cursor = (unsigned*)(ws + l.cursor);
    a.cap = 2L * H * W;
    a.psum = (double*)(ws + l.psum);
    a.pmax = (unsigned*)(ws + l.pmax); a.pcnt = (unsigned*)(ws + l.pcnt); a.ptau = (unsigned*)(ws + l.ptau);
    a.edt = nullptr;
    Tot t;
    t.sum = (double*)(ws + l.tsum);
    t.mx = (unsigned*)(ws + l.tmx); t.cnt = (unsigned*)(ws + l.tcnt); t.tau = (unsigned*)(ws + l.ttau);
    t.h = (double*)(ws + l.h);
    t.state = (Sel*)(ws + l.state);
    t.hist = (unsigned*)(ws + l.hist);
    const bool iso = sy == sx;
    const dim3 rgrid((unsigned)H, (unsigned)pairs * 2);
    if (iso)
        launch_rows<true, false>(rgrid, W, a, st);
    else
        launch_rows<false, false>(rgrid, W, a, st);
    total_kernel<<<pairs, NT, 0, st>>>(H, pairs, percentile, a, t);
    const long hb = std::min<long>(HBMAX, std::max<long>(1, (a.cap + 4095) / 4096));
    for (int k = 0; k < PASSES; ++k)
        hist_kernel<<<dim3((unsigned)hb, (unsigned)pairs), NT, 0, st>>>(k, pairs, a.keys, a.cap, a.cursor, t);
    if (iso)
        finish_kernel<true><<<(pairs + 63) / 64, 64, 0, st>>>(pairs, C, out_classes, out_c0, a.s2, t, out);
    else
        finish_kernel<false><<<(pairs + 63) / 64, 64, 0, st>>>(pairs, C, out_classes, out_c0, a.s2, t, out);
    return check_launch("surface_metrics");
}

extern "C" size_t csu_edt_workspace(int B, int H, int W) {
    if (check_dims(B, 1, H, W) || B > 65535) return 0;
    return up256((size_t)B * H * W * 2);
}

extern "C" int csu_edt(int B, int H, int W, int dtype, const void* mask, double sy, double sx, void* workspace,
                       size_t ws_bytes, float* out, void* stream) {
    if (const char* e = check_dims(B, 1, H, W)) return fail(CSU_E_ARG, std::string("edt: ") + e);
    if (B > 65535) return fail(CSU_E_ARG, "edt: B <= 65535 images per call");
    if (!dtype_ok(dtype)) return fail(CSU_E_ARG, "edt: the mask must be CSU_SURFACE_U8 or CSU_SURFACE_I64");
    if (!(sy > 0.0) || !(sx > 0.0) || !(sy < INFINITY) || !(sx < INFINITY))
        return fail(CSU_E_ARG, "edt: spacing must be positive and finite");
    if (!mask || !workspace || !out) return fail(CSU_E_ARG, "edt: null mask, workspace or out");
    if (ws_bytes < csu_edt_workspace(B, H, W)) return fail(CSU_E_WORKSPACE, "edt: workspace smaller than csu_edt_workspace(B, H, W)");
    hipStream_t st = as_stream(stream);
    unsigned short* g = (unsigned short*)workspace;
    launch_columns<SITE_ZERO>(dtype, B, 1, H, W, 1, 0, 0, mask, g, st);
    RowArgs a = {};
    a.H = H; a.W = W;
    a.sy2 = (float)(sy * sy); a.sx2 = (float)(sx * sx);
    a.s2 = sy * sy;
    a.g = g;
    a.edt = out;
    const dim3 rgrid((unsigned)H, (unsigned)B);
    if (sy == sx)
        launch_rows<true, true>(rgrid, W, a, st);
    else
        launch_rows<false, true>(rgrid, W, a, st);
    return check_launch("edt");
}

// ---- signed distance maps of a label map's classes (the boundary loss's phi) --------------------------
static const char* check_signed(int B, int C, int H, int W) {
    if (B < 1 || H < 1 || W < 1) return "B, H and W must be >= 1";
    if (H > SDMAX || W > SDMAX) return "H, W <= 16383";
    if (C < 1 || C > CMAX) return "1 <= C <= 32 classes per call";
    if ((long)B * C * 2 > 65535) return "B * C * 2 fields must be <= 65535 per call";
    return nullptr;
}

extern "C" size_t csu_signed_distance_workspace(int B, int C, int H, int W) {
    if (check_signed(B, C, H, W)) return 0;
    return up256((size_t)B * C * 2 * H * W * 2);
}

extern "C" int csu_signed_distance(int B, int C, int H, int W, int class0, int dtype, const void* labels, double sy,
                                   double sx, double clip, void* workspace, size_t ws_bytes, float* out, int out_classes,
                                   int out_c0, void* stream) {
    if (const char* e = check_signed(B, C, H, W)) return fail(CSU_E_ARG, std::string("signed_distance: ") + e);
    if (!dtype_ok(dtype)) return fail(CSU_E_ARG, "signed_distance: the label map must be CSU_SURFACE_U8 or CSU_SURFACE_I64");
    if (!(sy > 0.0) || !(sx > 0.0) || !(sy < INFINITY) || !(sx < INFINITY))
        return fail(CSU_E_ARG, "signed_distance: spacing must be positive and finite");
    if (!(clip < 0.0) && !(clip > 0.0 && clip < INFINITY))
        return fail(CSU_E_ARG, "signed_distance: clip must be positive and finite, or negative for none");
    if (out_classes < C || out_c0 < 0 || out_c0 + C > out_classes)
        return fail(CSU_E_ARG, "signed_distance: the C classes must lie inside the out_classes planes of out");
    if (!labels || !workspace || !out) return fail(CSU_E_ARG, "signed_distance: null labels, workspace or out");
    if (ws_bytes < csu_signed_distance_workspace(B, C, H, W))
        return fail(CSU_E_WORKSPACE, "signed_distance: workspace smaller than csu_signed_distance_workspace(B, C, H, W)");
    hipStream_t st = as_stream(stream);
    const int pairs = B * C;
    unsigned short* g = (unsigned short*)workspace;
    launch_columns<SITE_EQ>(dtype, pairs, C, H, W, 2, 0, class0, labels, g, st);
    launch_columns<SITE_NE>(dtype, pairs, C, H, W, 2, 1, class0, labels, g, st);
    SignedArgs a;
    a.H = H; a.W = W; a.C = C; a.out_classes = out_classes; a.out_c0 = out_c0;
    a.sy2 = (float)(sy * sy); a.sx2 = (float)(sx * sx);
    a.s2 = sy * sy; a.step = std::min(sy, sx); a.clip = clip;
    // columns from sx k >= clip + step on lie beyond every value the clip lets through; one more for the rounding
    const double kcut = clip > 0.0 ? std::ceil((clip + a.step) / sx) + 1.0 : (double)W;
    a.kmax = (int)std::min<double>(kcut, (double)W);
    a.g = g;
    a.out = out;
    const size_t lds = ((size_t)((W + 7) & ~7) * 2 + (size_t)W * 2 + 15) & ~(size_t)15;
    const dim3 grid((unsigned)H, (unsigned)pairs);
    const bool iso = sy == sx;
    // as launch_rows: the longest rows fill 64 KiB and __syncthreads_or keeps a few words of its own
    if (lds + 1024 > 65536)
        (void)hipFuncSetAttribute(iso ? (const void*)signed_row_kernel<true> : (const void*)signed_row_kernel<false>,
                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (iso)
        signed_row_kernel<true><<<grid, NT, lds, st>>>(a);
    else
        signed_row_kernel<false><<<grid, NT, lds, st>>>(a);
    return check_launch("signed_distance");
}
