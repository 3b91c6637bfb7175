// Affine + elastic + intensity augmentation for gfx950 with parameters drawn on the device (include/csu.h,
// "Affine + elastic + intensity augmentation"): rotation by any angle, zoom, shift, flips, quarter turns,
// a cubic B-spline deformation, contrast / brightness / gamma / noise, for uint8 images with binary masks
// (bilinear or nearest) or label maps (nearest, int64 out).  The reference has no counterpart.
//
//   augment_draw_kernel   one thread per image: 6 Philox calls -> the raw draws and the folded inverse
//                         affine (composed in fp64, rounded once) of table row b
//   augment_ctrl_kernel   the control displacements, 4 per Philox call
//   augment_sum_kernel    exact integer byte sum per image (16-byte loads, v_sad_u8, one 64-bit atomic per block)
//   warp_kernel<POOL>     the hot one: a 64 x 4 output tile per 256-thread block (each wave stores 256
//                         contiguous bytes per plane), the tile's control points staged in LDS, a gather of the
//                         4 bilinear taps from the uint8 source, intensity steps in registers, one pass, no atomics;
//                         the source is a batch of the output's size, or per slot an image of a patch pool
#include "common.hpp"
#include "rng.hpp"

namespace csu {
namespace {

constexpr int NT = 256;
constexpr int P = CSU_AUGMENT_P;
constexpr int TX = 64, TY = 4;                 // output tile of the warp kernel
constexpr int MIN_SPACING = 4;
constexpr int ORIGIN_MAX = 1 << 24;            // a patch origin beyond it is clamped (floats stay exact)
constexpr int CX = TX / MIN_SPACING + 4;       // control points a tile can need at the smallest spacing
constexpr int CY = TY / MIN_SPACING + 4;
enum { T_HFLIP, T_VFLIP, T_ROT90, T_ANGLE, T_SCALE, T_TX, T_TY, T_CONTRAST, T_BRIGHT, T_GAMMA, T_SIGMA, T_ELASTIC, T_A };

__device__ __forceinline__ float in_range(float u, float lo, float hi) { return fminf(fmaxf(lo + u * (hi - lo), lo), hi); }

__global__ __launch_bounds__(NT) void augment_draw_kernel(csu_augment_config cfg, int B, int H, int W,
                                                          const uint64_t* __restrict__ rng, uint32_t site,
                                                          float* __restrict__ table) {
    const int b = blockIdx.x * NT + threadIdx.x;
    if (b >= B) return;
    const Snap s = load_snap(rng);
    float u[24];
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        const uint4 v = draw4(s, (uint32_t)j, b, site);
        u[4 * j] = u01(v.x); u[4 * j + 1] = u01(v.y); u[4 * j + 2] = u01(v.z); u[4 * j + 3] = u01(v.w);
    }
    const int hf = u[0] < cfg.p_hflip, vf = u[1] < cfg.p_vflip;
    int k = 0;
    if (u[2] < cfg.p_rot90) { k = 1 + (int)(u[3] * 3.f); k = k > 3 ? 3 : k; }
    const float angle = u[4] < cfg.p_rotate ? in_range(u[5], cfg.rotate_lo, cfg.rotate_hi) : 0.f;
    float scale = 1.f;
    if (u[6] < cfg.p_scale) {
        const float l0 = logf(cfg.scale_lo), l1 = logf(cfg.scale_hi);
        scale = fminf(fmaxf(expf(l0 + u[7] * (l1 - l0)), cfg.scale_lo), cfg.scale_hi);
    }
    const bool tr = u[8] < cfg.p_translate;
    const float tx = tr ? in_range(u[9], -cfg.translate_x, cfg.translate_x) : 0.f;
    const float ty = tr ? in_range(u[10], -cfg.translate_y, cfg.translate_y) : 0.f;
    float* row = table + (long)b * P;
    row[T_HFLIP] = (float)hf;
    row[T_VFLIP] = (float)vf;
    row[T_ROT90] = (float)k;
    row[T_ANGLE] = angle;
    row[T_SCALE] = scale;
    row[T_TX] = tx;
    row[T_TY] = ty;
    row[T_CONTRAST] = u[11] < cfg.p_contrast ? in_range(u[12], cfg.contrast_lo, cfg.contrast_hi) : 1.f;
    row[T_BRIGHT] = u[13] < cfg.p_brightness ? in_range(u[14], cfg.brightness_lo, cfg.brightness_hi) : 1.f;
    row[T_GAMMA] = u[15] < cfg.p_gamma ? in_range(u[16], cfg.gamma_lo, cfg.gamma_hi) : 1.f;
    row[T_SIGMA] = u[17] < cfg.p_noise ? in_range(u[18], cfg.noise_lo, cfg.noise_hi) : 0.f;
    row[T_ELASTIC] = u[19] < cfg.p_elastic ? in_range(u[20], cfg.elastic_lo, cfg.elastic_hi) : 0.f;
    // L = F Q(k)^T R(angle)^T / scale, in fp64 (B threads: the cost is nothing, and A is then the fp64
    // composition rounded once)
    double c = 1.0, sn = 0.0;
    if (angle != 0.f) { c = cos((double)angle); sn = sin((double)angle); }
    const double inv = 1.0 / (double)scale;
    double l00 = c * inv, l01 = sn * inv, l10 = -sn * inv, l11 = c * inv;
    for (int i = 0; i < k; ++i) {      // Q^T = [[0, 1], [-1, 0]] from the left
        const double r00 = l10, r01 = l11, r10 = -l00, r11 = -l01;
        l00 = r00; l01 = r01; l10 = r10; l11 = r11;
    }
    if (hf) { l00 = -l00; l01 = -l01; }
    if (vf) { l10 = -l10; l11 = -l11; }
    const double cx = 0.5 * (W - 1), cy = 0.5 * (H - 1), px = cx + (double)tx, py = cy + (double)ty;
    row[T_A + 0] = (float)l00;
    row[T_A + 1] = (float)l01;
    row[T_A + 2] = (float)(cx - (l00 * px + l01 * py));
    row[T_A + 3] = (float)l10;
    row[T_A + 4] = (float)l11;
    row[T_A + 5] = (float)(cy - (l10 * px + l11 * py));
    row[T_A + 6] = 0.f;
    row[T_A + 7] = 0.f;
}

// ctrl[b][e], e over the n = 2 Gy Gx values of an image: 4 per Philox call
__global__ __launch_bounds__(NT) void augment_ctrl_kernel(int B, int n, const uint64_t* __restrict__ rng, uint32_t site,
                                                          const float* __restrict__ table, float* __restrict__ ctrl) {
    const Snap s = load_snap(rng);
    const int ng = (n + 3) / 4;
    const long total = (long)B * ng;
    for (long q = (long)blockIdx.x * NT + threadIdx.x; q < total; q += (long)gridDim.x * NT) {
        const int b = (int)(q / ng), g = (int)(q - (long)b * ng);
        const float mag = table[(long)b * P + T_ELASTIC];
        const uint4 v = draw4(s, (uint32_t)g, b, site);
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (4 * g + j < n) ctrl[(long)b * n + 4 * g + j] = (2.f * u01(w[j]) - 1.f) * mag;
    }
}

__device__ __forceinline__ uint32_t sum4(uint32_t w) { return __builtin_amdgcn_sad_u8(w, 0u, 0u); }

// sums[b] += the bytes of image b (n each): grid (blocks, B)
__global__ __launch_bounds__(NT) void augment_sum_kernel(long n, const uint8_t* __restrict__ img,
                                                         unsigned long long* __restrict__ sums) {
    __shared__ unsigned long long part[NT / 64];
    const int b = blockIdx.y;
    const uint8_t* p = img + (long)b * n;
    long head = (long)((16 - ((uintptr_t)p & 15)) & 15);
    if (head > n) head = n;
    const long nvec = (n - head) / 16, tail = n - head - nvec * 16;
    const uint4* pv = reinterpret_cast<const uint4*>(p + head);
    unsigned long long acc = 0;
    for (long i = (long)blockIdx.x * NT + threadIdx.x; i < nvec; i += (long)gridDim.x * NT) {
        const uint4 v = pv[i];
        acc += sum4(v.x) + sum4(v.y) + sum4(v.z) + sum4(v.w);
    }
    if (blockIdx.x == 0) {     // the unaligned ends, at most 15 bytes each
        if ((long)threadIdx.x < head) acc += p[threadIdx.x];
        if ((long)threadIdx.x < tail) acc += p[head + nvec * 16 + threadIdx.x];
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o, 64);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long t = 0;
#pragma unroll
        for (int i = 0; i < NT / 64; ++i) t += part[i];
        atomicAdd(&sums[b], t);
    }
}

__global__ void augment_mean_kernel(int B, long n, const unsigned long long* __restrict__ sums, float* __restrict__ mean) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < B) mean[b] = (float)((double)sums[b] / (255.0 * (double)n));
}

struct WarpArgs {
    int B, H, W;
    uint32_t site;
    int spacing, border, mask_mode, pad_label;
    float fill;            // image_fill in source units (x 255)
};

// uniform cubic B-spline basis at f in [0, 1)
__device__ __forceinline__ void bspline(float f, float* w) {
    const float g = 1.f - f, f2 = f * f, f3 = f2 * f;
    w[0] = g * g * g * (1.f / 6.f);
    w[1] = (3.f * f3 - 6.f * f2 + 4.f) * (1.f / 6.f);
    w[2] = (-3.f * f3 + 3.f * f2 + 3.f * f + 1.f) * (1.f / 6.f);
    w[3] = f3 * (1.f / 6.f);
}

// Both warp kernels.  POOL = false: slot b reads image b of an (B, H, W) batch, the output's size
// (csu_augment_warp; meta, record and N are unused).  POOL = true: slot b reads image record[b][0] of a patch pool
// (csu_patch_warp): its own H_n x W_n, pixel offset and mean from meta / means, the patch's integer origin (ox, oy)
// from the record.  The source position is evaluated in the output's frame and the origin is added to the integer
// tap coordinates only, so its precision does not depend on where in a large image the patch lies; with origin 0
// and equal sizes the arithmetic is the batch kernel's operation for operation.  The kernel itself is the
// template: as an inlined device function the same body loses the kernel arguments' noalias and schedules
// differently (3 VGPRs more); this way the POOL = false instantiation is instruction for instruction what it was.
// grid (tiles in x, tiles in y, slots): the tile comes from the block index with no division; the pointers are
// restrict kernel arguments, so the block-uniform table, record and meta rows are read with scalar loads
template <bool POOL>
__global__ __launch_bounds__(NT) void warp_kernel(WarpArgs a, const uint8_t* __restrict__ img,
                                                  const uint8_t* __restrict__ mask, const float* __restrict__ table,
                                                  const float* __restrict__ ctrl, const float* __restrict__ means,
                                                  const uint64_t* __restrict__ rng, float* __restrict__ oimg,
                                                  void* __restrict__ omask, const long long* __restrict__ meta,
                                                  const int* __restrict__ record, int N) {
    __shared__ float cs[2][CY][CX];
    const int H = a.H, W = a.W, sp = a.spacing;
    const int lx = threadIdx.x & (TX - 1), ly = threadIdx.x / TX;
    const int x0 = blockIdx.x * TX, y0 = blockIdx.y * TY, x = x0 + lx, y = y0 + ly;
    const int Gx = sp > 0 ? (W + sp - 1) / sp + 3 : 0, Gy = sp > 0 ? (H + sp - 1) / sp + 3 : 0;
    const bool replicate = a.border == CSU_AUG_REPLICATE;
    for (int b = blockIdx.z; b < a.B; b += gridDim.z) {
        const float* row = table + (long)b * P;
        const bool elastic = ctrl != nullptr && row[T_ELASTIC] != 0.f;     // the same in the whole block
        const int ix0 = elastic ? x0 / sp : 0, iy0 = elastic ? y0 / sp : 0;
        if (elastic) {
            const int xl = min(x0 + TX, W) - 1, yl = min(y0 + TY, H) - 1;
            const int nx = min(xl / sp - ix0 + 4, CX), ny = min(yl / sp - iy0 + 4, CY);
            __syncthreads();      // the tile before has been read
            for (int i = threadIdx.x; i < 2 * ny * nx; i += NT) {
                const int ch = i / (ny * nx), q = i - ch * ny * nx, jy = q / nx, jx = q - jy * nx;
                cs[ch][jy][jx] = ctrl[(((long)b * 2 + ch) * Gy + iy0 + jy) * Gx + ix0 + jx];
            }
            __syncthreads();
        }
        if (x >= W || y >= H) continue;     // no barrier below
        // the source of this slot: SH x SW pixels from pixel `pbase` on, the output's (0, 0) at (ox, oy) in it
        int SH = H, SW = W, ox = 0, oy = 0, mi = b;
        long pbase = 0;
        if constexpr (POOL) {
            const int* rec = record + (long)b * CSU_PATCH_RECORD;
            mi = min(max(rec[0], 0), N - 1);
            const long long* m = meta + (long)mi * 4;
            pbase = (long)m[0]; SH = (int)m[1]; SW = (int)m[2];
            oy = min(max(rec[4], -ORIGIN_MAX), ORIGIN_MAX);
            ox = min(max(rec[5], -ORIGIN_MAX), ORIGIN_MAX);
        }
        float px = (float)x, py = (float)y;
        if (elastic) {
            const int ix = x / sp, iy = y / sp;
            float wx[4], wy[4];
            bspline((float)(x - ix * sp) / (float)sp, wx);
            bspline((float)(y - iy * sp) / (float)sp, wy);
            const int jx = min(ix - ix0, CX - 4), jy = min(iy - iy0, CY - 4);
            const float bx = cs[0][jy][jx], by = cs[1][jy][jx];
            float dx = 0.f, dy = 0.f;
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float w = wy[i] * wx[j];
                    dx += w * (cs[0][jy + i][jx + j] - bx);
                    dy += w * (cs[1][jy + i][jx + j] - by);
                }
            px += bx + dx;
            py += by + dy;
        }
        float sx = fmaf(row[T_A + 0], px, fmaf(row[T_A + 1], py, row[T_A + 2]));
        float sy = fmaf(row[T_A + 3], px, fmaf(row[T_A + 4], py, row[T_A + 5]));
        // replicate: the coordinate is clamped to the image; constant: to a band in which every tap is
        // still outside (keeps the integer conversions in range for any table, NaN included)
        // (in the output's frame: the bounds are the source's less the origin, exact floats below 2^24)
        sx = replicate ? fminf(fmaxf(sx, (float)(0 - ox)), (float)(SW - 1 - ox))
                       : fminf(fmaxf(sx, (float)(-2 - ox)), (float)(SW + 1 - ox));
        sy = replicate ? fminf(fmaxf(sy, (float)(0 - oy)), (float)(SH - 1 - oy))
                       : fminf(fmaxf(sy, (float)(-2 - oy)), (float)(SH + 1 - oy));
        const float flx = floorf(sx), fly = floorf(sy);
        const float fx = sx - flx, fy = sy - fly;
        const int xi[2] = {(int)flx + ox, (int)flx + ox + 1}, yi[2] = {(int)fly + oy, (int)fly + oy + 1};
        const float wx2[2] = {1.f - fx, fx}, wy2[2] = {1.f - fy, fy};
        const bool bilinear_mask = a.mask_mode == CSU_AUG_MASK_BILINEAR;
        const long ibase = POOL ? pbase : (long)b * H * W;
        // Every load is unconditional, from a clamped (always legal) address, and all are issued before the first
        // use: a load written under `inside ? load : fill` compiles to a branch and a full wait per tap.
        long pix[4];
        float w[4];
        bool in[4];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                in[2 * i + j] = replicate || ((unsigned)yi[i] < (unsigned)SH && (unsigned)xi[j] < (unsigned)SW);
                pix[2 * i + j] = ibase + (long)min(max(yi[i], 0), SH - 1) * SW + min(max(xi[j], 0), SW - 1);
                w[2 * i + j] = wy2[i] * wx2[j];
            }
        const int nxi = (int)floorf(sx + 0.5f) + ox, nyi = (int)floorf(sy + 0.5f) + oy;
        const bool nin = replicate || ((unsigned)nyi < (unsigned)SH && (unsigned)nxi < (unsigned)SW);
        const long npix = ibase + (long)min(max(nyi, 0), SH - 1) * SW + min(max(nxi, 0), SW - 1);
        uint8_t tap[4][3], mtap[4];
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
            for (int c = 0; c < 3; ++c) tap[k][c] = img[pix[k] * 3 + c];
#pragma unroll
        for (int k = 0; k < 4; ++k) mtap[k] = mask[bilinear_mask ? pix[k] : npix];
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
#pragma unroll
            for (int c = 0; c < 3; ++c) acc[c] += w[k] * (in[k] ? (float)tap[k][c] : a.fill);
            acc[3] += w[k] * (in[k] ? (float)mtap[k] : 0.f);
        }
        const float contrast = row[T_CONTRAST], bright = row[T_BRIGHT], gamma = row[T_GAMMA];
        const float sigma = rng ? row[T_SIGMA] : 0.f, mean = means[mi];
        float n[3] = {0.f, 0.f, 0.f};
        if (sigma > 0.f) {
            const uint4 v = draw4(load_snap(rng), (uint32_t)(y * W + x), b, a.site);
            const float r0 = sqrtf(-2.f * kLn2 * __log2f((float)((v.x >> 8) + 1u) * (1.f / 16777216.f)));
            const float r1 = sqrtf(-2.f * kLn2 * __log2f((float)((v.z >> 8) + 1u) * (1.f / 16777216.f)));
            const float t0 = u01(v.y), t1 = u01(v.w);                       // turns: v_sin / v_cos take revolutions
            n[0] = r0 * __builtin_amdgcn_cosf(t0);
            n[1] = r0 * __builtin_amdgcn_sinf(t0);
            n[2] = r1 * __builtin_amdgcn_cosf(t1);
        }
        const long opix = (long)y * W + x, plane = (long)H * W;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float v = acc[c] / 255.f;       // an IEEE division, as csu_augment_batch
            if (contrast != 1.f) v = (v - mean) * contrast + mean;
            if (bright != 1.f) v *= bright;
            v = fminf(fmaxf(v, 0.f), 1.f);
            if (gamma != 1.f) v = __builtin_amdgcn_exp2f(gamma * __log2f(v));      // v_exp_f32(gamma v_log_f32(v)); 0 stays 0
            if (sigma > 0.f) v = fminf(fmaxf(v + sigma * n[c], 0.f), 1.f);
            oimg[((long)b * 3 + c) * plane + opix] = v;
        }
        if (bilinear_mask) {
            ((float*)omask)[(long)b * plane + opix] = acc[3] / 255.f;
        } else {
            const int lab = nin ? (int)mtap[0] : a.pad_label;
            if (a.mask_mode == CSU_AUG_MASK_LABELS) ((long long*)omask)[(long)b * plane + opix] = lab;
            else ((float*)omask)[(long)b * plane + opix] = (float)lab / 255.f;
        }
    }
}

bool prob_ok(float p) { return p >= 0.f && p <= 1.f; }
bool range_ok(float lo, float hi, float least) { return lo >= least && hi >= lo; }

}  // namespace
}  // namespace csu

using namespace csu;

extern "C" int csu_augment_draw(const csu_augment_config* cfg, int B, int H, int W, const uint64_t* rng, unsigned site,
                                unsigned site_ctrl, float* table, float* ctrl, void* stream) {
    if (!cfg || B < 1 || B > (1 << 20) || H < 1 || W < 1 || !rng || !table || site >= 4096u || site_ctrl >= 4096u)
        return fail(CSU_E_ARG, "augment_draw: bad args");
    const csu_augment_config& c = *cfg;
    if (!(prob_ok(c.p_hflip) && prob_ok(c.p_vflip) && prob_ok(c.p_rot90) && prob_ok(c.p_rotate) && prob_ok(c.p_scale) &&
          prob_ok(c.p_translate) && prob_ok(c.p_contrast) && prob_ok(c.p_brightness) && prob_ok(c.p_gamma) &&
          prob_ok(c.p_noise) && prob_ok(c.p_elastic)))
        return fail(CSU_E_ARG, "augment_draw: a probability outside [0, 1]");
    if (!(c.rotate_hi >= c.rotate_lo && c.translate_x >= 0.f && c.translate_y >= 0.f && c.contrast_hi >= c.contrast_lo &&
          c.brightness_hi >= c.brightness_lo && range_ok(c.noise_lo, c.noise_hi, 0.f) &&
          range_ok(c.elastic_lo, c.elastic_hi, 0.f)) ||
        (c.p_scale > 0.f && !(c.scale_lo > 0.f && c.scale_hi >= c.scale_lo)) ||
        (c.p_gamma > 0.f && !(c.gamma_lo > 0.f && c.gamma_hi >= c.gamma_lo)))
        return fail(CSU_E_ARG, "augment_draw: an empty or illegal range");
    hipStream_t st = as_stream(stream);
    augment_draw_kernel<<<(B + NT - 1) / NT, NT, 0, st>>>(c, B, H, W, rng, site, table);
    if (ctrl) {
        if (c.spacing < MIN_SPACING) return fail(CSU_E_ARG, "augment_draw: control-grid spacing below 4");
        const long n = 2L * ((H + c.spacing - 1) / c.spacing + 3) * ((W + c.spacing - 1) / c.spacing + 3);
        if (n >= (1L << 31)) return fail(CSU_E_ARG, "augment_draw: control grid too large");
        const long g = ((long)B * ((n + 3) / 4) + NT - 1) / NT;
        augment_ctrl_kernel<<<(unsigned)(g > 4096 ? 4096 : g), NT, 0, st>>>(B, (int)n, rng, site_ctrl, table, ctrl);
    }
    return check_launch("augment_draw");
}

extern "C" int csu_augment_mean(int B, long n, const void* img, uint64_t* sums, float* mean, void* stream) {
    if (B < 1 || B > 65535 || n < 1 || !img || !sums || !mean) return fail(CSU_E_ARG, "augment_mean: bad args");
    hipStream_t st = as_stream(stream);
    hipError_t e = hipMemsetAsync(sums, 0, (size_t)B * sizeof(uint64_t), st);
    if (e != hipSuccess) return fail((int)e, std::string("augment_mean: ") + hipGetErrorString(e));
    long g = (n / 16 + NT * 4 - 1) / (NT * 4);     // ~4 vector loads per thread, at most 64 atomics per image
    g = g < 1 ? 1 : (g > 64 ? 64 : g);
    augment_sum_kernel<<<dim3((unsigned)g, (unsigned)B), NT, 0, st>>>(n, (const uint8_t*)img, (unsigned long long*)sums);
    augment_mean_kernel<<<(B + 63) / 64, 64, 0, st>>>(B, n, (const unsigned long long*)sums, mean);
    return check_launch("augment_mean");
}

extern "C" int csu_augment_warp(int B, int H, int W, const void* img, const void* mask, const float* table,
                                const float* ctrl, int spacing, const float* mean, const uint64_t* rng,
                                unsigned noise_site, int border, float image_fill, int pad_label, int mask_mode,
                                float* out_img, void* out_mask, void* stream) {
    if (B < 1 || B > (1 << 20) || H < 1 || W < 1 || (long)H * W >= (1L << 31) || !img || !mask || !table || !mean ||
        !out_img || !out_mask || noise_site >= 4096u)
        return fail(CSU_E_ARG, "augment_warp: bad args");
    if (ctrl && spacing < MIN_SPACING) return fail(CSU_E_ARG, "augment_warp: control-grid spacing below 4");
    if ((border != CSU_AUG_CONSTANT && border != CSU_AUG_REPLICATE) || mask_mode < CSU_AUG_MASK_BILINEAR ||
        mask_mode > CSU_AUG_MASK_LABELS || !(image_fill >= 0.f && image_fill <= 1.f))
        return fail(CSU_E_ARG, "augment_warp: bad border, mask mode or image_fill");
    const int ntx = (W + TX - 1) / TX, nty = (H + TY - 1) / TY;
    if (nty > 65535) return fail(CSU_E_ARG, "augment_warp: image too tall");
    WarpArgs a;
    a.B = B; a.H = H; a.W = W;
    a.site = noise_site;
    a.spacing = ctrl ? spacing : 0; a.border = border; a.mask_mode = mask_mode; a.pad_label = pad_label;
    a.fill = image_fill * 255.f;
    warp_kernel<false><<<dim3((unsigned)ntx, (unsigned)nty, (unsigned)(B > 65535 ? 65535 : B)), NT, 0, as_stream(stream)>>>(
        a, (const uint8_t*)img, (const uint8_t*)mask, table, ctrl, mean, rng, out_img, out_mask, nullptr, nullptr, 0);
    return check_launch("augment_warp");
}

extern "C" int csu_patch_warp(int B, int Ph, int Pw, int N, const void* pixels, const void* labels, const int64_t* meta,
                              const float* mean, const int32_t* record, const float* table, const float* ctrl, int spacing,
                              const uint64_t* rng, unsigned noise_site, int border, float image_fill, int pad_label,
                              int mask_mode, float* out_img, void* out_mask, void* stream) {
    if (B < 1 || B > (1 << 20) || Ph < 1 || Pw < 1 || (long)Ph * Pw >= (1L << 31) || N < 1 || N > (1 << 20) || !pixels ||
        !labels || !meta || !mean || !record || !table || !out_img || !out_mask || noise_site >= 4096u)
        return fail(CSU_E_ARG, "patch_warp: bad args");
    if (ctrl && spacing < MIN_SPACING) return fail(CSU_E_ARG, "patch_warp: control-grid spacing below 4");
    if ((border != CSU_AUG_CONSTANT && border != CSU_AUG_REPLICATE) || mask_mode < CSU_AUG_MASK_BILINEAR ||
        mask_mode > CSU_AUG_MASK_LABELS || !(image_fill >= 0.f && image_fill <= 1.f))
        return fail(CSU_E_ARG, "patch_warp: bad border, mask mode or image_fill");
    const int ntx = (Pw + TX - 1) / TX, nty = (Ph + TY - 1) / TY;
    if (nty > 65535) return fail(CSU_E_ARG, "patch_warp: patch too tall");
    WarpArgs a;
    a.B = B; a.H = Ph; a.W = Pw;
    a.site = noise_site;
    a.spacing = ctrl ? spacing : 0; a.border = border; a.mask_mode = mask_mode; a.pad_label = pad_label;
    a.fill = image_fill * 255.f;
    warp_kernel<true><<<dim3((unsigned)ntx, (unsigned)nty, (unsigned)(B > 65535 ? 65535 : B)), NT, 0, as_stream(stream)>>>(
        a, (const uint8_t*)pixels, (const uint8_t*)labels, table, ctrl, mean, rng, out_img, out_mask, (const long long*)meta,
        record, N);
    return check_launch("patch_warp");
}
