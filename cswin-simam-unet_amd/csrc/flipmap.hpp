// The eight flip / quarter-turn variants of a square S x S image, shared by the training augmentation
// (augment.hip) and the tiled inference kernels (tile.hip): R = rot(vflip(hflip(I))), rot = clockwise
// quarter turns applied after the flips.
#pragma once
#include <hip/hip_runtime.h>

namespace csu {

// pixel (y, x) of the rotated/flipped square image -> pixel of the stored image
__device__ __forceinline__ void src_of(int S, int hflip, int vflip, int rot, int y, int x, int* sy, int* sx) {
    // inverse rotation (rot = clockwise quarter turns applied after the flips)
    int a = y, b = x;
    if (rot == 1) { a = S - 1 - x; b = y; }          // R[y][x] = F[S-1-x][y]   (90 clockwise)
    else if (rot == 2) { a = S - 1 - y; b = S - 1 - x; }
    else if (rot == 3) { a = x; b = S - 1 - y; }     // R[y][x] = F[x][S-1-y]   (90 counter-clockwise)
    // inverse flips: F = vflip(hflip(I))
    if (vflip) a = S - 1 - a;
    if (hflip) b = S - 1 - b;
    *sy = a;
    *sx = b;
}

// the inverse of src_of: pixel (sy, sx) of the stored image -> the pixel (y, x) of the rotated/flipped
// image that shows it
__device__ __forceinline__ void dst_of(int S, int hflip, int vflip, int rot, int sy, int sx, int* y, int* x) {
    const int a = vflip ? S - 1 - sy : sy, b = hflip ? S - 1 - sx : sx;   // pixel of F
    int p = a, q = b;
    if (rot == 1) { p = b; q = S - 1 - a; }
    else if (rot == 2) { p = S - 1 - a; q = S - 1 - b; }
    else if (rot == 3) { p = S - 1 - b; q = a; }
    *y = p;
    *x = q;
}

}  // namespace csu
