/* pretorched-x_amd: interpolated per-clip warps of decoded uint8 frames on the device -- affine (shear, translate, scale,
 * rotate) and perspective, with Pillow's bilinear or bicubic interpolation (and nearest, for a perspective) --, equal to
 * Pillow's Image.transform bit for bit (csrc/warp_frames.h), exported by the same libptx_amd.so.  A header of its own, like
 * ptx_amd_randaug.h and ptx_amd_mix.h: ptx_amd.h is the census of the drop-in contract as it stood before, this file adds to it. */
#ifndef PTX_AMD_WARP_H
#define PTX_AMD_WARP_H

#include "ptx_amd_resample.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Every clip has a KIND and a row of eight fp64 coefficients a0 .. a7; one call of ptx_warp_frames warps every frame of every
 * clip, reading uint8 frames and writing uint8 frames.  The arithmetic is Pillow's generic transform (Geometry.c): for output
 * pixel (x, y) of an H x W frame, all in IEEE fp64, every operation rounded, none contracted, in exactly this order:
 *
 *   X = x + 0.5,  Y = y + 0.5
 *   IDENTITY      the frame (copied; the coefficients are not read)
 *   AFFINE        xin = a0 * X + a1 * Y + a2                             yin = a3 * X + a4 * Y + a5            (a6, a7 not read)
 *   PERSPECTIVE   xin = (a0 * X + a1 * Y + a2) / (a6 * X + a7 * Y + 1)   yin = (a3 * X + a4 * Y + a5) / (a6 * X + a7 * Y + 1)
 *
 *   NEAREST (PERSPECTIVE only, see below):
 *       xi = xin < 0 ? -1 : (int)xin, yi the same;  out = in(xi, yi) when 0 <= xi < W and 0 <= yi < H, else the fill colour
 *   BILINEAR / BICUBIC:
 *       xin < 0 or xin >= W or yin < 0 or yin >= H gives the fill colour (tested BEFORE the shift);  then
 *       xin -= 0.5, yin -= 0.5, xi = floor(xin), yi = floor(yin), dx = xin - xi, dy = yin - yi,  clamp(i) = min(max(i, 0), extent - 1)
 *   BILINEAR, per channel:
 *       row(r) = in[r][x0] + (in[r][x1] - in[r][x0]) * dx   with x0 = clamp(xi), x1 = clamp(xi + 1)
 *       v1 = row(clamp(yi));  v2 = row(yi + 1) when 0 <= yi + 1 < H, else v1;  out = (uint8)trunc(v1 + (v2 - v1) * dy)
 *   BICUBIC, per channel:
 *       xi -= 1, yi -= 1;  cub(v1, v2, v3, v4, d) = p1 + d * (p2 + d * (p3 + d * p4))  with  p1 = v2,  p2 = -v1 + v3,
 *       p3 = 2 * (v1 - v2) + v3 - v4,  p4 = -v1 + v2 - v3 + v4;
 *       cubrow(r) = cub(in[r][clamp(xi)], in[r][clamp(xi + 1)], in[r][clamp(xi + 2)], in[r][clamp(xi + 3)], dx)
 *       r1 = cubrow(clamp(yi));  r2 = cubrow(yi + 1) when 0 <= yi + 1 < H, else r1;  r3 = cubrow(yi + 2) when 0 <= yi + 2 < H,
 *       else r2;  r4 = cubrow(yi + 3) when 0 <= yi + 3 < H, else r3;  v = cub(r1, r2, r3, r4, dy);
 *       out = 0 when v <= 0, 255 when v >= 255, else (uint8)trunc(v)
 *
 * The fill colour is what PIL puts in the new image before the transform writes to it.  A source coordinate that is not a
 * number gives the fill colour.  NEAREST with an AFFINE kind is not offered here: PIL walks a nearest affine transform in 16.16
 * fixed point, which is a geometric row of ptx_rand_augment_apply (ptx_amd_randaug.h). */
#define PTX_WARP_IDENTITY     0
#define PTX_WARP_AFFINE       1
#define PTX_WARP_PERSPECTIVE  2
#define PTX_WARP_COEFFS       8      /* doubles per clip: a0 .. a7 */

/* frames, y: contiguous uint8 [N][T][H][W][3], any byte alignment; y must not overlap frames.
 * kinds: int32 [N];  coeffs: double [N][PTX_WARP_COEFFS], 8-byte aligned. */
typedef struct ptx_warp_desc {
    int32_t N, T, H, W;
    int32_t filter;                    /* PTX_RESAMPLE_NEAREST, PTX_RESAMPLE_BILINEAR or PTX_RESAMPLE_BICUBIC              */
    int32_t fill_r, fill_g, fill_b;    /* what a pixel without a source takes, 0 .. 255 each                               */
    int32_t reserved;
} ptx_warp_desc;

/* Host-side check, no device needed: the descriptor and HOST copies of the kinds and the coefficients.  1 when the launch
 * accepts them, else 0 with ptx_last_error(): a null pointer, a non-positive extent, a frame of 2^31 bytes or more or N, T
 * beyond the grid, a filter that is not one of the three, a fill out of range, a kind out of range, NEAREST with an AFFINE
 * kind, a coefficient (a0 .. a5 of an AFFINE, a0 .. a7 of a PERSPECTIVE clip) that is not finite, a PERSPECTIVE row whose
 * denominator a6 * X + a7 * Y + 1 does not have the same strict sign at the four corner pixel centres (the denominator is
 * monotonic in X and in Y, so it is then non-zero on the whole frame). */
int ptx_warp_frames_supported(const ptx_warp_desc* desc, const int32_t* kinds_host, const double* coeffs_host);
/* One launch.  kinds / coeffs are DEVICE arrays.  The descriptor is checked as above (not the rows: check them with
 * ptx_warp_frames_supported first); nothing is launched when the call returns a status.  A row that the check refuses cannot
 * make the kernel read or write out of bounds: a kind out of range copies the clip, a NEAREST AFFINE clip takes the NEAREST
 * rule above on its fp64 coordinates (not PIL's bits). */
int ptx_warp_frames(const ptx_warp_desc* desc, const uint8_t* frames, const int32_t* kinds, const double* coeffs, uint8_t* y,
                    ptx_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif  /* PTX_AMD_WARP_H */
