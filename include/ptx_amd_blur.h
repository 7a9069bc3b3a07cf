/* pretorched-x_amd: per-clip GaussianBlur of decoded uint8 frames on the device (csrc/blur_frames.h), exported by the same
 * libptx_amd.so: the blur of the contrastive / self-distillation view recipes (SimCLR, MoCo, BYOL and their video forms),
 * torchvision's GaussianBlur on a PIL / uint8 image.  A header of its own, like ptx_amd_color.h and ptx_amd_warp.h: ptx_amd.h
 * is the census of the drop-in contract as it stood before, this file adds to it. */
#ifndef PTX_AMD_BLUR_H
#define PTX_AMD_BLUR_H

#include "ptx_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Every clip has an apply flag and two rows of fp32 weights, wx[kx] and wy[ky] (built on the host: torchvision's
 * exp(-0.5 (x / sigma)^2) / sum on linspace(-(k - 1) / 2, (k - 1) / 2, k), so one sigma per clip; the launch takes any
 * non-negative finite weights).  Per frame and per channel, on bytes p, with rx = kx / 2, ry = ky / 2 and
 *     refl(i, n) = i < 0 ? -i : i >= n ? 2 (n - 1) - i : i            (torch's "reflect" padding: needs rx < W and ry < H)
 *   h[y][x] = sum over j = 0 .. kx - 1, in this order, from 0.0, of  (double)wx[j] * p[y][refl(x + j - rx, W)]
 *   v[y][x] = sum over i = 0 .. ky - 1, in this order, from 0.0, of  (double)wy[i] * h[refl(y + i - ry, H)][x]
 *   out     = clamp(round_half_to_even(v), 0, 255)
 * All arithmetic is IEEE fp64.  Every product of the first sum is exact (24 x 8 bits); in the second sum the product and the add
 * are two roundings (no fused multiply-add).  The order is fixed, so the result is a pure function of the inputs.  A clip whose
 * apply flag is 0 is copied byte for byte (its weights are not read).
 * torchvision computes the same real number as one fp32 depthwise conv2d with the outer-product kernel and rounds it the same
 * way: it can differ by one level where v lies within fp32 summation error of a half-integer. */
#define PTX_BLUR_MAX_TAPS 33

/* frames: contiguous uint8 [N][T][H][W][3], any byte alignment.  out_mode: PTX_RESIZE_OUT_U8 writes uint8 [N][T][H][W][3] (any
 * alignment); PTX_RESIZE_OUT_F32 / PTX_RESIZE_OUT_BF16 write the normalised clip [N][3][T][H][W] (4- / 2-byte aligned), every
 * value exactly what ptx_frames_u8_to_ncdhw / PTX_RESIZE_OUT_BF16 make of the blurred byte.  kx, ky: odd tap counts 1 ..
 * PTX_BLUR_MAX_TAPS of the horizontal and the vertical pass. */
typedef struct ptx_blur_desc {
    int32_t N, T, H, W;
    int32_t kx, ky;
    int32_t out_mode;
} ptx_blur_desc;

/* Host-side check, no device needed: the descriptor and HOST copies of the flags ([N]) and the weights ([N][kx], [N][ky]).  1
 * when the launch accepts them, else 0 with ptx_last_error(): a null pointer, a non-positive extent, a tap count that is even,
 * non-positive or above PTX_BLUR_MAX_TAPS, kx / 2 >= W or ky / 2 >= H (reflect padding is not defined), a flag that is not 0 or
 * 1, a weight that is negative or not finite, an unknown out_mode, a frame of 2^31 bytes or more or N, T beyond the grid. */
int ptx_gaussian_blur_supported(const ptx_blur_desc* desc, const int32_t* apply_host, const float* wx_host, const float* wy_host);
/* One launch.  apply / wx / wy are DEVICE arrays (4-byte aligned).  The descriptor is checked as above (not the rows: check them
 * with ptx_gaussian_blur_supported first) and y == frames is refused (y must not overlap frames); nothing is launched when the
 * call returns a status.  A row that the check refuses cannot make the kernel read or write out of bounds.  norm is read for
 * the two normalised outputs only. */
int ptx_gaussian_blur_frames(const ptx_blur_desc* desc, const uint8_t* frames, const int32_t* apply, const float* wx,
                             const float* wy, void* y, const ptx_norm_desc* norm, ptx_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif  /* PTX_AMD_BLUR_H */
