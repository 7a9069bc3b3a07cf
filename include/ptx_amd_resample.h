/* pretorched-x_amd: Pillow's other resize filters (Image.NEAREST, BOX, BILINEAR, HAMMING, BICUBIC, LANCZOS) on the resize
 * entry points of ptx_amd.h / ptx_amd_yuv16.h, exported by the same libptx_amd.so.  A header of its own, like
 * ptx_amd_randaug.h: ptx_amd.h is the census of the drop-in contract as it stood before, this file adds to it.
 *
 * The resize kernels apply whatever integer tap tables they are given, so a filter is a different TABLE, never a different
 * kernel: every ptx_resize_frames_*, ptx_resize_views_* and ptx_resize_clips_* call takes the tables of any filter.  What
 * a table may hold, for every one of those entry points:
 *   - row_k / col_k MAY BE NEGATIVE (bicubic, Lanczos and Hamming have negative lobes).  Both passes compute
 *       out = clip8((2^21 + sum_j k[j] * in[lo + j]) >> 22)        with an ARITHMETIC shift: a negative sum gives 0;
 *   - every |k| < 2^23                      (the kernels multiply with 24-bit integer multiplies);
 *   - per entry 255 * sum_j |k[j]| + 2^21 < 2^31   (the 32-bit accumulator cannot wrap).
 * Pillow's own tables keep far inside both bounds (the largest sum |k| of any filter is about 1.55 * 2^22).  The kernels do
 * not check the bounds (a table that breaks them gives wrong pixels, never a stray access); the Python layer checks every
 * table it builds or is given.
 * PIL's Image.NEAREST is a table too: one tap of 2^22 per output index, at the index of PIL's affine walk (below). */
#ifndef PTX_AMD_RESAMPLE_H
#define PTX_AMD_RESAMPLE_H

#include "ptx_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Pillow's filter codes (Image.Resampling) */
#define PTX_RESAMPLE_NEAREST   0
#define PTX_RESAMPLE_LANCZOS   1
#define PTX_RESAMPLE_BILINEAR  2
#define PTX_RESAMPLE_BICUBIC   3
#define PTX_RESAMPLE_BOX       4
#define PTX_RESAMPLE_HAMMING   5
#define PTX_RESAMPLE_NEAREST_MAX_EXTENT 65536  /* NEAREST: a resized extent (h, w of a row) is clamped to this: the walk's length */

/* ptx_resize_build_tables / ptx_resize_build_tables_clips for a filter: the same arguments, meaning of a geometry row, clamps
 * of a garbage row and table layout; `filter` is a PTX_RESAMPLE_* code.  Per axis, in IEEE fp64 without contraction and in the
 * host builder's operation order (transforms.resize_axis_table), so an entry has that builder's bits:
 *   an axis with box extent == resized extent is not resampled, for every filter: one tap of 2^22;
 *   BOX / BILINEAR / BICUBIC  PIL's precompute_coeffs + normalize_coeffs_8bpc as stated at ptx_resize_build_tables, with
 *       support = 0.5 / 1 / 2 * fs in place of fs in lo and hi, and the filter's weight of x = (j + lo - center + 0.5) * ss:
 *         BOX       1 if -0.5 < x <= 0.5, else 0
 *         BILINEAR  1 - |x| (0 if not positive)
 *         BICUBIC   with x = |x|, a = -0.5:  ((a + 2) x - (a + 3)) x x + 1  if x < 1,   (((x - 5) x + 8) x - 4) a  if x < 2,  else 0
 *       k_j = (int)(w_j * 4194304.0 + 0.5) for w_j >= 0 and (int)(-0.5 + w_j * 4194304.0) for w_j < 0;
 *       the pitches: n <= 2 * ceil(support) + 1;
 *   NEAREST   PIL's affine walk (ImagingScaleAffine): a = n_in / n_out, xo = a * 0.5, then index i of the resized box is
 *       (int)xo after i sequential additions xo += a -- a window that starts at s costs s additions, not a multiply, because
 *       the sum is not the product in the last bit --, clamped to the box; one tap of 2^22 there;
 *   BILINEAR writes exactly what ptx_resize_build_tables writes.
 * HAMMING / LANCZOS return PTX_ERR_UNSUPPORTED: their weights are sin / cos of the C library on the host, which the device's
 * fp64 sin / cos cannot be promised to equal bit for bit.  Their tables are built on the host (one per frame size, cached)
 * and serve every entry point that takes host tables. */
int ptx_resize_build_tables_filter(const ptx_resize_desc* desc, const ptx_resize_geom* geoms, int32_t filter,
                                   int32_t* row_lo, int32_t* row_n, int32_t* row_k, /* [N][Ho], [N][Ho], [N][Ho][taps_h] */
                                   int32_t* col_lo, int32_t* col_n, int32_t* col_k, /* [N][Wo], [N][Wo], [N][Wo][taps_w] */
                                   ptx_stream_t stream);
int ptx_resize_build_tables_clips_filter(const ptx_resize_desc* desc, const ptx_clip_src* srcs, const ptx_resize_geom* geoms,
                                         int32_t filter, int32_t* row_lo, int32_t* row_n, int32_t* row_k,
                                         int32_t* col_lo, int32_t* col_n, int32_t* col_k, ptx_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif  /* PTX_AMD_RESAMPLE_H */
