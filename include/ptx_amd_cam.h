/* pretorched-x_amd: class activation maps (Zhou et al., CVPR 2016) of the networks that end in global average pool + one
 * Linear, and their overlay on decoded uint8 frames (csrc/cam.h), exported by the same libptx_amd.so.  For that head the map of
 * class c is the classifier row applied at every position of the final feature map; its mean over the positions is the logit.
 * A header of its own, like ptx_amd_color.h and ptx_amd_blur.h: ptx_amd.h is the census of the drop-in contract as it stood
 * before, this file adds to it. */
#ifndef PTX_AMD_CAM_H
#define PTX_AMD_CAM_H

#include "ptx_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PTX_CAM_MAX_CLASSES 8      /* class rows of one ptx_cam_scores launch (they live in LDS)            */
#define PTX_CAM_MAX_LDS_BYTES 65536 /* k * C * 4 of a launch: 8 rows of 2048 channels                        */

/* 1. Class scores at every position.
 *   x   channels-last feature map [N][S][ld] (S = T' * H' * W'), fp32 (x_bf16 == 0; 4-byte aligned) or bf16 (x_bf16 != 0; 16-byte
 *       aligned rows: ld % 8 == 0).  Channels [C, ld) are never read.
 *   w   fp32 [classes][C], b fp32 [classes] or NULL.
 *   cls DEVICE int32 [N][k], 1 <= k <= PTX_CAM_MAX_CLASSES: a class list of its own per clip, repeats allowed.  An index outside
 *       [0, classes) is clamped into it: a wrong list gives a wrong map, never a stray access.
 *   y   fp32 [N][k][S]:  y[n][j][s] = b[cls[n][j]] + sum_c w[cls[n][j]][c] * x[n][s][c], accumulated in fp32 (bf16 features are
 *       widened exactly; the summation order is the kernel's own).
 * Any C >= 1 and S >= 1; the offset of a clip is 64-bit.  _supported needs no device: 1 when the launch takes these extents, else 0
 * with ptx_last_error() (a non-positive extent, ld < C, bf16 with ld % 8 != 0, k outside 1 .. PTX_CAM_MAX_CLASSES, k * C * 4 above
 * PTX_CAM_MAX_LDS_BYTES, a clip of 2^31 elements or more, N or S beyond the grid). */
int ptx_cam_scores_supported(int32_t N, int64_t S, int32_t C, int32_t ld, int32_t k, int32_t classes, int32_t x_bf16);
int ptx_cam_scores(const void* x, int32_t x_bf16, const float* w, const float* b, const int32_t* cls, float* y,
                   int32_t N, int64_t S, int32_t C, int32_t ld, int32_t k, int32_t classes, ptx_stream_t stream);

/* 2. One uint8 map per row of scores.  scores fp32 [maps][S] -> q uint8 [maps][S]: with mn / mx the smallest / largest score of the
 * row that is not a NaN,
 *   v = 255.0f * ((s - mn) / (mx - mn))        every operation rounded to fp32 (IEEE division)
 *   q = v >= 255 ? 255 : v > 0 ? (uint8)v : 0  truncation; a NaN (a NaN score, inf - inf) gives 0
 * and a flat row (mx == mn, or no score that is not a NaN) gives all zeros.  Minimum and maximum are exact in any order, so q is a
 * pure function of the scores. */
int ptx_cam_quantize(const float* scores, uint8_t* q, int64_t maps, int64_t S, ptx_stream_t stream);

/* 3. Overlay: every frame gets its map, resized as Pillow resizes an "L" image with BILINEAR, coloured and blended in.
 *   q      uint8 [N][k][Tm][h][w], the maps (Tm time steps)
 *   frames uint8 [N][T][H][W][3], any byte alignment (not read in the heat and map modes: may be NULL)
 *   lut    uint8 [256][3], the colour of every level
 *   row_* / col_*  the tables of ptx_resize_frames_u8 (2^22 fixed point) for h -> H ([H], [H], [H][taps_h]) and w -> W ([W], [W],
 *          [W][taps_w]), DEVICE arrays
 *   step   DEVICE int32 [T]: frame t shows time step step[t] of the maps (clamped into [0, Tm))
 * Per output pixel (Y, X) of frame t of clip n and class j, with m = q[n][j][step[t]]:
 *   mid[y][X] = clip8((2^21 + sum_i col_k[X][i] * m[y][col_lo[X] + i]) >> 22)       horizontal pass, uint8 intermediate
 *   v         = clip8((2^21 + sum_i row_k[Y][i] * mid[row_lo[Y] + i][X]) >> 22)     vertical pass
 *   heat      = lut[v]
 *   out[c]    = PTX_CAM_OUT_OVERLAY: Image.blend(frame, heat, alpha): t = (float)f + alpha * (float)(heat[c] - f), the product and
 *               the sum rounded to fp32 one by one; 0 if t <= 0, 255 if t >= 255, else (uint8)t
 *               PTX_CAM_OUT_HEAT: heat[c]          PTX_CAM_OUT_MAP: v itself, one byte per pixel
 * y: uint8 [N][k][T][H][W][3] (overlay, heat) or [N][k][T][H][W] (map), any alignment.  Table entries are clamped to the map as
 * everywhere: a wrong table gives wrong pixels, never a stray access.  A workgroup stages its map and the map's horizontal pass
 * in LDS once: h * (w + W) bytes, at most PTX_CAM_MAX_MAP_BYTES. */
#define PTX_CAM_OUT_OVERLAY 0
#define PTX_CAM_OUT_HEAT 1
#define PTX_CAM_OUT_MAP 2
#define PTX_CAM_MAX_MAP_BYTES 40960
typedef struct ptx_cam_overlay_desc {
    int32_t N, k, Tm, h, w;      /* the maps                        */
    int32_t T, H, W;             /* the frames                      */
    int32_t taps_h, taps_w;      /* row pitch of row_k / col_k      */
    int32_t mode;                /* PTX_CAM_OUT_*                   */
    float alpha;                 /* 0 .. 1, read by the overlay mode */
} ptx_cam_overlay_desc;
/* Host-side check, no device needed: the descriptor and, when they are not NULL, HOST copies of row_k / col_k.  1 when the launch
 * accepts them, else 0 with ptx_last_error(): a non-positive extent, a tap count outside 1 .. PTX_RESIZE_MAX_TAPS (strong
 * down-sampling of a large map), a map whose staging exceeds PTX_CAM_MAX_MAP_BYTES, an unknown mode, alpha outside [0, 1] (or NaN),
 * an output of 2^31 bytes or more (the caller then launches ranges of (n, j)), a frame of 2^31 bytes or more, a coefficient with
 * |k| >= 2^23 or an entry with 255 * sum|k| + 2^21 >= 2^31. */
int ptx_cam_overlay_supported(const ptx_cam_overlay_desc* desc, const int32_t* row_k_host, const int32_t* col_k_host);
int ptx_cam_overlay(const ptx_cam_overlay_desc* desc, const uint8_t* q, const uint8_t* frames, const uint8_t* lut,
                    const int32_t* row_lo, const int32_t* row_n, const int32_t* row_k,
                    const int32_t* col_lo, const int32_t* col_n, const int32_t* col_k,
                    const int32_t* step, uint8_t* y, ptx_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif  /* PTX_AMD_CAM_H */
