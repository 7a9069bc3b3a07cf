/* pretorched-x_amd: per-clip RandAugment of decoded uint8 frames on the device, equal to torchvision's RandAugment on its
 * PIL-image code path (nearest interpolation) bit for bit (csrc/rand_augment.h), exported by the same libptx_amd.so.  A header
 * of its own, like ptx_amd_color.h: ptx_amd.h is the census of the drop-in contract as it stood before, this file adds to it. */
#ifndef PTX_AMD_RANDAUG_H
#define PTX_AMD_RANDAUG_H

#include "ptx_amd_color.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Every clip has `num_ops` POSITIONS, run in order; a position is one row of PTX_RANDAUG_ROW int32 words: the op code and up to
 * six arguments.  One call of ptx_rand_augment_apply runs ONE position on every frame of every clip, reading uint8 frames and
 * writing uint8 frames (the caller ping-pongs two buffers) or, at the last position, the requested output.  With L and blend of
 * ptx_amd_color.h, on the frame as it stands at that position (H x W pixels, (x, y) the output pixel):
 *
 *   IDENTITY      the frame
 *   SHEAR_X .. ROTATE   words 1..6 hold a0 .. a5, PIL's 16.16 fixed-point affine walk (Geometry.c, nearest):
 *                 xin = (a2 + a1 * y + a0 * x) >> 16,  yin = (a5 + a4 * y + a3 * x) >> 16   (32-bit wrap-around sums, arithmetic
 *                 shift); the pixel is in(xin, yin) when 0 <= xin < W and 0 <= yin < H, else the fill colour.  From the six
 *                 coefficients m0..m5 of Image.transform(AFFINE):  FIX(v) = floor(v * 65536 + 0.5),  a0, a1, a3, a4 = FIX(m0),
 *                 FIX(m1), FIX(m3), FIX(m4),  a2 = FIX(m2 + m0 * 0.5 + m1 * 0.5),  a5 = FIX(m5 + m3 * 0.5 + m4 * 0.5).
 *   BRIGHTNESS    c = blend(0, c, f)                          word 1 holds the bits of the fp32 factor f (here and below)
 *   COLOR         c = blend(L(pixel), c, f)
 *   CONTRAST      c = blend(m, c, f),   m = int(sum_L / (H * W) + 0.5) in fp64, sum_L the integer sum of L over THAT FRAME
 *   SHARPNESS     c = blend(smooth(c), c, f);  smooth is ImageFilter.SMOOTH: an interior pixel is (2 * S + 13) / 26 (integer
 *                 division), S = the sum of the channel over the 3 x 3 neighbourhood + 4 * the centre; the pixels of the first
 *                 and last row and column -- every pixel when H < 3 or W < 3 -- are copied
 *   POSTERIZE     c = c & mask                                word 1 holds the mask, ~(2^(8 - bits) - 1) & 255
 *   SOLARIZE      c = c < thr ? c : 255 - c                   word 1 holds the bits of the fp32 threshold thr
 *   AUTOCONTRAST  c = lut_ch[c], per channel from THAT FRAME's 256-bin histogram h of the channel: lo / hi the lowest / highest
 *                 non-empty bin; hi <= lo leaves the channel as it is; else, in fp64 without FMA, scale = 255.0 / (hi - lo),
 *                 offset = -lo * scale, lut[i] = clip8(trunc(i * scale + offset))
 *   EQUALIZE      c = lut_ch[c]: with `last` the highest non-empty bin, step = (H * W - h[last]) / 255 (integer); fewer than two
 *                 non-empty bins or step == 0 leave the channel as it is; else lut[i] = min(255, (step / 2 + h[0] + .. +
 *                 h[i - 1]) / step)
 *
 * Words that an op does not use are ignored. */
#define PTX_RANDAUG_IDENTITY      0
#define PTX_RANDAUG_SHEAR_X       1
#define PTX_RANDAUG_SHEAR_Y       2
#define PTX_RANDAUG_TRANSLATE_X   3
#define PTX_RANDAUG_TRANSLATE_Y   4
#define PTX_RANDAUG_ROTATE        5
#define PTX_RANDAUG_BRIGHTNESS    6
#define PTX_RANDAUG_COLOR         7
#define PTX_RANDAUG_CONTRAST      8
#define PTX_RANDAUG_SHARPNESS     9
#define PTX_RANDAUG_POSTERIZE     10
#define PTX_RANDAUG_SOLARIZE      11
#define PTX_RANDAUG_AUTOCONTRAST  12
#define PTX_RANDAUG_EQUALIZE      13
#define PTX_RANDAUG_NUM_CODES     14
#define PTX_RANDAUG_MAX_OPS       4
#define PTX_RANDAUG_ROW           8      /* int32 words per (clip, position): code, six arguments, one reserved          */
#define PTX_RANDAUG_STATS_WORDS   770    /* uint32 words per frame: 3 x 256 bins (R, G, B), then the 64-bit luma sum      */

/* frames: contiguous uint8 [N][T][H][W][3], any byte alignment.  out_mode: PTX_RESIZE_OUT_U8 writes uint8 [N][T][H][W][3]
 * (any alignment); PTX_RESIZE_OUT_F32 / PTX_RESIZE_OUT_BF16 write the normalised clip [N][3][T][H][W] (4- / 2-byte
 * aligned), every value exactly what ptx_frames_u8_to_ncdhw / PTX_RESIZE_OUT_BF16 make of the augmented byte.
 * rows: int32 [N][num_ops][PTX_RANDAUG_ROW]; `position` selects the row of every clip that this call runs.
 * stats: non-zero iff some clip's op at `position` is CONTRAST, AUTOCONTRAST or EQUALIZE; then ptx_rand_augment_stats runs
 * before ptx_rand_augment_apply on the same frames and stream and both take `stats` (N * T * PTX_RANDAUG_STATS_WORDS uint32,
 * 8-byte aligned; the statistics call zeroes it itself and fills the frames of the clips that need it). */
typedef struct ptx_randaug_desc {
    int32_t N, T, H, W;
    int32_t out_mode;                  /* PTX_RESIZE_OUT_*                                                         */
    int32_t num_ops;                   /* positions per clip, 1 .. PTX_RANDAUG_MAX_OPS                             */
    int32_t position;                  /* the position this call runs, 0 .. num_ops - 1                            */
    int32_t stats;                     /* does any clip's op at `position` need the frame statistics               */
    int32_t fill_r, fill_g, fill_b;    /* what a geometric op writes where it has no source pixel, 0 .. 255 each   */
    int32_t reserved;
} ptx_randaug_desc;

/* Host-side check, no device needed: the descriptor and a HOST copy of the rows.  1 when the launches accept them, else 0
 * with ptx_last_error(): a null pointer, extents, num_ops / position / fill out of range, an op code out of range, a factor
 * that is negative or not finite, a posterize mask outside 0..255, a geometric row that leaves PIL's fixed-point range (a
 * source coordinate of a frame corner beyond +-32768), `stats` not matching the rows at `position`. */
int ptx_rand_augment_supported(const ptx_randaug_desc* desc, const int32_t* rows_host);
/* rows / stats are DEVICE arrays from here on. */
int ptx_rand_augment_stats(const ptx_randaug_desc* desc, const uint8_t* frames, const int32_t* rows, uint32_t* stats,
                           ptx_stream_t stream);
int ptx_rand_augment_apply(const ptx_randaug_desc* desc, const uint8_t* frames, const int32_t* rows, const uint32_t* stats,
                           void* y, const ptx_norm_desc* norm, ptx_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif  /* PTX_AMD_RANDAUG_H */
