/* pretorched-x_amd: RandomErasing per clip and MixUp / CutMix across the clips of a batch, on the normalised clip, in one launch
 * (csrc/batch_mix.h), exported by the same libptx_amd.so.  A header of its own, like ptx_amd_randaug.h: ptx_amd.h is the census
 * of the drop-in contract as it stood before, this file adds to it. */
#ifndef PTX_AMD_MIX_H
#define PTX_AMD_MIX_H

#include "ptx_amd_randaug.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Every clip has one row of PTX_MIX_ROW int32 words.  With x_n the normalised value of clip n (the source element, or, from
 * uint8 frames, exactly ptx_frames_u8_to_ncdhw's value of the byte -- for bf16 output that value rounded once, as
 * PTX_RESIZE_OUT_BF16 writes it), E_n the erase of clip n (inside its rectangle, on every frame, output channel c takes the
 * constant c or the clip's noise element; outside it x_n), p the partner of clip i, (y, x) the pixel:
 *
 *   PTX_MIX_NONE    out_i = E_i(x_i)
 *   PTX_MIX_MIXUP   out_i = fadd(fmul(E_p(x_p), b), fmul(E_i(x_i), a))        fp32: three roundings, no FMA contraction
 *                   bf16:   bf16(float(bf16(E_p(x_p) * b)) + float(bf16(E_i(x_i) * a)))   (products and sum in fp32, each rounded)
 *                   which is torch's  E_p(x_p).mul(1.0 - lam).add_(E_i(x_i).mul(lam))  with a = fp32(lam), b = fp32(1.0 - lam)
 *   PTX_MIX_CUTMIX  out_i = E_p(x_p) where y0 <= y < y1 and x0 <= x < x1, else E_i(x_i); pure moves.  Outside the box the
 *                   partner's elements are not used, inside it the clip's own are not.
 *
 * Words of a row: */
#define PTX_MIX_W_PARTNER     0      /* clip index 0 .. N - 1 (read for MIXUP / CUTMIX only, checked always)               */
#define PTX_MIX_W_MODE        1      /* PTX_MIX_NONE / _MIXUP / _CUTMIX                                                      */
#define PTX_MIX_W_A           2      /* bits of the fp32 a = lam                                                             */
#define PTX_MIX_W_B           3      /* bits of the fp32 b = 1.0 - lam (subtracted in double, rounded once)                  */
#define PTX_MIX_W_BOX         4      /* y0, x0, y1, x1: the CutMix box, half open, 0 <= y0 <= y1 <= H, 0 <= x0 <= x1 <= W     */
#define PTX_MIX_W_ERASE       8      /* top, left, h, w: the erase rectangle, h, w >= 0, top + h <= H, left + w <= W          */
#define PTX_MIX_W_ERASE_KIND  12     /* PTX_MIX_ERASE_NONE / _CONST / _NOISE                                                 */
#define PTX_MIX_W_CONST       13     /* bits of three fp32 constants, one per OUTPUT channel (bf16 output rounds them once)  */
#define PTX_MIX_W_NOISE       16     /* low, high word of the clip's 64-bit element offset into the noise buffer             */
#define PTX_MIX_ROW           20     /* int32 words per clip (18, 19 reserved)                                               */

#define PTX_MIX_NONE          0
#define PTX_MIX_MIXUP         1
#define PTX_MIX_CUTMIX        2
#define PTX_MIX_ERASE_NONE    0
#define PTX_MIX_ERASE_CONST   1
#define PTX_MIX_ERASE_NOISE   2      /* the clip's noise is [3][T][h][w] elements of the output type at its offset            */

#define PTX_MIX_SRC_U8        0      /* uint8 frames [N][T][H][W][3], any byte alignment; needs the norm descriptor           */
#define PTX_MIX_SRC_F32       1      /* normalised fp32 clip [N][3][T][H][W], 4-byte aligned; out_mode PTX_RESIZE_OUT_F32     */
#define PTX_MIX_SRC_BF16      2      /* normalised bf16 clip [N][3][T][H][W], 2-byte aligned; out_mode PTX_RESIZE_OUT_BF16    */

typedef struct ptx_mix_desc {
    int32_t N, T, H, W;
    int32_t src_mode;                  /* PTX_MIX_SRC_*                                                            */
    int32_t out_mode;                  /* PTX_RESIZE_OUT_F32 / PTX_RESIZE_OUT_BF16; the output is [N][3][T][H][W]  */
    int64_t noise_elems;               /* elements in the noise buffer (0: none)                                   */
} ptx_mix_desc;

/* Host-side check, no device needed: the descriptor and a HOST copy of the rows.  1 when the launch accepts them, else 0 with
 * ptx_last_error(): a null pointer, a non-positive extent, a source / output mode out of range or a normalised source whose
 * output is not its own type, a partner or a mode code or an erase kind out of range, a box or an erase rectangle outside the
 * frame or with a negative extent, a lam (a or b) that is not finite or outside [0, 1], a noise offset whose [3][T][h][w]
 * block does not lie inside the noise buffer. */
int ptx_batch_mix_supported(const ptx_mix_desc* desc, const int32_t* rows_host);
/* One launch.  rows: DEVICE int32 [N][PTX_MIX_ROW]; noise: DEVICE elements of the output type (may be null when noise_elems is
 * 0); y must not overlap src.  The descriptor is checked as above (not the rows: check them with ptx_batch_mix_supported
 * first); nothing is launched when the call returns a status. */
int ptx_batch_mix_apply(const ptx_mix_desc* desc, const void* src, const int32_t* rows, const void* noise, void* y,
                        const ptx_norm_desc* norm, ptx_stream_t stream);
/* Soft targets y fp32 [N][K] of int64 labels [N] (DEVICE arrays; a label outside 0 .. K - 1 gives a row of `off`): with
 * r_n[k] = (k == labels[n] ? on : off), NONE writes r_i, MIXUP and CUTMIX write fadd(fmul(r_p, b), fmul(r_i, a)). */
int ptx_batch_mix_targets(const int64_t* labels, const int32_t* rows, float* y, int32_t N, int32_t K, float off, float on,
                          ptx_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif  /* PTX_AMD_MIX_H */
