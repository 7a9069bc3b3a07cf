/* pretorched-x_amd: per-clip ColorJitter / RandomGrayscale of decoded uint8 frames on the device, equal to Pillow's
 * ImageEnhance / convert("L") / HSV arithmetic bit for bit (csrc/color_jitter.h), exported by the same libptx_amd.so.  The
 * entry points live in a header of their own, like ptx_amd_wino4.h, ptx_amd_tfir.h and ptx_amd_yuv16.h: ptx_amd.h is the
 * census of the drop-in contract as it stood before them, this file adds to it. */
#ifndef PTX_AMD_COLOR_H
#define PTX_AMD_COLOR_H

#include "ptx_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Every clip has an ordered list of PTX_COLOR_MAX_OPS entries: an op code and an fp32 factor.  PTX_COLOR_NONE entries are
 * skipped; every other code appears at most once per clip.  On one RGB pixel (r, g, b), with
 *     L(r, g, b)     = (r * 19595 + g * 38470 + b * 7471 + 0x8000) >> 16
 *     blend(d, x, f) = t <= 0 ? 0 : t >= 255 ? 255 : trunc(t),   t = fp32(d) + fp32(f * fp32(x - d))    (no FMA)
 *   BRIGHTNESS  c = blend(0, c, f)                         per channel
 *   SATURATION  c = blend(L(pixel), c, f)                  per channel
 *   CONTRAST    c = blend(m, c, f),  m = int(sum_L / (H * W) + 0.5) in fp64, sum_L the integer sum of L over THAT FRAME as
 *               it stands when contrast is applied (after the entries in front of it)
 *   HUE         RGB -> HSV bytes (fp32 divisions, PIL's rgb2hsv), H = (H + shift) & 255, HSV -> RGB (fp64, PIL's hsv2rgb);
 *               the factor holds the integer shift 0..255 (trunc(hue_factor * 255) mod 256); a shift of 0 still runs the
 *               (lossy) round trip
 *   GRAYSCALE   (L, L, L)
 * Factors of BRIGHTNESS / CONTRAST / SATURATION are finite and >= 0. */
#define PTX_COLOR_NONE        0
#define PTX_COLOR_BRIGHTNESS  1
#define PTX_COLOR_CONTRAST    2
#define PTX_COLOR_SATURATION  3
#define PTX_COLOR_HUE         4
#define PTX_COLOR_GRAYSCALE   5
#define PTX_COLOR_MAX_OPS     5

/* frames: contiguous uint8 [N][T][H][W][3], any byte alignment.  out_mode: PTX_RESIZE_OUT_U8 writes uint8 [N][T][H][W][3]
 * (any alignment); PTX_RESIZE_OUT_F32 / PTX_RESIZE_OUT_BF16 write the normalised clip [N][3][T][H][W] (4- / 2-byte
 * aligned), every value exactly what ptx_frames_u8_to_ncdhw / PTX_RESIZE_OUT_BF16 make of the jittered byte.
 * contrast: non-zero iff a list holds PTX_COLOR_CONTRAST; then ptx_color_jitter_stats runs before ptx_color_jitter_apply
 * on the same stream and both take `sums` (N * T 64-bit counters, 8-byte aligned, zeroed by the statistics call itself).
 * With contrast == 0 the statistics call is not needed and `sums` may be null. */
typedef struct ptx_color_desc {
    int32_t N, T, H, W;
    int32_t out_mode;                  /* PTX_RESIZE_OUT_*                                                         */
    int32_t contrast;                  /* does any clip's list hold PTX_COLOR_CONTRAST                             */
} ptx_color_desc;

/* Host-side check, no device needed: the descriptor and HOST copies of the lists ([N][PTX_COLOR_MAX_OPS] each).  1 when the
 * launches accept them, else 0 with ptx_last_error(): a null pointer, extents, an op code out of range, a repeated code, a
 * hue shift that is not an integer 0..255, a factor that is negative or not finite, `contrast` not matching the lists. */
int ptx_color_jitter_supported(const ptx_color_desc* desc, const int32_t* ops_host, const float* factors_host);
/* ops / factors / sums are DEVICE arrays from here on. */
int ptx_color_jitter_stats(const ptx_color_desc* desc, const uint8_t* frames, const int32_t* ops, const float* factors,
                           uint64_t* sums, ptx_stream_t stream);
int ptx_color_jitter_apply(const ptx_color_desc* desc, const uint8_t* frames, const int32_t* ops, const float* factors,
                           const uint64_t* sums, void* y, const ptx_norm_desc* norm, ptx_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif  /* PTX_AMD_COLOR_H */
