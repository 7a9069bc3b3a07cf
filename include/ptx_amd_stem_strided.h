/* pretorched-x_amd: the patch-resident bf16 stem (csrc/conv_stem_bf16.hip) reading every frame_step-th frame of its source --
 * the two entry points behind bf16 SlowFast / SlowOnly / FastOnly, whose pathways sub-sample the clip in time
 * (input[:, :, ::step]).  Exported by the same libptx_amd.so.  They live in a header of their own, like ptx_amd_wino4.h and
 * ptx_amd_tfir.h: ptx_amd.h is the census of the drop-in contract as it stood before them, this file adds to it. */
#ifndef PTX_AMD_STEM_STRIDED_H
#define PTX_AMD_STEM_STRIDED_H

#include "ptx_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ptx_conv_stem_bf16_fwd on a frame-strided source.  desc->Ti counts the frames the convolution USES; the source holds
 * T_full frames and conv frame t is source frame t * frame_step (the convention of ptx_fold_kw_frames_u8):
 *   PTX_STEM_SRC_BF16_NCDHW   [N][3][T_full][H][W] bf16, frame base ((n*3 + c)*T_full + t*frame_step) * H*W
 *   PTX_STEM_SRC_U8_NTHWC     [N][T_full][H][W][3] uint8, frame base (n*T_full + t*frame_step) * H*W*3
 * (frame bases in 64 bits, offsets inside a frame in 32).  Frames between the used ones are never read.  Temporal taps
 * outside the USED clip are skipped.  The filter and bias are ptx_pack_stem_bf16_weight's output; tiling, normalisation of
 * uint8 frames, arithmetic, rounding and the zero pad channels [Co, ldy) are ptx_conv_stem_bf16_fwd's, whose bits
 * frame_step = 1, T_full = Ti reproduces.
 * Refused (reason in ptx_last_error()): frame_step < 1, desc->Ti != ceil(T_full / frame_step), and everything
 * ptx_conv_stem_bf16_supported refuses (SAME-padded extents included). */
int ptx_conv_stem_bf16_strided_supported(const ptx_conv3d_desc* desc, int32_t src, int32_t frame_step, int32_t T_full);
int ptx_conv_stem_bf16_strided_fwd(const ptx_conv3d_desc* desc, const void* x, int32_t src, const struct ptx_norm_desc* norm,
                                   int32_t frame_step, int32_t T_full, const void* w_stem, const float* bias, void* y,
                                   ptx_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif  /* PTX_AMD_STEM_STRIDED_H */
