/* pretorched-x_amd: Winograd F(4x4,3x3) for stride-1 (kT,3,3) fp32 convolutions -- the seven entry points that mirror the
 * F(2x2) calls of ptx_amd.h (csrc/conv_wino_f32.hip), exported by the same libptx_amd.so.  They live in a header of their
 * own: ptx_amd.h is the census of the drop-in contract as it stood before them, this file adds to it. */
#ifndef PTX_AMD_WINO4_H
#define PTX_AMD_WINO4_H

#include "ptx_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The same convolution as Winograd F(4x4,3x3): 36 multiplies per 4x4 outputs and channel pair (2.25 per output against 4 for
 * F(2x2) and 9 direct), V and M 2.25x the activation instead of 4x.  The seven calls mirror the seven above and take the same
 * DIRECT descriptor; what differs:
 *   tiles      H4 x W4 = ceil(Hi / 4) x ceil(Wi / 4) per frame, ANY positive Hi and Wi: ptx_wino4_in_f32 reads the 6x6 patch at
 *              rows 4i-1..4i+4, columns 4j-1..4j+4 as zero outside the frame (the overhang of a partial tile included),
 *              ptx_wino4_out_f32 masks the outputs of a partial tile that lie outside the frame.
 *   layouts    V [N][T][H4][W4][36 * Cg], M [N][T][H4][W4][36 * Cog], transform position xi = 6 a + b;
 *              w_wino [kt][rows][Cg], row = xi * Cog + co, rows = round_up(36 * Cog, 128).
 *   grouped    ptx_conv_wino4_f32_gemm_desc: groups = 36, Hi = Wi = H4, W4, Ci = ldx = 36 * Cg, Co = ldy = 36 * Cog, Kc = Cg,
 *              Co_pad = rows.
 *   matrices   Lavin's for the points 0, +-1, +-2, inf; the filter transform U = G g G^T runs in fp32.
 * Arithmetic: fp32 throughout; the transforms' larger constants cost 10-20x the direct path's rounding error per conv
 * (measured: up to 2e-5 of the output scale at 256 channels, 1e-6 on the logits of a whole network). */
int ptx_conv_wino4_f32_supported(const ptx_conv3d_desc* desc);
size_t ptx_conv_wino4_f32_workspace_bytes(const ptx_conv3d_desc* desc);
int ptx_conv_wino4_f32_gemm_desc(const ptx_conv3d_desc* desc, ptx_conv3d_desc* gemm);
size_t ptx_wino4_f32_weight_elems(const ptx_conv3d_desc* desc);
int ptx_pack_wino4_f32_weight(const ptx_conv3d_desc* desc, const float* w_packed, float* w_wino, ptx_stream_t stream);
int ptx_wino4_in_f32(const ptx_conv3d_desc* desc, const float* x, float* V, ptx_stream_t stream);
int ptx_wino4_out_f32(const ptx_conv3d_desc* desc, const float* M, const float* bias, const float* res, float* y,
                      ptx_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif  /* PTX_AMD_WINO4_H */
