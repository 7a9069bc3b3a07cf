/* pretorched-x_amd: depthwise 3-D convolution in fp32 (csrc/conv_dw_f32.h), exported by the same libptx_amd.so -- the 3x3x3 conv
 * of the channel-separated networks (ir-CSN / ip-CSN; Tran et al., ICCV 2019): groups == Ci == Co, one filter of kT*kH*kW taps per
 * channel.  ptx_conv3d_fwd keeps refusing such descriptors (Ci / groups % 4 != 0); the matrix cores have nothing to do here, the
 * launch is a streaming pass over the activation.  A header of its own, like ptx_amd_cam.h and ptx_amd_bn.h: ptx_amd.h is the
 * census of the drop-in contract as it stood before, this file adds to it. */
#ifndef PTX_AMD_DW_H
#define PTX_AMD_DW_H

#include "ptx_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* 1. What the launch takes, from the descriptor alone (no device needed): 1, else 0 with ptx_last_error().  Refused as
 * PTX_ERR_UNSUPPORTED: anything but
 *   groups == Ci == Co = C with C % 4 == 0;
 *   kT, kH, kW in {1, 3};  strides 1 or 2 per axis;  0 <= pad < k per axis;
 *   To / Ho / Wo == (in + 2 pad - k) / stride + 1, all extents positive;
 *   ldx, ldy >= C and both % 4 == 0 (16-byte rows);
 *   flags within PTX_EPI_RELU;
 *   one input frame (Hi * Wi * ldx * 4 bytes) and one output frame (Ho * Wo * ldy * 4 bytes) below 2^31 bytes: a frame's base is
 *   64-bit, the offsets inside it are 32-bit and never wrap; one clip below 2^31 work items (any number of clips: the launch walks
 *   them in ranges).
 * Kc, Co_pad, the residual and second-source fields are not read. */
int ptx_conv3d_dw_f32_supported(const ptx_conv3d_desc* desc);

/* 2. Pack: w [C][1][kT][kH][kW] (nn.Conv3d(groups = C).weight) -> w_packed [kT*kH*kW][C], tap = (kt*kH + kh)*kW + kw, so the 4
 * channels of a lane are one 16-byte load per tap; with a BatchNorm (bn_gamma != NULL) folded in fp32, as ptx_pack_conv_weight folds:
 *   scale[c]        = gamma[c] * (1 / sqrtf(var[c] + eps))          (1 without a BatchNorm)
 *   w_packed[tap][c] = w[c][tap] * scale[c]
 *   bias_out[c]      = beta[c] + (conv_bias[c] - mean[c]) * scale[c]   (conv_bias may be NULL: 0)
 * w_packed: C * kT*kH*kW floats, bias_out: C floats.  Rewrites both in place (a refresh after the weights changed). */
int ptx_pack_dw_weight_f32(int32_t C, int32_t kT, int32_t kH, int32_t kW, const float* w, const float* conv_bias,
                           const float* bn_gamma, const float* bn_beta, const float* bn_mean, const float* bn_var, float bn_eps,
                           float* w_packed, float* bias_out, ptx_stream_t stream);

/* 3. Forward.  x: NDHWC fp32 [N][Ti][Hi][Wi][ldx]; y: NDHWC fp32 [N][To][Ho][Wo][ldy]; w / bias: from ptx_pack_dw_weight_f32; all
 * four 16-byte aligned.  Asynchronous on `stream`, no workspace, nothing allocated.
 *   acc = 0;  for kt, for kh, for kw (in this order): if the tap lies inside the volume: acc = fmaf(x[tap][c], w[tap][c], acc)
 *   y[n][to][ho][wo][c] = acc + bias[c], then max(., 0) under PTX_EPI_RELU
 * Taps outside the volume are skipped, not multiplied by zero.  The bits of an output depend on its own window alone: not on the
 * strip it was computed in, the grid, or the batch it arrived in.  Only channels [0, C) of a row are written: y may be a channel
 * slice of a wider tensor (its neighbours stay as they were). */
int ptx_conv3d_dw_f32_fwd(const ptx_conv3d_desc* desc, const float* x, const float* w, const float* bias, float* y,
                          ptx_stream_t stream);

/* 4. The form a launch takes, for measurements (scripts/gpu_csn_bench.py alternates the forms in one process): 0 = the library's own
 * rule (the default), else one of the codes below -- register-window strips of 4 or 8 output columns, or the LDS-staged halo tile
 * that was measured against them and lost.  Process-wide and not synchronised: set it while no launch is being issued.  The
 * environment variable PTX_DW_FORM gives the initial value, read once.  The bits of an output are the same under every form. */
#define PTX_DW_FORM_STRIP4 4
#define PTX_DW_FORM_STRIP8 8
#define PTX_DW_FORM_LDS 16
int ptx_conv3d_dw_f32_force_form(int32_t form);

#ifdef __cplusplus
}
#endif

#endif  /* PTX_AMD_DW_H */
