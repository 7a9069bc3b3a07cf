/* pretorched-x_amd: the fp32 RGB stem as a fast FIR along time (csrc/conv_stem_tfir_f32.hip), exported by the same
 * libptx_amd.so.  The entry points live in a header of their own, like ptx_amd_wino4.h: ptx_amd.h is the census of the
 * drop-in contract as it stood before them, this file adds to it. */
#ifndef PTX_AMD_TFIR_H
#define PTX_AMD_TFIR_H

#include "ptx_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* A 7x7x7 stem with temporal stride 1 is, along time, a 7-tap FIR.  A Toom-Cook / Winograd FIR F(m, 7) computes m output
 * frames from P < 7 m FRAME-CONVOLUTIONS -- 2-D kH x 7 convolutions of a linear combination of input frames with a linear
 * combination of temporal filter taps:
 *     y[t0 + o] = sum_j AT[o][j] * conv2d( sum_i BT[j][i] * x[t0 - pT + i],  sum_k G[j][k] * w[k] )
 *                 o < m,  i < m + 6,  j < P,  k < 7;  frames outside the clip are zero;  t0 = g m for the ceil(To / m) groups g.
 * The direct kernel (ptx_conv_stem_f32_fwd) runs 100 frame-convolutions per 16-frame clip after its end-of-clip pruning.
 *   scheme 1   F(2,7) on the points 0, +-1, +-2, +-1/2, inf                                   m = 2, P = 8:   64 per 16 frames
 *   scheme 2   taps 0..3 by F(4,4) (0, +-1, +-2, 1/2, inf) + taps 4..6 by F(4,3) (0, +-1, +-2, inf)  m = 4, P = 13:  52
 *   scheme 3   F(4,7) on the points 0, +-1, +-2, +-1/2, 4, 1/4, inf                           m = 4, P = 10:  40
 * Three launches: ptx_pack_stem_tfir_f32_weight once per filter, then per forward ptx_stem_tfir_in_f32 (the temporal input
 * transform, memory bound) and ptx_conv_stem_tfir_f32_fwd (the direct stem's step loop over the P products of a group, the
 * 64-channel product tile folded into m output accumulators at every product change).
 *
 * desc, stride_n / stride_c / stride_t: exactly the arguments of ptx_conv_stem_f32_fwd (the DIRECT descriptor and the strides
 * of x).  ptx_conv_stem_tfir_f32_supported is that kernel's rule plus: sT == 1, kT == 7, a known scheme, V and every operand
 * below 2 GiB; everything else is PTX_ERR_UNSUPPORTED from the calls.
 *   ptx_stem_tfir_scheme      m, P and the tables of a scheme, row-major: AT [m][P], G [P][7], BT [P][m + 6] (any pointer may
 *                             be NULL).  Exact rationals from the Vandermonde matrices of the points, rounded once to fp32.
 *   w_tfir                    the layout of ptx_pack_stem_f32_weight with kT replaced by P: [j * kH + kh][tile][11][2][64],
 *                             ptx_stem_tfir_f32_weight_elems floats, made from the packed (BN-folded) w_stem in fp32.
 *   V                         [N][3][groups * P][Hi][pitch] fp32, ptx_stem_tfir_f32_workspace_bytes: a plain NCDHW tensor whose
 *                             "frames" are the (group, product) pairs, so the stem's patch DMA reads it unchanged.
 * Arithmetic: fp32 throughout.  Measured against float64: schemes 1 and 2 within 1e-5 of the output scale (direct: 2e-7),
 * scheme 3 within 5e-5. */
int ptx_stem_tfir_scheme(int32_t scheme, int32_t* m, int32_t* P, float* AT, float* G, float* BT);
int ptx_conv_stem_tfir_f32_supported(const ptx_conv3d_desc* desc, int64_t stride_n, int64_t stride_c, int64_t stride_t,
                                     int32_t scheme);
size_t ptx_stem_tfir_f32_weight_elems(const ptx_conv3d_desc* desc, int32_t scheme);
size_t ptx_stem_tfir_f32_workspace_bytes(const ptx_conv3d_desc* desc, int32_t scheme);
int ptx_pack_stem_tfir_f32_weight(const ptx_conv3d_desc* desc, int32_t scheme, const float* w_stem, float* w_tfir,
                                  ptx_stream_t stream);
int ptx_stem_tfir_in_f32(const ptx_conv3d_desc* desc, int32_t scheme, const float* x, int64_t stride_n, int64_t stride_c,
                         int64_t stride_t, float* V, ptx_stream_t stream);
int ptx_conv_stem_tfir_f32_fwd(const ptx_conv3d_desc* desc, int32_t scheme, const float* V, const float* w_tfir,
                               const float* bias, float* y, ptx_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif  /* PTX_AMD_TFIR_H */
