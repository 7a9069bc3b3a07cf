/*
 * Pointer alignment contract of the entry points declared in ptx_amd.h (whose bytes are pinned by a test and so cannot
 * carry these sentences itself).  Comments only: this header declares nothing.  Each line is what the entry accepts -- a
 * weaker pointer is PTX_ERR_INVALID with a message where a check exists ("refused"), and is legal where the kernel reads and
 * writes one element at a time ("any").  tests/test_gpu_footprint_*.py run the entries they cover at exactly this alignment.
 *
 * Dense convolution (everything that goes through make_conv_args: ptx_conv3d_fwd, ptx_conv3d_dual_fwd,
 * ptx_conv3d_fused_fwd, the stages of a conv program):
 *   x, x2, w_packed, bias, res, y, workspace   16 bytes, refused otherwise.  bias too: the row-major epilogues, the direct
 *                                              kernel and the split-K reduction read four biases with one load.
 *   ptx_conv_fused_ext scale / shift           16 bytes and ld_affine % 4 == 0, refused otherwise, by EVERY entry that takes
 *                                              the struct (ptx_conv3d_fused_fwd, ptx_conv3x3_f16/bf16_fwd,
 *                                              ptx_conv1x1_skip_f16/bf16_fwd, ptx_conv1x1_pro_f16_fwd): four channels per load.
 *   y_raw                                      16 bytes, refused otherwise.
 * ptx_conv3d_chain_fwd:  x, w_packed, w2_packed, res, y and bias2 16 bytes, refused otherwise (bias2 feeds the row-major
 *                        epilogue); bias is read one float at a time: any 4-byte alignment.
 * ptx_conv_body_f32_fwd, ptx_conv_body_chain_f32_fwd:  x, w_body, w_tail, res, y 16 bytes, refused otherwise; bias and bias2
 *                        are read one float at a time: any 4-byte alignment.
 * ptx_bgemm_nt:          A, B, C 16 bytes, refused otherwise; lda / ldb >= round_up(K, 4), strides multiples of 4; columns
 *                        [Nn, ldc) of C are written as zero.
 * ptx_pack_conv_weight:  every pointer any 4-byte alignment (2-byte for a 16-bit packed filter).
 * ptx_conv_program_build / _fwd: the stage pointers as ptx_conv3d_fwd; the workspace 256 bytes, refused otherwise
 *                        (PTX_ERR_WORKSPACE); the device image holds pointers: keep it 16-byte aligned.
 * Stems: ptx_conv_stem_f32_fwd, ptx_conv_stem_x3_fwd, ptx_conv_stem_x3p_fwd: x, filter, y 16 bytes, refused otherwise.
 *        ptx_conv_stem_bf16_fwd / _strided_fwd: the bf16 clip any 2-byte alignment, uint8 frames any byte; filter and y 16
 *        bytes, refused otherwise.  ptx_pack_stem_bf16_weight: packed filter 2 bytes, stem filter 16, refused otherwise.
 * The filter re-packs (ptx_pack_stem_f32_weight, ptx_pack_stem_x3p_weight, ptx_pack_conv_body_f32_weight,
 *        ptx_pack_conv_body_tail_f32_weight, ptx_pack_wino_f32_weight, ptx_pack_wino4_f32_weight, ptx_pack_rgb_conv_weight)
 *        move one element at a time; pass them the 16-byte aligned buffers their consumers need anyway.
 *
 * Pooling and head:
 *   ptx_maxpool3d_fwd                          x, y 16 bytes, refused otherwise.
 *   ptx_copy2d                                 x, y 16 bytes, refused otherwise.
 *   ptx_affine_act_upsample                    x, y 16 bytes, refused otherwise; scale / shift any 4-byte alignment, any ld_scale
 *                                              (16-byte aligned tables with C and ld_scale multiples of 4 are read a quad at a
 *                                              time: the same values).
 *   ptx_cbn_fold, ptx_outer_sum_relu, ptx_window_mean, ptx_global_avgpool (both layouts), ptx_softmax_rows,
 *   ptx_transpose_last2, ptx_pad_rows          every pointer any 4-byte alignment; ptx_global_avgpool_bf16: x any 2-byte.
 *   ptx_linear_fwd                             x, w, b, y any 4-byte alignment, any K / ldx / ldy.  The matrix-core route
 *                                              (M >= 32, no flag but PTX_EPI_RELU) is taken only when all four are 16-byte
 *                                              aligned and K, Nout, ldx, ldy are multiples of 4; the 16-byte GEMV route when x
 *                                              and w are aligned and K, ldx multiples of 4; the scalar kernel otherwise.
 *   ptx_relation_linear_fwd, ptx_linear_setsum_fwd   x, w 16 bytes, refused otherwise; b, y any 4-byte alignment.
 *
 * Layout:
 *   ptx_ncdhw_to_ndhwc, ptx_ndhwc_to_ncdhw     any 4-byte alignment, ld % 4 == 0 (C <= 4, ld == 4 and a 16-byte aligned y write
 *                                              whole positions; any other y runs the tile transpose: the same values).
 *   ptx_ncdhw_to_split4                        x any 4-byte alignment; y 16 bytes, refused otherwise.
 *   ptx_ncdhw_to_split_planes                  x, y 16 bytes and W % 8 == 0, refused otherwise.
 *   ptx_fold_kw_ncdhw, ptx_fold_kw_strided     x any 4-byte alignment; y 16 bytes, refused otherwise.
 *   ptx_f32_to_bf16, ptx_bf16_to_f32           element size (4 bytes fp32, 2 bytes bf16); any n.
 *   ptx_checksum_f32, ptx_checksum_b16         table and out 8 bytes, the tensors their element size; only *out is written.
 *
 * Attention:
 *   ptx_nonlocal_fwd, ptx_nonlocal_ws_fwd      theta, phi, g, y 16 bytes, refused otherwise; a workspace that is not 16-byte
 *                                              aligned is not an error: the call runs what ptx_nonlocal_fwd runs.
 *
 * Already stated next to their declarations: ptx_nonlocal_bf16_fwd, ptx_conv_stem_bf16_fwd, ptx_im2col_hw_bf16 and the bf16
 * transposes (ptx_amd.h), ptx_amd_bn.h, ptx_amd_dw.h, ptx_amd_linear_bf16.h.
 */
#ifndef PTX_AMD_ALIGNMENT_H
#define PTX_AMD_ALIGNMENT_H
#include "ptx_amd.h"
#endif
