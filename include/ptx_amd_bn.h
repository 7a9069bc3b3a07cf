/* pretorched-x_amd: batch-statistics BatchNorm forward on channels-last fp32 activations (csrc/bn_batch.hip) -- what
 * update_bn (recomputing running_mean / running_var with a forward-only pass) is built from.  Exported by the same
 * libptx_amd.so.  They live in a header of their own, like ptx_amd_linear_bf16.h: ptx_amd.h is the census of the drop-in
 * contract as it stood before them, this file adds to it.
 *
 * One BatchNorm of a batch-statistics plan is four launches:
 *   ptx_bn_batch_stats_f32   2 launches: per-workgroup partial sums into `workspace`, then a fixed-order combine
 *   ptx_bn_batch_update_f32  1 launch:   scale / shift of this batch, running_mean / running_var moved towards it
 *   ptx_bn_apply_f32         1 launch:   y = act(raw * scale + shift [+ residual])
 *
 * Arithmetic of the moments.  Every channel c has the pivot p[c] = x[0][c] (its first row).  A lane owns 4 consecutive
 * channels (one 16-byte load per row) and accumulates s1 = sum (x - p) and s2 = sum (x - p)^2 over its rows in fp32; the
 * lanes of a workgroup that share a channel quad are added by a tree in LDS; one (s1, s2) pair per workgroup and channel
 * goes to the workspace.  The combine launch adds the pairs of a channel in double precision, workgroup index ascending,
 * and writes mean = p + S1 / n and var = S2 / n - (S1 / n)^2 (biased, clamped at 0).  Raw values are never squared: the
 * cancellation in S2 / n - (S1 / n)^2 is governed by (mean - p)^2 / var -- how far the first row lies from the mean in
 * standard deviations -- instead of mean^2 / var.  Which rows a lane reads, the tree and the order of the combine are
 * functions of (rows, C) alone: no floating-point atomic is used, and two runs on the same input give the same bits. */
#ifndef PTX_AMD_BN_H
#define PTX_AMD_BN_H

#include "ptx_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of device workspace ptx_bn_batch_stats_f32 needs for (rows, C); a function of the two extents only.  16-byte aligned;
 * not read after the call's kernels have run. */
size_t ptx_bn_batch_stats_workspace_bytes(int64_t rows, int32_t C);

/* mean[c], var[c] (biased: divided by rows) of x[rows][ld] over the rows, for the channels c < C.  ld >= C, ld % 4 == 0, x
 * 16-byte aligned.  Channels [C, ld) are read only inside the last channel quad (C % 4 != 0) and influence no output. */
int ptx_bn_batch_stats_f32(const float* x, int64_t rows, int32_t C, int32_t ld, float* mean, float* var, void* workspace,
                           size_t workspace_bytes, ptx_stream_t stream);

/* From the batch moments of n values per channel (n >= 2):
 *   scale[c] = gamma[c] / sqrt(var[c] + eps)        shift[c] = beta[c] - mean[c] * scale[c]      (gamma / beta NULL: 1 / 0)
 *   running_mean[c] = (1 - f) * running_mean[c] + f * mean[c]
 *   running_var[c]  = (1 - f) * running_var[c]  + f * var[c] * n / (n - 1)
 * running_mean / running_var may both be NULL (nothing tracked). */
int ptx_bn_batch_update_f32(const float* mean, const float* var, int64_t n, float f, float eps, const float* gamma,
                            const float* beta, float* running_mean, float* running_var, float* scale, float* shift, int32_t C,
                            ptx_stream_t stream);

/* y = act(raw * scale + shift [+ residual]) on [N][T][H][W] positions of C channels.  flags: PTX_EPI_RELU, and at most one of
 * PTX_EPI_RES_ADD (res has y's positions, row stride ldr) and PTX_EPI_RES_PADA (shortcut A: res is [N][res_T][res_H][res_W]
 * with res_C <= C channels, read at (t * res_sT, h * res_sH, w * res_sW); channels >= res_C add nothing).  The other fields
 * of the residual are ignored without a residual flag. */
typedef struct ptx_bn_apply_desc {
    int32_t N, T, H, W, C, ldx, ldy;
    uint32_t flags;
    int32_t ldr, res_C, res_T, res_H, res_W, res_sT, res_sH, res_sW;
} ptx_bn_apply_desc;

/* raw: [N*T*H*W][ldx], y: [N*T*H*W][ldy] (y == raw is allowed: in place), scale / shift: [C].  Row strides are multiples of 4
 * covering round_up(C, 4); raw, y and res are 16-byte aligned.  Channels [C, round_up(C, 4)) of y are written as zero. */
int ptx_bn_apply_f32(const ptx_bn_apply_desc* desc, const float* raw, const float* scale, const float* shift, const float* res,
                     float* y, ptx_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* PTX_AMD_BN_H */
