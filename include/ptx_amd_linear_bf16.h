/* pretorched-x_amd: Linear layers with bf16 WEIGHTS for few input rows (csrc/linear_bf16.hip) -- the TRN relation MLPs and the
 * classifier of a bfloat16 model.  Exported by the same libptx_amd.so.  They live in a header of their own, like
 * ptx_amd_nl_ks.h: ptx_amd.h is the census of the drop-in contract as it stood before them, this file adds to it.
 *
 * The three entry points mirror ptx_linear_fwd / ptx_relation_linear_fwd / ptx_linear_setsum_fwd (ptx_amd.h) and reuse
 * ptx_relation_desc, PTX_REL_MAX_SETS and PTX_REL_MAX_FRAMES.  Flags: PTX_PRO_RELU (ReLU on x), PTX_EPI_RELU, PTX_EPI_ACCUM.
 *
 * Arithmetic contract (all three):
 *   - a bf16 weight (and bias) is widened to fp32 exactly;
 *   - a bf16 x, after the optional ReLU, times a bf16 weight is exact in fp32; an fp32 x enters as fmaf(x, widen(w), acc);
 *   - accumulation is fp32, in an order fixed by (M, K, Nout) and by which of the two paths below runs -- never by the data,
 *     the stream or the launch: two runs give the same bits, and no floating-point atomic is used anywhere;
 *   - bias, PTX_EPI_ACCUM and PTX_EPI_RELU are applied in fp32; y is fp32 and nothing is rounded to bf16 inside the kernel.
 *
 * Paths:
 *   matrix-core path   bf16 x whose rows are 16-byte aligned (K % 8 == 0, ldx % 8 == 0, x and w 16-byte aligned): a workgroup
 *                      stages its <= 32 input rows of a 256-wide K slab in LDS once (ReLU and the frame gather applied while
 *                      staging) and streams 128 weight rows x 256 k straight from global memory into
 *                      v_mfma_f32_16x16x32_bf16.  K is split across workgroups; the partial tiles go through `workspace`
 *                      and are summed in split order by a second launch (ptx_linear_bf16w_workspace_bytes says how much).
 *                      The gather entry point always runs here, so a gather launch has the bits of the dense launch on the
 *                      gathered rows.
 *   vector-unit path   everything else (fp32 x, set-sum, unaligned or odd-K bf16 x): one wave per output feature, 8 k per lane
 *                      and step; needs no workspace. */
#ifndef PTX_AMD_LINEAR_BF16_H
#define PTX_AMD_LINEAR_BF16_H

#include "ptx_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PTX_LIN_X_BF16 0 /* x is bf16 [M][ldx] */
#define PTX_LIN_X_F32 1  /* x is fp32 [M][ldx] */

/* Bytes of device workspace a dense / gather launch of (M, K, Nout) may need (0 when K is not split).  A function of the three
 * extents only.  The workspace needs 16-byte alignment and is not read after the call's kernels have run. */
size_t ptx_linear_bf16w_workspace_bytes(int32_t M, int32_t K, int32_t Nout);

/* y[m][j] (+)= sum_k act(x[m][k]) * w[j][k] + b[j]     x: bf16 or fp32 [M][ldx] (x_kind), w: bf16 [Nout][K], b: bf16 [Nout] or
 * NULL, y: fp32 [M][ldy]; columns [Nout, ldy) of y are not touched.  Any K >= 1 and Nout >= 1.
 * _supported: 1 if the call can run, else 0 with the reason in ptx_last_error() (the pointers are only looked at). */
int ptx_linear_bf16w_supported(const void* x, int32_t x_kind, const void* w, const void* b, const float* y, int32_t M, int32_t K,
                               int32_t Nout, int32_t ldx, int32_t ldy, uint32_t flags);
int ptx_linear_bf16w_fwd(const void* x, int32_t x_kind, const void* w, const void* b, float* y, int32_t M, int32_t K,
                         int32_t Nout, int32_t ldx, int32_t ldy, uint32_t flags, void* workspace, size_t workspace_bytes,
                         ptx_stream_t stream);

/* First Linear of every frame subset of one TRN relation scale: row r*B + v of y reads the frames desc->idx[r][0..n_frames) of
 * video v out of bf16 x[B][ldx] (frame f at x + v*ldx + f*frame_len), K = n_frames * frame_len, M = n_sets * B.
 * Requires frame_len % 8 == 0, ldx % 8 == 0 and 16-byte aligned x and w (the matrix-core path). */
int ptx_relation_linear_bf16w_supported(const ptx_relation_desc* desc, const void* x, int32_t ldx, const void* w, const void* b,
                                        const float* y, int32_t Nout, int32_t ldy, uint32_t flags);
int ptx_relation_linear_bf16w_fwd(const ptx_relation_desc* desc, const void* x, int32_t ldx, const void* w, const void* b,
                                  float* y, int32_t Nout, int32_t ldy, uint32_t flags, void* workspace, size_t workspace_bytes,
                                  ptx_stream_t stream);

/* Second Linear of those relations, summed over the subsets:  y[v][j] (+)= sum_k (sum_r x[r*B + v][k]) * w[j][k] + n_sets * b[j]
 * with fp32 x [n_sets * B][ldx] (the set sum is taken in fp32, r ascending, before the optional ReLU). */
int ptx_linear_setsum_bf16w_supported(const float* x, const void* w, const void* b, const float* y, int32_t B, int32_t n_sets,
                                      int32_t K, int32_t Nout, int32_t ldx, int32_t ldy, uint32_t flags);
int ptx_linear_setsum_bf16w_fwd(const float* x, const void* w, const void* b, float* y, int32_t B, int32_t n_sets, int32_t K,
                                int32_t Nout, int32_t ldx, int32_t ldy, uint32_t flags, ptx_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* PTX_AMD_LINEAR_BF16_H */
