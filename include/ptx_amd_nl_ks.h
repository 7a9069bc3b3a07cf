/* pretorched-x_amd: the two forms of the bf16 non-local attention (csrc/nonlocal_attn.hip, ptx_nonlocal_bf16_fwd) by name --
 * which one the dispatcher picks for a descriptor, whether a form covers it, and a launch of exactly one form.  Exported by
 * the same libptx_amd.so.  They live in a header of their own, like ptx_amd_wino4.h and ptx_amd_stem_strided.h: ptx_amd.h
 * is the census of the drop-in contract as it stood before them, this file adds to it. */
#ifndef PTX_AMD_NL_KS_H
#define PTX_AMD_NL_KS_H

#include "ptx_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Forms of the bf16 attention kernel:
 *   0  single group: 4 waves per workgroup on 32-key tiles (16-key tiles at d > 512) -- every PTX_NL_BF16 descriptor
 *      ptx_nonlocal_supported accepts;
 *   1  key split: 8 waves per workgroup on 64-key tiles; wave group wave / 4 takes 32 keys of every tile for the same 64
 *      queries with its own fp32 online-softmax state (m, l, O), the two states are merged once through LDS before the
 *      (unchanged) epilogue.  Covers d <= 256, any dv, all three modes (softmax, scale, scale + relu).
 * Both forms write the same columns of y ([0, round8(dv)), zeros above dv) and differ in fp32 summation order only. */

/* The form ptx_nonlocal_bf16_fwd runs for `desc`: a function of the per-sample extents (Nk, d, dv) and the mode only -- never
 * of desc->batch, so a clip's bits do not depend on the batch it arrives in.  PTX_NL_BF16_KSPLIT=0 / 1 (read at every call)
 * forces the key split off / on wherever it is supported.  0 for anything variant 1 does not cover. */
int ptx_nonlocal_bf16_variant(const ptx_nonlocal_desc* desc);

/* 1 when form `variant` runs `desc` (a PTX_NL_BF16 descriptor ptx_nonlocal_supported accepts), else 0. */
int ptx_nonlocal_bf16_variant_supported(const ptx_nonlocal_desc* desc, int variant);

/* ptx_nonlocal_bf16_fwd with the form named: same operands, same checks, then PTX_ERR_UNSUPPORTED (before any launch) when
 * `variant` does not cover `desc`.  ptx_nonlocal_bf16_fwd(desc, ...) is this call with ptx_nonlocal_bf16_variant(desc). */
int ptx_nonlocal_bf16_variant_fwd(const ptx_nonlocal_desc* desc, int variant, const void* theta, const void* phi, const void* g,
                                  void* y, ptx_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif  /* PTX_AMD_NL_KS_H */
