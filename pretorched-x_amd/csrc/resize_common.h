// Pieces shared by the two PIL-exact resize kernels: resize_frames_u8_kernel (pack_layout.hip: one window of every
// frame) and resize_views_u8_kernel (resize_views.hip: clips x crops of a video, sampled through an index table).
#pragma once
#include "ptx_common.h"
#include <algorithm>

namespace ptx {

// TransformImage's tensor half on one byte (ToTensor /255, ToRange255 *255, Normalize): the _rn intrinsics keep the
// compiler from contracting the operations, so the result is bit-identical to the CPU tensors.
__device__ __forceinline__ float normalise_u8(unsigned char u, float mean, float stdv, int to_255) {
    float v = __fdiv_rn((float)u, 255.0f);
    if (to_255) v = __fmul_rn(v, 255.0f);
    return __fdiv_rn(__fsub_rn(v, mean), stdv);
}

constexpr int kResizeBand = 16;                 // output rows per workgroup (fewer when the LDS image would not fit)
constexpr int kResizeLdsCap = 64 * 1024;
constexpr int kResizeBits = 22;                 // PIL's PRECISION_BITS for 8-bit channels

struct ResizePlan {
    int band, lds_rows, stage_stride, istride, vec_store;
    int k_in_lds, k_off, stage_off;          // coefficient tables copied to LDS (when they fit); byte offsets of the carves
    size_t lds_bytes;
};

__device__ __forceinline__ void resize_entry(const int* __restrict__ lo_t, const int* __restrict__ n_t, int i, int extent,
                                             int taps, int& lo, int& n) {
    lo = min(max(lo_t[i], 0), extent - 1);
    n = min(max(n_t[i], 0), min(taps, extent - lo));
}

__device__ __forceinline__ int clip8(int v) { return min(max(v, 0), 255); }

// The bytes [off, end) of input row `row` that the column table references, relative to the 16-byte aligned address g:
// a byte head [off, vb), 16-byte pieces [vb, ve), a byte tail [ve, end).  g itself may lie before the row: only
// [off, end) is dereferenced.
__device__ __forceinline__ const unsigned char* resize_row_span(const unsigned char* fin, int row, int W, int cmin, int C,
                                                                int span_bytes, int& off, int& vb, int& ve, int& end) {
    const unsigned char* src = fin + ((size_t)row * W + cmin) * C;
    off = (int)(reinterpret_cast<uintptr_t>(src) & 15);
    end = off + span_bytes;
    vb = min((off + 15) & ~15, end);
    ve = max(vb, end & ~15);
    return src - off;
}

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
struct ResizeRow {               // one lane's share of the first 3 KiB of a row, on its way from HBM to LDS
    u32x4 v0, v1, v2;
    unsigned head, tail;
};

__device__ __forceinline__ void resize_fetch_row(ResizeRow& r, int i, int nrows, const unsigned char* fin, int lo0, int W,
                                                 int cmin, int C, int span_bytes, int lane) {
    if (i >= nrows) return;
    int off, vb, ve, end;
    const unsigned char* g = resize_row_span(fin, lo0 + i, W, cmin, C, span_bytes, off, vb, ve, end);
    if (lane < vb - off) r.head = g[off + lane];
    if (vb + lane * 16 < ve) r.v0 = *reinterpret_cast<const u32x4*>(g + vb + lane * 16);
    if (vb + (64 + lane) * 16 < ve) r.v1 = *reinterpret_cast<const u32x4*>(g + vb + (64 + lane) * 16);
    if (vb + (128 + lane) * 16 < ve) r.v2 = *reinterpret_cast<const u32x4*>(g + vb + (128 + lane) * 16);
    if (lane < end - ve) r.tail = g[ve + lane];
}

// Launch shape of resize_frames_u8_kernel, or the reason there is none.  taps_h is the widest row's tap count, and a
// row of support s has more than 2 s - 1 taps, so output rows advance by at most taps_h / 2 input rows: a band of b
// output rows references at most b * taps_h / 2 + taps_h + 1 input rows (b when taps_h == 1: the axis is not resampled).
inline int resize_plan(const ptx_resize_desc* d, const void* y, ResizePlan* p, const char* who) {
    if (!d) return fail(PTX_ERR_INVALID, "%s: null descriptor", who);
    if (d->N <= 0 || d->T <= 0 || d->H <= 0 || d->W <= 0 || d->Ho <= 0 || d->Wo <= 0)
        return fail(PTX_ERR_INVALID, "%s: non-positive extent (N=%d T=%d H=%d W=%d Ho=%d Wo=%d)", who, d->N, d->T, d->H, d->W,
                    d->Ho, d->Wo);
    if (d->C <= 0 || d->C > 4) return fail(PTX_ERR_INVALID, "%s: C=%d must be 1..4", who, d->C);
    if (d->taps_h <= 0 || d->taps_w <= 0) return fail(PTX_ERR_INVALID, "%s: taps_h=%d taps_w=%d must be positive", who, d->taps_h, d->taps_w);
    if (d->out_mode != PTX_RESIZE_OUT_U8 && d->out_mode != PTX_RESIZE_OUT_F32 && d->out_mode != PTX_RESIZE_OUT_BF16)
        return fail(PTX_ERR_INVALID, "%s: out_mode=%d is not a PTX_RESIZE_OUT_* value", who, d->out_mode);
    if (d->taps_h > PTX_RESIZE_MAX_TAPS || d->taps_w > PTX_RESIZE_MAX_TAPS)
        return fail(PTX_ERR_UNSUPPORTED, "%s: taps_h=%d taps_w=%d exceed PTX_RESIZE_MAX_TAPS=%d", who, d->taps_h, d->taps_w,
                    PTX_RESIZE_MAX_TAPS);
    const int64_t lim = INT32_MAX;
    if ((int64_t)d->H * d->W * d->C > lim || (int64_t)d->Ho * d->Wo * d->C > lim || (int64_t)d->Ho * d->taps_h > lim ||
        (int64_t)d->Wo * d->taps_w > lim || (int64_t)d->N * d->T > lim)
        return fail(PTX_ERR_UNSUPPORTED, "%s: a frame or a table exceeds 32-bit indexing", who);
    p->stage_stride = ((d->W * d->C + 15) & ~15) + 16;
    p->istride = (d->Wo * d->C + 3) & ~3;
    auto rows_of = [&](int b) { return d->taps_h > 1 ? (b * d->taps_h + 1) / 2 + d->taps_h + 1 : b; };
    // LDS carves: header + clamped lo / n entries, [the coefficient tables], 4 row stages, the intermediate image.  The
    // coefficients stay in global memory (L2) when copying them would leave no room for a band of 8 rows.
    const int64_t entries = 16 + (((2 * (int64_t)d->Wo + 2 * kResizeBand) * 4 + 15) & ~(int64_t)15);
    const int64_t coeffs = (((int64_t)d->Wo * d->taps_w + (int64_t)kResizeBand * d->taps_h) * 4 + 15) & ~(int64_t)15;
    const int64_t stages = 4 * (int64_t)p->stage_stride;
    p->k_in_lds = entries + coeffs + stages + (int64_t)rows_of(std::min(8, d->Ho)) * p->istride <= kResizeLdsCap;
    const int64_t fixed = entries + (p->k_in_lds ? coeffs : 0) + stages;
    if (fixed + (int64_t)d->taps_h * p->istride > kResizeLdsCap)
        return fail(PTX_ERR_UNSUPPORTED, "%s: W=%d, Wo=%d, taps_h=%d need %lld bytes of LDS staging (cap %d)", who, d->W, d->Wo,
                    d->taps_h, (long long)(fixed + (int64_t)d->taps_h * p->istride), kResizeLdsCap);
    p->k_off = (int)entries;
    p->stage_off = (int)(entries + (p->k_in_lds ? coeffs : 0));
    const int max_rows = (int)((kResizeLdsCap - fixed) / p->istride);
    int band = std::min(kResizeBand, d->Ho);
    while (band > 1 && rows_of(band) > max_rows) --band;
    p->band = band;
    p->lds_rows = std::max(std::min(max_rows, rows_of(band)), d->taps_h);
    p->lds_bytes = (size_t)fixed + (size_t)p->lds_rows * p->istride;
    if ((int64_t)d->N * d->T * cdiv(d->Ho, band) > lim) return fail(PTX_ERR_UNSUPPORTED, "%s: too many workgroups", who);
    const uintptr_t ya = reinterpret_cast<uintptr_t>(y);
    p->vec_store = d->out_mode == PTX_RESIZE_OUT_U8 ? ((d->Wo * d->C) % 4 == 0 && ya % 4 == 0)
                                                    : (d->Wo % 4 == 0 && ya % (d->out_mode == PTX_RESIZE_OUT_F32 ? 16 : 8) == 0);
    return PTX_OK;
}

}  // namespace ptx
