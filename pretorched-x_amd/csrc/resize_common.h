// Pieces shared by the two PIL-exact resize kernels: resize_frames_u8_kernel (pack_layout.hip: one window of every
// frame) and resize_views_u8_kernel (resize_views.hip: clips x crops of a video, sampled through an index table).
#pragma once
#include "ptx_common.h"
#include "../../include/ptx_amd_yuv16.h"
#include "../../include/ptx_amd_resample.h"
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

// clip8(sum >> kResizeBits) of a resampling sum as an unsigned byte, for the pass that packs four of them into a word.
// Coefficients may be negative (bicubic, Lanczos, Hamming: ptx_amd_resample.h), so a sum may be: clamp below, UNSIGNED shift,
// min -- yuv_clip8's form, one v_max_i32 more per byte than the unsigned shift + min it replaces, and for a sum >= 0 the same
// bits.  The signed clamp of the SHIFTED value is not used there: of two neighbouring sums it is selected as one
// v_ashr_pk_u8_i32, whose result hipcc then ORs with the other two bytes as if its upper half were zero; on gfx950 that upper
// half came back non-zero.  (Clamping into [0, 2^30 - 1] before the shift is one v_med3_i32 and no instruction more than
// before, but it changed the register allocation of the whole kernel and measured 1 % slower on the fp32 output: DESIGN 3.34.)
__device__ __forceinline__ unsigned resize_clip8(int sum) { return min((unsigned)max(sum, 0) >> kResizeBits, 255u); }

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

// ---------------------------------------------------------------------------------------------
// YUV 4:2:0 sources (ptx_yuv420_src: NV12 / I420 planes, any row pitch).  The row staging converts to RGB on the way
// from the registers to the row stage, so the stage holds the interleaved RGB bytes the horizontal pass reads and no
// RGB frame exists in HBM.  A lane owns GROUPS of 16 pixels that start at an even pixel (e0 = cmin & ~1, group g is
// [e0 + 16 g, e0 + 16 g + 16)): its 16 luma bytes and its 8 chroma pairs are exactly the bytes it needs, whatever the
// planes' alignments, so nothing crosses lanes.  A whole group is three loads (16 luma bytes; 16 interleaved or 8 + 8
// planar chroma bytes) through align-1 vector types -- gfx950 global loads take any address -- and the last, partial
// group of a row is fetched byte by byte, so no byte past the referenced span [cmin, cmax) is touched.
//   R = clip8((ky y' + krv cr + 2^15) >> 16)   G = clip8((ky y' - kgu cb - kgv cr + 2^15) >> 16)   B = clip8((ky y' + kbu cb + 2^15) >> 16)
// with y' = Y - y_off, cb = Cb - 128, cr = Cr - 128; chroma of pixel (r, c) is the sample (r >> 1, c >> 1).
// ---------------------------------------------------------------------------------------------
typedef u32x4 u32x4_any __attribute__((aligned(1)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef u32x2 u32x2_any __attribute__((aligned(1)));

struct YuvFrame {                // one frame of a ptx_yuv420_src
    const unsigned char *y, *u, *v;
};
struct YuvGroup {                // 16 pixels: luma bytes, then chroma as 8 U bytes (c.x, c.y) and 8 V bytes (c.z, c.w)
    u32x4 y, c;
};
struct YuvRow {                  // one lane's share of the first 2048 pixels of a row, on its way from HBM to LDS
    YuvGroup g0, g1;
};

__device__ __forceinline__ YuvFrame yuv_frame(const ptx_yuv420_src& s, int n, int t) {
    YuvFrame f;
    f.y = s.y + (int64_t)n * s.stride_n_y + (int64_t)t * s.stride_t_y;
    f.u = s.u + (int64_t)n * s.stride_n_c + (int64_t)t * s.stride_t_c;
    f.v = s.v + (int64_t)n * s.stride_n_c + (int64_t)t * s.stride_t_c;
    return f;
}

// Pixels [p0, min(p0 + 16, px_end)) of input row `row`; p0 is even and below px_end.
__device__ __forceinline__ void yuv_load_group(YuvGroup& g, const ptx_yuv420_src& s, const YuvFrame& f, int row, int p0,
                                               int px_end) {
    const unsigned char* yp = f.y + (size_t)row * s.pitch_y + p0;
    const size_t co = (size_t)(row >> 1) * s.pitch_c + (size_t)(p0 >> 1) * s.step_c;
    const int rem = px_end - p0;
    if (rem >= 16) {
        g.y = *reinterpret_cast<const u32x4_any*>(yp);
        if (s.step_c == 2) {
            const bool vu = f.v < f.u;                               // V first (NV21 order)
            const u32x4 q = *reinterpret_cast<const u32x4_any*>((vu ? f.v : f.u) + co);
            const unsigned e0 = __builtin_amdgcn_perm(q.y, q.x, 0x06040200u), e1 = __builtin_amdgcn_perm(q.w, q.z, 0x06040200u);
            const unsigned o0 = __builtin_amdgcn_perm(q.y, q.x, 0x07050301u), o1 = __builtin_amdgcn_perm(q.w, q.z, 0x07050301u);
            g.c = vu ? u32x4{o0, o1, e0, e1} : u32x4{e0, e1, o0, o1};
        } else {
            const u32x2 a = *reinterpret_cast<const u32x2_any*>(f.u + co), b = *reinterpret_cast<const u32x2_any*>(f.v + co);
            g.c = u32x4{a.x, a.y, b.x, b.y};
        }
    } else {
        unsigned yy[4] = {0, 0, 0, 0}, cc[4] = {0, 0, 0, 0};
#pragma unroll
        for (int k = 0; k < 16; ++k)
            if (k < rem) yy[k >> 2] |= (unsigned)yp[k] << (8 * (k & 3));
        const int nc = (rem + 1) >> 1;
#pragma unroll
        for (int k = 0; k < 8; ++k)
            if (k < nc) {
                cc[k >> 2] |= (unsigned)f.u[co + (size_t)k * s.step_c] << (8 * (k & 3));
                cc[2 + (k >> 2)] |= (unsigned)f.v[co + (size_t)k * s.step_c] << (8 * (k & 3));
            }
        g.y = u32x4{yy[0], yy[1], yy[2], yy[3]};
        g.c = u32x4{cc[0], cc[1], cc[2], cc[3]};
    }
}

// A negative sum gives 0: clamp below before the UNSIGNED shift, then min (not the signed clamp of the shifted value,
// see resize_frames_u8_kernel on v_ashr_pk_u8_i32).
__device__ __forceinline__ unsigned yuv_clip8(int sum) { return min((unsigned)max(sum, 0) >> 16, 255u); }

// Converts the group and writes its RGB bytes to dst (16-byte aligned): 48 bytes, or only the 4-byte words that hold
// one of the first `rem` pixels when the group is the partial last one of its row.
__device__ __forceinline__ void yuv_stage_group(unsigned char* dst, const YuvGroup& g, const ptx_yuv420_src& s, int rem) {
    const unsigned yw[4] = {g.y.x, g.y.y, g.y.z, g.y.w}, cw[4] = {g.c.x, g.c.y, g.c.z, g.c.w};
    unsigned o[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};          // 16 x RGB, byte 3 p + c of the group in word (3 p + c) / 4
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int cb = (int)((cw[k >> 2] >> (8 * (k & 3))) & 255u) - 128;
        const int cr = (int)((cw[2 + (k >> 2)] >> (8 * (k & 3))) & 255u) - 128;
        const int rv = __mul24(s.krv, cr) + 32768;
        const int gv = 32768 - __mul24(s.kgu, cb) - __mul24(s.kgv, cr);
        const int bv = __mul24(s.kbu, cb) + 32768;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int p = 2 * k + h;
            const int yy = __mul24(s.ky, (int)((yw[p >> 2] >> (8 * (p & 3))) & 255u) - s.y_off);
            o[(3 * p) >> 2] |= yuv_clip8(yy + rv) << (8 * ((3 * p) & 3));
            o[(3 * p + 1) >> 2] |= yuv_clip8(yy + gv) << (8 * ((3 * p + 1) & 3));
            o[(3 * p + 2) >> 2] |= yuv_clip8(yy + bv) << (8 * ((3 * p + 2) & 3));
        }
    }
    if (rem >= 16) {
#pragma unroll
        for (int q = 0; q < 3; ++q) *reinterpret_cast<u32x4*>(dst + 16 * q) = u32x4{o[4 * q], o[4 * q + 1], o[4 * q + 2], o[4 * q + 3]};
    } else {
#pragma unroll
        for (int j = 0; j < 12; ++j)
            if (4 * j < 3 * rem) *reinterpret_cast<unsigned*>(dst + 4 * j) = o[j];
    }
}

// The YUV counterparts of resize_fetch_row and of the kernels' "registers -> row stage" step.  Lane l owns groups l,
// 64 + l (prefetched in registers) and 128 + l, 192 + l, ... (rows of more than 2048 referenced pixels load those when
// the row is staged).  The stage holds pixel e0 at byte 0, so the horizontal pass reads pixel c at (cmin - e0) * 3 +
// (c - cmin) * 3: yuv_stage_row returns that first offset (0 or 3) as the RGB path returns its address mod 16.  The
// last word written ends below (cmax - e0) * 3 + 3 <= W * 3 + 6, inside the stage's W * 3 + 16 bytes.
__device__ __forceinline__ void yuv_fetch_row(YuvRow& r, int i, int nrows, const ptx_yuv420_src& s, const YuvFrame& f, int lo0,
                                              int cmin, int px_end, int lane) {
    if (i >= nrows) return;
    const int e0 = cmin & ~1;
    if (e0 + lane * 16 < px_end) yuv_load_group(r.g0, s, f, lo0 + i, e0 + lane * 16, px_end);
    if (e0 + (64 + lane) * 16 < px_end) yuv_load_group(r.g1, s, f, lo0 + i, e0 + (64 + lane) * 16, px_end);
}

__device__ __forceinline__ int yuv_stage_row(unsigned char* sw, const YuvRow& r, const ptx_yuv420_src& s, const YuvFrame& f,
                                             int row, int cmin, int px_end, int lane) {
    const int e0 = cmin & ~1;
    int p0 = e0 + lane * 16;
    if (p0 < px_end) yuv_stage_group(sw + (p0 - e0) * 3, r.g0, s, px_end - p0);
    p0 += 64 * 16;
    if (p0 < px_end) yuv_stage_group(sw + (p0 - e0) * 3, r.g1, s, px_end - p0);
    for (p0 += 64 * 16; p0 < px_end; p0 += 64 * 16) {
        YuvGroup g;
        yuv_load_group(g, s, f, row, p0, px_end);
        yuv_stage_group(sw + (p0 - e0) * 3, g, s, px_end - p0);
    }
    return (cmin - e0) * 3;
}

// Host-side checks of a ptx_yuv420_src for N x T frames of H x W pixels (no device needed).
inline int yuv_check(const ptx_yuv420_src* s, int C, int H, int W, const char* who) {
    if (!s) return fail(PTX_ERR_INVALID, "%s: null source descriptor", who);
    if (C != 3) return fail(PTX_ERR_INVALID, "%s: C=%d, a YUV source converts to 3 channels", who, C);
    if (!s->y || !s->u || !s->v) return fail(PTX_ERR_INVALID, "%s: null plane pointer", who);
    if (s->pitch_y <= 0 || s->pitch_c <= 0)
        return fail(PTX_ERR_INVALID, "%s: pitch_y=%d / pitch_c=%d must be positive", who, s->pitch_y, s->pitch_c);
    if (s->step_c != 1 && s->step_c != 2) return fail(PTX_ERR_INVALID, "%s: step_c=%d must be 1 (planar) or 2 (interleaved)", who, s->step_c);
    if (s->step_c == 2 && s->v != s->u + 1 && s->u != s->v + 1)
        return fail(PTX_ERR_INVALID, "%s: interleaved chroma (step_c=2) needs v == u + 1 (or u == v + 1)", who);
    const int64_t Hc = ((int64_t)H + 1) / 2, Wc = ((int64_t)W + 1) / 2;
    if (s->pitch_y < W || s->pitch_c < Wc * s->step_c)
        return fail(PTX_ERR_INVALID, "%s: pitch_y=%d / pitch_c=%d are shorter than a row (%d luma, %lld chroma bytes)", who,
                    s->pitch_y, s->pitch_c, W, (long long)(Wc * s->step_c));
    if ((int64_t)H * s->pitch_y > INT32_MAX || Hc * s->pitch_c > INT32_MAX)
        return fail(PTX_ERR_UNSUPPORTED, "%s: a plane of a frame exceeds 32-bit indexing", who);
    return PTX_OK;
}

// ---------------------------------------------------------------------------------------------
// 10- / 12-bit YUV 4:2:0 sources (ptx_yuv420p16_src: P010 / P012 / P016 surfaces, yuv420p10le / p12le planes): the
// same five pieces on 16-bit words.  A group is still 16 pixels that start at an even pixel, now 32 luma bytes and 32
// chroma bytes: four 16-byte loads (interleaved chroma is de-interleaved with v_perm on 16-bit lanes, planar chroma is
// one 16-byte load per plane), and the partial last group of a row is fetched sample by sample.  A sample is
// (word >> shift) & (2^bits - 1), and with d = bits - 8
//   R = clip8((ky y' + krv cr + 2^(15+d)) >> (16+d))   G = clip8((ky y' - kgu cb - kgv cr + 2^(15+d)) >> (16+d))
//   B = clip8((ky y' + kbu cb + 2^(15+d)) >> (16+d))   y' = Y - y_off, cb = Cb - (128 << d), cr = Cr - (128 << d)
// Products stay below 2^30 and sums below 2^31 (coefficients < 2^18, samples < 2^12), so __mul24 serves as it does
// for bytes.  The group is staged as the same 48 RGB bytes at the same place, so everything behind the row stage is
// shared with the other two flavours.
// ---------------------------------------------------------------------------------------------
constexpr int kSrcRgb = 0, kSrcYuv8 = 1, kSrcYuv16 = 2;     // the kernels' source flavour (template parameter SRC)
constexpr int kYuv16Prefetch = 2;                           // groups per lane a 16-bit row keeps in registers (of 1024 pixels each)

struct Yuv16Group {              // 16 pixels: 16 luma words (y0, y1), then 8 U words (u) and 8 V words (v)
    u32x4 y0, y1, u, v;
};
struct Yuv16Row {                // one lane's share of the first kYuv16Prefetch * 1024 pixels of a row
    Yuv16Group g[kYuv16Prefetch];
};

__device__ __forceinline__ YuvFrame yuv_frame(const ptx_yuv420p16_src& s, int n, int t) {
    YuvFrame f;                  // byte pointers: strides and pitches are in bytes
    f.y = reinterpret_cast<const unsigned char*>(s.y) + (int64_t)n * s.stride_n_y + (int64_t)t * s.stride_t_y;
    f.u = reinterpret_cast<const unsigned char*>(s.u) + (int64_t)n * s.stride_n_c + (int64_t)t * s.stride_t_c;
    f.v = reinterpret_cast<const unsigned char*>(s.v) + (int64_t)n * s.stride_n_c + (int64_t)t * s.stride_t_c;
    return f;
}

// Pixels [p0, min(p0 + 16, px_end)) of input row `row`; p0 is even and below px_end.
__device__ __forceinline__ void yuv_load_group(Yuv16Group& g, const ptx_yuv420p16_src& s, const YuvFrame& f, int row, int p0,
                                               int px_end) {
    const unsigned char* yp = f.y + (size_t)row * s.pitch_y + (size_t)p0 * 2;
    const size_t co = (size_t)(row >> 1) * s.pitch_c + (size_t)(p0 >> 1) * s.step_c;
    const int rem = px_end - p0;
    if (rem >= 16) {
        g.y0 = *reinterpret_cast<const u32x4_any*>(yp);
        g.y1 = *reinterpret_cast<const u32x4_any*>(yp + 16);
        if (s.step_c == 4) {
            const bool vu = f.v < f.u;                               // V first (P010 with swapped chroma)
            const unsigned char* cp = (vu ? f.v : f.u) + co;
            const u32x4 a = *reinterpret_cast<const u32x4_any*>(cp), b = *reinterpret_cast<const u32x4_any*>(cp + 16);
            const u32x4 e = {__builtin_amdgcn_perm(a.y, a.x, 0x05040100u), __builtin_amdgcn_perm(a.w, a.z, 0x05040100u),
                             __builtin_amdgcn_perm(b.y, b.x, 0x05040100u), __builtin_amdgcn_perm(b.w, b.z, 0x05040100u)};
            const u32x4 o = {__builtin_amdgcn_perm(a.y, a.x, 0x07060302u), __builtin_amdgcn_perm(a.w, a.z, 0x07060302u),
                             __builtin_amdgcn_perm(b.y, b.x, 0x07060302u), __builtin_amdgcn_perm(b.w, b.z, 0x07060302u)};
            g.u = vu ? o : e;
            g.v = vu ? e : o;
        } else {
            g.u = *reinterpret_cast<const u32x4_any*>(f.u + co);
            g.v = *reinterpret_cast<const u32x4_any*>(f.v + co);
        }
    } else {
        unsigned yy[8] = {0, 0, 0, 0, 0, 0, 0, 0}, uu[4] = {0, 0, 0, 0}, vv[4] = {0, 0, 0, 0};
#pragma unroll
        for (int k = 0; k < 16; ++k)
            if (k < rem) yy[k >> 1] |= (unsigned)*reinterpret_cast<const unsigned short*>(yp + 2 * k) << (16 * (k & 1));
        const int nc = (rem + 1) >> 1;
#pragma unroll
        for (int k = 0; k < 8; ++k)
            if (k < nc) {
                uu[k >> 1] |= (unsigned)*reinterpret_cast<const unsigned short*>(f.u + co + (size_t)k * s.step_c) << (16 * (k & 1));
                vv[k >> 1] |= (unsigned)*reinterpret_cast<const unsigned short*>(f.v + co + (size_t)k * s.step_c) << (16 * (k & 1));
            }
        g.y0 = u32x4{yy[0], yy[1], yy[2], yy[3]};
        g.y1 = u32x4{yy[4], yy[5], yy[6], yy[7]};
        g.u = u32x4{uu[0], uu[1], uu[2], uu[3]};
        g.v = u32x4{vv[0], vv[1], vv[2], vv[3]};
    }
}

// Converts the group and writes its RGB bytes to dst exactly as the 8-bit yuv_stage_group does.
__device__ __forceinline__ void yuv_stage_group(unsigned char* dst, const Yuv16Group& g, const ptx_yuv420p16_src& s, int rem) {
    const unsigned yw[8] = {g.y0.x, g.y0.y, g.y0.z, g.y0.w, g.y1.x, g.y1.y, g.y1.z, g.y1.w};
    const unsigned uw[4] = {g.u.x, g.u.y, g.u.z, g.u.w}, vw[4] = {g.v.x, g.v.y, g.v.z, g.v.w};
    const unsigned mask = (1u << s.bits) - 1u;
    const int d = s.bits - 8, mid = 128 << d, half = 1 << (15 + d), sh = 16 + d;
    // a negative sum gives 0, as in yuv_clip8: clamp below, unsigned shift, min
    auto clip = [&](int sum) { return min((unsigned)max(sum, 0) >> sh, 255u); };
    unsigned o[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};          // 16 x RGB, byte 3 p + c of the group in word (3 p + c) / 4
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int cb = (int)((uw[k >> 1] >> (16 * (k & 1) + s.shift)) & mask) - mid;
        const int cr = (int)((vw[k >> 1] >> (16 * (k & 1) + s.shift)) & mask) - mid;
        const int rv = __mul24(s.krv, cr) + half;
        const int gv = half - __mul24(s.kgu, cb) - __mul24(s.kgv, cr);
        const int bv = __mul24(s.kbu, cb) + half;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int p = 2 * k + h;
            const int yy = __mul24(s.ky, (int)((yw[k] >> (16 * h + s.shift)) & mask) - s.y_off);
            o[(3 * p) >> 2] |= clip(yy + rv) << (8 * ((3 * p) & 3));
            o[(3 * p + 1) >> 2] |= clip(yy + gv) << (8 * ((3 * p + 1) & 3));
            o[(3 * p + 2) >> 2] |= clip(yy + bv) << (8 * ((3 * p + 2) & 3));
        }
    }
    if (rem >= 16) {
#pragma unroll
        for (int q = 0; q < 3; ++q) *reinterpret_cast<u32x4*>(dst + 16 * q) = u32x4{o[4 * q], o[4 * q + 1], o[4 * q + 2], o[4 * q + 3]};
    } else {
#pragma unroll
        for (int j = 0; j < 12; ++j)
            if (4 * j < 3 * rem) *reinterpret_cast<unsigned*>(dst + 4 * j) = o[j];
    }
}

// Lane l owns groups l, 64 + l, ... as in the 8-bit form; the first kYuv16Prefetch of them are prefetched.
__device__ __forceinline__ void yuv_fetch_row(Yuv16Row& r, int i, int nrows, const ptx_yuv420p16_src& s, const YuvFrame& f,
                                              int lo0, int cmin, int px_end, int lane) {
    if (i >= nrows) return;
    const int e0 = cmin & ~1;
#pragma unroll
    for (int k = 0; k < kYuv16Prefetch; ++k)
        if (e0 + (64 * k + lane) * 16 < px_end) yuv_load_group(r.g[k], s, f, lo0 + i, e0 + (64 * k + lane) * 16, px_end);
}

__device__ __forceinline__ int yuv_stage_row(unsigned char* sw, const Yuv16Row& r, const ptx_yuv420p16_src& s, const YuvFrame& f,
                                             int row, int cmin, int px_end, int lane) {
    const int e0 = cmin & ~1;
    int p0 = e0 + lane * 16;
#pragma unroll
    for (int k = 0; k < kYuv16Prefetch; ++k, p0 += 64 * 16)
        if (p0 < px_end) yuv_stage_group(sw + (p0 - e0) * 3, r.g[k], s, px_end - p0);
    for (; p0 < px_end; p0 += 64 * 16) {
        Yuv16Group g;
        yuv_load_group(g, s, f, row, p0, px_end);
        yuv_stage_group(sw + (p0 - e0) * 3, g, s, px_end - p0);
    }
    return (cmin - e0) * 3;
}

// What a kernel of source flavour SRC takes: the descriptor, the per-clip row of the clips launch, the prefetched row.
template <int SRC> struct YuvSource {
    typedef ptx_yuv420_src Desc;
    typedef ptx_clip_src_yuv420 Clip;
    typedef YuvRow Row;
};
template <> struct YuvSource<kSrcYuv16> {
    typedef ptx_yuv420p16_src Desc;
    typedef ptx_clip_src_yuv420p16 Clip;
    typedef Yuv16Row Row;
};

// Host-side checks of a ptx_yuv420p16_src for N x T frames of H x W pixels (no device needed): yuv_check's, in bytes.
inline int yuv_check(const ptx_yuv420p16_src* s, int C, int H, int W, const char* who) {
    if (!s) return fail(PTX_ERR_INVALID, "%s: null source descriptor", who);
    if (C != 3) return fail(PTX_ERR_INVALID, "%s: C=%d, a YUV source converts to 3 channels", who, C);
    if (!s->y || !s->u || !s->v) return fail(PTX_ERR_INVALID, "%s: null plane pointer", who);
    if (s->bits != 10 && s->bits != 12) return fail(PTX_ERR_INVALID, "%s: bits=%d must be 10 or 12", who, s->bits);
    if (s->shift != 0 && s->shift != 16 - s->bits)
        return fail(PTX_ERR_INVALID, "%s: shift=%d must be 0 (LSB-aligned) or %d (MSB-aligned %d-bit samples)", who, s->shift,
                    16 - s->bits, s->bits);
    if (s->pitch_y <= 0 || s->pitch_c <= 0)
        return fail(PTX_ERR_INVALID, "%s: pitch_y=%d / pitch_c=%d must be positive", who, s->pitch_y, s->pitch_c);
    if (s->step_c != 2 && s->step_c != 4) return fail(PTX_ERR_INVALID, "%s: step_c=%d must be 2 (planar) or 4 (interleaved)", who, s->step_c);
    if (s->step_c == 4 && s->v != s->u + 1 && s->u != s->v + 1)
        return fail(PTX_ERR_INVALID, "%s: interleaved chroma (step_c=4) needs v == u + 1 (or u == v + 1)", who);
    if (((reinterpret_cast<uintptr_t>(s->y) | reinterpret_cast<uintptr_t>(s->u) | reinterpret_cast<uintptr_t>(s->v)) & 1) ||
        ((s->pitch_y | s->pitch_c) & 1) || ((s->stride_n_y | s->stride_t_y | s->stride_n_c | s->stride_t_c) & 1))
        return fail(PTX_ERR_INVALID, "%s: plane pointers, pitches and strides of 16-bit samples must be even", who);
    const int64_t Hc = ((int64_t)H + 1) / 2, Wc = ((int64_t)W + 1) / 2;
    if (s->pitch_y < (int64_t)W * 2 || s->pitch_c < Wc * s->step_c)
        return fail(PTX_ERR_INVALID, "%s: pitch_y=%d / pitch_c=%d are shorter than a row (%lld luma, %lld chroma bytes)", who,
                    s->pitch_y, s->pitch_c, (long long)W * 2, (long long)(Wc * s->step_c));
    if ((int64_t)H * s->pitch_y > INT32_MAX || Hc * s->pitch_c > INT32_MAX)
        return fail(PTX_ERR_UNSUPPORTED, "%s: a plane of a frame exceeds 32-bit indexing", who);
    return PTX_OK;
}

// Launch shape of resize_frames_u8_kernel, or the reason there is none.  taps_h is the widest row's tap count.  For a filter
// of support >= 1 (bilinear, Hamming, bicubic, Lanczos) a row of support s has more than 2 s - 1 taps, so output rows advance
// by at most taps_h / 2 input rows: a band of b output rows references at most b * taps_h / 2 + taps_h + 1 input rows (b when
// taps_h == 1: the axis is not resampled), and rows_of(b) below is that bound: the band is one chunk.
// It is NOT a bound for the two filters whose taps do not overlap: BOX (support 0.5: rows advance by about taps_h - 1, so a
// band references about b * (taps_h - 1) rows) and a one-tap NEAREST table of a down-scale (lo jumps by the scale while
// rows_of(b) = b).  Those stay correct because the kernel never relies on rows_of: its chunk loop (`while (r < y1)`) takes
// as many output rows as fit lds_rows intermediate rows and starts another chunk for the rest, and one output row always fits
// (n is clamped to lds_rows >= taps_h).  The cost is more, smaller chunks per band (a barrier pair each), and for NEAREST
// the horizontal pass also resamples the unreferenced input rows between two referenced ones, because a chunk stages the
// whole span [lo0, hi0).  Bilinear launch shapes are what they were.
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
