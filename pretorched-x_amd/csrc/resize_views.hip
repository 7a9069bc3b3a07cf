// Multi-view sampling of decoded video: uint8 [N][Tv][H][W][C] -> clips x crops views, resized + cropped with PIL's
// integer arithmetic (resize_common.h; the per-pixel work is resize_frames_u8_kernel's, so the bits are too).
//
// The host passes a device table of source frame indices [clips][T] and the row / column tables of ALL crop windows as
// "union" tables: the sorted distinct rows / columns of the resized frame that any window contains (Ur / Uc entries;
// window k is the run [row_off[k], row_off[k] + S) x [col_off[k], col_off[k] + S) of them).  Source frames are read in
// place through the index table (frame strides in bytes), so no gathered copy of the video exists anywhere.
//
// Two workgroup shapes:
//   shared     (sampled frame, band of UNION rows): one horizontal pass over the Uc union columns of the input rows the
//              band references, then the vertical pass writes the band's rows of every window that contains them.  A
//              landscape frame's windows share rows and differ in columns (Uc up to crops * S), a portrait frame's
//              share columns and differ in rows (bands run over the Ur union rows, each row resampled once).
//   per window (sampled frame, window, band of its S rows): resize_frames_u8_kernel's shape with the frame looked up
//              in the index table; taken when the union intermediate leaves no room in LDS, or where it measured
//              faster (views_plan: short input rows against a wide union).
// Only views [v0, v0 + nv) are written: y holds nv views per video (view v at slot v - v0).
#include "resize_common.h"

namespace ptx {

constexpr int kViewsMinSharedBand = 4;      // below this the shared pass re-reads too many halo rows: one window per workgroup

template <int C, int SRC = kSrcRgb>
__global__ void __launch_bounds__(256) resize_views_u8_kernel(ptx_views_desc d, const unsigned char* __restrict__ f,
                                                              const int* __restrict__ frame_idx,
                                                              const int* __restrict__ row_lo, const int* __restrict__ row_n,
                                                              const int* __restrict__ row_k, const int* __restrict__ col_lo,
                                                              const int* __restrict__ col_n, const int* __restrict__ col_k,
                                                              void* __restrict__ y, ptx_norm_desc nd, ResizePlan pl, int shared,
                                                              int clip0, int nclips, typename YuvSource<SRC>::Desc ys) {
    constexpr bool YUV = SRC != kSrcRgb;         // the source flavour, as in resize_frames_u8_kernel
    extern __shared__ __attribute__((aligned(16))) unsigned char views_smem[];
    int* hdr = reinterpret_cast<int*>(views_smem);                  // [0] first, [1] one-past-last referenced column
    const int Rn = shared ? d.Ur : d.S, Cn = shared ? d.Uc : d.S;   // rows / columns this launch shape resamples per frame
    int* t_clo = hdr + 4;                                           // clamped table entries: columns [Cn], [Cn] ...
    int* t_cn = t_clo + Cn;
    int* t_rlo = t_cn + Cn;                                         // ... and this band's rows [kResizeBand], [kResizeBand]
    int* t_rn = t_rlo + kResizeBand;
    int* t_k = reinterpret_cast<int*>(views_smem + pl.k_off);       // col_k [Cn][taps_w], then the band's row_k [band][taps_h]
    unsigned char* stage = views_smem + pl.stage_off;               // [4 waves][stage_stride]: one input row segment each
    unsigned char* inter = stage + 4 * pl.stage_stride;             // [lds_rows][istride] (+ 16 bytes): resampled rows

    // workgroup -> (video, clip, frame of the clip, [window], band); everything below is uniform over the workgroup
    const int bands = (Rn + pl.band - 1) / pl.band;
    int wg = xcd_remap((int)blockIdx.x, (int)gridDim.x);            // neighbouring bands share halo rows: same L2
    const int band_i = wg % bands;
    wg /= bands;
    int k0 = 0, k1 = d.crops;
    if (!shared) {
        k0 = wg % d.crops;
        k1 = k0 + 1;
        wg /= d.crops;
    }
    const int ti = wg % d.T;
    wg /= d.T;
    const int clip = clip0 + wg % nclips;
    const int n = wg / nclips;
    const int rbase = shared ? 0 : d.row_off[k0], cbase = shared ? 0 : d.col_off[k0];
    k0 = max(k0, d.v0 - clip * d.crops);                            // the windows of this clip inside the view range
    k1 = min(k1, d.v0 + d.nv - clip * d.crops);
    if (k0 >= k1) return;
    const int y0 = band_i * pl.band, y1 = min(y0 + pl.band, Rn);    // band of rows, relative to rbase
    {
        bool any = false;
        for (int k = k0; k < k1; ++k) any = any || (rbase + y0 < d.row_off[k] + d.S && rbase + y1 > d.row_off[k]);
        if (!any) return;                                           // union rows of windows outside the view range
    }
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int SC = d.S * C, istride = pl.istride;
    const int half = 1 << (kResizeBits - 1);
    const int src_t = min(max(frame_idx[clip * d.T + ti], 0), d.Tv - 1);
    const unsigned char* fin = YUV ? nullptr : f + (size_t)n * (size_t)d.stride_n + (size_t)src_t * (size_t)d.stride_t;
    const YuvFrame yf = YUV ? yuv_frame(ys, n, src_t) : YuvFrame{};      // a YUV source: the planes of ys, converted in the row staging
    row_lo += rbase + y0;
    row_n += rbase + y0;
    row_k += (size_t)(rbase + y0) * d.taps_h;
    col_lo += cbase;
    col_n += cbase;
    col_k += (size_t)cbase * d.taps_w;

    if (tid == 0) {
        hdr[0] = d.W;
        hdr[1] = 0;
    }
    __syncthreads();
    {
        int cmin = d.W, cmax = 0;
        for (int x = tid; x < Cn; x += 256) {
            int lo, nn;
            resize_entry(col_lo, col_n, x, d.W, d.taps_w, lo, nn);
            t_clo[x] = lo;
            t_cn[x] = nn;
            cmin = min(cmin, lo);
            cmax = max(cmax, lo + nn);
        }
        atomicMin(&hdr[0], cmin);
        atomicMax(&hdr[1], cmax);
        for (int i = tid; i < y1 - y0; i += 256) {
            int lo, nn;
            resize_entry(row_lo, row_n, i, d.H, min(d.taps_h, pl.lds_rows), lo, nn);
            t_rlo[i] = lo;
            t_rn[i] = nn;
        }
        if (pl.k_in_lds) {
            const int nck = Cn * d.taps_w, nrk = (y1 - y0) * d.taps_h;
            for (int i = tid; i < nck; i += 256) t_k[i] = col_k[i];
            for (int i = tid; i < nrk; i += 256) t_k[nck + i] = row_k[i];
        }
    }
    __syncthreads();
    const int* ck = pl.k_in_lds ? t_k : col_k;                      // [Cn][taps_w]
    const int* rk = pl.k_in_lds ? t_k + Cn * d.taps_w : row_k;      // [y1 - y0][taps_h]
    const int cmin = hdr[0];
    const int span_bytes = max(hdr[1] - cmin, 0) * C;               // <= W * C
    const int px_end = max(hdr[1], cmin);                           // one past the last referenced column

    int r = y0;
    while (r < y1) {
        // the chunk [r, r1) of rows whose referenced input rows [lo0, hi0) fit the intermediate image
        int lo0 = t_rlo[r - y0];
        int hi0 = lo0 + t_rn[r - y0], r1 = r + 1;
        while (r1 < y1) {
            const int lo = t_rlo[r1 - y0], nn = t_rn[r1 - y0];
            const int l2 = min(lo0, lo), h2 = max(hi0, lo + nn);
            if (h2 - l2 > pl.lds_rows) break;
            lo0 = l2;
            hi0 = h2;
            ++r1;
        }
        const int nrows = hi0 - lo0;

        // horizontal pass (as resize_frames_u8_kernel): wave w resamples input rows lo0 + w, lo0 + w + 4, ..., the next
        // row's bytes already on their way in registers
        unsigned char* sw = stage + wave * pl.stage_stride;
        ResizeRow pre = {};
        typename YuvSource<SRC>::Row ypre = {};
        if constexpr (YUV) yuv_fetch_row(ypre, 0 + wave, nrows, ys, yf, lo0, cmin, px_end, lane);
        else resize_fetch_row(pre, 0 + wave, nrows, fin, lo0, d.W, cmin, C, span_bytes, lane);
        for (int i0 = 0; i0 < nrows; i0 += 4) {
            const int i = i0 + wave;
            int off = 0;
            if constexpr (YUV) {
                if (i < nrows) off = yuv_stage_row(sw, ypre, ys, yf, lo0 + i, cmin, px_end, lane);
            } else if (i < nrows) {
                int vb, ve, end;
                const unsigned char* g = resize_row_span(fin, lo0 + i, d.W, cmin, C, span_bytes, off, vb, ve, end);
                if (lane < vb - off) sw[off + lane] = (unsigned char)pre.head;
                if (vb + lane * 16 < ve) *reinterpret_cast<u32x4*>(sw + vb + lane * 16) = pre.v0;
                if (vb + (64 + lane) * 16 < ve) *reinterpret_cast<u32x4*>(sw + vb + (64 + lane) * 16) = pre.v1;
                if (vb + (128 + lane) * 16 < ve) *reinterpret_cast<u32x4*>(sw + vb + (128 + lane) * 16) = pre.v2;
                for (int v = vb + (192 + lane) * 16; v < ve; v += 64 * 16)
                    *reinterpret_cast<uint4*>(sw + v) = *reinterpret_cast<const uint4*>(g + v);
                if (lane < end - ve) sw[ve + lane] = (unsigned char)pre.tail;
            }
            __syncthreads();
            if constexpr (YUV) yuv_fetch_row(ypre, i + 4, nrows, ys, yf, lo0, cmin, px_end, lane);
            else resize_fetch_row(pre, i + 4, nrows, fin, lo0, d.W, cmin, C, span_bytes, lane);
            if (i < nrows) {
                for (int x = lane; x < Cn; x += 64) {
                    const int lo = t_clo[x], nn = t_cn[x];
                    const unsigned char* p = sw + off + (lo - cmin) * C;
                    const int* kk = ck + x * d.taps_w;
                    int acc[C];
#pragma unroll
                    for (int c = 0; c < C; ++c) acc[c] = half;
#pragma unroll 4
                    for (int j = 0; j < nn; ++j) {
                        const int k = kk[j];
#pragma unroll
                        for (int c = 0; c < C; ++c) acc[c] += __mul24(k, (int)p[j * C + c]);
                    }
#pragma unroll
                    for (int c = 0; c < C; ++c) inter[i * istride + x * C + c] = (unsigned char)clip8(acc[c] >> kResizeBits);
                }
            }
        }
        __syncthreads();

        // vertical pass: rows [r, r1) of every live window that contains them
        for (int k = k0; k < k1; ++k) {
            const int wr = d.row_off[k] - rbase;                     // the window's first row, relative to rbase
            const int a = max(r, wr), b = min(r1, wr + d.S);
            if (a >= b) continue;
            const int nout = b - a;
            const int cb = (d.col_off[k] - cbase) * C;               // byte offset of the window's first column in a row
            const size_t view = (size_t)n * d.nv + (size_t)(clip * d.crops + k - d.v0);
            if (d.out_mode == PTX_RESIZE_OUT_U8) {
                unsigned char* yo = static_cast<unsigned char*>(y) + (view * d.T + ti) * (size_t)d.S * SC;
                const int q4 = (SC + 3) / 4;                         // 4 interleaved bytes per thread
                const int sh = cb & 3;                               // the window may start at any byte of an LDS word
                for (int it = tid; it < nout * q4; it += 256) {
                    const int yy = it / q4, q = it - yy * q4, row = a + yy;
                    const int lo = t_rlo[row - y0], nn = t_rn[row - y0];
                    const unsigned char* p = inter + (lo - lo0) * istride + (cb - sh) + q * 4;
                    const int* kk = rk + (row - y0) * d.taps_h;
                    int acc[4] = {half, half, half, half};
                    for (int j = 0; j < nn; ++j) {
                        const int kc = kk[j];
                        unsigned v = *reinterpret_cast<const unsigned*>(p + j * istride);
                        if (sh) v = __builtin_amdgcn_alignbyte(*reinterpret_cast<const unsigned*>(p + j * istride + 4), v, sh);
#pragma unroll
                        for (int e = 0; e < 4; ++e) acc[e] += __mul24(kc, (int)((v >> (8 * e)) & 255u));
                    }
                    // a negative sum (negative coefficients) gives 0, and no packed shift-and-saturate: see resize_clip8
                    unsigned o = 0;
#pragma unroll
                    for (int e = 0; e < 4; ++e) o |= resize_clip8(acc[e]) << (8 * e);
                    unsigned char* ob = yo + (size_t)(row - wr) * SC + q * 4;
                    if (pl.vec_store) {
                        *reinterpret_cast<unsigned*>(ob) = o;
                    } else {
#pragma unroll
                        for (int e = 0; e < 4; ++e)
                            if (q * 4 + e < SC) ob[e] = (unsigned char)(o >> (8 * e));
                    }
                }
            } else {
                const int Wg = (d.S + 3) / 4;                        // 4 pixels of one plane row per thread
                for (int it = tid; it < nout * C * Wg; it += 256) {
                    const int xg = it % Wg, t2 = it / Wg;
                    const int c = t2 % C, row = a + t2 / C;
                    const int cin = (nd.swap_rb && (c == 0 || c == 2)) ? 2 - c : c;
                    const int lo = t_rlo[row - y0], nn = t_rn[row - y0];
                    const unsigned char* p = inter + (lo - lo0) * istride + cb + cin;
                    const int* kk = rk + (row - y0) * d.taps_h;
                    int xo[4];
#pragma unroll
                    for (int e = 0; e < 4; ++e) xo[e] = min(xg * 4 + e, d.S - 1) * C;
                    int acc[4] = {half, half, half, half};
                    for (int j = 0; j < nn; ++j) {
                        const int kc = kk[j];
#pragma unroll
                        for (int e = 0; e < 4; ++e) acc[e] += __mul24(kc, (int)p[j * istride + xo[e]]);
                    }
                    float v[4];
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        v[e] = normalise_u8((unsigned char)clip8(acc[e] >> kResizeBits), nd.mean[c], nd.std[c], nd.to_255);
                    const size_t o = (((view * C + c) * d.T + ti) * d.S + (size_t)(row - wr)) * d.S + (size_t)xg * 4;
                    if (d.out_mode == PTX_RESIZE_OUT_F32) {
                        float* yo = static_cast<float*>(y) + o;
                        if (pl.vec_store) {
                            f32x4 q = {v[0], v[1], v[2], v[3]};
                            *reinterpret_cast<f32x4*>(yo) = q;
                        } else {
#pragma unroll
                            for (int e = 0; e < 4; ++e)
                                if (xg * 4 + e < d.S) yo[e] = v[e];
                        }
                    } else {
                        __bf16* yo = static_cast<__bf16*>(y) + o;
                        unsigned short bb[4];
#pragma unroll
                        for (int e = 0; e < 4; ++e) bb[e] = __builtin_bit_cast(unsigned short, (__bf16)v[e]);   // nearest even
                        if (pl.vec_store) {
                            uint2 q = {(unsigned)bb[0] | ((unsigned)bb[1] << 16), (unsigned)bb[2] | ((unsigned)bb[3] << 16)};
                            *reinterpret_cast<uint2*>(yo) = q;
                        } else {
#pragma unroll
                            for (int e = 0; e < 4; ++e)
                                if (xg * 4 + e < d.S) reinterpret_cast<unsigned short*>(yo)[e] = bb[e];
                        }
                    }
                }
            }
        }
        __syncthreads();                                             // the next chunk overwrites the intermediate image
        r = r1;
    }
}

// Launch shape, or the reason there is none.  *shared: 1 = one workgroup per (frame, band of union rows), 0 = per window.
static int views_plan(const ptx_views_desc* d, const void* y, ResizePlan* p, int* shared, const char* who,
                      const ptx_yuv420_src* src = nullptr, const ptx_yuv420p16_src* src16 = nullptr) {
    if (!d) return fail(PTX_ERR_INVALID, "%s: null descriptor", who);
    if (d->N <= 0 || d->Tv <= 0 || d->H <= 0 || d->W <= 0 || d->S <= 0 || d->clips <= 0 || d->T <= 0)
        return fail(PTX_ERR_INVALID, "%s: non-positive extent (N=%d Tv=%d H=%d W=%d S=%d clips=%d T=%d)", who, d->N, d->Tv, d->H,
                    d->W, d->S, d->clips, d->T);
    if (d->C <= 0 || d->C > 4) return fail(PTX_ERR_INVALID, "%s: C=%d must be 1..4", who, d->C);
    if (d->crops <= 0 || d->crops > PTX_VIEWS_MAX_CROPS)
        return fail(PTX_ERR_INVALID, "%s: crops=%d must be 1..%d", who, d->crops, PTX_VIEWS_MAX_CROPS);
    if (d->share < PTX_VIEWS_SHARE_AUTO || d->share > PTX_VIEWS_SHARE_NEVER)
        return fail(PTX_ERR_INVALID, "%s: share=%d is not a PTX_VIEWS_SHARE_* value", who, d->share);
    const int64_t frame_bytes = (int64_t)d->H * d->W * d->C;
    if (src) {                                                       // the source addresses its frames itself: d's strides are not read
        if (int s = yuv_check(src, d->C, d->H, d->W, who)) return s;
    } else if (src16) {
        if (int s = yuv_check(src16, d->C, d->H, d->W, who)) return s;
    } else if (d->stride_t < frame_bytes || d->stride_n < frame_bytes)
        return fail(PTX_ERR_INVALID, "%s: stride_t=%lld / stride_n=%lld are smaller than a frame (%lld bytes)", who,
                    (long long)d->stride_t, (long long)d->stride_n, (long long)frame_bytes);
    const int64_t V = (int64_t)d->clips * d->crops;
    if (d->v0 < 0 || d->nv <= 0 || (int64_t)d->v0 + d->nv > V)
        return fail(PTX_ERR_INVALID, "%s: view range [%d, %d + %d) is outside the %lld views", who, d->v0, d->v0, d->nv, (long long)V);
    if (d->Ur < d->S || d->Uc < d->S) return fail(PTX_ERR_INVALID, "%s: Ur=%d / Uc=%d hold less than one window (S=%d)", who, d->Ur, d->Uc, d->S);
    for (int k = 0; k < d->crops; ++k)
        if (d->row_off[k] < 0 || d->col_off[k] < 0 || (int64_t)d->row_off[k] + d->S > d->Ur || (int64_t)d->col_off[k] + d->S > d->Uc)
            return fail(PTX_ERR_INVALID, "%s: window %d (row_off=%d, col_off=%d) leaves the union tables (Ur=%d, Uc=%d)", who, k,
                        d->row_off[k], d->col_off[k], d->Ur, d->Uc);
    if ((int64_t)d->clips * d->T > INT32_MAX || V > INT32_MAX || (int64_t)d->N * d->nv > INT32_MAX)
        return fail(PTX_ERR_UNSUPPORTED, "%s: too many views", who);
    // resize_plan validates the rest (taps, out_mode, 32-bit frames) and carves LDS for a Ho x Wo resample of one frame
    ptx_resize_desc one = {1, 1, d->H, d->W, d->C, d->Ur, d->Uc, d->taps_h, d->taps_w, d->out_mode};
    int s = PTX_ERR_UNSUPPORTED;
    *shared = 0;
    if (d->share != PTX_VIEWS_SHARE_NEVER && d->crops > 1) {
        s = resize_plan(&one, y, p, who);
        if (s == PTX_ERR_INVALID) return s;
        // Measured: the shared pass wins where the windows differ in rows only (portrait: nothing is given
        // up for it) and where the input rows are long against the union (720x1280 -> 455 columns: every window would
        // stage most of each 3840-byte row again); on 360x640 its 55 KB of LDS per workgroup (32 KB per window) leave two
        // workgroups per CU where five fit, and one window per workgroup is 8 % faster.  One window per workgroup also
        // keeps a full band where the union image would leave only a sliver of LDS.
        const bool pays = d->Uc == d->S || d->W >= 2 * d->Uc;
        *shared = s == PTX_OK && (d->share == PTX_VIEWS_SHARE_ALWAYS || (pays && p->band >= std::min(kViewsMinSharedBand, d->Ur)));
        if (d->share == PTX_VIEWS_SHARE_ALWAYS && s != PTX_OK) return s;
    }
    if (!*shared) {
        one.Ho = one.Wo = d->S;
        s = resize_plan(&one, y, p, who);
        if (s) return s;
    }
    const int64_t frames = (int64_t)d->N * (cdiv(d->v0 + d->nv, d->crops) - d->v0 / d->crops) * d->T;
    if (frames * (*shared ? 1 : d->crops) * cdiv(*shared ? d->Ur : d->S, p->band) > INT32_MAX)
        return fail(PTX_ERR_UNSUPPORTED, "%s: too many workgroups", who);
    const uintptr_t ya = reinterpret_cast<uintptr_t>(y);
    p->vec_store = d->out_mode == PTX_RESIZE_OUT_U8 ? ((d->S * d->C) % 4 == 0 && ya % 4 == 0)
                                                    : (d->S % 4 == 0 && ya % (d->out_mode == PTX_RESIZE_OUT_F32 ? 16 : 8) == 0);
    p->lds_bytes += 16;      // the uint8 vertical pass reads the word after a window's last one (shifted out again)
    return PTX_OK;
}

}  // namespace ptx

using namespace ptx;

extern "C" int ptx_resize_views_u8_supported(const ptx_views_desc* desc) {
    ResizePlan p;
    int shared;
    if (views_plan(desc, nullptr, &p, &shared, "ptx_resize_views_u8_supported") != PTX_OK) return 0;
    return shared ? 2 : 1;
}

// All sources: `video` (interleaved uint8) or, when src / src16 is not null, the planes of a YUV 4:2:0 source.
static int resize_views_run(const ptx_views_desc* desc, const uint8_t* video, const ptx_yuv420_src* src, const int32_t* frame_idx,
                            const int32_t* row_lo, const int32_t* row_n, const int32_t* row_k, const int32_t* col_lo,
                            const int32_t* col_n, const int32_t* col_k, void* y, const ptx_norm_desc* norm, ptx_stream_t stream,
                            const char* who, const ptx_yuv420p16_src* src16 = nullptr) {
    ResizePlan p;
    int shared;
    int s = views_plan(desc, y, &p, &shared, who, src, src16);
    if (s) return s;
    if ((!video && !src && !src16) || !frame_idx || !y || !row_lo || !row_n || !row_k || !col_lo || !col_n || !col_k)
        return fail(PTX_ERR_INVALID, "%s: null pointer", who);
    ptx_norm_desc nd = {};
    if (desc->out_mode != PTX_RESIZE_OUT_U8) {
        if (!norm) return fail(PTX_ERR_INVALID, "%s: null norm descriptor", who);
        for (int c = 0; c < desc->C; ++c)
            if (!(norm->std[c] != 0.f)) return fail(PTX_ERR_INVALID, "%s: std[%d] must be non-zero", who, c);
        if (norm->swap_rb && desc->C < 3) return fail(PTX_ERR_INVALID, "%s: BGR swap needs 3 channels", who);
        nd = *norm;
    }
    const int clip0 = desc->v0 / desc->crops, nclips = cdiv(desc->v0 + desc->nv, desc->crops) - clip0;
    const int64_t wgs = (int64_t)desc->N * nclips * desc->T * (shared ? 1 : desc->crops) * cdiv(shared ? desc->Ur : desc->S, p.band);
    const dim3 grid((unsigned)wgs);
    hipStream_t st = (hipStream_t)stream;
#define PTX_VIEWS_LAUNCH(CH)                                                                                                \
    hipLaunchKernelGGL(resize_views_u8_kernel<CH>, grid, dim3(256), p.lds_bytes, st, *desc, video, frame_idx, row_lo, row_n, \
                       row_k, col_lo, col_n, col_k, y, nd, p, shared, clip0, nclips, ptx_yuv420_src{})
    if (src16) {
        hipLaunchKernelGGL((resize_views_u8_kernel<3, kSrcYuv16>), grid, dim3(256), p.lds_bytes, st, *desc, (const unsigned char*)nullptr,
                           frame_idx, row_lo, row_n, row_k, col_lo, col_n, col_k, y, nd, p, shared, clip0, nclips, *src16);
        return hip_check(hipGetLastError(), who);
    }
    if (src) {
        hipLaunchKernelGGL((resize_views_u8_kernel<3, kSrcYuv8>), grid, dim3(256), p.lds_bytes, st, *desc, (const unsigned char*)nullptr, frame_idx, row_lo,
                           row_n, row_k, col_lo, col_n, col_k, y, nd, p, shared, clip0, nclips, *src);
        return hip_check(hipGetLastError(), who);
    }
    switch (desc->C) {
        case 1: PTX_VIEWS_LAUNCH(1); break;
        case 2: PTX_VIEWS_LAUNCH(2); break;
        case 3: PTX_VIEWS_LAUNCH(3); break;
        default: PTX_VIEWS_LAUNCH(4); break;
    }
#undef PTX_VIEWS_LAUNCH
    return hip_check(hipGetLastError(), "ptx_resize_views_u8 launch");
}

extern "C" int ptx_resize_views_u8(const ptx_views_desc* desc, const uint8_t* video, const int32_t* frame_idx,
                                   const int32_t* row_lo, const int32_t* row_n, const int32_t* row_k, const int32_t* col_lo,
                                   const int32_t* col_n, const int32_t* col_k, void* y, const ptx_norm_desc* norm,
                                   ptx_stream_t stream) {
    return resize_views_run(desc, video, nullptr, frame_idx, row_lo, row_n, row_k, col_lo, col_n, col_k, y, norm, stream,
                            "ptx_resize_views_u8");
}

extern "C" int ptx_resize_views_yuv420_supported(const ptx_views_desc* desc, const ptx_yuv420_src* src) {
    const char* who = "ptx_resize_views_yuv420_supported";
    ResizePlan p;
    int shared;
    if (!src) return fail(PTX_ERR_INVALID, "%s: null source descriptor", who), 0;
    if (views_plan(desc, nullptr, &p, &shared, who, src) != PTX_OK) return 0;
    return shared ? 2 : 1;
}

extern "C" int ptx_resize_views_yuv420(const ptx_views_desc* desc, const ptx_yuv420_src* src, const int32_t* frame_idx,
                                       const int32_t* row_lo, const int32_t* row_n, const int32_t* row_k, const int32_t* col_lo,
                                       const int32_t* col_n, const int32_t* col_k, void* y, const ptx_norm_desc* norm,
                                       ptx_stream_t stream) {
    const char* who = "ptx_resize_views_yuv420";
    if (!src) return fail(PTX_ERR_INVALID, "%s: null source descriptor", who);
    return resize_views_run(desc, nullptr, src, frame_idx, row_lo, row_n, row_k, col_lo, col_n, col_k, y, norm, stream, who);
}

// The same on a 10- / 12-bit source (include/ptx_amd_yuv16.h).
extern "C" int ptx_resize_views_yuv420p16_supported(const ptx_views_desc* desc, const ptx_yuv420p16_src* src) {
    const char* who = "ptx_resize_views_yuv420p16_supported";
    ResizePlan p;
    int shared;
    if (!src) return fail(PTX_ERR_INVALID, "%s: null source descriptor", who), 0;
    if (views_plan(desc, nullptr, &p, &shared, who, nullptr, src) != PTX_OK) return 0;
    return shared ? 2 : 1;
}

extern "C" int ptx_resize_views_yuv420p16(const ptx_views_desc* desc, const ptx_yuv420p16_src* src, const int32_t* frame_idx,
                                          const int32_t* row_lo, const int32_t* row_n, const int32_t* row_k,
                                          const int32_t* col_lo, const int32_t* col_n, const int32_t* col_k, void* y,
                                          const ptx_norm_desc* norm, ptx_stream_t stream) {
    const char* who = "ptx_resize_views_yuv420p16";
    if (!src) return fail(PTX_ERR_INVALID, "%s: null source descriptor", who);
    return resize_views_run(desc, nullptr, nullptr, frame_idx, row_lo, row_n, row_k, col_lo, col_n, col_k, y, norm, stream, who, src);
}
