// Load-time weight packing (BN fold + K-major relayout) and the layout transforms at the API edge.
// All of these are HBM-bound byte movers: coalesced 16-byte accesses on the channels-last side,
// LDS tile transposes where both sides cannot be contiguous at once.
#include "ptx_common.h"
#include "resize_common.h"
#include <algorithm>

namespace ptx {

thread_local char g_last_error[512] = "";
char* last_error_buf() { return g_last_error; }

// ---------------------------------------------------------------------------------------------
// weight packing
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ float bn_scale(const float* gamma, const float* var, float eps, int co) {
    return gamma ? gamma[co] * (1.0f / sqrtf(var[co] + eps)) : 1.0f;
}

__global__ void __launch_bounds__(256) pack_weight_kernel(ptx_pack_desc d, const float* __restrict__ w,
                                                          const float* __restrict__ gamma,
                                                          const float* __restrict__ var, float eps,
                                                          float* __restrict__ out, size_t total) {
    const int taps_hw = d.kH * d.kW;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const int k = (int)(i % d.Kc);
        size_t t = i / d.Kc;
        const int co = (int)(t % d.Co_pad);
        const int tap = (int)(t / d.Co_pad);
        int kt, kh, kw, c;
        bool valid = co < d.Co;
        if (d.fold_kw) {
            kt = tap / d.kH;
            kh = tap % d.kH;
            kw = k / d.Ci;
            c = k % d.Ci;
            valid = valid && k < d.kW * d.Ci;
        } else {
            kt = tap / taps_hw;
            const int r = tap % taps_hw;
            kh = r / d.kW;
            kw = r % d.kW;
            c = k;
            valid = valid && k < d.Ci;
        }
        int ci_src = d.Ci;                 // channels per filter row in the source tensor
        if (d.sub_groups > 1 && valid) {
            // block-diagonal super-group: row co keeps only the columns of its own real group
            ci_src = d.Ci / d.sub_groups;
            const int cog = d.co_per_super / d.sub_groups;      // output channels per real group
            const int g_row = (co % d.co_per_super) / cog, g_col = c / ci_src;
            valid = g_row == g_col;
            c -= g_col * ci_src;
        }
        float v = 0.f;
        if (valid) {
            const size_t src = ((((size_t)co * ci_src + c) * d.kT + kt) * d.kH + kh) * d.kW + kw;
            v = w[src] * bn_scale(gamma, var, eps, co);
        }
        const size_t ld = d.ld_k > 0 ? (size_t)d.ld_k : (size_t)d.Kc;
        const size_t dst = ((size_t)tap * d.Co_pad + co) * ld + d.k_off + k;
        if (d.f16 == 2) {
            // split operands (PTX_F16X3_OPERANDS): the 8-channel block of column k holds 8 hi halfs then 8 lo halfs
            const size_t row_h = (((size_t)tap * d.Co_pad + co) * ld + d.k_off) * 2;      // row start, in halfs
            const _Float16 hi = (_Float16)v;
            const _Float16 lo = (_Float16)((v - (float)hi) * 4096.f);       // scaled lo: a normal half whenever hi is one
            _Float16* o = reinterpret_cast<_Float16*>(out) + row_h + (size_t)(k >> 3) * 16 + (k & 7);
            o[0] = hi;
            o[8] = lo;
        } else if (d.f16 == 3) reinterpret_cast<__bf16*>(out)[dst] = (__bf16)v;       // bf16: one rounding of the folded value
        else if (d.f16) reinterpret_cast<_Float16*>(out)[dst] = (_Float16)v;     // round-to-nearest-even
        else out[dst] = v;
    }
}

__global__ void pack_bias_kernel(int Co, int Co_pad, const float* __restrict__ conv_bias,
                                 const float* __restrict__ gamma, const float* __restrict__ beta,
                                 const float* __restrict__ mean, const float* __restrict__ var, float eps,
                                 float* __restrict__ out, int accumulate) {
    const int co = blockIdx.x * blockDim.x + threadIdx.x;
    if (co >= Co_pad) return;
    float b = 0.f;
    if (co < Co) {
        const float s = bn_scale(gamma, var, eps, co);
        const float cb = conv_bias ? conv_bias[co] : 0.f;
        const float mu = mean ? mean[co] : 0.f;
        b = (beta ? beta[co] : 0.f) + (cb - mu) * s;
    }
    out[co] = accumulate ? out[co] + b : b;
}

// ---------------------------------------------------------------------------------------------
// [N][C][S] <-> [N][S][ld] tile transposes (32 x 32 floats through LDS, +1 pad)
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) ncs_to_nsc_kernel(const float* __restrict__ x, float* __restrict__ y, int C,
                                                         long long S, int ld) {
    __shared__ float tile[32][33];
    const int n = blockIdx.z;
    const long long s0 = (long long)blockIdx.x * 32;
    const int c0 = blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;   // 32 x 8
    const float* xn = x + (size_t)n * C * S;
    float* yn = y + (size_t)n * S * ld;
#pragma unroll
    for (int j = 0; j < 32; j += 8) {
        const int c = c0 + ty + j;
        const long long s = s0 + tx;
        tile[ty + j][tx] = (c < C && s < S) ? xn[(size_t)c * S + s] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 32; j += 8) {
        const long long s = s0 + ty + j;
        const int c = c0 + tx;
        if (s < S && c < ld) yn[(size_t)s * ld + c] = tile[tx][ty + j];   // zero beyond C by construction
    }
}

__global__ void __launch_bounds__(256) nsc_to_ncs_kernel(const float* __restrict__ x, float* __restrict__ y, int C,
                                                         long long S, int ld) {
    __shared__ float tile[32][33];
    const int n = blockIdx.z;
    const long long s0 = (long long)blockIdx.x * 32;
    const int c0 = blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const float* xn = x + (size_t)n * S * ld;
    float* yn = y + (size_t)n * C * S;
#pragma unroll
    for (int j = 0; j < 32; j += 8) {
        const long long s = s0 + ty + j;
        const int c = c0 + tx;
        tile[ty + j][tx] = (s < S && c < C) ? xn[(size_t)s * ld + c] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 32; j += 8) {
        const int c = c0 + ty + j;
        const long long s = s0 + tx;
        if (c < C && s < S) yn[(size_t)c * S + s] = tile[tx][ty + j];
    }
}

// y[b][c][r] = x[b][r][c]; rows r in [R, ldy) of y are zero-filled
__global__ void __launch_bounds__(256) transpose_last2_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                              int R, int Cc, int ldx, int ldy) {
    __shared__ float tile[32][33];
    const int b = blockIdx.z;
    const int r0 = blockIdx.x * 32, c0 = blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const float* xb = x + (size_t)b * R * ldx;
    float* yb = y + (size_t)b * Cc * ldy;
#pragma unroll
    for (int j = 0; j < 32; j += 8) {
        const int r = r0 + ty + j, c = c0 + tx;
        tile[ty + j][tx] = (r < R && c < Cc) ? xb[(size_t)r * ldx + c] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 32; j += 8) {
        const int c = c0 + ty + j, r = r0 + tx;
        if (c < Cc && r < ldy) yb[(size_t)c * ldy + r] = tile[tx][ty + j];
    }
}

// ---------------------------------------------------------------------------------------------
// small-Cin stem: NCDHW -> [N][T][H][Wo][ld] with the kW taps folded into the channel axis.
// One workgroup per input row (n, t, h): the C channel rows are staged in LDS with coalesced
// loads, then the Wo x ld output row (contiguous in memory) is written as float4s.  A thread's
// float4 column q is fixed, so its four (kw, c) pairs are decoded once.
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) fold_kw_kernel(const float* __restrict__ x, float* __restrict__ y, int C,
                                                      int T, int H, int W, long long stride_n, long long stride_c,
                                                      long long stride_t, int kW, int sW, int pW, int Wo, int ld) {
    extern __shared__ float rowbuf[];      // [C][W]
    const int h = blockIdx.x % H;
    const int t = (blockIdx.x / H) % T;
    const int n = blockIdx.x / (H * T);
    const float* xin = x + (size_t)n * stride_n + (size_t)t * stride_t + (size_t)h * W;
    for (int i = threadIdx.x; i < C * W; i += 256) {
        const int c = i / W, w = i - c * W;
        rowbuf[i] = xin[(size_t)c * stride_c + w];
    }
    __syncthreads();
    const int f4r = ld / 4;
    const int rows_per_pass = 256 / f4r;
    const int q = threadIdx.x % f4r;
    const int r0 = threadIdx.x / f4r;
    if (r0 >= rows_per_pass) return;
    int off[4], kwp[4];
    bool live[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int k = q * 4 + e;
        const int kw = k / C, c = k - kw * C;
        live[e] = k < kW * C;
        kwp[e] = kw - pW;
        off[e] = c * W + kw - pW;          // + wo * sW gives the LDS index of (c, wo*sW - pW + kw)
    }
    float* yrow = y + (size_t)blockIdx.x * Wo * ld;
    for (int wo = r0; wo < Wo; wo += rows_per_pass) {
        float v[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int wi = wo * sW + kwp[e];                  // input column of this tap
            v[e] = (live[e] && wi >= 0 && wi < W) ? rowbuf[off[e] + wo * sW] : 0.f;
        }
        f32x4 o = {v[0], v[1], v[2], v[3]};
        *reinterpret_cast<f32x4*>(yrow + (size_t)wo * ld + q * 4) = o;
    }
}

// ---------------------------------------------------------------------------------------------
// uint8 frames [N][T][H][W][C] -> normalised fp32 (TransformImage's tensor half, utils.py:72-75).
// The fp32 operations and their order are the reference's (ToTensor /255, ToRange255 *255,
// Normalize (v - mean) / std); the _rn intrinsics keep the compiler from contracting them into FMAs
// or reciprocal multiplies, so the result is bit-identical to the CPU tensors.
// ---------------------------------------------------------------------------------------------

__global__ void __launch_bounds__(256) frames_u8_to_ncdhw_kernel(const unsigned char* __restrict__ f, float* __restrict__ y,
                                                                 size_t total, int C, long long THW, ptx_norm_desc nd) {
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
        const size_t s = e % (size_t)THW;              // (t, h, w)
        const size_t nc = e / (size_t)THW;
        const int c = (int)(nc % C);
        const size_t n = nc / C;
        const int cin = (nd.swap_rb && (c == 0 || c == 2)) ? 2 - c : c;
        y[e] = normalise_u8(f[(n * THW + s) * C + cin], nd.mean[c], nd.std[c], nd.to_255);
    }
}

// one block per (n, t, h) input row: W*C bytes -> normalised floats in LDS (kept channel-interleaved, so
// the folded row of output column wo is the contiguous run rowbuf[(wo*sW - pW)*C ...][0, kW*C)).
__global__ void __launch_bounds__(256) fold_kw_frames_u8_kernel(const unsigned char* __restrict__ f, float* __restrict__ y,
                                                                int C, int T, int H, int W, int frame_step, int T_full,
                                                                int kW, int sW, int pW, int Wo, int ld, ptx_norm_desc nd) {
    extern __shared__ float rowbuf[];      // [W][C]
    const int h = blockIdx.x % H;
    const int t = (blockIdx.x / H) % T;
    const int n = blockIdx.x / (H * T);
    const unsigned char* fin = f + ((((size_t)n * T_full + (size_t)t * frame_step) * H + h) * W) * C;
    for (int i = threadIdx.x; i < W * C; i += 256) {
        const int w = i / C, c = i - w * C;
        const int cin = (nd.swap_rb && (c == 0 || c == 2)) ? 2 - c : c;
        rowbuf[i] = normalise_u8(fin[w * C + cin], nd.mean[c], nd.std[c], nd.to_255);
    }
    __syncthreads();
    const int f4r = ld / 4;
    const int rows_per_pass = 256 / f4r;
    const int q = threadIdx.x % f4r;
    const int r0 = threadIdx.x / f4r;
    if (r0 >= rows_per_pass) return;
    float* yrow = y + (size_t)blockIdx.x * Wo * ld;
    for (int wo = r0; wo < Wo; wo += rows_per_pass) {
        const int base = (wo * sW - pW) * C;           // rowbuf index of folded column 0 (may be negative)
        float v[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int k = q * 4 + e;
            const int idx = base + k;
            v[e] = (k < kW * C && idx >= 0 && idx < W * C) ? rowbuf[idx] : 0.f;
        }
        f32x4 o = {v[0], v[1], v[2], v[3]};
        *reinterpret_cast<f32x4*>(yrow + (size_t)wo * ld + q * 4) = o;
    }
}

// ---------------------------------------------------------------------------------------------
// uint8 frames [N][T][H][W][C] -> resize (bilinear, or any other PIL filter: the filter is in the tables) + crop (+ flip),
// bit-exact with PIL's 8-bit resampling (TransformImage's PIL half, utils.py:53-64).  The host builds PIL's fixed-point
// tables (per output index: first input index, tap count, 2^22-scaled coefficients), with crop and flip folded in; this
// kernel is integer work only:
//   horizontal pass -> uint8 intermediate -> vertical pass,  out = clip8((2^21 + sum k[j] * in[lo + j]) >> 22).
// Coefficients may be negative (ptx_amd_resample.h): |k| < 2^23 for __mul24, 255 * sum |k| + 2^21 < 2^31 for the accumulator,
// and >> is arithmetic, so a negative sum clips to 0.
// One workgroup per (frame, band of output rows).  It copies the tables it needs to LDS (entries clamped to the frame;
// the coefficients too when they fit), then each wave stages one referenced input row at a time in LDS (only the
// column span the column table references; 16-byte loads between a byte head and tail, LDS offset = global address
// mod 16 so both sides stay aligned; the next row is already on its way in registers), resamples it into the band's
// uint8 intermediate image in LDS, and after a barrier the vertical pass reads that image and writes either the
// interleaved uint8 rows or the normalised planes (normalise_u8: FramesToTensor's operations) with 16-byte stores.
// If a band references more rows than the intermediate holds (the host sizes bands so it does not), the band is done
// in several chunks.
// Table entries are clamped to the frame: a wrong table gives wrong pixels, never a stray access.
// ---------------------------------------------------------------------------------------------

// SRC is the source flavour: kSrcRgb (interleaved uint8 frames f), kSrcYuv8 or kSrcYuv16 (YUV below: the frames are the
// planes of `ys`, 8-bit or 10- / 12-bit in 16-bit words, f is unused, and a row is converted to RGB while it is staged,
// resize_common.h); everything from the staged row on is the same code.
// WIN (ptx_resize_frames_*_windows): the tables cover the whole resized frame (win.h rows, win.w columns) and every clip
// has a window of its own: output pixel (r, c) of clip n takes table row top_n + (vflip_n ? Ho-1-r : r) and table column
// left_n + (hflip_n ? Wo-1-c : c).  Only the table INDEX changes: the workgroup copies those entries to LDS where the
// fixed-window kernel copies entries y0 + i and x, and everything derived from the copied entries (the referenced column
// span, the head / tail split of the row staging, the YUV group origin, the chunks of a band, whose rows now may descend)
// follows per clip.  top / left are clamped so the window lies inside the tables.
// TAB (ptx_resize_frames_*_tables): every clip has tables of its own, [N][Ho] / [N][Ho][taps_h] / [N][Wo] / [N][Wo][taps_w]
// with d.taps_* the common pitch.  A workgroup of clip n moves the six table pointers to the clip's tables once and is
// the fixed-window kernel from there on: tap loops run to the entry's n, never to the pitch, and the entries are clamped
// as everywhere else.
struct ResizeWindows {
    const ptx_resize_window* wins;   // device, [N]
    int h, w;                        // entries of the row / column tables
};

// CLIPS (ptx_resize_clips_*, resize_clips.hip): every clip has a SOURCE of its own as well as tables of its own: row
// clip of `clips` gives the video's frame 0, frame stride, frame size H x W and length Tv, and frame_idx [N][T] the source
// frame of every output frame.  The workgroup reads its clip's row once (uniform), takes the clamped frame in place and
// is the TAB kernel from there on with the clip's H, W where that reads d.H, d.W; d.H / d.W are the batch maxima the plan
// sized the row stages from, and H, W are clamped into them.
struct ResizeClips {
    const ptx_clip_src* srcs;              // device, [N] (RGB)
    const void* ysrcs;                     // device, [N] (YUV: ptx_clip_src_yuv420 or ptx_clip_src_yuv420p16 rows)
    const int* frame_idx;                  // device, [N][T]
};

template <int C, int SRC = kSrcRgb, bool WIN = false, bool TAB = false, bool CLIPS = false>
__global__ void __launch_bounds__(256) resize_frames_u8_kernel(ptx_resize_desc d, const unsigned char* __restrict__ f,
                                                               const int* __restrict__ row_lo, const int* __restrict__ row_n,
                                                               const int* __restrict__ row_k, const int* __restrict__ col_lo,
                                                               const int* __restrict__ col_n, const int* __restrict__ col_k,
                                                               void* __restrict__ y, ptx_norm_desc nd, ResizePlan pl,
                                                               typename YuvSource<SRC>::Desc ys, ResizeWindows win,
                                                               ResizeClips clips) {
    constexpr bool YUV = SRC != kSrcRgb;
    extern __shared__ __attribute__((aligned(16))) unsigned char resize_smem[];
    int* hdr = reinterpret_cast<int*>(resize_smem);                 // [0] first, [1] one-past-last referenced column
    int* t_clo = hdr + 4;                                           // clamped table entries: columns [Wo], [Wo] ...
    int* t_cn = t_clo + d.Wo;
    int* t_rlo = t_cn + d.Wo;                                       // ... and this band's rows [kResizeBand], [kResizeBand]
    int* t_rn = t_rlo + kResizeBand;
    int* t_k = reinterpret_cast<int*>(resize_smem + pl.k_off);      // col_k [Wo][taps_w], then the band's row_k [band][taps_h]
    unsigned char* stage = resize_smem + pl.stage_off;              // [4 waves][stage_stride]: one input row segment each
    unsigned char* inter = stage + 4 * pl.stage_stride;             // [lds_rows][istride]: horizontally resampled rows
    const int bands = (d.Ho + pl.band - 1) / pl.band;
    const int wg = xcd_remap((int)blockIdx.x, (int)gridDim.x);      // neighbouring bands share halo rows: same L2
    const int frame = wg / bands;
    const int y0 = (wg - frame * bands) * pl.band, y1 = min(y0 + pl.band, d.Ho);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int WoC = d.Wo * C, istride = pl.istride;
    const int half = 1 << (kResizeBits - 1);
    int H = d.H, W = d.W;                                           // the frame extents of this workgroup's source
    const unsigned char* fin = YUV || CLIPS ? nullptr : f + (size_t)frame * d.H * d.W * C;
    YuvFrame yf = YUV && !CLIPS ? yuv_frame(ys, frame / d.T, frame % d.T) : YuvFrame{};
    if constexpr (CLIPS) {
        int Tv;
        int64_t stride_t = 0;
        const unsigned char* base = nullptr;
        if constexpr (YUV) {
            const auto cs = static_cast<const typename YuvSource<SRC>::Clip*>(clips.ysrcs)[frame / d.T];
            ys = cs.planes;
            H = cs.H, W = cs.W, Tv = cs.Tv;
        } else {
            const ptx_clip_src cs = clips.srcs[frame / d.T];
            base = cs.base, stride_t = cs.stride_t;
            H = cs.H, W = cs.W, Tv = cs.Tv;
        }
        H = min(max(H, 1), d.H);                                    // a garbage row cannot outrun the row stages
        W = min(max(W, 1), d.W);
        const int t = min(max(clips.frame_idx[frame], 0), max(Tv, 1) - 1);
        if constexpr (YUV) yf = yuv_frame(ys, 0, t);
        else fin = base + (int64_t)t * stride_t;
    }
    if constexpr (TAB || CLIPS) {
        const size_t clip = (size_t)(frame / d.T);
        row_lo += clip * d.Ho;
        row_n += clip * d.Ho;
        row_k += clip * d.Ho * d.taps_h;
        col_lo += clip * d.Wo;
        col_n += clip * d.Wo;
        col_k += clip * d.Wo * d.taps_w;
    }
    int top = 0, left = 0, hflip = 0, vflip = 0;
    if constexpr (WIN) {
        const ptx_resize_window wn = win.wins[frame / d.T];
        top = min(max(wn.top, 0), max(win.h - d.Ho, 0));
        left = min(max(wn.left, 0), max(win.w - d.Wo, 0));
        hflip = wn.hflip != 0;
        vflip = wn.vflip != 0;
    }
    auto col_of = [&](int x) { return WIN ? left + (hflip ? d.Wo - 1 - x : x) : x; };      // table column of output column x
    auto row_of = [&](int r) { return WIN ? top + (vflip ? d.Ho - 1 - r : r) : r; };        // table row of output row r

    if (tid == 0) {
        hdr[0] = W;
        hdr[1] = 0;
    }
    __syncthreads();
    {
        int cmin = W, cmax = 0;
        for (int x = tid; x < d.Wo; x += 256) {
            int lo, n;
            resize_entry(col_lo, col_n, col_of(x), W, d.taps_w, lo, n);
            t_clo[x] = lo;
            t_cn[x] = n;
            cmin = min(cmin, lo);
            cmax = max(cmax, lo + n);
        }
        atomicMin(&hdr[0], cmin);
        atomicMax(&hdr[1], cmax);
        for (int i = tid; i < y1 - y0; i += 256) {
            int lo, n;
            resize_entry(row_lo, row_n, row_of(y0 + i), H, min(d.taps_h, pl.lds_rows), lo, n);
            t_rlo[i] = lo;
            t_rn[i] = n;
        }
        if (pl.k_in_lds) {
            const int nck = d.Wo * d.taps_w, nrk = (y1 - y0) * d.taps_h;
            if constexpr (WIN) {
                for (int i = tid; i < nck; i += 256) {
                    const int x = i / d.taps_w;
                    t_k[i] = col_k[(size_t)col_of(x) * d.taps_w + (i - x * d.taps_w)];
                }
                for (int i = tid; i < nrk; i += 256) {
                    const int ri = i / d.taps_h;
                    t_k[nck + i] = row_k[(size_t)row_of(y0 + ri) * d.taps_h + (i - ri * d.taps_h)];
                }
            } else {
                for (int i = tid; i < nck; i += 256) t_k[i] = col_k[i];
                for (int i = tid; i < nrk; i += 256) t_k[nck + i] = row_k[(size_t)y0 * d.taps_h + i];
            }
        }
    }
    __syncthreads();
    const int* ck = pl.k_in_lds ? t_k : col_k;                                            // [Wo][taps_w]
    const int* rk = pl.k_in_lds ? t_k + d.Wo * d.taps_w : row_k + (size_t)y0 * d.taps_h;  // [y1 - y0][taps_h]
    // coefficients of output column x / output row `row`: the LDS copies are in output order, the global tables of the
    // windows kernel are indexed through the clip's window
    auto col_coeffs = [&](int x) {
        if constexpr (WIN) return pl.k_in_lds ? ck + x * d.taps_w : col_k + (size_t)col_of(x) * d.taps_w;
        else return ck + x * d.taps_w;
    };
    auto row_coeffs = [&](int row) {
        if constexpr (WIN) return pl.k_in_lds ? rk + (row - y0) * d.taps_h : row_k + (size_t)row_of(row) * d.taps_h;
        else return rk + (row - y0) * d.taps_h;
    };
    const int cmin = hdr[0];
    const int span_bytes = max(hdr[1] - cmin, 0) * C;               // <= W * C
    const int px_end = max(hdr[1], cmin);                           // one past the last referenced column

    int r = y0;
    while (r < y1) {
        // the chunk [r, r1) of output rows whose referenced input rows [lo0, hi0) fit the intermediate image
        int lo0 = t_rlo[r - y0];
        int hi0 = lo0 + t_rn[r - y0], r1 = r + 1;
        while (r1 < y1) {
            const int lo = t_rlo[r1 - y0], n = t_rn[r1 - y0];
            const int l2 = min(lo0, lo), h2 = max(hi0, lo + n);
            if (h2 - l2 > pl.lds_rows) break;
            lo0 = l2;
            hi0 = h2;
            ++r1;
        }
        const int nrows = hi0 - lo0;

        // horizontal pass: wave w resamples input rows lo0 + w, lo0 + w + 4, ...  The next row's bytes are fetched into
        // registers (3 x 1 KiB per wave; wider rows copy the rest when the row is staged) before the current
        // row is resampled, so the HBM latency hides under the LDS work instead of adding to every row.
        unsigned char* sw = stage + wave * pl.stage_stride;
        ResizeRow pre = {};
        typename YuvSource<SRC>::Row ypre = {};
        if constexpr (YUV) yuv_fetch_row(ypre, 0 + wave, nrows, ys, yf, lo0, cmin, px_end, lane);
        else resize_fetch_row(pre, 0 + wave, nrows, fin, lo0, W, cmin, C, span_bytes, lane);
        for (int i0 = 0; i0 < nrows; i0 += 4) {
            const int i = i0 + wave;
            int off = 0;
            if constexpr (YUV) {
                if (i < nrows) off = yuv_stage_row(sw, ypre, ys, yf, lo0 + i, cmin, px_end, lane);
            } else if (i < nrows) {
                int vb, ve, end;
                const unsigned char* g = resize_row_span(fin, lo0 + i, W, cmin, C, span_bytes, off, vb, ve, end);
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
            else resize_fetch_row(pre, i + 4, nrows, fin, lo0, W, cmin, C, span_bytes, lane);
            if (i < nrows) {
                for (int x = lane; x < d.Wo; x += 64) {
                    const int lo = t_clo[x], n = t_cn[x];
                    const unsigned char* p = sw + off + (lo - cmin) * C;
                    const int* kk = col_coeffs(x);
                    int acc[C];
#pragma unroll
                    for (int c = 0; c < C; ++c) acc[c] = half;
#pragma unroll 4
                    for (int j = 0; j < n; ++j) {
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

        // vertical pass over output rows [r, r1)
        const int nout = r1 - r;
        if (d.out_mode == PTX_RESIZE_OUT_U8) {
            unsigned char* yo = static_cast<unsigned char*>(y);
            const int q4 = istride / 4;                              // 4 interleaved bytes per thread
            for (int it = tid; it < nout * q4; it += 256) {
                const int yy = it / q4, q = it - yy * q4, row = r + yy;
                const int lo = t_rlo[row - y0], n = t_rn[row - y0];
                const unsigned char* p = inter + (lo - lo0) * istride + q * 4;
                const int* kk = row_coeffs(row);
                int acc[4] = {half, half, half, half};
                for (int j = 0; j < n; ++j) {
                    const int k = kk[j];
                    const unsigned v = *reinterpret_cast<const unsigned*>(p + j * istride);
#pragma unroll
                    for (int e = 0; e < 4; ++e) acc[e] += __mul24(k, (int)((v >> (8 * e)) & 255u));
                }
                // a negative sum (negative coefficients) gives 0, and no packed shift-and-saturate: see resize_clip8
                unsigned o = 0;
#pragma unroll
                for (int e = 0; e < 4; ++e) o |= resize_clip8(acc[e]) << (8 * e);
                unsigned char* ob = yo + ((size_t)frame * d.Ho + row) * WoC + q * 4;
                if (pl.vec_store) {
                    *reinterpret_cast<unsigned*>(ob) = o;
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (q * 4 + e < WoC) ob[e] = (unsigned char)(o >> (8 * e));
                }
            }
        } else {
            const int Wg = (d.Wo + 3) / 4;                           // 4 pixels of one plane row per thread
            const int n_ = frame / d.T, t = frame - n_ * d.T;
            for (int it = tid; it < nout * C * Wg; it += 256) {
                const int xg = it % Wg, t2 = it / Wg;
                const int c = t2 % C, row = r + t2 / C;
                const int cin = (nd.swap_rb && (c == 0 || c == 2)) ? 2 - c : c;
                const int lo = t_rlo[row - y0], n = t_rn[row - y0];
                const unsigned char* p = inter + (lo - lo0) * istride + cin;
                const int* kk = row_coeffs(row);
                int xo[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) xo[e] = min(xg * 4 + e, d.Wo - 1) * C;
                int acc[4] = {half, half, half, half};
                for (int j = 0; j < n; ++j) {
                    const int k = kk[j];
#pragma unroll
                    for (int e = 0; e < 4; ++e) acc[e] += __mul24(k, (int)p[j * istride + xo[e]]);
                }
                float v[4];
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    v[e] = normalise_u8((unsigned char)clip8(acc[e] >> kResizeBits), nd.mean[c], nd.std[c], nd.to_255);
                const size_t o = ((((size_t)n_ * C + c) * d.T + t) * d.Ho + row) * d.Wo + (size_t)xg * 4;
                if (d.out_mode == PTX_RESIZE_OUT_F32) {
                    float* yo = static_cast<float*>(y) + o;
                    if (pl.vec_store) {
                        f32x4 q = {v[0], v[1], v[2], v[3]};
                        *reinterpret_cast<f32x4*>(yo) = q;
                    } else {
#pragma unroll
                        for (int e = 0; e < 4; ++e)
                            if (xg * 4 + e < d.Wo) yo[e] = v[e];
                    }
                } else {
                    __bf16* yo = static_cast<__bf16*>(y) + o;
                    unsigned short b[4];
#pragma unroll
                    for (int e = 0; e < 4; ++e) b[e] = __builtin_bit_cast(unsigned short, (__bf16)v[e]);   // nearest even
                    if (pl.vec_store) {
                        uint2 q = {(unsigned)b[0] | ((unsigned)b[1] << 16), (unsigned)b[2] | ((unsigned)b[3] << 16)};
                        *reinterpret_cast<uint2*>(yo) = q;
                    } else {
#pragma unroll
                        for (int e = 0; e < 4; ++e)
                            if (xg * 4 + e < d.Wo) reinterpret_cast<unsigned short*>(yo)[e] = b[e];
                    }
                }
            }
        }
        __syncthreads();                                             // the next chunk overwrites the intermediate image
        r = r1;
    }
}

// ---------------------------------------------------------------------------------------------
// The per-clip tables of ptx_resize_frames_*_tables, built on the device from one ptx_resize_geom per clip
// (ptx_resize_build_tables, ptx_resize_build_tables_filter): one thread per (clip, axis, output index) restates PIL's
// precompute_coeffs + normalize_coeffs_8bpc for its entry in IEEE fp64, in the operation order of
// transforms.resize_axis_table -- the host builder the fixed-window launch uses -- so the entry has that builder's bits.
// Contraction is OFF: hipcc otherwise fuses (i + 0.5) * scale - fs, 1 - |..| * ss, the bicubic polynomial and w * 2^22 + 0.5
// into FMAs, which moves the last bit of `center` and of the weights and with it a coefficient here and there.  The sum of
// the weights is taken sequentially.  `filter` is a PTX_RESAMPLE_* code of BOX, BILINEAR, BICUBIC (PIL's filter functions,
// support 0.5 / 1 / 2) or NEAREST (PIL's affine walk: one tap at (int)(a / 2 + a + a + ...), i sequential additions for index
// i, because the walk's sum differs from a product in the last bit); the bilinear branch is the code it was.
// Garbage rows are safe: the box is clamped into the frame, the resized extent to >= 1 (NEAREST: and to the longest walk),
// the window into the resized frame, the table index into [0, extent), n to the pitch; the resize kernel clamps the entries
// once more.
// ---------------------------------------------------------------------------------------------
// The entry of (clip, axis entry e) for frames of H x W: the body shared by resize_build_tables_kernel (H, W of the
// descriptor) and resize_build_tables_clips_kernel (resize_clips.hip: H, W of the clip's source row).
__device__ __forceinline__ void resize_build_entry(const ptx_resize_desc& d, int H, int W, int clip, int e,
                                                   const ptx_resize_geom* __restrict__ geoms, int filter,
                                                   int* __restrict__ row_lo, int* __restrict__ row_n, int* __restrict__ row_k,
                                                   int* __restrict__ col_lo, int* __restrict__ col_n, int* __restrict__ col_k) {
#pragma clang fp contract(off)
    const bool rows = e < d.Ho;
    const int o = rows ? e : e - d.Ho;                               // output index on this axis
    const int S = rows ? d.Ho : d.Wo, extent = rows ? H : W, taps = rows ? d.taps_h : d.taps_w;
    const ptx_resize_geom g = geoms[clip];
    const int origin = min(max(rows ? g.box_top : g.box_left, 0), extent - 1);
    const int n_in = min(max(rows ? g.box_h : g.box_w, 1), extent - origin);
    int n_out = max(rows ? g.h : g.w, 1);
    if (filter == PTX_RESAMPLE_NEAREST) n_out = min(n_out, PTX_RESAMPLE_NEAREST_MAX_EXTENT);   // bounds the walk below
    const int start = min(max(rows ? g.top : g.left, 0), max(n_out - S, 0));
    const int flip = (rows ? g.vflip : g.hflip) != 0;
    const int i = min(start + (flip ? S - 1 - o : o), n_out - 1);   // index in the resized box
    const size_t at = (size_t)clip * S + o;
    int* lo_t = rows ? row_lo : col_lo;
    int* n_t = rows ? row_n : col_n;
    int* k = (rows ? row_k : col_k) + at * taps;
    if (n_in == n_out || filter == PTX_RESAMPLE_NEAREST) {           // one tap of 2^22: not resampled, or PIL's nearest index
        int idx = i;
        if (n_in != n_out) {
            const double a = (double)n_in / (double)n_out;
            double xo = a * 0.5;
            for (int t = 0; t < i; ++t) xo = xo + a;
            idx = min(max((int)fmin(xo, 2147483647.0), 0), n_in - 1);
        }
        lo_t[at] = origin + idx;
        n_t[at] = 1;
        k[0] = 1 << kResizeBits;
        for (int j = 1; j < taps; ++j) k[j] = 0;
        return;
    }
    const double scale = (double)n_in / (double)n_out;
    const double fs = scale > 1.0 ? scale : 1.0;
    const double support = (filter == PTX_RESAMPLE_BOX ? 0.5 : filter == PTX_RESAMPLE_BICUBIC ? 2.0 : 1.0) * fs;
    const double ss = 1.0 / fs;
    const double center = ((double)i + 0.5) * scale;
    // C's (int) truncates (a value in (-1, 0) gives 0, a lower one is clamped to 0 as PIL clamps it); clamped in double
    // first, both values lie inside int whatever the row held
    const int lo = min(max((int)fmin(fmax(center - support + 0.5, -2147483648.0), 2147483647.0), 0), n_in - 1);   // below n_in for every real row
    const int hi = min((int)fmin(center + support + 0.5, 2147483647.0), n_in);
    const int n = min(max(hi - lo, 0), taps);
    auto weight = [&](int j) {
        double x = ((double)j + (double)lo - center + 0.5) * ss;
        if (filter == PTX_RESAMPLE_BOX) return x > -0.5 && x <= 0.5 ? 1.0 : 0.0;
        if (filter == PTX_RESAMPLE_BICUBIC) {                        // PIL's bicubic_filter, a = -0.5: (a + 2) = 1.5, (a + 3) = 2.5
            if (x < 0.0) x = -x;
            if (x < 1.0) return (1.5 * x - 2.5) * x * x + 1.0;
            if (x < 2.0) return (((x - 5.0) * x + 8.0) * x - 4.0) * -0.5;
            return 0.0;
        }
        const double w = 1.0 - fabs(x);
        return w > 0.0 ? w : 0.0;
    };
    double ww = 0.0;
    for (int j = 0; j < n; ++j) ww = ww + weight(j);
    lo_t[at] = origin + lo;
    n_t[at] = n;
    for (int j = 0; j < taps; ++j) {
        int c = 0;
        if (j < n) {
            double w = weight(j);
            if (ww != 0.0) w = w / ww;
            c = w < 0.0 ? (int)(-0.5 + w * 4194304.0) : (int)(w * 4194304.0 + 0.5);
        }
        k[j] = c;
    }
}

__global__ void __launch_bounds__(256) resize_build_tables_kernel(ptx_resize_desc d, const ptx_resize_geom* __restrict__ geoms,
                                                                  int filter, int* __restrict__ row_lo, int* __restrict__ row_n,
                                                                  int* __restrict__ row_k, int* __restrict__ col_lo,
                                                                  int* __restrict__ col_n, int* __restrict__ col_k) {
    const int per_clip = d.Ho + d.Wo;
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long long)d.N * per_clip) return;
    const int clip = (int)(idx / per_clip), e = (int)(idx - (long long)clip * per_clip);
    resize_build_entry(d, d.H, d.W, clip, e, geoms, filter, row_lo, row_n, row_k, col_lo, col_n, col_k);
}

// The filters the device builder takes, or the reason it does not (no device needed).
static int resize_filter_check(int filter, const char* who) {
    switch (filter) {
        case PTX_RESAMPLE_NEAREST: case PTX_RESAMPLE_BOX: case PTX_RESAMPLE_BILINEAR: case PTX_RESAMPLE_BICUBIC:
            return PTX_OK;
        case PTX_RESAMPLE_HAMMING: case PTX_RESAMPLE_LANCZOS:
            return fail(PTX_ERR_UNSUPPORTED, "%s: filter=%d (%s): its weights are sin / cos of the host's C library, which the "
                        "device cannot be promised to equal bit for bit; the device builder takes nearest, box, bilinear and "
                        "bicubic (build the table on the host)", who, filter, filter == PTX_RESAMPLE_HAMMING ? "hamming" : "lanczos");
        default:
            return fail(PTX_ERR_INVALID, "%s: filter=%d is not a PTX_RESAMPLE_* code", who, filter);
    }
}

static unsigned grid_for(size_t work_items) {
    size_t b = (work_items + 255) / 256;
    const size_t cap = (size_t)kNumCU * 8;
    if (b > cap) b = cap;
    if (b == 0) b = 1;
    return (unsigned)b;
}

// ---------------------------------------------------------------------------------------------
// parameter checksum: a 64-bit, position-sensitive sum over the bit patterns of a SET of fp32 tensors
// (table of (device pointer, element count) pairs).  The host compares it between forwards to notice
// weight edits that bypass torch's version counters (`p.data.fill_(..)`); HBM-bound, one launch.
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) checksum_f32_kernel(const long long* __restrict__ table, int n,
                                                           unsigned long long* __restrict__ out) {
    const int t = blockIdx.y;
    const unsigned* __restrict__ p = reinterpret_cast<const unsigned*>(table[2 * t]);
    const long long cnt = table[2 * t + 1];
    unsigned long long acc = 0;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < cnt; i += (long long)gridDim.x * 256)
        acc += (unsigned long long)p[i] * (unsigned long long)(2654435761u * (unsigned)i | 1u);
    acc *= (unsigned long long)(2 * t + 1);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)acc, o, 64);
        const unsigned hi = (unsigned)__shfl_xor((int)(unsigned)(acc >> 32), o, 64);
        acc += ((unsigned long long)hi << 32) | lo;
    }
    if ((threadIdx.x & 63) == 0 && acc) atomicAdd(out, acc);
}

// the same sum over 16-bit elements (bf16 / fp16 parameter tensors); table counts are 16-bit elements
__global__ void __launch_bounds__(256) checksum_b16_kernel(const long long* __restrict__ table, int n,
                                                           unsigned long long* __restrict__ out) {
    const int t = blockIdx.y;
    const unsigned short* __restrict__ p = reinterpret_cast<const unsigned short*>(table[2 * t]);
    const long long cnt = table[2 * t + 1];
    unsigned long long acc = 0;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < cnt; i += (long long)gridDim.x * 256)
        acc += (unsigned long long)(p[i] + 1u) * (unsigned long long)(2654435761u * (unsigned)i | 1u);
    acc *= (unsigned long long)(2 * t + 1);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)acc, o, 64);
        const unsigned hi = (unsigned)__shfl_xor((int)(unsigned)(acc >> 32), o, 64);
        acc += ((unsigned long long)hi << 32) | lo;
    }
    if ((threadIdx.x & 63) == 0 && acc) atomicAdd(out, acc);
}

// ---------------------------------------------------------------------------------------------
// bf16 plans: 16-bit NCDHW <-> NDHWC tile transposes (bit-exact moves, 32 x 32 elements through LDS), the (kh, kw) fold
// of the RGB stem, and the rounding of the logits
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) ncs_to_nsc_b16_kernel(const unsigned short* __restrict__ x, unsigned short* __restrict__ y,
                                                             int C, long long S, int ld) {
    __shared__ unsigned short tile[32][33];
    const int n = blockIdx.z;
    const long long s0 = (long long)blockIdx.x * 32;
    const int c0 = blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const unsigned short* xn = x + (size_t)n * C * S;
    unsigned short* yn = y + (size_t)n * S * ld;
#pragma unroll
    for (int j = 0; j < 32; j += 8) {
        const int c = c0 + ty + j;
        const long long s = s0 + tx;
        tile[ty + j][tx] = (c < C && s < S) ? xn[(size_t)c * S + s] : (unsigned short)0;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 32; j += 8) {
        const long long s = s0 + ty + j;
        const int c = c0 + tx;
        if (s < S && c < ld) yn[(size_t)s * ld + c] = tile[tx][ty + j];   // zero beyond C by construction
    }
}

__global__ void __launch_bounds__(256) nsc_to_ncs_b16_kernel(const unsigned short* __restrict__ x, unsigned short* __restrict__ y,
                                                             int C, long long S, int ld) {
    __shared__ unsigned short tile[32][33];
    const int n = blockIdx.z;
    const long long s0 = (long long)blockIdx.x * 32;
    const int c0 = blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const unsigned short* xn = x + (size_t)n * S * ld;
    unsigned short* yn = y + (size_t)n * C * S;
#pragma unroll
    for (int j = 0; j < 32; j += 8) {
        const long long s = s0 + ty + j;
        const int c = c0 + tx;
        tile[ty + j][tx] = (s < S && c < C) ? xn[(size_t)s * ld + c] : (unsigned short)0;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 32; j += 8) {
        const int c = c0 + ty + j;
        const long long s = s0 + tx;
        if (c < C && s < S) yn[(size_t)c * S + s] = tile[tx][ty + j];
    }
}

// one thread per 8 output columns (one 16-byte store) of one output position: column k = (kh * kW + kw) * C + c gathers
// x[n][c][t][ho*sH - pH + kh][wo*sW - pW + kw] (zero outside the image and for k >= kH * kW * C)
__global__ void __launch_bounds__(256) im2col_hw_bf16_kernel(const unsigned short* __restrict__ x, unsigned short* __restrict__ y,
                                                             int C, int T, int H, int W, int kH, int kW, int sH, int sW,
                                                             int pH, int pW, int Ho, int Wo, int ld, long long total) {
    typedef unsigned short u16x8 __attribute__((ext_vector_type(8)));
    const int g8 = ld / 8, kk = kH * kW * C;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const long long pos = i / g8;
        const int k0 = (int)(i - pos * g8) * 8;
        const int wo = (int)(pos % Wo);
        long long r = pos / Wo;
        const int ho = (int)(r % Ho);
        r /= Ho;
        const int t = (int)(r % T);
        const long long n = r / T;
        u16x8 v;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int k = k0 + e;
            const int c = k % C, tap = k / C;
            const int kh = tap / kW, kw = tap - (tap / kW) * kW;
            const int h = ho * sH - pH + kh, w = wo * sW - pW + kw;
            const bool ok = k < kk && (unsigned)h < (unsigned)H && (unsigned)w < (unsigned)W;
            v[e] = ok ? x[(((size_t)n * C + c) * T + t) * (size_t)H * W + (size_t)h * W + w] : (unsigned short)0;
        }
        *reinterpret_cast<u16x8*>(y + (size_t)i * 8) = v;
    }
}

__global__ void __launch_bounds__(256) f32_to_bf16_kernel(const float* __restrict__ x, __bf16* __restrict__ y, long long n) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256)
        y[i] = (__bf16)x[i];      // v_cvt_pk_bf16_f32: round to nearest even, NaN stays NaN
}

__global__ void __launch_bounds__(256) bf16_to_f32_kernel(const __bf16* __restrict__ x, float* __restrict__ y, long long n) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256)
        y[i] = (float)x[i];       // exact
}

}  // namespace ptx

using namespace ptx;

// PTX_SOURCE_SHA256: sha256 of csrc/*.hip, csrc/*.h and include/ptx_amd.h, computed by build.py (source_hash) and passed on
// this file's command line -- `ptx_version()` names the source the loaded binary was compiled from
#ifndef PTX_SOURCE_SHA256
#define PTX_SOURCE_SHA256 "unstamped"
#endif
extern "C" const char* ptx_version(void) { return "ptx_amd 0.5.0 (gfx950, fp32 MFMA) src:" PTX_SOURCE_SHA256; }
extern "C" const char* ptx_last_error(void) { return last_error_buf(); }

extern "C" size_t ptx_packed_weight_elems(const ptx_pack_desc* d) {
    if (!d) return 0;
    const size_t taps = d->fold_kw ? (size_t)d->kT * d->kH : (size_t)d->kT * d->kH * d->kW;
    return taps * d->Co_pad * (d->ld_k > 0 ? d->ld_k : d->Kc);
}

extern "C" int ptx_pack_conv_weight(const ptx_pack_desc* d, const float* w, const float* conv_bias,
                                    const float* bn_gamma, const float* bn_beta, const float* bn_mean,
                                    const float* bn_var, float bn_eps, float* w_packed, float* bias_out,
                                    ptx_stream_t stream) {
    if (!d || !w || !w_packed || !bias_out) return fail(PTX_ERR_INVALID, "pack: null pointer");
    if (d->Co <= 0 || d->Ci <= 0 || d->kT <= 0 || d->kH <= 0 || d->kW <= 0)
        return fail(PTX_ERR_INVALID, "pack: non-positive extent");
    if (d->ld_k < 0 || d->k_off < 0 || (d->ld_k > 0 && (d->k_off + d->Kc > d->ld_k || d->ld_k % 4 || d->k_off % 4)))
        return fail(PTX_ERR_INVALID, "pack: bad K-concatenation window (ld_k=%d k_off=%d Kc=%d)", d->ld_k, d->k_off, d->Kc);
    if (d->ld_k == 0 && d->k_off != 0) return fail(PTX_ERR_INVALID, "pack: k_off needs ld_k");
    if (d->sub_groups > 1 && (d->fold_kw || d->Ci % d->sub_groups || d->co_per_super <= 0 ||
                              d->co_per_super % d->sub_groups || d->Co % d->co_per_super))
        return fail(PTX_ERR_INVALID, "pack: super-group packing needs sub_groups | Ci, sub_groups | co_per_super | Co, no kW fold");
    const int keff = d->fold_kw ? d->kW * d->Ci : d->Ci;
    if ((d->f16 == 1 || d->f16 == 3) && (d->Kc % 8 || d->ld_k || d->k_off))
        return fail(PTX_ERR_INVALID, "pack: fp16 filters need Kc %% 8 == 0 and no K-concatenation window");
    if (d->f16 == 2 && (d->Kc % 8 || d->ld_k % 8 || d->k_off % 8 || d->sub_groups > 1))
        return fail(PTX_ERR_INVALID, "pack: split (hi8 | lo8) filters need Kc, ld_k and k_off %% 8 == 0, no super-groups");
    if (d->f16 < 0 || d->f16 > 3)
        return fail(PTX_ERR_INVALID, "pack: f16 must be 0 (fp32), 1 (halfs), 2 (split halfs) or 3 (bf16)");
    if (d->Kc < keff || d->Kc % 4 || d->Co_pad < d->Co || d->Co_pad % 128)
        return fail(PTX_ERR_INVALID, "pack: Kc=%d must cover K=%d (multiple of 4); Co_pad=%d must cover Co=%d (multiple of 128)",
                    d->Kc, keff, d->Co_pad, d->Co);
    if ((bn_gamma != nullptr) != (bn_var != nullptr))
        return fail(PTX_ERR_INVALID, "pack: bn_gamma and bn_var must be given together");
    const size_t taps = d->fold_kw ? (size_t)d->kT * d->kH : (size_t)d->kT * d->kH * d->kW;
    const size_t total = taps * d->Co_pad * d->Kc;     // elements written by this call (one K window)
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(pack_weight_kernel, dim3(grid_for(total)), dim3(256), 0, st, *d, w, bn_gamma, bn_var, bn_eps,
                       w_packed, total);
    PTX_HIP(hipGetLastError());
    hipLaunchKernelGGL(pack_bias_kernel, dim3(cdiv(d->Co_pad, 256)), dim3(256), 0, st, d->Co, d->Co_pad, conv_bias,
                       bn_gamma, bn_beta, bn_mean, bn_var, bn_eps, bias_out, d->bias_accumulate);
    return hip_check(hipGetLastError(), "pack launch");
}

static int check_layout_args(const void* x, const void* y, int N, int C, int64_t S, int ld) {
    if (!x || !y) return fail(PTX_ERR_INVALID, "layout: null pointer");
    if (N <= 0 || C <= 0 || S <= 0 || ld < C || ld % 4) return fail(PTX_ERR_INVALID, "layout: bad extents");
    if (N > 65535 || cdiv(ld, 32) > 65535) return fail(PTX_ERR_INVALID, "layout: N or C too large for the grid");
    return PTX_OK;
}

// C <= 4 channels -> 16-byte positions (the split-operand stem's input): every thread gathers its position's channels
// from C coalesced planes and writes one float4 -- the 32 x 32 tile transpose above spends 29 of its 32 channel rows
// on padding for an RGB clip (1.6 TB/s; this one streams at the HBM rate)
__global__ void __launch_bounds__(256) ncs_to_ns4_kernel(const float* __restrict__ x, float* __restrict__ y, int C,
                                                         long long S, long long total) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const long long n = i / S, sp = i - n * S;
        const float* xn = x + (size_t)n * C * S + sp;
        f32x4 v = {xn[0], 0.f, 0.f, 0.f};
        if (C > 1) v.y = xn[S];
        if (C > 2) v.z = xn[2 * S];
        if (C > 3) v.w = xn[3 * S];
        *reinterpret_cast<f32x4*>(y + (size_t)i * 4) = v;
    }
}

// The split-operand stem's input format: one 16-byte position = 4 channels as (hi4 | lo4) halfs, hi = half(v),
// lo = half(v - hi) -- the split the x3 tiles do in registers, done once here, in the pass that leaves NCDHW anyway.
typedef _Float16 half8_s __attribute__((ext_vector_type(8)));
__global__ void __launch_bounds__(256) ncs_to_split4_kernel(const float* __restrict__ x, float* __restrict__ y, int C,
                                                            long long S, long long total) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const long long n = i / S, sp = i - n * S;
        const float* xn = x + (size_t)n * C * S + sp;
        float v[4] = {xn[0], 0.f, 0.f, 0.f};
        if (C > 1) v[1] = xn[S];
        if (C > 2) v[2] = xn[2 * S];
        if (C > 3) v[3] = xn[3 * S];
        half8_s o;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const _Float16 h = (_Float16)v[c];
            o[c] = h;
            o[4 + c] = (_Float16)((v[c] - (float)h) * 4096.f);      // scaled lo (conv_igemm.hip, X3)
        }
        *reinterpret_cast<half8_s*>(y + (size_t)i * 4) = o;
    }
}

extern "C" int ptx_ncdhw_to_split4(const float* x, void* y, int32_t N, int32_t C, int64_t S, ptx_stream_t stream) {
    if (!x || !y) return fail(PTX_ERR_INVALID, "ncdhw_to_split4: null pointer");
    if (N <= 0 || C <= 0 || C > 4 || S <= 0 || (((uintptr_t)y) & 15)) return fail(PTX_ERR_INVALID, "ncdhw_to_split4: 1..4 channels, 16-byte aligned output");
    const long long total = (long long)N * S;
    const unsigned blocks = (unsigned)std::min<long long>((total + 255) / 256, (long long)kNumCU * 32);
    hipLaunchKernelGGL(ncs_to_split4_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, x, static_cast<float*>(y), C, (long long)S, total);
    return hip_check(hipGetLastError(), "ncdhw_to_split4 launch");
}

extern "C" int ptx_ncdhw_to_ndhwc(const float* x, float* y, int32_t N, int32_t C, int64_t S, int32_t ld,
                                  ptx_stream_t stream) {
    int s = check_layout_args(x, y, N, C, S, ld);
    if (s) return s;
    if (C <= 4 && ld == 4 && (((uintptr_t)y) & 15) == 0) {
        const long long total = (long long)N * S;
        const unsigned blocks = (unsigned)std::min<long long>((total + 255) / 256, (long long)kNumCU * 32);
        hipLaunchKernelGGL(ncs_to_ns4_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, x, y, C, (long long)S, total);
        return hip_check(hipGetLastError(), "ncdhw_to_ndhwc launch");
    }
    dim3 grid((unsigned)cdiv64(S, 32), (unsigned)cdiv(ld, 32), (unsigned)N);
    hipLaunchKernelGGL(ncs_to_nsc_kernel, grid, dim3(256), 0, (hipStream_t)stream, x, y, C, (long long)S, ld);
    return hip_check(hipGetLastError(), "ncdhw_to_ndhwc launch");
}

extern "C" int ptx_ndhwc_to_ncdhw(const float* x, float* y, int32_t N, int32_t C, int64_t S, int32_t ld,
                                  ptx_stream_t stream) {
    int s = check_layout_args(x, y, N, C, S, ld);
    if (s) return s;
    dim3 grid((unsigned)cdiv64(S, 32), (unsigned)cdiv(C, 32), (unsigned)N);
    hipLaunchKernelGGL(nsc_to_ncs_kernel, grid, dim3(256), 0, (hipStream_t)stream, x, y, C, (long long)S, ld);
    return hip_check(hipGetLastError(), "ndhwc_to_ncdhw launch");
}

extern "C" int ptx_transpose_last2(const float* x, float* y, int32_t batch, int32_t R, int32_t Cc, int32_t ldx,
                                   int32_t ldy, ptx_stream_t stream) {
    if (!x || !y) return fail(PTX_ERR_INVALID, "transpose: null pointer");
    if (batch <= 0 || batch > 65535 || R <= 0 || Cc <= 0 || ldx < Cc || ldy < R)
        return fail(PTX_ERR_INVALID, "transpose: bad extents");
    dim3 grid((unsigned)cdiv(ldy, 32), (unsigned)cdiv(Cc, 32), (unsigned)batch);
    hipLaunchKernelGGL(transpose_last2_kernel, grid, dim3(256), 0, (hipStream_t)stream, x, y, R, Cc, ldx, ldy);
    return hip_check(hipGetLastError(), "transpose_last2 launch");
}

static int check_fold_args(const void* x, const void* y, int N, int C, int T, int H, int W, int kW, int sW, int pW, int Wo,
                           int ld);

extern "C" int ptx_fold_kw_ncdhw(const float* x, float* y, int32_t N, int32_t C, int32_t T, int32_t H, int32_t W,
                                 int32_t kW, int32_t sW, int32_t pW, int32_t Wo, int32_t ld, ptx_stream_t stream) {
    const int64_t plane = (int64_t)T * H * W;
    return ptx_fold_kw_strided(x, y, N, C, T, H, W, (int64_t)C * plane, plane, (int64_t)H * W, kW, sW, pW, Wo, ld, stream);
}

static int check_fold_args(const void* x, const void* y, int N, int C, int T, int H, int W, int kW, int sW, int pW, int Wo,
                           int ld) {
    if (!x || !y) return fail(PTX_ERR_INVALID, "fold_kw: null pointer");
    if (N <= 0 || C <= 0 || T <= 0 || H <= 0 || W <= 0 || kW <= 0 || sW <= 0 || pW < 0 || Wo <= 0)
        return fail(PTX_ERR_INVALID, "fold_kw: non-positive extent");
    if (ld < kW * C || ld % 4) return fail(PTX_ERR_INVALID, "fold_kw: ld=%d must cover kW*C=%d and be a multiple of 4", ld, kW * C);
    {
        const int same = (W + sW - 1) / sW;              // TF-"SAME": pW is the front pad floor(total/2)
        const int total = std::max((same - 1) * sW + kW - W, 0);
        if (Wo != (W + 2 * pW - kW) / sW + 1 && !(Wo == same && pW == total / 2))
            return fail(PTX_ERR_INVALID, "fold_kw: Wo mismatch");
    }
    if ((uintptr_t)y & 15) return fail(PTX_ERR_INVALID, "fold_kw: misaligned output");
    if (ld / 4 > 256 || (size_t)C * W * sizeof(float) > 64 * 1024)
        return fail(PTX_ERR_UNSUPPORTED, "fold_kw: row of %d x %d floats does not fit the LDS staging buffer", C, W);
    if ((int64_t)N * T * H > 0x7fffffffLL) return fail(PTX_ERR_INVALID, "fold_kw: too many rows");
    return PTX_OK;
}

extern "C" int ptx_fold_kw_strided(const float* x, float* y, int32_t N, int32_t C, int32_t T, int32_t H, int32_t W,
                                   int64_t stride_n, int64_t stride_c, int64_t stride_t, int32_t kW, int32_t sW,
                                   int32_t pW, int32_t Wo, int32_t ld, ptx_stream_t stream) {
    int s = check_fold_args(x, y, N, C, T, H, W, kW, sW, pW, Wo, ld);
    if (s) return s;
    if (stride_n <= 0 || stride_c < (int64_t)H * W || stride_t < (int64_t)H * W)
        return fail(PTX_ERR_INVALID, "fold_kw: strides must be at least one H x W plane");
    hipLaunchKernelGGL(fold_kw_kernel, dim3((unsigned)(N * T * H)), dim3(256), (size_t)C * W * sizeof(float),
                       (hipStream_t)stream, x, y, C, T, H, W, (long long)stride_n, (long long)stride_c,
                       (long long)stride_t, kW, sW, pW, Wo, ld);
    return hip_check(hipGetLastError(), "fold_kw launch");
}

static int check_norm(const ptx_norm_desc* nd, int C) {
    if (!nd) return fail(PTX_ERR_INVALID, "frames_u8: null norm descriptor");
    if (C <= 0 || C > 4) return fail(PTX_ERR_INVALID, "frames_u8: C=%d must be 1..4", C);
    for (int c = 0; c < C; ++c)
        if (!(nd->std[c] != 0.f)) return fail(PTX_ERR_INVALID, "frames_u8: std[%d] must be non-zero", c);
    if (nd->swap_rb && C < 3) return fail(PTX_ERR_INVALID, "frames_u8: BGR swap needs 3 channels");
    return PTX_OK;
}

extern "C" int ptx_frames_u8_to_ncdhw(const uint8_t* frames, float* y, int32_t N, int32_t T, int32_t H, int32_t W,
                                      int32_t C, const ptx_norm_desc* norm, ptx_stream_t stream) {
    if (!frames || !y) return fail(PTX_ERR_INVALID, "frames_u8: null pointer");
    if (N <= 0 || T <= 0 || H <= 0 || W <= 0) return fail(PTX_ERR_INVALID, "frames_u8: non-positive extent");
    int s = check_norm(norm, C);
    if (s) return s;
    const long long THW = (long long)T * H * W;
    const size_t total = (size_t)N * C * THW;
    hipLaunchKernelGGL(frames_u8_to_ncdhw_kernel, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, frames, y,
                       total, C, THW, *norm);
    return hip_check(hipGetLastError(), "frames_u8_to_ncdhw launch");
}

extern "C" int ptx_fold_kw_frames_u8(const uint8_t* frames, float* y, int32_t N, int32_t C, int32_t T, int32_t H,
                                     int32_t W, int32_t frame_step, int32_t T_full, int32_t kW, int32_t sW, int32_t pW,
                                     int32_t Wo, int32_t ld, const ptx_norm_desc* norm, ptx_stream_t stream) {
    int s = check_fold_args(frames, y, N, C, T, H, W, kW, sW, pW, Wo, ld);
    if (s) return s;
    s = check_norm(norm, C);
    if (s) return s;
    if (frame_step <= 0 || T_full <= 0 || (int64_t)(T - 1) * frame_step >= T_full)
        return fail(PTX_ERR_INVALID, "fold_kw_frames_u8: T=%d frames at step %d do not fit T_full=%d", T, frame_step, T_full);
    hipLaunchKernelGGL(fold_kw_frames_u8_kernel, dim3((unsigned)(N * T * H)), dim3(256), (size_t)C * W * sizeof(float),
                       (hipStream_t)stream, frames, y, C, T, H, W, frame_step, T_full, kW, sW, pW, Wo, ld, *norm);
    return hip_check(hipGetLastError(), "fold_kw_frames_u8 launch");
}


extern "C" int ptx_resize_frames_u8_supported(const ptx_resize_desc* desc) {
    ResizePlan p;
    return resize_plan(desc, nullptr, &p, "ptx_resize_frames_u8_supported") == PTX_OK;
}

// The windows entry points' own host-side checks: tables of h x w entries that hold an Ho x Wo window (no device needed).
static int resize_windows_check(const ptx_resize_desc* d, int h, int w, const char* who) {
    if (h < d->Ho || w < d->Wo)
        return fail(PTX_ERR_INVALID, "%s: the %dx%d window does not fit the %dx%d resized frame of the tables", who, d->Ho, d->Wo, h, w);
    if ((int64_t)h * d->taps_h > INT32_MAX || (int64_t)w * d->taps_w > INT32_MAX)
        return fail(PTX_ERR_UNSUPPORTED, "%s: a table exceeds 32-bit indexing", who);
    return PTX_OK;
}

// The normalisation of a launch that writes planes (left zeroed for uint8 output), checked.
static int resize_norm(const ptx_resize_desc* desc, const ptx_norm_desc* norm, ptx_norm_desc* nd, const char* who) {
    if (desc->out_mode == PTX_RESIZE_OUT_U8) return PTX_OK;
    if (!norm) return fail(PTX_ERR_INVALID, "%s: null norm descriptor", who);
    for (int c = 0; c < desc->C; ++c)
        if (!(norm->std[c] != 0.f)) return fail(PTX_ERR_INVALID, "%s: std[%d] must be non-zero", who, c);
    if (norm->swap_rb && desc->C < 3) return fail(PTX_ERR_INVALID, "%s: BGR swap needs 3 channels", who);
    *nd = *norm;
    return PTX_OK;
}

// All sources: `frames` (interleaved uint8) or, when src / src16 is not null, the planes of a YUV 4:2:0 source.  All three
// table modes: the fixed window (win == nullptr: the tables hold the window's entries), one window per clip (win->wins,
// tables of win->h x win->w entries) or tables per clip (per_clip: every table has a leading [N]).
static int resize_frames_run(const ptx_resize_desc* desc, const uint8_t* frames, const ptx_yuv420_src* src, const int32_t* row_lo,
                             const int32_t* row_n, const int32_t* row_k, const int32_t* col_lo, const int32_t* col_n,
                             const int32_t* col_k, void* y, const ptx_norm_desc* norm, ptx_stream_t stream, const char* who,
                             const ResizeWindows* win = nullptr, bool per_clip = false, const ptx_yuv420p16_src* src16 = nullptr) {
    ResizePlan p;
    int s = resize_plan(desc, y, &p, who);
    if (s) return s;
    if (src && (s = yuv_check(src, desc->C, desc->H, desc->W, who))) return s;
    if (src16 && (s = yuv_check(src16, desc->C, desc->H, desc->W, who))) return s;
    if (win && (s = resize_windows_check(desc, win->h, win->w, who))) return s;
    if ((!frames && !src && !src16) || !y || !row_lo || !row_n || !row_k || !col_lo || !col_n || !col_k || (win && !win->wins))
        return fail(PTX_ERR_INVALID, "%s: null pointer", who);
    ptx_norm_desc nd = {};
    if ((s = resize_norm(desc, norm, &nd, who))) return s;
    const dim3 grid((unsigned)((int64_t)desc->N * desc->T * cdiv(desc->Ho, p.band)));
    hipStream_t st = (hipStream_t)stream;
    const ResizeWindows rw = win ? *win : ResizeWindows{};
    const unsigned char* none = nullptr;
#define PTX_RESIZE_LAUNCH(CH, YUV, WIN, TAB)                                                                          \
    hipLaunchKernelGGL((resize_frames_u8_kernel<CH, YUV ? kSrcYuv8 : kSrcRgb, WIN, TAB>), grid, dim3(256), p.lds_bytes, st, *desc, \
                       YUV ? none : frames, row_lo, row_n, row_k, col_lo, col_n, col_k, y, nd, p, YUV ? *src : ptx_yuv420_src{}, \
                       rw, ResizeClips{})
#define PTX_RESIZE_LAUNCH16(WIN, TAB)                                                                                 \
    hipLaunchKernelGGL((resize_frames_u8_kernel<3, kSrcYuv16, WIN, TAB>), grid, dim3(256), p.lds_bytes, st, *desc, none, \
                       row_lo, row_n, row_k, col_lo, col_n, col_k, y, nd, p, *src16, rw, ResizeClips{})
#define PTX_RESIZE_LAUNCH_C(WIN, TAB)                          \
    switch (desc->C) {                                         \
        case 1: PTX_RESIZE_LAUNCH(1, false, WIN, TAB); break;  \
        case 2: PTX_RESIZE_LAUNCH(2, false, WIN, TAB); break;  \
        case 3: PTX_RESIZE_LAUNCH(3, false, WIN, TAB); break;  \
        default: PTX_RESIZE_LAUNCH(4, false, WIN, TAB); break; \
    }
    if (src16) {
        if (per_clip) {
            PTX_RESIZE_LAUNCH16(false, true);
        } else if (win) {
            PTX_RESIZE_LAUNCH16(true, false);
        } else {
            PTX_RESIZE_LAUNCH16(false, false);
        }
        return hip_check(hipGetLastError(), who);
    }
    if (src) {
        if (per_clip) {
            PTX_RESIZE_LAUNCH(3, true, false, true);
        } else if (win) {
            PTX_RESIZE_LAUNCH(3, true, true, false);
        } else {
            PTX_RESIZE_LAUNCH(3, true, false, false);
        }
        return hip_check(hipGetLastError(), who);
    }
    if (per_clip) {
        PTX_RESIZE_LAUNCH_C(false, true)
        return hip_check(hipGetLastError(), who);
    }
    if (win) {
        PTX_RESIZE_LAUNCH_C(true, false)
        return hip_check(hipGetLastError(), who);
    }
    PTX_RESIZE_LAUNCH_C(false, false)
#undef PTX_RESIZE_LAUNCH_C
#undef PTX_RESIZE_LAUNCH16
#undef PTX_RESIZE_LAUNCH
    return hip_check(hipGetLastError(), "ptx_resize_frames_u8 launch");
}

extern "C" int ptx_resize_frames_u8(const ptx_resize_desc* desc, const uint8_t* frames, const int32_t* row_lo,
                                    const int32_t* row_n, const int32_t* row_k, const int32_t* col_lo, const int32_t* col_n,
                                    const int32_t* col_k, void* y, const ptx_norm_desc* norm, ptx_stream_t stream) {
    return resize_frames_run(desc, frames, nullptr, row_lo, row_n, row_k, col_lo, col_n, col_k, y, norm, stream, "ptx_resize_frames_u8");
}

extern "C" int ptx_resize_frames_yuv420_supported(const ptx_resize_desc* desc, const ptx_yuv420_src* src) {
    const char* who = "ptx_resize_frames_yuv420_supported";
    ResizePlan p;
    return resize_plan(desc, nullptr, &p, who) == PTX_OK && yuv_check(src, desc->C, desc->H, desc->W, who) == PTX_OK;
}

extern "C" int ptx_resize_frames_yuv420(const ptx_resize_desc* desc, const ptx_yuv420_src* src, const int32_t* row_lo,
                                        const int32_t* row_n, const int32_t* row_k, const int32_t* col_lo, const int32_t* col_n,
                                        const int32_t* col_k, void* y, const ptx_norm_desc* norm, ptx_stream_t stream) {
    const char* who = "ptx_resize_frames_yuv420";
    if (!src) return fail(PTX_ERR_INVALID, "%s: null source descriptor", who);
    return resize_frames_run(desc, nullptr, src, row_lo, row_n, row_k, col_lo, col_n, col_k, y, norm, stream, who);
}

extern "C" int ptx_resize_frames_u8_windows_supported(const ptx_resize_desc* desc, int32_t h, int32_t w) {
    const char* who = "ptx_resize_frames_u8_windows_supported";
    ResizePlan p;
    return resize_plan(desc, nullptr, &p, who) == PTX_OK && resize_windows_check(desc, h, w, who) == PTX_OK;
}

extern "C" int ptx_resize_frames_u8_windows(const ptx_resize_desc* desc, const uint8_t* frames, const int32_t* row_lo,
                                            const int32_t* row_n, const int32_t* row_k, const int32_t* col_lo,
                                            const int32_t* col_n, const int32_t* col_k, int32_t h, int32_t w,
                                            const ptx_resize_window* windows, void* y, const ptx_norm_desc* norm,
                                            ptx_stream_t stream) {
    const ResizeWindows win = {windows, h, w};
    return resize_frames_run(desc, frames, nullptr, row_lo, row_n, row_k, col_lo, col_n, col_k, y, norm, stream,
                             "ptx_resize_frames_u8_windows", &win);
}

extern "C" int ptx_resize_frames_yuv420_windows_supported(const ptx_resize_desc* desc, const ptx_yuv420_src* src, int32_t h,
                                                          int32_t w) {
    const char* who = "ptx_resize_frames_yuv420_windows_supported";
    ResizePlan p;
    return resize_plan(desc, nullptr, &p, who) == PTX_OK && yuv_check(src, desc->C, desc->H, desc->W, who) == PTX_OK &&
           resize_windows_check(desc, h, w, who) == PTX_OK;
}

extern "C" int ptx_resize_frames_yuv420_windows(const ptx_resize_desc* desc, const ptx_yuv420_src* src, const int32_t* row_lo,
                                                const int32_t* row_n, const int32_t* row_k, const int32_t* col_lo,
                                                const int32_t* col_n, const int32_t* col_k, int32_t h, int32_t w,
                                                const ptx_resize_window* windows, void* y, const ptx_norm_desc* norm,
                                                ptx_stream_t stream) {
    const char* who = "ptx_resize_frames_yuv420_windows";
    if (!src) return fail(PTX_ERR_INVALID, "%s: null source descriptor", who);
    const ResizeWindows win = {windows, h, w};
    return resize_frames_run(desc, nullptr, src, row_lo, row_n, row_k, col_lo, col_n, col_k, y, norm, stream, who, &win);
}

// Per-clip tables (every table has a leading [N]; desc->taps_* is the common pitch) and their builder on the device.
extern "C" int ptx_resize_frames_u8_tables_supported(const ptx_resize_desc* desc) {
    ResizePlan p;
    return resize_plan(desc, nullptr, &p, "ptx_resize_frames_u8_tables_supported") == PTX_OK;
}

extern "C" int ptx_resize_frames_u8_tables(const ptx_resize_desc* desc, const uint8_t* frames, const int32_t* row_lo,
                                           const int32_t* row_n, const int32_t* row_k, const int32_t* col_lo,
                                           const int32_t* col_n, const int32_t* col_k, void* y, const ptx_norm_desc* norm,
                                           ptx_stream_t stream) {
    return resize_frames_run(desc, frames, nullptr, row_lo, row_n, row_k, col_lo, col_n, col_k, y, norm, stream,
                             "ptx_resize_frames_u8_tables", nullptr, true);
}

extern "C" int ptx_resize_frames_yuv420_tables_supported(const ptx_resize_desc* desc, const ptx_yuv420_src* src) {
    const char* who = "ptx_resize_frames_yuv420_tables_supported";
    ResizePlan p;
    return resize_plan(desc, nullptr, &p, who) == PTX_OK && yuv_check(src, desc->C, desc->H, desc->W, who) == PTX_OK;
}

extern "C" int ptx_resize_frames_yuv420_tables(const ptx_resize_desc* desc, const ptx_yuv420_src* src, const int32_t* row_lo,
                                               const int32_t* row_n, const int32_t* row_k, const int32_t* col_lo,
                                               const int32_t* col_n, const int32_t* col_k, void* y, const ptx_norm_desc* norm,
                                               ptx_stream_t stream) {
    const char* who = "ptx_resize_frames_yuv420_tables";
    if (!src) return fail(PTX_ERR_INVALID, "%s: null source descriptor", who);
    return resize_frames_run(desc, nullptr, src, row_lo, row_n, row_k, col_lo, col_n, col_k, y, norm, stream, who, nullptr, true);
}

// The same three launches on a 10- / 12-bit source (include/ptx_amd_yuv16.h).
extern "C" int ptx_resize_frames_yuv420p16_supported(const ptx_resize_desc* desc, const ptx_yuv420p16_src* src) {
    const char* who = "ptx_resize_frames_yuv420p16_supported";
    ResizePlan p;
    return resize_plan(desc, nullptr, &p, who) == PTX_OK && yuv_check(src, desc->C, desc->H, desc->W, who) == PTX_OK;
}

extern "C" int ptx_resize_frames_yuv420p16(const ptx_resize_desc* desc, const ptx_yuv420p16_src* src, const int32_t* row_lo,
                                           const int32_t* row_n, const int32_t* row_k, const int32_t* col_lo,
                                           const int32_t* col_n, const int32_t* col_k, void* y, const ptx_norm_desc* norm,
                                           ptx_stream_t stream) {
    const char* who = "ptx_resize_frames_yuv420p16";
    if (!src) return fail(PTX_ERR_INVALID, "%s: null source descriptor", who);
    return resize_frames_run(desc, nullptr, nullptr, row_lo, row_n, row_k, col_lo, col_n, col_k, y, norm, stream, who, nullptr,
                             false, src);
}

extern "C" int ptx_resize_frames_yuv420p16_windows_supported(const ptx_resize_desc* desc, const ptx_yuv420p16_src* src, int32_t h,
                                                             int32_t w) {
    const char* who = "ptx_resize_frames_yuv420p16_windows_supported";
    ResizePlan p;
    return resize_plan(desc, nullptr, &p, who) == PTX_OK && yuv_check(src, desc->C, desc->H, desc->W, who) == PTX_OK &&
           resize_windows_check(desc, h, w, who) == PTX_OK;
}

extern "C" int ptx_resize_frames_yuv420p16_windows(const ptx_resize_desc* desc, const ptx_yuv420p16_src* src,
                                                   const int32_t* row_lo, const int32_t* row_n, const int32_t* row_k,
                                                   const int32_t* col_lo, const int32_t* col_n, const int32_t* col_k, int32_t h,
                                                   int32_t w, const ptx_resize_window* windows, void* y,
                                                   const ptx_norm_desc* norm, ptx_stream_t stream) {
    const char* who = "ptx_resize_frames_yuv420p16_windows";
    if (!src) return fail(PTX_ERR_INVALID, "%s: null source descriptor", who);
    const ResizeWindows win = {windows, h, w};
    return resize_frames_run(desc, nullptr, nullptr, row_lo, row_n, row_k, col_lo, col_n, col_k, y, norm, stream, who, &win,
                             false, src);
}

extern "C" int ptx_resize_frames_yuv420p16_tables_supported(const ptx_resize_desc* desc, const ptx_yuv420p16_src* src) {
    const char* who = "ptx_resize_frames_yuv420p16_tables_supported";
    ResizePlan p;
    return resize_plan(desc, nullptr, &p, who) == PTX_OK && yuv_check(src, desc->C, desc->H, desc->W, who) == PTX_OK;
}

extern "C" int ptx_resize_frames_yuv420p16_tables(const ptx_resize_desc* desc, const ptx_yuv420p16_src* src, const int32_t* row_lo,
                                                  const int32_t* row_n, const int32_t* row_k, const int32_t* col_lo,
                                                  const int32_t* col_n, const int32_t* col_k, void* y,
                                                  const ptx_norm_desc* norm, ptx_stream_t stream) {
    const char* who = "ptx_resize_frames_yuv420p16_tables";
    if (!src) return fail(PTX_ERR_INVALID, "%s: null source descriptor", who);
    return resize_frames_run(desc, nullptr, nullptr, row_lo, row_n, row_k, col_lo, col_n, col_k, y, norm, stream, who, nullptr,
                             true, src);
}

static int resize_build_tables_run(const ptx_resize_desc* desc, const ptx_resize_geom* geoms, int filter, int32_t* row_lo,
                                   int32_t* row_n, int32_t* row_k, int32_t* col_lo, int32_t* col_n, int32_t* col_k,
                                   ptx_stream_t stream, const char* who) {
    ResizePlan p;
    int s = resize_plan(desc, nullptr, &p, who);                     // the extents and pitches the launch will be given
    if (s) return s;
    if ((s = resize_filter_check(filter, who))) return s;
    if (!geoms || !row_lo || !row_n || !row_k || !col_lo || !col_n || !col_k) return fail(PTX_ERR_INVALID, "%s: null pointer", who);
    const int64_t entries = (int64_t)desc->N * ((int64_t)desc->Ho + desc->Wo);
    if (entries > INT32_MAX) return fail(PTX_ERR_UNSUPPORTED, "%s: N * (Ho + Wo) exceeds 32-bit indexing", who);
    hipLaunchKernelGGL(resize_build_tables_kernel, dim3((unsigned)cdiv64(entries, 256)), dim3(256), 0, (hipStream_t)stream,
                       *desc, geoms, filter, row_lo, row_n, row_k, col_lo, col_n, col_k);
    return hip_check(hipGetLastError(), who);
}

extern "C" int ptx_resize_build_tables(const ptx_resize_desc* desc, const ptx_resize_geom* geoms, int32_t* row_lo,
                                       int32_t* row_n, int32_t* row_k, int32_t* col_lo, int32_t* col_n, int32_t* col_k,
                                       ptx_stream_t stream) {
    return resize_build_tables_run(desc, geoms, PTX_RESAMPLE_BILINEAR, row_lo, row_n, row_k, col_lo, col_n, col_k, stream,
                                   "ptx_resize_build_tables");
}

extern "C" int ptx_resize_build_tables_filter(const ptx_resize_desc* desc, const ptx_resize_geom* geoms, int32_t filter,
                                              int32_t* row_lo, int32_t* row_n, int32_t* row_k, int32_t* col_lo, int32_t* col_n,
                                              int32_t* col_k, ptx_stream_t stream) {
    return resize_build_tables_run(desc, geoms, filter, row_lo, row_n, row_k, col_lo, col_n, col_k, stream,
                                   "ptx_resize_build_tables_filter");
}

// y[r][0..W) = x[r][0..W), y[r][W..ld) = 0: gives rows whose length is not a multiple of 4 floats a 16-byte pitch
__global__ void __launch_bounds__(256) pad_rows_kernel(const float* __restrict__ x, float* __restrict__ y, size_t total,
                                                       int W, int ld) {
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
        const size_t r = e / (size_t)ld;
        const int c = (int)(e - r * (size_t)ld);
        y[e] = c < W ? x[r * (size_t)W + c] : 0.f;
    }
}

extern "C" int ptx_pad_rows(const float* x, float* y, int64_t rows, int32_t W, int32_t ld, ptx_stream_t stream) {
    if (!x || !y) return fail(PTX_ERR_INVALID, "pad_rows: null pointer");
    if (rows <= 0 || W <= 0 || ld < W) return fail(PTX_ERR_INVALID, "pad_rows: bad extents (rows=%lld W=%d ld=%d)", (long long)rows, W, ld);
    const size_t total = (size_t)rows * ld;
    hipLaunchKernelGGL(pad_rows_kernel, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, x, y, total, W, ld);
    return hip_check(hipGetLastError(), "pad_rows launch");
}

extern "C" int ptx_checksum_f32(const int64_t* table, int32_t n, uint64_t* out, ptx_stream_t stream) {
    if (!table || !out || n <= 0) return fail(PTX_ERR_INVALID, "checksum: null pointer / empty table");
    if (n > 65535) return fail(PTX_ERR_UNSUPPORTED, "checksum: more than 65535 tensors");
    hipLaunchKernelGGL(checksum_f32_kernel, dim3(32, (unsigned)n), dim3(256), 0, (hipStream_t)stream,
                       reinterpret_cast<const long long*>(table), n, reinterpret_cast<unsigned long long*>(out));
    return hip_check(hipGetLastError(), "checksum launch");
}

extern "C" int ptx_checksum_b16(const int64_t* table, int32_t n, uint64_t* out, ptx_stream_t stream) {
    if (!table || !out || n <= 0) return fail(PTX_ERR_INVALID, "checksum_b16: null pointer / empty table");
    if (n > 65535) return fail(PTX_ERR_UNSUPPORTED, "checksum_b16: more than 65535 tensors");
    hipLaunchKernelGGL(checksum_b16_kernel, dim3(32, (unsigned)n), dim3(256), 0, (hipStream_t)stream,
                       reinterpret_cast<const long long*>(table), n, reinterpret_cast<unsigned long long*>(out));
    return hip_check(hipGetLastError(), "checksum_b16 launch");
}

static int check_layout_b16(const void* x, const void* y, int N, int C, int64_t S, int ld, const void* cl) {
    if (!x || !y) return fail(PTX_ERR_INVALID, "layout_bf16: null pointer");
    if (N <= 0 || C <= 0 || S <= 0 || ld < C || ld % 8) return fail(PTX_ERR_INVALID, "layout_bf16: bad extents (ld %% 8 == 0, >= C)");
    if (N > 65535 || cdiv(ld, 32) > 65535 || cdiv64(S, 32) > 0x7fffffffLL) return fail(PTX_ERR_INVALID, "layout_bf16: extents too large for the grid");
    if ((uintptr_t)cl & 15) return fail(PTX_ERR_INVALID, "layout_bf16: the channels-last tensor must be 16-byte aligned");
    if (((uintptr_t)x | (uintptr_t)y) & 1) return fail(PTX_ERR_INVALID, "layout_bf16: misaligned pointer");
    return PTX_OK;
}

extern "C" int ptx_ncdhw_to_ndhwc_bf16(const void* x, void* y, int32_t N, int32_t C, int64_t S, int32_t ld, ptx_stream_t stream) {
    int s = check_layout_b16(x, y, N, C, S, ld, y);
    if (s) return s;
    dim3 grid((unsigned)cdiv64(S, 32), (unsigned)cdiv(ld, 32), (unsigned)N);
    hipLaunchKernelGGL(ncs_to_nsc_b16_kernel, grid, dim3(256), 0, (hipStream_t)stream, static_cast<const unsigned short*>(x),
                       static_cast<unsigned short*>(y), C, (long long)S, ld);
    return hip_check(hipGetLastError(), "ncdhw_to_ndhwc_bf16 launch");
}

extern "C" int ptx_ndhwc_to_ncdhw_bf16(const void* x, void* y, int32_t N, int32_t C, int64_t S, int32_t ld, ptx_stream_t stream) {
    int s = check_layout_b16(x, y, N, C, S, ld, x);
    if (s) return s;
    dim3 grid((unsigned)cdiv64(S, 32), (unsigned)cdiv(C, 32), (unsigned)N);
    hipLaunchKernelGGL(nsc_to_ncs_b16_kernel, grid, dim3(256), 0, (hipStream_t)stream, static_cast<const unsigned short*>(x),
                       static_cast<unsigned short*>(y), C, (long long)S, ld);
    return hip_check(hipGetLastError(), "ndhwc_to_ncdhw_bf16 launch");
}

extern "C" int ptx_im2col_hw_bf16(const void* x, void* y, int32_t N, int32_t C, int32_t T, int32_t H, int32_t W, int32_t kH,
                                  int32_t kW, int32_t sH, int32_t sW, int32_t pH, int32_t pW, int32_t Ho, int32_t Wo, int32_t ld,
                                  ptx_stream_t stream) {
    if (!x || !y) return fail(PTX_ERR_INVALID, "im2col_hw_bf16: null pointer");
    if (N <= 0 || C <= 0 || T <= 0 || H <= 0 || W <= 0 || kH <= 0 || kW <= 0 || sH <= 0 || sW <= 0 || pH < 0 || pW < 0 ||
        Ho <= 0 || Wo <= 0)
        return fail(PTX_ERR_INVALID, "im2col_hw_bf16: non-positive extent");
    if (ld % 32 || ld < kH * kW * C) return fail(PTX_ERR_INVALID, "im2col_hw_bf16: ld=%d must cover kH*kW*C=%d, multiple of 32", ld, kH * kW * C);
    if (Ho != (H + 2 * pH - kH) / sH + 1 || Wo != (W + 2 * pW - kW) / sW + 1)
        return fail(PTX_ERR_INVALID, "im2col_hw_bf16: output extent does not match the geometry");
    if (((uintptr_t)x & 1) || ((uintptr_t)y & 15)) return fail(PTX_ERR_INVALID, "im2col_hw_bf16: misaligned pointer");
    const long long total = (long long)N * T * Ho * Wo * (ld / 8);
    hipLaunchKernelGGL(im2col_hw_bf16_kernel, dim3(grid_for((size_t)total)), dim3(256), 0, (hipStream_t)stream,
                       static_cast<const unsigned short*>(x), static_cast<unsigned short*>(y), C, T, H, W, kH, kW, sH, sW, pH, pW,
                       Ho, Wo, ld, total);
    return hip_check(hipGetLastError(), "im2col_hw_bf16 launch");
}

extern "C" int ptx_f32_to_bf16(const float* x, void* y, int64_t n, ptx_stream_t stream) {
    if (!x || !y || n <= 0) return fail(PTX_ERR_INVALID, "f32_to_bf16: null pointer / empty");
    if ((uintptr_t)y & 1) return fail(PTX_ERR_INVALID, "f32_to_bf16: misaligned output");
    hipLaunchKernelGGL(f32_to_bf16_kernel, dim3(grid_for((size_t)n)), dim3(256), 0, (hipStream_t)stream, x,
                       static_cast<__bf16*>(y), (long long)n);
    return hip_check(hipGetLastError(), "f32_to_bf16 launch");
}

extern "C" int ptx_bf16_to_f32(const void* x, float* y, int64_t n, ptx_stream_t stream) {
    if (!x || !y || n <= 0) return fail(PTX_ERR_INVALID, "bf16_to_f32: null pointer / empty");
    if (((uintptr_t)x & 1) || ((uintptr_t)y & 3)) return fail(PTX_ERR_INVALID, "bf16_to_f32: misaligned pointer");
    hipLaunchKernelGGL(bf16_to_f32_kernel, dim3(grid_for((size_t)n)), dim3(256), 0, (hipStream_t)stream,
                       static_cast<const __bf16*>(x), y, (long long)n);
    return hip_check(hipGetLastError(), "bf16_to_f32 launch");
}

// The multi-view resize kernel is a file of its own compiled as part of this translation unit (build.py follows the
// include, so its bytes are in this object's stamp and in ptx_version()'s source hash).
#include "resize_views.hip"

// So are the entry points that sample training clips from videos of any size (a source row per clip).
#include "resize_clips.hip"

// So is the patch-resident bf16 stem (it normalises uint8 frames with resize_common.h's normalise_u8 while it stages them).
#include "conv_stem_bf16.hip"

// So are the Winograd F(2x2, 3x3) transforms around the grouped implicit GEMM (two memory-bound passes and a filter transform).
#include "conv_wino_f32.hip"

// So is the fp32 stem as a fast FIR along time (a filter transform, a memory-bound input transform and the stem's step loop over
// the transformed frames).
#include "conv_stem_tfir_f32.hip"

// So are the per-clip ColorJitter / RandomGrayscale launches on uint8 frames (include/ptx_amd_color.h): the statistics and
// the apply kernel, whose plane output is ptx_frames_u8_to_ncdhw's value of the jittered byte.
#include "color_jitter.h"

// So are the per-clip RandAugment launches (include/ptx_amd_randaug.h): per op position a statistics kernel (histograms and the
// luma sum of every frame, when an op needs them) and an apply kernel that shares color_jitter.h's blend, luma and mean.
#include "rand_augment.h"

// So is the last stage of the training input path (include/ptx_amd_mix.h): RandomErasing per clip and MixUp / CutMix across the
// clips of the batch on the normalised values, from uint8 frames or a normalised clip, in one launch that writes the NCDHW clip.
#include "batch_mix.h"

// So are the interpolated per-clip warps (include/ptx_amd_warp.h): affine and perspective transforms of uint8 frames with
// Pillow's bilinear / bicubic interpolation in fp64, one launch per batch.
#include "warp_frames.h"

// So is the per-clip GaussianBlur (include/ptx_amd_blur.h): a separable fp64 blur with reflect padding over LDS tiles, one launch
// per batch, whose plane output is ptx_frames_u8_to_ncdhw's value of the blurred byte.
#include "blur_frames.h"

// So are the class activation maps (include/ptx_amd_cam.h): the classifier rows applied at every position of the final feature
// map, one uint8 map per class, and its Pillow-exact overlay on uint8 frames through the resize tables above.
#include "cam.h"
