// Interpolated per-clip warps of decoded uint8 frames [N][T][H][W][3]: affine and perspective with Pillow's bilinear or bicubic
// interpolation (nearest for a perspective), equal to Image.transform bit for bit (include/ptx_amd_warp.h states the arithmetic;
// transforms.warp_numpy is its numpy statement).  Compiled as part of pack_layout.hip's translation unit, behind batch_mix.h.
//
// warp_frames_kernel runs over (tile, t, n): a workgroup owns a kWarpTileW x kWarpTileH tile of one frame of one clip, so the
// clip's kind and its eight coefficients are uniform over the workgroup (scalar loads, scalar branches), and a rotated tile's
// source footprint is a compact patch, not a long diagonal run.  A lane owns one output pixel, all three channels: the source
// coordinate is computed once, in fp64 with contraction off and in Pillow's operation order, and the 4 (bilinear) or 16
// (bicubic) taps are gathers through L1 / L2: a row's taps are 6 or 12 consecutive bytes, read as the dwords that hold them
// (any alignment), not byte by byte -- the launch is bound by the number of gather instructions, not by their bytes or by the
// fp64 arithmetic.  A lane's three output bytes follow its neighbour's.
//
// Every tap index is clamped or tested against the frame before it is used and a coordinate is converted to an integer only
// after it was found inside the frame, so no row -- also none that ptx_warp_frames_supported refuses -- reads or writes out of
// bounds.  Offsets inside a frame are 32-bit (a frame is below 2^31 bytes), frame bases are 64-bit.
#pragma once
#include "batch_mix.h"
#include "../../include/ptx_amd_warp.h"
#include <cmath>

namespace ptx {

constexpr int kWarpTileW = 32;
constexpr int kWarpTileH = 8;                          // 256 pixels per workgroup, one per lane

__host__ __device__ __forceinline__ double warp_denominator(double a6, double a7, double X, double Y) {
#pragma clang fp contract(off)
    return a6 * X + a7 * Y + 1.0;
}

// The source coordinate of output pixel (x, y): Geometry.c's affine_transform / perspective_transform
__device__ __forceinline__ void warp_source(int kind, const double (&a)[8], int x, int y, double& xin, double& yin) {
#pragma clang fp contract(off)
    const double X = (double)x + 0.5, Y = (double)y + 0.5;
    xin = a[0] * X + a[1] * Y + a[2];
    yin = a[3] * X + a[4] * Y + a[5];
    if (kind == PTX_WARP_PERSPECTIVE) {
        const double den = warp_denominator(a[6], a[7], X, Y);
        xin = xin / den;
        yin = yin / den;
    }
}

__device__ __forceinline__ double warp_lerp(int v0, int v1, double d) {
#pragma clang fp contract(off)
    return (double)v0 + (double)(v1 - v0) * d;
}

__device__ __forceinline__ double warp_lerp(double v0, double v1, double d) {
#pragma clang fp contract(off)
    return v0 + (v1 - v0) * d;
}

// Geometry.c's BICUBIC macro, on doubles (the row pass takes bytes, whose integer sums are the same numbers)
__device__ __forceinline__ double warp_cubic(double v1, double v2, double v3, double v4, double d) {
#pragma clang fp contract(off)
    const double p1 = v2;
    const double p2 = -v1 + v3;
    const double p3 = 2.0 * (v1 - v2) + v3 - v4;
    const double p4 = -v1 + v2 - v3 + v4;
    return p1 + d * (p2 + d * (p3 + d * p4));
}

// Any-alignment loads of 4 and 2 bytes (gfx950 global loads take unaligned addresses): one instruction, not one per byte
__device__ __forceinline__ unsigned warp_load4(const unsigned char* p) {
    unsigned v;
    __builtin_memcpy(&v, p, 4);
    return v;
}

__device__ __forceinline__ unsigned warp_load2(const unsigned char* p) {
    unsigned short v;
    __builtin_memcpy(&v, p, 2);
    return v;
}

// The NP taps of a row at columns clamp(xi) .. clamp(xi + NP - 1), three channels each.  Where no column is clamped the taps
// are 3 * NP consecutive bytes, read as the dwords (and, for two taps, the halfword) that hold exactly those bytes; a lane at
// the frame's edge reads its taps byte by byte.
template <int NP>
__device__ __forceinline__ void warp_taps(const unsigned char* __restrict__ row, int xi, int W, int (&c)[NP][3]) {
    static_assert(NP == 2 || NP == 4, "two (bilinear) or four (bicubic) taps");
    if (xi >= 0 && xi + NP - 1 < W) {
        const unsigned char* p = row + 3 * xi;
        unsigned d[3];
        d[0] = warp_load4(p);
        if (NP == 2) {
            d[1] = warp_load2(p + 4), d[2] = 0;
        } else {
            d[1] = warp_load4(p + 4), d[2] = warp_load4(p + 8);
        }
#pragma unroll
        for (int j = 0; j < NP; ++j)
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                const int b = 3 * j + ch;
                c[j][ch] = (int)((d[b >> 2] >> (8 * (b & 3))) & 255u);
            }
        return;
    }
#pragma unroll
    for (int j = 0; j < NP; ++j) {
        const int xo = 3 * min(max(xi + j, 0), W - 1);
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) c[j][ch] = row[xo + ch];
    }
}

template <int FILTER>
__global__ void __launch_bounds__(256) warp_frames_kernel(const unsigned char* __restrict__ frames, const int* __restrict__ kinds,
                                                          const double* __restrict__ coeffs, unsigned char* __restrict__ y, int T, int H,
                                                          int W, int tiles_x, int fill_r, int fill_g, int fill_b) {
    const int tile = blockIdx.x, t = blockIdx.y, n = blockIdx.z;
    const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
    const int x = tx * kWarpTileW + (threadIdx.x & (kWarpTileW - 1));
    const int yy = ty * kWarpTileH + (threadIdx.x / kWarpTileW);
    if (x >= W || yy >= H) return;
    int kind = kinds[n];                               // uniform over the workgroup
    if (kind != PTX_WARP_AFFINE && kind != PTX_WARP_PERSPECTIVE) kind = PTX_WARP_IDENTITY;
    const size_t frame = ((size_t)n * T + t) * ((size_t)H * W * 3);
    const unsigned char* fin = frames + frame;
    unsigned char* o = y + frame + 3 * (yy * W + x);
    if (kind == PTX_WARP_IDENTITY) {
        const unsigned char* q = fin + 3 * (yy * W + x);
        o[0] = q[0], o[1] = q[1], o[2] = q[2];
        return;
    }
    double a[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) a[i] = coeffs[(size_t)n * PTX_WARP_COEFFS + i];
    double xin, yin;
    warp_source(kind, a, x, yy, xin, yin);
    // written so that a coordinate that is not a number is outside
    if (!(xin >= 0.0 && xin < (double)W && yin >= 0.0 && yin < (double)H)) {
        o[0] = (unsigned char)fill_r, o[1] = (unsigned char)fill_g, o[2] = (unsigned char)fill_b;
        return;
    }
    if (FILTER == PTX_RESAMPLE_NEAREST) {              // 0 <= xin < W: (int)xin is 0 .. W - 1
        const unsigned char* q = fin + 3 * ((int)yin * W + (int)xin);
        o[0] = q[0], o[1] = q[1], o[2] = q[2];
        return;
    }
    xin -= 0.5, yin -= 0.5;                            // -0.5 <= xin < W - 0.5: the floor is -1 .. W - 1
    const double fx = floor(xin), fy = floor(yin);
    const double dx = xin - fx, dy = yin - fy;
    int xi = (int)fx, yi = (int)fy;
    if (FILTER == PTX_RESAMPLE_BILINEAR) {
        const bool two = yi + 1 >= 0 && yi + 1 < H;
        int c0[2][3], c1[2][3] = {};
        warp_taps<2>(fin + min(max(yi, 0), H - 1) * (W * 3), xi, W, c0);
        if (two) warp_taps<2>(fin + (yi + 1) * (W * 3), xi, W, c1);
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const double v1 = warp_lerp(c0[0][ch], c0[1][ch], dx);
            const double v2 = two ? warp_lerp(c1[0][ch], c1[1][ch], dx) : v1;
            o[ch] = (unsigned char)(int)warp_lerp(v1, v2, dy);       // 0 <= the value <= 255: the conversion truncates
        }
        return;
    }
    xi -= 1, yi -= 1;
    double v[3][4];                                    // per channel the four row results; a row outside takes the one before
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int r = yi + k;
        const bool in = k == 0 || (r >= 0 && r < H);   // row 0 is clamped, the others are tested
        if (in) {
            int c[4][3];
            warp_taps<4>(fin + min(max(r, 0), H - 1) * (W * 3), xi, W, c);
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) v[ch][k] = warp_cubic((double)c[0][ch], (double)c[1][ch], (double)c[2][ch], (double)c[3][ch], dx);
        } else {
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) v[ch][k] = v[ch][k > 0 ? k - 1 : 0];
        }
    }
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        const double r = warp_cubic(v[ch][0], v[ch][1], v[ch][2], v[ch][3], dy);
        o[ch] = r <= 0.0 ? (unsigned char)0 : r >= 255.0 ? (unsigned char)255 : (unsigned char)(int)r;
    }
}

// Host-side checks shared by the two entry points (no device needed).
static int warp_desc_check(const ptx_warp_desc* d, const char* who) {
    if (!d) return fail(PTX_ERR_INVALID, "%s: null descriptor", who);
    if (d->N <= 0 || d->T <= 0 || d->H <= 0 || d->W <= 0)
        return fail(PTX_ERR_INVALID, "%s: non-positive extent (N=%d T=%d H=%d W=%d)", who, d->N, d->T, d->H, d->W);
    if (d->filter != PTX_RESAMPLE_NEAREST && d->filter != PTX_RESAMPLE_BILINEAR && d->filter != PTX_RESAMPLE_BICUBIC)
        return fail(PTX_ERR_INVALID, "%s: filter=%d must be PTX_RESAMPLE_NEAREST, PTX_RESAMPLE_BILINEAR or PTX_RESAMPLE_BICUBIC", who,
                    d->filter);
    if ((unsigned)d->fill_r > 255u || (unsigned)d->fill_g > 255u || (unsigned)d->fill_b > 255u)
        return fail(PTX_ERR_INVALID, "%s: fill (%d, %d, %d) must be 0..255", who, d->fill_r, d->fill_g, d->fill_b);
    const int64_t P = (int64_t)d->H * d->W;
    if (P * 3 > INT32_MAX) return fail(PTX_ERR_UNSUPPORTED, "%s: a frame of %dx%d pixels exceeds 32-bit indexing", who, d->H, d->W);
    if (d->T > 65535 || d->N > 65535)
        return fail(PTX_ERR_UNSUPPORTED, "%s: %d x %d frames exceed the grid (N, T <= 65535)", who, d->N, d->T);
    return PTX_OK;
}

}  // namespace ptx

using namespace ptx;

extern "C" int ptx_warp_frames_supported(const ptx_warp_desc* desc, const int32_t* kinds, const double* coeffs) {
    const char* who = "ptx_warp_frames_supported";
    if (warp_desc_check(desc, who)) return 0;
    if (!kinds || !coeffs) return fail(PTX_ERR_INVALID, "%s: null pointer", who), 0;
    for (int n = 0; n < desc->N; ++n) {
        const int kind = kinds[n];
        const double* a = coeffs + (size_t)n * PTX_WARP_COEFFS;
        if (kind < PTX_WARP_IDENTITY || kind > PTX_WARP_PERSPECTIVE)
            return fail(PTX_ERR_INVALID, "%s: clip %d: kind %d out of range 0..%d", who, n, kind, PTX_WARP_PERSPECTIVE), 0;
        if (kind == PTX_WARP_IDENTITY) continue;
        if (kind == PTX_WARP_AFFINE && desc->filter == PTX_RESAMPLE_NEAREST)
            return fail(PTX_ERR_UNSUPPORTED, "%s: clip %d: a nearest affine warp is PIL's 16.16 fixed-point walk: run it as a geometric "
                        "row of ptx_rand_augment_apply", who, n), 0;
        for (int i = 0; i < (kind == PTX_WARP_AFFINE ? 6 : 8); ++i)
            if (!std::isfinite(a[i]))
                return fail(PTX_ERR_INVALID, "%s: clip %d: coefficient a%d = %g is not finite", who, n, i, a[i]), 0;
        if (kind == PTX_WARP_PERSPECTIVE) {
            int pos = 0, neg = 0;
            for (int c = 0; c < 4; ++c) {
                const double X = (c & 1) ? (double)desc->W - 0.5 : 0.5, Y = (c & 2) ? (double)desc->H - 0.5 : 0.5;
                const double den = warp_denominator(a[6], a[7], X, Y);
                pos += den > 0.0, neg += den < 0.0;
            }
            if (pos != 4 && neg != 4)
                return fail(PTX_ERR_INVALID, "%s: clip %d: the perspective denominator a6 * X + a7 * Y + 1 changes sign or vanishes on the "
                            "%dx%d frame (a6 = %g, a7 = %g): a degenerate quadrilateral", who, n, desc->H, desc->W, a[6], a[7]), 0;
        }
    }
    return 1;
}

extern "C" int ptx_warp_frames(const ptx_warp_desc* desc, const uint8_t* frames, const int32_t* kinds, const double* coeffs, uint8_t* y,
                               ptx_stream_t stream) {
    const char* who = "ptx_warp_frames";
    int s = warp_desc_check(desc, who);
    if (s) return s;
    if (!frames || !kinds || !coeffs || !y) return fail(PTX_ERR_INVALID, "%s: null pointer", who);
    if ((uintptr_t)kinds & 3) return fail(PTX_ERR_INVALID, "%s: misaligned kinds", who);
    if ((uintptr_t)coeffs & 7) return fail(PTX_ERR_INVALID, "%s: misaligned coefficients", who);
    const int tiles_x = cdiv(desc->W, kWarpTileW), tiles_y = cdiv(desc->H, kWarpTileH);
    const dim3 grid((unsigned)((int64_t)tiles_x * tiles_y), (unsigned)desc->T, (unsigned)desc->N);
    const hipStream_t st = (hipStream_t)stream;
    if (desc->filter == PTX_RESAMPLE_NEAREST)
        hipLaunchKernelGGL(warp_frames_kernel<PTX_RESAMPLE_NEAREST>, grid, dim3(256), 0, st, frames, kinds, coeffs, y, desc->T, desc->H,
                           desc->W, tiles_x, desc->fill_r, desc->fill_g, desc->fill_b);
    else if (desc->filter == PTX_RESAMPLE_BILINEAR)
        hipLaunchKernelGGL(warp_frames_kernel<PTX_RESAMPLE_BILINEAR>, grid, dim3(256), 0, st, frames, kinds, coeffs, y, desc->T, desc->H,
                           desc->W, tiles_x, desc->fill_r, desc->fill_g, desc->fill_b);
    else
        hipLaunchKernelGGL(warp_frames_kernel<PTX_RESAMPLE_BICUBIC>, grid, dim3(256), 0, st, frames, kinds, coeffs, y, desc->T, desc->H,
                           desc->W, tiles_x, desc->fill_r, desc->fill_g, desc->fill_b);
    return hip_check(hipGetLastError(), "warp_frames launch");
}
