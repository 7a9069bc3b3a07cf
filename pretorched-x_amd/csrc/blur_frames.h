// Per-clip GaussianBlur of decoded uint8 frames [N][T][H][W][3]: a separable blur in fp64 with reflect padding, a pure function
// of the bytes and the clip's fp32 weights (include/ptx_amd_blur.h states the arithmetic; transforms.gaussian_blur_numpy is its
// numpy statement).  Compiled as part of pack_layout.hip's translation unit, behind warp_frames.h.
//
// blur_frames_kernel runs over (tile, t, n): a workgroup owns a kBlurTile x kBlurTile tile of one frame of one clip, all three
// channels, so the clip's flag and weights are uniform over the workgroup; they are read once and widened to double in LDS.
//   1. stage: the tile plus its (kx - 1) x (ky - 1) halo, (32 + ky - 1) rows of (32 + kx - 1) pixels, from the interleaved frame
//      into LDS with reflect indexing (byte loads: any alignment; every index is clamped into the frame after it is reflected);
//   2. horizontal pass: every staged row into a row of 96 doubles in LDS.  A work item is four neighbouring pixels of one
//      channel of one row: it keeps a window of four bytes in registers and reads ONE new byte per tap.  A product of an fp32
//      weight and a byte is exact in fp64, so fma(w, p, acc) is the contract's multiply and add in one instruction;
//   3. vertical pass from LDS: a work item is four rows of one column, a window of four doubles, one new double per tap.  Here
//      the product rounds, so multiply and add stay two instructions: contraction is off for the body, as in warp_frames.h;
//   4. round half to even (v_rndne_f64), clamp, write the byte or its normalised value.
// A clip whose flag is 0 runs the same code with one tap of weight 1.0 per pass: 1.0 * p + 0.0 is p, a byte-for-byte copy.
// LDS: 16 * 33 bytes of weights + (32 + ky - 1) * (96 * 8 + (32 + kx - 1) * 3) + 16 bytes, 36 KiB at 9 taps, 50 KiB at 23, 61 KiB at
// 33 (dynamic, below the 64 KiB a launch gets without asking).  The arithmetic of the choice is in DESIGN.md 3.41.
// Offsets inside a frame are 32-bit (a frame is below 2^31 bytes), frame and plane bases are 64-bit.
#pragma once
#include "warp_frames.h"
#include "../../include/ptx_amd_blur.h"
#include <cmath>

namespace ptx {

constexpr int kBlurTile = 32;                          // output pixels per tile side
constexpr int kBlurCols = kBlurTile * 3;               // doubles per row of the horizontal pass
constexpr int kBlurRun = 4;                            // outputs per work item of a pass
constexpr int kBlurTaps = PTX_BLUR_MAX_TAPS;
// Both passes load the window's next element while they run a tap, also behind the last tap (an unconditional load lets the
// compiler issue the loads of an unrolled group of taps together; that value is not used).  Behind the last tap the horizontal
// pass reads the pixel that follows its row's last staged pixel -- for the last row up to 3 bytes past the staged bytes, which
// are therefore followed by kBlurPad bytes --, the vertical pass the row behind the last row of doubles, 768 bytes that lie in
// the staged bytes (at least 32 * 32 * 3 of them).
constexpr int kBlurPad = 16;
static_assert(kBlurCols * 8 <= kBlurTile * kBlurTile * 3, "the vertical pass's look-ahead stays inside the staged bytes");
static_assert(3 <= kBlurPad, "the horizontal pass's look-ahead stays inside the pad");

__host__ __device__ __forceinline__ int blur_lds_bytes(int kx, int ky) {
    const int sh = kBlurTile + ky - 1, sw = kBlurTile + kx - 1;
    return 2 * kBlurTaps * 8 + sh * kBlurCols * 8 + sh * sw * 3 + kBlurPad;
}

// torch's "reflect" index, then clamped: inside the frame whatever i is (a tile's halo beyond a ragged edge is never used)
__device__ __forceinline__ int blur_reflect(int i, int n) {
    i = i < 0 ? -i : (i >= n ? 2 * (n - 1) - i : i);
    return min(max(i, 0), n - 1);
}

// four outputs of the vertical pass: acc[r] = sum_i wy[i] * h[(y0 + r + i)][col], the multiply and the add rounded one by one
__device__ __forceinline__ void blur_column(const double* __restrict__ hp, const double* __restrict__ wy, int ky, double (&acc)[kBlurRun]) {
#pragma clang fp contract(off)
    double win[kBlurRun];
#pragma unroll
    for (int r = 0; r < kBlurRun; ++r) win[r] = hp[r * kBlurCols], acc[r] = 0.0;
#pragma unroll 4
    for (int i = 0; i < ky; ++i) {
        const double w = wy[i];
#pragma unroll
        for (int r = 0; r < kBlurRun; ++r) {
            const double prod = w * win[r];
            acc[r] = acc[r] + prod;
        }
#pragma unroll
        for (int r = 0; r + 1 < kBlurRun; ++r) win[r] = win[r + 1];
        win[kBlurRun - 1] = hp[(i + kBlurRun) * kBlurCols];   // behind the last tap: inside the allocation, not used
    }
}

__device__ __forceinline__ int blur_round8(double v) {
    const double r = __builtin_rint(v);                // round half to even (the default rounding mode)
    return r <= 0.0 ? 0 : (r >= 255.0 ? 255 : (int)r);
}

template <int OUT>
__global__ void __launch_bounds__(256) blur_frames_kernel(const unsigned char* __restrict__ frames, const int* __restrict__ apply,
                                                          const float* __restrict__ wx, const float* __restrict__ wy,
                                                          void* __restrict__ y, int T, int H, int W, int kx_all, int ky_all, int tiles_x,
                                                          ptx_norm_desc nd) {
    extern __shared__ double blur_lds[];
    const int tile = blockIdx.x, t = blockIdx.y, n = blockIdx.z;
    const int tyi = tile / tiles_x, txi = tile - tyi * tiles_x;
    const int tx0 = txi * kBlurTile, ty0 = tyi * kBlurTile;
    const bool on = apply[n] != 0;                     // uniform over the workgroup
    const int kx = on ? kx_all : 1, ky = on ? ky_all : 1;
    const int rx = kx >> 1, ry = ky >> 1;
    const int sw = kBlurTile + kx - 1, sh = kBlurTile + ky - 1;
    double* s_wx = blur_lds;
    double* s_wy = s_wx + kBlurTaps;
    double* s_h = s_wy + kBlurTaps;                    // [sh][96]
    unsigned char* s_px = reinterpret_cast<unsigned char*>(s_h + sh * kBlurCols);   // [sh][sw][3]
    const int tid = threadIdx.x;
    if (tid < kx) s_wx[tid] = on ? (double)wx[(size_t)n * kx_all + tid] : 1.0;
    if (tid >= 64 && tid - 64 < ky) s_wy[tid - 64] = on ? (double)wy[(size_t)n * ky_all + (tid - 64)] : 1.0;
    const size_t P = (size_t)H * W;
    const unsigned char* fin = frames + ((size_t)n * T + t) * P * 3;
    for (int idx = tid; idx < sh * sw; idx += 256) {
        const int sy = idx / sw, sx = idx - sy * sw;
        const int gy = blur_reflect(ty0 + sy - ry, H), gx = blur_reflect(tx0 + sx - rx, W);
        const unsigned char* q = fin + 3 * (gy * W + gx);
        unsigned char* d = s_px + 3 * idx;
        d[0] = q[0], d[1] = q[1], d[2] = q[2];
    }
    __syncthreads();
    // horizontal pass: item = (row, group of four pixels, channel)
    constexpr int kGroups = kBlurTile / kBlurRun;
    for (int item = tid; item < sh * kGroups * 3; item += 256) {
        const int row = item / (kGroups * 3), rest = item - row * (kGroups * 3);
        const int xg = rest / 3, ch = rest - xg * 3;
        const unsigned char* p = s_px + (row * sw + xg * kBlurRun) * 3 + ch;
        double win[kBlurRun], acc[kBlurRun];
#pragma unroll
        for (int r = 0; r < kBlurRun; ++r) win[r] = (double)p[3 * r], acc[r] = 0.0;
#pragma unroll 4
        for (int j = 0; j < kx; ++j) {
            const double w = s_wx[j];
#pragma unroll
            for (int r = 0; r < kBlurRun; ++r) acc[r] = __builtin_fma(w, win[r], acc[r]);   // w * byte is exact: one rounding, the add's
#pragma unroll
            for (int r = 0; r + 1 < kBlurRun; ++r) win[r] = win[r + 1];
            win[kBlurRun - 1] = (double)p[3 * (j + kBlurRun)];   // behind the last tap: inside the pad, not used
        }
        double* hrow = s_h + row * kBlurCols + xg * kBlurRun * 3 + ch;
#pragma unroll
        for (int r = 0; r < kBlurRun; ++r) hrow[3 * r] = acc[r];
    }
    __syncthreads();
    // vertical pass: item = (group of four rows, column).  uint8 out: columns in the frame's interleaved order, a wave's bytes are
    // consecutive; plane out: channel by channel, a wave's elements of a plane row are consecutive.
    const size_t frame = (size_t)n * T + t;
    for (int item = tid; item < kGroups * kBlurCols; item += 256) {
        const int yg = item / kBlurCols, c = item - yg * kBlurCols;
        int x, ch;
        if (OUT == PTX_RESIZE_OUT_U8) {
            x = c / 3, ch = c - x * 3;
        } else {
            ch = c / kBlurTile, x = c - ch * kBlurTile;
        }
        const int gx = tx0 + x, gy0 = ty0 + yg * kBlurRun;
        if (gx >= W || gy0 >= H) continue;
        double acc[kBlurRun];
        blur_column(s_h + yg * kBlurRun * kBlurCols + x * 3 + ch, s_wy, ky, acc);
        // input channel ch is plane co of the normalised clip
        const int co = (nd.swap_rb && ch != 1) ? 2 - ch : ch;
#pragma unroll
        for (int r = 0; r < kBlurRun; ++r) {
            const int gy = gy0 + r;
            if (gy >= H) break;
            const int b = blur_round8(acc[r]);
            const int pix = gy * W + gx;
            if (OUT == PTX_RESIZE_OUT_U8) {
                static_cast<unsigned char*>(y)[frame * P * 3 + (3 * pix + ch)] = (unsigned char)b;
            } else {
                const float v = normalise_u8((unsigned char)b, nd.mean[co], nd.std[co], nd.to_255);
                const size_t o = (((size_t)n * 3 + co) * T + t) * P + pix;
                if (OUT == PTX_RESIZE_OUT_F32)
                    static_cast<float*>(y)[o] = v;
                else
                    static_cast<unsigned short*>(y)[o] = __builtin_bit_cast(unsigned short, (__bf16)v);   // nearest even, as PTX_RESIZE_OUT_BF16
            }
        }
    }
}

// Host-side checks shared by the two entry points (no device needed).
static int blur_desc_check(const ptx_blur_desc* d, const char* who) {
    if (!d) return fail(PTX_ERR_INVALID, "%s: null descriptor", who);
    if (d->N <= 0 || d->T <= 0 || d->H <= 0 || d->W <= 0)
        return fail(PTX_ERR_INVALID, "%s: non-positive extent (N=%d T=%d H=%d W=%d)", who, d->N, d->T, d->H, d->W);
    if (d->kx <= 0 || d->ky <= 0 || !(d->kx & 1) || !(d->ky & 1) || d->kx > PTX_BLUR_MAX_TAPS || d->ky > PTX_BLUR_MAX_TAPS)
        return fail(PTX_ERR_INVALID, "%s: tap counts kx=%d ky=%d must be odd and 1..PTX_BLUR_MAX_TAPS = %d", who, d->kx, d->ky,
                    PTX_BLUR_MAX_TAPS);
    if (d->kx / 2 >= d->W || d->ky / 2 >= d->H)
        return fail(PTX_ERR_INVALID, "%s: reflect padding needs kx / 2 < W and ky / 2 < H (kx=%d ky=%d H=%d W=%d)", who, d->kx, d->ky,
                    d->H, d->W);
    if (d->out_mode != PTX_RESIZE_OUT_U8 && d->out_mode != PTX_RESIZE_OUT_F32 && d->out_mode != PTX_RESIZE_OUT_BF16)
        return fail(PTX_ERR_INVALID, "%s: out_mode=%d is not a PTX_RESIZE_OUT_* value", who, d->out_mode);
    const int64_t P = (int64_t)d->H * d->W;
    if (P * 3 > INT32_MAX) return fail(PTX_ERR_UNSUPPORTED, "%s: a frame of %dx%d pixels exceeds 32-bit indexing", who, d->H, d->W);
    if (d->T > 65535 || d->N > 65535)
        return fail(PTX_ERR_UNSUPPORTED, "%s: %d x %d frames exceed the grid (N, T <= 65535)", who, d->N, d->T);
    return PTX_OK;
}

}  // namespace ptx

using namespace ptx;

extern "C" int ptx_gaussian_blur_supported(const ptx_blur_desc* desc, const int32_t* apply, const float* wx, const float* wy) {
    const char* who = "ptx_gaussian_blur_supported";
    if (blur_desc_check(desc, who)) return 0;
    if (!apply || !wx || !wy) return fail(PTX_ERR_INVALID, "%s: null pointer", who), 0;
    for (int n = 0; n < desc->N; ++n) {
        if (apply[n] != 0 && apply[n] != 1) return fail(PTX_ERR_INVALID, "%s: clip %d: apply flag %d is not 0 or 1", who, n, apply[n]), 0;
        for (int j = 0; j < desc->kx; ++j) {
            const float w = wx[(size_t)n * desc->kx + j];
            if (!(w >= 0.f) || !std::isfinite(w))
                return fail(PTX_ERR_INVALID, "%s: clip %d: weight wx[%d] = %g must be finite and >= 0", who, n, j, (double)w), 0;
        }
        for (int i = 0; i < desc->ky; ++i) {
            const float w = wy[(size_t)n * desc->ky + i];
            if (!(w >= 0.f) || !std::isfinite(w))
                return fail(PTX_ERR_INVALID, "%s: clip %d: weight wy[%d] = %g must be finite and >= 0", who, n, i, (double)w), 0;
        }
    }
    return 1;
}

extern "C" int ptx_gaussian_blur_frames(const ptx_blur_desc* desc, const uint8_t* frames, const int32_t* apply, const float* wx,
                                        const float* wy, void* y, const ptx_norm_desc* norm, ptx_stream_t stream) {
    const char* who = "ptx_gaussian_blur_frames";
    int s = blur_desc_check(desc, who);
    if (s) return s;
    if (!frames || !apply || !wx || !wy || !y) return fail(PTX_ERR_INVALID, "%s: null pointer", who);
    if ((const void*)y == (const void*)frames) return fail(PTX_ERR_INVALID, "%s: y must not be frames (the blur reads neighbours)", who);
    if (((uintptr_t)apply | (uintptr_t)wx | (uintptr_t)wy) & 3) return fail(PTX_ERR_INVALID, "%s: misaligned flags or weights", who);
    ptx_norm_desc nd = {};
    if (desc->out_mode != PTX_RESIZE_OUT_U8) {
        if ((s = check_norm(norm, 3))) return s;
        nd = *norm;
        if ((uintptr_t)y & (desc->out_mode == PTX_RESIZE_OUT_F32 ? 3 : 1)) return fail(PTX_ERR_INVALID, "%s: misaligned output", who);
    }
    const int tiles_x = cdiv(desc->W, kBlurTile), tiles_y = cdiv(desc->H, kBlurTile);
    const dim3 grid((unsigned)((int64_t)tiles_x * tiles_y), (unsigned)desc->T, (unsigned)desc->N);
    const size_t lds = (size_t)blur_lds_bytes(desc->kx, desc->ky);
    const hipStream_t st = (hipStream_t)stream;
    if (desc->out_mode == PTX_RESIZE_OUT_U8)
        hipLaunchKernelGGL(blur_frames_kernel<PTX_RESIZE_OUT_U8>, grid, dim3(256), lds, st, frames, apply, wx, wy, y, desc->T, desc->H,
                           desc->W, desc->kx, desc->ky, tiles_x, nd);
    else if (desc->out_mode == PTX_RESIZE_OUT_F32)
        hipLaunchKernelGGL(blur_frames_kernel<PTX_RESIZE_OUT_F32>, grid, dim3(256), lds, st, frames, apply, wx, wy, y, desc->T, desc->H,
                           desc->W, desc->kx, desc->ky, tiles_x, nd);
    else
        hipLaunchKernelGGL(blur_frames_kernel<PTX_RESIZE_OUT_BF16>, grid, dim3(256), lds, st, frames, apply, wx, wy, y, desc->T, desc->H,
                           desc->W, desc->kx, desc->ky, tiles_x, nd);
    return hip_check(hipGetLastError(), "gaussian_blur_frames launch");
}
