// Class activation maps of the global-average-pool + Linear heads and their overlay on decoded uint8 frames
// (include/ptx_amd_cam.h states the arithmetic; transforms.cam_quantize_numpy / cam_overlay_numpy are its numpy statements).
// Compiled as part of pack_layout.hip's translation unit, behind blur_frames.h.
//
// cam_scores_kernel runs over (16 positions, clip): the k classifier rows of the clip's class list are copied into LDS once
// (row pitch C rounded up to 4 floats, so a lane's 16-byte LDS read is aligned), then each of the four waves takes every fourth
// position of the workgroup's 16: a lane reads 16 bytes of the feature row (4 fp32 / 8 bf16 channels) per step, multiplies them
// into k accumulators, the wave sums across its lanes.  The feature map is read once; the channels behind the last full group of
// 4 / 8 are read one by one, so nothing at or behind channel C is touched.  fp32 rows that are not 16-byte aligned (ld % 4 != 0 or
// such a base) take the one-channel-per-lane loop throughout.
// cam_quantize_kernel is one workgroup per map: minimum and maximum over the scores that are not NaN, then the bytes.
// cam_overlay_kernel runs over (run of output rows, frame, (clip, class)), a run being about 4096 pixels and at most 64 rows.  A
// workgroup stages in LDS, once: the colour table (one packed word per level), the row-table entries of its rows, the frame's map
// (h x w bytes) and the horizontal pass (W bytes per row) of the map rows its entries read.  After that it touches global memory
// for the frame and the output alone: a work item owns four neighbouring pixels -- the vertical pass from LDS, the colour, the blend
// with 12 frame bytes, 12 output bytes, three aligned dwords each way where the frame's, the output's and the run's first byte
// allow it (uniform over the workgroup), single bytes otherwise (rows of 159 bytes).
// Offsets inside a clip / frame are 32-bit, clip and frame bases 64-bit.
#pragma once
#include "blur_frames.h"
#include "../../include/ptx_amd_cam.h"

namespace ptx {

constexpr int kCamRows = 16;                           // positions per workgroup of the scores kernel
constexpr int kCamPix = 4;                             // pixels per work item of the overlay
constexpr int kCamChunk = 4096;                        // pixels per workgroup of the overlay, about
constexpr int kCamMaxRows = 64;                        // output rows per workgroup of the overlay, at most
constexpr int kCamHalf = 1 << 21, kCamShift = 22;      // the resize tables' fixed point

__device__ __forceinline__ float cam_bf16_lo(unsigned u) { return __uint_as_float(u << 16); }
__device__ __forceinline__ float cam_bf16_hi(unsigned u) { return __uint_as_float(u & 0xffff0000u); }

template <bool BF16, int KMAX>
__global__ void __launch_bounds__(256) cam_scores_kernel(const void* __restrict__ xv, const float* __restrict__ w,
                                                         const float* __restrict__ b, const int* __restrict__ cls,
                                                         float* __restrict__ y, int S, int C, int ld, int k, int classes, int vec) {
    extern __shared__ float cam_w[];                   // [k][Cp]
    __shared__ int s_cls[PTX_CAM_MAX_CLASSES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = blockIdx.y, s0 = blockIdx.x * kCamRows;
    const int Cp = (C + 3) & ~3;
    if (tid < k) s_cls[tid] = min(max(cls[(size_t)n * k + tid], 0), classes - 1);
    __syncthreads();
    for (int i = tid; i < k * C; i += 256) {
        const int j = i / C, c = i - j * C;
        cam_w[j * Cp + c] = w[(size_t)s_cls[j] * C + c];
    }
    __syncthreads();
    const size_t clip = (size_t)n * S * ld;
    const int s_end = min(s0 + kCamRows, S);
    for (int s = s0 + wave; s < s_end; s += 4) {
        float acc[KMAX];
#pragma unroll
        for (int j = 0; j < KMAX; ++j) acc[j] = 0.f;
        int tail = 0;                                  // first channel of the one-by-one loop
        if (BF16) {
            const unsigned short* row = static_cast<const unsigned short*>(xv) + clip + (size_t)s * ld;
            for (int c = lane * 8; c + 8 <= C; c += 512) {
                const uint4 u = *reinterpret_cast<const uint4*>(row + c);
                const float xs[8] = {cam_bf16_lo(u.x), cam_bf16_hi(u.x), cam_bf16_lo(u.y), cam_bf16_hi(u.y),
                                     cam_bf16_lo(u.z), cam_bf16_hi(u.z), cam_bf16_lo(u.w), cam_bf16_hi(u.w)};
#pragma unroll
                for (int j = 0; j < KMAX; ++j) {
                    if (j < k) {
                        const float4 w0 = *reinterpret_cast<const float4*>(cam_w + j * Cp + c);
                        const float4 w1 = *reinterpret_cast<const float4*>(cam_w + j * Cp + c + 4);
                        acc[j] += xs[0] * w0.x + xs[1] * w0.y + xs[2] * w0.z + xs[3] * w0.w + xs[4] * w1.x + xs[5] * w1.y +
                                  xs[6] * w1.z + xs[7] * w1.w;
                    }
                }
            }
            tail = C & ~7;
            for (int c = tail + lane; c < C; c += 64) {
                const float xs = cam_bf16_lo(row[c]);
#pragma unroll
                for (int j = 0; j < KMAX; ++j)
                    if (j < k) acc[j] += xs * cam_w[j * Cp + c];
            }
        } else {
            const float* row = static_cast<const float*>(xv) + clip + (size_t)s * ld;
            if (vec) {
                for (int c = lane * 4; c + 4 <= C; c += 256) {
                    const float4 xs = *reinterpret_cast<const float4*>(row + c);
#pragma unroll
                    for (int j = 0; j < KMAX; ++j) {
                        if (j < k) {
                            const float4 wv = *reinterpret_cast<const float4*>(cam_w + j * Cp + c);
                            acc[j] += xs.x * wv.x + xs.y * wv.y + xs.z * wv.z + xs.w * wv.w;
                        }
                    }
                }
                tail = C & ~3;
            }
            for (int c = tail + lane; c < C; c += 64) {
                const float xs = row[c];
#pragma unroll
                for (int j = 0; j < KMAX; ++j)
                    if (j < k) acc[j] += xs * cam_w[j * Cp + c];
            }
        }
        float mine = 0.f;
#pragma unroll
        for (int j = 0; j < KMAX; ++j) {
            float v = acc[j];
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
            if (lane == j) mine = v;
        }
        if (lane < k) y[((size_t)n * k + lane) * S + s] = (b ? b[s_cls[lane]] : 0.f) + mine;
    }
}

__global__ void __launch_bounds__(256) cam_quantize_kernel(const float* __restrict__ scores, unsigned char* __restrict__ q, long long S) {
#pragma clang fp contract(off)
    __shared__ float s_mn[4], s_mx[4];
    const int tid = threadIdx.x;
    const float* row = scores + (size_t)blockIdx.x * S;
    unsigned char* out = q + (size_t)blockIdx.x * S;
    float mn = INFINITY, mx = -INFINITY;
    for (long long i = tid; i < S; i += 256) {
        const float v = row[i];
        if (v == v) {                                  // a NaN takes no part
            mn = v < mn ? v : mn;
            mx = v > mx ? v : mx;
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float a = __shfl_xor(mn, off), c = __shfl_xor(mx, off);
        mn = a < mn ? a : mn;
        mx = c > mx ? c : mx;
    }
    if ((tid & 63) == 0) s_mn[tid >> 6] = mn, s_mx[tid >> 6] = mx;
    __syncthreads();
    mn = fminf(fminf(s_mn[0], s_mn[1]), fminf(s_mn[2], s_mn[3]));      // none of the eight is a NaN
    mx = fmaxf(fmaxf(s_mx[0], s_mx[1]), fmaxf(s_mx[2], s_mx[3]));
    const bool flat = !(mx > mn);                      // equal, or no score at all
    const float d = mx - mn;
    for (long long i = tid; i < S; i += 256) {
        const float t = (row[i] - mn) / d;             // IEEE division (the compiler's default for fp32)
        const float v = 255.0f * t;
        out[i] = flat ? 0 : (v >= 255.0f ? 255 : (v > 0.f ? (unsigned char)(int)v : 0));
    }
}

struct __attribute__((packed, aligned(4))) CamWords {
    unsigned a, b, c;
};

__device__ __forceinline__ int cam_clip8(int v) { return min(max(v, 0), 255); }

// Image.blend(frame, heat, alpha) on one channel: the product and the sum are two roundings (color_jitter.h's blend)
__device__ __forceinline__ int cam_blend(int f, int heat, float alpha) {
#pragma clang fp contract(off)
    const float scaled = alpha * (float)(heat - f);
    const float t = (float)f + scaled;
    return cam_clip8((int)t);                          // |t| < 2^9: 0 for t <= 0 (truncation towards zero), 255 for t >= 255
}

// rows of the output a workgroup owns: about kCamChunk pixels, at most kCamMaxRows (their row tables live in LDS)
__host__ __device__ __forceinline__ int cam_rows_per_wg(int W) { return min(kCamMaxRows, max(1, kCamChunk / W)); }

__host__ __device__ __forceinline__ size_t cam_overlay_lds(int R, int taps_h, int h, int w, int W) {
    return 1024 + (size_t)R * (2 + taps_h) * 4 + (((size_t)h * w + 3) & ~(size_t)3) + (size_t)h * W;
}

template <int MODE>
__global__ void __launch_bounds__(256) cam_overlay_kernel(const unsigned char* __restrict__ q, const unsigned char* __restrict__ frames,
                                                          const unsigned char* __restrict__ lut, const int* __restrict__ row_lo,
                                                          const int* __restrict__ row_n, const int* __restrict__ row_k,
                                                          const int* __restrict__ col_lo, const int* __restrict__ col_n,
                                                          const int* __restrict__ col_k, const int* __restrict__ step,
                                                          unsigned char* __restrict__ y, ptx_cam_overlay_desc d, int R) {
    extern __shared__ unsigned cam_lds[];              // lut [256] packed | row_lo [R] | row_n [R] | row_k [R][taps_h] | map [h][w] | mid [h][W]
    __shared__ int s_r0, s_r1;                         // the map rows this workgroup's output rows read
    const int tid = threadIdx.x;
    const int t = blockIdx.y, nj = blockIdx.z, n = nj / d.k;
    const int h = d.h, w = d.w, H = d.H, W = d.W, taps_h = d.taps_h;
    unsigned* s_lut = cam_lds;
    int* s_rlo = reinterpret_cast<int*>(s_lut + 256);
    int* s_rn = s_rlo + R;
    int* s_rk = s_rn + R;
    unsigned char* s_map = reinterpret_cast<unsigned char*>(s_rk + R * taps_h);
    unsigned char* s_mid = s_map + ((h * w + 3) & ~3);   // on a 4-byte boundary
    const int Y0 = blockIdx.x * R, rows = min(R, H - Y0);
    const int tm = min(max(step[t], 0), d.Tm - 1);
    const unsigned char* m = q + ((size_t)nj * d.Tm + tm) * ((size_t)h * w);
    if (tid == 0) s_r0 = h, s_r1 = 0;
    s_lut[tid] = (unsigned)lut[3 * tid] | ((unsigned)lut[3 * tid + 1] << 8) | ((unsigned)lut[3 * tid + 2] << 16);   // 256 threads
    for (int i = tid; i < h * w; i += 256) s_map[i] = m[i];
    __syncthreads();
    for (int r = tid; r < rows; r += 256) {
        const int lo = min(max(row_lo[Y0 + r], 0), h - 1), cnt = min(max(row_n[Y0 + r], 0), taps_h);
        s_rlo[r] = lo, s_rn[r] = cnt;
        atomicMin(&s_r0, lo);
        atomicMax(&s_r1, min(lo + max(cnt, 1), h));
    }
    for (int i = tid; i < rows * taps_h; i += 256) s_rk[i] = row_k[(size_t)Y0 * taps_h + i];
    __syncthreads();
    // horizontal pass of map rows [r0, r1): one output column per work item, its entry read once
    const int r0 = s_r0, r1 = s_r1;
    for (int X = tid; X < W; X += 256) {
        const int lo = min(max(col_lo[X], 0), w - 1), cnt = min(max(col_n[X], 0), d.taps_w);
        const int* kk = col_k + (size_t)X * d.taps_w;
        if (cnt <= 4) {                                // up-sampling: the entry fits registers (an absent tap is 0 * a byte)
            int k4[4], x4[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) k4[i] = i < cnt ? kk[i] : 0, x4[i] = min(lo + i, w - 1);
            for (int yy = r0; yy < r1; ++yy) {
                const unsigned char* mr = s_map + yy * w;
                const int acc = kCamHalf + k4[0] * (int)mr[x4[0]] + k4[1] * (int)mr[x4[1]] + k4[2] * (int)mr[x4[2]] + k4[3] * (int)mr[x4[3]];
                s_mid[yy * W + X] = (unsigned char)cam_clip8(acc >> kCamShift);
            }
        } else {
            for (int yy = r0; yy < r1; ++yy) {
                int acc = kCamHalf;
                for (int i = 0; i < cnt; ++i) acc += kk[i] * (int)s_map[yy * w + min(lo + i, w - 1)];
                s_mid[yy * W + X] = (unsigned char)cam_clip8(acc >> kCamShift);
            }
        }
    }
    __syncthreads();
    const int P = H * W;
    constexpr int kBytes = MODE == PTX_CAM_OUT_MAP ? 1 : 3;
    const size_t out_frame = ((size_t)nj * d.T + t) * (size_t)P * kBytes;
    const size_t in_frame = ((size_t)n * d.T + t) * (size_t)P * 3;
    unsigned char* yo = y + out_frame;
    const unsigned char* fi = MODE == PTX_CAM_OUT_OVERLAY ? frames + in_frame : nullptr;
    const int p_begin = Y0 * W, p_end = (Y0 + rows) * W;
    // uniform over the workgroup: every work item's first byte is 12 (map mode: 4) bytes past an aligned one
    const bool words = ((uintptr_t)yo & 3) == 0 && (MODE != PTX_CAM_OUT_OVERLAY || ((uintptr_t)fi & 3) == 0) && (p_begin & 3) == 0;
    // the frame words of the NEXT round are requested before this round's arithmetic: two loads in flight per work item
    CamWords pre = {0, 0, 0};
    const int p_first = p_begin + tid * kCamPix;
    if (MODE == PTX_CAM_OUT_OVERLAY && words && p_first + kCamPix <= p_end) pre = *reinterpret_cast<const CamWords*>(fi + (size_t)p_first * 3);
    const int step_y = (256 * kCamPix) / W, step_x = (256 * kCamPix) - step_y * W;     // one round further, as rows and columns
    int Yc = p_first / W, Xc = p_first - Yc * W;
    for (int p0 = p_first; p0 < p_end; p0 += 256 * kCamPix) {
        const int cnt_px = min(kCamPix, p_end - p0);
        const CamWords in = pre;
        const int p_next = p0 + 256 * kCamPix;
        if (MODE == PTX_CAM_OUT_OVERLAY && words && p_next + kCamPix <= p_end) pre = *reinterpret_cast<const CamWords*>(fi + (size_t)p_next * 3);
        int Y = Yc, X = Xc;
        Xc += step_x, Yc += step_y;
        if (Xc >= W) Xc -= W, ++Yc;
        int v[kCamPix];
        if (cnt_px == kCamPix && X + kCamPix <= W) {   // four pixels of one row: one entry, four neighbouring bytes per tap
            const int r = Y - Y0, rlo = s_rlo[r], rn = s_rn[r];
            int acc[kCamPix];
#pragma unroll
            for (int px = 0; px < kCamPix; ++px) acc[px] = kCamHalf;
            if ((W & 3) == 0) {                        // X is a multiple of 4 too: the four bytes of a tap are one aligned word
                for (int i = 0; i < rn; ++i) {
                    const int kk = s_rk[r * taps_h + i];
                    const unsigned mw = *reinterpret_cast<const unsigned*>(s_mid + min(rlo + i, h - 1) * W + X);
#pragma unroll
                    for (int px = 0; px < kCamPix; ++px) acc[px] += kk * (int)((mw >> (8 * px)) & 255u);
                }
            } else {
                for (int i = 0; i < rn; ++i) {
                    const int kk = s_rk[r * taps_h + i];
                    const unsigned char* mp = s_mid + min(rlo + i, h - 1) * W + X;
#pragma unroll
                    for (int px = 0; px < kCamPix; ++px) acc[px] += kk * (int)mp[px];
                }
            }
#pragma unroll
            for (int px = 0; px < kCamPix; ++px) v[px] = cam_clip8(acc[px] >> kCamShift);
        } else {
#pragma unroll
            for (int px = 0; px < kCamPix; ++px) {
                v[px] = 0;
                if (px < cnt_px) {
                    if (X == W) X = 0, ++Y;
                    const int r = Y - Y0, rlo = s_rlo[r], rn = s_rn[r];
                    int acc = kCamHalf;
                    for (int i = 0; i < rn; ++i) acc += s_rk[r * taps_h + i] * (int)s_mid[min(rlo + i, h - 1) * W + X];
                    v[px] = cam_clip8(acc >> kCamShift);
                    ++X;
                }
            }
        }
        if (MODE == PTX_CAM_OUT_MAP) {
            if (words && cnt_px == kCamPix) {
                *reinterpret_cast<unsigned*>(yo + p0) = (unsigned)v[0] | ((unsigned)v[1] << 8) | ((unsigned)v[2] << 16) | ((unsigned)v[3] << 24);
            } else {
#pragma unroll
                for (int px = 0; px < kCamPix; ++px)
                    if (px < cnt_px) yo[p0 + px] = (unsigned char)v[px];
            }
            continue;
        }
        unsigned char fb[3 * kCamPix], ob[3 * kCamPix];
        const bool fast = words && cnt_px == kCamPix;
        if (MODE == PTX_CAM_OUT_OVERLAY) {
            if (fast) {
                __builtin_memcpy(fb, &in, 12);
            } else {
#pragma unroll
                for (int i = 0; i < 3 * kCamPix; ++i) fb[i] = i < 3 * cnt_px ? fi[(size_t)p0 * 3 + i] : 0;
            }
        }
#pragma unroll
        for (int px = 0; px < kCamPix; ++px) {
            const unsigned colour = s_lut[v[px]];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const int heat = (int)((colour >> (8 * c)) & 255u);
                ob[3 * px + c] = (unsigned char)(MODE == PTX_CAM_OUT_OVERLAY ? cam_blend(fb[3 * px + c], heat, d.alpha) : heat);
            }
        }
        if (fast) {
            CamWords o;
            __builtin_memcpy(&o, ob, 12);
            *reinterpret_cast<CamWords*>(yo + (size_t)p0 * 3) = o;
        } else {
#pragma unroll
            for (int i = 0; i < 3 * kCamPix; ++i)
                if (i < 3 * cnt_px) yo[(size_t)p0 * 3 + i] = ob[i];
        }
    }
}

static int cam_scores_check(int32_t N, int64_t S, int32_t C, int32_t ld, int32_t k, int32_t classes, int32_t x_bf16, const char* who) {
    if (N <= 0 || S <= 0 || C <= 0 || classes <= 0)
        return fail(PTX_ERR_INVALID, "%s: non-positive extent (N=%d S=%lld C=%d classes=%d)", who, N, (long long)S, C, classes);
    if (ld < C) return fail(PTX_ERR_INVALID, "%s: ld=%d is below C=%d", who, ld, C);
    if (x_bf16 && (ld & 7)) return fail(PTX_ERR_INVALID, "%s: bf16 rows need ld %% 8 == 0 (ld=%d)", who, ld);
    if (k < 1 || k > PTX_CAM_MAX_CLASSES)
        return fail(PTX_ERR_INVALID, "%s: k=%d classes per clip, a launch takes 1..PTX_CAM_MAX_CLASSES = %d", who, k, PTX_CAM_MAX_CLASSES);
    if ((int64_t)k * ((C + 3) & ~3) * 4 > PTX_CAM_MAX_LDS_BYTES)
        return fail(PTX_ERR_UNSUPPORTED, "%s: %d classifier rows of %d channels exceed the %d bytes of LDS a launch holds (fewer classes "
                    "per launch)", who, k, C, PTX_CAM_MAX_LDS_BYTES);
    if (S * ld > INT32_MAX) return fail(PTX_ERR_UNSUPPORTED, "%s: a clip of %lld x %d elements exceeds 32-bit indexing", who, (long long)S, ld);
    if (N > 65535) return fail(PTX_ERR_UNSUPPORTED, "%s: %d clips exceed the grid (N <= 65535)", who, N);
    return PTX_OK;
}

static int cam_overlay_check(const ptx_cam_overlay_desc* d, const char* who) {
    if (!d) return fail(PTX_ERR_INVALID, "%s: null descriptor", who);
    if (d->N <= 0 || d->k <= 0 || d->Tm <= 0 || d->h <= 0 || d->w <= 0 || d->T <= 0 || d->H <= 0 || d->W <= 0)
        return fail(PTX_ERR_INVALID, "%s: non-positive extent (N=%d k=%d Tm=%d h=%d w=%d T=%d H=%d W=%d)", who, d->N, d->k, d->Tm, d->h,
                    d->w, d->T, d->H, d->W);
    if (d->taps_h < 1 || d->taps_w < 1) return fail(PTX_ERR_INVALID, "%s: tap counts must be positive (taps_h=%d taps_w=%d)", who, d->taps_h, d->taps_w);
    if (d->taps_h > PTX_RESIZE_MAX_TAPS || d->taps_w > PTX_RESIZE_MAX_TAPS)
        return fail(PTX_ERR_UNSUPPORTED, "%s: down-sampling a %dx%d map to %dx%d needs %d x %d taps, the cap is PTX_RESIZE_MAX_TAPS = %d", who,
                    d->h, d->w, d->H, d->W, d->taps_h, d->taps_w, PTX_RESIZE_MAX_TAPS);
    if (d->mode != PTX_CAM_OUT_OVERLAY && d->mode != PTX_CAM_OUT_HEAT && d->mode != PTX_CAM_OUT_MAP)
        return fail(PTX_ERR_INVALID, "%s: mode=%d is not a PTX_CAM_OUT_* value", who, d->mode);
    if (d->mode == PTX_CAM_OUT_OVERLAY && !(d->alpha >= 0.f && d->alpha <= 1.f))
        return fail(PTX_ERR_INVALID, "%s: alpha=%g must lie in [0, 1]", who, (double)d->alpha);
    if ((int64_t)d->h * ((int64_t)d->w + d->W) > PTX_CAM_MAX_MAP_BYTES)
        return fail(PTX_ERR_UNSUPPORTED, "%s: staging a %dx%d map and its %dx%d horizontal pass exceeds PTX_CAM_MAX_MAP_BYTES = %d", who,
                    d->h, d->w, d->h, d->W, PTX_CAM_MAX_MAP_BYTES);
    const int64_t P = (int64_t)d->H * d->W;
    if (P * 3 > INT32_MAX) return fail(PTX_ERR_UNSUPPORTED, "%s: a frame of %dx%d pixels exceeds 32-bit indexing", who, d->H, d->W);
    const int64_t maps = (int64_t)d->N * d->k;
    if (maps > 65535 || d->T > 65535) return fail(PTX_ERR_UNSUPPORTED, "%s: %lld maps x %d frames exceed the grid (N * k, T <= 65535)", who, (long long)maps, d->T);
    const int64_t bytes = P * (d->mode == PTX_CAM_OUT_MAP ? 1 : 3);
    if ((double)maps * (double)d->T * (double)bytes > (double)INT32_MAX)
        return fail(PTX_ERR_UNSUPPORTED, "%s: an output of %lld x %d frames of %lld bytes exceeds the 2 GiB per-launch limit (launch ranges "
                    "of (n, j))", who, (long long)maps, d->T, (long long)bytes);
    return PTX_OK;
}

static int cam_coeff_check(const int32_t* k, int entries, int taps, const char* what, const char* who) {
    for (int e = 0; e < entries; ++e) {
        int64_t total = 0;
        for (int i = 0; i < taps; ++i) {
            const int64_t a = k[(size_t)e * taps + i] < 0 ? -(int64_t)k[(size_t)e * taps + i] : (int64_t)k[(size_t)e * taps + i];
            if (a >= (1 << 23)) return fail(PTX_ERR_INVALID, "%s: %s entry %d: a coefficient of magnitude %lld is not below 2^23", who, what, e, (long long)a);
            total += a;
        }
        if (255 * total + kCamHalf >= (1LL << 31))
            return fail(PTX_ERR_INVALID, "%s: %s entry %d: sum|k| = %lld overflows the 32-bit accumulator", who, what, e, (long long)total);
    }
    return PTX_OK;
}

}  // namespace ptx

using namespace ptx;

extern "C" int ptx_cam_scores_supported(int32_t N, int64_t S, int32_t C, int32_t ld, int32_t k, int32_t classes, int32_t x_bf16) {
    return cam_scores_check(N, S, C, ld, k, classes, x_bf16, "ptx_cam_scores_supported") == PTX_OK;
}

template <bool BF16>
static void cam_scores_launch(dim3 grid, size_t lds, hipStream_t st, const void* x, const float* w, const float* b, const int32_t* cls,
                              float* y, int S, int C, int ld, int k, int classes, int vec) {
    if (k == 1)
        hipLaunchKernelGGL((cam_scores_kernel<BF16, 1>), grid, dim3(256), lds, st, x, w, b, cls, y, S, C, ld, k, classes, vec);
    else if (k <= 4)
        hipLaunchKernelGGL((cam_scores_kernel<BF16, 4>), grid, dim3(256), lds, st, x, w, b, cls, y, S, C, ld, k, classes, vec);
    else
        hipLaunchKernelGGL((cam_scores_kernel<BF16, PTX_CAM_MAX_CLASSES>), grid, dim3(256), lds, st, x, w, b, cls, y, S, C, ld, k, classes, vec);
}

extern "C" int ptx_cam_scores(const void* x, int32_t x_bf16, const float* w, const float* b, const int32_t* cls, float* y, int32_t N,
                              int64_t S, int32_t C, int32_t ld, int32_t k, int32_t classes, ptx_stream_t stream) {
    const char* who = "ptx_cam_scores";
    int s = cam_scores_check(N, S, C, ld, k, classes, x_bf16, who);
    if (s) return s;
    if (!x || !w || !cls || !y) return fail(PTX_ERR_INVALID, "%s: null pointer", who);
    if (((uintptr_t)w | (uintptr_t)b | (uintptr_t)cls | (uintptr_t)y) & 3) return fail(PTX_ERR_INVALID, "%s: misaligned weights, classes or output", who);
    if ((uintptr_t)x & (x_bf16 ? 15 : 3)) return fail(PTX_ERR_INVALID, "%s: misaligned feature map", who);
    const int vec = !x_bf16 && (ld & 3) == 0 && ((uintptr_t)x & 15) == 0;
    const dim3 grid((unsigned)cdiv64(S, kCamRows), (unsigned)N);
    const size_t lds = (size_t)k * ((C + 3) & ~3) * 4;
    if (x_bf16)
        cam_scores_launch<true>(grid, lds, (hipStream_t)stream, x, w, b, cls, y, (int)S, C, ld, k, classes, vec);
    else
        cam_scores_launch<false>(grid, lds, (hipStream_t)stream, x, w, b, cls, y, (int)S, C, ld, k, classes, vec);
    return hip_check(hipGetLastError(), "cam_scores launch");
}

extern "C" int ptx_cam_quantize(const float* scores, uint8_t* q, int64_t maps, int64_t S, ptx_stream_t stream) {
    const char* who = "ptx_cam_quantize";
    if (!scores || !q) return fail(PTX_ERR_INVALID, "%s: null pointer", who);
    if (maps <= 0 || S <= 0) return fail(PTX_ERR_INVALID, "%s: non-positive extent (maps=%lld S=%lld)", who, (long long)maps, (long long)S);
    if ((uintptr_t)scores & 3) return fail(PTX_ERR_INVALID, "%s: misaligned scores", who);
    if (maps > INT32_MAX) return fail(PTX_ERR_UNSUPPORTED, "%s: %lld maps exceed the grid", who, (long long)maps);
    hipLaunchKernelGGL(cam_quantize_kernel, dim3((unsigned)maps), dim3(256), 0, (hipStream_t)stream, scores, q, (long long)S);
    return hip_check(hipGetLastError(), "cam_quantize launch");
}

extern "C" int ptx_cam_overlay_supported(const ptx_cam_overlay_desc* desc, const int32_t* row_k, const int32_t* col_k) {
    const char* who = "ptx_cam_overlay_supported";
    if (cam_overlay_check(desc, who)) return 0;
    if (row_k && cam_coeff_check(row_k, desc->H, desc->taps_h, "row", who)) return 0;
    if (col_k && cam_coeff_check(col_k, desc->W, desc->taps_w, "column", who)) return 0;
    return 1;
}

extern "C" int ptx_cam_overlay(const ptx_cam_overlay_desc* desc, const uint8_t* q, const uint8_t* frames, const uint8_t* lut,
                               const int32_t* row_lo, const int32_t* row_n, const int32_t* row_k, const int32_t* col_lo,
                               const int32_t* col_n, const int32_t* col_k, const int32_t* step, uint8_t* y, ptx_stream_t stream) {
    const char* who = "ptx_cam_overlay";
    int s = cam_overlay_check(desc, who);
    if (s) return s;
    if (!q || !lut || !row_lo || !row_n || !row_k || !col_lo || !col_n || !col_k || !step || !y) return fail(PTX_ERR_INVALID, "%s: null pointer", who);
    if (desc->mode == PTX_CAM_OUT_OVERLAY && !frames) return fail(PTX_ERR_INVALID, "%s: the overlay mode needs frames", who);
    if (((uintptr_t)row_lo | (uintptr_t)row_n | (uintptr_t)row_k | (uintptr_t)col_lo | (uintptr_t)col_n | (uintptr_t)col_k | (uintptr_t)step) & 3)
        return fail(PTX_ERR_INVALID, "%s: misaligned tables", who);
    if ((const void*)y == (const void*)frames) return fail(PTX_ERR_INVALID, "%s: y must not be frames (k outputs read one frame)", who);
    const int R = cam_rows_per_wg(desc->W);
    const dim3 grid((unsigned)cdiv(desc->H, R), (unsigned)desc->T, (unsigned)(desc->N * desc->k));
    const size_t lds = cam_overlay_lds(R, desc->taps_h, desc->h, desc->w, desc->W);
    const hipStream_t st = (hipStream_t)stream;
    if (desc->mode == PTX_CAM_OUT_OVERLAY)
        hipLaunchKernelGGL(cam_overlay_kernel<PTX_CAM_OUT_OVERLAY>, grid, dim3(256), lds, st, q, frames, lut, row_lo, row_n, row_k, col_lo,
                           col_n, col_k, step, y, *desc, R);
    else if (desc->mode == PTX_CAM_OUT_HEAT)
        hipLaunchKernelGGL(cam_overlay_kernel<PTX_CAM_OUT_HEAT>, grid, dim3(256), lds, st, q, frames, lut, row_lo, row_n, row_k, col_lo,
                           col_n, col_k, step, y, *desc, R);
    else
        hipLaunchKernelGGL(cam_overlay_kernel<PTX_CAM_OUT_MAP>, grid, dim3(256), lds, st, q, frames, lut, row_lo, row_n, row_k, col_lo,
                           col_n, col_k, step, y, *desc, R);
    return hip_check(hipGetLastError(), "cam_overlay launch");
}
