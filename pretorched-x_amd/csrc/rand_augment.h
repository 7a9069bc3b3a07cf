// Per-clip RandAugment of decoded uint8 frames [N][T][H][W][3], equal to torchvision's RandAugment on its PIL-image code path
// (nearest interpolation) bit for bit (include/ptx_amd_randaug.h states the arithmetic; transforms.rand_augment_numpy is its
// numpy statement).  Compiled as part of pack_layout.hip's translation unit, behind color_jitter.h, whose device functions
// (luma, blend, mean) the enhancement ops share.
//
// One POSITION of every clip's op list per call, two launches.  randaug_stats_kernel (only when some clip's op at the position
// is contrast, autocontrast or equalize) counts every frame's three 256-bin histograms in LDS with integer atomics and sums its
// luma, then flushes the non-empty bins and the sum with one integer atomic each: integer sums do not depend on the order, so
// the result is deterministic.  randaug_apply_kernel runs the op per pixel.  Both run over (tile, t, n): a workgroup owns
// kRaTile consecutive pixels of one frame, so the op code is uniform over a workgroup, every branch on it is a scalar branch,
// and the workgroups of a clip that needs no statistics leave the statistics kernel at once.  A clip whose op needs a LUT
// builds it in LDS from the frame's histogram (256 threads: one entry per thread and channel).
//
// Frames are read and written byte by byte (any alignment; a lane's three bytes follow its neighbour's), planes are written one
// element per lane.  The floating-point pieces (blend, mean, the autocontrast LUT) switch contraction off, as color_jitter.h's.
#pragma once
#include "color_jitter.h"
#include "../../include/ptx_amd_randaug.h"
#include <cstring>

namespace ptx {

constexpr int kRaRow = PTX_RANDAUG_ROW;
constexpr int kRaTile = 4096;                          // pixels per workgroup (16 per lane)
constexpr int kRaStatsWords = PTX_RANDAUG_STATS_WORDS;

__device__ __forceinline__ bool ra_needs_stats(int op) {
    return op == PTX_RANDAUG_CONTRAST || op == PTX_RANDAUG_AUTOCONTRAST || op == PTX_RANDAUG_EQUALIZE;
}

// ImageOps.autocontrast's LUT entry i of a channel whose lowest / highest non-empty bins are lo / hi
__device__ __forceinline__ int ra_autocontrast(int i, int lo, int hi) {
#pragma clang fp contract(off)
    if (hi <= lo) return i;
    const double scale = 255.0 / (double)(hi - lo);
    const double offset = -(double)lo * scale;
    const double v = (double)i * scale + offset;
    return clip8((int)v);                              // trunc, then the clamp
}

// ImageOps.equalize's LUT entry i of a channel with histogram h (LDS), `nz` non-empty bins, the highest of them `last`
__device__ __forceinline__ int ra_equalize(int i, const unsigned* h, int nz, int last, int P) {
    if (nz <= 1) return i;
    const unsigned step = ((unsigned)P - h[last]) / 255u;
    if (step == 0) return i;
    unsigned n = step / 2;
    for (int j = 0; j < i; ++j) n += h[j];             // below P + step / 2 < 2^31
    return (int)min(n / step, 255u);
}

__global__ void __launch_bounds__(256) randaug_stats_kernel(const unsigned char* __restrict__ frames, const int* __restrict__ rows,
                                                            unsigned* __restrict__ stats, int T, int P, int row_pitch, int position) {
    __shared__ unsigned bins[768];
    __shared__ unsigned part[4];
    const int tile = blockIdx.x, t = blockIdx.y, n = blockIdx.z;
    const int op = rows[(size_t)n * row_pitch + position * kRaRow];
    if (!ra_needs_stats(op)) return;                   // uniform: this clip's op needs no statistics
    const bool hist = op != PTX_RANDAUG_CONTRAST;      // contrast takes the luma sum alone
    const size_t frame = (size_t)n * T + t;
    const unsigned char* fin = frames + frame * P * 3;
    for (int i = threadIdx.x; i < 768; i += 256) bins[i] = 0;
    __syncthreads();
    const int p0 = tile * kRaTile, p1 = min(p0 + kRaTile, P);
    unsigned acc = 0;                                  // at most 16 pixels x 255
    for (int p = p0 + threadIdx.x; p < p1; p += 256) {
        const int r = fin[3 * (size_t)p], g = fin[3 * (size_t)p + 1], b = fin[3 * (size_t)p + 2];
        if (hist) {
            atomicAdd(&bins[r], 1u);
            atomicAdd(&bins[256 + g], 1u);
            atomicAdd(&bins[512 + b], 1u);
        }
        acc += cj_luma(r, g, b);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
    __syncthreads();
    unsigned* out = stats + frame * kRaStatsWords;
    if (hist)
        for (int i = threadIdx.x; i < 768; i += 256)
            if (bins[i]) atomicAdd(&out[i], bins[i]);
    if (threadIdx.x == 0)
        atomicAdd(reinterpret_cast<unsigned long long*>(out + 768), (unsigned long long)part[0] + part[1] + part[2] + part[3]);
}

template <int OUT>
__global__ void __launch_bounds__(256) randaug_apply_kernel(const unsigned char* __restrict__ frames, const int* __restrict__ rows,
                                                            const unsigned* __restrict__ stats, void* __restrict__ y, int T, int H, int W,
                                                            int row_pitch, int position, int fill_r, int fill_g, int fill_b,
                                                            ptx_norm_desc nd) {
    __shared__ unsigned sh_h[768];
    __shared__ unsigned char sh_lut[768];
    __shared__ int sh_lo[3], sh_hi[3], sh_nz[3];
    const int tile = blockIdx.x, t = blockIdx.y, n = blockIdx.z;
    const int* row = rows + (size_t)n * row_pitch + position * kRaRow;
    const int op = row[0];                             // uniform over the workgroup
    const int P = H * W;
    const size_t frame = (size_t)n * T + t;
    const unsigned char* fin = frames + frame * P * 3;
    const float f = __builtin_bit_cast(float, row[1]);
    const int a0 = row[1], a1 = row[2], a2 = row[3], a3 = row[4], a4 = row[5], a5 = row[6];
    const bool geometric = op >= PTX_RANDAUG_SHEAR_X && op <= PTX_RANDAUG_ROTATE;
    const bool lut = (op == PTX_RANDAUG_AUTOCONTRAST || op == PTX_RANDAUG_EQUALIZE) && stats;
    int mean = 0;
    if (op == PTX_RANDAUG_CONTRAST && stats)
        mean = cj_mean(*reinterpret_cast<const unsigned long long*>(stats + frame * kRaStatsWords + 768), P);
    if (lut) {                                         // uniform
        const unsigned* hs = stats + frame * kRaStatsWords;
        const int i = threadIdx.x;
        for (int k = i; k < 768; k += 256) sh_h[k] = hs[k];
        if (i < 3) sh_lo[i] = 256, sh_hi[i] = -1, sh_nz[i] = 0;
        __syncthreads();
#pragma unroll
        for (int ch = 0; ch < 3; ++ch)
            if (sh_h[ch * 256 + i]) {
                atomicMin(&sh_lo[ch], i);
                atomicMax(&sh_hi[ch], i);
                atomicAdd(&sh_nz[ch], 1);
            }
        __syncthreads();
#pragma unroll
        for (int ch = 0; ch < 3; ++ch)
            sh_lut[ch * 256 + i] = (unsigned char)(op == PTX_RANDAUG_AUTOCONTRAST ? ra_autocontrast(i, sh_lo[ch], sh_hi[ch])
                                                                                  : ra_equalize(i, sh_h + ch * 256, sh_nz[ch], sh_hi[ch], P));
        __syncthreads();
    }
    // uint8 out: pixel p of the frame is byte (frame P + p) 3 of y.  planes out: element (plane P + p), plane = (3 n + ch) T + t
    const size_t plane0 = (size_t)n * 3 * T + t;
    const int p0 = tile * kRaTile, p1 = min(p0 + kRaTile, P);
#pragma unroll 1
    for (int p = p0 + threadIdx.x; p < p1; p += 256) {
        int r, g, b;
        if (geometric) {
            const int yy = p / W, xx = p - yy * W;
            // the walk's running sums are C ints that wrap; the sum of the products modulo 2^32 is the same number
            const int xin = (int)((unsigned)a2 + (unsigned)a1 * (unsigned)yy + (unsigned)a0 * (unsigned)xx) >> 16;
            const int yin = (int)((unsigned)a5 + (unsigned)a4 * (unsigned)yy + (unsigned)a3 * (unsigned)xx) >> 16;
            if (xin >= 0 && xin < W && yin >= 0 && yin < H) {
                const unsigned char* q = fin + 3 * ((size_t)yin * W + xin);
                r = q[0], g = q[1], b = q[2];
            } else {
                r = fill_r, g = fill_g, b = fill_b;
            }
        } else {
            const unsigned char* q = fin + 3 * (size_t)p;
            r = q[0], g = q[1], b = q[2];
            if (op == PTX_RANDAUG_BRIGHTNESS) {
                r = cj_blend(0, r, f), g = cj_blend(0, g, f), b = cj_blend(0, b, f);
            } else if (op == PTX_RANDAUG_COLOR) {
                const int d = cj_luma(r, g, b);
                r = cj_blend(d, r, f), g = cj_blend(d, g, f), b = cj_blend(d, b, f);
            } else if (op == PTX_RANDAUG_CONTRAST) {
                r = cj_blend(mean, r, f), g = cj_blend(mean, g, f), b = cj_blend(mean, b, f);
            } else if (op == PTX_RANDAUG_SHARPNESS) {
                const int yy = p / W, xx = p - yy * W;
                int sr = r, sg = g, sb = b;
                if (H >= 3 && W >= 3 && xx > 0 && xx < W - 1 && yy > 0 && yy < H - 1) {
                    sr = 4 * r, sg = 4 * g, sb = 4 * b;
#pragma unroll
                    for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
                        for (int dx = -1; dx <= 1; ++dx) {
                            const unsigned char* s = fin + 3 * ((size_t)(yy + dy) * W + (xx + dx));
                            sr += s[0], sg += s[1], sb += s[2];
                        }
                    sr = (2 * sr + 13) / 26, sg = (2 * sg + 13) / 26, sb = (2 * sb + 13) / 26;
                }
                r = cj_blend(sr, r, f), g = cj_blend(sg, g, f), b = cj_blend(sb, b, f);
            } else if (op == PTX_RANDAUG_POSTERIZE) {
                r &= a0, g &= a0, b &= a0;
            } else if (op == PTX_RANDAUG_SOLARIZE) {
                r = (float)r < f ? r : 255 - r, g = (float)g < f ? g : 255 - g, b = (float)b < f ? b : 255 - b;
            } else if (lut) {
                r = sh_lut[r], g = sh_lut[256 + g], b = sh_lut[512 + b];
            }
        }
        if (OUT == PTX_RESIZE_OUT_U8) {
            unsigned char* o = static_cast<unsigned char*>(y) + (frame * P + p) * 3;
            o[0] = (unsigned char)r, o[1] = (unsigned char)g, o[2] = (unsigned char)b;
            continue;
        }
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const int cin = (nd.swap_rb && ch != 1) ? 2 - ch : ch;
            const float v = normalise_u8((unsigned char)(cin == 0 ? r : cin == 1 ? g : b), nd.mean[ch], nd.std[ch], nd.to_255);
            const size_t o = (plane0 + (size_t)ch * T) * P + p;
            if (OUT == PTX_RESIZE_OUT_F32)
                static_cast<float*>(y)[o] = v;
            else
                static_cast<unsigned short*>(y)[o] = __builtin_bit_cast(unsigned short, (__bf16)v);   // nearest even, as PTX_RESIZE_OUT_BF16
        }
    }
}

// Host-side checks shared by the three entry points (no device needed).
static int randaug_desc_check(const ptx_randaug_desc* d, const char* who) {
    if (!d) return fail(PTX_ERR_INVALID, "%s: null descriptor", who);
    if (d->N <= 0 || d->T <= 0 || d->H <= 0 || d->W <= 0)
        return fail(PTX_ERR_INVALID, "%s: non-positive extent (N=%d T=%d H=%d W=%d)", who, d->N, d->T, d->H, d->W);
    if (d->out_mode != PTX_RESIZE_OUT_U8 && d->out_mode != PTX_RESIZE_OUT_F32 && d->out_mode != PTX_RESIZE_OUT_BF16)
        return fail(PTX_ERR_INVALID, "%s: out_mode=%d is not a PTX_RESIZE_OUT_* value", who, d->out_mode);
    if (d->num_ops < 1 || d->num_ops > PTX_RANDAUG_MAX_OPS)
        return fail(PTX_ERR_INVALID, "%s: num_ops=%d must be 1..%d (PTX_RANDAUG_MAX_OPS)", who, d->num_ops, PTX_RANDAUG_MAX_OPS);
    if (d->position < 0 || d->position >= d->num_ops)
        return fail(PTX_ERR_INVALID, "%s: position=%d must be 0..%d", who, d->position, d->num_ops - 1);
    if ((unsigned)d->fill_r > 255u || (unsigned)d->fill_g > 255u || (unsigned)d->fill_b > 255u)
        return fail(PTX_ERR_INVALID, "%s: fill (%d, %d, %d) must be 0..255", who, d->fill_r, d->fill_g, d->fill_b);
    const int64_t P = (int64_t)d->H * d->W;
    if (P * 3 > INT32_MAX) return fail(PTX_ERR_UNSUPPORTED, "%s: a frame of %dx%d pixels exceeds 32-bit indexing", who, d->H, d->W);
    if (d->T > 65535 || d->N > 65535)
        return fail(PTX_ERR_UNSUPPORTED, "%s: %d x %d frames exceed the grid (N, T <= 65535)", who, d->N, d->T);
    return PTX_OK;
}

static dim3 randaug_grid(const ptx_randaug_desc* d) {
    return dim3((unsigned)cdiv64((int64_t)d->H * d->W, kRaTile), (unsigned)d->T, (unsigned)d->N);
}

}  // namespace ptx

using namespace ptx;

extern "C" int ptx_rand_augment_supported(const ptx_randaug_desc* desc, const int32_t* rows) {
    const char* who = "ptx_rand_augment_supported";
    if (randaug_desc_check(desc, who)) return 0;
    if (!rows) return fail(PTX_ERR_INVALID, "%s: null pointer", who), 0;
    bool stats = false;
    for (int n = 0; n < desc->N; ++n)
        for (int k = 0; k < desc->num_ops; ++k) {
            const int32_t* row = rows + ((size_t)n * desc->num_ops + k) * kRaRow;
            const int op = row[0];
            if (op < 0 || op >= PTX_RANDAUG_NUM_CODES)
                return fail(PTX_ERR_INVALID, "%s: clip %d position %d: op code %d out of range 0..%d", who, n, k, op, PTX_RANDAUG_NUM_CODES - 1), 0;
            float f;
            memcpy(&f, row + 1, sizeof f);
            if (op >= PTX_RANDAUG_SHEAR_X && op <= PTX_RANDAUG_ROTATE) {
                for (int c = 0; c < 4; ++c) {          // the frame's corners, as PIL checks them before it takes the fixed-point walk
                    const int64_t x = (c & 1) ? desc->W : 0, yv = (c & 2) ? desc->H : 0;
                    const int64_t xs = (int64_t)row[3] + (int64_t)row[1] * x + (int64_t)row[2] * yv;
                    const int64_t ys = (int64_t)row[6] + (int64_t)row[4] * x + (int64_t)row[5] * yv;
                    const int64_t lim = (int64_t)32768 << 16;
                    if (xs <= -lim || xs >= lim || ys <= -lim || ys >= lim)
                        return fail(PTX_ERR_UNSUPPORTED, "%s: clip %d position %d: the affine row leaves PIL's fixed-point range (a source "
                                    "coordinate of a %dx%d frame's corner beyond +-32768)", who, n, k, desc->H, desc->W), 0;
                }
            } else if (op >= PTX_RANDAUG_BRIGHTNESS && op <= PTX_RANDAUG_SHARPNESS) {
                if (!(f >= 0.f) || !(f <= 3.0e38f))
                    return fail(PTX_ERR_INVALID, "%s: clip %d position %d: factor %g must be finite and >= 0", who, n, k, (double)f), 0;
            } else if (op == PTX_RANDAUG_POSTERIZE) {
                if ((unsigned)row[1] > 255u)
                    return fail(PTX_ERR_INVALID, "%s: clip %d position %d: posterize mask %d must be 0..255", who, n, k, row[1]), 0;
            } else if (op == PTX_RANDAUG_SOLARIZE) {
                if (!(f >= -3.0e38f) || !(f <= 3.0e38f))
                    return fail(PTX_ERR_INVALID, "%s: clip %d position %d: solarize threshold %g must be finite", who, n, k, (double)f), 0;
            }
            if (k == desc->position)
                stats |= op == PTX_RANDAUG_CONTRAST || op == PTX_RANDAUG_AUTOCONTRAST || op == PTX_RANDAUG_EQUALIZE;
        }
    if (stats != (desc->stats != 0))
        return fail(PTX_ERR_INVALID, "%s: desc.stats=%d but %s op at position %d needs the statistics", who, desc->stats, stats ? "an" : "no",
                    desc->position), 0;
    return 1;
}

extern "C" int ptx_rand_augment_stats(const ptx_randaug_desc* desc, const uint8_t* frames, const int32_t* rows, uint32_t* stats,
                                      ptx_stream_t stream) {
    const char* who = "ptx_rand_augment_stats";
    int s = randaug_desc_check(desc, who);
    if (s) return s;
    if (!frames || !rows || !stats) return fail(PTX_ERR_INVALID, "%s: null pointer", who);
    if ((uintptr_t)stats & 7) return fail(PTX_ERR_INVALID, "%s: misaligned statistics", who);
    const size_t nframes = (size_t)desc->N * desc->T;
    PTX_HIP(hipMemsetAsync(stats, 0, nframes * kRaStatsWords * sizeof(uint32_t), (hipStream_t)stream));
    hipLaunchKernelGGL(randaug_stats_kernel, randaug_grid(desc), dim3(256), 0, (hipStream_t)stream, frames, rows, stats, desc->T,
                       desc->H * desc->W, desc->num_ops * kRaRow, desc->position);
    return hip_check(hipGetLastError(), "rand_augment_stats launch");
}

extern "C" int ptx_rand_augment_apply(const ptx_randaug_desc* desc, const uint8_t* frames, const int32_t* rows, const uint32_t* stats,
                                      void* y, const ptx_norm_desc* norm, ptx_stream_t stream) {
    const char* who = "ptx_rand_augment_apply";
    int s = randaug_desc_check(desc, who);
    if (s) return s;
    if (!frames || !rows || !y || (desc->stats && !stats)) return fail(PTX_ERR_INVALID, "%s: null pointer", who);
    if ((uintptr_t)stats & 7) return fail(PTX_ERR_INVALID, "%s: misaligned statistics", who);
    ptx_norm_desc nd = {};
    if (desc->out_mode != PTX_RESIZE_OUT_U8) {
        if ((s = check_norm(norm, 3))) return s;
        nd = *norm;
        if ((uintptr_t)y & (desc->out_mode == PTX_RESIZE_OUT_F32 ? 3 : 1)) return fail(PTX_ERR_INVALID, "%s: misaligned output", who);
    }
    const dim3 grid = randaug_grid(desc);
    const int pitch = desc->num_ops * kRaRow;
    if (desc->out_mode == PTX_RESIZE_OUT_U8)
        hipLaunchKernelGGL(randaug_apply_kernel<PTX_RESIZE_OUT_U8>, grid, dim3(256), 0, (hipStream_t)stream, frames, rows, stats, y,
                           desc->T, desc->H, desc->W, pitch, desc->position, desc->fill_r, desc->fill_g, desc->fill_b, nd);
    else if (desc->out_mode == PTX_RESIZE_OUT_F32)
        hipLaunchKernelGGL(randaug_apply_kernel<PTX_RESIZE_OUT_F32>, grid, dim3(256), 0, (hipStream_t)stream, frames, rows, stats, y,
                           desc->T, desc->H, desc->W, pitch, desc->position, desc->fill_r, desc->fill_g, desc->fill_b, nd);
    else
        hipLaunchKernelGGL(randaug_apply_kernel<PTX_RESIZE_OUT_BF16>, grid, dim3(256), 0, (hipStream_t)stream, frames, rows, stats, y,
                           desc->T, desc->H, desc->W, pitch, desc->position, desc->fill_r, desc->fill_g, desc->fill_b, nd);
    return hip_check(hipGetLastError(), "rand_augment_apply launch");
}
