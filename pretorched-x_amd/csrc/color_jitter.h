// Per-clip ColorJitter / RandomGrayscale of decoded uint8 frames [N][T][H][W][3], equal to Pillow bit for bit
// (include/ptx_amd_color.h states the arithmetic; transforms.color_jitter_numpy is its numpy statement).  Compiled as part
// of pack_layout.hip's translation unit, like resize_views.hip.
//
// Two launches.  color_stats_kernel (only when a clip's list holds contrast) recomputes the pointwise entries in front of
// contrast and sums the luma of every frame into one 64-bit counter (wave shuffles, LDS across the four waves, one integer
// atomic per workgroup: integer sums do not depend on the order, so the result is deterministic).  color_apply_kernel runs
// the whole list per pixel and writes uint8 frames or the normalised planes.  Both run over (frame, chunk): a workgroup
// owns kCjChunk groups of FOUR pixels of one frame -- 12 bytes = three whole dwords, whatever the frame's alignment:
// a frame at byte address a has `head` = a & 3 leading pixels in front of the first pixel that starts on a dword, then the
// groups, then a tail of 0..3 pixels; head and tail are done byte by byte by chunk 0.  A lane's four pixels are consecutive,
// so a plane store is one 16-byte (fp32) or 8-byte (bf16) piece per lane and channel, coalesced over the wave.
// A list is uniform over a workgroup (one frame, one clip): every branch on an op code is a scalar branch, and clips without
// hue never enter the fp64 HSV code nor build its tables.
//
// Nothing here may be contracted or re-associated.  The _rn intrinsics are inline functions around the plain operators (the
// compiler contracts through them), so every function that does floating-point work is written with operators and
// switches contraction off for its body, like the fp64 table builder of pack_layout.hip.
#pragma once
#include "resize_common.h"
#include "../../include/ptx_amd_color.h"

namespace ptx {

constexpr int kCjOps = PTX_COLOR_MAX_OPS;
constexpr int kCjPerLane = 4;                        // groups of four pixels per lane
constexpr int kCjChunk = 256 * kCjPerLane;           // groups per workgroup

// HSV -> RGB needs H * 6 / 255 (its floor and its fraction) and S / 255 in fp64: functions of one byte, so a workgroup
// whose list has hue builds them once (256 threads, one entry each) and the pixels skip two fp64 divisions.
struct CjHueTables {
    double f[256], fs[256];
    int sextant[256];
};

// position of `code` in one clip's list (uniform scalar loads), or -1
__device__ __forceinline__ int cj_index_of(const int* __restrict__ ops, int code) {
    int at = -1;
#pragma unroll
    for (int k = kCjOps - 1; k >= 0; --k)
        if (ops[k] == code) at = k;
    return at;
}

__device__ __forceinline__ void cj_build_hue_tables(CjHueTables& t) {
#pragma clang fp contract(off)
    const int i = threadIdx.x;                         // 256 threads
    const double x = (double)i * 6.0 / 255.0;
    const double fl = floor(x);
    t.f[i] = x - fl;
    t.sextant[i] = (int)fl % 6;
    t.fs[i] = (double)i / 255.0;
}

__device__ __forceinline__ int cj_luma(int r, int g, int b) { return (r * 19595 + g * 38470 + b * 7471 + 0x8000) >> 16; }

__device__ __forceinline__ int cj_blend(int d, int x, float f) {
#pragma clang fp contract(off)
    const float scaled = f * (float)(x - d);           // rounded to fp32 on its own: no FMA
    const float t = (float)d + scaled;
    return t <= 0.f ? 0 : (t >= 255.f ? 255 : (int)t);
}

__device__ __forceinline__ int cj_round8(double a) {
#pragma clang fp contract(off)
    return clip8((int)floor(a + 0.5));
}

// the frame's mean luma as ImageEnhance.Contrast takes it: int(sum / count + 0.5) in fp64
__device__ __forceinline__ int cj_mean(unsigned long long sum, int P) {
#pragma clang fp contract(off)
    return (int)((double)sum / (double)P + 0.5);
}

__device__ __forceinline__ void cj_hue(int& r, int& g, int& b, int shift, const CjHueTables& tab) {
#pragma clang fp contract(off)
    const int maxc = max(r, max(g, b)), minc = min(r, min(g, b));
    int H = 0, S = 0;
    const int V = maxc;
    if (maxc != minc) {
        const float cr = (float)(maxc - minc);
        const float s = cr / (float)maxc;              // fp32 divisions, correctly rounded
        const float rc = (float)(maxc - r) / cr, gc = (float)(maxc - g) / cr, bc = (float)(maxc - b) / cr;
        double hd;
        if (r == maxc) hd = (double)bc - (double)gc;
        else if (g == maxc) hd = 2.0 + (double)rc - (double)bc;
        else hd = 4.0 + (double)gc - (double)rc;
        const float hf = (float)hd;
        const double h6 = (double)hf / 6.0 + 1.0;      // in [5/6, 2): fmod(h6, 1) is h6 - floor(h6), exact
        const float h2 = (float)(h6 - floor(h6));
        H = clip8((int)((double)h2 * 255.0));
        S = clip8((int)((double)s * 255.0));
    }
    H = (H + shift) & 255;
    if (S == 0) {
        r = g = b = V;
        return;
    }
    const double f = tab.f[H], fs = tab.fs[S], v = (double)V;
    const int p = cj_round8(v * (1.0 - fs));
    const int q = cj_round8(v * (1.0 - fs * f));
    const int t = cj_round8(v * (1.0 - fs * (1.0 - f)));
    switch (tab.sextant[H]) {
        case 0: r = V, g = t, b = p; break;
        case 1: r = q, g = V, b = p; break;
        case 2: r = p, g = V, b = t; break;
        case 3: r = p, g = q, b = V; break;
        case 4: r = t, g = p, b = V; break;
        default: r = V, g = p, b = q; break;
    }
}

// The first `count` entries of one clip's list on a lane's four pixels; m is the frame's mean luma (contrast only).  The
// entries are read where they lie (uniform addresses: scalar loads), the loop over them is not unrolled, so the code of an
// op exists once per kernel.
__device__ __forceinline__ void cj_run(int (&r)[4], int (&g)[4], int (&b)[4], const int* __restrict__ ops, const float* __restrict__ fac,
                                       int count, int m, const CjHueTables& tab) {
#pragma unroll 1
    for (int k = 0; k < count; ++k) {
        const int op = ops[k];                         // uniform over the workgroup
        const float f = fac[k];
        if (op == PTX_COLOR_HUE) {
            const int shift = (int)f & 255;
#pragma unroll
            for (int e = 0; e < 4; ++e) cj_hue(r[e], g[e], b[e], shift, tab);
        } else if (op == PTX_COLOR_GRAYSCALE) {
#pragma unroll
            for (int e = 0; e < 4; ++e) r[e] = g[e] = b[e] = cj_luma(r[e], g[e], b[e]);
        } else if (op != PTX_COLOR_NONE) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int d = op == PTX_COLOR_BRIGHTNESS ? 0 : (op == PTX_COLOR_CONTRAST ? m : cj_luma(r[e], g[e], b[e]));
                r[e] = cj_blend(d, r[e], f), g[e] = cj_blend(d, g[e], f), b[e] = cj_blend(d, b[e], f);
            }
        }
    }
}

// A frame of P pixels at `fin`: `head` pixels in front of the first pixel that starts on a dword (3 p + a = 0 mod 4 <=>
// p = a mod 4), `groups` groups of four pixels (three aligned dwords each), `tail` pixels behind them.
struct CjSpan {
    int head, groups, tail;
};
__device__ __forceinline__ CjSpan cj_span(const unsigned char* fin, int P) {
    CjSpan s;
    s.head = min((int)(reinterpret_cast<uintptr_t>(fin) & 3), P);
    s.groups = (P - s.head) >> 2;
    s.tail = P - s.head - 4 * s.groups;
    return s;
}

// The byte-by-byte pixels, done by chunk 0 in a pass of their own (pass -1, one pixel per lane in slot 0): thread t < head
// is pixel t, thread 64 + t (t < tail) is pixel head + 4 groups + t.  -1: this lane has none.
__device__ __forceinline__ int cj_edge_pixel(const CjSpan& s) {
    const int t = threadIdx.x;
    if (t < s.head) return t;
    if (t >= 64 && t - 64 < s.tail) return s.head + 4 * s.groups + (t - 64);
    return -1;
}

// Pass `it` of a workgroup's lane: the pixel index of slot 0 and how many slots are live (0: nothing to do), loaded.
__device__ __forceinline__ int cj_load(const unsigned char* __restrict__ fin, const CjSpan& sp, int chunk, int it, int& p0,
                                       int (&r)[4], int (&g)[4], int (&b)[4]) {
    if (it < 0) {
        p0 = cj_edge_pixel(sp);
        if (p0 < 0) return 0;
#pragma unroll
        for (int e = 0; e < 4; ++e) r[e] = g[e] = b[e] = 0;
        r[0] = fin[3 * p0], g[0] = fin[3 * p0 + 1], b[0] = fin[3 * p0 + 2];
        return 1;
    }
    const int gi = chunk * kCjChunk + it * 256 + threadIdx.x;
    if (gi >= sp.groups) return 0;
    p0 = sp.head + 4 * gi;
    const unsigned* w = reinterpret_cast<const unsigned*>(fin + 3 * p0);       // a dword boundary by the choice of head
    const unsigned w0 = w[0], w1 = w[1], w2 = w[2];
    r[0] = w0 & 255, g[0] = (w0 >> 8) & 255, b[0] = (w0 >> 16) & 255;
    r[1] = w0 >> 24, g[1] = w1 & 255, b[1] = (w1 >> 8) & 255;
    r[2] = (w1 >> 16) & 255, g[2] = w1 >> 24, b[2] = w2 & 255;
    r[3] = (w2 >> 8) & 255, g[3] = (w2 >> 16) & 255, b[3] = w2 >> 24;
    return 4;
}

__global__ void __launch_bounds__(256) color_stats_kernel(const unsigned char* __restrict__ frames, const int* __restrict__ ops,
                                                          const float* __restrict__ fac, unsigned long long* __restrict__ sums,
                                                          int T, int P, int chunks) {
    __shared__ CjHueTables tab;
    __shared__ unsigned part[4];
    const int frame = blockIdx.x / chunks, chunk = blockIdx.x - frame * chunks;
    ops += (size_t)(frame / T) * kCjOps, fac += (size_t)(frame / T) * kCjOps;
    const int count = cj_index_of(ops, PTX_COLOR_CONTRAST);   // the entries in front of contrast
    if (count < 0) return;                                    // uniform: this clip has no contrast
    const int hue = cj_index_of(ops, PTX_COLOR_HUE);
    if (hue >= 0 && hue < count) {
        cj_build_hue_tables(tab);
        __syncthreads();
    }
    const unsigned char* fin = frames + (size_t)frame * P * 3;
    const CjSpan sp = cj_span(fin, P);
    unsigned acc = 0;
#pragma unroll 1
    for (int it = chunk == 0 ? -1 : 0; it < kCjPerLane; ++it) {
        int r[4], g[4], b[4], p0;
        const int live = cj_load(fin, sp, chunk, it, p0, r, g, b);
        if (live == 0) continue;
        cj_run(r, g, b, ops, fac, count, 0, tab);
        acc += cj_luma(r[0], g[0], b[0]);
        if (live == 4) acc += cj_luma(r[1], g[1], b[1]) + cj_luma(r[2], g[2], b[2]) + cj_luma(r[3], g[3], b[3]);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) atomicAdd(&sums[frame], (unsigned long long)part[0] + part[1] + part[2] + part[3]);
}

template <int OUT>
__global__ void __launch_bounds__(256) color_apply_kernel(const unsigned char* __restrict__ frames, const int* __restrict__ ops,
                                                          const float* __restrict__ fac,
                                                          const unsigned long long* __restrict__ sums, void* __restrict__ y,
                                                          int T, int P, int chunks, ptx_norm_desc nd) {
    __shared__ CjHueTables tab;
    const int frame = blockIdx.x / chunks, chunk = blockIdx.x - frame * chunks;
    const int n = frame / T, t = frame - n * T;
    ops += (size_t)n * kCjOps, fac += (size_t)n * kCjOps;
    int m = 0;
    if (sums && cj_index_of(ops, PTX_COLOR_CONTRAST) >= 0)
        m = cj_mean(sums[frame], P);
    if (cj_index_of(ops, PTX_COLOR_HUE) >= 0) {               // uniform
        cj_build_hue_tables(tab);
        __syncthreads();
    }
    const unsigned char* fin = frames + (size_t)frame * P * 3;
    const CjSpan sp = cj_span(fin, P);
    // uint8 out: pixel p of the frame is byte (frame P + p) 3 of y.  planes out: element (plane P + p), plane = (3 n + ch) T + t
    const size_t plane0 = (size_t)n * 3 * T + t;
    // whole-piece stores need the piece of group 0 aligned (every group then is: a group is 12 / 16 / 8 bytes further)
    bool vec;
    if (OUT == PTX_RESIZE_OUT_U8)
        vec = ((reinterpret_cast<uintptr_t>(y) + ((size_t)frame * P + sp.head) * 3) & 3) == 0;
    else {
        const int esz = OUT == PTX_RESIZE_OUT_F32 ? 4 : 2;
        vec = ((reinterpret_cast<uintptr_t>(y) + (plane0 * P + sp.head) * esz) & (4 * esz - 1)) == 0 &&
              (((size_t)T * P * esz) & (4 * esz - 1)) == 0;   // the three planes of a frame are T * P elements apart
    }
#pragma unroll 1
    for (int it = chunk == 0 ? -1 : 0; it < kCjPerLane; ++it) {
        int r[4], g[4], b[4], p0;
        const int live = cj_load(fin, sp, chunk, it, p0, r, g, b);
        if (live == 0) continue;
        cj_run(r, g, b, ops, fac, kCjOps, m, tab);
        if (OUT == PTX_RESIZE_OUT_U8) {
            unsigned char* o = static_cast<unsigned char*>(y) + ((size_t)frame * P + p0) * 3;
            if (live == 4 && vec) {
                unsigned* ow = reinterpret_cast<unsigned*>(o);
                ow[0] = r[0] | g[0] << 8 | b[0] << 16 | (unsigned)r[1] << 24;
                ow[1] = g[1] | b[1] << 8 | r[2] << 16 | (unsigned)g[2] << 24;
                ow[2] = b[2] | r[3] << 8 | g[3] << 16 | (unsigned)b[3] << 24;
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (e < live) o[3 * e] = (unsigned char)r[e], o[3 * e + 1] = (unsigned char)g[e], o[3 * e + 2] = (unsigned char)b[e];
            }
            continue;
        }
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const int cin = (nd.swap_rb && ch != 1) ? 2 - ch : ch;
            float v[4];
#pragma unroll
            for (int e = 0; e < 4; ++e)
                v[e] = normalise_u8((unsigned char)(cin == 0 ? r[e] : cin == 1 ? g[e] : b[e]), nd.mean[ch], nd.std[ch], nd.to_255);
            const size_t o = (plane0 + (size_t)ch * T) * P + p0;
            if (OUT == PTX_RESIZE_OUT_F32) {
                float* yo = static_cast<float*>(y) + o;
                if (live == 4 && vec) {
                    *reinterpret_cast<f32x4*>(yo) = f32x4{v[0], v[1], v[2], v[3]};
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (e < live) yo[e] = v[e];
                }
            } else {
                unsigned short h[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) h[e] = __builtin_bit_cast(unsigned short, (__bf16)v[e]);   // nearest even, as PTX_RESIZE_OUT_BF16
                unsigned short* yo = static_cast<unsigned short*>(y) + o;
                if (live == 4 && vec) {
                    *reinterpret_cast<u32x2*>(yo) = u32x2{h[0] | (unsigned)h[1] << 16, h[2] | (unsigned)h[3] << 16};
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (e < live) yo[e] = h[e];
                }
            }
        }
    }
}

// Host-side checks shared by the three entry points (no device needed).
static int color_desc_check(const ptx_color_desc* d, const char* who) {
    if (!d) return fail(PTX_ERR_INVALID, "%s: null descriptor", who);
    if (d->N <= 0 || d->T <= 0 || d->H <= 0 || d->W <= 0)
        return fail(PTX_ERR_INVALID, "%s: non-positive extent (N=%d T=%d H=%d W=%d)", who, d->N, d->T, d->H, d->W);
    if (d->out_mode != PTX_RESIZE_OUT_U8 && d->out_mode != PTX_RESIZE_OUT_F32 && d->out_mode != PTX_RESIZE_OUT_BF16)
        return fail(PTX_ERR_INVALID, "%s: out_mode=%d is not a PTX_RESIZE_OUT_* value", who, d->out_mode);
    const int64_t P = (int64_t)d->H * d->W;
    if (P * 3 > INT32_MAX) return fail(PTX_ERR_UNSUPPORTED, "%s: a frame of %dx%d pixels exceeds 32-bit indexing", who, d->H, d->W);
    const int64_t chunks = std::max<int64_t>(1, cdiv64(P >> 2, kCjChunk));
    if ((int64_t)d->N * d->T * chunks > INT32_MAX || (int64_t)d->N * kCjOps > INT32_MAX)
        return fail(PTX_ERR_UNSUPPORTED, "%s: %d x %d frames of %dx%d exceed the grid", who, d->N, d->T, d->H, d->W);
    return PTX_OK;
}

static int color_chunks(const ptx_color_desc* d) { return (int)std::max<int64_t>(1, cdiv64(((int64_t)d->H * d->W) >> 2, kCjChunk)); }

}  // namespace ptx

using namespace ptx;

extern "C" int ptx_color_jitter_supported(const ptx_color_desc* desc, const int32_t* ops, const float* factors) {
    const char* who = "ptx_color_jitter_supported";
    if (color_desc_check(desc, who)) return 0;
    if (!ops || !factors) return fail(PTX_ERR_INVALID, "%s: null pointer", who), 0;
    bool contrast = false;
    for (int n = 0; n < desc->N; ++n) {
        unsigned seen = 0;
        for (int k = 0; k < kCjOps; ++k) {
            const int op = ops[n * kCjOps + k];
            const float f = factors[n * kCjOps + k];
            if (op < PTX_COLOR_NONE || op > PTX_COLOR_GRAYSCALE)
                return fail(PTX_ERR_INVALID, "%s: clip %d entry %d: op code %d out of range 0..%d", who, n, k, op, PTX_COLOR_GRAYSCALE), 0;
            if (op == PTX_COLOR_NONE) continue;
            if (seen >> op & 1) return fail(PTX_ERR_INVALID, "%s: clip %d entry %d: op code %d is repeated", who, n, k, op), 0;
            seen |= 1u << op;
            if (op == PTX_COLOR_HUE) {
                if (!(f >= 0.f && f <= 255.f) || f != (float)(int)f)
                    return fail(PTX_ERR_INVALID, "%s: clip %d entry %d: hue shift %g is not an integer 0..255", who, n, k, (double)f), 0;
            } else if (op != PTX_COLOR_GRAYSCALE) {
                if (!(f >= 0.f) || !(f <= 3.0e38f))
                    return fail(PTX_ERR_INVALID, "%s: clip %d entry %d: factor %g must be finite and >= 0", who, n, k, (double)f), 0;
            }
            contrast |= op == PTX_COLOR_CONTRAST;
        }
    }
    if (contrast != (desc->contrast != 0))
        return fail(PTX_ERR_INVALID, "%s: desc.contrast=%d but the lists %s contrast", who, desc->contrast, contrast ? "hold" : "hold no"), 0;
    return 1;
}

extern "C" int ptx_color_jitter_stats(const ptx_color_desc* desc, const uint8_t* frames, const int32_t* ops, const float* factors,
                                      uint64_t* sums, ptx_stream_t stream) {
    const char* who = "ptx_color_jitter_stats";
    int s = color_desc_check(desc, who);
    if (s) return s;
    if (!frames || !ops || !factors || !sums) return fail(PTX_ERR_INVALID, "%s: null pointer", who);
    if ((uintptr_t)sums & 7) return fail(PTX_ERR_INVALID, "%s: misaligned counters", who);
    const int chunks = color_chunks(desc);
    const size_t nframes = (size_t)desc->N * desc->T;
    PTX_HIP(hipMemsetAsync(sums, 0, nframes * sizeof(uint64_t), (hipStream_t)stream));
    hipLaunchKernelGGL(color_stats_kernel, dim3((unsigned)(nframes * chunks)), dim3(256), 0, (hipStream_t)stream, frames, ops, factors,
                       reinterpret_cast<unsigned long long*>(sums), desc->T, desc->H * desc->W, chunks);
    return hip_check(hipGetLastError(), "color_jitter_stats launch");
}

extern "C" int ptx_color_jitter_apply(const ptx_color_desc* desc, const uint8_t* frames, const int32_t* ops, const float* factors,
                                      const uint64_t* sums, void* y, const ptx_norm_desc* norm, ptx_stream_t stream) {
    const char* who = "ptx_color_jitter_apply";
    int s = color_desc_check(desc, who);
    if (s) return s;
    if (!frames || !ops || !factors || !y || (desc->contrast && !sums)) return fail(PTX_ERR_INVALID, "%s: null pointer", who);
    if ((uintptr_t)sums & 7) return fail(PTX_ERR_INVALID, "%s: misaligned counters", who);
    ptx_norm_desc nd = {};
    if (desc->out_mode != PTX_RESIZE_OUT_U8) {
        if ((s = check_norm(norm, 3))) return s;
        nd = *norm;
        if ((uintptr_t)y & (desc->out_mode == PTX_RESIZE_OUT_F32 ? 3 : 1)) return fail(PTX_ERR_INVALID, "%s: misaligned output", who);
    }
    const int chunks = color_chunks(desc);
    const dim3 grid((unsigned)((size_t)desc->N * desc->T * chunks));
    const int P = desc->H * desc->W;
    const unsigned long long* su = desc->contrast ? reinterpret_cast<const unsigned long long*>(sums) : nullptr;
    if (desc->out_mode == PTX_RESIZE_OUT_U8)
        hipLaunchKernelGGL(color_apply_kernel<PTX_RESIZE_OUT_U8>, grid, dim3(256), 0, (hipStream_t)stream, frames, ops, factors, su, y,
                           desc->T, P, chunks, nd);
    else if (desc->out_mode == PTX_RESIZE_OUT_F32)
        hipLaunchKernelGGL(color_apply_kernel<PTX_RESIZE_OUT_F32>, grid, dim3(256), 0, (hipStream_t)stream, frames, ops, factors, su, y,
                           desc->T, P, chunks, nd);
    else
        hipLaunchKernelGGL(color_apply_kernel<PTX_RESIZE_OUT_BF16>, grid, dim3(256), 0, (hipStream_t)stream, frames, ops, factors, su, y,
                           desc->T, P, chunks, nd);
    return hip_check(hipGetLastError(), "color_jitter_apply launch");
}
