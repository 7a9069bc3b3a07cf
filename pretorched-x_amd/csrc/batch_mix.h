// RandomErasing per clip and MixUp / CutMix across the clips of a batch on the NORMALISED clip, in one launch
// (include/ptx_amd_mix.h states the arithmetic; transforms.batch_mix_torch is its torch statement).  Compiled as part of
// pack_layout.hip's translation unit, behind rand_augment.h.
//
// batch_mix_kernel runs over (tile, t, n): a workgroup owns kMixTile consecutive pixels of one frame of one OUTPUT clip, so the
// clip's row and its partner's are uniform over the workgroup and every branch on them is a scalar branch.  A lane owns groups
// of four consecutive pixels.  From uint8 frames it reads the group's 12 interleaved bytes of the clip and of its partner as
// the aligned dwords that cover them (any byte alignment: v_alignbyte puts them in place), de-interleaves them in registers,
// normalises through a 3 x 256 table in LDS (normalise_u8 of every byte value, built once per workgroup: the same bits, without
// 24 divisions per group) and writes each of the three planes with one 16-byte (bf16: 8-byte) store.  The groups start where
// plane 0's store is aligned; the pixels in front of and behind them are done one per lane by tile 0.  Outside a CutMix box the
// partner's group is not loaded, inside it the clip's own is not.  The memory traffic is the compulsory one: per sample one
// byte of the clip, one of the partner (MixUp) and the output element.
//
// Every element offset is 64-bit.  The multiply and the add of MixUp are compiled with contraction off (mix_up).
// A row that ptx_batch_mix_supported refuses cannot make the kernel read or write out of bounds: a partner or mode out of range
// makes the clip unmixed, a box is clamped to the frame, an erase rectangle outside the frame or a noise block outside the
// buffer is dropped.
#pragma once
#include "rand_augment.h"
#include "../../include/ptx_amd_mix.h"
#include <cmath>
#include <cstring>

namespace ptx {

constexpr int kMixRow = PTX_MIX_ROW;
constexpr int kMixPasses = 4;
constexpr int kMixTile = 256 * 4 * kMixPasses;         // pixels per workgroup: four groups of four per lane

struct MixErase {
    int kind, top, left, h, w;
    float c[3];
    long long off;
};

template <int OUT>
__device__ __forceinline__ float mix_round(float v) {  // the value as the output type holds it
    if (OUT == PTX_RESIZE_OUT_BF16) return (float)(__bf16)v;   // nearest even, as PTX_RESIZE_OUT_BF16
    return v;
}

// torch's x_p.mul(b).add_(x_i.mul(a)) on tensors of the output type: every operation rounded, none contracted
template <int OUT>
__device__ __forceinline__ float mix_up(float vp, float b, float vi, float a) {
#pragma clang fp contract(off)
    const float p = mix_round<OUT>(vp * b);
    const float q = mix_round<OUT>(vi * a);
    return mix_round<OUT>(p + q);
}

__device__ __forceinline__ float mix_widen(unsigned short h) { return __builtin_bit_cast(float, (unsigned)h << 16); }

template <int OUT>
__device__ __forceinline__ MixErase mix_erase(const int* __restrict__ row, int T, int H, int W, const void* noise, long long noise_elems) {
    MixErase e;
    e.kind = row[PTX_MIX_W_ERASE_KIND];
    e.top = row[PTX_MIX_W_ERASE], e.left = row[PTX_MIX_W_ERASE + 1], e.h = row[PTX_MIX_W_ERASE + 2], e.w = row[PTX_MIX_W_ERASE + 3];
    e.off = (long long)(((unsigned long long)(unsigned)row[PTX_MIX_W_NOISE + 1] << 32) | (unsigned)row[PTX_MIX_W_NOISE]);
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) e.c[ch] = mix_round<OUT>(__builtin_bit_cast(float, row[PTX_MIX_W_CONST + ch]));
    bool ok = (e.kind == PTX_MIX_ERASE_CONST || e.kind == PTX_MIX_ERASE_NOISE) && e.top >= 0 && e.left >= 0 && e.h > 0 && e.w > 0 &&
              e.h <= H - e.top && e.w <= W - e.left;
    if (ok && e.kind == PTX_MIX_ERASE_NOISE)
        ok = noise && e.off >= 0 && e.off <= noise_elems && 3ll * T * e.h * e.w <= noise_elems - e.off;
    if (!ok) e.kind = PTX_MIX_ERASE_NONE;
    return e;
}

__device__ __forceinline__ bool mix_in_erase(const MixErase& e, int yy, int xx) {
    return e.kind != PTX_MIX_ERASE_NONE && (unsigned)(yy - e.top) < (unsigned)e.h && (unsigned)(xx - e.left) < (unsigned)e.w;
}

template <int OUT>
__device__ __forceinline__ float mix_erased(const MixErase& e, const void* __restrict__ noise, int ch, int t, int T, int yy, int xx) {
    if (e.kind == PTX_MIX_ERASE_CONST) return e.c[ch];
    const size_t o = (size_t)e.off + ((size_t)(ch * T + t) * e.h + (yy - e.top)) * e.w + (xx - e.left);
    if (OUT == PTX_RESIZE_OUT_F32) return static_cast<const float*>(noise)[o];
    return mix_widen(static_cast<const unsigned short*>(noise)[o]);
}

// The 12 bytes at `p` (any alignment) as three dwords, read as the aligned dwords that cover them: every dword read holds at
// least one of the 12 bytes, so no read leaves the pages of the frame.
__device__ __forceinline__ void mix_load12(const unsigned char* __restrict__ p, unsigned (&d)[3]) {
    const unsigned sh = (unsigned)(reinterpret_cast<uintptr_t>(p) & 3);
    const unsigned* w = reinterpret_cast<const unsigned*>(p - sh);
    const unsigned w0 = w[0], w1 = w[1], w2 = w[2];
    if (sh == 0) {
        d[0] = w0, d[1] = w1, d[2] = w2;
        return;
    }
    const unsigned w3 = w[3];
    d[0] = __builtin_amdgcn_alignbyte(w1, w0, sh);
    d[1] = __builtin_amdgcn_alignbyte(w2, w1, sh);
    d[2] = __builtin_amdgcn_alignbyte(w3, w2, sh);
}

// The normalised values v[ch][e] of `live` pixels from pixel p0 of a frame of clip q.  u8: `fin` is the frame's first byte and
// lut the 3 x 256 table (output channel major).  planes: `fin` is plane 0's first element of the frame, the planes TP elements
// apart.
template <int SRC, int OUT>
__device__ __forceinline__ void mix_load(const void* __restrict__ fin, size_t TP, int p0, int live, const float* lut, int swap_rb,
                                         float (&v)[3][4]) {
    if (SRC == PTX_MIX_SRC_U8) {
        const unsigned char* f = static_cast<const unsigned char*>(fin) + 3 * (size_t)p0;
        int c[3][4];
        if (live == 4) {
            unsigned d[3];
            mix_load12(f, d);
            c[0][0] = d[0] & 255, c[1][0] = (d[0] >> 8) & 255, c[2][0] = (d[0] >> 16) & 255;
            c[0][1] = d[0] >> 24, c[1][1] = d[1] & 255, c[2][1] = (d[1] >> 8) & 255;
            c[0][2] = (d[1] >> 16) & 255, c[1][2] = d[1] >> 24, c[2][2] = d[2] & 255;
            c[0][3] = (d[2] >> 8) & 255, c[1][3] = (d[2] >> 16) & 255, c[2][3] = d[2] >> 24;
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int k = 0; k < 3; ++k) c[k][e] = e < live ? f[3 * e + k] : 0;
        }
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const int cin = (swap_rb && ch != 1) ? 2 - ch : ch;
#pragma unroll
            for (int e = 0; e < 4; ++e) v[ch][e] = lut[ch * 256 + (cin == 0 ? c[0][e] : cin == 1 ? c[1][e] : c[2][e])];
        }
        return;
    }
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        if (SRC == PTX_MIX_SRC_F32) {
            const float* s = static_cast<const float*>(fin) + ch * TP + p0;
            if (live == 4 && (reinterpret_cast<uintptr_t>(s) & 15) == 0) {
                const f32x4 q = *reinterpret_cast<const f32x4*>(s);
                v[ch][0] = q[0], v[ch][1] = q[1], v[ch][2] = q[2], v[ch][3] = q[3];
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) v[ch][e] = e < live ? s[e] : 0.f;
            }
        } else {
            const unsigned short* s = static_cast<const unsigned short*>(fin) + ch * TP + p0;
            if (live == 4 && (reinterpret_cast<uintptr_t>(s) & 7) == 0) {
                const u32x2 q = *reinterpret_cast<const u32x2*>(s);
                v[ch][0] = mix_widen((unsigned short)q[0]), v[ch][1] = mix_widen((unsigned short)(q[0] >> 16));
                v[ch][2] = mix_widen((unsigned short)q[1]), v[ch][3] = mix_widen((unsigned short)(q[1] >> 16));
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) v[ch][e] = e < live ? mix_widen(s[e]) : 0.f;
            }
        }
    }
}

template <int SRC, int OUT>
__global__ void __launch_bounds__(256) batch_mix_kernel(const void* __restrict__ src, const int* __restrict__ rows,
                                                        const void* __restrict__ noise, void* __restrict__ y, int N, int T, int H, int W,
                                                        unsigned wdiv0, unsigned wdiv1, long long noise_elems, ptx_norm_desc nd) {
    __shared__ float lut[768];
    const int tile = blockIdx.x, t = blockIdx.y, n = blockIdx.z;
    const unsigned wdiv[2] = {wdiv0, wdiv1};
    const int* ri = rows + (size_t)n * kMixRow;
    int mode = ri[PTX_MIX_W_MODE], pn = ri[PTX_MIX_W_PARTNER];
    if ((mode != PTX_MIX_MIXUP && mode != PTX_MIX_CUTMIX) || (unsigned)pn >= (unsigned)N) mode = PTX_MIX_NONE, pn = n;
    const int* rp = rows + (size_t)pn * kMixRow;
    const float a = __builtin_bit_cast(float, ri[PTX_MIX_W_A]), b = __builtin_bit_cast(float, ri[PTX_MIX_W_B]);
    const int by0 = min(max(ri[PTX_MIX_W_BOX], 0), H), bx0 = min(max(ri[PTX_MIX_W_BOX + 1], 0), W);
    const int by1 = min(max(ri[PTX_MIX_W_BOX + 2], 0), H), bx1 = min(max(ri[PTX_MIX_W_BOX + 3], 0), W);
    const MixErase ei = mix_erase<OUT>(ri, T, H, W, noise, noise_elems);
    MixErase ep = ei;
    if (mode != PTX_MIX_NONE) ep = mix_erase<OUT>(rp, T, H, W, noise, noise_elems);
    if (SRC == PTX_MIX_SRC_U8) {
        for (int i = threadIdx.x; i < 768; i += 256) {
            const int ch = i >> 8;
            lut[i] = mix_round<OUT>(normalise_u8((unsigned char)(i & 255), nd.mean[ch], nd.std[ch], nd.to_255));
        }
        __syncthreads();
    }
    const int P = H * W;
    const size_t TP = (size_t)T * P;
    const int esz = OUT == PTX_RESIZE_OUT_F32 ? 4 : 2;
    // the frame in the clip and in its partner, and plane 0 of the output frame (the three planes are TP elements apart)
    const void *fi, *fp;
    if (SRC == PTX_MIX_SRC_U8) {
        fi = static_cast<const unsigned char*>(src) + ((size_t)n * T + t) * P * 3;
        fp = static_cast<const unsigned char*>(src) + ((size_t)pn * T + t) * P * 3;
    } else {
        fi = static_cast<const unsigned char*>(src) + ((size_t)n * 3 * T + t) * P * esz;
        fp = static_cast<const unsigned char*>(src) + ((size_t)pn * 3 * T + t) * P * esz;
    }
    const size_t o0 = ((size_t)n * 3 * T + t) * P;
    // groups start where plane 0's store is aligned; whole-group stores also need the other planes to agree (TP = 0 mod 4)
    const int head = min((int)((0 - (reinterpret_cast<uintptr_t>(y) / esz + o0)) & 3), P);
    const int groups = (P - head) >> 2;
    const int tail = P - head - 4 * groups;
    const bool vec = (TP & 3) == 0;
#pragma unroll 1
    for (int it = tile == 0 ? -1 : 0; it < kMixPasses; ++it) {
        int p0, live;
        if (it < 0) {                                  // the pixels outside the groups, one per lane: lanes 0.., lanes 64..
            const int l = threadIdx.x;
            live = 1;
            if (l < head) p0 = l;
            else if (l >= 64 && l - 64 < tail) p0 = head + 4 * groups + (l - 64);
            else continue;
        } else {
            const int gi = (tile * kMixPasses + it) * 256 + threadIdx.x;
            if (gi >= groups) continue;
            p0 = head + 4 * gi, live = 4;
        }
        int yy[4], xx[4];
        unsigned inb = 0;                              // bit e: pixel e takes the partner's value (CutMix)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int pe = min(p0 + e, P - 1);
            yy[e] = (int)fdiv((unsigned)pe, wdiv), xx[e] = pe - yy[e] * W;
            if (mode == PTX_MIX_CUTMIX && yy[e] >= by0 && yy[e] < by1 && xx[e] >= bx0 && xx[e] < bx1) inb |= 1u << e;
        }
        const unsigned livemask = (1u << live) - 1;
        const bool own = mode != PTX_MIX_CUTMIX || (inb & livemask) != livemask;
        const bool partner = mode == PTX_MIX_MIXUP || (inb & livemask) != 0;
        float vi[3][4] = {}, vp[3][4] = {};
        if (own) {
            mix_load<SRC, OUT>(fi, TP, p0, live, lut, nd.swap_rb, vi);
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (e < live && mix_in_erase(ei, yy[e], xx[e])) {
#pragma unroll
                    for (int ch = 0; ch < 3; ++ch) vi[ch][e] = mix_erased<OUT>(ei, noise, ch, t, T, yy[e], xx[e]);
                }
        }
        if (partner) {
            mix_load<SRC, OUT>(fp, TP, p0, live, lut, nd.swap_rb, vp);
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (e < live && mix_in_erase(ep, yy[e], xx[e])) {
#pragma unroll
                    for (int ch = 0; ch < 3; ++ch) vp[ch][e] = mix_erased<OUT>(ep, noise, ch, t, T, yy[e], xx[e]);
                }
        }
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            float o[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if (mode == PTX_MIX_MIXUP)
                    o[e] = mix_up<OUT>(vp[ch][e], b, vi[ch][e], a);
                else
                    o[e] = (inb >> e & 1) ? vp[ch][e] : vi[ch][e];
            }
            const size_t oe = o0 + (size_t)ch * TP + p0;
            if (OUT == PTX_RESIZE_OUT_F32) {
                float* yo = static_cast<float*>(y) + oe;
                if (live == 4 && vec) {
                    *reinterpret_cast<f32x4*>(yo) = f32x4{o[0], o[1], o[2], o[3]};
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (e < live) yo[e] = o[e];
                }
            } else {
                unsigned short h[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) h[e] = (unsigned short)(__builtin_bit_cast(unsigned, o[e]) >> 16);   // exact: o is a bf16 value
                unsigned short* yo = static_cast<unsigned short*>(y) + oe;
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

// Soft targets: element k of row n, one element per lane.
__global__ void __launch_bounds__(256) batch_mix_targets_kernel(const long long* __restrict__ labels, const int* __restrict__ rows,
                                                                float* __restrict__ y, int N, int K, float off, float on) {
    const int n = blockIdx.y;
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= K) return;
    const int* ri = rows + (size_t)n * kMixRow;
    int mode = ri[PTX_MIX_W_MODE], pn = ri[PTX_MIX_W_PARTNER];
    if ((mode != PTX_MIX_MIXUP && mode != PTX_MIX_CUTMIX) || (unsigned)pn >= (unsigned)N) mode = PTX_MIX_NONE, pn = n;
    const float vi = labels[n] == k ? on : off;
    float v = vi;
    if (mode != PTX_MIX_NONE) {
        const float a = __builtin_bit_cast(float, ri[PTX_MIX_W_A]), b = __builtin_bit_cast(float, ri[PTX_MIX_W_B]);
        const float vp = labels[pn] == k ? on : off;
        v = mix_up<PTX_RESIZE_OUT_F32>(vp, b, vi, a);
    }
    y[(size_t)n * K + k] = v;
}

// Host-side checks shared by the entry points (no device needed).
static int mix_desc_check(const ptx_mix_desc* d, const char* who) {
    if (!d) return fail(PTX_ERR_INVALID, "%s: null descriptor", who);
    if (d->N <= 0 || d->T <= 0 || d->H <= 0 || d->W <= 0)
        return fail(PTX_ERR_INVALID, "%s: non-positive extent (N=%d T=%d H=%d W=%d)", who, d->N, d->T, d->H, d->W);
    if (d->src_mode != PTX_MIX_SRC_U8 && d->src_mode != PTX_MIX_SRC_F32 && d->src_mode != PTX_MIX_SRC_BF16)
        return fail(PTX_ERR_INVALID, "%s: src_mode=%d is not a PTX_MIX_SRC_* value", who, d->src_mode);
    if (d->out_mode != PTX_RESIZE_OUT_F32 && d->out_mode != PTX_RESIZE_OUT_BF16)
        return fail(PTX_ERR_INVALID, "%s: out_mode=%d must be PTX_RESIZE_OUT_F32 or PTX_RESIZE_OUT_BF16 (the arithmetic is defined on "
                    "normalised values)", who, d->out_mode);
    if ((d->src_mode == PTX_MIX_SRC_F32 && d->out_mode != PTX_RESIZE_OUT_F32) ||
        (d->src_mode == PTX_MIX_SRC_BF16 && d->out_mode != PTX_RESIZE_OUT_BF16))
        return fail(PTX_ERR_INVALID, "%s: a normalised source writes its own type (src_mode=%d, out_mode=%d)", who, d->src_mode, d->out_mode);
    if (d->noise_elems < 0) return fail(PTX_ERR_INVALID, "%s: noise_elems=%lld is negative", who, (long long)d->noise_elems);
    const int64_t P = (int64_t)d->H * d->W;
    if (P * 3 > INT32_MAX) return fail(PTX_ERR_UNSUPPORTED, "%s: a frame of %dx%d pixels exceeds 32-bit indexing", who, d->H, d->W);
    if (d->T > 65535 || d->N > 65535)
        return fail(PTX_ERR_UNSUPPORTED, "%s: %d x %d frames exceed the grid (N, T <= 65535)", who, d->N, d->T);
    return PTX_OK;
}

template <int SRC, int OUT>
static void mix_launch(const ptx_mix_desc* d, const void* src, const int32_t* rows, const void* noise, void* y, const ptx_norm_desc& nd,
                       hipStream_t st) {
    unsigned wdiv[2];
    fdiv_make((unsigned)d->W, wdiv);
    const int64_t P = (int64_t)d->H * d->W;
    const dim3 grid((unsigned)std::max<int64_t>(1, cdiv64(P >> 2, kMixTile / 4)), (unsigned)d->T, (unsigned)d->N);
    hipLaunchKernelGGL((batch_mix_kernel<SRC, OUT>), grid, dim3(256), 0, st, src, rows, noise, y, d->N, d->T, d->H, d->W, wdiv[0], wdiv[1],
                       (long long)d->noise_elems, nd);
}

}  // namespace ptx

using namespace ptx;

extern "C" int ptx_batch_mix_supported(const ptx_mix_desc* desc, const int32_t* rows) {
    const char* who = "ptx_batch_mix_supported";
    if (mix_desc_check(desc, who)) return 0;
    if (!rows) return fail(PTX_ERR_INVALID, "%s: null pointer", who), 0;
    for (int n = 0; n < desc->N; ++n) {
        const int32_t* row = rows + (size_t)n * kMixRow;
        const int pn = row[PTX_MIX_W_PARTNER], mode = row[PTX_MIX_W_MODE], kind = row[PTX_MIX_W_ERASE_KIND];
        if (pn < 0 || pn >= desc->N)
            return fail(PTX_ERR_INVALID, "%s: clip %d: partner %d out of range 0..%d", who, n, pn, desc->N - 1), 0;
        if (mode < PTX_MIX_NONE || mode > PTX_MIX_CUTMIX)
            return fail(PTX_ERR_INVALID, "%s: clip %d: mode code %d out of range 0..%d", who, n, mode, PTX_MIX_CUTMIX), 0;
        if (kind < PTX_MIX_ERASE_NONE || kind > PTX_MIX_ERASE_NOISE)
            return fail(PTX_ERR_INVALID, "%s: clip %d: erase kind %d out of range 0..%d", who, n, kind, PTX_MIX_ERASE_NOISE), 0;
        float ab[2];
        memcpy(ab, row + PTX_MIX_W_A, sizeof ab);
        for (int k = 0; k < 2; ++k)
            if (!std::isfinite(ab[k]) || ab[k] < 0.f || ab[k] > 1.f)
                return fail(PTX_ERR_INVALID, "%s: clip %d: lam weight %c = %g must be finite and in [0, 1]", who, n, "ab"[k], (double)ab[k]), 0;
        const int32_t* bx = row + PTX_MIX_W_BOX;
        if (bx[0] < 0 || bx[1] < 0 || bx[2] < bx[0] || bx[3] < bx[1] || bx[2] > desc->H || bx[3] > desc->W)
            return fail(PTX_ERR_INVALID, "%s: clip %d: the box rows %d..%d, columns %d..%d has a negative extent or leaves the %dx%d frame",
                        who, n, bx[0], bx[2], bx[1], bx[3], desc->H, desc->W), 0;
        const int32_t* er = row + PTX_MIX_W_ERASE;
        if (er[0] < 0 || er[1] < 0 || er[2] < 0 || er[3] < 0 || er[2] > desc->H - er[0] || er[3] > desc->W - er[1])
            return fail(PTX_ERR_INVALID, "%s: clip %d: the %dx%d erase rectangle at (%d, %d) has a negative extent or leaves the %dx%d "
                        "frame", who, n, er[2], er[3], er[0], er[1], desc->H, desc->W), 0;
        if (kind == PTX_MIX_ERASE_NOISE) {
            const int64_t off = (int64_t)(((uint64_t)(uint32_t)row[PTX_MIX_W_NOISE + 1] << 32) | (uint32_t)row[PTX_MIX_W_NOISE]);
            const int64_t need = 3ll * desc->T * er[2] * er[3];
            if (off < 0 || off > desc->noise_elems || need > desc->noise_elems - off)
                return fail(PTX_ERR_INVALID, "%s: clip %d: the noise block of %lld elements at offset %lld lies beyond the noise buffer "
                            "(%lld elements)", who, n, (long long)need, (long long)off, (long long)desc->noise_elems), 0;
        }
    }
    return 1;
}

extern "C" int ptx_batch_mix_apply(const ptx_mix_desc* desc, const void* src, const int32_t* rows, const void* noise, void* y,
                                   const ptx_norm_desc* norm, ptx_stream_t stream) {
    const char* who = "ptx_batch_mix_apply";
    int s = mix_desc_check(desc, who);
    if (s) return s;
    if (!src || !rows || !y || (desc->noise_elems > 0 && !noise)) return fail(PTX_ERR_INVALID, "%s: null pointer", who);
    const int esz = desc->out_mode == PTX_RESIZE_OUT_F32 ? 4 : 2;
    if ((uintptr_t)y & (esz - 1)) return fail(PTX_ERR_INVALID, "%s: misaligned output", who);
    if ((uintptr_t)noise & (esz - 1)) return fail(PTX_ERR_INVALID, "%s: misaligned noise", who);
    if (desc->src_mode != PTX_MIX_SRC_U8 && ((uintptr_t)src & (esz - 1))) return fail(PTX_ERR_INVALID, "%s: misaligned source", who);
    if ((uintptr_t)rows & 3) return fail(PTX_ERR_INVALID, "%s: misaligned rows", who);
    ptx_norm_desc nd = {};
    if (desc->src_mode == PTX_MIX_SRC_U8) {
        if ((s = check_norm(norm, 3))) return s;
        nd = *norm;
    }
    const hipStream_t st = (hipStream_t)stream;
    if (desc->src_mode == PTX_MIX_SRC_U8 && desc->out_mode == PTX_RESIZE_OUT_F32)
        mix_launch<PTX_MIX_SRC_U8, PTX_RESIZE_OUT_F32>(desc, src, rows, noise, y, nd, st);
    else if (desc->src_mode == PTX_MIX_SRC_U8)
        mix_launch<PTX_MIX_SRC_U8, PTX_RESIZE_OUT_BF16>(desc, src, rows, noise, y, nd, st);
    else if (desc->src_mode == PTX_MIX_SRC_F32)
        mix_launch<PTX_MIX_SRC_F32, PTX_RESIZE_OUT_F32>(desc, src, rows, noise, y, nd, st);
    else
        mix_launch<PTX_MIX_SRC_BF16, PTX_RESIZE_OUT_BF16>(desc, src, rows, noise, y, nd, st);
    return hip_check(hipGetLastError(), "batch_mix_apply launch");
}

extern "C" int ptx_batch_mix_targets(const int64_t* labels, const int32_t* rows, float* y, int32_t N, int32_t K, float off, float on,
                                     ptx_stream_t stream) {
    const char* who = "ptx_batch_mix_targets";
    if (!labels || !rows || !y) return fail(PTX_ERR_INVALID, "%s: null pointer", who);
    if (N <= 0 || K <= 0) return fail(PTX_ERR_INVALID, "%s: non-positive extent (N=%d K=%d)", who, N, K);
    if (N > 65535) return fail(PTX_ERR_UNSUPPORTED, "%s: N=%d exceeds the grid (N <= 65535)", who, N);
    if (((uintptr_t)labels & 7) || ((uintptr_t)rows & 3) || ((uintptr_t)y & 3)) return fail(PTX_ERR_INVALID, "%s: misaligned pointer", who);
    hipLaunchKernelGGL(batch_mix_targets_kernel, dim3((unsigned)cdiv(K, 256), (unsigned)N), dim3(256), 0, (hipStream_t)stream,
                       reinterpret_cast<const long long*>(labels), rows, y, N, K, off, on);
    return hip_check(hipGetLastError(), "batch_mix_targets launch");
}
