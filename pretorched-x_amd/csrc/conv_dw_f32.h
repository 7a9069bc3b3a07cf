// Depthwise 3-D convolution in fp32 on channels-last activations (include/ptx_amd_dw.h states the arithmetic): the 3x3x3 conv of
// the channel-separated networks.  Compiled as part of pool_head.hip's translation unit, like linear_bf16.hip and bn_batch.hip.
//
// A streaming kernel: 27 multiply-adds per output against 8 bytes of compulsory traffic, nothing for the matrix cores.  Lanes run
// along the channels, one float4 per lane, so every global access is a coalesced 16-byte access (a wave reads up to 1 KiB of one
// row).  A lane produces a STRIP of WSEG consecutive output columns of one (n, to, ho, channel quad): per (kt, kh) it loads the
// (WSEG - 1) * SW + KW input columns under the strip once and serves all kW taps of every output from that register window --
// 9 * (WSEG + 2) loads per strip of a 3x3x3 / stride-1 conv instead of 27 * WSEG.  Every output is still its OWN fmaf chain over
// (kt, kh, kw) in that order, taps outside the volume skipped: its bits do not depend on the strip, the grid or the batch.
//
// Tile order: channel quad, strip, row inside a band of kDwBand output rows, output FRAME, band, clip -- the frames of one band
// follow each other, and every XCD owns a contiguous chunk of that list (xcd_remap), so the kT input frames two consecutive output
// frames share are re-read from that XCD's own L2, as the stem pools do.  The grid is sized to the CUs; a workgroup loops.
#include <algorithm>
#include "../../include/ptx_amd_dw.h"

namespace ptx {

constexpr int kDwBand = 4;          // output rows of a band

struct DwArgs {
    int N, Ti, Hi, Wi, ldx, To, Ho, Wo, ldy, C;
    int kT, kH, sT, sH, pT, pH, pW;
    int relu;
    int f4r, wsegs, bands;          // channel quads, strips per row, bands per frame
    unsigned total;                 // work items of this launch (< 2^31)
};

__device__ __forceinline__ f32x4 dw_fma4(const f32x4 a, const f32x4 b, const f32x4 c) {
    f32x4 r;
    r.x = fmaf(a.x, b.x, c.x); r.y = fmaf(a.y, b.y, c.y); r.z = fmaf(a.z, b.z, c.z); r.w = fmaf(a.w, b.w, c.w);
    return r;
}

template <int KW, int SW, int WSEG>
__global__ void __launch_bounds__(256) conv_dw_f32_kernel(const DwArgs a, const float* __restrict__ x, const float* __restrict__ w,
                                                          const float* __restrict__ bias, float* __restrict__ y) {
    constexpr int NCOL = (WSEG - 1) * SW + KW;
    const unsigned blk = (unsigned)xcd_remap((int)blockIdx.x, (int)gridDim.x);
    const size_t xframe = (size_t)a.Hi * a.Wi * a.ldx, yframe = (size_t)a.Ho * a.Wo * a.ldy;
    for (unsigned i = blk * 256u + threadIdx.x; i < a.total; i += gridDim.x * 256u) {
        const int q = (int)(i % (unsigned)a.f4r);
        unsigned r = i / (unsigned)a.f4r;
        const int seg = (int)(r % (unsigned)a.wsegs);
        r /= (unsigned)a.wsegs;
        const int hb = (int)(r % (unsigned)kDwBand);
        r /= (unsigned)kDwBand;
        const int to = (int)(r % (unsigned)a.To);
        r /= (unsigned)a.To;
        const int band = (int)(r % (unsigned)a.bands);
        const int n = (int)(r / (unsigned)a.bands);
        const int ho = band * kDwBand + hb;
        if (ho >= a.Ho) continue;                               // the last band of a frame may be ragged
        const int wo0 = seg * WSEG;
        const int nlive = min(WSEG, a.Wo - wo0);                // outputs of this strip inside the row (>= 1)
        const int t0 = to * a.sT - a.pT, h0 = ho * a.sH - a.pH, w0 = wo0 * SW - a.pW;
        unsigned live = 0;                                      // window columns inside the input that a live output reads
#pragma unroll
        for (int c = 0; c < NCOL; ++c) {
            bool used = false;
#pragma unroll
            for (int j = 0; j < WSEG; ++j)
                if (c >= j * SW && c < j * SW + KW && j < nlive) used = true;
            if (used && w0 + c >= 0 && w0 + c < a.Wi) live |= 1u << c;
        }
        const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
        f32x4 acc[WSEG];
#pragma unroll
        for (int j = 0; j < WSEG; ++j) acc[j] = zero;
        for (int kt = 0; kt < a.kT; ++kt) {
            const int t = t0 + kt;
            if (t < 0 || t >= a.Ti) continue;
            const float* frame = x + ((size_t)n * a.Ti + t) * xframe + q * 4;      // 64-bit base of the frame
            for (int kh = 0; kh < a.kH; ++kh) {
                const int h = h0 + kh;
                if (h < 0 || h >= a.Hi) continue;
                const float* row = frame + (ptrdiff_t)(h * a.Wi + w0) * a.ldx;     // 32-bit offsets inside the frame
                const float* wrow = w + (size_t)((kt * a.kH + kh) * KW) * a.C + q * 4;
                f32x4 v[NCOL], wk[KW];
#pragma unroll
                for (int c = 0; c < NCOL; ++c) {
                    v[c] = zero;
                    if (live >> c & 1) v[c] = *reinterpret_cast<const f32x4*>(row + (ptrdiff_t)c * a.ldx);
                }
#pragma unroll
                for (int kw = 0; kw < KW; ++kw) wk[kw] = *reinterpret_cast<const f32x4*>(wrow + (size_t)kw * a.C);
#pragma unroll
                for (int j = 0; j < WSEG; ++j)
#pragma unroll
                    for (int kw = 0; kw < KW; ++kw)
                        if (live >> (j * SW + kw) & 1) acc[j] = dw_fma4(v[j * SW + kw], wk[kw], acc[j]);
            }
        }
        const f32x4 b = *reinterpret_cast<const f32x4*>(bias + q * 4);
        float* yrow = y + ((size_t)n * a.To + to) * yframe + (size_t)(ho * a.Wo + wo0) * a.ldy + q * 4;
#pragma unroll
        for (int j = 0; j < WSEG; ++j)
            if (j < nlive) {
                f32x4 o;
                o.x = acc[j].x + b.x; o.y = acc[j].y + b.y; o.z = acc[j].z + b.z; o.w = acc[j].w + b.w;
                if (a.relu) { o.x = fmaxf(o.x, 0.f); o.y = fmaxf(o.y, 0.f); o.z = fmaxf(o.z, 0.f); o.w = fmaxf(o.w, 0.f); }
                *reinterpret_cast<f32x4*>(yrow + (size_t)j * a.ldy) = o;
            }
    }
}

// The alternative that was measured against the register window and lost (PTX_DW_FORM_LDS of
// ptx_conv3d_dw_f32_force_form keeps it runnable): a workgroup owns kDwBand x kDwLdsW outputs of kDwLdsQ channel quads of one
// output frame, stages the halo of one temporal tap in LDS -- every input element is requested from L1 / L2 ONCE per tap and
// workgroup -- and every lane reads its kH x kW taps from there.  The chain of an output is the same (kt, kh, kw), so are its bits.
constexpr int kDwLdsW = 8, kDwLdsQ = 16;
constexpr int kDwLdsRows = (kDwBand - 1) * 2 + 3, kDwLdsCols = (kDwLdsW - 1) * 2 + 3;       // the halo at stride 2, 3 taps

__global__ void __launch_bounds__(256) conv_dw_f32_lds_kernel(const DwArgs a, int kW, int sW, int wtiles, int qgroups,
                                                              const float* __restrict__ x, const float* __restrict__ w,
                                                              const float* __restrict__ bias, float* __restrict__ y) {
    __shared__ f32x4 halo[kDwLdsRows * kDwLdsCols * kDwLdsQ];
    const int ql = threadIdx.x % kDwLdsQ, pos0 = threadIdx.x / kDwLdsQ;          // 16 quads x 16 positions; 2 outputs per lane
    const int nrows = (kDwBand - 1) * a.sH + a.kH, ncols = (kDwLdsW - 1) * sW + kW;
    const size_t xframe = (size_t)a.Hi * a.Wi * a.ldx, yframe = (size_t)a.Ho * a.Wo * a.ldy;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    for (unsigned tile = (unsigned)xcd_remap((int)blockIdx.x, (int)gridDim.x); tile < a.total; tile += gridDim.x) {
        unsigned r = tile;
        const int qg = (int)(r % (unsigned)qgroups);
        r /= (unsigned)qgroups;
        const int wt = (int)(r % (unsigned)wtiles);
        r /= (unsigned)wtiles;
        const int to = (int)(r % (unsigned)a.To);
        r /= (unsigned)a.To;
        const int band = (int)(r % (unsigned)a.bands);
        const int n = (int)(r / (unsigned)a.bands);
        const int q = qg * kDwLdsQ + ql;
        const bool q_ok = q < a.f4r;
        const int ho0 = band * kDwBand, wo0 = wt * kDwLdsW;
        const int t0 = to * a.sT - a.pT, h0 = ho0 * a.sH - a.pH, w0 = wo0 * sW - a.pW;
        f32x4 acc[2] = {zero, zero};
        for (int kt = 0; kt < a.kT; ++kt) {
            const int t = t0 + kt;
            if (t < 0 || t >= a.Ti) continue;                   // uniform over the workgroup
            const float* frame = x + ((size_t)n * a.Ti + t) * xframe;
            __syncthreads();                                    // the previous tap's readers are done
            for (int e = threadIdx.x; e < nrows * ncols * kDwLdsQ; e += 256) {
                const int eq = e % kDwLdsQ, p = e / kDwLdsQ;
                const int c = p % ncols, rr = p / ncols;
                const int h = h0 + rr, wi = w0 + c, gq = qg * kDwLdsQ + eq;
                f32x4 v = zero;
                if (h >= 0 && h < a.Hi && wi >= 0 && wi < a.Wi && gq < a.f4r)
                    v = *reinterpret_cast<const f32x4*>(frame + (size_t)(h * a.Wi + wi) * a.ldx + gq * 4);
                halo[e] = v;
            }
            __syncthreads();
            if (!q_ok) continue;
            for (int kh = 0; kh < a.kH; ++kh)
                for (int kw = 0; kw < kW; ++kw) {
                    const f32x4 wk = *reinterpret_cast<const f32x4*>(w + (size_t)((kt * a.kH + kh) * kW + kw) * a.C + q * 4);
#pragma unroll
                    for (int o = 0; o < 2; ++o) {
                        const int pos = pos0 + o * 16, oh = pos / kDwLdsW, ow = pos % kDwLdsW;
                        const int rr = oh * a.sH + kh, c = ow * sW + kw;
                        const int h = h0 + rr, wi = w0 + c;
                        if (h >= 0 && h < a.Hi && wi >= 0 && wi < a.Wi)          // a tap outside the volume is skipped
                            acc[o] = dw_fma4(halo[(rr * ncols + c) * kDwLdsQ + ql], wk, acc[o]);
                    }
                }
        }
        if (!q_ok) continue;
        const f32x4 b = *reinterpret_cast<const f32x4*>(bias + q * 4);
#pragma unroll
        for (int o = 0; o < 2; ++o) {
            const int pos = pos0 + o * 16, ho = ho0 + pos / kDwLdsW, wo = wo0 + pos % kDwLdsW;
            if (ho >= a.Ho || wo >= a.Wo) continue;
            f32x4 v;
            v.x = acc[o].x + b.x; v.y = acc[o].y + b.y; v.z = acc[o].z + b.z; v.w = acc[o].w + b.w;
            if (a.relu) { v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f); }
            *reinterpret_cast<f32x4*>(y + ((size_t)n * a.To + to) * yframe + (size_t)(ho * a.Wo + wo) * a.ldy + q * 4) = v;
        }
    }
}

__global__ void __launch_bounds__(256) pack_dw_weight_kernel(int C, int taps, const float* __restrict__ w,
                                                             const float* __restrict__ conv_bias, const float* __restrict__ gamma,
                                                             const float* __restrict__ beta, const float* __restrict__ mean,
                                                             const float* __restrict__ var, float eps, float* __restrict__ out,
                                                             float* __restrict__ bias_out) {
    const int total = C * taps;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256) {
        const int c = i % C, tap = i / C;
        const float s = gamma ? gamma[c] * (1.0f / sqrtf(var[c] + eps)) : 1.0f;
        out[i] = w[(size_t)c * taps + tap] * s;
        if (tap == 0) {
            const float cb = conv_bias ? conv_bias[c] : 0.f;
            bias_out[c] = (beta ? beta[c] : 0.f) + (cb - (mean ? mean[c] : 0.f)) * s;
        }
    }
}

static int dw_check(const ptx_conv3d_desc* d) {
    if (!d) return fail(PTX_ERR_INVALID, "conv3d_dw: null descriptor");
    if (d->N <= 0 || d->Ti <= 0 || d->Hi <= 0 || d->Wi <= 0 || d->To <= 0 || d->Ho <= 0 || d->Wo <= 0 || d->Ci <= 0)
        return fail(PTX_ERR_UNSUPPORTED, "conv3d_dw: non-positive extent");
    if (d->groups != d->Ci || d->Ci != d->Co)
        return fail(PTX_ERR_UNSUPPORTED, "conv3d_dw: depthwise means groups == Ci == Co (groups=%d Ci=%d Co=%d)", d->groups, d->Ci, d->Co);
    if (d->Ci % 4) return fail(PTX_ERR_UNSUPPORTED, "conv3d_dw: C=%d must be a multiple of 4 (one float4 per lane)", d->Ci);
    const int k[3] = {d->kT, d->kH, d->kW}, s[3] = {d->sT, d->sH, d->sW}, p[3] = {d->pT, d->pH, d->pW};
    const int in[3] = {d->Ti, d->Hi, d->Wi}, out[3] = {d->To, d->Ho, d->Wo};
    for (int i = 0; i < 3; ++i) {
        if (k[i] != 1 && k[i] != 3) return fail(PTX_ERR_UNSUPPORTED, "conv3d_dw: taps (%d,%d,%d): 1 or 3 per axis", d->kT, d->kH, d->kW);
        if (s[i] != 1 && s[i] != 2) return fail(PTX_ERR_UNSUPPORTED, "conv3d_dw: stride (%d,%d,%d): 1 or 2 per axis", d->sT, d->sH, d->sW);
        if (p[i] < 0 || p[i] >= k[i])
            return fail(PTX_ERR_UNSUPPORTED, "conv3d_dw: padding (%d,%d,%d) must satisfy 0 <= pad < k per axis", d->pT, d->pH, d->pW);
        if (in[i] + 2 * p[i] < k[i] || out[i] != (in[i] + 2 * p[i] - k[i]) / s[i] + 1)
            return fail(PTX_ERR_UNSUPPORTED, "conv3d_dw: output extent (%d,%d,%d) does not follow from the input, padding and stride",
                        d->To, d->Ho, d->Wo);
    }
    if (d->ldx < d->Ci || d->ldx % 4) return fail(PTX_ERR_UNSUPPORTED, "conv3d_dw: ldx=%d must cover C=%d and be a multiple of 4", d->ldx, d->Ci);
    if (d->ldy < d->Co || d->ldy % 4) return fail(PTX_ERR_UNSUPPORTED, "conv3d_dw: ldy=%d must cover C=%d and be a multiple of 4", d->ldy, d->Co);
    if (d->flags & ~PTX_EPI_RELU) return fail(PTX_ERR_UNSUPPORTED, "conv3d_dw: flags 0x%x: only PTX_EPI_RELU applies", d->flags);
    if ((int64_t)d->Hi * d->Wi * d->ldx * 4 >= (1ll << 31) || (int64_t)d->Ho * d->Wo * d->ldy * 4 >= (1ll << 31))
        return fail(PTX_ERR_UNSUPPORTED, "conv3d_dw: a frame of 2^31 bytes or more (64-bit frame base + 32-bit offsets inside it)");
    // the work items of ONE clip at the shortest strip (4 columns): the launch walks the clips in ranges below 2^31 items
    const int64_t per_clip = (int64_t)cdiv(d->Ho, kDwBand) * kDwBand * d->To * cdiv(d->Wo, 4) * (d->Ci / 4);
    if (per_clip >= (1ll << 31)) return fail(PTX_ERR_UNSUPPORTED, "conv3d_dw: a clip of 2^31 work items or more");
    return PTX_OK;
}

// which form a launch takes: 0 = the rule below, else a PTX_DW_FORM_* code (ptx_conv3d_dw_f32_force_form; PTX_DW_FORM in the
// environment sets it once, when the library is first asked)
static int g_dw_form = -1;
static int dw_form() {
    if (g_dw_form < 0) {
        const char* v = getenv("PTX_DW_FORM");
        const int f = v ? atoi(v) : 0;
        g_dw_form = (f == PTX_DW_FORM_STRIP4 || f == PTX_DW_FORM_STRIP8 || f == PTX_DW_FORM_LDS) ? f : 0;
    }
    return g_dw_form;
}

static DwArgs dw_args(const ptx_conv3d_desc* d) {
    DwArgs a;
    a.N = d->N; a.total = 0; a.wsegs = 0;
    a.Ti = d->Ti; a.Hi = d->Hi; a.Wi = d->Wi; a.ldx = d->ldx; a.To = d->To; a.Ho = d->Ho; a.Wo = d->Wo; a.ldy = d->ldy; a.C = d->Ci;
    a.kT = d->kT; a.kH = d->kH; a.sT = d->sT; a.sH = d->sH; a.pT = d->pT; a.pH = d->pH; a.pW = d->pW;
    a.relu = (d->flags & PTX_EPI_RELU) != 0;
    a.f4r = d->Ci / 4; a.bands = cdiv(d->Ho, kDwBand);
    return a;
}

static int dw_launch_lds(const ptx_conv3d_desc* d, const float* x, const float* w, const float* bias, float* y, hipStream_t st) {
    DwArgs a = dw_args(d);
    const int wtiles = cdiv(d->Wo, kDwLdsW), qgroups = cdiv(a.f4r, kDwLdsQ);
    const int64_t per_clip = (int64_t)a.bands * d->To * wtiles * qgroups;         // <= the one-row form's items: below 2^31
    const int clips = (int)std::max<int64_t>(1, std::min<int64_t>(d->N, ((1ll << 31) - 1) / per_clip));
    for (int n0 = 0; n0 < d->N; n0 += clips) {
        a.N = std::min(clips, d->N - n0);
        a.total = (unsigned)(per_clip * a.N);
        const float* xn = x + (size_t)n0 * d->Ti * d->Hi * d->Wi * d->ldx;
        float* yn = y + (size_t)n0 * d->To * d->Ho * d->Wo * d->ldy;
        const unsigned grid = (unsigned)std::min<int64_t>(a.total, (int64_t)kNumCU * 8);
        hipLaunchKernelGGL(conv_dw_f32_lds_kernel, dim3(grid), dim3(256), 0, st, a, d->kW, d->sW, wtiles, qgroups, xn, w, bias, yn);
        PTX_HIP(hipGetLastError());
    }
    return PTX_OK;
}

template <int KW, int SW>
static int dw_launch(const ptx_conv3d_desc* d, const float* x, const float* w, const float* bias, float* y, hipStream_t st) {
    // the rule, from scripts/gpu_csn_bench.py's forced forms: strips of 8 columns where a row holds two of them, else strips of 4
    const int form = dw_form();
    const int wseg = form == PTX_DW_FORM_STRIP4 ? 4 : form == PTX_DW_FORM_STRIP8 ? 8 : (d->Wo >= 16 ? 8 : 4);
    DwArgs a = dw_args(d);
    a.wsegs = cdiv(d->Wo, wseg);
    const int64_t per_clip = (int64_t)a.bands * kDwBand * d->To * a.wsegs * a.f4r;
    const int clips = (int)std::max<int64_t>(1, std::min<int64_t>(d->N, ((1ll << 31) - 1) / per_clip));
    for (int n0 = 0; n0 < d->N; n0 += clips) {
        a.N = std::min(clips, d->N - n0);
        a.total = (unsigned)(per_clip * a.N);
        const float* xn = x + (size_t)n0 * d->Ti * d->Hi * d->Wi * d->ldx;
        float* yn = y + (size_t)n0 * d->To * d->Ho * d->Wo * d->ldy;
        const dim3 g(grid_for(a.total)), b(256);
        if (wseg == 8) hipLaunchKernelGGL((conv_dw_f32_kernel<KW, SW, 8>), g, b, 0, st, a, xn, w, bias, yn);
        else hipLaunchKernelGGL((conv_dw_f32_kernel<KW, SW, 4>), g, b, 0, st, a, xn, w, bias, yn);
        PTX_HIP(hipGetLastError());
    }
    return PTX_OK;
}

}  // namespace ptx

extern "C" int ptx_conv3d_dw_f32_force_form(int32_t form) {
    if (form != 0 && form != PTX_DW_FORM_STRIP4 && form != PTX_DW_FORM_STRIP8 && form != PTX_DW_FORM_LDS)
        return fail(PTX_ERR_INVALID, "conv3d_dw: form %d is none of 0 (the library's rule), PTX_DW_FORM_STRIP4, _STRIP8, _LDS", form);
    g_dw_form = form;
    return PTX_OK;
}

extern "C" int ptx_conv3d_dw_f32_supported(const ptx_conv3d_desc* desc) {
    return dw_check(desc) == PTX_OK ? 1 : 0;
}

extern "C" int ptx_pack_dw_weight_f32(int32_t C, int32_t kT, int32_t kH, int32_t kW, const float* w, const float* conv_bias,
                                      const float* bn_gamma, const float* bn_beta, const float* bn_mean, const float* bn_var,
                                      float bn_eps, float* w_packed, float* bias_out, ptx_stream_t stream) {
    if (!w || !w_packed || !bias_out) return fail(PTX_ERR_INVALID, "pack_dw_weight: null pointer (w, w_packed and bias_out are required)");
    if (C <= 0 || C % 4 || (kT != 1 && kT != 3) || (kH != 1 && kH != 3) || (kW != 1 && kW != 3))
        return fail(PTX_ERR_INVALID, "pack_dw_weight: C=%d must be a positive multiple of 4, taps (%d,%d,%d) 1 or 3 per axis", C, kT, kH, kW);
    if (bn_gamma && (!bn_beta || !bn_mean || !bn_var)) return fail(PTX_ERR_INVALID, "pack_dw_weight: a BatchNorm needs gamma, beta, mean and var");
    const int taps = kT * kH * kW;
    hipLaunchKernelGGL(pack_dw_weight_kernel, dim3(grid_for((size_t)C * taps)), dim3(256), 0, (hipStream_t)stream, C, taps, w, conv_bias,
                       bn_gamma, bn_beta, bn_mean, bn_var, bn_eps, w_packed, bias_out);
    return hip_check(hipGetLastError(), "pack_dw_weight launch");
}

extern "C" int ptx_conv3d_dw_f32_fwd(const ptx_conv3d_desc* d, const float* x, const float* w, const float* bias, float* y,
                                     ptx_stream_t stream) {
    if (!d || !x || !w || !bias || !y) return fail(PTX_ERR_INVALID, "conv3d_dw: null pointer");
    const int s = dw_check(d);
    if (s != PTX_OK) return s;
    if (((uintptr_t)x | (uintptr_t)w | (uintptr_t)bias | (uintptr_t)y) & 15) return fail(PTX_ERR_INVALID, "conv3d_dw: misaligned pointer (16 bytes)");
    const hipStream_t st = (hipStream_t)stream;
    if (dw_form() == PTX_DW_FORM_LDS) return dw_launch_lds(d, x, w, bias, y, st);
    if (d->kW == 3 && d->sW == 1) return dw_launch<3, 1>(d, x, w, bias, y, st);
    if (d->kW == 3) return dw_launch<3, 2>(d, x, w, bias, y, st);
    if (d->sW == 1) return dw_launch<1, 1>(d, x, w, bias, y, st);
    return dw_launch<1, 2>(d, x, w, bias, y, st);
}
