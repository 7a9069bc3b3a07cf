// Batch-statistics BatchNorm forward on channels-last fp32 activations (include/ptx_amd_bn.h): per-channel batch moments,
// the scale / shift + running-statistics update, and the normalise (+ residual) (+ ReLU) pass.  update_bn is built from them.
//
// All three passes are HBM bound and share one thread layout: a lane owns 4 consecutive channels (one 16-byte load per row),
// QT = min(64, next power of two of ceil(C / 4)) neighbouring lanes cover QT quads of one row -- a wave reads up to 1 KiB of
// contiguous bytes -- and the 256 / QT lane groups of a workgroup take rows RPB apart; blockIdx.y walks the quads beyond QT.
//
// Moments (bn_stats_partial_kernel + bn_stats_combine_kernel): sums about the per-channel pivot p[c] = x[0][c], see the header.
// A lane keeps 4 loads in flight (rows r, r + step, r + 2 step, r + 3 step; a row past the end is replaced by the pivot, which
// adds zero to both sums).  The grid is capped at kBnMaxWGs workgroups, so the combine adds at most that many pairs per channel:
// 64 channels x 4 slices of the workgroup list per combine workgroup, in double, the slices joined in slice order.
// Compiled as part of pool_head.hip's translation unit (its last line includes this file), like linear_bf16.hip.
#include "../../include/ptx_amd_bn.h"

namespace ptx {

constexpr int kBnMaxWGs = 4 * kNumCU;        // 4 workgroups of 4 waves per CU: 16 loads of 16 bytes in flight per lane slot

struct BnGeom {
    int c4;          // channel quads
    int qt_log2;     // log2 of the quads one workgroup covers
    int gy;          // workgroups along the channels
    int gx;          // workgroups along the rows
    int cw;          // floats per workspace row: gy * QT * 4
};

static BnGeom bn_geom(int64_t rows, int C, int rows_per_lane) {
    BnGeom g;
    g.c4 = (C + 3) / 4;
    g.qt_log2 = 0;
    while ((1 << g.qt_log2) < g.c4 && g.qt_log2 < 6) ++g.qt_log2;
    const int qt = 1 << g.qt_log2, rpb = 256 >> g.qt_log2;
    g.gy = cdiv(g.c4, qt);
    const int64_t want = cdiv64(rows, (int64_t)rpb * rows_per_lane);
    const int cap = kBnMaxWGs / g.gy > 0 ? kBnMaxWGs / g.gy : 1;
    g.gx = (int)(want < 1 ? 1 : want > cap ? cap : want);
    g.cw = g.gy * qt * 4;
    return g;
}

__global__ void __launch_bounds__(256) bn_stats_partial_kernel(const float* __restrict__ x, float* __restrict__ part,
                                                               long long rows, int c4, int ld, int qt_log2, int cw) {
    __shared__ f32x4 s1s[256], s2s[256];
    const int tid = threadIdx.x, qt = 1 << qt_log2, rpb = 256 >> qt_log2;
    const int q = blockIdx.y * qt + (tid & (qt - 1)), r0 = tid >> qt_log2;
    f32x4 s1 = {0.f, 0.f, 0.f, 0.f}, s2 = {0.f, 0.f, 0.f, 0.f};
    if (q < c4) {
        const float* col = x + (size_t)q * 4;
        const f32x4 p = *reinterpret_cast<const f32x4*>(col);
        const long long step = (long long)gridDim.x * rpb;
        for (long long r = (long long)blockIdx.x * rpb + r0; r < rows; r += 4 * step) {
            f32x4 v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const long long rr = r + u * step;
                v[u] = rr < rows ? *reinterpret_cast<const f32x4*>(col + (size_t)rr * ld) : p;
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const f32x4 d = v[u] - p;
                s1 += d;
                s2 += d * d;
            }
        }
    }
    s1s[tid] = s1;
    s2s[tid] = s2;
    __syncthreads();
    for (int s = rpb >> 1; s > 0; s >>= 1) {           // lane groups r0 and r0 + s share their quads: a fixed tree
        if (r0 < s) {
            s1s[tid] += s1s[tid + (s << qt_log2)];
            s2s[tid] += s2s[tid + (s << qt_log2)];
        }
        __syncthreads();
    }
    if (r0 == 0 && q < c4) {
        *reinterpret_cast<f32x4*>(part + ((size_t)blockIdx.x * 2 + 0) * cw + (size_t)q * 4) = s1s[tid];
        *reinterpret_cast<f32x4*>(part + ((size_t)blockIdx.x * 2 + 1) * cw + (size_t)q * 4) = s2s[tid];
    }
}

__global__ void __launch_bounds__(256) bn_stats_combine_kernel(const float* __restrict__ x, const float* __restrict__ part,
                                                               float* __restrict__ mean, float* __restrict__ var,
                                                               long long rows, int C, int cw, int nparts) {
    __shared__ double a1[256], a2[256];
    const int tid = threadIdx.x, c = blockIdx.x * 64 + (tid & 63), sl = tid >> 6;
    double S1 = 0.0, S2 = 0.0;
    if (c < C) {
        for (int b = sl; b < nparts; b += 4) {
            S1 += (double)part[((size_t)b * 2 + 0) * cw + c];
            S2 += (double)part[((size_t)b * 2 + 1) * cw + c];
        }
    }
    a1[tid] = S1;
    a2[tid] = S2;
    __syncthreads();
    if (sl == 0 && c < C) {
        S1 = ((a1[tid] + a1[tid + 64]) + a1[tid + 128]) + a1[tid + 192];
        S2 = ((a2[tid] + a2[tid + 64]) + a2[tid + 128]) + a2[tid + 192];
        const double n = (double)rows, m = S1 / n, v = S2 / n - m * m;
        mean[c] = (float)((double)x[c] + m);
        var[c] = (float)(v > 0.0 ? v : 0.0);
    }
}

__global__ void __launch_bounds__(256) bn_update_kernel(const float* __restrict__ mean, const float* __restrict__ var,
                                                        float unbias, float f, float eps, const float* __restrict__ gamma,
                                                        const float* __restrict__ beta, float* __restrict__ rmean,
                                                        float* __restrict__ rvar, float* __restrict__ scale,
                                                        float* __restrict__ shift, int C) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    const float m = mean[c], v = var[c];
    const float s = (gamma ? gamma[c] : 1.f) / sqrtf(v + eps);
    scale[c] = s;
    shift[c] = fmaf(-m, s, beta ? beta[c] : 0.f);          // one rounding: beta - mean * scale may cancel
    if (rmean) {
        rmean[c] = (1.f - f) * rmean[c] + f * m;
        rvar[c] = (1.f - f) * rvar[c] + f * (v * unbias);
    }
}

struct BnApplyArgs {
    const float* raw;
    const float* scale;
    const float* shift;
    const float* res;
    float* y;
    long long rows;
    int C, c4, ldx, ldy, qt_log2;
    unsigned flags;
    int ldr, res_C, res_T, res_H, res_W, res_sT, res_sH, res_sW;
    unsigned dW[2], dH[2], dT[2];    // fdiv constants of the output extents (shortcut A)
    int T, H, W;
};

// raw and y may be the same buffer (in place): a lane reads its 16 bytes before it writes them, and no other lane touches them
__global__ void __launch_bounds__(256) bn_apply_kernel(const BnApplyArgs a) {
    const int tid = threadIdx.x, qt = 1 << a.qt_log2, rpb = 256 >> a.qt_log2;
    const int q = blockIdx.y * qt + (tid & (qt - 1)), r0 = tid >> a.qt_log2;
    if (q >= a.c4) return;
    float sc[4], sh[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int c = q * 4 + e;
        sc[e] = c < a.C ? a.scale[c] : 0.f;
        sh[e] = c < a.C ? a.shift[c] : 0.f;
    }
    const bool relu = (a.flags & PTX_EPI_RELU) != 0, add = (a.flags & PTX_EPI_RES_ADD) != 0;
    const bool pada = (a.flags & PTX_EPI_RES_PADA) != 0 && q * 4 < a.res_C;
    const long long step = (long long)gridDim.x * rpb;
    for (long long r = (long long)blockIdx.x * rpb + r0; r < a.rows; r += step) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(a.raw + (size_t)r * a.ldx + (size_t)q * 4);
        float o[4] = {fmaf(v.x, sc[0], sh[0]), fmaf(v.y, sc[1], sh[1]), fmaf(v.z, sc[2], sh[2]), fmaf(v.w, sc[3], sh[3])};
        if (add) {
            const f32x4 t = *reinterpret_cast<const f32x4*>(a.res + (size_t)r * a.ldr + (size_t)q * 4);
            o[0] += t.x; o[1] += t.y; o[2] += t.z; o[3] += t.w;
        } else if (pada) {
            const unsigned m = (unsigned)r;
            unsigned t = fdiv(m, a.dW);
            const unsigned wo = m - t * a.W;
            unsigned u = fdiv(t, a.dH);
            const unsigned ho = t - u * a.H;
            const unsigned n = fdiv(u, a.dT);
            const unsigned to = u - n * a.T;
            const size_t pos = (((size_t)n * a.res_T + to * a.res_sT) * a.res_H + ho * a.res_sH) * a.res_W + wo * a.res_sW;
            const f32x4 s = *reinterpret_cast<const f32x4*>(a.res + pos * a.ldr + (size_t)q * 4);
            const float rv[4] = {s.x, s.y, s.z, s.w};
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (q * 4 + e < a.res_C) o[e] += rv[e];
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (relu) o[e] = fmaxf(o[e], 0.f);
            if (q * 4 + e >= a.C) o[e] = 0.f;
        }
        const f32x4 w4 = {o[0], o[1], o[2], o[3]};
        *reinterpret_cast<f32x4*>(a.y + (size_t)r * a.ldy + (size_t)q * 4) = w4;
    }
}

}  // namespace ptx

extern "C" size_t ptx_bn_batch_stats_workspace_bytes(int64_t rows, int32_t C) {
    if (rows <= 0 || C <= 0) return 0;
    const BnGeom g = bn_geom(rows, C, 16);
    return (size_t)g.gx * 2 * g.cw * sizeof(float);
}

extern "C" int ptx_bn_batch_stats_f32(const float* x, int64_t rows, int32_t C, int32_t ld, float* mean, float* var,
                                      void* workspace, size_t workspace_bytes, ptx_stream_t stream) {
    if (!x || !mean || !var) return fail(PTX_ERR_INVALID, "bn_batch_stats: null pointer");
    if (rows <= 0 || C <= 0 || ld < (C + 3) / 4 * 4 || ld % 4)
        return fail(PTX_ERR_INVALID, "bn_batch_stats: need rows >= 1, C >= 1 and a row stride that is a multiple of 4 covering round_up(C, 4) "
                    "(rows=%lld C=%d ld=%d)", (long long)rows, C, ld);
    if ((uintptr_t)x & 15) return fail(PTX_ERR_INVALID, "bn_batch_stats: x must be 16-byte aligned");
    const BnGeom g = bn_geom(rows, C, 16);
    const size_t need = (size_t)g.gx * 2 * g.cw * sizeof(float);
    if (!workspace || workspace_bytes < need || ((uintptr_t)workspace & 15))
        return fail(PTX_ERR_WORKSPACE, "bn_batch_stats: %zu bytes of 16-byte aligned workspace, ptx_bn_batch_stats_workspace_bytes asks for %zu",
                    workspace ? workspace_bytes : (size_t)0, need);
    float* part = static_cast<float*>(workspace);
    hipLaunchKernelGGL(bn_stats_partial_kernel, dim3((unsigned)g.gx, (unsigned)g.gy), dim3(256), 0, (hipStream_t)stream, x, part,
                       (long long)rows, g.c4, ld, g.qt_log2, g.cw);
    PTX_HIP(hipGetLastError());
    hipLaunchKernelGGL(bn_stats_combine_kernel, dim3((unsigned)cdiv(C, 64)), dim3(256), 0, (hipStream_t)stream, x,
                       (const float*)part, mean, var, (long long)rows, C, g.cw, g.gx);
    return hip_check(hipGetLastError(), "bn_batch_stats launch");
}

extern "C" int ptx_bn_batch_update_f32(const float* mean, const float* var, int64_t n, float f, float eps, const float* gamma,
                                       const float* beta, float* running_mean, float* running_var, float* scale, float* shift,
                                       int32_t C, ptx_stream_t stream) {
    if (!mean || !var || !scale || !shift) return fail(PTX_ERR_INVALID, "bn_batch_update: null pointer");
    if ((running_mean == nullptr) != (running_var == nullptr))
        return fail(PTX_ERR_INVALID, "bn_batch_update: running_mean and running_var go together");
    if (C <= 0) return fail(PTX_ERR_INVALID, "bn_batch_update: C=%d", C);
    if (n < 2) return fail(PTX_ERR_INVALID, "bn_batch_update: expected more than 1 value per channel (n=%lld)", (long long)n);
    const float unbias = (float)((double)n / (double)(n - 1));
    hipLaunchKernelGGL(bn_update_kernel, dim3((unsigned)cdiv(C, 256)), dim3(256), 0, (hipStream_t)stream, mean, var, unbias, f, eps,
                       gamma, beta, running_mean, running_var, scale, shift, C);
    return hip_check(hipGetLastError(), "bn_batch_update launch");
}

extern "C" int ptx_bn_apply_f32(const ptx_bn_apply_desc* d, const float* raw, const float* scale, const float* shift,
                                const float* res, float* y, ptx_stream_t stream) {
    if (!d || !raw || !scale || !shift || !y) return fail(PTX_ERR_INVALID, "bn_apply: null pointer");
    if (d->flags & ~(uint32_t)(PTX_EPI_RELU | PTX_EPI_RES_ADD | PTX_EPI_RES_PADA))
        return fail(PTX_ERR_INVALID, "bn_apply: flags 0x%x: only PTX_EPI_RELU, PTX_EPI_RES_ADD and PTX_EPI_RES_PADA apply", d->flags);
    const bool add = (d->flags & PTX_EPI_RES_ADD) != 0, pada = (d->flags & PTX_EPI_RES_PADA) != 0;
    if (add && pada) return fail(PTX_ERR_INVALID, "bn_apply: RES_ADD and RES_PADA are exclusive");
    if ((add || pada) && !res) return fail(PTX_ERR_INVALID, "bn_apply: residual flag set but res == NULL");
    const int c4 = (d->C + 3) / 4 * 4;
    if (d->N <= 0 || d->T <= 0 || d->H <= 0 || d->W <= 0 || d->C <= 0 || d->ldx < c4 || d->ldy < c4 || d->ldx % 4 || d->ldy % 4)
        return fail(PTX_ERR_INVALID, "bn_apply: bad extents (row strides are multiples of 4 covering round_up(C, 4))");
    const int64_t rows = (int64_t)d->N * d->T * d->H * d->W;
    if (rows > 0x7fffffffLL) return fail(PTX_ERR_UNSUPPORTED, "bn_apply: more than 2^31 positions");
    if (((uintptr_t)raw | (uintptr_t)y | (uintptr_t)res) & 15) return fail(PTX_ERR_INVALID, "bn_apply: misaligned pointer");
    if (add && (d->ldr < c4 || d->ldr % 4)) return fail(PTX_ERR_INVALID, "bn_apply: residual stride %d does not cover C=%d", d->ldr, d->C);
    if (pada && (d->res_C <= 0 || d->res_C > d->C || d->ldr < (d->res_C + 3) / 4 * 4 || d->ldr % 4 || d->res_T <= 0 || d->res_H <= 0 ||
                 d->res_W <= 0 || d->res_sT <= 0 || d->res_sH <= 0 || d->res_sW <= 0 || (int64_t)(d->T - 1) * d->res_sT >= d->res_T ||
                 (int64_t)(d->H - 1) * d->res_sH >= d->res_H || (int64_t)(d->W - 1) * d->res_sW >= d->res_W))
        return fail(PTX_ERR_INVALID, "bn_apply: shortcut-A residual geometry out of range");
    const BnGeom g = bn_geom(rows, d->C, 4);
    BnApplyArgs a{};
    a.raw = raw; a.scale = scale; a.shift = shift; a.res = res; a.y = y;
    a.rows = rows; a.C = d->C; a.c4 = g.c4; a.ldx = d->ldx; a.ldy = d->ldy; a.qt_log2 = g.qt_log2;
    a.flags = d->flags;
    a.ldr = d->ldr; a.res_C = d->res_C; a.res_T = d->res_T; a.res_H = d->res_H; a.res_W = d->res_W;
    a.res_sT = d->res_sT; a.res_sH = d->res_sH; a.res_sW = d->res_sW;
    a.T = d->T; a.H = d->H; a.W = d->W;
    fdiv_make((unsigned)d->W, a.dW);
    fdiv_make((unsigned)d->H, a.dH);
    fdiv_make((unsigned)d->T, a.dT);
    hipLaunchKernelGGL(bn_apply_kernel, dim3((unsigned)g.gx, (unsigned)g.gy), dim3(256), 0, (hipStream_t)stream, a);
    return hip_check(hipGetLastError(), "bn_apply launch");
}
