// Winograd F(2x2, 3x3) around the implicit-GEMM tiles: the three-launch form of a stride-1 (kT,3,3) fp32 convolution.
//
//   V = B^T d B   ptx_wino_in_f32     x [N][T][H][W][ldx]            -> V [N][T][H/2][W/2][16 * Cg]     Cg  = round_up(Ci, 4)
//   M = U . V     ptx_conv3d_fwd      a grouped (kT,1,1) conv, groups = 16 (ptx_conv_wino_f32_gemm_desc): the 16 transform
//                                     positions are the groups, the temporal taps extend K
//   y = A^T m A   ptx_wino_out_f32    M [N][T][H/2][W/2][16 * Cog]   -> y [N][T][H][W][ldy]             Cog = round_up(Co, 4)
//
// 16 multiplies per 2x2 outputs and channel pair instead of 36.  The only device code here is memory bound: the two transforms
// (adds only: B and A hold 0 / +-1) and the one-off filter transform U = G g G^T (factors 1/2 and 1/4, exact scalings).
// Transform position xi = 4 a + b for row a / column b of the 4x4 transformed patch; one lane of the transforms owns four
// consecutive channels of one 2x2-output tile, lanes run along channels: both sides move 16-byte pieces of contiguous rows.
//
// Winograd F(4x4, 3x3) is the same three launches on 6x6 patches (the ptx_*wino4* entry points below): 36 multiplies per 4x4
// outputs and channel pair (2.25 per output against 4), V and M 2.25x the activation instead of 4x, groups = 36, xi = 6 a + b.
// Frames of any extent: H4 x W4 = ceil(H / 4) x ceil(W / 4) tiles, reads outside the frame are zero, stores outside are masked.
//
// Compiled as part of pack_layout.hip's translation unit (see the include at its end).
#include "../../include/ptx_amd_wino4.h"

namespace ptx {

typedef float f32x2 __attribute__((ext_vector_type(2)));


constexpr uint64_t kWinoLimit = 0x80000000ull;      // every buffer of one launch stays below 2 GiB

struct WinoGeom {
    int frames, H, W, H2, W2, Ci, Co, Cg, Cog, ldx, ldy, ldr, kT;
    uint64_t tiles, x_bytes, y_bytes, r_bytes, v_bytes, m_bytes, u_elems;
};

// The eligibility rule, and the extents of everything the three launches touch.  Returns nullptr when `d` is eligible,
// else the reason.  m: outputs per tile edge -- 2 (F(2x2): H and W even) or 4 (F(4x4): any extent, the last tile of a row /
// column may be partial); H2 x W2 is then the tile grid of a frame and a tile has (m + 2)^2 transform positions.
static const char* wino_geom(const ptx_conv3d_desc* d, WinoGeom& g, int m = 2) {
    if (!d) return "null descriptor";
    if (d->N <= 0 || d->Ti <= 0 || d->Hi <= 0 || d->Wi <= 0 || d->Ci <= 0 || d->Co <= 0) return "non-positive extent";
    if (d->flags & ~(PTX_EPI_RELU | PTX_EPI_RES_ADD | PTX_SPLITK_FUSED))
        return "the fp32 path with flags within PTX_EPI_RELU | PTX_EPI_RES_ADD only";
    if (d->kH != 3 || d->kW != 3 || (d->kT != 1 && d->kT != 3)) return "filters (1|3)x3x3 only";
    if (d->sT != 1 || d->sH != 1 || d->sW != 1) return "unit strides only";
    if (d->pT != d->kT / 2 || d->pH != 1 || d->pW != 1) return "padding (kT/2, 1, 1) only";
    if (d->groups > 1) return "dense convolutions only";
    if (m == 2 && ((d->Hi & 1) || (d->Wi & 1))) return "H and W must be even";
    if (d->To != d->Ti || d->Ho != d->Hi || d->Wo != d->Wi) return "output extents must equal the input extents";
    if (d->ldx < d->Ci || d->ldx % 4 || d->ldy < d->Co || d->ldy % 4) return "channel strides must be >= C and multiples of 4";
    if (d->Kc < d->Ci || d->Kc % 4 || d->Co_pad < (d->Co + 3) / 4 * 4) return "packed weight extents do not cover Ci / Co";
    if ((d->flags & PTX_EPI_RES_ADD) && (d->ldr < (d->Co + 3) / 4 * 4 || d->ldr % 4)) return "residual stride does not cover Co";
    g.frames = 0;
    g.H = d->Hi; g.W = d->Wi; g.H2 = (d->Hi + m - 1) / m; g.W2 = (d->Wi + m - 1) / m;
    g.Ci = d->Ci; g.Co = d->Co; g.Cg = (d->Ci + 3) / 4 * 4; g.Cog = (d->Co + 3) / 4 * 4;
    g.ldx = d->ldx; g.ldy = d->ldy; g.ldr = (d->flags & PTX_EPI_RES_ADD) ? d->ldr : 0; g.kT = d->kT;
    const uint64_t frames = (uint64_t)d->N * d->Ti, pos = frames * d->Hi * d->Wi, npos = (uint64_t)(m + 2) * (m + 2);
    g.tiles = frames * g.H2 * g.W2;
    g.x_bytes = pos * d->ldx * 4ull;
    g.y_bytes = pos * d->ldy * 4ull;
    g.r_bytes = pos * g.ldr * 4ull;
    g.v_bytes = g.tiles * npos * g.Cg * 4ull;
    g.m_bytes = g.tiles * npos * g.Cog * 4ull;
    const uint64_t rows = (npos * g.Cog + 127) / 128 * 128;
    g.u_elems = (uint64_t)d->kT * rows * g.Cg;
    if (frames >= kWinoLimit || pos >= kWinoLimit || g.x_bytes >= kWinoLimit || g.y_bytes >= kWinoLimit || g.r_bytes >= kWinoLimit ||
        g.v_bytes >= kWinoLimit || g.m_bytes >= kWinoLimit || g.u_elems * 4ull >= kWinoLimit ||
        (uint64_t)d->kT * 9ull * d->Co_pad * d->Kc * 4ull >= kWinoLimit || npos * g.Cg >= kWinoLimit || rows >= kWinoLimit)
        return "every operand of one launch (x, y, res, V, M, U) must be < 2 GiB; split the batch";
    g.frames = (int)frames;
    return nullptr;
}

// V = B^T d B, B^T = [1 0 -1 0; 0 1 1 0; 0 -1 1 0; 0 1 0 -1], on the 4x4 patch at rows 2i-1..2i+2, columns 2j-1..2j+2.
__global__ void __launch_bounds__(256) wino_in_f32_kernel(const float* __restrict__ x, float* __restrict__ V, WinoGeom g,
                                                          unsigned total) {
    const unsigned idx = blockIdx.x * 256u + threadIdx.x;
    if (idx >= total) return;
    const unsigned cq = (unsigned)g.Cg / 4u;
    const unsigned c = (idx % cq) * 4u;
    const unsigned tile = idx / cq;
    const unsigned tj = tile % (unsigned)g.W2;
    const unsigned r = tile / (unsigned)g.W2;
    const unsigned ti = r % (unsigned)g.H2;
    const unsigned f = r / (unsigned)g.H2;
    const int h0 = 2 * (int)ti - 1, w0 = 2 * (int)tj - 1;
    const float* xf = x + (size_t)f * g.H * g.W * g.ldx + c;
    const bool ragged = c + 4u > (unsigned)g.Ci;          // the last quad of a channel count that is no multiple of 4
    f32x4 d[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int h = h0 + i;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int w = w0 + j;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (h >= 0 && h < g.H && w >= 0 && w < g.W) v = *reinterpret_cast<const f32x4*>(xf + ((size_t)h * g.W + w) * g.ldx);
            if (ragged) {                                 // pad channels are written as zero whatever the row holds there
                if (c + 1u >= (unsigned)g.Ci) v.y = 0.f;
                if (c + 2u >= (unsigned)g.Ci) v.z = 0.f;
                v.w = 0.f;
            }
            d[i][j] = v;
        }
    }
    f32x4 t[4][4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        t[0][j] = d[0][j] - d[2][j];
        t[1][j] = d[1][j] + d[2][j];
        t[2][j] = d[2][j] - d[1][j];
        t[3][j] = d[1][j] - d[3][j];
    }
    float* vt = V + (size_t)tile * 16u * g.Cg + c;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        *reinterpret_cast<f32x4*>(vt + (size_t)(4 * i + 0) * g.Cg) = t[i][0] - t[i][2];
        *reinterpret_cast<f32x4*>(vt + (size_t)(4 * i + 1) * g.Cg) = t[i][1] + t[i][2];
        *reinterpret_cast<f32x4*>(vt + (size_t)(4 * i + 2) * g.Cg) = t[i][2] - t[i][1];
        *reinterpret_cast<f32x4*>(vt + (size_t)(4 * i + 3) * g.Cg) = t[i][1] - t[i][3];
    }
}

// y = A^T m A + bias (+ res) (ReLU), A^T = [1 1 1 0; 0 1 -1 -1]: the 2x2 outputs of one tile.  Columns [Co, round_up(Co, 4))
// of y are written as zero, columns beyond are left untouched (ptx_conv3d_fwd's rule).
__global__ void __launch_bounds__(256) wino_out_f32_kernel(const float* __restrict__ M, const float* __restrict__ bias,
                                                           const float* __restrict__ res, float* __restrict__ y, WinoGeom g,
                                                           unsigned total, int relu) {
    const unsigned idx = blockIdx.x * 256u + threadIdx.x;
    if (idx >= total) return;
    const unsigned cq = (unsigned)g.Cog / 4u;
    const unsigned c = (idx % cq) * 4u;
    const unsigned tile = idx / cq;
    const unsigned tj = tile % (unsigned)g.W2;
    const unsigned r = tile / (unsigned)g.W2;
    const unsigned ti = r % (unsigned)g.H2;
    const unsigned f = r / (unsigned)g.H2;
    const float* mt = M + (size_t)tile * 16u * g.Cog + c;
    f32x4 m[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) m[a][b] = *reinterpret_cast<const f32x4*>(mt + (size_t)(4 * a + b) * g.Cog);
    f32x4 s[2][4];
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        s[0][b] = m[0][b] + m[1][b] + m[2][b];
        s[1][b] = m[1][b] - m[2][b] - m[3][b];
    }
    f32x4 b4 = {0.f, 0.f, 0.f, 0.f};
    if (bias) b4 = *reinterpret_cast<const f32x4*>(bias + c);
    const bool ragged = c + 4u > (unsigned)g.Co;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            f32x4 v = (j == 0 ? s[i][0] + s[i][1] + s[i][2] : s[i][1] - s[i][2] - s[i][3]) + b4;
            const size_t pos = ((size_t)f * g.H + (2u * ti + i)) * g.W + (2u * tj + j);
            if (res) v += *reinterpret_cast<const f32x4*>(res + pos * g.ldr + c);
            if (relu) { v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f); }
            if (ragged) {
                if (c + 1u >= (unsigned)g.Co) v.y = 0.f;
                if (c + 2u >= (unsigned)g.Co) v.z = 0.f;
                v.w = 0.f;
            }
            *reinterpret_cast<f32x4*>(y + pos * g.ldy + c) = v;
        }
    }
}

// U = G g G^T per (co, kt, ci), G = [1 0 0; 1/2 1/2 1/2; 1/2 -1/2 1/2; 0 0 1], from the BN-folded K-major filter
// src [(kt*3 + kh)*3 + kw][Co_pad][Kc] into the grouped layout dst [kt][rows][Cg], row = xi * Cog + co (rows = 16 * Cog rounded up
// to 128); rows of pad channels and the rows past 16 * Cog are written as zero.  One thread per element of dst.
__global__ void __launch_bounds__(256) wino_pack_f32_kernel(const float* __restrict__ src, float* __restrict__ dst, int Co,
                                                            int Cog, int Cg, int rows, int src_rows, int src_kc, unsigned total) {
    const unsigned idx = blockIdx.x * 256u + threadIdx.x;
    if (idx >= total) return;
    const int k = (int)(idx % (unsigned)Cg);
    const unsigned rr = idx / (unsigned)Cg;
    const int row = (int)(rr % (unsigned)rows), kt = (int)(rr / (unsigned)rows);
    const int xi = row / Cog, co = row % Cog;
    float val = 0.f;
    if (xi < 16 && co < Co && k < src_kc) {
        const int a = xi >> 2, b = xi & 3;
        float t[3];
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const size_t tap = (size_t)(kt * 3) * 3 + j;              // (kt, kh = 0, kw = j); kh advances by 3 taps
            const size_t plane = (size_t)src_rows * src_kc;
            const float g0 = src[(tap + 0) * plane + (size_t)co * src_kc + k];
            const float g1 = src[(tap + 3) * plane + (size_t)co * src_kc + k];
            const float g2 = src[(tap + 6) * plane + (size_t)co * src_kc + k];
            t[j] = a == 0 ? g0 : a == 3 ? g2 : a == 1 ? 0.5f * ((g0 + g2) + g1) : 0.5f * ((g0 + g2) - g1);
        }
        val = b == 0 ? t[0] : b == 3 ? t[2] : b == 1 ? 0.5f * ((t[0] + t[2]) + t[1]) : 0.5f * ((t[0] + t[2]) - t[1]);
    }
    dst[idx] = val;
}

// ---------------------------------------------------------------- F(4x4, 3x3)
// One 6-vector through B^T = [4 0 -5 0 1 0; 0 -4 -4 1 1 0; 0 4 -4 -1 1 0; 0 -2 -1 2 1 0; 0 2 -1 -2 1 0; 0 4 0 -5 0 1], in place.
template <typename T>
__device__ __forceinline__ void wino4_bt(T& d0, T& d1, T& d2, T& d3, T& d4, T& d5) {
    const T e = d4 - 4.f * d2, o = d3 - 4.f * d1, p = d4 - d2, q = 2.f * (d3 - d1);
    const T t0 = 4.f * d0 - 5.f * d2 + d4, t5 = 4.f * d1 - 5.f * d3 + d5;
    d0 = t0; d1 = e + o; d2 = e - o; d3 = p + q; d4 = p - q; d5 = t5;
}

// V = B^T d B on the 6x6 patch at rows 4i-1..4i+4, columns 4j-1..4j+4 (zero outside the frame).  One lane owns a channel PAIR
// of one tile: the whole patch stays in registers (72 for the data; a channel quad would need 144), lanes run along channels,
// so a wave still moves contiguous 512-byte pieces of every row on both sides.
__global__ void __launch_bounds__(256) wino4_in_f32_kernel(const float* __restrict__ x, float* __restrict__ V, WinoGeom g,
                                                           unsigned total) {
    const unsigned idx = blockIdx.x * 256u + threadIdx.x;
    if (idx >= total) return;
    const unsigned ch = (unsigned)g.Cg / 2u;
    const unsigned c = (idx % ch) * 2u;
    const unsigned tile = idx / ch;
    const unsigned tj = tile % (unsigned)g.W2;
    const unsigned r = tile / (unsigned)g.W2;
    const unsigned ti = r % (unsigned)g.H2;
    const unsigned f = r / (unsigned)g.H2;
    const int h0 = 4 * (int)ti - 1, w0 = 4 * (int)tj - 1;
    const float* xf = x + (size_t)f * g.H * g.W * g.ldx + c;
    const bool live0 = c < (unsigned)g.Ci, live1 = c + 1u < (unsigned)g.Ci;      // pad channels are written as zero
    f32x2 d[6][6];
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        const int h = h0 + i;
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            const int w = w0 + j;
            f32x2 v = {0.f, 0.f};
            if (h >= 0 && h < g.H && w >= 0 && w < g.W) v = *reinterpret_cast<const f32x2*>(xf + ((size_t)h * g.W + w) * g.ldx);
            if (!live0) v.x = 0.f;
            if (!live1) v.y = 0.f;
            d[i][j] = v;
        }
    }
#pragma unroll
    for (int j = 0; j < 6; ++j) wino4_bt(d[0][j], d[1][j], d[2][j], d[3][j], d[4][j], d[5][j]);
    float* vt = V + (size_t)tile * 36u * g.Cg + c;
#pragma unroll
    for (int a = 0; a < 6; ++a) {
        wino4_bt(d[a][0], d[a][1], d[a][2], d[a][3], d[a][4], d[a][5]);
#pragma unroll
        for (int b = 0; b < 6; ++b) *reinterpret_cast<f32x2*>(vt + (size_t)(6 * a + b) * g.Cg) = d[a][b];
    }
}

// y = A^T m A + bias (+ res) (ReLU), A^T = [1 1 1 1 1 0; 0 1 -1 2 -2 0; 0 1 1 4 4 0; 0 1 -1 8 -8 1]: the 4x4 outputs of one
// tile, rows / columns past the frame masked.  One lane owns four consecutive channels; the rows of m are transformed as they
// arrive and folded into the 16 outputs, so the lane never holds more than one row of m.  Pad columns as wino_out_f32_kernel.
__global__ void __launch_bounds__(256) wino4_out_f32_kernel(const float* __restrict__ M, const float* __restrict__ bias,
                                                            const float* __restrict__ res, float* __restrict__ y, WinoGeom g,
                                                            unsigned total, int relu) {
    const unsigned idx = blockIdx.x * 256u + threadIdx.x;
    if (idx >= total) return;
    const unsigned cq = (unsigned)g.Cog / 4u;
    const unsigned c = (idx % cq) * 4u;
    const unsigned tile = idx / cq;
    const unsigned tj = tile % (unsigned)g.W2;
    const unsigned r = tile / (unsigned)g.W2;
    const unsigned ti = r % (unsigned)g.H2;
    const unsigned f = r / (unsigned)g.H2;
    const float* mt = M + (size_t)tile * 36u * g.Cog + c;
    f32x4 o[4][4];
#pragma unroll
    for (int a = 0; a < 6; ++a) {
        f32x4 m[6];
#pragma unroll
        for (int b = 0; b < 6; ++b) m[b] = *reinterpret_cast<const f32x4*>(mt + (size_t)(6 * a + b) * g.Cog);
        const f32x4 p12 = m[1] + m[2], q12 = m[1] - m[2], p34 = m[3] + m[4], q34 = m[3] - m[4];
        f32x4 s[4];
        s[0] = m[0] + p12 + p34;
        s[1] = q12 + 2.f * q34;
        s[2] = p12 + 4.f * p34;
        s[3] = q12 + 8.f * q34 + m[5];
        // column a of A^T: (1 0 0 0), (1 1 1 1), (1 -1 1 -1), (1 2 4 8), (1 -2 4 -8), (0 0 0 1)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (a == 0) { o[0][j] = s[j]; }
            else if (a == 1) { o[0][j] += s[j]; o[1][j] = s[j]; o[2][j] = s[j]; o[3][j] = s[j]; }
            else if (a == 2) { o[0][j] += s[j]; o[1][j] -= s[j]; o[2][j] += s[j]; o[3][j] -= s[j]; }
            else if (a == 3) { o[0][j] += s[j]; o[1][j] += 2.f * s[j]; o[2][j] += 4.f * s[j]; o[3][j] += 8.f * s[j]; }
            else if (a == 4) { o[0][j] += s[j]; o[1][j] -= 2.f * s[j]; o[2][j] += 4.f * s[j]; o[3][j] -= 8.f * s[j]; }
            else { o[3][j] += s[j]; }
        }
    }
    f32x4 b4 = {0.f, 0.f, 0.f, 0.f};
    if (bias) b4 = *reinterpret_cast<const f32x4*>(bias + c);
    const bool ragged = c + 4u > (unsigned)g.Co;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const unsigned h = 4u * ti + i;
        if (h >= (unsigned)g.H) continue;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const unsigned w = 4u * tj + j;
            if (w >= (unsigned)g.W) continue;
            f32x4 v = o[i][j] + b4;
            const size_t pos = ((size_t)f * g.H + h) * g.W + w;
            if (res) v += *reinterpret_cast<const f32x4*>(res + pos * g.ldr + c);
            if (relu) { v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f); }
            if (ragged) {
                if (c + 1u >= (unsigned)g.Co) v.y = 0.f;
                if (c + 2u >= (unsigned)g.Co) v.z = 0.f;
                v.w = 0.f;
            }
            *reinterpret_cast<f32x4*>(y + pos * g.ldy + c) = v;
        }
    }
}

// Row a of G g for G = [1/4 0 0; -1/6 -1/6 -1/6; -1/6 1/6 -1/6; 1/24 1/12 1/6; 1/24 -1/12 1/6; 0 0 1].
__device__ __forceinline__ float wino4_g(int a, float g0, float g1, float g2) {
    switch (a) {
        case 0: return 0.25f * g0;
        case 1: return (-1.f / 6.f) * ((g0 + g2) + g1);
        case 2: return (-1.f / 6.f) * ((g0 + g2) - g1);
        case 3: return ((1.f / 24.f) * g0 + (1.f / 6.f) * g2) + (1.f / 12.f) * g1;
        case 4: return ((1.f / 24.f) * g0 + (1.f / 6.f) * g2) - (1.f / 12.f) * g1;
        default: return g2;
    }
}

// U = G g G^T per (co, kt, ci) from the BN-folded K-major filter src [(kt*3 + kh)*3 + kw][Co_pad][Kc] into the grouped layout
// dst [kt][rows][Cg], row = xi * Cog + co, xi = 6 a + b (rows = 36 * Cog rounded up to 128); rows of pad channels and the rows
// past 36 * Cog are written as zero.  One thread per element of dst.
__global__ void __launch_bounds__(256) wino4_pack_f32_kernel(const float* __restrict__ src, float* __restrict__ dst, int Co,
                                                             int Cog, int Cg, int rows, int src_rows, int src_kc, unsigned total) {
    const unsigned idx = blockIdx.x * 256u + threadIdx.x;
    if (idx >= total) return;
    const int k = (int)(idx % (unsigned)Cg);
    const unsigned rr = idx / (unsigned)Cg;
    const int row = (int)(rr % (unsigned)rows), kt = (int)(rr / (unsigned)rows);
    const int xi = row / Cog, co = row % Cog;
    float val = 0.f;
    if (xi < 36 && co < Co && k < src_kc) {
        const int a = xi / 6, b = xi % 6;
        float t[3];
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const size_t tap = (size_t)(kt * 3) * 3 + j;              // (kt, kh = 0, kw = j); kh advances by 3 taps
            const size_t plane = (size_t)src_rows * src_kc;
            const float g0 = src[(tap + 0) * plane + (size_t)co * src_kc + k];
            const float g1 = src[(tap + 3) * plane + (size_t)co * src_kc + k];
            const float g2 = src[(tap + 6) * plane + (size_t)co * src_kc + k];
            t[j] = wino4_g(a, g0, g1, g2);
        }
        val = wino4_g(b, t[0], t[1], t[2]);
    }
    dst[idx] = val;
}

}  // namespace ptx

extern "C" int ptx_conv_wino_f32_supported(const ptx_conv3d_desc* desc) {
    ptx::WinoGeom g;
    const char* why = ptx::wino_geom(desc, g);
    if (why) { ptx::fail(PTX_ERR_UNSUPPORTED, "conv_wino_f32: %s", why); return 0; }
    return 1;
}

extern "C" size_t ptx_conv_wino_f32_workspace_bytes(const ptx_conv3d_desc* desc) {
    ptx::WinoGeom g;
    if (ptx::wino_geom(desc, g)) return 0;
    return (size_t)((g.v_bytes + 255) / 256 * 256 + g.m_bytes);
}

extern "C" size_t ptx_wino_f32_weight_elems(const ptx_conv3d_desc* desc) {
    ptx::WinoGeom g;
    if (ptx::wino_geom(desc, g)) return 0;
    return (size_t)g.u_elems;
}

extern "C" int ptx_conv_wino_f32_gemm_desc(const ptx_conv3d_desc* desc, ptx_conv3d_desc* gemm) {
    ptx::WinoGeom g;
    const char* why = ptx::wino_geom(desc, g);
    if (why) return ptx::fail(PTX_ERR_UNSUPPORTED, "conv_wino_f32: %s", why);
    if (!gemm) return ptx::fail(PTX_ERR_INVALID, "conv_wino_f32: null descriptor");
    ptx_conv3d_desc o = {};
    o.N = desc->N; o.Ti = o.To = desc->Ti; o.Hi = o.Ho = g.H2; o.Wi = o.Wo = g.W2;
    o.Ci = o.ldx = 16 * g.Cg; o.Co = o.ldy = 16 * g.Cog;
    o.kT = g.kT; o.kH = o.kW = 1; o.sT = o.sH = o.sW = 1; o.pT = g.kT / 2;
    o.Kc = g.Cg; o.Co_pad = (16 * g.Cog + 127) / 128 * 128;
    o.groups = 16;
    *gemm = o;
    return PTX_OK;
}

extern "C" int ptx_pack_wino_f32_weight(const ptx_conv3d_desc* desc, const float* w_packed, float* w_wino, ptx_stream_t stream) {
    ptx::WinoGeom g;
    const char* why = ptx::wino_geom(desc, g);
    if (why) return ptx::fail(PTX_ERR_UNSUPPORTED, "pack_wino_f32: %s", why);
    if (!w_packed || !w_wino) return ptx::fail(PTX_ERR_INVALID, "pack_wino_f32: null pointer");
    const unsigned total = (unsigned)g.u_elems;
    const int rows = (16 * g.Cog + 127) / 128 * 128;
    hipLaunchKernelGGL(ptx::wino_pack_f32_kernel, dim3((total + 255u) / 256u), dim3(256), 0, (hipStream_t)stream, w_packed, w_wino,
                       g.Co, g.Cog, g.Cg, rows, desc->Co_pad, desc->Kc, total);
    return ptx::hip_check(hipGetLastError(), "pack_wino_f32 launch");
}

extern "C" int ptx_wino_in_f32(const ptx_conv3d_desc* desc, const float* x, float* V, ptx_stream_t stream) {
    ptx::WinoGeom g;
    const char* why = ptx::wino_geom(desc, g);
    if (why) return ptx::fail(PTX_ERR_UNSUPPORTED, "wino_in_f32: %s", why);
    if (!x || !V) return ptx::fail(PTX_ERR_INVALID, "wino_in_f32: null pointer");
    if (((uintptr_t)x | (uintptr_t)V) & 15) return ptx::fail(PTX_ERR_INVALID, "wino_in_f32: pointers must be 16-byte aligned");
    const unsigned total = (unsigned)(g.tiles * (unsigned)(g.Cg / 4));       // V < 2 GiB: at most 2^23 lanes
    hipLaunchKernelGGL(ptx::wino_in_f32_kernel, dim3((total + 255u) / 256u), dim3(256), 0, (hipStream_t)stream, x, V, g, total);
    return ptx::hip_check(hipGetLastError(), "wino_in_f32 launch");
}

extern "C" int ptx_wino_out_f32(const ptx_conv3d_desc* desc, const float* M, const float* bias, const float* res, float* y,
                                ptx_stream_t stream) {
    ptx::WinoGeom g;
    const char* why = ptx::wino_geom(desc, g);
    if (why) return ptx::fail(PTX_ERR_UNSUPPORTED, "wino_out_f32: %s", why);
    if (!M || !y) return ptx::fail(PTX_ERR_INVALID, "wino_out_f32: null pointer");
    if ((desc->flags & PTX_EPI_RES_ADD) && !res) return ptx::fail(PTX_ERR_INVALID, "wino_out_f32: residual flag set but res == NULL");
    if (((uintptr_t)M | (uintptr_t)y | (uintptr_t)bias | (uintptr_t)res) & 15)
        return ptx::fail(PTX_ERR_INVALID, "wino_out_f32: pointers must be 16-byte aligned");
    const unsigned total = (unsigned)(g.tiles * (unsigned)(g.Cog / 4));
    hipLaunchKernelGGL(ptx::wino_out_f32_kernel, dim3((total + 255u) / 256u), dim3(256), 0, (hipStream_t)stream, M, bias,
                       (desc->flags & PTX_EPI_RES_ADD) ? res : nullptr, y, g, total, (desc->flags & PTX_EPI_RELU) ? 1 : 0);
    return ptx::hip_check(hipGetLastError(), "wino_out_f32 launch");
}

extern "C" int ptx_conv_wino4_f32_supported(const ptx_conv3d_desc* desc) {
    ptx::WinoGeom g;
    const char* why = ptx::wino_geom(desc, g, 4);
    if (why) { ptx::fail(PTX_ERR_UNSUPPORTED, "conv_wino4_f32: %s", why); return 0; }
    return 1;
}

extern "C" size_t ptx_conv_wino4_f32_workspace_bytes(const ptx_conv3d_desc* desc) {
    ptx::WinoGeom g;
    if (ptx::wino_geom(desc, g, 4)) return 0;
    return (size_t)((g.v_bytes + 255) / 256 * 256 + g.m_bytes);
}

extern "C" size_t ptx_wino4_f32_weight_elems(const ptx_conv3d_desc* desc) {
    ptx::WinoGeom g;
    if (ptx::wino_geom(desc, g, 4)) return 0;
    return (size_t)g.u_elems;
}

extern "C" int ptx_conv_wino4_f32_gemm_desc(const ptx_conv3d_desc* desc, ptx_conv3d_desc* gemm) {
    ptx::WinoGeom g;
    const char* why = ptx::wino_geom(desc, g, 4);
    if (why) return ptx::fail(PTX_ERR_UNSUPPORTED, "conv_wino4_f32: %s", why);
    if (!gemm) return ptx::fail(PTX_ERR_INVALID, "conv_wino4_f32: null descriptor");
    ptx_conv3d_desc o = {};
    o.N = desc->N; o.Ti = o.To = desc->Ti; o.Hi = o.Ho = g.H2; o.Wi = o.Wo = g.W2;
    o.Ci = o.ldx = 36 * g.Cg; o.Co = o.ldy = 36 * g.Cog;
    o.kT = g.kT; o.kH = o.kW = 1; o.sT = o.sH = o.sW = 1; o.pT = g.kT / 2;
    o.Kc = g.Cg; o.Co_pad = (36 * g.Cog + 127) / 128 * 128;
    o.groups = 36;
    *gemm = o;
    return PTX_OK;
}

extern "C" int ptx_pack_wino4_f32_weight(const ptx_conv3d_desc* desc, const float* w_packed, float* w_wino, ptx_stream_t stream) {
    ptx::WinoGeom g;
    const char* why = ptx::wino_geom(desc, g, 4);
    if (why) return ptx::fail(PTX_ERR_UNSUPPORTED, "pack_wino4_f32: %s", why);
    if (!w_packed || !w_wino) return ptx::fail(PTX_ERR_INVALID, "pack_wino4_f32: null pointer");
    const unsigned total = (unsigned)g.u_elems;
    const int rows = (36 * g.Cog + 127) / 128 * 128;
    hipLaunchKernelGGL(ptx::wino4_pack_f32_kernel, dim3((total + 255u) / 256u), dim3(256), 0, (hipStream_t)stream, w_packed, w_wino,
                       g.Co, g.Cog, g.Cg, rows, desc->Co_pad, desc->Kc, total);
    return ptx::hip_check(hipGetLastError(), "pack_wino4_f32 launch");
}

extern "C" int ptx_wino4_in_f32(const ptx_conv3d_desc* desc, const float* x, float* V, ptx_stream_t stream) {
    ptx::WinoGeom g;
    const char* why = ptx::wino_geom(desc, g, 4);
    if (why) return ptx::fail(PTX_ERR_UNSUPPORTED, "wino4_in_f32: %s", why);
    if (!x || !V) return ptx::fail(PTX_ERR_INVALID, "wino4_in_f32: null pointer");
    if (((uintptr_t)x | (uintptr_t)V) & 15) return ptx::fail(PTX_ERR_INVALID, "wino4_in_f32: pointers must be 16-byte aligned");
    const unsigned total = (unsigned)(g.tiles * (unsigned)(g.Cg / 2));       // V < 2 GiB: fewer than 2^23 lanes
    hipLaunchKernelGGL(ptx::wino4_in_f32_kernel, dim3((total + 255u) / 256u), dim3(256), 0, (hipStream_t)stream, x, V, g, total);
    return ptx::hip_check(hipGetLastError(), "wino4_in_f32 launch");
}

extern "C" int ptx_wino4_out_f32(const ptx_conv3d_desc* desc, const float* M, const float* bias, const float* res, float* y,
                                 ptx_stream_t stream) {
    ptx::WinoGeom g;
    const char* why = ptx::wino_geom(desc, g, 4);
    if (why) return ptx::fail(PTX_ERR_UNSUPPORTED, "wino4_out_f32: %s", why);
    if (!M || !y) return ptx::fail(PTX_ERR_INVALID, "wino4_out_f32: null pointer");
    if ((desc->flags & PTX_EPI_RES_ADD) && !res) return ptx::fail(PTX_ERR_INVALID, "wino4_out_f32: residual flag set but res == NULL");
    if (((uintptr_t)M | (uintptr_t)y | (uintptr_t)bias | (uintptr_t)res) & 15)
        return ptx::fail(PTX_ERR_INVALID, "wino4_out_f32: pointers must be 16-byte aligned");
    const unsigned total = (unsigned)(g.tiles * (unsigned)(g.Cog / 4));
    hipLaunchKernelGGL(ptx::wino4_out_f32_kernel, dim3((total + 255u) / 256u), dim3(256), 0, (hipStream_t)stream, M, bias,
                       (desc->flags & PTX_EPI_RES_ADD) ? res : nullptr, y, g, total, (desc->flags & PTX_EPI_RELU) ? 1 : 0);
    return ptx::hip_check(hipGetLastError(), "wino4_out_f32 launch");
}
