// The fp32 RGB stem (Conv3d(3, Co, 7, stride (1,s,s), pad 3) + BN + ReLU) as a fast FIR along time: fewer frame-convolutions
// than conv_stem_f32.hip issues, on the same patch-resident step loop.
//
// The stem's temporal stride is 1 and it has 7 temporal taps, so along time it is a 7-tap FIR.  A Toom-Cook form F(m, 7)
// computes m output frames from P < 7 m products, each a 2-D kH x 7 convolution of a linear combination of input frames with
// a linear combination of filter taps (include/ptx_amd_tfir.h has the bilinear form; scripts/gen_tfir_tables.py derives the
// tables below from rational Vandermonde matrices):
//     direct, after its end-of-clip pruning   100 frame-convolutions per 16-frame clip
//     scheme 1  F(2,7)                         64
//     scheme 2  F(4,4) + F(4,3) on split taps  52
//     scheme 3  F(4,7)                         40
// Three kernels:
//   tfir_pack_kernel   U[j] = sum_k G[j][k] w_stem[kt = k] over the packed stem filter, once per filter;
//   tfir_in_kernel     V[n][c][g P + j] = sum_i BT[j][i] x[n][c][g m - pT + i]: one lane is a float4 of a row, reads its m + 6
//                      frames once (zero outside the clip) and writes P combinations.  V is a plain NCDHW tensor whose frames
//                      are the (group, product) pairs;
//   conv_stem_tfir_f32_kernel   the direct stem's step loop (conv_stem_f32.hip: patch of a "frame" LDS-DMA'd once, kH steps of
//                      11 v_mfma_f32_32x32x2_f32 per row tile on it, three filter slots) with three changes: "temporal tap kt
//                      of frame to" is "product j of group g" (no pruning: every group runs all P products); at each product
//                      change, where the patch is re-staged anyway, the product's accumulator tile is folded into the m output
//                      accumulators with VALU FMAs (Y[o] += AT[o][j] M, zero coefficients skipped, while the next patch's DMA
//                      is in flight); the epilogue runs per output frame, frames past To masked.
// Register budget: the product tile + m output tiles.  At the direct kernel's 64 rows per wave that is 64 + 64 m accumulators
// (one wave per SIMD for either m); a wave therefore owns 32 rows (32 + 32 m accumulators: 153 VGPRs and three workgroups per
// CU for m = 2, 217 and two for m = 4, no scratch) and a workgroup 128 outputs, whose smaller patch keeps LDS under 48 KB.
// Arithmetic: fp32 throughout.
#include "ptx_common.h"
#include "../../include/ptx_amd_tfir.h"
#include <algorithm>

namespace ptx {

constexpr int kTfirKT = 7;                          // temporal taps
constexpr int kTfirMaxM = 4, kTfirMaxP = 13, kTfirMaxWin = kTfirMaxM + kTfirKT - 1;
constexpr int kTfirNT = 256;                        // 4 waves
constexpr int kTfirBN = 64;                         // output channels per workgroup
constexpr int kTfirPatchMax = 12288;                // floats of the patch buffer: 48 KiB
constexpr int kTfirK2 = 11;                         // MFMAs per (product, kh) step and accumulator tile
constexpr int kTfirBTile = kTfirK2 * 2 * kTfirBN;   // floats of one (step, channel tile) filter block: 5.5 KiB

// ---- scheme tables (scripts/gen_tfir_tables.py) ----
// scheme 1: m = 2, P = 8
static const float kAT1[] = {
    1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 0.f,
    0.f, 1.f, -1.f, 2.f, -2.f, 1.f / 2.f, -1.f / 2.f, 1.f};
static const float kG1[] = {
    1.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f,
    1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f,
    1.f, -1.f, 1.f, -1.f, 1.f, -1.f, 1.f,
    1.f, 2.f, 4.f, 8.f, 16.f, 32.f, 64.f,
    1.f, -2.f, 4.f, -8.f, 16.f, -32.f, 64.f,
    1.f, 1.f / 2.f, 1.f / 4.f, 1.f / 8.f, 1.f / 16.f, 1.f / 32.f, 1.f / 64.f,
    1.f, -1.f / 2.f, 1.f / 4.f, -1.f / 8.f, 1.f / 16.f, -1.f / 32.f, 1.f / 64.f,
    0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 1.f};
static const float kBT1[] = {
    1.f, 0.f, -21.f / 4.f, 0.f, 21.f / 4.f, 0.f, -1.f, 0.f,
    0.f, -2.f / 9.f, -2.f / 9.f, 17.f / 18.f, 17.f / 18.f, -2.f / 9.f, -2.f / 9.f, 0.f,
    0.f, 2.f / 9.f, -2.f / 9.f, -17.f / 18.f, 17.f / 18.f, 2.f / 9.f, -2.f / 9.f, 0.f,
    0.f, 1.f / 180.f, 1.f / 360.f, -1.f / 36.f, -1.f / 72.f, 1.f / 45.f, 1.f / 90.f, 0.f,
    0.f, -1.f / 180.f, 1.f / 360.f, 1.f / 36.f, -1.f / 72.f, -1.f / 45.f, 1.f / 90.f, 0.f,
    0.f, 64.f / 45.f, 128.f / 45.f, -16.f / 9.f, -32.f / 9.f, 16.f / 45.f, 32.f / 45.f, 0.f,
    0.f, -64.f / 45.f, 128.f / 45.f, 16.f / 9.f, -32.f / 9.f, -16.f / 45.f, 32.f / 45.f, 0.f,
    0.f, -1.f, 0.f, 21.f / 4.f, 0.f, -21.f / 4.f, 0.f, 1.f};
// scheme 2: m = 4, P = 13
static const float kAT2[] = {
    1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 0.f, 1.f, 1.f, 1.f, 1.f, 1.f, 0.f,
    0.f, 1.f, -1.f, 2.f, -2.f, 1.f / 2.f, 0.f, 0.f, 1.f, -1.f, 2.f, -2.f, 0.f,
    0.f, 1.f, 1.f, 4.f, 4.f, 1.f / 4.f, 0.f, 0.f, 1.f, 1.f, 4.f, 4.f, 0.f,
    0.f, 1.f, -1.f, 8.f, -8.f, 1.f / 8.f, 1.f, 0.f, 1.f, -1.f, 8.f, -8.f, 1.f};
static const float kG2[] = {
    1.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f,
    1.f, 1.f, 1.f, 1.f, 0.f, 0.f, 0.f,
    1.f, -1.f, 1.f, -1.f, 0.f, 0.f, 0.f,
    1.f, 2.f, 4.f, 8.f, 0.f, 0.f, 0.f,
    1.f, -2.f, 4.f, -8.f, 0.f, 0.f, 0.f,
    1.f, 1.f / 2.f, 1.f / 4.f, 1.f / 8.f, 0.f, 0.f, 0.f,
    0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f,
    0.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f,
    0.f, 0.f, 0.f, 0.f, 1.f, 1.f, 1.f,
    0.f, 0.f, 0.f, 0.f, 1.f, -1.f, 1.f,
    0.f, 0.f, 0.f, 0.f, 1.f, 2.f, 4.f,
    0.f, 0.f, 0.f, 0.f, 1.f, -2.f, 4.f,
    0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 1.f};
static const float kBT2[] = {
    1.f, -2.f, -5.f / 4.f, 5.f / 2.f, 1.f / 4.f, -1.f / 2.f, 0.f, 0.f, 0.f, 0.f,
    0.f, -2.f / 3.f, 2.f / 3.f, 3.f / 2.f, -1.f / 6.f, -1.f / 3.f, 0.f, 0.f, 0.f, 0.f,
    0.f, -2.f / 9.f, 2.f / 3.f, -7.f / 18.f, -1.f / 6.f, 1.f / 9.f, 0.f, 0.f, 0.f, 0.f,
    0.f, 1.f / 36.f, -1.f / 24.f, -1.f / 18.f, 1.f / 24.f, 1.f / 36.f, 0.f, 0.f, 0.f, 0.f,
    0.f, 1.f / 60.f, -1.f / 24.f, 0.f, 1.f / 24.f, -1.f / 60.f, 0.f, 0.f, 0.f, 0.f,
    0.f, 128.f / 45.f, 0.f, -32.f / 9.f, 0.f, 32.f / 45.f, 0.f, 0.f, 0.f, 0.f,
    0.f, -2.f, 4.f, 5.f / 2.f, -5.f, -1.f / 2.f, 1.f, 0.f, 0.f, 0.f,
    0.f, 0.f, 0.f, 0.f, 1.f, 0.f, -5.f / 4.f, 0.f, 1.f / 4.f, 0.f,
    0.f, 0.f, 0.f, 0.f, 0.f, 2.f / 3.f, 2.f / 3.f, -1.f / 6.f, -1.f / 6.f, 0.f,
    0.f, 0.f, 0.f, 0.f, 0.f, -2.f / 3.f, 2.f / 3.f, 1.f / 6.f, -1.f / 6.f, 0.f,
    0.f, 0.f, 0.f, 0.f, 0.f, -1.f / 12.f, -1.f / 24.f, 1.f / 12.f, 1.f / 24.f, 0.f,
    0.f, 0.f, 0.f, 0.f, 0.f, 1.f / 12.f, -1.f / 24.f, -1.f / 12.f, 1.f / 24.f, 0.f,
    0.f, 0.f, 0.f, 0.f, 0.f, 4.f, 0.f, -5.f, 0.f, 1.f};
// scheme 3: m = 4, P = 10
static const float kAT3[] = {
    1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 0.f,
    0.f, 1.f, -1.f, 2.f, -2.f, 1.f / 2.f, -1.f / 2.f, 4.f, 1.f / 4.f, 0.f,
    0.f, 1.f, 1.f, 4.f, 4.f, 1.f / 4.f, 1.f / 4.f, 16.f, 1.f / 16.f, 0.f,
    0.f, 1.f, -1.f, 8.f, -8.f, 1.f / 8.f, -1.f / 8.f, 64.f, 1.f / 64.f, 1.f};
static const float kG3[] = {
    1.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f,
    1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f,
    1.f, -1.f, 1.f, -1.f, 1.f, -1.f, 1.f,
    1.f, 2.f, 4.f, 8.f, 16.f, 32.f, 64.f,
    1.f, -2.f, 4.f, -8.f, 16.f, -32.f, 64.f,
    1.f, 1.f / 2.f, 1.f / 4.f, 1.f / 8.f, 1.f / 16.f, 1.f / 32.f, 1.f / 64.f,
    1.f, -1.f / 2.f, 1.f / 4.f, -1.f / 8.f, 1.f / 16.f, -1.f / 32.f, 1.f / 64.f,
    1.f, 4.f, 16.f, 64.f, 256.f, 1024.f, 4096.f,
    1.f, 1.f / 4.f, 1.f / 16.f, 1.f / 64.f, 1.f / 256.f, 1.f / 1024.f, 1.f / 4096.f,
    0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 1.f};
static const float kBT3[] = {
    1.f, -17.f / 4.f, -17.f / 4.f, 357.f / 16.f, 0.f, -357.f / 16.f, 17.f / 4.f, 17.f / 4.f, -1.f, 0.f,
    0.f, 8.f / 81.f, -26.f / 81.f, -20.f / 27.f, 79.f / 54.f, 79.f / 54.f, -20.f / 27.f, -26.f / 81.f, 8.f / 81.f, 0.f,
    0.f, 8.f / 225.f, -14.f / 75.f, 8.f / 225.f, 341.f / 450.f, -341.f / 450.f, -8.f / 225.f, 14.f / 75.f, -8.f / 225.f, 0.f,
    0.f, -1.f / 630.f, 1.f / 168.f, 7.f / 720.f, -11.f / 360.f, -11.f / 720.f, 1.f / 36.f, 1.f / 140.f, -1.f / 315.f, 0.f,
    0.f, -1.f / 2430.f, 19.f / 9720.f, 1.f / 1296.f, -31.f / 3240.f, 31.f / 6480.f, 11.f / 1620.f, -5.f / 972.f, 1.f / 1215.f, 0.f,
    0.f, -512.f / 315.f, 128.f / 35.f, 128.f / 9.f, -352.f / 45.f, -704.f / 45.f, 224.f / 45.f, 64.f / 21.f, -256.f / 315.f, 0.f,
    0.f, -512.f / 1215.f, 640.f / 243.f, -1408.f / 405.f, -992.f / 405.f, 1984.f / 405.f, -32.f / 81.f, -1216.f / 1215.f, 256.f / 1215.f, 0.f,
    0.f, 1.f / 170100.f, -1.f / 42525.f, -1.f / 32400.f, 1.f / 8100.f, 1.f / 32400.f, -1.f / 8100.f, -1.f / 170100.f, 1.f / 42525.f, 0.f,
    0.f, 262144.f / 42525.f, -65536.f / 42525.f, -65536.f / 2025.f, 16384.f / 2025.f, 65536.f / 2025.f, -16384.f / 2025.f, -262144.f / 42525.f, 65536.f / 42525.f, 0.f,
    0.f, -1.f, 17.f / 4.f, 17.f / 4.f, -357.f / 16.f, 0.f, 357.f / 16.f, -17.f / 4.f, -17.f / 4.f, 1.f};

struct TfirScheme {
    int m, P;
    const float *AT, *G, *BT;      // [m][P], [P][7], [P][m + 6]
};
static const TfirScheme kSchemes[3] = {{2, 8, kAT1, kG1, kBT1}, {4, 13, kAT2, kG2, kBT2}, {4, 10, kAT3, kG3, kBT3}};
static_assert(sizeof(kAT2) == 4 * 13 * sizeof(float) && sizeof(kG2) == 13 * 7 * sizeof(float) && sizeof(kBT2) == 13 * 10 * sizeof(float), "");
static_assert(sizeof(kAT1) == 2 * 8 * sizeof(float) && sizeof(kBT1) == 8 * 8 * sizeof(float) && sizeof(kBT3) == 10 * 10 * sizeof(float), "");

static const TfirScheme* tfir_scheme(int id) { return id >= 1 && id <= 3 ? &kSchemes[id - 1] : nullptr; }

__device__ __forceinline__ unsigned tfir_fdiv(unsigned n, const unsigned (&dv)[2]) {
    return dv[0] ? (__umulhi(n, dv[0]) >> dv[1]) : n;
}
static inline void tfir_fdiv_make(unsigned d, unsigned (&out)[2]) {
    if (d <= 1) { out[0] = 0; out[1] = 0; return; }
    unsigned l = 0;
    while ((1ull << l) < d) ++l;
    out[0] = (unsigned)(((1ull << (31 + l)) + d - 1) / d);
    out[1] = l - 1;
}

// ---------------------------------------------------------------------------------------------------------------------
// filter: U[j] = sum_k G[j][k] w[k] over blocks of `inner` floats (one temporal tap of the packed stem filter)
// ---------------------------------------------------------------------------------------------------------------------
struct TfirCoefG { float g[kTfirMaxP][kTfirKT]; };

__global__ void __launch_bounds__(256) tfir_pack_kernel(const float* __restrict__ w, float* __restrict__ u, int inner, int P,
                                                        const TfirCoefG c) {
    for (int r = blockIdx.x * 256 + threadIdx.x; r < inner; r += gridDim.x * 256) {
        float wk[kTfirKT];
#pragma unroll
        for (int k = 0; k < kTfirKT; ++k) wk[k] = w[(size_t)k * inner + r];
        for (int j = 0; j < P; ++j) {
            float s = 0.f;
#pragma unroll
            for (int k = 0; k < kTfirKT; ++k) s = fmaf(c.g[j][k], wk[k], s);
            u[(size_t)j * inner + r] = s;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// temporal input transform
// ---------------------------------------------------------------------------------------------------------------------
struct TfirInArgs {
    const float* x;
    float* v;
    int Ti, Hi, pitch4, G, P, pT;
    long long sn, sc, st;             // strides of x, floats
    long long total;                  // lanes: N * 3 * G * Hi * pitch4
    float bt[kTfirMaxP][kTfirMaxWin];
};

// one lane: the float4 (h, w4) of channel c of sample n, group g -- w4 fastest, so a wave reads and writes whole rows
template <int M>
__global__ void __launch_bounds__(256) tfir_in_kernel(const TfirInArgs p) {
    constexpr int WIN = M + kTfirKT - 1;
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= p.total) return;
    const int w4 = (int)(idx % p.pitch4);
    long long r = idx / p.pitch4;
    const int h = (int)(r % p.Hi);
    r /= p.Hi;
    const int g = (int)(r % p.G);
    r /= p.G;
    const int c = (int)(r % 3), n = (int)(r / 3);
    const long long row = (long long)h * p.pitch4 * 4 + w4 * 4;
    const float* xs = p.x + n * p.sn + c * p.sc + row;
    f32x4 xin[WIN];
#pragma unroll
    for (int i = 0; i < WIN; ++i) {
        const int t = g * M - p.pT + i;
        xin[i] = (unsigned)t < (unsigned)p.Ti ? *reinterpret_cast<const f32x4*>(xs + t * p.st) : f32x4{0.f, 0.f, 0.f, 0.f};
    }
    const long long frame = (long long)p.Hi * p.pitch4 * 4;
    float* vs = p.v + (((long long)n * 3 + c) * ((long long)p.G * p.P) + (long long)g * p.P) * frame + row;
    for (int j = 0; j < p.P; ++j) {
        f32x4 s = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int i = 0; i < WIN; ++i) {
            const float b = p.bt[j][i];                   // uniform: a zero coefficient costs a scalar branch
            if (b != 0.f) {
                s.x = fmaf(b, xin[i].x, s.x);
                s.y = fmaf(b, xin[i].y, s.y);
                s.z = fmaf(b, xin[i].z, s.z);
                s.w = fmaf(b, xin[i].w, s.w);
            }
        }
        *reinterpret_cast<f32x4*>(vs + j * frame) = s;
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// forward
// ---------------------------------------------------------------------------------------------------------------------
struct TfirArgs {
    const float* v;       // [N][3][G * P][Hi][pitch]
    const float* w;       // [P * kH][w_tiles][11][2][64]
    const float* bias;
    float* y;             // [N][To][Ho][Wo][ldy]
    int N, Hi, Wi, To, Ho, Wo, ldy, ncol;
    int pitch;            // floats per input row
    int kH, sH, sW, pH;
    int sn, sc, st;       // sample / channel / frame strides of V
    int P, G;             // products per group, groups per clip
    int PR, PC, plane;    // patch rows, floats per patch row (multiple of 4), PR * PC
    int shift, wbase;     // patch column 0 is input column wbase (<= 0, multiple of 4); a window starts at wo*sW + shift
    int tiles_per_frame, n_tiles, n_pieces, w_tiles;
    unsigned flags;
    unsigned v_bytes, w_bytes, y_bytes;
    unsigned dv_wo[2];
    unsigned dv_plane4[2], dv_pc4[2];     // fast division by plane / 4 and PC / 4 (the prologue's patch-piece decode)
    float at[kTfirMaxM][kTfirMaxP];
};

// the whole patch of "frame" F of V, global -> LDS: piece q = tid + 256 i lands at As + 16 q; lanes past the patch stay out of
// the DMA (nothing is written for them), pieces outside the image read as zero
#define PTX_TFIR_DMA_PATCH(F)                                                                                          \
    do {                                                                                                               \
        const unsigned fbase_ = (unsigned)(n * p.sn + (F) * p.st) * 4u;                                                \
        _Pragma("unroll") for (int i_ = 0; i_ < NP; ++i_)                                                              \
            if (tid + kTfirNT * i_ < p.n_pieces)                                                                       \
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_v, (lds_ptr_t)(As + (wave * 64 + kTfirNT * i_) * 4), 16,  \
                                                         a_src[i_] == kOOB ? kOOB : a_src[i_] + fbase_, 0, 0, 0);      \
    } while (0)

// M: output frames per group.  RT: 32-row tiles per wave (2 = the direct kernel's 64 rows, 1 = 32 rows and a 128-output
// workgroup).  NP: 16-byte patch pieces per thread (8 or 12).
template <int M, int RT, int NP>
__global__ void __launch_bounds__(kTfirNT, (RT * (M + 1) >= 6 ? 1 : 2)) conv_stem_tfir_f32_kernel(const TfirArgs p) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int kRows = 4 * 32 * RT;                  // outputs per workgroup
    float* As = smem;                                   // [3 * plane]: the patch of the current product
    float* Bs = smem + 3 * p.plane;                     // [3][kTfirBTile]: filter tiles of steps s, s + 1, s + 2
    constexpr unsigned kOOB = 0x80000000u;
    typedef __attribute__((address_space(3))) void* lds_ptr_t;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    // tile order: bands of one (sample, group) follow each other (they share patch halo rows, and all of them are on the same
    // product at about the same time), an XCD owns a contiguous chunk of the list
    const int nt = blockIdx.y;
    const int tile = xcd_remap(blockIdx.x, p.n_tiles);
    const int band = tile % p.tiles_per_frame;
    const int grp_ = tile / p.tiles_per_frame;
    const int grp = grp_ % p.G, n = grp_ / p.G;
    const int m0 = band * kRows;                        // first output (raster index inside the frame)
    const int ho_a = (int)tfir_fdiv((unsigned)m0, p.dv_wo);
    const int h_base = ho_a * p.sH - p.pH;

    const __amdgpu_buffer_rsrc_t rs_v = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.v), 0, p.v_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rs_w = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.w), 0, p.w_bytes, 0x00020000);

    // ---- per-thread sources of the patch pieces (product independent): piece q = tid + 256 i of the three planes ----
    unsigned a_src[12];       // (sized 12, used to NP)
    const int pc4 = p.PC >> 2, plane4 = p.plane >> 2;
#pragma unroll
    for (int i = 0; i < NP; ++i) {
        const int q = tid + kTfirNT * i;
        const int c = (int)tfir_fdiv((unsigned)q, p.dv_plane4);
        const int rem = q - c * plane4;
        const int pr = (int)tfir_fdiv((unsigned)rem, p.dv_pc4);
        const int h = h_base + pr, w = (rem - pr * pc4) * 4 + p.wbase;
        const bool ok = c < 3 && (unsigned)h < (unsigned)p.Hi && (unsigned)w < (unsigned)p.Wi;
        a_src[i] = ok ? (unsigned)((c * p.sc + h * p.pitch + w) * 4) : kOOB;
    }
    unsigned b_src[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) b_src[i] = (unsigned)((nt * kTfirBTile + (tid + kTfirNT * i) * 4) * 4);

    auto issue_b = [&](int buf, int s) {                  // filter tile of step s = j * kH + kh
        const unsigned tbase = (unsigned)(s * p.w_tiles * kTfirBTile * 4);
#pragma unroll
        for (int i = 0; i < 2; ++i)
            if (tid + kTfirNT * i < kTfirBTile / 4)
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_w, (lds_ptr_t)(Bs + buf * kTfirBTile + (wave * 64 + kTfirNT * i) * 4), 16,
                                                         b_src[i] + tbase, 0, 0, 0);
    };

    // ---- this lane's output rows: ml = m0 + wave * 32 RT + i * 32 + lane % 32 -> (ho, wo) ----
    const int g = lane >> 5, l32 = lane & 31;
    const int frame_out = p.Ho * p.Wo;
    // K pairing (conv_stem_f32.hip): five address flavours per row tile, fixed for the whole kernel
    int a_base[RT][5];
#pragma unroll
    for (int i = 0; i < RT; ++i) {
        const int ml = m0 + wave * (32 * RT) + i * 32 + l32;
        const int mm = ml < frame_out ? ml : m0;
        const int ho = (int)tfir_fdiv((unsigned)mm, p.dv_wo);
        const int wo = mm - ho * p.Wo;
        const int a_row = ((ho - ho_a) * p.sH) * p.PC + wo * p.sW + p.shift;
        a_base[i][0] = a_row + g;                      // j = 0..2 : plane 0, kw = 2p + g
        a_base[i][1] = a_row + g + p.plane;            // j = 3..5 : plane 1
        a_base[i][2] = a_row + g + 2 * p.plane;        // j = 6..8 : plane 2
        a_base[i][3] = a_row + g * p.plane + 6;        // j = 9    : (c = g, kw = 6)
        a_base[i][4] = a_row + 2 * p.plane + 6;        // j = 10   : (c = 2, kw = 6) | g = 1 multiplies a zero
    }

    f32x16 acc[RT][2];        // the current product
    f32x16 Y[M][RT][2];       // the group's output frames
#pragma unroll
    for (int i = 0; i < RT; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
#pragma unroll
            for (int o = 0; o < M; ++o)
#pragma unroll
                for (int r = 0; r < 16; ++r) Y[o][i][j][r] = 0.f;
        }
    // Y[o] += AT[o][jp] * acc; acc = 0.  The coefficients are uniform (kernel arguments): zeros are skipped by a scalar branch.
    auto fold = [&](int jp) {
#pragma unroll
        for (int o = 0; o < M; ++o) {
            const float c = p.at[o][jp];
            if (c != 0.f) {
#pragma unroll
                for (int i = 0; i < RT; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j)
#pragma unroll
                        for (int r = 0; r < 16; ++r) Y[o][i][j][r] = fmaf(c, acc[i][j][r], Y[o][i][j][r]);
            }
        }
#pragma unroll
        for (int i = 0; i < RT; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    };

    // ---- main loop: one step per (product, kh).  The fragment registers of k-pair group q are refilled for step s + 1 right
    // after the MFMAs of group q of step s have issued, so inside a product no MFMA waits on LDS.  Needs filter tile s + 1
    // landed at barrier(s): three filter slots.
    const int n_steps = p.P * p.kH;
    const int f0 = grp * p.P;                             // first "frame" of this group in V
    float fa[RT][kTfirK2], fb[2][kTfirK2];
    auto load_group = [&](int q, const float* Ab, const float* Bb) {
#pragma unroll
        for (int t = 0; t < 3; ++t) {
            const int j = q * 3 + t;
            if (j < kTfirK2) {
#pragma unroll
                for (int i = 0; i < RT; ++i) fa[i][j] = j < 9 ? Ab[a_base[i][j / 3] + 2 * (j % 3)] : Ab[a_base[i][j - 6]];
                fb[0][j] = Bb[j * 2 * kTfirBN];
                fb[1][j] = Bb[j * 2 * kTfirBN + 32];
            }
        }
    };
    auto mma_group = [&](int q) {
#pragma unroll
        for (int t = 0; t < 3; ++t) {
            const int j = q * 3 + t;
            if (j < kTfirK2) {
#pragma unroll
                for (int i = 0; i < RT; ++i) {
                    float a = fa[i][j];
                    if (j == 10) a = g ? 0.f : a;
                    acc[i][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, fb[0][j], acc[i][0], 0, 0, 0);
                    acc[i][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, fb[1][j], acc[i][1], 0, 0, 0);
                }
            }
        }
    };
    {
        // prologue: the first patch, filter tiles 0 and 1; then the fragments of step 0
        PTX_TFIR_DMA_PATCH(f0);
        issue_b(0, 0);
        issue_b(1, 1);                                    // (kH >= 2)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        asm volatile("; LDS reads stay below the barrier" : "+v"(a_base[0][0])::"memory");
#pragma unroll
        for (int q = 0; q < 4; ++q) load_group(q, As, Bs + g * kTfirBN + l32);
        int jp = 0, kh = 0, slot = 0;                     // state of step s: product, row tap, filter slot
        for (int s = 0; s < n_steps; ++s) {
            // filter tile s + 1 (issued during step s - 1) has landed for everyone; slot (s + 2) % 3 is free: its last reads
            // were issued during step s - 2 and consumed during step s - 1.  (Unconditional: at s == 0 it repeats the
            // prologue's barrier -- an `if (s > 0)` makes the compiler peel the first step, and the peeled copy of the body
            // spills the output accumulators.)
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            int kh1 = kh + 1, jp1 = jp;                   // (product, kh) of step s + 1
            if (kh1 == p.kH) { kh1 = 0; ++jp1; }
            const int slot1 = slot == 2 ? 0 : slot + 1;
            const int slot2 = slot1 == 2 ? 0 : slot1 + 1;
            if (s + 2 < n_steps) issue_b(slot2, s + 2);
            const bool more = s + 1 < n_steps;
            const bool same_product = kh1 != 0;
            const float* Bb = Bs + slot1 * kTfirBTile + g * kTfirBN + l32;
            const bool prefetch = more && same_product;
            const float* Ab = As + kh1 * p.PC;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                mma_group(q);
                __builtin_amdgcn_sched_barrier(0);
                if (prefetch) load_group(q, Ab, Bb);
                __builtin_amdgcn_sched_barrier(0);
            }
            if (more && !same_product) {
                // product change: every wave is done with the old patch; the next one is LDS-DMA'd while the finished
                // product is folded into the output accumulators
                __syncthreads();
                PTX_TFIR_DMA_PATCH(f0 + jp1);
                fold(jp);
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                __syncthreads();
                asm volatile("; LDS reads stay below the barrier" : "+v"(a_base[0][0])::"memory");
#pragma unroll
                for (int q = 0; q < 4; ++q) load_group(q, As, Bb);
            }
            kh = kh1; jp = jp1; slot = slot1;
        }
        fold(p.P - 1);        // (after the loop: folded inside it, the last product's outputs would be a second live copy of Y)
    }

    // ---- epilogue per output frame: bias (+ folded BN) + ReLU; lane = output channel, 16 rows per accumulator tile ----
    const bool relu = (p.flags & PTX_EPI_RELU) != 0;
    const __amdgpu_buffer_rsrc_t rs_y = __builtin_amdgcn_make_buffer_rsrc(p.y, 0, p.y_bytes, 0x00020000);
    float bv[2];
    bool co_ok[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int co = nt * kTfirBN + j * 32 + l32;
        co_ok[j] = co < p.ncol;
        bv[j] = (p.bias && co_ok[j]) ? p.bias[co] : 0.f;
    }
#pragma unroll
    for (int o = 0; o < M; ++o) {
        const int to = grp * M + o;
        if (to < p.To) {                                  // (uniform) frames past the clip's end are not written
            const int m_frame = (n * p.To + to) * frame_out;
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int co = nt * kTfirBN + j * 32 + l32;
#pragma unroll
                for (int i = 0; i < RT; ++i) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        // accumulator element r of this lane belongs to tile row (r & 3) + 8 * (r >> 2) + 4 * g
                        const int ml = m0 + wave * (32 * RT) + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * g;
                        float v = Y[o][i][j][r] + bv[j];
                        v = relu ? fmaxf(v, 0.f) : v;
                        const unsigned off = ((unsigned)(m_frame + ml) * (unsigned)p.ldy + (unsigned)co) * 4u;
                        __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), rs_y,
                                                              (co_ok[j] && ml < frame_out) ? off : kOOB, 0, 0);
                    }
                }
            }
        }
    }
}

template <int M, int RT, int NP>
static int launch_tfir(const TfirArgs& a, dim3 grid, size_t lds, ptx_stream_t stream) {
    static bool attr_set[64] = {};
    int dev = 0;
    PTX_HIP(hipGetDevice(&dev));
    if (dev < 0 || dev >= 64 || !attr_set[dev]) {
        PTX_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&conv_stem_tfir_f32_kernel<M, RT, NP>),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, (int)((kTfirPatchMax + 3 * kTfirBTile) * sizeof(float))));
        if (dev >= 0 && dev < 64) attr_set[dev] = true;
    }
    hipLaunchKernelGGL(HIP_KERNEL_NAME(conv_stem_tfir_f32_kernel<M, RT, NP>), grid, dim3(kTfirNT), lds, (hipStream_t)stream, a);
    return PTX_OK;
}

template <int M, int RT>
static int launch_tfir_np(const TfirArgs& a, dim3 grid, size_t lds, ptx_stream_t stream) {
    return cdiv(a.n_pieces, kTfirNT) <= 8 ? launch_tfir<M, RT, 8>(a, grid, lds, stream) : launch_tfir<M, RT, 12>(a, grid, lds, stream);
}

struct TfirGeom {
    int PR, PC, shift, wbase, tiles_per_frame;
};

// the patch of a workgroup of `rows` consecutive outputs (conv_stem_f32.hip's rule at its 256)
static bool tfir_geom(const ptx_conv3d_desc* d, int rows, TfirGeom* g) {
    const int frame = d->Ho * d->Wo;
    const int nrows = std::min(d->Ho, (rows - 1 + d->Wo - 1) / d->Wo + 1);
    g->PR = (nrows - 1) * d->sH + d->kH;
    g->wbase = -((d->pW + 3) / 4 * 4);
    g->shift = -g->wbase - d->pW;
    g->PC = ((d->Wo - 1) * d->sW + g->shift + d->kW + 3) / 4 * 4;
    g->tiles_per_frame = cdiv(frame, rows);
    return (int64_t)3 * g->PR * g->PC <= kTfirPatchMax;
}

// 32-row tiles per wave of the forward kernel.  Measured on MI355X at 8x3x16x224x224: 1 (32 rows per wave, two
// or three workgroups per CU) beats 2 (the direct kernel's 64 rows, one wave per SIMD) for every scheme -- in + forward 1.13 /
// 1.06 / 0.83 ms against 1.66 / 1.48 / 1.16 ms for schemes 1 / 2 / 3 -- so only RT = 1 is instantiated.
constexpr int kTfirRowTiles = 1;

static int64_t tfir_groups(const ptx_conv3d_desc* d, const TfirScheme* s) { return (d->To + s->m - 1) / s->m; }

static int64_t tfir_v_elems(const ptx_conv3d_desc* d, const TfirScheme* s) {
    const int64_t pitch = d->ldx > 0 ? d->ldx : d->Wi;
    return (int64_t)d->N * 3 * tfir_groups(d, s) * s->P * d->Hi * pitch;
}

}  // namespace ptx

using namespace ptx;

extern "C" int ptx_stem_tfir_scheme(int32_t scheme, int32_t* m, int32_t* P, float* AT, float* G, float* BT) {
    const TfirScheme* s = tfir_scheme(scheme);
    if (!s) return fail(PTX_ERR_UNSUPPORTED, "stem_tfir: scheme %d (1..3)", (int)scheme);
    if (m) *m = s->m;
    if (P) *P = s->P;
    if (AT) std::copy(s->AT, s->AT + s->m * s->P, AT);
    if (G) std::copy(s->G, s->G + s->P * kTfirKT, G);
    if (BT) std::copy(s->BT, s->BT + s->P * (s->m + kTfirKT - 1), BT);
    return PTX_OK;
}

extern "C" int ptx_conv_stem_tfir_f32_supported(const ptx_conv3d_desc* d, int64_t stride_n, int64_t stride_c, int64_t stride_t,
                                                int32_t scheme) {
    const TfirScheme* s = tfir_scheme(scheme);
    if (!d || !s) return 0;
    if (!ptx_conv_stem_f32_supported(d, stride_n, stride_c, stride_t)) return 0;
    if (d->sT != 1 || d->kT != kTfirKT) return 0;
    TfirGeom g;
    if (!tfir_geom(d, 128 * kTfirRowTiles, &g)) return 0;
    // V, the filter and y are addressed with 32-bit byte offsets
    if (tfir_v_elems(d, s) * 4 >= 0x80000000LL) return 0;
    if ((int64_t)s->P * d->kH * (d->Co_pad / kTfirBN) * kTfirBTile * 4 >= 0x80000000LL) return 0;
    return 1;
}

extern "C" size_t ptx_stem_tfir_f32_weight_elems(const ptx_conv3d_desc* d, int32_t scheme) {
    const TfirScheme* s = tfir_scheme(scheme);
    if (!d || !s || d->Co_pad <= 0 || d->Co_pad % kTfirBN || d->kH <= 0) return 0;
    return (size_t)s->P * d->kH * (d->Co_pad / kTfirBN) * kTfirBTile;
}

extern "C" size_t ptx_stem_tfir_f32_workspace_bytes(const ptx_conv3d_desc* d, int32_t scheme) {
    const TfirScheme* s = tfir_scheme(scheme);
    if (!d || !s || d->N <= 0 || d->To <= 0 || d->Hi <= 0 || d->Wi <= 0) return 0;
    return (size_t)tfir_v_elems(d, s) * sizeof(float);
}

extern "C" int ptx_pack_stem_tfir_f32_weight(const ptx_conv3d_desc* d, int32_t scheme, const float* w_stem, float* w_tfir,
                                             ptx_stream_t stream) {
    const TfirScheme* s = tfir_scheme(scheme);
    if (!d || !w_stem || !w_tfir) return fail(PTX_ERR_INVALID, "pack_stem_tfir_f32: null pointer");
    if (!s || d->kT != kTfirKT || d->Co_pad <= 0 || d->Co_pad % kTfirBN || d->kH <= 0)
        return fail(PTX_ERR_UNSUPPORTED, "pack_stem_tfir_f32: a packed stem filter with 7 temporal taps and a scheme 1..3");
    const size_t inner = (size_t)d->kH * (d->Co_pad / kTfirBN) * kTfirBTile;
    if (inner * s->P >= (1ull << 29)) return fail(PTX_ERR_UNSUPPORTED, "pack_stem_tfir_f32: filter too large");
    TfirCoefG c{};
    for (int j = 0; j < s->P; ++j)
        for (int k = 0; k < kTfirKT; ++k) c.g[j][k] = s->G[j * kTfirKT + k];
    hipLaunchKernelGGL(tfir_pack_kernel, dim3((unsigned)std::min<size_t>(cdiv64(inner, 256), 4096)), dim3(256), 0, (hipStream_t)stream,
                       w_stem, w_tfir, (int)inner, s->P, c);
    return hip_check(hipGetLastError(), "pack_stem_tfir_f32 launch");
}

extern "C" int ptx_stem_tfir_in_f32(const ptx_conv3d_desc* d, int32_t scheme, const float* x, int64_t stride_n, int64_t stride_c,
                                    int64_t stride_t, float* V, ptx_stream_t stream) {
    if (!d || !x || !V) return fail(PTX_ERR_INVALID, "stem_tfir_in_f32: null pointer");
    if (((uintptr_t)x | (uintptr_t)V) & 15) return fail(PTX_ERR_INVALID, "stem_tfir_in_f32: pointers must be 16-byte aligned");
    if (!ptx_conv_stem_tfir_f32_supported(d, stride_n, stride_c, stride_t, scheme))
        return fail(PTX_ERR_UNSUPPORTED, "stem_tfir_in_f32: needs what conv_stem_f32 takes, temporal stride 1, 7 temporal taps, "
                    "a scheme 1..3 and a transformed input below 2 GiB");
    const TfirScheme* s = tfir_scheme(scheme);
    TfirInArgs a{};
    a.x = x; a.v = V;
    a.Ti = d->Ti; a.Hi = d->Hi; a.pitch4 = (d->ldx > 0 ? d->ldx : d->Wi) / 4;
    a.G = (int)tfir_groups(d, s); a.P = s->P; a.pT = d->pT;
    a.sn = stride_n; a.sc = stride_c; a.st = stride_t;
    a.total = (long long)d->N * 3 * a.G * d->Hi * a.pitch4;
    const int win = s->m + kTfirKT - 1;
    for (int j = 0; j < s->P; ++j)
        for (int i = 0; i < win; ++i) a.bt[j][i] = s->BT[j * win + i];
    const dim3 grid((unsigned)cdiv64(a.total, 256));
    if (s->m == 2) hipLaunchKernelGGL(HIP_KERNEL_NAME(tfir_in_kernel<2>), grid, dim3(256), 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(HIP_KERNEL_NAME(tfir_in_kernel<4>), grid, dim3(256), 0, (hipStream_t)stream, a);
    return hip_check(hipGetLastError(), "stem_tfir_in_f32 launch");
}

extern "C" int ptx_conv_stem_tfir_f32_fwd(const ptx_conv3d_desc* d, int32_t scheme, const float* V, const float* w_tfir,
                                          const float* bias, float* y, ptx_stream_t stream) {
    if (!d || !V || !w_tfir || !y) return fail(PTX_ERR_INVALID, "conv_stem_tfir_f32: null pointer");
    if (((uintptr_t)V | (uintptr_t)w_tfir | (uintptr_t)y) & 15)
        return fail(PTX_ERR_INVALID, "conv_stem_tfir_f32: pointers must be 16-byte aligned");
    const TfirScheme* s = tfir_scheme(scheme);
    const int pitch = d->ldx > 0 ? d->ldx : d->Wi;
    // V is dense: its own strides stand in for the caller's in the direct stem's rule
    const int64_t v_frame = (int64_t)d->Hi * pitch;
    const int64_t x_st = v_frame, x_sc = (int64_t)d->Ti * v_frame, x_sn = 3 * x_sc;
    if (!s || !ptx_conv_stem_tfir_f32_supported(d, x_sn, x_sc, x_st, scheme))
        return fail(PTX_ERR_UNSUPPORTED, "conv_stem_tfir_f32: needs what conv_stem_f32 takes, temporal stride 1, 7 temporal taps, "
                    "a scheme 1..3 and a transformed input below 2 GiB");
    if (d->ldy < d->Co || d->ldy % 4) return fail(PTX_ERR_INVALID, "conv_stem_tfir_f32: bad output stride");
    TfirGeom g;
    tfir_geom(d, 128 * kTfirRowTiles, &g);
    TfirArgs a{};
    a.v = V; a.w = w_tfir; a.bias = bias; a.y = y;
    a.N = d->N; a.Hi = d->Hi; a.Wi = d->Wi; a.To = d->To; a.Ho = d->Ho; a.Wo = d->Wo; a.ldy = d->ldy;
    a.ncol = (d->Co + 3) / 4 * 4;
    a.kH = d->kH; a.sH = d->sH; a.sW = d->sW; a.pH = d->pH;
    a.pitch = pitch;
    a.P = s->P; a.G = (int)tfir_groups(d, s);
    a.st = (int)v_frame; a.sc = (int)((int64_t)a.G * s->P * v_frame); a.sn = 3 * a.sc;
    a.PR = g.PR; a.PC = g.PC; a.plane = g.PR * g.PC; a.shift = g.shift; a.wbase = g.wbase;
    a.tiles_per_frame = g.tiles_per_frame;
    a.n_tiles = d->N * a.G * g.tiles_per_frame;
    a.n_pieces = 3 * a.plane / 4;                           // 16-byte pieces of the patch (PC % 4 == 0)
    a.w_tiles = d->Co_pad / kTfirBN;
    a.flags = d->flags;
    a.v_bytes = (unsigned)(tfir_v_elems(d, s) * 4);
    a.w_bytes = (unsigned)(ptx_stem_tfir_f32_weight_elems(d, scheme) * 4ull);
    a.y_bytes = (unsigned)((uint64_t)d->N * d->To * d->Ho * d->Wo * d->ldy * 4ull);
    tfir_fdiv_make((unsigned)d->Wo, a.dv_wo);
    tfir_fdiv_make((unsigned)(a.plane / 4), a.dv_plane4);
    tfir_fdiv_make((unsigned)(a.PC / 4), a.dv_pc4);
    for (int o = 0; o < s->m; ++o)
        for (int j = 0; j < s->P; ++j) a.at[o][j] = s->AT[o * s->P + j];
    const size_t lds = (size_t)(3 * a.plane + 3 * kTfirBTile) * sizeof(float);
    const dim3 grid((unsigned)a.n_tiles, (unsigned)cdiv(a.ncol, kTfirBN));
    int rc;
    if (s->m == 2) rc = launch_tfir_np<2, kTfirRowTiles>(a, grid, lds, stream);
    else rc = launch_tfir_np<4, kTfirRowTiles>(a, grid, lds, stream);
    if (rc != PTX_OK) return rc;
    return hip_check(hipGetLastError(), "conv_stem_tfir_f32 launch");
}
