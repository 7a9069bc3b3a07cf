// The fp32 RGB stem (Conv3d(3, Co, 7, stride (1,s,s), pad 3) + BN + ReLU) as a fast FIR along time: fewer frame-convolutions
// than conv_stem_f32.hip issues, on the same patch-resident step loop (conv_stem_patch_f32.h).
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
//   conv_stem_tfir_f32_kernel   the shared step loop over the P "frames" of group g of V (no pruning: every group runs all P
//                      products); at each product change, where the patch is re-staged anyway, the product's accumulator tile
//                      is folded into the m output accumulators with VALU FMAs (Y[o] += AT[o][j] M, zero coefficients skipped,
//                      while the next patch's DMA is in flight); the epilogue runs per output frame, frames past To masked.
// Register budget: the product tile + m output tiles.  At the direct kernel's 64 rows per wave that is 64 + 64 m accumulators
// (one wave per SIMD for either m); a wave therefore owns 32 rows (32 + 32 m accumulators: 153 VGPRs and three workgroups per
// CU for m = 2, 217 and two for m = 4, no scratch) and a workgroup 128 outputs, whose smaller patch keeps LDS under 48 KB.
// Arithmetic: fp32 throughout.
#include "conv_stem_patch_f32.h"
#include "../../include/ptx_amd_tfir.h"

namespace ptx {

constexpr int kTfirKT = 7;                          // temporal taps
constexpr int kTfirMaxM = 4, kTfirMaxP = 13, kTfirMaxWin = kTfirMaxM + kTfirKT - 1;
// 32-row tiles per wave of the forward kernel.  Measured on MI355X at 8x3x16x224x224: 1 (32 rows per wave, two
// or three workgroups per CU) beats 2 (the direct kernel's 64 rows, one wave per SIMD) for every scheme -- in + forward 1.13 /
// 1.06 / 0.83 ms against 1.66 / 1.48 / 1.16 ms for schemes 1 / 2 / 3.
constexpr int kTfirRT = 1;
constexpr int kTfirRows = 4 * 32 * kTfirRT;         // outputs per workgroup

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
    StemPatchArgs s;      // x: V, [N][3][G * P][Hi][pitch]; w: [P * kH][w_tiles][11][2][64]
    int P, G;             // products per group, groups per clip
    float at[kTfirMaxM][kTfirMaxP];
};

// M: output frames per group.  NP: 16-byte patch pieces per thread (8 or 12).
template <int M, int NP>
// (flatten: see conv_stem_patch_f32.h on how its functions are inlined)
__global__ void __launch_bounds__(kStemNT, 2) __attribute__((flatten)) conv_stem_tfir_f32_kernel(const TfirArgs p) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int RT = kTfirRT;
    // tile order: bands of one (sample, group) follow each other (they share patch halo rows, and all of them are on the same
    // product at about the same time), an XCD owns a contiguous chunk of the list
    const int tile = xcd_remap(blockIdx.x, p.s.n_tiles);
    const int grp_ = tile / p.s.tiles_per_frame;
    const int grp = grp_ % p.G;
    StemPatchTile<RT> c;
    stem_patch_tile<RT, NP>(p.s, smem, tile % p.s.tiles_per_frame, grp_ / p.G, c);

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
            const float cf = p.at[o][jp];
            if (cf != 0.f) {
#pragma unroll
                for (int i = 0; i < RT; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j)
#pragma unroll
                        for (int r = 0; r < 16; ++r) Y[o][i][j][r] = fmaf(cf, acc[i][j][r], Y[o][i][j][r]);
            }
        }
#pragma unroll
        for (int i = 0; i < RT; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    };

    // one step per (product, kh): the group's products are frames grp * P ... of V, filter blocks 0 ... P * kH - 1
    stem_patch_loop<RT, NP>(p.s, c, p.P, 0, grp * p.P, acc, fold);
    fold(p.P - 1);            // (after the loop: folded inside it, the last product's outputs would be a second live copy of Y)

    const StemPatchEpi e = stem_patch_epi(p.s, c);
#pragma unroll
    for (int o = 0; o < M; ++o) {
        const int to = grp * M + o;
        if (to < p.s.To) stem_patch_store(p.s, c, e, to, Y[o]);      // (uniform) frames past the clip's end are not written
    }
}

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
    StemPatchGeom g;
    if (!stem_patch_geom(d, kTfirRows, &g)) return 0;
    // V, the filter and y are addressed with 32-bit byte offsets
    if (tfir_v_elems(d, s) * 4 >= 0x80000000LL) return 0;
    if ((int64_t)s->P * d->kH * (d->Co_pad / kStemBN) * kStemBTile * 4 >= 0x80000000LL) return 0;
    return 1;
}

extern "C" size_t ptx_stem_tfir_f32_weight_elems(const ptx_conv3d_desc* d, int32_t scheme) {
    const TfirScheme* s = tfir_scheme(scheme);
    if (!d || !s || d->Co_pad <= 0 || d->Co_pad % kStemBN || d->kH <= 0) return 0;
    return (size_t)s->P * d->kH * (d->Co_pad / kStemBN) * kStemBTile;
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
    if (!s || d->kT != kTfirKT || d->Co_pad <= 0 || d->Co_pad % kStemBN || d->kH <= 0)
        return fail(PTX_ERR_UNSUPPORTED, "pack_stem_tfir_f32: a packed stem filter with 7 temporal taps and a scheme 1..3");
    const size_t inner = (size_t)d->kH * (d->Co_pad / kStemBN) * kStemBTile;
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
    TfirArgs a{};
    a.P = s->P; a.G = (int)tfir_groups(d, s);
    const int64_t v_sc = (int64_t)a.G * s->P * v_frame;
    stem_patch_fill(a.s, d, kTfirRows, d->N * a.G, V, 3 * v_sc, v_sc, v_frame, (uint64_t)tfir_v_elems(d, s) * 4ull, w_tfir,
                    ptx_stem_tfir_f32_weight_elems(d, scheme) * 4ull, bias, y);
    for (int o = 0; o < s->m; ++o)
        for (int j = 0; j < s->P; ++j) a.at[o][j] = s->AT[o * s->P + j];
    const bool np8 = cdiv(a.s.n_pieces, kStemNT) <= 8;
    const int rc = s->m == 2 ? (np8 ? stem_patch_launch<&conv_stem_tfir_f32_kernel<2, 8>>(a, a.s, stream)
                                    : stem_patch_launch<&conv_stem_tfir_f32_kernel<2, 12>>(a, a.s, stream))
                             : (np8 ? stem_patch_launch<&conv_stem_tfir_f32_kernel<4, 8>>(a, a.s, stream)
                                    : stem_patch_launch<&conv_stem_tfir_f32_kernel<4, 12>>(a, a.s, stream));
    if (rc != PTX_OK) return rc;
    return hip_check(hipGetLastError(), "conv_stem_tfir_f32 launch");
}
