// The patch-resident step loop of the fp32 RGB stems, shared by its two users: the direct kernel (conv_stem_f32.hip, RT = 2) and
// the fast FIR along time (conv_stem_tfir_f32.hip, RT = 1).  Everything about how a workgroup stages an input patch and runs a
// 7-wide, 3-channel filter over it on the fp32 matrix cores is here; what the two kernels do around it (which frames they walk,
// what happens to a finished accumulator tile) is in their own files.
//
// A workgroup (4 waves, each RT 32-row tiles) owns 128 RT consecutive outputs (raster order) of one output frame and stages the
// INPUT PATCH of one source frame once with LDS-DMA -- three channel planes of PR rows x PC floats, exactly the source's NCDHW
// rows (16-byte pieces, zero outside the image) -- and serves all kH x 7 taps of that frame from it.  No fold, no layout pass:
// the kernel reads the user tensor.  LDS per workgroup = the patch + three 5.5 KiB filter slots, so two or three workgroups
// share a CU and cover each other's frame-change DMA wait, barriers, prologue and epilogue (one 8-wave workgroup
// per CU could not be scheduled out of its bubbles).
//
// K axis of one (frame, kh) step: 21 = 3 channels x 7 kw, issued as 11 v_mfma_f32_32x32x2_f32 (k = 2 per instruction; lanes
// 0-31 hold k0, lanes 32-63 hold k1 =: g).  Pairing keeps the g-dependence of the A address a constant:
//     j = 3c + p (j < 9): (c, kw = 2p + g)         -- one float apart
//     j = 9             : (c = g, kw = 6)          -- one plane apart
//     j = 10            : (c = 2, kw = 6) | zero
// so a fragment is one ds_read_b32 at (patch row r*sH + kh, column wo*sW + shift + kw) of plane c.  The filter comes
// from ptx_pack_stem_f32_weight in exactly that order ([step][64-channel tile][11][2][64] floats, conflict-free reads).
// Arithmetic: fp32 operands, fp32 accumulate -- the reference's own.
#pragma once
#include "ptx_common.h"
#include <algorithm>

namespace ptx {

constexpr int kStemNT = 256;                         // 4 waves
constexpr int kStemBN = 64;                          // output channels per workgroup
constexpr int kStemPatchMax = 12288;                 // floats of the patch buffer: 48 KiB
constexpr int kStemK2 = 11;                          // MFMAs per step and accumulator tile
constexpr int kStemBTile = kStemK2 * 2 * kStemBN;    // floats of one (step, channel tile) filter block: 5.5 KiB
constexpr unsigned kStemOOB = 0x80000000u;           // a buffer offset past every descriptor's range: loads zero, stores nothing

// diagnostic phase clock of the direct kernel (conv_stem_f32.hip defines it under -DPTX_STEM_TIMELINE); nothing otherwise
#ifndef PTX_STEM_TL
#define PTX_STEM_TL(k) do {} while (0)
#endif

// what both kernels take from the descriptor
struct StemPatchArgs {
    const float* x;       // NCDHW source (strides below, in floats): the caller's tensor, or the fast FIR's transformed V
    const float* w;       // [steps][w_tiles][11][2][64]
    const float* bias;
    float* y;             // [N][To][Ho][Wo][ldy]
    int N, Hi, Wi, To, Ho, Wo, ldy, ncol;
    int pitch;            // floats per input row (>= Wi, multiple of 4; [Wi, pitch) are zero)
    int kH, sH, sW, pH;
    int sn, sc, st;       // batch / channel / frame strides of x
    int PR, PC, plane;    // patch rows, floats per patch row (multiple of 4), PR * PC
    int shift, wbase;     // patch column 0 is input column wbase (<= 0, multiple of 4); a window starts at wo*sW + shift
    int tiles_per_frame, n_tiles, n_pieces, w_tiles;
    unsigned flags;
    unsigned x_bytes, w_bytes, y_bytes;
    unsigned dv_wo[2];
    unsigned dv_plane4[2], dv_pc4[2];     // fast division by plane / 4 and PC / 4 (the prologue's patch-piece decode)
};

struct StemPatchGeom {
    int PR, PC, shift, wbase, tiles_per_frame;
};

// the patch of a workgroup of `rows` consecutive outputs (256 direct, 128 fast FIR); false when it does not fit
static bool stem_patch_geom(const ptx_conv3d_desc* d, int rows, StemPatchGeom* g) {
    const int frame = d->Ho * d->Wo;
    // rows a `rows`-output raster span can touch
    const int nrows = std::min(d->Ho, (rows - 1 + d->Wo - 1) / d->Wo + 1);
    g->PR = (nrows - 1) * d->sH + d->kH;
    g->wbase = -((d->pW + 3) / 4 * 4);
    g->shift = -g->wbase - d->pW;
    g->PC = ((d->Wo - 1) * d->sW + g->shift + d->kW + 3) / 4 * 4;
    g->tiles_per_frame = cdiv(frame, rows);
    return (int64_t)3 * g->PR * g->PC <= kStemPatchMax;
}

// `groups`: (sample, output frame) pairs of the direct kernel, (sample, frame group) pairs of the fast FIR
static void stem_patch_fill(StemPatchArgs& a, const ptx_conv3d_desc* d, int rows, int groups, const float* x, int64_t sn, int64_t sc,
                            int64_t st, uint64_t x_bytes, const float* w, uint64_t w_bytes, const float* bias, float* y) {
    StemPatchGeom g;
    stem_patch_geom(d, rows, &g);
    a.x = x; a.w = w; a.bias = bias; a.y = y;
    a.N = d->N; a.Hi = d->Hi; a.Wi = d->Wi; a.To = d->To; a.Ho = d->Ho; a.Wo = d->Wo; a.ldy = d->ldy;
    a.ncol = (d->Co + 3) / 4 * 4;
    a.pitch = d->ldx > 0 ? d->ldx : d->Wi;
    a.kH = d->kH; a.sH = d->sH; a.sW = d->sW; a.pH = d->pH;
    a.sn = (int)sn; a.sc = (int)sc; a.st = (int)st;
    a.PR = g.PR; a.PC = g.PC; a.plane = g.PR * g.PC; a.shift = g.shift; a.wbase = g.wbase;
    a.tiles_per_frame = g.tiles_per_frame;
    a.n_tiles = groups * g.tiles_per_frame;
    a.n_pieces = 3 * a.plane / 4;                           // 16-byte pieces of the patch (PC % 4 == 0)
    a.w_tiles = d->Co_pad / kStemBN;
    a.flags = d->flags;
    a.x_bytes = (unsigned)x_bytes;
    a.w_bytes = (unsigned)w_bytes;
    a.y_bytes = (unsigned)((uint64_t)d->N * d->To * d->Ho * d->Wo * d->ldy * 4ull);
    fdiv_make((unsigned)d->Wo, a.dv_wo);
    fdiv_make((unsigned)(a.plane / 4), a.dv_plane4);
    fdiv_make((unsigned)(a.PC / 4), a.dv_pc4);
}

static size_t stem_patch_lds_bytes(const StemPatchArgs& a) { return (size_t)(3 * a.plane + 3 * kStemBTile) * sizeof(float); }

// launch with the dynamic-LDS limit raised once per device
template <auto Kernel, class Args>
static int stem_patch_launch(const Args& a, const StemPatchArgs& s, ptx_stream_t stream) {
    static bool attr_set[64] = {};
    int dev = 0;
    PTX_HIP(hipGetDevice(&dev));
    if (dev < 0 || dev >= 64 || !attr_set[dev]) {
        PTX_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)((kStemPatchMax + 3 * kStemBTile) * sizeof(float))));
        if (dev >= 0 && dev < 64) attr_set[dev] = true;
    }
    hipLaunchKernelGGL(Kernel, dim3((unsigned)s.n_tiles, (unsigned)cdiv(s.ncol, kStemBN)), dim3(kStemNT), stem_patch_lds_bytes(s),
                       (hipStream_t)stream, a);
    return PTX_OK;
}

typedef __attribute__((address_space(3))) void* stem_lds_ptr_t;

// The device functions below are `inline`, not __forceinline__, on purpose, and both kernels carry __attribute__((flatten)) so
// that all of them are inlined whatever the inliner's cost model says (they take references to fa / fb / acc: left as calls, those
// arrays would go to scratch).  Measured, not derived: with __forceinline__ the direct kernel compiles to 150 / 154 / 159 VGPRs
// and the fast FIR <2, 12> to 173 (two workgroups per CU), its IR keeps fa and fb as two 22-float vectors and the step loop
// copies every fragment; the likely reason is that forced inlining runs before the callees' loops are unrolled, so the arrays
// still look dynamically indexed when the backend decides how to keep them.  After a toolchain change rerun
// `python pretorched-x_amd/csrc/build.py --force --report` and compare with profiles/stem_patch_refactor_resources.txt.

// per-thread state of a workgroup's tile.  RT: 32-row tiles per wave
template <int RT>
struct StemPatchTile {
    float* As;            // [3 * plane]: the patch of the current source frame
    float* Bs;            // [3][kStemBTile]: filter tiles of steps s, s + 1, s + 2
    float *a_dst, *b_dst; // where this wave's 64 DMA pieces (1 KiB) land in As / in a filter slot
    __amdgpu_buffer_rsrc_t rs_x, rs_w;
    int tid, wave, g, l32;
    int n, nt, m0;        // sample, channel tile, first output (raster index inside the frame)
    int frame_out;
    unsigned a_src[12];   // (sized 12, used to NP: a template-dependent extent here makes hipcc's host pass drop the kernel stub)
    unsigned b_src[2];
    unsigned b_step;      // bytes between the filter blocks of consecutive steps
    int a_base[RT][5];
};

// NP: 16-byte patch pieces per thread (4, 8 or 12)
template <int RT, int NP>
__device__ inline void stem_patch_tile(const StemPatchArgs& p, float* smem, int band, int n, StemPatchTile<RT>& c) {
    c.As = smem;
    c.Bs = smem + 3 * p.plane;
    c.tid = threadIdx.x;
    const int lane = c.tid & 63;
    c.wave = __builtin_amdgcn_readfirstlane(c.tid >> 6);
    // (made once: recomputed at each use, the copies meet in a phi behind the per-thread `piece < n_pieces` branches, the
    //  compiler has to call that phi divergent, and every DMA address costs a VGPR and a readfirstlane)
    c.a_dst = c.As + c.wave * 64 * 4;
    c.b_dst = c.Bs + c.wave * 64 * 4;
    c.b_step = (unsigned)(p.w_tiles * kStemBTile * 4);
    // (band and n are workgroup-uniform quotients; integer division runs on the vector unit, so say it, or the frame offset of
    //  every DMA and the row arithmetic below stay vector work)
    c.n = __builtin_amdgcn_readfirstlane(n);
    c.nt = blockIdx.y;
    c.m0 = __builtin_amdgcn_readfirstlane(band) * (4 * 32 * RT);
    const int ho_a = (int)fdiv((unsigned)c.m0, p.dv_wo);
    const int h_base = ho_a * p.sH - p.pH;

    c.rs_x = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.x), 0, p.x_bytes, 0x00020000);
    c.rs_w = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.w), 0, p.w_bytes, 0x00020000);

    // ---- per-thread sources of the patch pieces (frame independent): piece q = tid + 256 i of the three planes ----
    // (multiply-shift divisions: two plain integer divisions per piece were ~1000 VALU instructions per thread, and VALU
    //  work shares the fp32 datapath with the co-resident workgroups' MFMAs -- the phase clock, scripts/gpu_stem_timeline.py,
    //  showed 22 us of a 177-us workgroup life before the first request went out, 9.6 of 34 us on the (1,7,7) stem)
    const int pc4 = p.PC >> 2, plane4 = p.plane >> 2;
#pragma unroll
    for (int i = 0; i < NP; ++i) {
        const int q = c.tid + kStemNT * i;
        const int ch = (int)fdiv((unsigned)q, p.dv_plane4);
        const int rem = q - ch * plane4;
        const int pr = (int)fdiv((unsigned)rem, p.dv_pc4);
        const int h = h_base + pr, w = (rem - pr * pc4) * 4 + p.wbase;
        const bool ok = ch < 3 && (unsigned)h < (unsigned)p.Hi && (unsigned)w < (unsigned)p.Wi;
        c.a_src[i] = ok ? (unsigned)((ch * p.sc + h * p.pitch + w) * 4) : kStemOOB;
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) c.b_src[i] = (unsigned)((c.nt * kStemBTile + (c.tid + kStemNT * i) * 4) * 4);

    // ---- this lane's output rows: ml = m0 + wave * 32 RT + i * 32 + lane % 32 -> (ho, wo) ----
    c.g = lane >> 5;
    c.l32 = lane & 31;
    c.frame_out = p.Ho * p.Wo;
    // K pairing (see the header): five address flavours per row tile, fixed for the whole kernel -- a step only adds its
    // kh offset, so the loop spends well under one VALU instruction per MFMA on addresses
#pragma unroll
    for (int i = 0; i < RT; ++i) {
        const int ml = c.m0 + c.wave * (32 * RT) + i * 32 + c.l32;
        const int mm = ml < c.frame_out ? ml : c.m0;
        const int ho = (int)fdiv((unsigned)mm, p.dv_wo);
        const int wo = mm - ho * p.Wo;
        // float offset of (patch row (ho - ho_a) * sH, column wo * sW + shift)
        const int a_row = ((ho - ho_a) * p.sH) * p.PC + wo * p.sW + p.shift;
        c.a_base[i][0] = a_row + c.g;                      // j = 0..2 : plane 0, kw = 2p + g
        c.a_base[i][1] = a_row + c.g + p.plane;            // j = 3..5 : plane 1
        c.a_base[i][2] = a_row + c.g + 2 * p.plane;        // j = 6..8 : plane 2
        c.a_base[i][3] = a_row + c.g * p.plane + 6;        // j = 9    : (c = g, kw = 6)
        c.a_base[i][4] = a_row + 2 * p.plane + 6;          // j = 10   : (c = 2, kw = 6) | g = 1 multiplies a zero
    }
}

// fragments of k-pair group q (j = 3q .. 3q + 2)
template <int RT>
__device__ inline void stem_patch_load_group(const StemPatchTile<RT>& c, int q, const float* Ab, const float* Bb,
                                             float (&fa)[RT][kStemK2], float (&fb)[2][kStemK2]) {
#pragma unroll
    for (int t = 0; t < 3; ++t) {
        const int j = q * 3 + t;
        if (j < kStemK2) {
#pragma unroll
            for (int i = 0; i < RT; ++i) fa[i][j] = j < 9 ? Ab[c.a_base[i][j / 3] + 2 * (j % 3)] : Ab[c.a_base[i][j - 6]];
            fb[0][j] = Bb[j * 2 * kStemBN];
            fb[1][j] = Bb[j * 2 * kStemBN + 32];
        }
    }
}

template <int RT>
__device__ inline void stem_patch_mma_group(int g, int q, const float (&fa)[RT][kStemK2], const float (&fb)[2][kStemK2],
                                            f32x16 (&acc)[RT][2]) {
#pragma unroll
    for (int t = 0; t < 3; ++t) {
        const int j = q * 3 + t;
        if (j < kStemK2) {
#pragma unroll
            for (int i = 0; i < RT; ++i) {
                float a = fa[i][j];
                if (j == 10) a = g ? 0.f : a;
                acc[i][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, fb[0][j], acc[i][0], 0, 0, 0);
                acc[i][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, fb[1][j], acc[i][1], 0, 0, 0);
            }
        }
    }
}

template <int RT>
__device__ inline void stem_patch_reads_below_barrier(StemPatchTile<RT>& c) {
    if constexpr (RT == 1) asm volatile("; LDS reads stay below the barrier" : "+v"(c.a_base[0][0])::"memory");
    else asm volatile("; LDS reads stay below the barrier" : "+v"(c.a_base[0][0]), "+v"(c.a_base[RT - 1][0])::"memory");
}

// The step loop: n_frames source frames frame0, frame0 + 1, ... of sample c.n, kH steps each; step (i, kh) multiplies patch rows
// kh, kh + sH, ... of frame frame0 + i with filter block (tap0 + i) * kH + kh and accumulates into acc.  The direct kernel walks the
// valid temporal taps of one output frame (tap0 = kt_lo), the fast FIR the products of one group (tap0 = 0).  at_change(i) runs
// after frame i's last step while the next patch's DMA is in flight -- acc then holds frame i's contribution (the fast FIR folds
// it away there; the direct kernel keeps accumulating).
// The fragment registers of k-pair group q are refilled for step s + 1 right after the MFMAs of group q of step s have issued, so
// inside a frame no MFMA waits on LDS.  Needs filter tile s + 1 landed at barrier(s): three filter slots.
template <int RT, int NP, class AtChange>
__device__ inline void stem_patch_loop(const StemPatchArgs& p, StemPatchTile<RT>& c, int n_frames, int tap0, int frame0,
                                       f32x16 (&acc)[RT][2], AtChange at_change) {
    const int n_steps = n_frames * p.kH;
    if (n_steps <= 0) return;
    float fa[RT][kStemK2], fb[2][kStemK2];
    // (the two DMA issuers are lambdas of this function, not function templates of their own: hipcc's host pass rejects calls to
    //  a function template whose body holds the LDS-DMA builtin -- "no matching function", for some instantiations only)
    // the whole patch of source frame `frame`, global -> LDS: piece q = tid + 256 i lands at As + 16 q; lanes past the patch stay
    // out of the DMA (nothing is written for them), pieces outside the image read as zero
    // (a piece outside the image keeps no select: fbase <= x_bytes < 2^31, so kStemOOB + fbase stays in [2^31, 2^32) and past the
    //  descriptor's range -- the select cost a VGPR for the constant and an SGPR pair per piece through the whole loop)
    auto dma_patch = [&](int frame) {
        const unsigned fbase = (unsigned)(c.n * p.sn + frame * p.st) * 4u;
#pragma unroll
        for (int i = 0; i < NP; ++i)
            if (c.tid + kStemNT * i < p.n_pieces)
                __builtin_amdgcn_raw_ptr_buffer_load_lds(c.rs_x, (stem_lds_ptr_t)(c.a_dst + kStemNT * i * 4), 16, c.a_src[i] + fbase, 0,
                                                         0, 0);
    };
    // filter block `step` of this workgroup's channel tile -> slot `buf`
    auto issue_b = [&](int buf, int step) {
        const unsigned tbase = (unsigned)step * c.b_step;
#pragma unroll
        for (int i = 0; i < 2; ++i)
            if (c.tid + kStemNT * i < kStemBTile / 4)
                __builtin_amdgcn_raw_ptr_buffer_load_lds(c.rs_w, (stem_lds_ptr_t)(c.b_dst + buf * kStemBTile + kStemNT * i * 4), 16,
                                                         c.b_src[i] + tbase, 0, 0, 0);
    };
    // prologue: the first patch, filter tiles 0 and 1 (kH >= 2); then the fragments of step 0
    dma_patch(frame0);
    issue_b(0, tap0 * p.kH);
    issue_b(1, tap0 * p.kH + 1);
    PTX_STEM_TL(1);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    PTX_STEM_TL(2);
    stem_patch_reads_below_barrier(c);
#pragma unroll
    for (int q = 0; q < 4; ++q) stem_patch_load_group(c, q, c.As, c.Bs + c.g * kStemBN + c.l32, fa, fb);
    int i = 0, kh = 0, slot = 0;                      // state of step s: frame, row tap, filter slot
    for (int s = 0; s < n_steps; ++s) {
        // filter tile s + 1 (issued during step s - 1) has landed for everyone; slot (s + 2) % 3 is free: its last reads
        // were issued during step s - 2 and consumed during step s - 1.  (Unconditional: at s == 0 it repeats the
        // prologue's barrier -- an `if (s > 0)` makes the compiler peel the first step, and with the fast FIR's output
        // accumulators live the peeled copy of the body spills them: 600 VGPRs.)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        int kh1 = kh + 1, i1 = i;                     // (frame, kh) of step s + 1
        if (kh1 == p.kH) { kh1 = 0; ++i1; }
        const int slot1 = slot == 2 ? 0 : slot + 1;
        const int slot2 = slot1 == 2 ? 0 : slot1 + 1;
        if (s + 2 < n_steps) issue_b(slot2, tap0 * p.kH + s + 2);     // (the steps' filter blocks are consecutive)
        const bool more = s + 1 < n_steps;
        const bool same_frame = kh1 != 0;
        const float* Bb = c.Bs + slot1 * kStemBTile + c.g * kStemBN + c.l32;
        const bool prefetch = more && same_frame;
        const float* Ab = c.As + kh1 * p.PC;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            stem_patch_mma_group(c.g, q, fa, fb, acc);
            __builtin_amdgcn_sched_barrier(0);
            if (prefetch) stem_patch_load_group(c, q, Ab, Bb, fa, fb);
            __builtin_amdgcn_sched_barrier(0);
        }
        if (more && !same_frame) {
            // frame change: every wave is done with the old patch; the next one is LDS-DMA'd, exposed (no second patch buffer
            // and no staging registers: that is what lets a third workgroup share the CU and cover the wait)
            __syncthreads();
            dma_patch(frame0 + i1);
            at_change(i);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            stem_patch_reads_below_barrier(c);
            // (the filter slot goes through an asm of its own: read as the Bb above, the compiler keeps the five fragment
            //  addresses of the prefetch alive across the frame change, where the fast FIR folds: four VGPRs at its peak)
            int slot_b = slot1;
            asm volatile("; and the filter reads" : "+s"(slot_b)::"memory");
#pragma unroll
            for (int q = 0; q < 4; ++q) stem_patch_load_group(c, q, c.As, c.Bs + slot_b * kStemBTile + c.g * kStemBN + c.l32, fa, fb);
        }
        kh = kh1; i = i1; slot = slot1;
    }
}

// ---- epilogue: bias (+ folded BN) + ReLU; lane = output channel, 16 rows per accumulator tile.  Outputs of a tile are
// consecutive in (n, to, ho, wo) raster order, so the row index is arithmetic ----
struct StemPatchEpi {
    __amdgpu_buffer_rsrc_t rs_y;
    bool relu, co_ok[2];
    float bv[2];
};

template <int RT>
__device__ inline StemPatchEpi stem_patch_epi(const StemPatchArgs& p, const StemPatchTile<RT>& c) {
    StemPatchEpi e;
    e.relu = (p.flags & PTX_EPI_RELU) != 0;
    e.rs_y = __builtin_amdgcn_make_buffer_rsrc(p.y, 0, p.y_bytes, 0x00020000);
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int co = c.nt * kStemBN + j * 32 + c.l32;
        e.co_ok[j] = co < p.ncol;
        e.bv[j] = (p.bias && e.co_ok[j]) ? p.bias[co] : 0.f;
    }
    return e;
}

// the tile's outputs of output frame `to`
template <int RT>
__device__ inline void stem_patch_store(const StemPatchArgs& p, const StemPatchTile<RT>& c, const StemPatchEpi& e, int to,
                                        const f32x16 (&acc)[RT][2]) {
    const int m_frame = (c.n * p.To + to) * c.frame_out;
    const unsigned ldy = (unsigned)p.ldy;     // (a local: read through p inside the loop it is fetched again after every store)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int co = c.nt * kStemBN + j * 32 + c.l32;
#pragma unroll
        for (int i = 0; i < RT; ++i) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                // accumulator element r of this lane belongs to tile row (r & 3) + 8 * (r >> 2) + 4 * g
                const int ml = c.m0 + c.wave * (32 * RT) + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * c.g;
                float v = acc[i][j][r] + e.bv[j];
                v = e.relu ? fmaxf(v, 0.f) : v;
                const unsigned off = ((unsigned)(m_frame + ml) * ldy + (unsigned)co) * 4u;
                __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), e.rs_y,
                                                      (e.co_ok[j] && ml < c.frame_out) ? off : kStemOOB, 0, 0);
            }
        }
    }
}

}  // namespace ptx
