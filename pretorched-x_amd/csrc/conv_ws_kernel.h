// conv_ws_kernel.h -- persistent weight-stationary tiles ("/ws") for the short-K fp32 pointwise convs.
// Included by conv_igemm.hip, which owns the tile table; stand-alone so that no instantiation of conv_igemm_kernel changes.
//
// A 1x1x1 / stride 1 conv with K = Kc <= 288 is a GEMM whose generic-tile workgroup lives for 2..16 k-steps: its first
// loads and its epilogue are as long as its main loop, and co-resident workgroups run the same phases at the same time.
// Here a workgroup ("worker") is persistent instead:
//   * worker w of column block nb owns BN output columns for the whole launch and walks the row tiles w, w + workers, ...
//     in that fixed order (no work queue: the result does not depend on the worker count or on timing);
//   * its [BN][K] filter slice is staged to LDS ONCE, as K / 32 chunk images [BN][32] -- each the generic BK = 32 B stage,
//     same 16-byte-slot XOR swizzle, so the fragment reads are conv_igemm_kernel.h's;
//   * activation rows go through a ring of two whole-K row tiles, [K / 32][BM][32] each (a chunk image is the generic A
//     stage; a chunk is the unit a later version may fetch from another frame or source), filled by LDS-DMA in 16-byte
//     pieces.  The DMA of the NEXT row tile (and this tile's residual rows) is issued before this tile's main loop, so it
//     lands under the MFMAs and the epilogue's stores retire under it; the main loop itself has no barrier;
//   * the epilogue is the row-major one (RowEpi: per-wave LDS transpose, 16-byte residual loads and stores), bias + residual
//     + ReLU in conv_epilogue's order, in a parking area of its own (the ring is live).
// The k-order of every output is the generic BK = 32 tile's (chunk, sub-step, element): results are bit-identical to the
// "/dma/re" tile of the same MFMA shape.
#pragma once
#include "conv_igemm_kernel.h"

namespace ptx {

constexpr int kWsBK = 32;                       // floats per chunk row (128 bytes: 8 swizzled 16-byte slots)
constexpr size_t kWsLdsMax = 160 * 1024;        // LDS of a CU: filter slice + ring + parking area of one worker must fit

// LDS of one worker: the filter slice [BN][K], the ring of two [BM][K] row tiles, four parking slices of the row-major epilogue
inline size_t ws_lds_bytes(int BM, int BN, int MT, int kchunks) {
    return ((size_t)kchunks * kWsBK * (BN + 2 * BM) + 4 * MT * (BN / 2 + 4)) * sizeof(float);
}

template <int BM, int BN, int MT>
struct WsGeom {
    static constexpr int NT = 256;              // four waves, 2 x 2
    static constexpr int WTM = BM / 2, WTN = BN / 2;
    static constexpr int TM = WTM / MT, TN = WTN / MT;
    static constexpr int KG = 64 / MT;          // lane groups along k
    static constexpr int KSUB = kWsBK / (4 * KG);
    static constexpr int A_IT = BM * 8 / NT, B_IT = BN * 8 / NT;      // 16-byte pieces per thread and chunk
    static constexpr int EPI_FLOATS = 4 * RowEpi<WTN, MT>::FLOATS;
    static constexpr int NSTORE = TM * RowEpi<WTN, MT>::NP;           // buffer stores per wave and row tile
    static_assert(TM * MT * 2 == BM && TN * MT * 2 == BN && A_IT >= 1 && B_IT >= 1 && KSUB % 2 == 0, "tile shape");
    static_assert(EPI_FLOATS == 4 * MT * (BN / 2 + 4), "ws_lds_bytes counts the parking slices");
    static size_t lds_bytes(int kchunks) { return ws_lds_bytes(BM, BN, MT, kchunks); }
};

// the body of one worker (a __device__ function: the kernel below only calls it, like conv_igemm_kernel its tile)
template <int BM, int BN, int MT>
__device__ __forceinline__ void conv_ws_worker(const ConvArgs& p, const int workers, float* smem) {
    using G = WsGeom<BM, BN, MT>;
    using MF = Mfma<MT>;
    using RE = RowEpi<G::WTN, MT>;
    typedef __attribute__((address_space(3))) void* lds_ptr_t;
    constexpr unsigned kOOB = 0x80000000u;
    constexpr int TM = G::TM, TN = G::TN, KG = G::KG, KSUB = G::KSUB;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    // the column blocks of one worker sit on one XCD and walk the same rows at the same time: the rows cross HBM once
    const int logical = xcd_remap((int)blockIdx.x, (int)gridDim.x);
    const int nb = logical % p.n_tiles, w = logical / p.n_tiles;
    if (w >= p.m_tiles) return;                 // a worker without a row tile
    const int n0 = nb * BN, kch = p.kchunks;
    const int ASTG = kch * BM * kWsBK;
    float* Ws = smem;                           // [kch][BN][32]
    float* As = Ws + kch * BN * kWsBK;          // [2][kch][BM][32]
    float* Es = As + 2 * ASTG + wave * RE::FLOATS;

    const __amdgpu_buffer_rsrc_t rsrc_x = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.x), 0, p.x_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rsrc_w = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.w), 0, p.w_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rs_y = __builtin_amdgcn_make_buffer_rsrc(p.y, 0, p.y_bytes, 0x00020000);
    const bool res_add = (p.flags & PTX_EPI_RES_ADD) != 0, relu = (p.flags & PTX_EPI_RELU) != 0;
    const __amdgpu_buffer_rsrc_t rsrc_r =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(res_add ? p.res : p.x), 0, res_add ? p.r_bytes : 0u, 0x00020000);

    // staging slot idx = tid + 256 i of a chunk image: row idx / 8, physical 16-byte slot idx % 8 holding the logical slot
    // (idx % 8) ^ ((row >> 1) & 7) -- the generic tile's swizzle for 128-byte rows
    auto piece_row = [&](int i) { return (tid + G::NT * i) >> 3; };
    auto piece_col = [&](int i) { const int idx = tid + G::NT * i; return ((idx & 7) ^ (((idx >> 3) >> 1) & 7)) * 4; };

    // ---- the filter slice, once ----
    {
        unsigned b_off[G::B_IT];
#pragma unroll
        for (int i = 0; i < G::B_IT; ++i) {
            const int row = n0 + piece_row(i);
            b_off[i] = row < p.w_rows ? ((unsigned)row * (unsigned)p.ldw + (unsigned)piece_col(i)) * 4u : kOOB;
        }
        for (int c = 0; c < kch; ++c)
#pragma unroll
            for (int i = 0; i < G::B_IT; ++i)
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc_w, (lds_ptr_t)(Ws + c * BN * kWsBK + (wave * 64 + G::NT * i) * 4), 16,
                                                         b_off[i] + (unsigned)(c * kWsBK * 4), 0, 0, 0);
    }
    // ---- one row tile into ring buffer `buf`: rows >= M read as zero (offset beyond the resource: no traffic) ----
    auto issue_a = [&](int t, int buf) {
        unsigned a_off[G::A_IT];
#pragma unroll
        for (int i = 0; i < G::A_IT; ++i) {
            const int m = t * BM + piece_row(i);
            a_off[i] = m < p.M ? ((unsigned)m * (unsigned)p.ldx + (unsigned)piece_col(i)) * 4u : kOOB;
        }
        float* Ab = As + buf * ASTG;
        for (int c = 0; c < kch; ++c)
#pragma unroll
            for (int i = 0; i < G::A_IT; ++i)
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc_x, (lds_ptr_t)(Ab + c * BM * kWsBK + (wave * 64 + G::NT * i) * 4), 16,
                                                         a_off[i] + (unsigned)(c * kWsBK * 4), 0, 0, 0);
    };
    issue_a(w, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");

    const int frag_sw = ((lane % MT) >> 1) & 7;
    const int frag_off_a = (wm * G::WTM + (lane % MT)) * kWsBK, frag_off_b = (wn * G::WTN + (lane % MT)) * kWsBK;
    const int cl = (lane % RE::LPR) * 4;
    const int co4 = n0 + wn * G::WTN + cl;
    f32x4 b4 = {0.f, 0.f, 0.f, 0.f};
    if (p.bias && co4 < p.ncol) b4 = *reinterpret_cast<const f32x4*>(p.bias + co4);

    int buf = 0;
    for (int t = w; t < p.m_tiles; t += workers) {
        // Everything older than the previous tile's NSTORE stores has landed -- this tile's rows were requested before them
        // (vector memory operations of a wave retire in order) -- in every wave; and every wave is done reading the other
        // ring buffer, which the next tile's DMA overwrites below.
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"(G::NSTORE) : "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        int offa = frag_off_a, offb = frag_off_b;
        post_barrier_offsets(offa, offb);
        const int mbase = t * BM + wm * G::WTM;
        f32x4 res4[TM * RE::NP];
        rowmajor_load_residual<MF, TM, TN, G::WTM, G::WTN, MT>(res4, rsrc_r, res_add, mbase, n0 + wn * G::WTN, p.M, p.ncol, p.ldr, lane);
        if (t + workers < p.m_tiles) issue_a(t + workers, buf ^ 1);

        typename MF::acc_t acc[TM][TN];
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j)
#pragma unroll
                for (int r = 0; r < MF::NACC; ++r) acc[i][j][r] = 0.f;
        const float* Ab = As + buf * ASTG + offa;
        const float* Bb = Ws + offb;
        f32x4 fa[2][TM], fb[2][TN];
        auto read_frags = [&](int c, int ks, int slot) {
            const int koff = ((ks * KG + lane / MT) ^ frag_sw) * 4;
#pragma unroll
            for (int i = 0; i < TM; ++i) fa[slot][i] = *reinterpret_cast<const f32x4*>(Ab + c * BM * kWsBK + i * MT * kWsBK + koff);
#pragma unroll
            for (int j = 0; j < TN; ++j) fb[slot][j] = *reinterpret_cast<const f32x4*>(Bb + c * BN * kWsBK + j * MT * kWsBK + koff);
        };
        read_frags(0, 0, 0);
        for (int c = 0; c < kch; ++c) {
            const int cn = c + 1 < kch ? c + 1 : c;          // (the last prefetch re-reads the last chunk: unused)
#pragma unroll
            for (int ks = 0; ks < KSUB; ++ks) {
                // the next sub-step's fragments are requested BEFORE this sub-step's MFMAs and stay in flight under them
                // (left alone, the scheduler sinks the reads below the MFMAs and a lone wave on a SIMD waits for every read)
                if (ks == KSUB - 1) read_frags(cn, 0, (ks + 1) & 1);
                else read_frags(c, ks + 1, (ks + 1) & 1);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int r = 0; r < 4; ++r)
#pragma unroll
                    for (int i = 0; i < TM; ++i)
#pragma unroll
                        for (int j = 0; j < TN; ++j) acc[i][j] = MF::mma(fa[ks & 1][i][r], fb[ks & 1][j][r], acc[i][j]);
                __builtin_amdgcn_sched_barrier(0);
            }
        }

        // ---- row-major epilogue (rowmajor_store_tile with the bias held across tiles) ----
#pragma unroll
        for (int i = 0; i < TM; ++i) {
#pragma unroll
            for (int j = 0; j < TN; ++j)
#pragma unroll
                for (int r = 0; r < MF::NACC; ++r) Es[MF::row(r, lane) * RE::LDT + j * MT + (lane % MT)] = acc[i][j][r];
#pragma unroll
            for (int ps = 0; ps < RE::NP; ++ps) {
                const int row = ps * RE::RPP + lane / RE::LPR;
                const int m = mbase + i * MT + row;
                const bool ok = co4 < p.ncol && row < MT && m < p.M;
                f32x4 v = *reinterpret_cast<const f32x4*>(Es + (row < MT ? row : 0) * RE::LDT + cl) + b4 + res4[i * RE::NP + ps];
                if (relu) { v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f); }
                const unsigned off = ((unsigned)m * (unsigned)p.ldy + (unsigned)co4) * 4u;
                __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(__attribute__((ext_vector_type(4))) unsigned, v), rs_y,
                                                       ok ? off : kOOB, 0, 0);
            }
        }
        buf ^= 1;
    }
}

template <int BM, int BN, int MT>
__global__ void __launch_bounds__(256) conv_ws_kernel(const ConvArgs p, const int workers) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    conv_ws_worker<BM, BN, MT>(p, workers, smem);
}

}  // namespace ptx
