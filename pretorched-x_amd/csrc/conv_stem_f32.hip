// RGB stem convolution on the fp32 matrix cores, straight from the caller's NCDHW tensor:
// Conv3d(3, 64, 7, stride (1,2,2), pad 3) + BN + ReLU of the ResNet3D family (resnet3D.py:153-155), the 2-D ResNet stem
// (torchvision_models.py), the (1,7,7) spatial stem of the (2+1)D nets (r2plus1d.py:73-88), the SAME-padded I3D stem.
//
// Why a dedicated kernel.  On the generic implicit-GEMM tiles the stem is a (7,7,1) conv over a kW-FOLDED copy of the
// input (ptx_fold_kw_ncdhw: 77 MB -> 308 MB at config 2), and every (kt, kh) tap re-stages its A tile global -> VGPR ->
// LDS behind a barrier: the fp32 MFMA pipe sits at 75 %, plus the 82 us fold pass.  Here a workgroup (4
// waves x 64 rows) owns 256 consecutive outputs of one output frame and runs the patch-resident step loop of
// conv_stem_patch_f32.h over that frame's valid temporal taps, one source frame per tap.  LDS per workgroup = the patch +
// three 5.5 KiB filter slots (53 KB at config 2), 144 VGPRs: THREE workgroups share a CU -- what took the kernel from 1.76 to
// 1.55 ms.
// This file: the order workgroups take their tiles in, the temporal pruning, the filter pack, the entry points.
#include "ptx_common.h"

// Phase clock of a workgroup (diagnostic build only: scripts/micro/build_timeline.sh, -DPTX_STEM_TIMELINE; the product library
// carries none of it): thread 0 writes the 100 MHz wall clock at 0 entry, 1 requests issued, 2 first patch landed, 3 last
// step done, 5 stores retired; 6 = __smid().
#ifdef PTX_STEM_TIMELINE
namespace ptx {
__device__ unsigned long long* g_stem_tl = nullptr;
}
#define PTX_STEM_TL(k)                                                                                                 \
    do {                                                                                                               \
        if (threadIdx.x == 0 && g_stem_tl)                                                                             \
            g_stem_tl[(size_t)(blockIdx.y * gridDim.x + blockIdx.x) * 8 + (k)] =                                       \
                (k) == 6 ? (unsigned long long)__smid() : (unsigned long long)wall_clock64();                          \
    } while (0)
#endif
#include "conv_stem_patch_f32.h"

namespace ptx {

struct StemF32Args {
    StemPatchArgs s;      // x: the caller's tensor; w: [kT*kH][w_tiles][11][2][64]
    int Ti, kT, sT, pT;
    // longest-first tile order inside an XCD's chunk (0 = plain order): output frames grouped by their number of valid
    // temporal taps, most taps first -- the workgroups that finish a launch are the short ones
    int lpt, n_classes, groups_per_xcd;
    unsigned char cls_start[10];      // first entry of class k in `order` (n_classes + 1 entries)
    unsigned char order[64];          // output frames sorted by (taps desc, frame asc)
};

constexpr int kF32RT = 2;                           // 64 rows per wave
constexpr int kF32Rows = 4 * 32 * kF32RT;           // outputs per workgroup

// NP: 16-byte patch pieces per thread (4, 8 or 12)
template <int NP>
// (flatten: see conv_stem_patch_f32.h on how its functions are inlined)
__global__ void __launch_bounds__(kStemNT, 2) __attribute__((flatten)) conv_stem_f32_kernel(const StemF32Args p) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    PTX_STEM_TL(0);
    PTX_STEM_TL(6);
    // tile order: the frames of one band of rows follow each other (temporal L2 reuse of the kT-frame window), an XCD
    // owns a contiguous chunk of the list
    int to, t_;                                         // output frame, (n, band) group
    if (p.lpt) {
        const int xcd = blockIdx.x % kNumXCD, l = blockIdx.x / kNumXCD;      // workgroup b runs on XCD b % 8
        int k = 0;
        while (k + 1 < p.n_classes && l >= (int)p.cls_start[k + 1] * p.groups_per_xcd) ++k;
        const int first = p.cls_start[k], cnt = p.cls_start[k + 1] - first;
        const int idx = l - first * p.groups_per_xcd;
        const int grp = idx / cnt;
        to = p.order[first + (idx - grp * cnt)];
        t_ = xcd * p.groups_per_xcd + grp;
    } else {
        const int tile = xcd_remap(blockIdx.x, p.s.n_tiles);
        to = tile % p.s.To;
        t_ = tile / p.s.To;
    }
    // (uniform, but they come out of byte loads, which are vector loads: said once here, or everything computed from them --
    //  the step count, the filter tile of a step -- stays in vector registers and VALU instructions through the loop)
    to = __builtin_amdgcn_readfirstlane(to);
    StemPatchTile<kF32RT> c;
    stem_patch_tile<kF32RT, NP>(p.s, smem, t_ % p.s.tiles_per_frame, t_ / p.s.tiles_per_frame, c);

    // ---- valid temporal taps (uniform): frames outside the clip contribute nothing ----
    const int t_first = to * p.sT - p.pT;
    const int kt_lo = max(0, -t_first), kt_hi = min(p.kT - 1, p.Ti - 1 - t_first);

    f32x16 acc[kF32RT][2];
#pragma unroll
    for (int i = 0; i < kF32RT; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    // one step per (kt, kh) tap; nothing to do between the frames of an output frame
    stem_patch_loop<kF32RT, NP>(p.s, c, kt_hi - kt_lo + 1, kt_lo, t_first + kt_lo, acc, [](int) {});

    PTX_STEM_TL(3);
    stem_patch_store(p.s, c, stem_patch_epi(p.s, c), to, acc);
#ifdef PTX_STEM_TIMELINE
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    PTX_STEM_TL(5);
#endif
}

// folded K-major filter [tap][Co_pad][Kc] (k = kw * 3 + c, ptx_pack_conv_weight with fold_kw = 1) -> the stem's
// [tap][Co_pad / 64][11][2][64] blocks
__global__ void __launch_bounds__(256) pack_stem_f32_kernel(const float* __restrict__ wf, float* __restrict__ out, int taps,
                                                            int Co_pad, int Kc, int total) {
    for (int i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256) {
        const int col = i & 63;
        int r = i >> 6;
        const int g = r & 1;
        r >>= 1;
        const int j = r % kStemK2;
        r /= kStemK2;
        const int tiles = Co_pad / kStemBN;
        const int nt = r % tiles;
        const int tap = r / tiles;
        int c, kw;
        if (j < 9) { c = j / 3; kw = 2 * (j % 3) + g; }
        else if (j == 9) { c = g; kw = 6; }
        else { c = 2; kw = 6; }
        const bool zero = j == 10 && g == 1;
        out[i] = zero ? 0.f : wf[((size_t)tap * Co_pad + nt * kStemBN + col) * Kc + kw * 3 + c];
    }
}

}  // namespace ptx

using namespace ptx;

#ifdef PTX_STEM_TIMELINE
extern "C" int ptx_stem_f32_timeline(void* buf) {  // diagnostic build only: 8 x u64 per workgroup, or NULL to switch off
    return hip_check(hipMemcpyToSymbol(HIP_SYMBOL(g_stem_tl), &buf, sizeof(buf)), "ptx_stem_f32_timeline");
}
#endif

extern "C" int ptx_conv_stem_f32_supported(const ptx_conv3d_desc* d, int64_t stride_n, int64_t stride_c, int64_t stride_t) {
    if (!d) return 0;
    if (d->flags & ~PTX_EPI_RELU) return 0;
    if (d->Ci != 3 || d->kW != 7 || d->kT < 1 || d->kT > 8 || d->kH < 2 || d->kH > 8 || d->groups > 1 || d->Co_pad % kStemBN) return 0;
    if (d->sW < 1 || d->sW > 2 || d->sH < 1 || d->sT < 1 || d->Wo < 1 || d->Ho < 1 || d->To < 1 || d->pW < 0 || d->pW > 8) return 0;
    const int pitch = d->ldx > 0 ? d->ldx : d->Wi;             // floats per input row
    if (pitch % 4 || pitch < d->Wi || stride_n % 4 || stride_c % 4 || stride_t % 4) return 0;   // 16-byte DMA pieces of NCDHW rows
    // a plane inside its channel, a channel inside its sample: the buffer descriptor's range is derived from these
    const int64_t chan_extent = (int64_t)(d->Ti - 1) * stride_t + (int64_t)d->Hi * pitch;
    if (stride_t < (int64_t)d->Hi * pitch || stride_c < chan_extent || stride_n < 2 * stride_c + chan_extent) return 0;
    StemPatchGeom g;
    if (!stem_patch_geom(d, kF32Rows, &g)) return 0;
    if (((int64_t)(d->N - 1) * stride_n + 3 * stride_c) * 4 >= 0x80000000LL ||
        (int64_t)d->N * d->To * d->Ho * d->Wo * d->ldy * 4 >= 0x80000000LL)
        return 0;
    auto extent_ok = [](int in, int out, int k, int s, int p) {
        if (out == (in + 2 * p - k) / s + 1) return true;
        const int same = (in + s - 1) / s;
        const int total = std::max((same - 1) * s + k - in, 0);
        return out == same && p == total / 2;
    };
    if (!extent_ok(d->Wi, d->Wo, d->kW, d->sW, d->pW) || !extent_ok(d->Hi, d->Ho, d->kH, d->sH, d->pH) ||
        !extent_ok(d->Ti, d->To, d->kT, d->sT, d->pT))
        return 0;
    return 1;
}

extern "C" size_t ptx_stem_f32_weight_elems(const ptx_conv3d_desc* d) {
    if (!d || d->Co_pad <= 0 || d->Co_pad % kStemBN || d->kT <= 0 || d->kH <= 0) return 0;
    return (size_t)d->kT * d->kH * (d->Co_pad / kStemBN) * kStemBTile;
}

extern "C" int ptx_pack_stem_f32_weight(const ptx_conv3d_desc* d, const float* w_folded, int Kc, float* w_stem, ptx_stream_t stream) {
    if (!d || !w_folded || !w_stem) return fail(PTX_ERR_INVALID, "pack_stem_f32: null pointer");
    if (d->Ci != 3 || d->kW != 7 || Kc < 21 || d->Co_pad % kStemBN || d->kT <= 0 || d->kH <= 0)
        return fail(PTX_ERR_UNSUPPORTED, "pack_stem_f32: a folded 3-channel, kW = 7 filter with rows of >= 21 floats");
    const size_t total = ptx_stem_f32_weight_elems(d);
    if (total >= (1ull << 31)) return fail(PTX_ERR_UNSUPPORTED, "pack_stem_f32: filter too large");
    hipLaunchKernelGGL(pack_stem_f32_kernel, dim3((unsigned)std::min<size_t>(cdiv(total, 256), 4096)), dim3(256), 0, (hipStream_t)stream,
                       w_folded, w_stem, d->kT * d->kH, d->Co_pad, Kc, (int)total);
    return hip_check(hipGetLastError(), "pack_stem_f32 launch");
}

extern "C" int ptx_conv_stem_f32_fwd(const ptx_conv3d_desc* d, const float* x, int64_t stride_n, int64_t stride_c, int64_t stride_t,
                                     const float* w_stem, const float* bias, float* y, ptx_stream_t stream) {
    if (!d || !x || !w_stem || !y) return fail(PTX_ERR_INVALID, "conv_stem_f32: null pointer");
    if (((uintptr_t)x | (uintptr_t)w_stem | (uintptr_t)y) & 15) return fail(PTX_ERR_INVALID, "conv_stem_f32: pointers must be 16-byte aligned");
    if (!ptx_conv_stem_f32_supported(d, stride_n, stride_c, stride_t))
        return fail(PTX_ERR_UNSUPPORTED, "conv_stem_f32: needs a 3-channel NCDHW input (row pitch and strides multiples of 4 floats), kW == 7, "
                    "stride_w <= 2, symmetric or SAME padding, only the ReLU epilogue, and an input patch of at most %d floats", kStemPatchMax);
    if (d->ldy < d->Co || d->ldy % 4) return fail(PTX_ERR_INVALID, "conv_stem_f32: bad output stride");
    StemF32Args a{};
    stem_patch_fill(a.s, d, kF32Rows, d->N * d->To, x, stride_n, stride_c, stride_t,
                    ((uint64_t)(d->N - 1) * stride_n + 3ull * stride_c) * 4ull, w_stem, ptx_stem_f32_weight_elems(d) * 4ull, bias, y);
    a.Ti = d->Ti; a.kT = d->kT; a.sT = d->sT; a.pT = d->pT;
    {
        const int groups = d->N * a.s.tiles_per_frame;
        static const bool lpt_env = !(getenv("PTX_STEM_F32_LPT") && atoi(getenv("PTX_STEM_F32_LPT")) == 0);
        if (lpt_env && d->To <= 64 && d->To > 1 && groups % kNumXCD == 0) {
            int taps[64], idx[64];
            for (int to = 0; to < d->To; ++to) {
                const int t0 = to * d->sT - d->pT;
                taps[to] = std::max(0, std::min(d->kT - 1, d->Ti - 1 - t0) - std::max(0, -t0) + 1);
                idx[to] = to;
            }
            std::stable_sort(idx, idx + d->To, [&](int x, int y) { return taps[x] > taps[y]; });
            int nc = 0;
            for (int i = 0; i < d->To; ++i) {
                a.order[i] = (unsigned char)idx[i];
                if (i == 0 || taps[idx[i]] != taps[idx[i - 1]]) {
                    if (nc < 9) a.cls_start[nc++] = (unsigned char)i;
                    else { nc = 99; break; }
                }
            }
            if (nc > 1 && nc <= 9) {          // (one class: nothing to reorder)
                a.cls_start[nc] = (unsigned char)d->To;
                a.n_classes = nc;
                a.groups_per_xcd = groups / kNumXCD;
                a.lpt = 1;
            }
        }
    }
    const int np = cdiv(a.s.n_pieces, kStemNT);             // pieces per thread: 4 / 8 / 12
    const int rc = np <= 4 ? stem_patch_launch<&conv_stem_f32_kernel<4>>(a, a.s, stream)
                 : np <= 8 ? stem_patch_launch<&conv_stem_f32_kernel<8>>(a, a.s, stream)
                           : stem_patch_launch<&conv_stem_f32_kernel<12>>(a, a.s, stream);
    if (rc != PTX_OK) return rc;
    return hip_check(hipGetLastError(), "conv_stem_f32 launch");
}
