// RGB stem convolution on the bf16 matrix cores, input patch resident in LDS: Conv3d(3, 64, 7, stride (1,2,2), pad 3) +
// BN + ReLU of the ResNet3D family (resnet3D.py:153-155) and the (1,7,7) spatial stem of the (2+1)D nets
// (r2plus1d.py:73-88), for bf16 plans.  The fold path (ptx_im2col_hw_bf16 + a (kT,1,1) conv on the generic bf16 tiles)
// writes a 160-channel copy of the clip and reads it back; this kernel reads the clip once, from one of two sources:
//     PTX_STEM_SRC_BF16_NCDHW   the caller's contiguous bf16 clip [N][3][T][H][W], any 2-byte alignment
//     PTX_STEM_SRC_U8_NTHWC     decoded uint8 frames [N][T][H][W][3], any byte alignment, normalised while staged: the
//                               operand is bf16_rne(normalise_u8(pixel)) with the BGR swap of ptx_frames_u8_to_ncdhw --
//                               exactly PTX_RESIZE_OUT_BF16's value (a 3 x 256 table built per workgroup in LDS)
//
// Structure.  A workgroup (4 waves) owns up to 256 consecutive outputs of one output frame x 64 output channels.  Per
// temporal tap inside the clip (taps outside are skipped, not multiplied by zero) it stages the input patch ONCE, through
// registers (both sources need a conversion / an interleave: no LDS-DMA), as PIXEL-INTERLEAVED bf16 (c0, c1, c2, 0) -- 8
// bytes per pixel, zero outside the image -- and serves all kH x kW taps from it.  Patch column 0 is input column -pW of
// the tile's first output column, so the window of output column wo starts at pixel wo * 2: a 16-byte boundary.
//
// K axis of one (kt, kh) step: 8 pixels x 4 channels = 32 = ONE v_mfma_f32_16x16x32_bf16 k-step.  A lane's 8 consecutive
// k (k = 8 (lane / 16) + e) are the two adjacent pixels 2 (lane / 16) + (e >> 2), channel e & 3: ONE ds_read_b128, and
// consecutive output columns (stride 2) read consecutive 16-byte pieces -- conflict-free.  Filter entries of channel 3
// and of kw >= kW are zero, so the issued work is 32 / 21 of the algorithmic MACs (kW = 7).
// The MFMA's A operand is the FILTER (rows = output channels), B the activations (columns = output positions): a lane's
// four accumulator registers are then four consecutive channels of one position -- one 8-byte bf16 store, four times
// fewer store instructions than channel-on-lane.
// Shape: 16x16x32, not 32x32x16 -- per 64 x 64 wave tile and step both need 8 ds_read_b128 and the same matrix-core
// cycles, but the 16-row A tile gives the channel axis a granule of 16: the (2+1)D stems' ragged widths issue 112
// channels for 110 (and 96 for 83) instead of 128, the MFMAs of the unused 16-channel tiles of the last channel tile are
// skipped.  (32x32x16 was not built into the library, so there is no A/B of the two shapes.)
// The filter of step s + 1 (4 KiB: one 16-byte piece per thread, stored by ptx_pack_stem_bf16_weight in fragment order)
// travels global -> VGPR during step s and lands in the other of two LDS slots before the step's closing barrier.
//
// Tiling.  Normally a tile is a raster run of 256 outputs and the patch spans full input rows.  When that patch would not
// fit (wide frames, tall filters) a tile is a segment of <= 256 outputs of ONE output row, and the kH taps are staged in
// chunks of as many patch rows as fit -- any T, H, W, kH, kT runs.
// Arithmetic: bf16 operands, fp32 accumulate, bias (+ ReLU) in fp32, one round-to-nearest-even to bf16 per output (NaN
// kept).  Output: bf16 NDHWC, channels [Co, ldy) written as zero.  All global addressing is 64-bit per frame plus a
// 32-bit offset inside one frame (ptx_conv_stem_bf16_supported refuses frames past that).
// Frame sub-sampling (ptx_conv_stem_bf16_strided_fwd, include/ptx_amd_stem_strided.h: SlowFast's pathways read
// input[:, :, ::step]): the source holds T_full frames and conv frame t is source frame t * frame_step -- a stride in the
// 64-bit frame base of the staging loop, nothing else changes.  The stride is a template flag: the plain entry point (and
// frame_step == 1) runs the instances without it, whose machine code is the one it had before the flag existed -- one
// kernel for both measured 0.6 % slower on the plain path (0.3328 against 0.3306 ms at resnet3d50's config-2 stem, two
// copies of the old library agreeing to 0.0001 ms), with an instruction stream that differed by one scalar load and one
// multiply: the hot loop's placement, not its work.
// Compiled as part of pack_layout.hip's translation unit (its last line includes this file), like resize_views.hip.
#include "resize_common.h"
#include "../../include/ptx_amd_stem_strided.h"

namespace ptx {

typedef __bf16 sb_bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned int sb_u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int sb_u32x2 __attribute__((ext_vector_type(2)));

constexpr int kSbNT = 256;                  // 4 waves x 64 outputs
constexpr int kSbRows = 256;                // outputs per workgroup
constexpr int kSbBN = 64;                   // output channels per workgroup
constexpr int kSbPatchMax = 40960;          // bytes of the patch buffer
constexpr int kSbWSlot = 4 * 64 * 8;        // bf16 elements of one (step, channel tile) filter block: 4 KiB

struct StemBf16Args {
    const void* x;
    const unsigned short* w;      // [kT*kH][w_tiles][4 channel tiles of 16][64 lanes][8]
    const float* bias;
    unsigned short* y;            // [N][To][Ho][Wo][ldy] bf16
    ptx_norm_desc norm;
    int N, Ti, Hi, Wi, To, Ho, Wo, ldy, Co;
    int kT, kH, sT, sH, sW, pT, pH, pW;
    int row_mode, segs;           // a tile is a segment of one output row (segs per row) | a raster run of the frame
    int PR, PC, khc;              // patch rows, patch pixels per row (even), kh taps staged together
    int tiles_per_frame, n_tiles, w_tiles;
    unsigned flags;
    unsigned dv_wo[2], dv_pc2[2];
    int frame_step, T_full;       // STRIDED instances: conv frame t = source frame t * frame_step of T_full (last: the plain
                                  // instances never read them and keep the argument layout they had)
};

__device__ __forceinline__ unsigned short sb_bf16_bits(float v) { return __builtin_bit_cast(unsigned short, (__bf16)v); }

template <int SRC, bool STRIDED>
__global__ void __launch_bounds__(kSbNT, 2) conv_stem_bf16_kernel(const StemBf16Args p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char sb_smem[];
    const int patch_bytes = p.PR * p.PC * 8;
    unsigned char* Ps = sb_smem;                                                       // the patch: [PR][PC] pixels of 8 bytes
    unsigned short* Ws = reinterpret_cast<unsigned short*>(sb_smem + patch_bytes);     // [2][kSbWSlot]
    unsigned short* lut = Ws + 2 * kSbWSlot;                                           // [3][256] (uint8 source)

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 15, g = lane >> 4;
    const int nt = blockIdx.y;

    // tile order: the output frames of one band follow each other (temporal L2 reuse of the kT-frame window)
    const int tile = xcd_remap(blockIdx.x, p.n_tiles);
    const int to = tile % p.To;
    const int t_ = tile / p.To;
    const int band = t_ % p.tiles_per_frame;
    const int n = t_ / p.tiles_per_frame;
    const int frame_out = p.Ho * p.Wo;
    int ho_a, wo_a, m0 = 0;                               // first output row / column of the tile
    if (p.row_mode) {
        ho_a = band / p.segs;
        wo_a = (band - ho_a * p.segs) * kSbRows;
    } else {
        m0 = band * kSbRows;
        ho_a = (int)fdiv((unsigned)m0, p.dv_wo);
        wo_a = 0;
    }

    if (SRC == PTX_STEM_SRC_U8_NTHWC) {
#pragma unroll
        for (int c = 0; c < 3; ++c) lut[c * 256 + tid] = sb_bf16_bits(normalise_u8((unsigned char)tid, p.norm.mean[c], p.norm.std[c], p.norm.to_255));
        __syncthreads();
    }

    // ---- this lane's four output positions (position tile j): patch pixel of the window start, raster index ----
    int boff[4], mout[4];
    bool pos_ok[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int idx = wave * 64 + j * 16 + r;
        int ho, wo;
        if (p.row_mode) {
            pos_ok[j] = wo_a + idx < p.Wo;
            ho = ho_a;
            wo = pos_ok[j] ? wo_a + idx : wo_a;
        } else {
            pos_ok[j] = m0 + idx < frame_out;
            const int mm = pos_ok[j] ? m0 + idx : m0;
            ho = (int)fdiv((unsigned)mm, p.dv_wo);
            wo = mm - ho * p.Wo;
        }
        boff[j] = (ho - ho_a) * p.sH * p.PC + (wo - wo_a) * p.sW + 2 * g;
        mout[j] = ho * p.Wo + wo;
    }

    // ---- valid temporal taps (uniform): frames outside the clip contribute nothing ----
    const int t_first = to * p.sT - p.pT;
    const int kt_lo = max(0, -t_first), kt_hi = min(p.kT - 1, p.Ti - 1 - t_first);
    const int n_kt = max(0, kt_hi - kt_lo + 1);
    const int n_steps = n_kt * p.kH;

    const size_t HW = (size_t)p.Hi * p.Wi;
    const int pc2 = p.PC >> 1, npairs = p.PR * pc2;
    const int w0 = wo_a * p.sW - p.pW;

    // the patch of input frame t, rows from h0: pixel pairs (16 bytes) through registers
    auto stage = [&](int t, int h0) {
        // source frame and frames per clip: t * frame_step < T_full (Ti == ceil(T_full / frame_step)) | t of Ti
        const size_t ts = STRIDED ? (size_t)t * p.frame_step : (size_t)t;
        const int tf = STRIDED ? p.T_full : p.Ti;
        const unsigned short* xb = static_cast<const unsigned short*>(p.x) + ((size_t)n * 3 * tf + ts) * HW;
        const unsigned char* fb = static_cast<const unsigned char*>(p.x) + ((size_t)n * tf + ts) * HW * 3;
        const size_t cs = (size_t)tf * HW;
        for (int u = tid; u < npairs; u += kSbNT) {
            const int pr = (int)fdiv((unsigned)u, p.dv_pc2);
            const int hh = h0 + pr, ww = w0 + 2 * (u - pr * pc2);
            const bool hok = (unsigned)hh < (unsigned)p.Hi;
            const bool ok0 = hok && (unsigned)ww < (unsigned)p.Wi, ok1 = hok && (unsigned)(ww + 1) < (unsigned)p.Wi;
            unsigned v[2][3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                if (SRC == PTX_STEM_SRC_U8_NTHWC) {
                    const int cin = (p.norm.swap_rb && c != 1) ? 2 - c : c;
                    const int off = (hh * p.Wi + ww) * 3 + cin;
                    v[0][c] = ok0 ? lut[c * 256 + fb[off]] : 0u;
                    v[1][c] = ok1 ? lut[c * 256 + fb[off + 3]] : 0u;
                } else {
                    const unsigned short* xc = xb + c * cs;
                    const int off = hh * p.Wi + ww;
                    v[0][c] = ok0 ? xc[off] : 0u;
                    v[1][c] = ok1 ? xc[off + 1] : 0u;
                }
            }
            const sb_u32x4 o = {v[0][0] | (v[0][1] << 16), v[0][2], v[1][0] | (v[1][1] << 16), v[1][2]};
            *reinterpret_cast<sb_u32x4*>(Ps + (size_t)u * 16) = o;
        }
    };
    auto load_w = [&](int step) {
        return *reinterpret_cast<const sb_u32x4*>(p.w + ((size_t)step * p.w_tiles + nt) * kSbWSlot + tid * 8);
    };

    // 16-channel A tiles of this channel tile that hold channels below ldy (uniform): the others issue nothing
    const int n_at = min(4, (p.ldy - nt * kSbBN + 15) >> 4);
    f32x4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[i][j][e] = 0.f;

    if (n_steps > 0) *reinterpret_cast<sb_u32x4*>(Ws + tid * 8) = load_w(kt_lo * p.kH);
    int s = 0;
    for (int ikt = 0; ikt < n_kt; ++ikt) {
        for (int kh0 = 0; kh0 < p.kH; kh0 += p.khc) {
            // every wave is past the closing barrier of the last step: the old patch is free
            stage(t_first + kt_lo + ikt, ho_a * p.sH - p.pH + kh0);
            __syncthreads();
            const int kh1 = min(p.kH, kh0 + p.khc);
            for (int kh = kh0; kh < kh1; ++kh, ++s) {
                const bool more = s + 1 < n_steps;
                sb_u32x4 wn = {0u, 0u, 0u, 0u};
                if (more) wn = load_w(kt_lo * p.kH + s + 1);
                const unsigned short* Wb = Ws + (s & 1) * kSbWSlot + lane * 8;
                const unsigned char* Pb = Ps + (size_t)((kh - kh0) * p.PC) * 8;
                sb_bf16x8 a[4], b[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) a[i] = *reinterpret_cast<const sb_bf16x8*>(Wb + i * 512);
#pragma unroll
                for (int j = 0; j < 4; ++j) b[j] = *reinterpret_cast<const sb_bf16x8*>(Pb + (size_t)boff[j] * 8);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    if (i < n_at) {
#pragma unroll
                        for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[i], b[j], acc[i][j], 0, 0, 0);
                    }
                }
                // slot (s + 1) & 1 was last read during step s - 1, which every wave left through that step's barrier
                if (more) *reinterpret_cast<sb_u32x4*>(Ws + ((s + 1) & 1) * kSbWSlot + tid * 8) = wn;
                __syncthreads();
            }
        }
    }

    // ---- epilogue: accumulator element e of tile (i, j) is channel i*16 + 4 (lane / 16) + e of position j*16 + lane % 16:
    // a lane's four registers = four consecutive channels, one 8-byte store ----
    const bool relu = (p.flags & PTX_EPI_RELU) != 0;
    unsigned short* yb = p.y + ((size_t)n * p.To + to) * (size_t)frame_out * p.ldy;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int c0 = nt * kSbBN + i * 16 + 4 * g;
        if (c0 >= p.ldy) continue;
        float bv[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) bv[e] = (p.bias && c0 + e < p.Co) ? p.bias[c0 + e] : 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (!pos_ok[j]) continue;
            unsigned o[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float v = acc[i][j][e] + bv[e];
                v = relu ? fmaxf(v, 0.f) : v;
                o[e] = c0 + e < p.Co ? (unsigned)sb_bf16_bits(v) : 0u;
            }
            const sb_u32x2 st = {o[0] | (o[1] << 16), o[2] | (o[3] << 16)};
            *reinterpret_cast<sb_u32x2*>(yb + (size_t)mout[j] * p.ldy + c0) = st;
        }
    }
}

// ptx_pack_conv_weight(PTX_PACK_BF16) of the (kh, kw)-folded filter, [kT][Co_pad][Kc] with k = (kh*kW + kw)*3 + c  ->  the
// stem's fragment-ordered blocks: bit-exact moves of the once-rounded values
__global__ void __launch_bounds__(256) pack_stem_bf16_kernel(const unsigned short* __restrict__ wf, unsigned short* __restrict__ out,
                                                             int kH, int kW, int Co_pad, int Kc, size_t total) {
    for (size_t o = (size_t)blockIdx.x * 256 + threadIdx.x; o < total; o += (size_t)gridDim.x * 256) {
        const int e = (int)(o & 7), lane = (int)(o >> 3) & 63, i = (int)(o >> 9) & 3;
        size_t rest = o >> 11;
        const int tiles = Co_pad / kSbBN;
        const int nt = (int)(rest % tiles);
        const int step = (int)(rest / tiles);
        const int kt = step / kH, kh = step - kt * kH;
        const int co = nt * kSbBN + i * 16 + (lane & 15);
        const int kw = 2 * (lane >> 4) + (e >> 2), c = e & 3;
        out[o] = (c < 3 && kw < kW) ? wf[((size_t)kt * Co_pad + co) * Kc + (kh * kW + kw) * 3 + c] : (unsigned short)0;
    }
}

struct StemBf16Geom {
    int row_mode, segs, PR, PC, khc, tiles_per_frame;
};

// host-side twin: steps.StemBf16Step.issued_flop walks the same tiles
static void stem_bf16_geom(const ptx_conv3d_desc* d, StemBf16Geom* g) {
    const int nrows = std::min(d->Ho, (kSbRows - 1 + d->Wo - 1) / d->Wo + 1);     // rows a raster run of 256 outputs can touch
    const int64_t pc_full = (int64_t)(d->Wo - 1) * d->sW + 8;
    const int64_t pr_full = (int64_t)(nrows - 1) * d->sH + d->kH;
    if (pr_full * pc_full * 8 <= kSbPatchMax) {
        g->row_mode = 0; g->segs = 1;
        g->PR = (int)pr_full; g->PC = (int)pc_full; g->khc = d->kH;
        g->tiles_per_frame = cdiv(d->Ho * d->Wo, kSbRows);
        return;
    }
    g->row_mode = 1;
    g->segs = cdiv(d->Wo, kSbRows);
    g->PC = (std::min(d->Wo, kSbRows) - 1) * d->sW + 8;
    g->khc = std::min(d->kH, kSbPatchMax / (g->PC * 8));
    g->PR = g->khc;
    g->tiles_per_frame = d->Ho * g->segs;
}

static int sb_refuse(const char* why) {
    fail(PTX_ERR_UNSUPPORTED, "conv_stem_bf16: %s", why);
    return 0;
}

}  // namespace ptx

using namespace ptx;

extern "C" int ptx_conv_stem_bf16_supported(const ptx_conv3d_desc* d, int32_t src) {
    if (!d) return sb_refuse("null descriptor");
    if (src != PTX_STEM_SRC_BF16_NCDHW && src != PTX_STEM_SRC_U8_NTHWC) return sb_refuse("unknown source (PTX_STEM_SRC_*)");
    if (d->flags & ~(PTX_EPI_RELU | PTX_F16_OPERANDS | PTX_BF16_OPERANDS | PTX_EPI_OUT_F16)) return sb_refuse("only the ReLU epilogue is fused");
    if (d->Ci != 3) return sb_refuse("needs a 3-channel input (Ci == 3)");
    if (d->kW < 1 || d->kW > 8) return sb_refuse("filter width must be 1..8 (one 8-pixel K step per tap row)");
    if (d->sW != 2) return sb_refuse("stride_w must be 2 (window starts land on 16-byte patch pieces)");
    if (d->groups > 1) return sb_refuse("grouped stems are not supported");
    if (d->N < 1 || d->Ti < 1 || d->Hi < 1 || d->Wi < 1 || d->To < 1 || d->Ho < 1 || d->Wo < 1 || d->Co < 1) return sb_refuse("non-positive extent");
    if (d->kT < 1 || d->kH < 1 || d->sT < 1 || d->sH < 1 || d->pT < 0 || d->pH < 0 || d->pW < 0) return sb_refuse("bad filter / stride / padding");
    if (d->Co_pad < d->Co || d->Co_pad % kSbBN) return sb_refuse("Co_pad must cover Co in whole 64-channel tiles");
    if (d->ldy < d->Co || d->ldy % 8 || d->ldy > d->Co_pad) return sb_refuse("ldy must cover Co, be a multiple of 8 bf16 and stay within Co_pad");
    auto sym = [](int64_t in, int out, int k, int s, int pad) { return in + 2 * pad >= k && out == (in + 2 * pad - k) / s + 1; };
    if (!sym(d->Wi, d->Wo, d->kW, d->sW, d->pW) || !sym(d->Hi, d->Ho, d->kH, d->sH, d->pH) || !sym(d->Ti, d->To, d->kT, d->sT, d->pT))
        return sb_refuse("output extents are not those of symmetric padding (SAME-padded stems are not supported)");
    // addressing: 64-bit per frame, 32-bit inside one input / output frame
    if ((int64_t)d->Hi * d->Wi * 3 >= 0x7fffffffLL) return sb_refuse("one input frame exceeds 2^31 elements");
    if ((int64_t)d->Ho * d->Wo * d->ldy * 2 >= 0x7fffffffLL) return sb_refuse("one output frame exceeds 2 GiB");
    if ((int64_t)d->kT * d->kH >= (1 << 20)) return sb_refuse("filter too large");
    StemBf16Geom g;
    stem_bf16_geom(d, &g);
    if ((int64_t)d->N * d->To * g.tiles_per_frame >= 0x7fffffffLL) return sb_refuse("too many tiles for one launch");
    return 1;
}

extern "C" size_t ptx_stem_bf16_weight_elems(const ptx_conv3d_desc* d) {
    if (!d || d->Co_pad <= 0 || d->Co_pad % kSbBN || d->kT <= 0 || d->kH <= 0) return 0;
    return (size_t)d->kT * d->kH * (d->Co_pad / kSbBN) * kSbWSlot;
}

extern "C" int ptx_pack_stem_bf16_weight(const ptx_conv3d_desc* d, const void* w_packed, void* w_stem, ptx_stream_t stream) {
    if (!d || !w_packed || !w_stem) return fail(PTX_ERR_INVALID, "pack_stem_bf16: null pointer");
    if (d->Ci != 3 || d->kW < 1 || d->kW > 8 || d->Co_pad <= 0 || d->Co_pad % kSbBN || d->kT <= 0 || d->kH <= 0)
        return fail(PTX_ERR_UNSUPPORTED, "pack_stem_bf16: a 3-channel filter with kW <= 8 and Co_pad in whole 64-channel tiles");
    if (((uintptr_t)w_packed & 1) || ((uintptr_t)w_stem & 15)) return fail(PTX_ERR_INVALID, "pack_stem_bf16: misaligned pointer");
    const size_t total = ptx_stem_bf16_weight_elems(d);
    const int Kc = (d->kH * d->kW * 3 + 31) / 32 * 32;          // row length of the (kh, kw)-folded bf16 filter
    hipLaunchKernelGGL(pack_stem_bf16_kernel, dim3((unsigned)std::min<size_t>((total + 255) / 256, 4096)), dim3(256), 0, (hipStream_t)stream,
                       static_cast<const unsigned short*>(w_packed), static_cast<unsigned short*>(w_stem), d->kH, d->kW, d->Co_pad, Kc, total);
    return hip_check(hipGetLastError(), "pack_stem_bf16 launch");
}

extern "C" int ptx_conv_stem_bf16_strided_supported(const ptx_conv3d_desc* d, int32_t src, int32_t frame_step, int32_t T_full) {
    if (!d) return sb_refuse("null descriptor");
    if (frame_step < 1) return sb_refuse("frame_step must be >= 1");
    if (T_full < 1 || (int64_t)d->Ti != ((int64_t)T_full + frame_step - 1) / frame_step)
        return sb_refuse("Ti must be ceil(T_full / frame_step): the frames 0, frame_step, 2 frame_step, .. of the source");
    return ptx_conv_stem_bf16_supported(d, src);
}

extern "C" int ptx_conv_stem_bf16_strided_fwd(const ptx_conv3d_desc* d, const void* x, int32_t src, const ptx_norm_desc* norm,
                                              int32_t frame_step, int32_t T_full, const void* w_stem, const float* bias, void* y,
                                              ptx_stream_t stream) {
    if (!d || !x || !w_stem || !y) return fail(PTX_ERR_INVALID, "conv_stem_bf16: null pointer");
    if (!ptx_conv_stem_bf16_strided_supported(d, src, frame_step, T_full)) return PTX_ERR_UNSUPPORTED;     // (the reason is in the last-error string)
    if (src == PTX_STEM_SRC_U8_NTHWC && !norm) return fail(PTX_ERR_INVALID, "conv_stem_bf16: uint8 frames need a ptx_norm_desc");
    if (src == PTX_STEM_SRC_BF16_NCDHW && ((uintptr_t)x & 1)) return fail(PTX_ERR_INVALID, "conv_stem_bf16: misaligned bf16 clip");
    if (((uintptr_t)w_stem | (uintptr_t)y) & 15) return fail(PTX_ERR_INVALID, "conv_stem_bf16: filter and output must be 16-byte aligned");
    StemBf16Geom g;
    stem_bf16_geom(d, &g);
    StemBf16Args a{};
    a.x = x; a.w = static_cast<const unsigned short*>(w_stem); a.bias = bias; a.y = static_cast<unsigned short*>(y);
    if (norm) a.norm = *norm;
    a.frame_step = frame_step; a.T_full = T_full;
    a.N = d->N; a.Ti = d->Ti; a.Hi = d->Hi; a.Wi = d->Wi; a.To = d->To; a.Ho = d->Ho; a.Wo = d->Wo; a.ldy = d->ldy; a.Co = d->Co;
    a.kT = d->kT; a.kH = d->kH; a.sT = d->sT; a.sH = d->sH; a.sW = d->sW; a.pT = d->pT; a.pH = d->pH; a.pW = d->pW;
    a.row_mode = g.row_mode; a.segs = g.segs; a.PR = g.PR; a.PC = g.PC; a.khc = g.khc;
    a.tiles_per_frame = g.tiles_per_frame;
    a.n_tiles = d->N * d->To * g.tiles_per_frame;
    a.w_tiles = d->Co_pad / kSbBN;
    a.flags = d->flags;
    fdiv_make((unsigned)d->Wo, a.dv_wo);
    fdiv_make((unsigned)(g.PC / 2), a.dv_pc2);
    const size_t lds = (size_t)g.PR * g.PC * 8 + 2 * kSbWSlot * 2 + 3 * 256 * 2;
    const dim3 grid((unsigned)a.n_tiles, (unsigned)cdiv(d->ldy, kSbBN));
    // frame_step == 1 (then T_full == Ti) runs the plain instances: the code the plain entry point always ran
    const bool strided = frame_step != 1;
    if (src == PTX_STEM_SRC_U8_NTHWC && strided)
        hipLaunchKernelGGL(HIP_KERNEL_NAME(conv_stem_bf16_kernel<PTX_STEM_SRC_U8_NTHWC, true>), grid, dim3(kSbNT), lds, (hipStream_t)stream, a);
    else if (src == PTX_STEM_SRC_U8_NTHWC)
        hipLaunchKernelGGL(HIP_KERNEL_NAME(conv_stem_bf16_kernel<PTX_STEM_SRC_U8_NTHWC, false>), grid, dim3(kSbNT), lds, (hipStream_t)stream, a);
    else if (strided)
        hipLaunchKernelGGL(HIP_KERNEL_NAME(conv_stem_bf16_kernel<PTX_STEM_SRC_BF16_NCDHW, true>), grid, dim3(kSbNT), lds, (hipStream_t)stream, a);
    else
        hipLaunchKernelGGL(HIP_KERNEL_NAME(conv_stem_bf16_kernel<PTX_STEM_SRC_BF16_NCDHW, false>), grid, dim3(kSbNT), lds, (hipStream_t)stream, a);
    return hip_check(hipGetLastError(), "conv_stem_bf16 launch");
}

extern "C" int ptx_conv_stem_bf16_fwd(const ptx_conv3d_desc* d, const void* x, int32_t src, const ptx_norm_desc* norm,
                                      const void* w_stem, const float* bias, void* y, ptx_stream_t stream) {
    if (!d || !x || !w_stem || !y) return fail(PTX_ERR_INVALID, "conv_stem_bf16: null pointer");
    if (!ptx_conv_stem_bf16_supported(d, src)) return PTX_ERR_UNSUPPORTED;         // (the reason is in the last-error string)
    return ptx_conv_stem_bf16_strided_fwd(d, x, src, norm, 1, d->Ti, w_stem, bias, y, stream);
}
