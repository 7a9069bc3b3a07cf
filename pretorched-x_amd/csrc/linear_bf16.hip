// Linear layers with bf16 weights for few input rows (include/ptx_amd_linear_bf16.h): the TRN relation MLPs and the classifier
// of a bfloat16 model.  The weights are the only large stream (an MSTRN head on resnet50 at 8 segments reads 73 M of them), so
// the work is arranged around reading them ONCE at HBM rate; the fp32 skinny_linear_kernel (pool_head.hip) re-reads its input
// rows from L2 in every workgroup, once per two weight rows.
//
// Matrix-core path (bf16 x, 16-byte aligned rows) -- lbw_mfma_kernel.
//   grid (row groups of 32 rows, column groups of 128 features, K splits); 256 threads = 4 waves; wave w owns the two 16-column
//   tiles [32 w, 32 w + 32) of the column group and both 16-row tiles of the row group.
//   Per K slab of 256: (1) every lane issues its 16 weight loads of 16 bytes (2 column tiles x 8 k-steps; lane (r, g) = (lane %
//   16, lane / 16) reads w[n0 + r][kb + 32 j + 8 g .. + 8), so 16 lanes x 4 groups x 8 steps cover 16 rows x 512 contiguous bytes)
//   -- straight from global memory into the B operand registers, no LDS hop; (2) the workgroup stages its <= 32 input rows of the
//   slab in LDS once (ReLU and the frame gather applied on the way; rows >= M and k >= K are zero); (3) 8 k-steps of
//   v_mfma_f32_16x16x32_bf16 per (row tile, column tile): A = 8 consecutive k of input row r from LDS (one ds_read_b128; the
//   row pitch of 264 bf16 = 132 dwords walks 4 banks per row, so the 16 rows of a read hit 64 distinct banks), B = the weights.
//   M <= 16 issues one row tile, 16 < M <= 32 two on the same B registers: the weight stream is shared by both.
//   With one split the epilogue (bias, ACCUM, ReLU) runs in the kernel; otherwise every workgroup writes its fp32 partial tile
//   to workspace[split][M][Nout] and lbw_reduce_kernel sums the splits in a fixed order and applies the epilogue: no atomics.
//   Split rule (lbw_splits): as many splits as give about two workgroups per CU, at most one per slab -- a function of (M, K,
//   Nout) only.  Nout = 1024, K = 16384: 8 column groups x 64 splits = 512 workgroups of 64 KiB of weights each.
//
// Vector-unit path (fp32 x, set-sum, unaligned / odd-K bf16 x) -- lbw_valu_kernel.
//   One wave per output feature and 8 rows; lane l owns the k chunks [8 c, 8 c + 8) for c = l, l + 64, ..: acc = fmaf(x, widen(w),
//   acc) in ascending k, then a xor-butterfly over the lanes.  Aligned rows use 16-byte loads, anything else scalar loads, in the
//   same order -- the bits do not depend on the alignment.  These launches are small (the W2 launch reads 2 MiB).
// Compiled as part of pool_head.hip's translation unit (its last line includes this file), like pack_layout.hip's guests.
#include "../../include/ptx_amd_linear_bf16.h"

namespace ptx {

typedef __bf16 lb_bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned int lb_u32x4 __attribute__((ext_vector_type(4)));

constexpr int kLbSlab = 256;                 // k per staged slab
constexpr int kLbLd = kLbSlab + 8;           // LDS row pitch (bf16 elements)
constexpr int kLbCols = 128;                 // features per workgroup (4 waves x 2 tiles of 16)
constexpr int kLbRows = 32;                  // rows per workgroup (2 tiles of 16)
constexpr int kLbTargetWGs = 2 * kNumCU;

struct LbwArgs {
    const unsigned short* x;
    const unsigned short* w;
    const unsigned short* b;
    float* y;
    float* ws;
    int M, K, Nout, ldx, ldy;
    unsigned flags;
    int splits, slabs_per, slabs;
    int gather, B, frame_len;
    int idx[PTX_REL_MAX_SETS][PTX_REL_MAX_FRAMES];
};

__device__ __forceinline__ float lb_widen(unsigned short v) { return __builtin_bit_cast(float, (unsigned)v << 16); }

// ReLU on two packed bf16 (fmaxf(v, 0) of each half: NaN -> 0, like the fp32 kernels' prologue)
__device__ __forceinline__ unsigned lb_relu2(unsigned v) {
    const float lo = fmaxf(__builtin_bit_cast(float, v << 16), 0.f);
    const float hi = fmaxf(__builtin_bit_cast(float, v & 0xffff0000u), 0.f);
    return (__builtin_bit_cast(unsigned, lo) >> 16) | (__builtin_bit_cast(unsigned, hi) & 0xffff0000u);
}

__global__ void __launch_bounds__(256) lbw_mfma_kernel(const LbwArgs p) {
    __shared__ __attribute__((aligned(16))) unsigned short xs[kLbRows * kLbLd];
    __shared__ int sidx[PTX_REL_MAX_SETS * PTX_REL_MAX_FRAMES];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 15, g = lane >> 4;
    const int m_base = blockIdx.x * kLbRows;
    const int n_rt = min(kLbRows, p.M - m_base) > 16 ? 2 : 1;          // uniform
    const int col0 = blockIdx.y * kLbCols + wave * 32;
    const int split = blockIdx.z;
    const int slab_lo = split * p.slabs_per, slab_hi = min(p.slabs, slab_lo + p.slabs_per);
    const bool relu_in = (p.flags & PTX_PRO_RELU) != 0;
    if (p.gather) {
        for (int i = tid; i < PTX_REL_MAX_SETS * PTX_REL_MAX_FRAMES; i += 256)
            sidx[i] = p.idx[i / PTX_REL_MAX_FRAMES][i % PTX_REL_MAX_FRAMES];
    }
    bool tile_ok[2];
    const unsigned short* wrow[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        tile_ok[t] = col0 + t * 16 < p.Nout;                            // uniform per wave
        wrow[t] = p.w + (size_t)min(col0 + t * 16 + r, p.Nout - 1) * p.K;
    }
    f32x4 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int t = 0; t < 2; ++t) acc[a][t] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (int slab = slab_lo; slab < slab_hi; ++slab) {
        const int kb = slab * kLbSlab;
        // (1) the weights of this slab: 16 loads of 16 bytes in flight per lane
        lb_u32x4 bw[2][8];
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int k = kb + j * 32 + g * 8;
                bw[t][j] = lb_u32x4{0u, 0u, 0u, 0u};
                if (tile_ok[t] && k < p.K) bw[t][j] = *reinterpret_cast<const lb_u32x4*>(wrow[t] + k);
            }
        // (2) the input rows of this slab, once per workgroup
        __syncthreads();                                                // the previous slab's readers are done (and sidx is written)
        for (int i = tid; i < n_rt * 16 * (kLbSlab / 8); i += 256) {
            const int row = i >> 5, c = i & 31;
            const int m = m_base + row, k = kb + c * 8;
            lb_u32x4 v = lb_u32x4{0u, 0u, 0u, 0u};
            if (m < p.M && k < p.K) {
                const unsigned short* src;
                if (p.gather) {
                    const int rset = m / p.B, vid = m - rset * p.B;
                    const int f = k / p.frame_len, off = k - f * p.frame_len;
                    src = p.x + (size_t)vid * p.ldx + (size_t)sidx[rset * PTX_REL_MAX_FRAMES + f] * p.frame_len + off;
                } else {
                    src = p.x + (size_t)m * p.ldx + k;
                }
                v = *reinterpret_cast<const lb_u32x4*>(src);
                if (relu_in) {
                    v.x = lb_relu2(v.x); v.y = lb_relu2(v.y); v.z = lb_relu2(v.z); v.w = lb_relu2(v.w);
                }
            }
            *reinterpret_cast<lb_u32x4*>(xs + row * kLbLd + c * 8) = v;
        }
        __syncthreads();
        // (3) 8 k-steps: A from LDS, B from the registers
#pragma unroll
        for (int j = 0; j < 8; ++j) {
#pragma unroll
            for (int a = 0; a < 2; ++a) {
                if (a < n_rt) {
                    const lb_bf16x8 av = *reinterpret_cast<const lb_bf16x8*>(xs + (a * 16 + r) * kLbLd + j * 32 + g * 8);
#pragma unroll
                    for (int t = 0; t < 2; ++t)
                        if (tile_ok[t])
                            acc[a][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av, __builtin_bit_cast(lb_bf16x8, bw[t][j]), acc[a][t], 0, 0, 0);
                }
            }
        }
    }
    // epilogue: lane (r, g) holds rows 4 g + v, column r of every tile
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const int m = m_base + a * 16 + 4 * g + v, n = col0 + t * 16 + r;
                if (a >= n_rt || m >= p.M || n >= p.Nout) continue;
                float o = acc[a][t][v];
                if (p.splits > 1) {
                    p.ws[((size_t)split * p.M + m) * p.Nout + n] = o;
                    continue;
                }
                if (p.b) o += lb_widen(p.b[n]);
                float* dst = p.y + (size_t)m * p.ldy + n;
                if (p.flags & PTX_EPI_ACCUM) o += *dst;
                if (p.flags & PTX_EPI_RELU) o = fmaxf(o, 0.f);
                *dst = o;
            }
}

// y[m][n] = epilogue(sum over the splits of workspace[split][m][n]) in a fixed order: a workgroup owns 64 consecutive outputs,
// wave q sums the q-th quarter of the splits in ascending order (8 independent loads in flight per lane), the four partial sums
// are added in wave order through LDS.  (One thread per output walking all the splits serially measured 17 us at 64 splits --
// more than the kernel that reads the weights.)
__global__ void __launch_bounds__(256) lbw_reduce_kernel(const float* __restrict__ ws, const unsigned short* __restrict__ b,
                                                         float* __restrict__ y, int M, int Nout, int ldy, int splits, unsigned flags) {
    __shared__ float part[4][64];
    const int l = threadIdx.x & 63, q = threadIdx.x >> 6;
    const size_t total = (size_t)M * Nout;
    const size_t i = (size_t)blockIdx.x * 64 + l;
    const int per = (splits + 3) / 4;
    const int s0 = q * per, s1 = min(splits, s0 + per);
    float o = 0.f;
    if (i < total) {
        for (int s = s0; s < s1; s += 8) {
            float v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = s + u < s1 ? ws[(size_t)(s + u) * total + i] : 0.f;
#pragma unroll
            for (int u = 0; u < 8; ++u) o += v[u];
        }
    }
    part[q][l] = o;
    __syncthreads();
    if (q != 0 || i >= total) return;
    o = ((part[0][l] + part[1][l]) + part[2][l]) + part[3][l];
    const int m = (int)(i / Nout), n = (int)(i - (size_t)m * Nout);
    if (b) o += lb_widen(b[n]);
    float* dst = y + (size_t)m * ldy + n;
    if (flags & PTX_EPI_ACCUM) o += *dst;
    if (flags & PTX_EPI_RELU) o = fmaxf(o, 0.f);
    *dst = o;
}

struct LbwValuArgs {
    const void* x;
    const unsigned short* w;
    const unsigned short* b;
    float* y;
    int M, K, Nout, ldx, ldy;
    unsigned flags;
    int n_sets;              // set-sum: x_eff[m] = sum_r x[r * set_stride + m * ldx] (fp32 x only); else 1
    long long set_stride;
    float bias_scale;
    int vec;                 // rows of x and w are 16-byte aligned and K % 8 == 0: 16-byte loads
};

template <bool XBF16>
__global__ void __launch_bounds__(256) lbw_valu_kernel(const LbwValuArgs p) {
    constexpr int MR = 8;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int j = blockIdx.x * 4 + wave, m0 = blockIdx.y * MR;
    if (j >= p.Nout) return;                                            // no barrier below
    const bool relu_in = (p.flags & PTX_PRO_RELU) != 0;
    const unsigned short* wr = p.w + (size_t)j * p.K;
    float acc[MR];
#pragma unroll
    for (int m = 0; m < MR; ++m) acc[m] = 0.f;
    const int chunks = (p.K + 7) / 8;
    for (int c = lane; c < chunks; c += 64) {
        const int k0 = c * 8, n = min(8, p.K - k0);
        float wv[8];
        if (p.vec) {
            const lb_u32x4 q = *reinterpret_cast<const lb_u32x4*>(wr + k0);
            wv[0] = __builtin_bit_cast(float, q.x << 16); wv[1] = __builtin_bit_cast(float, q.x & 0xffff0000u);
            wv[2] = __builtin_bit_cast(float, q.y << 16); wv[3] = __builtin_bit_cast(float, q.y & 0xffff0000u);
            wv[4] = __builtin_bit_cast(float, q.z << 16); wv[5] = __builtin_bit_cast(float, q.z & 0xffff0000u);
            wv[6] = __builtin_bit_cast(float, q.w << 16); wv[7] = __builtin_bit_cast(float, q.w & 0xffff0000u);
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) wv[e] = e < n ? lb_widen(wr[k0 + e]) : 0.f;
        }
#pragma unroll
        for (int m = 0; m < MR; ++m) {
            if (m0 + m >= p.M) break;                                   // uniform
            float xv[8];
            if (XBF16) {
                const unsigned short* xr = static_cast<const unsigned short*>(p.x) + (size_t)(m0 + m) * p.ldx + k0;
                if (p.vec) {
                    const lb_u32x4 q = *reinterpret_cast<const lb_u32x4*>(xr);
                    xv[0] = __builtin_bit_cast(float, q.x << 16); xv[1] = __builtin_bit_cast(float, q.x & 0xffff0000u);
                    xv[2] = __builtin_bit_cast(float, q.y << 16); xv[3] = __builtin_bit_cast(float, q.y & 0xffff0000u);
                    xv[4] = __builtin_bit_cast(float, q.z << 16); xv[5] = __builtin_bit_cast(float, q.z & 0xffff0000u);
                    xv[6] = __builtin_bit_cast(float, q.w << 16); xv[7] = __builtin_bit_cast(float, q.w & 0xffff0000u);
                } else {
#pragma unroll
                    for (int e = 0; e < 8; ++e) xv[e] = e < n ? lb_widen(xr[e]) : 0.f;
                }
            } else {
                const float* xr = static_cast<const float*>(p.x) + (size_t)(m0 + m) * p.ldx + k0;
#pragma unroll
                for (int e = 0; e < 8; ++e) xv[e] = 0.f;
                for (int s = 0; s < p.n_sets; ++s) {                    // the set sum: fp32, r ascending
                    const float* xs_ = xr + (size_t)s * p.set_stride;
                    if (p.vec) {
                        const f32x4 q0 = *reinterpret_cast<const f32x4*>(xs_), q1 = *reinterpret_cast<const f32x4*>(xs_ + 4);
                        const float t[8] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w};
#pragma unroll
                        for (int e = 0; e < 8; ++e) xv[e] = s == 0 ? t[e] : xv[e] + t[e];
                    } else {
#pragma unroll
                        for (int e = 0; e < 8; ++e)
                            if (e < n) xv[e] = s == 0 ? xs_[e] : xv[e] + xs_[e];
                    }
                }
            }
            if (relu_in) {
#pragma unroll
                for (int e = 0; e < 8; ++e) xv[e] = fmaxf(xv[e], 0.f);
            }
            float a = acc[m];
#pragma unroll
            for (int e = 0; e < 8; ++e) a = fmaf(xv[e], wv[e], a);
            acc[m] = a;
        }
    }
#pragma unroll
    for (int m = 0; m < MR; ++m)
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) acc[m] += __shfl_xor(acc[m], off, 64);
    if (lane == 0) {
#pragma unroll
        for (int m = 0; m < MR; ++m) {
            if (m0 + m >= p.M) break;
            float o = acc[m] + (p.b ? p.bias_scale * lb_widen(p.b[j]) : 0.f);
            float* dst = p.y + (size_t)(m0 + m) * p.ldy + j;
            if (p.flags & PTX_EPI_ACCUM) o += *dst;
            if (p.flags & PTX_EPI_RELU) o = fmaxf(o, 0.f);
            *dst = o;
        }
    }
}

// ---- host side --------------------------------------------------------------------------------------------------------------
// K splits of the matrix-core path: a function of (M, K, Nout) only.  slabs_per: slabs of one split.
static int lbw_splits(int M, int K, int Nout, int* slabs_per) {
    const int slabs = cdiv(K, kLbSlab);
    const long long tiles = (long long)cdiv(M, kLbRows) * cdiv(Nout, kLbCols);
    long long want = tiles >= kLbTargetWGs ? 1 : kLbTargetWGs / tiles;
    if (want > slabs) want = slabs;
    const int per = cdiv(slabs, (int)want);
    if (slabs_per) *slabs_per = per;
    return cdiv(slabs, per);
}

static const unsigned kLbwFlags = PTX_PRO_RELU | PTX_EPI_RELU | PTX_EPI_ACCUM;

static bool lbw_dense_ok(const void* x, int x_kind, const void* w, const void* b, const float* y, int M, int K, int Nout, int ldx,
                         int ldy, unsigned flags) {
    if (!x || !w || !y) return fail(PTX_ERR_INVALID, "linear_bf16w: null pointer (x, w and y are required)"), false;
    if (x_kind != PTX_LIN_X_BF16 && x_kind != PTX_LIN_X_F32)
        return fail(PTX_ERR_INVALID, "linear_bf16w: x_kind=%d must be PTX_LIN_X_BF16 (0) or PTX_LIN_X_F32 (1)", x_kind), false;
    if (M <= 0 || K <= 0 || Nout <= 0) return fail(PTX_ERR_INVALID, "linear_bf16w: non-positive extent (M=%d K=%d Nout=%d)", M, K, Nout), false;
    if (ldx < K) return fail(PTX_ERR_INVALID, "linear_bf16w: ldx=%d is shorter than a row of K=%d", ldx, K), false;
    if (ldy < Nout) return fail(PTX_ERR_INVALID, "linear_bf16w: ldy=%d is shorter than a row of Nout=%d", ldy, Nout), false;
    if (flags & ~kLbwFlags) return fail(PTX_ERR_INVALID, "linear_bf16w: flags 0x%x: only PTX_PRO_RELU, PTX_EPI_RELU and PTX_EPI_ACCUM apply", flags), false;
    if (((uintptr_t)w & 1) || (b && ((uintptr_t)b & 1)) || ((uintptr_t)y & 3) || ((uintptr_t)x & (x_kind == PTX_LIN_X_F32 ? 3 : 1)))
        return fail(PTX_ERR_INVALID, "linear_bf16w: a pointer is not aligned to its element size"), false;
    if (cdiv(M, 8) > 65535) return fail(PTX_ERR_UNSUPPORTED, "linear_bf16w: M=%d rows are too many for a few-row kernel", M), false;
    return true;
}

static bool lbw_rel_ok(const ptx_relation_desc* d, const void* x, int ldx, const void* w, const void* b, const float* y, int Nout,
                       int ldy, unsigned flags) {
    if (!d || !x || !w || !y) return fail(PTX_ERR_INVALID, "relation_linear_bf16w: null pointer (desc, x, w and y are required)"), false;
    if (d->B <= 0 || d->n_sets <= 0 || d->n_sets > PTX_REL_MAX_SETS || d->n_frames <= 0 || d->n_frames > PTX_REL_MAX_FRAMES)
        return fail(PTX_ERR_INVALID, "relation_linear_bf16w: need B >= 1 and 1..%d subsets of 1..%d frames", PTX_REL_MAX_SETS, PTX_REL_MAX_FRAMES), false;
    if (d->frame_len <= 0 || d->frame_len % 8)
        return fail(PTX_ERR_INVALID, "relation_linear_bf16w: frame_len=%d must be a positive multiple of 8 (16-byte bf16 frames)", d->frame_len), false;
    if (ldx % 8) return fail(PTX_ERR_INVALID, "relation_linear_bf16w: ldx=%d must be a multiple of 8", ldx), false;
    if (Nout <= 0 || ldy < Nout) return fail(PTX_ERR_INVALID, "relation_linear_bf16w: ldy=%d is shorter than a row of Nout=%d", ldy, Nout), false;
    if (flags & ~kLbwFlags) return fail(PTX_ERR_INVALID, "relation_linear_bf16w: flags 0x%x: only PTX_PRO_RELU, PTX_EPI_RELU and PTX_EPI_ACCUM apply", flags), false;
    int max_idx = 0;
    for (int r = 0; r < d->n_sets; ++r)
        for (int f = 0; f < d->n_frames; ++f) {
            if (d->idx[r][f] < 0) return fail(PTX_ERR_INVALID, "relation_linear_bf16w: negative frame index"), false;
            max_idx = std::max(max_idx, (int)d->idx[r][f]);
        }
    if ((int64_t)(max_idx + 1) * d->frame_len > ldx)
        return fail(PTX_ERR_INVALID, "relation_linear_bf16w: frame index %d outside a video of ldx=%d elements", max_idx, ldx), false;
    if ((((uintptr_t)x | (uintptr_t)w) & 15) || (b && ((uintptr_t)b & 1)) || ((uintptr_t)y & 3))
        return fail(PTX_ERR_INVALID, "relation_linear_bf16w: misaligned pointer (x and w need 16 bytes)"), false;
    if ((int64_t)d->n_sets * d->B > 65535 * 8 || (int64_t)d->n_frames * d->frame_len > 0x7fffffffLL)
        return fail(PTX_ERR_UNSUPPORTED, "relation_linear_bf16w: problem too large"), false;
    return true;
}

static int lbw_launch_mfma(LbwArgs& a, void* workspace, size_t workspace_bytes, hipStream_t st, const char* who) {
    a.slabs = cdiv(a.K, kLbSlab);
    a.splits = lbw_splits(a.M, a.K, a.Nout, &a.slabs_per);
    const size_t need = a.splits > 1 ? (size_t)a.splits * a.M * a.Nout * sizeof(float) : 0;
    if (need) {
        if (!workspace || workspace_bytes < need)
            return fail(PTX_ERR_WORKSPACE, "%s: %zu bytes of workspace, ptx_linear_bf16w_workspace_bytes asks for %zu", who, workspace ? workspace_bytes : (size_t)0, need);
        if ((uintptr_t)workspace & 15) return fail(PTX_ERR_INVALID, "%s: the workspace needs 16-byte alignment", who);
    }
    a.ws = static_cast<float*>(workspace);
    const int rg = cdiv(a.M, kLbRows), cg = cdiv(a.Nout, kLbCols);
    if (cg > 65535) return fail(PTX_ERR_UNSUPPORTED, "%s: Nout=%d is too wide", who, a.Nout);
    hipLaunchKernelGGL(lbw_mfma_kernel, dim3((unsigned)rg, (unsigned)cg, (unsigned)a.splits), dim3(256), 0, st, a);
    int rc = hip_check(hipGetLastError(), who);
    if (rc != PTX_OK || a.splits == 1) return rc;
    const size_t total = (size_t)a.M * a.Nout;
    hipLaunchKernelGGL(lbw_reduce_kernel, dim3((unsigned)((total + 63) / 64)), dim3(256), 0, st, a.ws, a.b, a.y, a.M, a.Nout, a.ldy,
                       a.splits, a.flags);
    return hip_check(hipGetLastError(), who);
}

static int lbw_launch_valu(LbwValuArgs& a, bool xbf16, hipStream_t st, const char* who) {
    const dim3 grid((unsigned)cdiv(a.Nout, 4), (unsigned)cdiv(a.M, 8));
    if (xbf16) hipLaunchKernelGGL(lbw_valu_kernel<true>, grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL(lbw_valu_kernel<false>, grid, dim3(256), 0, st, a);
    return hip_check(hipGetLastError(), who);
}

}  // namespace ptx

using namespace ptx;

extern "C" size_t ptx_linear_bf16w_workspace_bytes(int32_t M, int32_t K, int32_t Nout) {
    if (M <= 0 || K <= 0 || Nout <= 0) return 0;
    const int s = lbw_splits(M, K, Nout, nullptr);
    return s > 1 ? (size_t)s * M * Nout * sizeof(float) : 0;
}

extern "C" int ptx_linear_bf16w_supported(const void* x, int32_t x_kind, const void* w, const void* b, const float* y, int32_t M,
                                          int32_t K, int32_t Nout, int32_t ldx, int32_t ldy, uint32_t flags) {
    return lbw_dense_ok(x, x_kind, w, b, y, M, K, Nout, ldx, ldy, flags) ? 1 : 0;
}

extern "C" int ptx_linear_bf16w_fwd(const void* x, int32_t x_kind, const void* w, const void* b, float* y, int32_t M, int32_t K,
                                    int32_t Nout, int32_t ldx, int32_t ldy, uint32_t flags, void* workspace,
                                    size_t workspace_bytes, ptx_stream_t stream) {
    if (!lbw_dense_ok(x, x_kind, w, b, y, M, K, Nout, ldx, ldy, flags)) return PTX_ERR_INVALID;
    const bool xbf16 = x_kind == PTX_LIN_X_BF16;
    const bool rows16 = K % 8 == 0 && !((uintptr_t)w & 15) && !((uintptr_t)x & 15) && ldx % (xbf16 ? 8 : 4) == 0;
    if (xbf16 && rows16) {
        LbwArgs a{};
        a.x = static_cast<const unsigned short*>(x); a.w = static_cast<const unsigned short*>(w);
        a.b = static_cast<const unsigned short*>(b); a.y = y;
        a.M = M; a.K = K; a.Nout = Nout; a.ldx = ldx; a.ldy = ldy; a.flags = flags;
        a.gather = 0; a.B = M; a.frame_len = K;
        return lbw_launch_mfma(a, workspace, workspace_bytes, (hipStream_t)stream, "linear_bf16w");
    }
    LbwValuArgs a{};
    a.x = x; a.w = static_cast<const unsigned short*>(w); a.b = static_cast<const unsigned short*>(b); a.y = y;
    a.M = M; a.K = K; a.Nout = Nout; a.ldx = ldx; a.ldy = ldy; a.flags = flags;
    a.n_sets = 1; a.set_stride = 0; a.bias_scale = 1.f; a.vec = rows16 ? 1 : 0;
    return lbw_launch_valu(a, xbf16, (hipStream_t)stream, "linear_bf16w");
}

extern "C" int ptx_relation_linear_bf16w_supported(const ptx_relation_desc* desc, const void* x, int32_t ldx, const void* w,
                                                   const void* b, const float* y, int32_t Nout, int32_t ldy, uint32_t flags) {
    return lbw_rel_ok(desc, x, ldx, w, b, y, Nout, ldy, flags) ? 1 : 0;
}

extern "C" int ptx_relation_linear_bf16w_fwd(const ptx_relation_desc* d, const void* x, int32_t ldx, const void* w, const void* b,
                                             float* y, int32_t Nout, int32_t ldy, uint32_t flags, void* workspace,
                                             size_t workspace_bytes, ptx_stream_t stream) {
    if (!lbw_rel_ok(d, x, ldx, w, b, y, Nout, ldy, flags)) return PTX_ERR_INVALID;
    LbwArgs a{};
    a.x = static_cast<const unsigned short*>(x); a.w = static_cast<const unsigned short*>(w);
    a.b = static_cast<const unsigned short*>(b); a.y = y;
    a.M = d->n_sets * d->B; a.K = d->n_frames * d->frame_len; a.Nout = Nout; a.ldx = ldx; a.ldy = ldy; a.flags = flags;
    a.gather = 1; a.B = d->B; a.frame_len = d->frame_len;
    for (int r = 0; r < PTX_REL_MAX_SETS; ++r)
        for (int f = 0; f < PTX_REL_MAX_FRAMES; ++f) a.idx[r][f] = (r < d->n_sets && f < d->n_frames) ? d->idx[r][f] : 0;
    return lbw_launch_mfma(a, workspace, workspace_bytes, (hipStream_t)stream, "relation_linear_bf16w");
}

static bool lbw_setsum_ok(const float* x, const void* w, const void* b, const float* y, int B, int n_sets, int K, int Nout, int ldx,
                          int ldy, unsigned flags) {
    if (!x || !w || !y) return fail(PTX_ERR_INVALID, "linear_setsum_bf16w: null pointer (x, w and y are required)"), false;
    if (B <= 0 || n_sets <= 0 || K <= 0 || Nout <= 0)
        return fail(PTX_ERR_INVALID, "linear_setsum_bf16w: non-positive extent (B=%d n_sets=%d K=%d Nout=%d)", B, n_sets, K, Nout), false;
    if (ldx < K) return fail(PTX_ERR_INVALID, "linear_setsum_bf16w: ldx=%d is shorter than a row of K=%d", ldx, K), false;
    if (ldy < Nout) return fail(PTX_ERR_INVALID, "linear_setsum_bf16w: ldy=%d is shorter than a row of Nout=%d", ldy, Nout), false;
    if (flags & ~kLbwFlags) return fail(PTX_ERR_INVALID, "linear_setsum_bf16w: flags 0x%x: only PTX_PRO_RELU, PTX_EPI_RELU and PTX_EPI_ACCUM apply", flags), false;
    if (((uintptr_t)w & 1) || (b && ((uintptr_t)b & 1)) || (((uintptr_t)x | (uintptr_t)y) & 3))
        return fail(PTX_ERR_INVALID, "linear_setsum_bf16w: a pointer is not aligned to its element size"), false;
    if (cdiv(B, 8) > 65535) return fail(PTX_ERR_UNSUPPORTED, "linear_setsum_bf16w: B=%d rows are too many for a few-row kernel", B), false;
    return true;
}

extern "C" int ptx_linear_setsum_bf16w_supported(const float* x, const void* w, const void* b, const float* y, int32_t B,
                                                 int32_t n_sets, int32_t K, int32_t Nout, int32_t ldx, int32_t ldy, uint32_t flags) {
    return lbw_setsum_ok(x, w, b, y, B, n_sets, K, Nout, ldx, ldy, flags) ? 1 : 0;
}

extern "C" int ptx_linear_setsum_bf16w_fwd(const float* x, const void* w, const void* b, float* y, int32_t B, int32_t n_sets,
                                           int32_t K, int32_t Nout, int32_t ldx, int32_t ldy, uint32_t flags, ptx_stream_t stream) {
    if (!lbw_setsum_ok(x, w, b, y, B, n_sets, K, Nout, ldx, ldy, flags)) return PTX_ERR_INVALID;
    LbwValuArgs a{};
    a.x = x; a.w = static_cast<const unsigned short*>(w); a.b = static_cast<const unsigned short*>(b); a.y = y;
    a.M = B; a.K = K; a.Nout = Nout; a.ldx = ldx; a.ldy = ldy; a.flags = flags;
    a.n_sets = n_sets; a.set_stride = (long long)B * ldx; a.bias_scale = (float)n_sets;
    a.vec = (K % 8 == 0 && ldx % 4 == 0 && !((uintptr_t)w & 15) && !((uintptr_t)x & 15)) ? 1 : 0;
    return lbw_launch_valu(a, false, (hipStream_t)stream, "linear_setsum_bf16w");
}
