// Training clips from videos of any size (ptx_resize_clips_u8 / _yuv420, ptx_resize_build_tables_clips): the CLIPS
// source mode of resize_frames_u8_kernel and the per-clip-extent form of the table builder.  Compiled as part of
// pack_layout.hip's translation unit (it instantiates that file's kernel template).
//
// A workgroup is (clip, frame of the clip, band of output rows), as in the per-clip-tables launch; what differs is where
// the frame comes from: srcs[clip] gives the clip's video (base, frame stride, H x W, Tv), frame_idx[clip * T + ti] the
// frame, and the kernel runs with that H, W.  The plan (band, LDS carves, row stages) is made from desc, whose H / W are
// the batch maxima, so one plan serves every clip of the launch.

namespace ptx {

__global__ void __launch_bounds__(256) resize_build_tables_clips_kernel(ptx_resize_desc d, const ptx_clip_src* __restrict__ srcs,
                                                                        const ptx_resize_geom* __restrict__ geoms, int filter,
                                                                        int* __restrict__ row_lo, int* __restrict__ row_n,
                                                                        int* __restrict__ row_k, int* __restrict__ col_lo,
                                                                        int* __restrict__ col_n, int* __restrict__ col_k) {
    const int per_clip = d.Ho + d.Wo;
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long long)d.N * per_clip) return;
    const int clip = (int)(idx / per_clip), e = (int)(idx - (long long)clip * per_clip);
    const int H = min(max(srcs[clip].H, 1), d.H), W = min(max(srcs[clip].W, 1), d.W);
    resize_build_entry(d, H, W, clip, e, geoms, filter, row_lo, row_n, row_k, col_lo, col_n, col_k);
}

}  // namespace ptx

// ysrcs: rows of ptx_clip_src_yuv420, or of ptx_clip_src_yuv420p16 when p16 is set
static int resize_clips_run(const ptx_resize_desc* desc, const ptx_clip_src* srcs, const void* ysrcs,
                            const int32_t* frame_idx, const int32_t* row_lo, const int32_t* row_n, const int32_t* row_k,
                            const int32_t* col_lo, const int32_t* col_n, const int32_t* col_k, void* y, const ptx_norm_desc* norm,
                            ptx_stream_t stream, const char* who, bool p16 = false) {
    ResizePlan p;
    int s = resize_plan(desc, y, &p, who);
    if (s) return s;
    if (ysrcs && desc->C != 3) return fail(PTX_ERR_INVALID, "%s: C=%d, a YUV source converts to 3 channels", who, desc->C);
    if ((!srcs && !ysrcs) || !frame_idx || !y || !row_lo || !row_n || !row_k || !col_lo || !col_n || !col_k)
        return fail(PTX_ERR_INVALID, "%s: null pointer", who);
    ptx_norm_desc nd = {};
    if ((s = resize_norm(desc, norm, &nd, who))) return s;
    const dim3 grid((unsigned)((int64_t)desc->N * desc->T * cdiv(desc->Ho, p.band)));
    const hipStream_t st = (hipStream_t)stream;
    const ResizeClips rc = {srcs, ysrcs, frame_idx};
    const unsigned char* none = nullptr;
#define PTX_CLIPS_LAUNCH(CH, SRC)                                                                                          \
    hipLaunchKernelGGL((resize_frames_u8_kernel<CH, SRC, false, false, true>), grid, dim3(256), p.lds_bytes, st, *desc, none, \
                       row_lo, row_n, row_k, col_lo, col_n, col_k, y, nd, p, YuvSource<SRC>::Desc{}, ResizeWindows{}, rc)
    if (ysrcs && p16) {
        PTX_CLIPS_LAUNCH(3, kSrcYuv16);
    } else if (ysrcs) {
        PTX_CLIPS_LAUNCH(3, kSrcYuv8);
    } else {
        switch (desc->C) {
            case 1: PTX_CLIPS_LAUNCH(1, kSrcRgb); break;
            case 2: PTX_CLIPS_LAUNCH(2, kSrcRgb); break;
            case 3: PTX_CLIPS_LAUNCH(3, kSrcRgb); break;
            default: PTX_CLIPS_LAUNCH(4, kSrcRgb); break;
        }
    }
#undef PTX_CLIPS_LAUNCH
    return hip_check(hipGetLastError(), who);
}

extern "C" int ptx_resize_clips_u8_supported(const ptx_resize_desc* desc) {
    ResizePlan p;
    return resize_plan(desc, nullptr, &p, "ptx_resize_clips_u8_supported") == PTX_OK;
}

extern "C" int ptx_resize_clips_u8(const ptx_resize_desc* desc, const ptx_clip_src* srcs, const int32_t* frame_idx,
                                   const int32_t* row_lo, const int32_t* row_n, const int32_t* row_k, const int32_t* col_lo,
                                   const int32_t* col_n, const int32_t* col_k, void* y, const ptx_norm_desc* norm,
                                   ptx_stream_t stream) {
    const char* who = "ptx_resize_clips_u8";
    if (!srcs) return fail(PTX_ERR_INVALID, "%s: null pointer", who);
    return resize_clips_run(desc, srcs, nullptr, frame_idx, row_lo, row_n, row_k, col_lo, col_n, col_k, y, norm, stream, who);
}

extern "C" int ptx_resize_clips_yuv420_supported(const ptx_resize_desc* desc) {
    const char* who = "ptx_resize_clips_yuv420_supported";
    ResizePlan p;
    if (resize_plan(desc, nullptr, &p, who) != PTX_OK) return 0;
    return desc->C == 3 || fail(PTX_ERR_INVALID, "%s: C=%d, a YUV source converts to 3 channels", who, desc->C) == PTX_OK;
}

extern "C" int ptx_resize_clips_yuv420(const ptx_resize_desc* desc, const ptx_clip_src_yuv420* srcs, const int32_t* frame_idx,
                                       const int32_t* row_lo, const int32_t* row_n, const int32_t* row_k, const int32_t* col_lo,
                                       const int32_t* col_n, const int32_t* col_k, void* y, const ptx_norm_desc* norm,
                                       ptx_stream_t stream) {
    const char* who = "ptx_resize_clips_yuv420";
    if (!srcs) return fail(PTX_ERR_INVALID, "%s: null pointer", who);
    return resize_clips_run(desc, nullptr, srcs, frame_idx, row_lo, row_n, row_k, col_lo, col_n, col_k, y, norm, stream, who);
}

extern "C" int ptx_resize_clips_yuv420p16_supported(const ptx_resize_desc* desc) {
    const char* who = "ptx_resize_clips_yuv420p16_supported";
    ResizePlan p;
    if (resize_plan(desc, nullptr, &p, who) != PTX_OK) return 0;
    return desc->C == 3 || fail(PTX_ERR_INVALID, "%s: C=%d, a YUV source converts to 3 channels", who, desc->C) == PTX_OK;
}

extern "C" int ptx_resize_clips_yuv420p16(const ptx_resize_desc* desc, const ptx_clip_src_yuv420p16* srcs, const int32_t* frame_idx,
                                          const int32_t* row_lo, const int32_t* row_n, const int32_t* row_k,
                                          const int32_t* col_lo, const int32_t* col_n, const int32_t* col_k, void* y,
                                          const ptx_norm_desc* norm, ptx_stream_t stream) {
    const char* who = "ptx_resize_clips_yuv420p16";
    if (!srcs) return fail(PTX_ERR_INVALID, "%s: null pointer", who);
    return resize_clips_run(desc, nullptr, srcs, frame_idx, row_lo, row_n, row_k, col_lo, col_n, col_k, y, norm, stream, who, true);
}

static int resize_build_tables_clips_run(const ptx_resize_desc* desc, const ptx_clip_src* srcs, const ptx_resize_geom* geoms,
                                         int filter, int32_t* row_lo, int32_t* row_n, int32_t* row_k, int32_t* col_lo,
                                         int32_t* col_n, int32_t* col_k, ptx_stream_t stream, const char* who) {
    ResizePlan p;
    int s = resize_plan(desc, nullptr, &p, who);                     // the extents and pitches the launch will be given
    if (s) return s;
    if ((s = resize_filter_check(filter, who))) return s;
    if (!srcs || !geoms || !row_lo || !row_n || !row_k || !col_lo || !col_n || !col_k)
        return fail(PTX_ERR_INVALID, "%s: null pointer", who);
    const int64_t entries = (int64_t)desc->N * ((int64_t)desc->Ho + desc->Wo);
    if (entries > INT32_MAX) return fail(PTX_ERR_UNSUPPORTED, "%s: N * (Ho + Wo) exceeds 32-bit indexing", who);
    hipLaunchKernelGGL(resize_build_tables_clips_kernel, dim3((unsigned)cdiv64(entries, 256)), dim3(256), 0, (hipStream_t)stream,
                       *desc, srcs, geoms, filter, row_lo, row_n, row_k, col_lo, col_n, col_k);
    return hip_check(hipGetLastError(), who);
}

extern "C" int ptx_resize_build_tables_clips(const ptx_resize_desc* desc, const ptx_clip_src* srcs, const ptx_resize_geom* geoms,
                                             int32_t* row_lo, int32_t* row_n, int32_t* row_k, int32_t* col_lo, int32_t* col_n,
                                             int32_t* col_k, ptx_stream_t stream) {
    return resize_build_tables_clips_run(desc, srcs, geoms, PTX_RESAMPLE_BILINEAR, row_lo, row_n, row_k, col_lo, col_n, col_k,
                                         stream, "ptx_resize_build_tables_clips");
}

// The same for a filter (include/ptx_amd_resample.h).
extern "C" int ptx_resize_build_tables_clips_filter(const ptx_resize_desc* desc, const ptx_clip_src* srcs,
                                                    const ptx_resize_geom* geoms, int32_t filter, int32_t* row_lo, int32_t* row_n,
                                                    int32_t* row_k, int32_t* col_lo, int32_t* col_n, int32_t* col_k,
                                                    ptx_stream_t stream) {
    return resize_build_tables_clips_run(desc, srcs, geoms, filter, row_lo, row_n, row_k, col_lo, col_n, col_k, stream,
                                         "ptx_resize_build_tables_clips_filter");
}
