/* pretorched-x_amd: 10- and 12-bit YUV 4:2:0 sources (P010 / P012 / P016 surfaces, yuv420p10le / yuv420p12le planes) for
 * the PIL-exact resize kernels (csrc/resize_common.h), exported by the same libptx_amd.so.  The entry points live in a
 * header of their own, like ptx_amd_wino4.h and ptx_amd_tfir.h: ptx_amd.h is the census of the drop-in contract as it
 * stood before them, this file adds to it. */
#ifndef PTX_AMD_YUV16_H
#define PTX_AMD_YUV16_H

#include "ptx_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* A ptx_yuv420_src whose samples are 16-bit little-endian words holding `bits` = 10 or 12 significant bits:
 *     s = (word >> shift) & (2^bits - 1)
 * shift = 16 - bits: MSB-aligned containers (P010 / P012 / P016: the low bits are ignored, whatever they hold);
 * shift = 0:         LSB-aligned containers (yuv420p10le / yuv420p12le: the high bits are masked).
 * The kernels convert to 8-bit RGB while they stage an input row on chip, with d = bits - 8:
 *     y' = Y - y_off   cb = Cb - (128 << d)   cr = Cr - (128 << d)
 *     R = clip8((ky y' + krv cr            + 2^(15+d)) >> (16+d))
 *     G = clip8((ky y' - kgu cb - kgv cr   + 2^(15+d)) >> (16+d))
 *     B = clip8((ky y' + kbu cb            + 2^(15+d)) >> (16+d))        (>> arithmetic)
 * the chroma sample of pixel (r, c) being (r >> 1, c >> 1); chroma planes have ceil(H/2) x ceil(W/2) samples.  Everything
 * behind the row stage is ptx_resize_frames_u8's code, so every output is bit-identical to that entry point on the
 * converted frames.  Transfer functions are not touched: PQ / HLG samples come out as PQ / HLG-coded RGB.
 * Strides and pitches are in BYTES, as in ptx_yuv420_src; step_c is 2 (planar chroma) or 4 (interleaved chroma, which
 * needs v == u + 1 or u == v + 1 in samples).  The host-side checks need no device: those of ptx_yuv420_src, plus
 * bits in {10, 12}, shift in {0, 16 - bits}, even pointers, pitches and strides (decoder surfaces and int16 tensors always
 * are), pitches of at least a row of 2-byte samples, and the 32-bit overflow of a plane in bytes. */
typedef struct ptx_yuv420p16_src {
    const uint16_t *y, *u, *v;         /* first sample of each plane of frame (0,0); interleaved UV: v == u + 1   */
    int64_t stride_n_y, stride_t_y;    /* bytes between videos / frames of the luma plane                         */
    int64_t stride_n_c, stride_t_c;    /* same for both chroma pointers                                           */
    int32_t pitch_y, pitch_c;          /* bytes between rows                                                      */
    int32_t step_c;                    /* bytes between chroma samples of a row: 2 planar, 4 interleaved          */
    int32_t y_off, ky, krv, kgu, kgv, kbu;
    int32_t bits, shift;               /* 10 or 12; 16 - bits (MSB-aligned) or 0 (LSB-aligned)                    */
} ptx_yuv420p16_src;
typedef struct ptx_clip_src_yuv420p16 {
    ptx_yuv420p16_src planes;          /* y/u/v at frame 0 of the clip's video; stride_n_* ignored                */
    int32_t H, W, Tv, reserved;
} ptx_clip_src_yuv420p16;

/* Arguments otherwise those of the _yuv420 twins in ptx_amd.h, results and error codes too. */
int ptx_resize_frames_yuv420p16_supported(const ptx_resize_desc* desc, const ptx_yuv420p16_src* src);
int ptx_resize_frames_yuv420p16(const ptx_resize_desc* desc, const ptx_yuv420p16_src* src,
                                const int32_t* row_lo, const int32_t* row_n, const int32_t* row_k,
                                const int32_t* col_lo, const int32_t* col_n, const int32_t* col_k,
                                void* y, const ptx_norm_desc* norm, ptx_stream_t stream);
int ptx_resize_frames_yuv420p16_windows_supported(const ptx_resize_desc* desc, const ptx_yuv420p16_src* src, int32_t h, int32_t w);
int ptx_resize_frames_yuv420p16_windows(const ptx_resize_desc* desc, const ptx_yuv420p16_src* src,
                                        const int32_t* row_lo, const int32_t* row_n, const int32_t* row_k,
                                        const int32_t* col_lo, const int32_t* col_n, const int32_t* col_k,
                                        int32_t h, int32_t w, const ptx_resize_window* windows,
                                        void* y, const ptx_norm_desc* norm, ptx_stream_t stream);
int ptx_resize_frames_yuv420p16_tables_supported(const ptx_resize_desc* desc, const ptx_yuv420p16_src* src);
int ptx_resize_frames_yuv420p16_tables(const ptx_resize_desc* desc, const ptx_yuv420p16_src* src,
                                       const int32_t* row_lo, const int32_t* row_n, const int32_t* row_k,
                                       const int32_t* col_lo, const int32_t* col_n, const int32_t* col_k,
                                       void* y, const ptx_norm_desc* norm, ptx_stream_t stream);
int ptx_resize_clips_yuv420p16_supported(const ptx_resize_desc* desc);
int ptx_resize_clips_yuv420p16(const ptx_resize_desc* desc, const ptx_clip_src_yuv420p16* srcs, const int32_t* frame_idx,
                               const int32_t* row_lo, const int32_t* row_n, const int32_t* row_k,
                               const int32_t* col_lo, const int32_t* col_n, const int32_t* col_k,
                               void* y, const ptx_norm_desc* norm, ptx_stream_t stream);
int ptx_resize_views_yuv420p16_supported(const ptx_views_desc* desc, const ptx_yuv420p16_src* src);
int ptx_resize_views_yuv420p16(const ptx_views_desc* desc, const ptx_yuv420p16_src* src, const int32_t* frame_idx,
                               const int32_t* row_lo, const int32_t* row_n, const int32_t* row_k,
                               const int32_t* col_lo, const int32_t* col_n, const int32_t* col_k,
                               void* y, const ptx_norm_desc* norm, ptx_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif  /* PTX_AMD_YUV16_H */
