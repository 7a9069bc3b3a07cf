"""ctypes binding of libptx_amd.so (the C ABI declared in include/ptx_amd.h).

There is deliberately no fallback: if the shared library is missing or a symbol cannot be
resolved this module raises, and every model in the package is unusable (SURVEY.md 8b:
"the product path must fail loudly when the HIP extension is missing").
"""
import ctypes as C
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libptx_amd.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "ptx_amd.h")
WINO4_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "ptx_amd_wino4.h")      # the F(4x4) Winograd calls
TFIR_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "ptx_amd_tfir.h")        # the stem's temporal fast-FIR calls
YUV16_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "ptx_amd_yuv16.h")      # 10- / 12-bit YUV 4:2:0 sources
COLOR_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "ptx_amd_color.h")      # ColorJitter / RandomGrayscale on uint8 frames
RANDAUG_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "ptx_amd_randaug.h")  # RandAugment on uint8 frames
RESAMPLE_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "ptx_amd_resample.h")  # PIL's other resize filters
MIX_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "ptx_amd_mix.h")          # RandomErasing + MixUp / CutMix
STEM_STRIDED_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "ptx_amd_stem_strided.h")  # the frame-strided bf16 stem
NL_KS_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "ptx_amd_nl_ks.h")      # the bf16 attention's two forms by name
LINEAR_BF16_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "ptx_amd_linear_bf16.h")  # Linear layers with bf16 weights
BN_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "ptx_amd_bn.h")            # batch-statistics BatchNorm (update_bn)
WARP_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "ptx_amd_warp.h")        # interpolated affine / perspective warps
BLUR_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "ptx_amd_blur.h")        # GaussianBlur on uint8 frames
CAM_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "ptx_amd_cam.h")          # class activation maps + overlay
DW_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "ptx_amd_dw.h")            # depthwise 3-D convolution (CSN)

PTX_EPI_RELU = 1
PTX_EPI_RES_ADD = 2
PTX_EPI_RES_PADA = 4
PTX_PRO_RELU = 8
PTX_EPI_ACCUM = 16
PTX_EPI_RES_UP = 64
PTX_F16_OPERANDS = 128
PTX_F16X3_OPERANDS = 0x8000
PTX_SPLITK_FUSED = 0x10000
PTX_BF16_OPERANDS = 0x20000      # with PTX_F16_OPERANDS: bfloat16 operands / 16-bit outputs and skips (bf16 plans)
PTX_PACK_BF16 = 3                # ptx_pack_desc.f16: filter written as bf16
PTX_ACT_OUT_F16 = 0x100
PTX_ACT_OUT_BF16 = 0x200         # ptx_affine_act_upsample: y written as bf16 (the fp32 result rounded once)
PTX_EPI_OUT_F16, PTX_EPI_AFFINE, PTX_EPI_DUAL_RAW, PTX_RES_F16, PTX_PRO_UP2, PTX_EPI_TANH = 0x200, 0x400, 0x800, 0x1000, 0x2000, 0x4000


class PtxError(RuntimeError):
    """`status` carries the library's status code (PTX_ERR_*: 1 invalid, 2 unsupported, 3 HIP, 4 workspace) when the
    error came from a libptx_amd call, else None."""
    status = None


class ConvDesc(C.Structure):
    _fields_ = [(n, C.c_int32) for n in
                ("N", "Ti", "Hi", "Wi", "Ci", "ldx", "To", "Ho", "Wo", "Co", "ldy",
                 "kT", "kH", "kW", "sT", "sH", "sW", "pT", "pH", "pW", "Kc", "Co_pad")] + \
               [("flags", C.c_uint32)] + \
               [(n, C.c_int32) for n in
                ("ldr", "res_C", "res_T", "res_H", "res_W", "res_sT", "res_sH", "res_sW",
                 "x2_C", "x2_ld", "x2_T", "x2_H", "x2_W", "x2_sT", "x2_sH", "x2_sW", "groups")]

    def key(self):
        """Identity of a conv PROBLEM for the tuned-tile table: every field, minus flag bits that do not change which
        tile is fastest by construction of the table (PTX_SPLITK_FUSED arrived after the table was keyed)."""
        return tuple((getattr(self, f) & ~0x10000) if f == "flags" else getattr(self, f) for f, _ in self._fields_)


class ConvStage(C.Structure):
    """ptx_conv_stage: one convolution of a conv program (ptx_conv_program_*)."""
    _fields_ = [("desc", ConvDesc), ("x", C.c_void_p), ("x2", C.c_void_p), ("w_packed", C.c_void_p), ("bias", C.c_void_p),
                ("res", C.c_void_p), ("y", C.c_void_p), ("tile", C.c_int32), ("split_k", C.c_int32)]


class ConvProgramInfo(C.Structure):
    """ptx_conv_program_info: sizes of a planned / built conv program."""
    _fields_ = [("n_stages", C.c_int32), ("total_items", C.c_int32), ("ctrl_words", C.c_int32), ("lds_bytes", C.c_int32),
                ("launches_replaced", C.c_int32), ("n_chunks", C.c_int32), ("image_bytes", C.c_uint64),
                ("workspace_bytes", C.c_uint64)]


class ConvFusedExt(C.Structure):
    """ptx_conv_fused_ext: operands of the fused generator-stage epilogue."""
    _fields_ = [("scale", C.c_void_p), ("shift", C.c_void_p), ("ld_affine", C.c_int32), ("ld_raw", C.c_int32),
                ("y_raw", C.c_void_p)]


class PackDesc(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("Co", "Ci", "kT", "kH", "kW", "Kc", "Co_pad", "fold_kw",
                                         "ld_k", "k_off", "bias_accumulate", "sub_groups", "co_per_super", "f16")]


class PoolDesc(C.Structure):
    _fields_ = [(n, C.c_int32) for n in
                ("N", "Ti", "Hi", "Wi", "C", "ld", "To", "Ho", "Wo",
                 "kT", "kH", "kW", "sT", "sH", "sW", "pT", "pH", "pW", "ldy")] + [("flags", C.c_uint32)]


class NormDesc(C.Structure):
    """ptx_norm_desc: TransformImage's tensor half (reference transforms/utils.py:72-75)."""
    _fields_ = [("mean", C.c_float * 4), ("std", C.c_float * 4), ("swap_rb", C.c_int32), ("to_255", C.c_int32)]

    @classmethod
    def make(cls, mean, std, input_space="RGB", input_range=(0, 1)):
        d = cls()
        for i in range(4):
            d.mean[i] = float(mean[i]) if i < len(mean) else 0.0
            d.std[i] = float(std[i]) if i < len(std) else 1.0
        d.swap_rb = int(input_space == "BGR")
        d.to_255 = int(max(input_range) == 255)
        return d


class ResizeDesc(C.Structure):
    """ptx_resize_desc: bilinear resize + crop of uint8 frames through host-built coefficient tables (PIL's arithmetic)."""
    _fields_ = [(n, C.c_int32) for n in ("N", "T", "H", "W", "C", "Ho", "Wo", "taps_h", "taps_w", "out_mode")]


class ResizeWindow(C.Structure):
    """ptx_resize_window: one clip's crop window in the resized frame and its flips (ptx_resize_frames_*_windows)."""
    _fields_ = [(n, C.c_int32) for n in ("top", "left", "hflip", "vflip")]


class ResizeGeom(C.Structure):
    """ptx_resize_geom: one clip's resize geometry (ptx_resize_build_tables): box in the frame, resized extent, window, flips."""
    _fields_ = [(n, C.c_int32) for n in ("box_top", "box_left", "box_h", "box_w", "h", "w", "top", "left", "hflip", "vflip")]


PTX_RESIZE_OUT_U8, PTX_RESIZE_OUT_F32, PTX_RESIZE_OUT_BF16 = 0, 1, 2
PTX_RESIZE_MAX_TAPS = 64
# ptx_amd_resample.h: Pillow's filter codes (Image.Resampling), and the longest NEAREST walk of the device builder
(PTX_RESAMPLE_NEAREST, PTX_RESAMPLE_LANCZOS, PTX_RESAMPLE_BILINEAR, PTX_RESAMPLE_BICUBIC, PTX_RESAMPLE_BOX,
 PTX_RESAMPLE_HAMMING) = range(6)
PTX_RESAMPLE_NEAREST_MAX_EXTENT = 65536
PTX_STEM_SRC_BF16_NCDHW, PTX_STEM_SRC_U8_NTHWC = 0, 1       # ptx_conv_stem_bf16_fwd: where the stem reads its input
PTX_VIEWS_MAX_CROPS = 4
PTX_VIEWS_SHARE_AUTO, PTX_VIEWS_SHARE_ALWAYS, PTX_VIEWS_SHARE_NEVER = 0, 1, 2


class ViewsDesc(C.Structure):
    """ptx_views_desc: clips x crops views of a decoded video, sampled through a frame index table and union tables."""
    _fields_ = [(n, C.c_int32) for n in ("N", "Tv", "H", "W", "C", "clips", "T", "crops")] + \
               [("stride_n", C.c_int64), ("stride_t", C.c_int64)] + \
               [(n, C.c_int32) for n in ("S", "Ur", "Uc", "taps_h", "taps_w")] + \
               [("row_off", C.c_int32 * PTX_VIEWS_MAX_CROPS), ("col_off", C.c_int32 * PTX_VIEWS_MAX_CROPS)] + \
               [(n, C.c_int32) for n in ("v0", "nv", "out_mode", "share")]


class Yuv420Src(C.Structure):
    """ptx_yuv420_src: the planes of a YUV 4:2:0 source (NV12 / I420, any row pitch) and the colour coefficients."""
    _fields_ = [("y", C.c_void_p), ("u", C.c_void_p), ("v", C.c_void_p)] + \
               [(n, C.c_int64) for n in ("stride_n_y", "stride_t_y", "stride_n_c", "stride_t_c")] + \
               [(n, C.c_int32) for n in ("pitch_y", "pitch_c", "step_c", "y_off", "ky", "krv", "kgu", "kgv", "kbu")]


class ClipSrc(C.Structure):
    """ptx_clip_src: the source of one OUTPUT clip of ptx_resize_clips_u8 (its video's frame 0, frame stride, size, length)."""
    _fields_ = [("base", C.c_void_p), ("stride_t", C.c_int64), ("H", C.c_int32), ("W", C.c_int32), ("Tv", C.c_int32),
                ("reserved", C.c_int32)]


class ClipSrcYuv420(C.Structure):
    """ptx_clip_src_yuv420: the same for ptx_resize_clips_yuv420 (the planes at frame 0 of the clip's video)."""
    _fields_ = [("planes", Yuv420Src), ("H", C.c_int32), ("W", C.c_int32), ("Tv", C.c_int32), ("reserved", C.c_int32)]


class Yuv420P16Src(C.Structure):
    """ptx_yuv420p16_src (ptx_amd_yuv16.h): ptx_yuv420_src with 16-bit words of `bits` significant bits, `shift` bits up."""
    _fields_ = Yuv420Src._fields_ + [("bits", C.c_int32), ("shift", C.c_int32)]


class ClipSrcYuv420P16(C.Structure):
    """ptx_clip_src_yuv420p16: the per-clip row of ptx_resize_clips_yuv420p16."""
    _fields_ = [("planes", Yuv420P16Src), ("H", C.c_int32), ("W", C.c_int32), ("Tv", C.c_int32), ("reserved", C.c_int32)]


class ColorDesc(C.Structure):
    """ptx_color_desc (ptx_amd_color.h): the frames of a ColorJitter launch, its output mode, whether a list holds contrast."""
    _fields_ = [(n, C.c_int32) for n in ("N", "T", "H", "W", "out_mode", "contrast")]


PTX_COLOR_NONE, PTX_COLOR_BRIGHTNESS, PTX_COLOR_CONTRAST, PTX_COLOR_SATURATION, PTX_COLOR_HUE, PTX_COLOR_GRAYSCALE = range(6)
PTX_COLOR_MAX_OPS = 5

class RandAugDesc(C.Structure):
    """ptx_randaug_desc (ptx_amd_randaug.h): the frames of one RandAugment position, its output mode, the fill colour."""
    _fields_ = [(n, C.c_int32) for n in ("N", "T", "H", "W", "out_mode", "num_ops", "position", "stats", "fill_r", "fill_g", "fill_b",
                                         "reserved")]


(PTX_RANDAUG_IDENTITY, PTX_RANDAUG_SHEAR_X, PTX_RANDAUG_SHEAR_Y, PTX_RANDAUG_TRANSLATE_X, PTX_RANDAUG_TRANSLATE_Y, PTX_RANDAUG_ROTATE,
 PTX_RANDAUG_BRIGHTNESS, PTX_RANDAUG_COLOR, PTX_RANDAUG_CONTRAST, PTX_RANDAUG_SHARPNESS, PTX_RANDAUG_POSTERIZE, PTX_RANDAUG_SOLARIZE,
 PTX_RANDAUG_AUTOCONTRAST, PTX_RANDAUG_EQUALIZE) = range(14)
PTX_RANDAUG_NUM_CODES, PTX_RANDAUG_MAX_OPS, PTX_RANDAUG_ROW, PTX_RANDAUG_STATS_WORDS = 14, 4, 8, 770


class MixDesc(C.Structure):
    """ptx_mix_desc (ptx_amd_mix.h): the clips of a BatchMix launch, its source and output modes, the size of the noise buffer."""
    _fields_ = [(n, C.c_int32) for n in ("N", "T", "H", "W", "src_mode", "out_mode")] + [("noise_elems", C.c_int64)]


PTX_MIX_NONE, PTX_MIX_MIXUP, PTX_MIX_CUTMIX = range(3)
PTX_MIX_ERASE_NONE, PTX_MIX_ERASE_CONST, PTX_MIX_ERASE_NOISE = range(3)
PTX_MIX_SRC_U8, PTX_MIX_SRC_F32, PTX_MIX_SRC_BF16 = range(3)
(PTX_MIX_W_PARTNER, PTX_MIX_W_MODE, PTX_MIX_W_A, PTX_MIX_W_B, PTX_MIX_W_BOX, PTX_MIX_W_ERASE, PTX_MIX_W_ERASE_KIND, PTX_MIX_W_CONST,
 PTX_MIX_W_NOISE, PTX_MIX_ROW) = 0, 1, 2, 3, 4, 8, 12, 13, 16, 20


class WarpDesc(C.Structure):
    """ptx_warp_desc (ptx_amd_warp.h): the frames of a warp launch, its filter (a PTX_RESAMPLE_* code), the fill colour."""
    _fields_ = [(n, C.c_int32) for n in ("N", "T", "H", "W", "filter", "fill_r", "fill_g", "fill_b", "reserved")]


PTX_WARP_IDENTITY, PTX_WARP_AFFINE, PTX_WARP_PERSPECTIVE = range(3)
PTX_WARP_COEFFS = 8


class BlurDesc(C.Structure):
    """ptx_blur_desc (ptx_amd_blur.h): the frames of a GaussianBlur launch, the tap counts of its two passes, its output mode."""
    _fields_ = [(n, C.c_int32) for n in ("N", "T", "H", "W", "kx", "ky", "out_mode")]


PTX_BLUR_MAX_TAPS = 33


class CamOverlayDesc(C.Structure):
    """ptx_cam_overlay_desc (ptx_amd_cam.h): the maps and the frames of an overlay launch, the tables' pitches, the mode, alpha."""
    _fields_ = [(n, C.c_int32) for n in ("N", "k", "Tm", "h", "w", "T", "H", "W", "taps_h", "taps_w", "mode")] + [("alpha", C.c_float)]


PTX_CAM_MAX_CLASSES, PTX_CAM_MAX_LDS_BYTES, PTX_CAM_MAX_MAP_BYTES = 8, 65536, 40960
PTX_CAM_OUT_OVERLAY, PTX_CAM_OUT_HEAT, PTX_CAM_OUT_MAP = range(3)

PTX_POOL_SAME, PTX_POOL_PAD_ZERO, PTX_POOL_BF16 = 1, 2, 4
PTX_REL_MAX_SETS, PTX_REL_MAX_FRAMES = 8, 16


class RelationDesc(C.Structure):
    """ptx_relation_desc: frame subsets of one TRN relation scale (reference trn.py:101-110)."""
    _fields_ = [("B", C.c_int32), ("n_sets", C.c_int32), ("n_frames", C.c_int32), ("frame_len", C.c_int32),
                ("idx", (C.c_int32 * PTX_REL_MAX_FRAMES) * PTX_REL_MAX_SETS)]


class NonlocalDesc(C.Structure):
    """ptx_nonlocal_desc: fused theta^T phi -> softmax -> . g (reference nonlocalnet.py:143-166)."""
    _fields_ = [(n, C.c_int32) for n in ("batch", "Nq", "Nk", "d", "dv", "ld_theta", "ld_phi", "ld_g", "ld_y")] + \
               [(n, C.c_int64) for n in ("bs_theta", "bs_phi", "bs_g", "bs_y")] + [("mode", C.c_int32)]


PTX_NL_SOFTMAX, PTX_NL_SCALE, PTX_NL_F16, PTX_NL_X3, PTX_NL_RELU, PTX_NL_OUT_F16, PTX_NL_BF16 = 0, 1, 2, 4, 8, 16, 32


class RgbConvDesc(C.Structure):
    """ptx_rgb_conv_desc: the generator's output layer BN -> ReLU -> conv3x3(C -> 3) -> tanh in one launch."""
    _fields_ = [(n, C.c_int32) for n in ("N", "H", "W", "C", "ldx", "ldy", "ld_affine")] + [("flags", C.c_uint32)]


_P = C.c_void_p
_I = C.c_int32
_L = C.c_int64
_U = C.c_uint32
_Z = C.c_size_t

# name -> (restype, argtypes); must list every function declared in include/ptx_amd.h
SIGNATURES = {
    "ptx_version": (C.c_char_p, []),
    "ptx_last_error": (C.c_char_p, []),
    "ptx_conv3d_num_configs": (C.c_int, []),
    "ptx_conv3d_num_configs_bf16": (C.c_int, []),
    "ptx_conv3d_config_name": (C.c_char_p, [C.c_int]),
    "ptx_conv3d_config_supported": (C.c_int, [C.POINTER(ConvDesc), C.c_int]),
    "ptx_conv3d_pick_config": (C.c_int, [C.POINTER(ConvDesc), C.POINTER(C.c_int)]),
    "ptx_conv3d_workspace_bytes": (_Z, [C.POINTER(ConvDesc), C.c_int]),
    "ptx_conv3d_fwd": (C.c_int, [C.POINTER(ConvDesc), _P, _P, _P, _P, _P, _P, _Z, C.c_int, C.c_int, _P]),
    "ptx_conv3d_fused_fwd": (C.c_int, [C.POINTER(ConvDesc), _P, _P, _P, _P, _P, C.POINTER(ConvFusedExt), _P, _Z, C.c_int,
                                       C.c_int, _P]),
    "ptx_conv3d_dual_fwd": (C.c_int, [C.POINTER(ConvDesc), _P, _P, _P, _P, _P, _P, _Z, C.c_int, C.c_int, _P]),
    "ptx_conv3d_chain_num_configs": (C.c_int, []),
    "ptx_conv3d_chain_config_name": (C.c_char_p, [C.c_int]),
    "ptx_conv3d_chain_supported": (C.c_int, [C.POINTER(ConvDesc), C.POINTER(ConvDesc), C.c_int]),
    "ptx_conv3d_chain_pick_config": (C.c_int, [C.POINTER(ConvDesc), C.POINTER(ConvDesc)]),
    "ptx_conv3d_chain_fwd": (C.c_int, [C.POINTER(ConvDesc), C.POINTER(ConvDesc), _P, _P, _P, _P, _P, _P, _P, C.c_int, _P]),
    "ptx_conv_body_f32_supported": (C.c_int, [C.POINTER(ConvDesc), C.c_int]),
    "ptx_conv_body_f32_weight_elems": (C.c_size_t, [C.POINTER(ConvDesc)]),
    "ptx_pack_conv_body_f32_weight": (C.c_int, [C.POINTER(ConvDesc), _P, _P, _P]),
    "ptx_conv_body_f32_fwd": (C.c_int, [C.POINTER(ConvDesc), _P, _P, _P, _P, _P, C.c_int, _P]),
    "ptx_conv_body_chain_f32_supported": (C.c_int, [C.POINTER(ConvDesc), C.POINTER(ConvDesc), C.c_int]),
    "ptx_conv_body_tail_f32_weight_elems": (C.c_size_t, [C.POINTER(ConvDesc)]),
    "ptx_pack_conv_body_tail_f32_weight": (C.c_int, [C.POINTER(ConvDesc), _P, _P, _P]),
    "ptx_conv_body_chain_f32_fwd": (C.c_int, [C.POINTER(ConvDesc), C.POINTER(ConvDesc), _P, _P, _P, _P, _P, _P, _P, C.c_int, _P]),
    "ptx_conv_wino_f32_supported": (C.c_int, [C.POINTER(ConvDesc)]),
    "ptx_conv_wino_f32_workspace_bytes": (C.c_size_t, [C.POINTER(ConvDesc)]),
    "ptx_conv_wino_f32_gemm_desc": (C.c_int, [C.POINTER(ConvDesc), C.POINTER(ConvDesc)]),
    "ptx_wino_f32_weight_elems": (C.c_size_t, [C.POINTER(ConvDesc)]),
    "ptx_pack_wino_f32_weight": (C.c_int, [C.POINTER(ConvDesc), _P, _P, _P]),
    "ptx_wino_in_f32": (C.c_int, [C.POINTER(ConvDesc), _P, _P, _P]),
    "ptx_wino_out_f32": (C.c_int, [C.POINTER(ConvDesc), _P, _P, _P, _P, _P]),
    "ptx_conv_program_num_tiles": (C.c_int, []),
    "ptx_conv_program_tile_name": (C.c_char_p, [C.c_int]),
    "ptx_conv_program_plan": (C.c_int, [C.POINTER(ConvStage), _I, C.POINTER(ConvProgramInfo)]),
    "ptx_conv_program_describe": (C.c_int, [C.POINTER(ConvStage), _I, C.c_char_p, _Z]),
    "ptx_conv_program_build": (C.c_int, [C.POINTER(ConvStage), _I, _P, _Z, _P, _Z, C.POINTER(ConvProgramInfo)]),
    "ptx_conv_program_fwd": (C.c_int, [C.POINTER(ConvProgramInfo), _P, _P, _I, _P]),
    "ptx_conv_program_trace_fwd": (C.c_int, [C.POINTER(ConvProgramInfo), _P, _P, _I, _P, _Z, _P]),
    "ptx_conv_program_error": (C.c_int, [_P, C.POINTER(C.c_int32), _P]),
    "ptx_ncdhw_to_split4": (C.c_int, [_P, _P, _I, _I, _L, _P]),
    "ptx_conv_stem_x3_supported": (C.c_int, [C.POINTER(ConvDesc)]),
    "ptx_conv_stem_x3_fwd": (C.c_int, [C.POINTER(ConvDesc), _P, _P, _P, _P, _P]),
    "ptx_ncdhw_to_split_planes": (C.c_int, [_P, _P, _I, _I, _I, _I, _I, _P]),
    "ptx_conv_stem_x3p_supported": (C.c_int, [C.POINTER(ConvDesc)]),
    "ptx_stem_x3p_weight_elems": (C.c_size_t, [C.POINTER(ConvDesc)]),
    "ptx_pack_stem_x3p_weight": (C.c_int, [C.POINTER(ConvDesc), _P, _P, _P]),
    "ptx_conv_stem_x3p_fwd": (C.c_int, [C.POINTER(ConvDesc), _P, _P, _P, _P, _P]),
    "ptx_conv_stem_f32_supported": (C.c_int, [C.POINTER(ConvDesc), _L, _L, _L]),
    "ptx_stem_f32_weight_elems": (C.c_size_t, [C.POINTER(ConvDesc)]),
    "ptx_pack_stem_f32_weight": (C.c_int, [C.POINTER(ConvDesc), _P, _I, _P, _P]),
    "ptx_conv_stem_f32_fwd": (C.c_int, [C.POINTER(ConvDesc), _P, _L, _L, _L, _P, _P, _P, _P]),
    "ptx_conv_stem_bf16_supported": (C.c_int, [C.POINTER(ConvDesc), _I]),
    "ptx_stem_bf16_weight_elems": (C.c_size_t, [C.POINTER(ConvDesc)]),
    "ptx_pack_stem_bf16_weight": (C.c_int, [C.POINTER(ConvDesc), _P, _P, _P]),
    "ptx_conv_stem_bf16_fwd": (C.c_int, [C.POINTER(ConvDesc), _P, _I, C.POINTER(NormDesc), _P, _P, _P, _P]),
    "ptx_packed_weight_elems": (_Z, [C.POINTER(PackDesc)]),
    "ptx_pack_conv_weight": (C.c_int, [C.POINTER(PackDesc), _P, _P, _P, _P, _P, _P, C.c_float, _P, _P, _P]),
    "ptx_checksum_f32": (C.c_int, [_P, _I, _P, _P]),
    "ptx_checksum_b16": (C.c_int, [_P, _I, _P, _P]),
    "ptx_ncdhw_to_ndhwc_bf16": (C.c_int, [_P, _P, _I, _I, _L, _I, _P]),
    "ptx_ndhwc_to_ncdhw_bf16": (C.c_int, [_P, _P, _I, _I, _L, _I, _P]),
    "ptx_im2col_hw_bf16": (C.c_int, [_P, _P] + [_I] * 14 + [_P]),
    "ptx_f32_to_bf16": (C.c_int, [_P, _P, _L, _P]),
    "ptx_bf16_to_f32": (C.c_int, [_P, _P, _L, _P]),
    "ptx_global_avgpool_bf16": (C.c_int, [_P, _P, _I, _I, _L, _I, _P]),
    "ptx_ncdhw_to_ndhwc": (C.c_int, [_P, _P, _I, _I, _L, _I, _P]),
    "ptx_ndhwc_to_ncdhw": (C.c_int, [_P, _P, _I, _I, _L, _I, _P]),
    "ptx_fold_kw_ncdhw": (C.c_int, [_P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _P]),
    "ptx_fold_kw_strided": (C.c_int, [_P, _P, _I, _I, _I, _I, _I, _L, _L, _L, _I, _I, _I, _I, _I, _P]),
    "ptx_pad_rows": (C.c_int, [_P, _P, _L, _I, _I, _P]),
    "ptx_frames_u8_to_ncdhw": (C.c_int, [_P, _P, _I, _I, _I, _I, _I, C.POINTER(NormDesc), _P]),
    "ptx_fold_kw_frames_u8": (C.c_int, [_P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, C.POINTER(NormDesc), _P]),
    "ptx_resize_frames_u8_supported": (C.c_int, [C.POINTER(ResizeDesc)]),
    "ptx_resize_frames_u8": (C.c_int, [C.POINTER(ResizeDesc), _P, _P, _P, _P, _P, _P, _P, _P, C.POINTER(NormDesc), _P]),
    "ptx_resize_views_u8_supported": (C.c_int, [C.POINTER(ViewsDesc)]),
    "ptx_resize_views_u8": (C.c_int, [C.POINTER(ViewsDesc), _P, _P, _P, _P, _P, _P, _P, _P, _P, C.POINTER(NormDesc), _P]),
    "ptx_resize_frames_yuv420_supported": (C.c_int, [C.POINTER(ResizeDesc), C.POINTER(Yuv420Src)]),
    "ptx_resize_frames_yuv420": (C.c_int, [C.POINTER(ResizeDesc), C.POINTER(Yuv420Src), _P, _P, _P, _P, _P, _P, _P,
                                           C.POINTER(NormDesc), _P]),
    "ptx_resize_frames_u8_windows_supported": (C.c_int, [C.POINTER(ResizeDesc), _I, _I]),
    "ptx_resize_frames_u8_windows": (C.c_int, [C.POINTER(ResizeDesc), _P, _P, _P, _P, _P, _P, _P, _I, _I, _P, _P,
                                               C.POINTER(NormDesc), _P]),
    "ptx_resize_frames_yuv420_windows_supported": (C.c_int, [C.POINTER(ResizeDesc), C.POINTER(Yuv420Src), _I, _I]),
    "ptx_resize_frames_yuv420_windows": (C.c_int, [C.POINTER(ResizeDesc), C.POINTER(Yuv420Src), _P, _P, _P, _P, _P, _P, _I, _I,
                                                   _P, _P, C.POINTER(NormDesc), _P]),
    "ptx_resize_frames_u8_tables_supported": (C.c_int, [C.POINTER(ResizeDesc)]),
    "ptx_resize_frames_u8_tables": (C.c_int, [C.POINTER(ResizeDesc), _P, _P, _P, _P, _P, _P, _P, _P, C.POINTER(NormDesc), _P]),
    "ptx_resize_frames_yuv420_tables_supported": (C.c_int, [C.POINTER(ResizeDesc), C.POINTER(Yuv420Src)]),
    "ptx_resize_frames_yuv420_tables": (C.c_int, [C.POINTER(ResizeDesc), C.POINTER(Yuv420Src), _P, _P, _P, _P, _P, _P, _P,
                                                  C.POINTER(NormDesc), _P]),
    "ptx_resize_build_tables": (C.c_int, [C.POINTER(ResizeDesc), _P, _P, _P, _P, _P, _P, _P, _P]),
    "ptx_resize_clips_u8_supported": (C.c_int, [C.POINTER(ResizeDesc)]),
    "ptx_resize_clips_u8": (C.c_int, [C.POINTER(ResizeDesc), _P, _P, _P, _P, _P, _P, _P, _P, _P, C.POINTER(NormDesc), _P]),
    "ptx_resize_clips_yuv420_supported": (C.c_int, [C.POINTER(ResizeDesc)]),
    "ptx_resize_clips_yuv420": (C.c_int, [C.POINTER(ResizeDesc), _P, _P, _P, _P, _P, _P, _P, _P, _P, C.POINTER(NormDesc), _P]),
    "ptx_resize_build_tables_clips": (C.c_int, [C.POINTER(ResizeDesc), _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "ptx_resize_views_yuv420_supported": (C.c_int, [C.POINTER(ViewsDesc), C.POINTER(Yuv420Src)]),
    "ptx_resize_views_yuv420": (C.c_int, [C.POINTER(ViewsDesc), C.POINTER(Yuv420Src), _P, _P, _P, _P, _P, _P, _P, _P,
                                          C.POINTER(NormDesc), _P]),
    "ptx_views_mean": (C.c_int, [_P, _P, _I, _I, _I, _L, _I, _I, _P]),
    "ptx_maxpool3d_fwd": (C.c_int, [C.POINTER(PoolDesc), _P, _P, _P]),
    "ptx_cbn_fold": (C.c_int, [_P, _P, _P, _P, C.c_float, _P, _P, _I, _I, _I, _I, _I, _I, _P]),
    "ptx_affine_act_upsample": (C.c_int, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _I, _P]),
    "ptx_outer_sum_relu": (C.c_int, [_P, _P, _P, _I, _I, _I, _I, _P]),
    "ptx_copy2d": (C.c_int, [_P, _P, _L, _I, _L, _L, _P]),
    "ptx_window_mean": (C.c_int, [_P, _P, _I, _I, _I, _I, _I, _P]),
    "ptx_global_avgpool": (C.c_int, [_P, _P, _I, _I, _L, _I, _I, _P]),
    "ptx_linear_fwd": (C.c_int, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _U, _P]),
    "ptx_relation_linear_fwd": (C.c_int, [C.POINTER(RelationDesc), _P, _I, _P, _P, _P, _I, _I, _U, _P]),
    "ptx_linear_setsum_fwd": (C.c_int, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _U, _P]),
    "ptx_nonlocal_supported": (C.c_int, [C.POINTER(NonlocalDesc)]),
    "ptx_nonlocal_fwd": (C.c_int, [C.POINTER(NonlocalDesc), _P, _P, _P, _P, _P]),
    "ptx_nonlocal_bf16_fwd": (C.c_int, [C.POINTER(NonlocalDesc), _P, _P, _P, _P, _P]),
    "ptx_nonlocal_workspace_bytes": (C.c_size_t, [C.POINTER(NonlocalDesc)]),
    "ptx_nonlocal_ws_fwd": (C.c_int, [C.POINTER(NonlocalDesc), _P, _P, _P, _P, _P, C.c_size_t, _P]),
    "ptx_bgemm_nt": (C.c_int, [_P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _L, _L, _L, _P]),
    "ptx_softmax_rows": (C.c_int, [_P, _L, _I, _I, _I, _P]),
    "ptx_transpose_last2": (C.c_int, [_P, _P, _I, _I, _I, _I, _I, _P]),
    "ptx_conv1x1_skip_f16_supported": (C.c_int, [C.POINTER(ConvDesc)]),
    "ptx_conv1x1_skip_f16_fwd": (C.c_int, [C.POINTER(ConvDesc), _P, _P, _P, _P, _P, C.POINTER(ConvFusedExt), _P]),
    "ptx_conv1x1_pro_f16_supported": (C.c_int, [C.POINTER(ConvDesc)]),
    "ptx_conv1x1_pro_f16_fwd": (C.c_int, [C.POINTER(ConvDesc), _P, C.POINTER(ConvFusedExt), _P, _P, _P, C.POINTER(ConvFusedExt), _P]),
    "ptx_conv3x3_f16_supported": (C.c_int, [C.POINTER(ConvDesc)]),
    "ptx_conv3x3_f16_fwd": (C.c_int, [C.POINTER(ConvDesc), _P, _P, _P, _P, C.POINTER(ConvFusedExt), _P]),
    "ptx_conv3x3_bf16_supported": (C.c_int, [C.POINTER(ConvDesc)]),
    "ptx_conv3x3_bf16_fwd": (C.c_int, [C.POINTER(ConvDesc), _P, _P, _P, _P, C.POINTER(ConvFusedExt), _P]),
    "ptx_conv1x1_skip_bf16_supported": (C.c_int, [C.POINTER(ConvDesc)]),
    "ptx_conv1x1_skip_bf16_fwd": (C.c_int, [C.POINTER(ConvDesc), _P, _P, _P, _P, _P, C.POINTER(ConvFusedExt), _P]),
    "ptx_rgb_conv3x3_f16_supported": (C.c_int, [C.POINTER(RgbConvDesc)]),
    "ptx_rgb_conv_weight_elems": (_Z, [_I]),
    "ptx_pack_rgb_conv_weight": (C.c_int, [_P, _I, _P, _P]),
    "ptx_rgb_conv3x3_f16_fwd": (C.c_int, [C.POINTER(RgbConvDesc), _P, _P, _P, _P, _P, _P, _P]),
}


# include/ptx_amd_wino4.h: the Winograd F(4x4,3x3) entry points, bound next to SIGNATURES (tests/test_wino4_host.py keeps the
# header, this table and the library's exports in step)
SIGNATURES_WINO4 = {
    "ptx_conv_wino4_f32_supported": (C.c_int, [C.POINTER(ConvDesc)]),
    "ptx_conv_wino4_f32_workspace_bytes": (C.c_size_t, [C.POINTER(ConvDesc)]),
    "ptx_conv_wino4_f32_gemm_desc": (C.c_int, [C.POINTER(ConvDesc), C.POINTER(ConvDesc)]),
    "ptx_wino4_f32_weight_elems": (C.c_size_t, [C.POINTER(ConvDesc)]),
    "ptx_pack_wino4_f32_weight": (C.c_int, [C.POINTER(ConvDesc), _P, _P, _P]),
    "ptx_wino4_in_f32": (C.c_int, [C.POINTER(ConvDesc), _P, _P, _P]),
    "ptx_wino4_out_f32": (C.c_int, [C.POINTER(ConvDesc), _P, _P, _P, _P, _P]),
}


# include/ptx_amd_tfir.h: the fp32 stem as a fast FIR along time (csrc/conv_stem_tfir_f32.hip), bound the same way
# (tests/test_stem_tfir_host.py)
_F = C.POINTER(C.c_float)
SIGNATURES_TFIR = {
    "ptx_stem_tfir_scheme": (C.c_int, [_I, C.POINTER(C.c_int32), C.POINTER(C.c_int32), _F, _F, _F]),
    "ptx_conv_stem_tfir_f32_supported": (C.c_int, [C.POINTER(ConvDesc), _L, _L, _L, _I]),
    "ptx_stem_tfir_f32_weight_elems": (C.c_size_t, [C.POINTER(ConvDesc), _I]),
    "ptx_stem_tfir_f32_workspace_bytes": (C.c_size_t, [C.POINTER(ConvDesc), _I]),
    "ptx_pack_stem_tfir_f32_weight": (C.c_int, [C.POINTER(ConvDesc), _I, _P, _P, _P]),
    "ptx_stem_tfir_in_f32": (C.c_int, [C.POINTER(ConvDesc), _I, _P, _L, _L, _L, _P, _P]),
    "ptx_conv_stem_tfir_f32_fwd": (C.c_int, [C.POINTER(ConvDesc), _I, _P, _P, _P, _P, _P]),
}


# include/ptx_amd_yuv16.h: the resize entry points on 10- / 12-bit YUV 4:2:0 sources, bound the same way
# (tests/test_yuv16_frames_host.py); every signature is its _yuv420 twin's with the 16-bit descriptor
SIGNATURES_YUV16 = {
    name.replace("_yuv420", "_yuv420p16"): (res, [C.POINTER(Yuv420P16Src) if a == C.POINTER(Yuv420Src) else a for a in args])
    for name, (res, args) in SIGNATURES.items() if "_yuv420" in name
}


# include/ptx_amd_color.h: per-clip ColorJitter / RandomGrayscale on uint8 frames (csrc/color_jitter.h), bound the same way
# (tests/test_color_jitter_host.py)
SIGNATURES_COLOR = {
    "ptx_color_jitter_supported": (C.c_int, [C.POINTER(ColorDesc), _P, _P]),
    "ptx_color_jitter_stats": (C.c_int, [C.POINTER(ColorDesc), _P, _P, _P, _P, _P]),
    "ptx_color_jitter_apply": (C.c_int, [C.POINTER(ColorDesc), _P, _P, _P, _P, _P, C.POINTER(NormDesc), _P]),
}


# include/ptx_amd_randaug.h: per-clip RandAugment on uint8 frames (csrc/rand_augment.h), bound the same way
# (tests/test_rand_augment_host.py)
SIGNATURES_RANDAUG = {
    "ptx_rand_augment_supported": (C.c_int, [C.POINTER(RandAugDesc), _P]),
    "ptx_rand_augment_stats": (C.c_int, [C.POINTER(RandAugDesc), _P, _P, _P, _P]),
    "ptx_rand_augment_apply": (C.c_int, [C.POINTER(RandAugDesc), _P, _P, _P, _P, C.POINTER(NormDesc), _P]),
}


# include/ptx_amd_resample.h: the per-clip table builders for PIL's other resize filters (csrc/pack_layout.hip,
# csrc/resize_clips.hip), bound the same way (tests/test_resample_frames_host.py): their bilinear twins' signatures with the
# filter code behind the geometry rows
SIGNATURES_RESAMPLE = {
    "ptx_resize_build_tables_filter": (C.c_int, [C.POINTER(ResizeDesc), _P, _I, _P, _P, _P, _P, _P, _P, _P]),
    "ptx_resize_build_tables_clips_filter": (C.c_int, [C.POINTER(ResizeDesc), _P, _P, _I, _P, _P, _P, _P, _P, _P, _P]),
}


# include/ptx_amd_mix.h: RandomErasing + MixUp / CutMix on the normalised clip in one launch (csrc/batch_mix.h), bound the same
# way (tests/test_batch_mix_host.py)
SIGNATURES_MIX = {
    "ptx_batch_mix_supported": (C.c_int, [C.POINTER(MixDesc), _P]),
    "ptx_batch_mix_apply": (C.c_int, [C.POINTER(MixDesc), _P, _P, _P, _P, C.POINTER(NormDesc), _P]),
    "ptx_batch_mix_targets": (C.c_int, [_P, _P, _P, _I, _I, C.c_float, C.c_float, _P]),
}


# include/ptx_amd_stem_strided.h: the patch-resident bf16 stem on every frame_step-th frame of its source
# (csrc/conv_stem_bf16.hip; bf16 SlowFast), bound the same way (tests/test_slowfast_bf16_host.py)
SIGNATURES_STEM_STRIDED = {
    "ptx_conv_stem_bf16_strided_supported": (C.c_int, [C.POINTER(ConvDesc), _I, _I, _I]),
    "ptx_conv_stem_bf16_strided_fwd": (C.c_int, [C.POINTER(ConvDesc), _P, _I, C.POINTER(NormDesc), _I, _I, _P, _P, _P, _P]),
}


# include/ptx_amd_nl_ks.h: the single-group / key-split forms of the bf16 attention by name (csrc/nonlocal_attn.hip), bound
# the same way (tests/test_nl_resnet_bf16_host.py)
SIGNATURES_NL_KS = {
    "ptx_nonlocal_bf16_variant": (C.c_int, [C.POINTER(NonlocalDesc)]),
    "ptx_nonlocal_bf16_variant_supported": (C.c_int, [C.POINTER(NonlocalDesc), _I]),
    "ptx_nonlocal_bf16_variant_fwd": (C.c_int, [C.POINTER(NonlocalDesc), _I, _P, _P, _P, _P, _P]),
}


# include/ptx_amd_linear_bf16.h: Linear layers with bf16 weights for few rows (csrc/linear_bf16.hip; the bf16 TRN heads), bound
# the same way (tests/test_trn_bf16_host.py)
PTX_LIN_X_BF16, PTX_LIN_X_F32 = 0, 1
SIGNATURES_LINEAR_BF16 = {
    "ptx_linear_bf16w_workspace_bytes": (C.c_size_t, [_I, _I, _I]),
    "ptx_linear_bf16w_supported": (C.c_int, [_P, _I, _P, _P, _P, _I, _I, _I, _I, _I, C.c_uint32]),
    "ptx_linear_bf16w_fwd": (C.c_int, [_P, _I, _P, _P, _P, _I, _I, _I, _I, _I, C.c_uint32, _P, C.c_size_t, _P]),
    "ptx_relation_linear_bf16w_supported": (C.c_int, [C.POINTER(RelationDesc), _P, _I, _P, _P, _P, _I, _I, C.c_uint32]),
    "ptx_relation_linear_bf16w_fwd": (C.c_int, [C.POINTER(RelationDesc), _P, _I, _P, _P, _P, _I, _I, C.c_uint32, _P, C.c_size_t, _P]),
    "ptx_linear_setsum_bf16w_supported": (C.c_int, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _I, C.c_uint32]),
    "ptx_linear_setsum_bf16w_fwd": (C.c_int, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _I, C.c_uint32, _P]),
}


class BnApplyDesc(C.Structure):
    """ptx_bn_apply_desc: y = act(raw * scale + shift [+ residual]) on [N][T][H][W] positions of C channels."""
    _fields_ = [(n, C.c_int32) for n in ("N", "T", "H", "W", "C", "ldx", "ldy")] + [("flags", C.c_uint32)] + \
               [(n, C.c_int32) for n in ("ldr", "res_C", "res_T", "res_H", "res_W", "res_sT", "res_sH", "res_sW")]


# include/ptx_amd_bn.h: batch-statistics BatchNorm forward (csrc/bn_batch.hip; update_bn), bound the same way
# (tests/test_update_bn_host.py)
SIGNATURES_BN = {
    "ptx_bn_batch_stats_workspace_bytes": (C.c_size_t, [_L, _I]),
    "ptx_bn_batch_stats_f32": (C.c_int, [_P, _L, _I, _I, _P, _P, _P, C.c_size_t, _P]),
    "ptx_bn_batch_update_f32": (C.c_int, [_P, _P, _L, C.c_float, C.c_float, _P, _P, _P, _P, _P, _P, _I, _P]),
    "ptx_bn_apply_f32": (C.c_int, [C.POINTER(BnApplyDesc), _P, _P, _P, _P, _P, _P]),
}


# include/ptx_amd_warp.h: interpolated per-clip affine / perspective warps of uint8 frames (csrc/warp_frames.h), bound the same
# way (tests/test_warp_frames_host.py)
SIGNATURES_WARP = {
    "ptx_warp_frames_supported": (C.c_int, [C.POINTER(WarpDesc), _P, _P]),
    "ptx_warp_frames": (C.c_int, [C.POINTER(WarpDesc), _P, _P, _P, _P, _P]),
}


# include/ptx_amd_blur.h: per-clip GaussianBlur of uint8 frames (csrc/blur_frames.h), bound the same way
# (tests/test_blur_frames_host.py)
SIGNATURES_BLUR = {
    "ptx_gaussian_blur_supported": (C.c_int, [C.POINTER(BlurDesc), _P, _P, _P]),
    "ptx_gaussian_blur_frames": (C.c_int, [C.POINTER(BlurDesc), _P, _P, _P, _P, _P, C.POINTER(NormDesc), _P]),
}


# include/ptx_amd_cam.h: class activation maps of the pool + Linear heads and their overlay on uint8 frames (csrc/cam.h), bound
# the same way (tests/test_cam_host.py)
SIGNATURES_CAM = {
    "ptx_cam_scores_supported": (C.c_int, [_I, _L, _I, _I, _I, _I, _I]),
    "ptx_cam_scores": (C.c_int, [_P, _I, _P, _P, _P, _P, _I, _L, _I, _I, _I, _I, _P]),
    "ptx_cam_quantize": (C.c_int, [_P, _P, _L, _L, _P]),
    "ptx_cam_overlay_supported": (C.c_int, [C.POINTER(CamOverlayDesc), _P, _P]),
    "ptx_cam_overlay": (C.c_int, [C.POINTER(CamOverlayDesc), _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
}

# include/ptx_amd_dw.h: the fp32 depthwise 3-D convolution of the channel-separated networks (csrc/conv_dw_f32.h), bound the same
# way (tests/test_csn_host.py)
SIGNATURES_DW = {
    "ptx_conv3d_dw_f32_supported": (C.c_int, [C.POINTER(ConvDesc)]),
    "ptx_pack_dw_weight_f32": (C.c_int, [_I, _I, _I, _I, _P, _P, _P, _P, _P, _P, C.c_float, _P, _P, _P]),
    "ptx_conv3d_dw_f32_fwd": (C.c_int, [C.POINTER(ConvDesc), _P, _P, _P, _P, _P]),
    "ptx_conv3d_dw_f32_force_form": (C.c_int, [_I]),
}
PTX_DW_FORM_STRIP4, PTX_DW_FORM_STRIP8, PTX_DW_FORM_LDS = 4, 8, 16


def header_symbols(path=HEADER_PATH):
    """Every function name declared in include/ptx_amd.h (used by the no-GPU ABI test)."""
    text = open(path).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(ptx_[a-z0-9_]+)\s*\(", text)))


def experimental_symbols(path=HEADER_PATH):
    """Function names declared with PTX_EXPERIMENTAL_API in include/ptx_amd.h: built, tested and exported, but off the
    default path (each measured slower than what the engine runs) -- their ABI is not part of the drop-in contract."""
    text = open(path).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"PTX_EXPERIMENTAL_API\s+[a-z_ \*]+?\b(ptx_[a-z0-9_]+)\s*\(", text)))


# the experimental part of SIGNATURES (kept in step with the header by tests/test_abi_and_host.py)
EXPERIMENTAL = ("ptx_conv_program_num_tiles", "ptx_conv_program_tile_name", "ptx_conv_program_plan", "ptx_conv_program_describe",
                "ptx_conv_program_build", "ptx_conv_program_fwd", "ptx_conv_program_trace_fwd", "ptx_conv_program_error",
                "ptx_nonlocal_workspace_bytes", "ptx_nonlocal_ws_fwd")

_lib = None


def lib():
    """Load (once) and return the shared library with typed entry points."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise PtxError(
                "libptx_amd.so not found at %s -- build it with "
                "`python pretorched-x_amd/csrc/build.py` (or __graft_entry__.build()); "
                "this package has no CPU / eager fallback" % LIB_PATH)
        handle = C.CDLL(LIB_PATH)
        for name, (res, args) in list(SIGNATURES.items()) + list(SIGNATURES_WINO4.items()) + list(SIGNATURES_TFIR.items()) + \
                list(SIGNATURES_YUV16.items()) + list(SIGNATURES_COLOR.items()) + list(SIGNATURES_RANDAUG.items()) + \
                list(SIGNATURES_RESAMPLE.items()) + list(SIGNATURES_MIX.items()) + list(SIGNATURES_STEM_STRIDED.items()) + \
                list(SIGNATURES_NL_KS.items()) + list(SIGNATURES_LINEAR_BF16.items()) + list(SIGNATURES_BN.items()) + \
                list(SIGNATURES_WARP.items()) + list(SIGNATURES_BLUR.items()) + list(SIGNATURES_CAM.items()) + \
                list(SIGNATURES_DW.items()):
            fn = getattr(handle, name)   # AttributeError if the symbol is missing: loud by design
            fn.restype = res
            fn.argtypes = args
        _lib = handle
    return _lib


def source_hash():
    """sha256 of the library's sources as they are in THIS tree (csrc/build.py:source_hash -- the same function build.py
    compiles into ptx_version()).  Equal to `binary_source_hash()` iff the loaded .so was built from this tree."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("ptx_build", os.path.join(_HERE, "csrc", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.source_hash()


def binary_source_hash():
    """The source hash the loaded libptx_amd.so carries (the part of ptx_version() after "src:")."""
    return lib().ptx_version().decode().rsplit("src:", 1)[-1]


def check(status, what=""):
    if status != 0:
        msg = lib().ptx_last_error().decode(errors="replace")
        err = PtxError("%s failed (status %d): %s" % (what or "libptx_amd call", status, msg))
        err.status = int(status)
        raise err
