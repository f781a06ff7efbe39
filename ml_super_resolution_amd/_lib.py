"""ctypes binding of libsrx.so (C ABI: include/srx.h).

There is NO fallback: if the shared library is missing or a call fails, an exception is
raised.  Nothing here imports the oracle.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, 'libsrx.so')

SRX_OK = 0
PAD_SAME, PAD_VALID = 0, 1
ACT_NONE, ACT_RELU, ACT_TANH, ACT_LRELU, ACT_SIGMOID = 0, 1, 2, 3, 4
OP_FWD, OP_BWD_DATA, OP_BWD_FILTER = 0, 1, 2
# srx_conv_desc.precision (include/srx.h): exact fp32, or split-bf16 products; named as torch.set_float32_matmul_precision
PRECISION_FP32, PRECISION_BF16X3 = 0, 1
PRECISION_BY_NAME = {'highest': PRECISION_FP32, 'high': PRECISION_BF16X3}

ACT_BY_NAME = {None: ACT_NONE, 'none': ACT_NONE, 'relu': ACT_RELU, 'tanh': ACT_TANH,
               'lrelu': ACT_LRELU, 'leaky_relu': ACT_LRELU, 'sigmoid': ACT_SIGMOID}
PAD_BY_NAME = {'same': PAD_SAME, 'valid': PAD_VALID}

# every symbol include/srx.h declares
EXPORTS = [
    'srx_version', 'srx_last_error', 'srx_set_conv_path', 'srx_set_wgrad_path', 'srx_set_chain', 'srx_set_chain_fixed', 'srx_conv_chain', 'srx_conv_chain_supported', 'srx_conv2d_precision_supported', 'srx_conv2d_workspace_bytes', 'srx_conv2d_fwd',
    'srx_conv2d_bwd_data', 'srx_conv2d_bwd_filter', 'srx_conv2d_bwd_filter_partials', 'srx_conv2d_bwd_filter_reduce',
    'srx_conv2d_bwd_filter_batch', 'srx_conv2d_bwd_filter_batch_workspace_bytes', 'srx_conv2d_bwd_filter_batch_plan', 'srx_set_wgrad_batch', 'srx_act_bwd', 'srx_depth_to_space',
    'srx_space_to_depth', 'srx_stream_copy', 'srx_mse_fwd_bwd', 'srx_l2_loss', 'srx_reduce_scratch_bytes',
    'srx_adam_tf_step', 'srx_adam_tf_step_dev', 'srx_momentum_clip_step', 'srx_rownorm_loss_fwd_bwd', 'srx_psnr', 'srx_ssim', 'srx_ssim_scratch_bytes', 'srx_saturate_u8', 'srx_affine', 'srx_u8_to_unit_float', 'srx_gaussian_blur', 'srx_resize_bilinear',
    'srx_upsample_nearest', 'srx_upsample_nearest_bwd', 'srx_add_relu_grad',
    'srx_conv2d_bwd_data_acc', 'srx_conv3x3_blocked', 'srx_conv3x3_blocked_bwd_filter_workspace_bytes', 'srx_conv3x3_blocked_bwd_filter',
    'srx_conv3x3_blocked_ex', 'srx_conv3x3_blocked_bwd_filter_ex_workspace_bytes', 'srx_conv3x3_blocked_bwd_filter_ex',
    'srx_espcn_forward', 'srx_espcn_forward_keep', 'srx_debug_poison_lds', 'srx_srcnn_forward', 'srx_maxpool2x2', 'srx_maxpool2x2_bwd', 'srx_maxpool2x2_bwd_masked', 'srx_subsample2', 'srx_subsample2_bwd',
    'srx_channel_blocks_to_nhwc', 'srx_nhwc_to_channel_blocks', 'srx_channel_normalize', 'srx_channel_normalize_bwd',
    'srx_extract_patches16', 'srx_texture_gram', 'srx_texture_gram_bwd', 'srx_pil_resample_ksize', 'srx_pil_resample_coeffs', 'srx_resample_u8', 'srx_u8_to_pm1', 'srx_log_loss', 'srx_vgg_preprocess', 'srx_add_scaled', 'srx_resize_bicubic_tf', 'srx_column_sums', 'srx_gemm_workspace_bytes', 'srx_gemm', 'srx_gemm_route_of',
    'srx_feature_mosaic_u8', 'srx_summary_panel_bytes', 'srx_summary_panel_range_bytes', 'srx_summary_panel_u8', 'srx_summary_panel_range',
    'srx_vdsr_patch_table_check', 'srx_vdsr_patch_pairs',
    'srx_espcn_patch_table_check', 'srx_espcn_patch_pairs',
    'srx_espcn_eval_table_check', 'srx_espcn_eval_tiles', 'srx_espcn_eval_pairs',
    'srx_vdsr_eval_table_check', 'srx_vdsr_eval_tiles', 'srx_vdsr_eval_footprint', 'srx_vdsr_eval_pairs',
    'srx_enet_pairs_table_words', 'srx_enet_pairs_tables', 'srx_enet_patch_table_check', 'srx_enet_patch_pairs',
    'srx_enet_eval_coeff_words', 'srx_enet_eval_coeffs', 'srx_enet_eval_table_check', 'srx_enet_eval_tiles', 'srx_enet_eval_footprint',
    'srx_enet_eval_pairs',
    'srx_image_scores_scratch_bytes', 'srx_image_scores_plan', 'srx_image_scores_lds_bytes', 'srx_image_scores',
    'srx_dihedral_expand', 'srx_dihedral_merge',
    'srx_srcnn_pairs_band', 'srx_srcnn_pairs_lds_bytes', 'srx_srcnn_patch_table_check', 'srx_srcnn_patch_pairs',
    'srx_srcnn_eval_table_check', 'srx_srcnn_eval_tiles', 'srx_srcnn_eval_footprint', 'srx_srcnn_eval_pairs',
    'srx_espcn_forward_u8', 'srx_u8_lut_float', 'srx_unit_u8',
    'srx_yuv420_coeffs', 'srx_yuv420_lut_float', 'srx_unit_yuv420',
    'srx_yuv_frame_bytes', 'srx_yuv_coeffs', 'srx_yuv_lut_float', 'srx_unit_yuv',
]


class SrxError(RuntimeError):
    pass


class ConvDesc(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in
                ('N', 'H', 'W', 'Cin', 'Cout', 'KH', 'KW', 'stride', 'pad_mode', 'act',
                 'post_add_relu', 'precision', 'subpixel_r')]


class PatchSrc(ctypes.Structure):
    """srx_patch_src (include/srx.h): one patch of a srx_vdsr_patch_pairs table, 32 bytes."""
    _fields_ = [('offset', ctypes.c_uint64), ('width', ctypes.c_int32), ('height', ctypes.c_int32), ('x', ctypes.c_int32),
                ('y', ctypes.c_int32), ('flip', ctypes.c_int32), ('scaling_factor', ctypes.c_float)]


class EvalImage(ctypes.Structure):
    """srx_eval_image (include/srx.h): one image of a srx_espcn_eval_pairs table, 32 bytes."""
    _fields_ = [('offset', ctypes.c_uint64), ('width', ctypes.c_int32), ('height', ctypes.c_int32), ('lr_offset', ctypes.c_uint64),
                ('first_tile', ctypes.c_uint32), ('reserved', ctypes.c_uint32)]


ESPCN_EVAL_TILE = 16            # SRX_ESPCN_EVAL_TILE


class VdsrEvalImage(ctypes.Structure):
    """srx_vdsr_eval_image (include/srx.h): one (image, scaling factor) record of a srx_vdsr_eval_pairs table, 32 bytes."""
    _fields_ = [('offset', ctypes.c_uint64), ('width', ctypes.c_int32), ('height', ctypes.c_int32), ('out_offset', ctypes.c_uint64),
                ('first_tile', ctypes.c_uint32), ('scaling_factor', ctypes.c_float)]


VDSR_EVAL_TILE = 32             # SRX_VDSR_EVAL_TILE


class EnetEvalImage(ctypes.Structure):
    """srx_enet_eval_image (include/srx.h): one trimmed image of a srx_enet_eval_pairs table, 48 bytes."""
    _fields_ = [('offset', ctypes.c_uint64), ('width', ctypes.c_int32), ('height', ctypes.c_int32), ('out_offset', ctypes.c_uint64),
                ('sd_offset', ctypes.c_uint64), ('first_tile', ctypes.c_uint32), ('width_coeffs', ctypes.c_uint32),
                ('height_coeffs', ctypes.c_uint32), ('reserved', ctypes.c_uint32)]


ENET_EVAL_TILE = 32             # SRX_ENET_EVAL_TILE


class SrcnnEvalImage(ctypes.Structure):
    """srx_srcnn_eval_image (include/srx.h): one image of a srx_srcnn_eval_pairs table, 40 bytes."""
    _fields_ = [('offset', ctypes.c_uint64), ('width', ctypes.c_int32), ('height', ctypes.c_int32), ('out_offset', ctypes.c_uint64),
                ('crop_offset', ctypes.c_uint64), ('first_tile', ctypes.c_uint32), ('reserved', ctypes.c_uint32)]


SRCNN_EVAL_TILE = 32            # SRX_SRCNN_EVAL_TILE


class PanelSrc(ctypes.Structure):
    """srx_panel_src (include/srx.h): one source of a summary panel, a view of W pixels per row; pitches in floats."""
    _fields_ = [('x', ctypes.c_void_p), ('W', ctypes.c_int32), ('reserved', ctypes.c_int32), ('row_pitch', ctypes.c_int64),
                ('image_pitch', ctypes.c_int64)]


class ScoresDesc(ctypes.Structure):
    """srx_scores_desc (include/srx.h): what one srx_image_scores call scores."""
    _fields_ = [(n, ctypes.c_int32) for n in ('N', 'H', 'W', 'C', 'n_cand', 'space', 'unit_clip')] + [('max_val', ctypes.c_float)]


SCORES_MAX_CAND = 4             # SRX_SCORES_MAX_CAND
SCORES_RGB, SCORES_Y = 0, 1     # SRX_SCORES_RGB, SRX_SCORES_Y
SCORES_MAX_TAP_STRIDE = 46      # SRX_SCORES_MAX_TAP_STRIDE
SCORES_SPACE_BY_NAME = {'rgb': SCORES_RGB, 'y': SCORES_Y}
DIHEDRAL_MAX_C = 8              # SRX_DIHEDRAL_MAX_C


YUV_BT601, YUV_BT709 = 0, 1     # SRX_YUV_BT601, SRX_YUV_BT709
YUV_MATRIX_BY_NAME = {'bt601': YUV_BT601, 'bt709': YUV_BT709}


def yuv420_frame_bytes(height, width):
    """Bytes of one planar 4:2:0 frame (the Y4M frame payload): Y [H,W], then U and V [(H + 1) // 2, (W + 1) // 2] each; odd
    sizes are legal."""
    return height * width + 2 * ((height + 1) // 2) * ((width + 1) // 2)


class Yuv420Coeffs(ctypes.Structure):
    """srx_yuv420_coeffs_t (include/srx.h): the integers of one matrix and range, filled by srx_yuv420_coeffs, 64 bytes."""
    _fields_ = [(n, ctypes.c_int32) for n in
                ('yoff', 'cy', 'crv', 'cgu', 'cgv', 'cbu', 'kry', 'kgy', 'kby', 'kru', 'kgu', 'kbu', 'krv', 'kgv', 'kbv', 'reserved')]


class YuvFormat(ctypes.Structure):
    """srx_yuv_format_t (include/srx.h): depth 8 / 10 / 12 and the chroma subsampling shifts, 16 bytes."""
    _fields_ = [(n, ctypes.c_int32) for n in ('depth', 'sub_x', 'sub_y', 'reserved')]


# name -> (depth, sub_x, sub_y): planar, little-endian 16-bit containers above 8 bits (the names FFmpeg gives them)
PIXEL_FORMATS = {'yuv%sp%s' % (sampling, suffix): (depth, sub_x, sub_y)
                 for sampling, sub_x, sub_y in (('420', 1, 1), ('422', 1, 0), ('444', 0, 0))
                 for suffix, depth in (('', 8), ('10le', 10), ('12le', 12))}


def yuv_format(pixel_format):
    """The YuvFormat of a name of PIXEL_FORMATS; any other name is refused by a ValueError that lists them."""
    if pixel_format not in PIXEL_FORMATS:
        raise ValueError('pixel_format must be one of %s, got %r' % (', '.join(sorted(PIXEL_FORMATS)), pixel_format))
    return YuvFormat(*PIXEL_FORMATS[pixel_format])


def yuv_frame_bytes(height, width, pixel_format):
    """Bytes of one planar frame of `pixel_format` (a name of PIXEL_FORMATS), from the library's srx_yuv_frame_bytes: the one
    place that computes them.  No GPU call."""
    f = yuv_format(pixel_format)
    n = lib().srx_yuv_frame_bytes(ctypes.byref(f), int(height), int(width))
    if n == 0:
        raise ValueError('%s frames of %d x %d: %s' % (pixel_format, height, width, lib().srx_last_error().decode()))
    return n


class GemmDesc(ctypes.Structure):
    _fields_ = ([(n, ctypes.c_int32) for n in ('M', 'N', 'K', 'batch')] +
                [(n, ctypes.c_int64) for n in ('a_row_stride', 'a_col_stride', 'a_batch_stride', 'b_row_stride',
                                               'b_col_stride', 'b_batch_stride', 'c_row_stride', 'c_col_stride',
                                               'c_batch_stride')] +
                [('alpha', ctypes.c_float), ('act', ctypes.c_int32), ('accumulate', ctypes.c_int32)])


_lib = None


def lib():
    """Load libsrx.so once; raise loudly if it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise SrxError('libsrx.so not found at %s -- build it with `make -C %s` (or '
                       '__graft_entry__.build()); there is no CPU fallback' %
                       (LIB_PATH, os.path.join(_HERE, 'csrc')))
    # One HIP runtime per process: PyTorch-ROCm ships its own libamdhip64.so, and the tensors handed to the library
    # live in that runtime.  Loading libsrx.so first would bind it to the system copy instead, and its launches then
    # fail with "no ROCm-capable device is detected" -- so torch's libraries are loaded before ours.
    import torch  # noqa: F401
    L = ctypes.CDLL(LIB_PATH)
    vp, sz, i, f = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_float
    dp = ctypes.POINTER(ConvDesc)
    L.srx_version.restype = ctypes.c_char_p
    L.srx_last_error.restype = ctypes.c_char_p
    L.srx_set_conv_path.argtypes = [i]
    L.srx_set_wgrad_path.argtypes = [i]
    L.srx_set_chain.argtypes = [i]
    L.srx_set_chain_fixed.argtypes = [i]
    L.srx_conv_chain_supported.argtypes = [dp, i, i]
    L.srx_conv_chain.argtypes = [dp, i, i, i, vp, vp, vp, vp, vp, vp]
    L.srx_conv2d_precision_supported.argtypes = [dp, i]
    L.srx_conv2d_workspace_bytes.argtypes = [dp, i]
    L.srx_conv2d_workspace_bytes.restype = sz
    L.srx_reduce_scratch_bytes.restype = sz
    L.srx_conv2d_fwd.argtypes = [dp, vp, vp, vp, vp, vp, vp, sz, vp]
    L.srx_conv2d_bwd_data.argtypes = [dp, vp, vp, vp, i, vp, vp, sz, vp]
    L.srx_conv2d_bwd_filter.argtypes = [dp, vp, vp, vp, vp, vp, f, vp, sz, vp]
    L.srx_conv2d_bwd_filter_partials.argtypes = [dp, vp, vp, vp, sz, ctypes.POINTER(ctypes.c_int), vp]
    L.srx_conv2d_bwd_filter_reduce.argtypes = [dp, vp, i, vp, vp, vp, f, vp]
    L.srx_conv2d_bwd_filter_batch.argtypes = [dp, i, vp, vp, vp, vp, vp, f, vp, sz, vp]
    L.srx_conv2d_bwd_filter_batch_workspace_bytes.argtypes = [dp, i]
    L.srx_conv2d_bwd_filter_batch_workspace_bytes.restype = sz
    L.srx_conv2d_bwd_filter_batch_plan.argtypes = [dp, i, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]
    L.srx_set_wgrad_batch.argtypes = [i]
    L.srx_act_bwd.argtypes = [vp, vp, vp, sz, i, vp]
    L.srx_depth_to_space.argtypes = [vp, vp, i, i, i, i, i, vp]
    L.srx_space_to_depth.argtypes = [vp, vp, i, i, i, i, i, vp]
    L.srx_stream_copy.argtypes = [vp, vp, sz, vp]
    L.srx_mse_fwd_bwd.argtypes = [vp, vp, sz, f, vp, i, vp, vp, vp]
    L.srx_l2_loss.argtypes = [vp, vp, sz, f, vp, i, vp, vp]
    L.srx_adam_tf_step.argtypes = [vp, vp, vp, vp, sz, f, f, f, f, ctypes.c_int64, f, vp]
    L.srx_adam_tf_step_dev.argtypes = [vp, vp, vp, vp, sz, vp, f, f, f, f, vp]
    L.srx_momentum_clip_step.argtypes = [vp, vp, vp, sz, f, f, f, f, vp]
    L.srx_rownorm_loss_fwd_bwd.argtypes = [vp, vp, sz, sz, vp, vp, vp, vp]
    L.srx_psnr.argtypes = [vp, vp, vp, i, sz, f, vp]
    L.srx_ssim.argtypes = [vp, vp, vp, i, i, i, i, f, vp, vp]
    L.srx_ssim_scratch_bytes.argtypes = [i]
    L.srx_ssim_scratch_bytes.restype = sz
    sp, ip = ctypes.POINTER(ScoresDesc), ctypes.POINTER(ctypes.c_int)
    L.srx_image_scores_scratch_bytes.argtypes = [sp]
    L.srx_image_scores_scratch_bytes.restype = sz
    L.srx_image_scores_plan.argtypes = [sp, ip, ip, ip, ip]
    L.srx_image_scores_lds_bytes.argtypes = [sp]
    L.srx_image_scores_lds_bytes.restype = sz
    L.srx_image_scores.argtypes = [sp, vp, vp, vp, vp, vp]
    L.srx_dihedral_expand.argtypes = [vp, vp, vp, i, i, i, i, vp]
    L.srx_dihedral_merge.argtypes = [vp, vp, vp, i, i, i, i, vp]
    L.srx_saturate_u8.argtypes = [vp, vp, sz, vp]
    L.srx_feature_mosaic_u8.argtypes = [vp, vp, i, i, i, vp]
    L.srx_summary_panel_bytes.argtypes = [vp, i, i, i, i]
    L.srx_summary_panel_bytes.restype = sz
    L.srx_summary_panel_range_bytes.restype = sz
    L.srx_summary_panel_u8.argtypes = [vp, i, i, i, i, vp, vp, vp]
    L.srx_summary_panel_range.argtypes = [vp, i, i, i, i, vp, vp]
    L.srx_vdsr_patch_table_check.argtypes = [vp, i, i, sz]
    L.srx_vdsr_patch_pairs.argtypes = [vp, vp, i, i, vp, vp, vp]
    L.srx_espcn_patch_table_check.argtypes = [vp, i, i, i, sz]
    L.srx_espcn_patch_pairs.argtypes = [vp, vp, i, i, i, vp, vp, vp]
    L.srx_espcn_eval_table_check.argtypes = [vp, i, i, sz, sz]
    L.srx_espcn_eval_tiles.argtypes = [vp, i, i]
    L.srx_espcn_eval_tiles.restype = sz
    L.srx_espcn_eval_pairs.argtypes = [vp, vp, i, i, vp, vp, vp]
    L.srx_vdsr_eval_table_check.argtypes = [vp, i, sz, sz]
    L.srx_vdsr_eval_tiles.argtypes = [vp, i]
    L.srx_vdsr_eval_tiles.restype = sz
    L.srx_vdsr_eval_footprint.argtypes = [i, ctypes.c_float, i, vp]
    L.srx_vdsr_eval_pairs.argtypes = [vp, vp, i, vp, vp, vp]
    L.srx_enet_pairs_table_words.argtypes = [i]
    L.srx_enet_pairs_tables.argtypes = [i, vp]
    L.srx_enet_patch_table_check.argtypes = [vp, i, i, sz]
    L.srx_enet_patch_pairs.argtypes = [vp, vp, i, i, vp, vp, vp, vp, vp]
    L.srx_enet_eval_coeff_words.argtypes = [i]
    L.srx_enet_eval_coeffs.argtypes = [i, vp]
    L.srx_enet_eval_table_check.argtypes = [vp, i, sz, sz, sz, vp, sz]
    L.srx_enet_eval_tiles.argtypes = [vp, i]
    L.srx_enet_eval_tiles.restype = sz
    L.srx_enet_eval_footprint.argtypes = [i, i, vp]
    L.srx_enet_eval_pairs.argtypes = [vp, vp, i, vp, vp, vp, vp, vp]
    L.srx_srcnn_pairs_band.argtypes = [i, i]
    L.srx_srcnn_pairs_lds_bytes.argtypes = [i, i]
    L.srx_srcnn_patch_table_check.argtypes = [vp, i, i, i, i, sz]
    L.srx_srcnn_patch_pairs.argtypes = [vp, vp, i, i, i, i, vp, vp, vp]
    L.srx_srcnn_eval_table_check.argtypes = [vp, i, i, i, sz, sz, sz]
    L.srx_srcnn_eval_tiles.argtypes = [vp, i]
    L.srx_srcnn_eval_tiles.restype = sz
    L.srx_srcnn_eval_footprint.argtypes = [i, i, i, vp]
    L.srx_srcnn_eval_pairs.argtypes = [vp, vp, i, i, i, vp, vp, vp, vp]
    L.srx_affine.argtypes = [vp, vp, sz, f, f, vp]
    L.srx_u8_to_unit_float.argtypes = [vp, vp, sz, vp]
    L.srx_gaussian_blur.argtypes = [vp, vp, vp, i, i, i, i, f, vp]
    L.srx_resize_bilinear.argtypes = [vp, vp, i, i, i, i, i, i, vp]
    L.srx_upsample_nearest.argtypes = [vp, vp, i, i, i, i, i, vp]
    L.srx_upsample_nearest_bwd.argtypes = [vp, vp, i, i, i, i, i, vp]
    L.srx_add_relu_grad.argtypes = [vp, vp, vp, vp, sz, vp]
    L.srx_conv2d_bwd_data_acc.argtypes = [dp, vp, vp, vp, vp, vp, sz, vp]
    L.srx_espcn_forward.argtypes = [vp] * 8 + [i, i, i, i, vp]
    L.srx_espcn_forward_keep.argtypes = [vp] * 10 + [i, i, i, i, vp]
    L.srx_espcn_forward_u8.argtypes = [vp] * 9 + [i, i, i, i, vp]
    L.srx_u8_lut_float.argtypes = [vp, vp, vp, sz, vp]
    L.srx_unit_u8.argtypes = [vp, vp, sz, vp]
    yp = ctypes.POINTER(Yuv420Coeffs)
    L.srx_yuv420_coeffs.argtypes = [i, i, yp]
    L.srx_yuv420_lut_float.argtypes = [vp, i, i, i, yp, vp, vp, vp]
    L.srx_unit_yuv420.argtypes = [vp, i, i, i, yp, vp, vp]
    fp = ctypes.POINTER(YuvFormat)
    L.srx_yuv_frame_bytes.argtypes = [fp, i, i]
    L.srx_yuv_frame_bytes.restype = sz
    L.srx_yuv_coeffs.argtypes = [i, i, i, yp]
    L.srx_yuv_lut_float.argtypes = [vp, i, i, i, fp, yp, vp, vp, vp]
    L.srx_unit_yuv.argtypes = [vp, i, i, i, fp, yp, vp, vp]
    L.srx_debug_poison_lds.argtypes = [vp]
    L.srx_srcnn_forward.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, i, i, i, vp]
    L.srx_conv3x3_blocked.argtypes = [vp, vp, vp, vp, i, vp, i, i, i, i, i, i, i, vp]
    L.srx_conv3x3_blocked_bwd_filter_workspace_bytes.restype = sz
    L.srx_conv3x3_blocked_bwd_filter_workspace_bytes.argtypes = [i, i, i, i, i]
    L.srx_conv3x3_blocked_bwd_filter.argtypes = [vp, vp, vp, vp, i, i, i, i, i, vp, sz, vp]
    L.srx_conv3x3_blocked_ex.argtypes = [vp, vp, vp, vp, i, vp, i, i, i, i, i, i, i, i, vp]
    L.srx_conv3x3_blocked_bwd_filter_ex_workspace_bytes.restype = sz
    L.srx_conv3x3_blocked_bwd_filter_ex_workspace_bytes.argtypes = [i, i, i, i, i, i]
    L.srx_conv3x3_blocked_bwd_filter_ex.argtypes = [vp, vp, vp, vp, i, i, i, i, i, i, vp, sz, vp]
    L.srx_texture_gram.argtypes = [vp, vp, i, i, i, i, f, vp]
    L.srx_texture_gram_bwd.argtypes = [vp, vp, vp, i, i, i, i, f, f, vp]
    L.srx_pil_resample_ksize.argtypes = [i, i, i]
    L.srx_pil_resample_coeffs.argtypes = [i, i, i, vp, vp]
    L.srx_resample_u8.argtypes = [vp, vp, ctypes.c_long, i, i, ctypes.c_long, vp, vp, i, vp]
    L.srx_u8_to_pm1.argtypes = [vp, vp, sz, vp]
    L.srx_maxpool2x2.argtypes = [vp, vp, i, i, i, i, vp]
    L.srx_maxpool2x2_bwd.argtypes = [vp, vp, vp, i, i, i, i, vp]
    L.srx_maxpool2x2_bwd_masked.argtypes = [vp, vp, vp, i, i, i, i, i, vp]
    L.srx_subsample2.argtypes = [vp, vp, i, i, i, i, i, i, vp]
    L.srx_subsample2_bwd.argtypes = [vp, vp, i, i, i, i, i, i, vp]
    L.srx_channel_blocks_to_nhwc.argtypes = [vp, vp, sz, i, vp]
    L.srx_nhwc_to_channel_blocks.argtypes = [vp, vp, sz, i, vp]
    L.srx_channel_normalize.argtypes = [vp, vp, sz, i, f, vp]
    L.srx_channel_normalize_bwd.argtypes = [vp, vp, vp, sz, i, f, vp]
    L.srx_extract_patches16.argtypes = [vp, vp, i, i, i, i, i, vp]
    L.srx_log_loss.argtypes = [vp, f, i, f, f, f, vp, i, vp, vp]
    L.srx_vgg_preprocess.argtypes = [vp, vp, sz, i, vp]
    L.srx_column_sums.argtypes = [vp, vp, i, i, i, vp]
    L.srx_add_scaled.argtypes = [vp, vp, vp, sz, f, f, vp]
    L.srx_resize_bicubic_tf.argtypes = [vp, vp, i, i, i, i, i, i, vp]
    L.srx_gemm_workspace_bytes.argtypes = [i, i, i, i]
    L.srx_gemm_workspace_bytes.restype = sz
    L.srx_gemm.argtypes = [ctypes.POINTER(GemmDesc), vp, vp, vp, vp, vp, sz, vp]
    L.srx_gemm_route_of.argtypes = [ctypes.POINTER(GemmDesc), vp, vp, vp, vp, sz, ctypes.POINTER(ctypes.c_int)]
    for name in EXPORTS:
        getattr(L, name)          # AttributeError if the library is stale
    _lib = L
    return L


def check(rc, what):
    if rc != SRX_OK:
        raise SrxError('%s failed (status %d): %s' % (what, rc, lib().srx_last_error().decode()))
