"""ctypes binding of libfemasr_hip.so (C ABI declared in include/femasr_hip.h).

There is NO fallback: if the shared library is missing or a call fails, this
module raises — the product path never silently degrades to a CPU / eager path.
Build the library with `python femasr_amd/csrc/build.py` (hipcc, gfx950).
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
SO_PATH = os.path.join(_HERE, 'csrc', 'libfemasr_hip.so')

c_int, c_i64, c_f32 = ctypes.c_int, ctypes.c_int64, ctypes.c_float
vp, szt = ctypes.c_void_p, ctypes.c_size_t


class FemasrError(RuntimeError):
    pass


MAX_CODEBOOKS = 3


class Config(ctypes.Structure):
    _fields_ = ([(n, ctypes.c_int32) for n in ('in_channel', 'gt_resolution', 'lq_stage', 'scale_factor', 'use_quantize',
                                               'use_residual', 'n_codebooks')] +
                [(n, ctypes.c_int32 * MAX_CODEBOOKS) for n in ('codebook_scale', 'n_e', 'e_dim')] +
                [('device', ctypes.c_int32)])


class ConvArgs(ctypes.Structure):
    _fields_ = [
        ('in_', vp), ('B', ctypes.c_int32), ('H', ctypes.c_int32), ('W', ctypes.c_int32), ('Cin', ctypes.c_int32),
        ('w', vp), ('bias', vp),
        ('Cout', ctypes.c_int32), ('ksz', ctypes.c_int32), ('stride', ctypes.c_int32), ('pad', ctypes.c_int32),
        ('up2', ctypes.c_int32), ('prologue', ctypes.c_int32),
        ('pro_a', vp), ('pro_b', vp), ('pro_c', vp),
        ('act', ctypes.c_int32),
        ('res1', vp), ('res2', vp), ('out', vp),
        ('Ho', ctypes.c_int32), ('Wo', ctypes.c_int32),
        ('w_bf16x3', vp), ('gn_part', vp), ('w_up2', vp), ('w_wino', vp), ('fast_act', ctypes.c_int32), ('in_add', vp), ('w_bf16s', vp),
        ('w_f16', vp),
    ]


ABI_VERSION = 107      # femasr_version(): (additive, number kept: femasr_resample_u8 / femasr_resample_tile; femasr_encode / femasr_encode_workspace_bytes, femasr_index_histogram / _workspace_bytes; femasr_channels_split_u8 / _merge_u8, femasr_png_filter_u8; femasr_png_filter_rgb8; femasr_dihedral_expand / _merge and their _u8 forms; femasr_repack_k1_f16, the ksz = 1 meaning of w_f16, linear_math 2) femasr_conv_args ends with w_f16, femasr_repack_oihw_f16, decoder_math 4; 106: femasr_blend_tiles / femasr_blend_tiles_u8; 105: femasr_niqe_*, femasr_imresize*; 104: the femasr_psnr_ssim* entry points; 103: FEMASR_ACT_RELU, femasr_lpips_* 
PRO_NONE, PRO_GN_SILU, PRO_LN = 0, 1, 2
ACT_NONE, ACT_GELU, ACT_RELU = 0, 1, 2

# name -> (restype, argtypes); every symbol include/femasr_hip.h declares
SIGNATURES = {
    'femasr_last_error': (ctypes.c_char_p, []),
    'femasr_version': (c_int, []),
    'femasr_create': (c_int, [ctypes.POINTER(Config), ctypes.POINTER(vp)]),
    'femasr_destroy': (None, [vp]),
    'femasr_num_weights': (c_int, [vp]),
    'femasr_weight_info': (c_int, [vp, c_int, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(c_i64 * 4), ctypes.POINTER(c_int)]),
    'femasr_set_weight': (c_int, [vp, ctypes.c_char_p, vp, ctypes.POINTER(c_i64), c_int]),
    'femasr_finalize_weights': (c_int, [vp]),
    'femasr_set_streams': (c_int, [vp, c_int]),
    'femasr_workspace_bytes': (c_int, [vp, c_int, c_int, c_int, c_int, ctypes.POINTER(szt)]),
    'femasr_forward_shapes': (c_int, [vp, c_int, c_int, c_int, ctypes.POINTER(c_int), ctypes.POINTER(c_int), ctypes.POINTER(c_int),
                                      ctypes.POINTER(c_int * MAX_CODEBOOKS), ctypes.POINTER(c_int * MAX_CODEBOOKS)]),
    'femasr_forward': (c_int, [vp, vp, vp, c_int, c_int, c_int, c_int, vp, vp, vp, szt]),
    'femasr_forward_u8': (c_int, [vp, vp, vp, c_int, c_int, c_int, c_int, c_int, vp, vp, vp, szt]),
    'femasr_pad_u8hwc_to_nhwc': (c_int, [vp, vp, c_int, c_int, c_int, c_int, c_int, c_int, vp]),
    'femasr_crop_nhwc_to_u8hwc': (c_int, [vp, vp, c_int, c_int, c_int, c_int, c_int, c_int, vp]),
    'femasr_decode_workspace_bytes': (c_int, [vp, c_int, c_int, c_int, ctypes.POINTER(szt)]),
    'femasr_decode_indices': (c_int, [vp, vp, vp, c_int, c_int, c_int, vp, vp, szt]),
    'femasr_profile_enable': (c_int, [vp, c_int]),
    'femasr_profile_reset': (c_int, [vp]),
    'femasr_profile_slots': (c_int, [vp]),
    'femasr_profile_name': (ctypes.c_char_p, [vp, c_int]),
    'femasr_profile_get': (c_int, [vp, c_int, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(c_i64),
                                   ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double)]),
    'femasr_pad_nchw_to_nhwc': (c_int, [vp, vp, c_int, c_int, c_int, c_int, c_int, c_int, vp]),
    'femasr_crop_nhwc_to_nchw': (c_int, [vp, vp, c_int, c_int, c_int, c_int, c_int, c_int, vp]),
    'femasr_conv2d': (c_int, [vp, ctypes.POINTER(ConvArgs)]),
    'femasr_gn_coeffs': (c_int, [vp, vp, c_int, c_int, c_int, c_int, c_int, vp, vp, c_f32, vp, vp, vp]),
    'femasr_gn_coeffs_from_partials': (c_int, [vp, vp, c_int, c_int, c_int, c_int, c_int, c_int, vp, vp, c_f32, vp, vp]),
    'femasr_ln_stats': (c_int, [vp, vp, c_i64, c_int, c_f32, vp]),
    'femasr_layernorm': (c_int, [vp, vp, c_i64, c_int, vp, vp, c_f32, vp]),
    'femasr_gn_scratch_bytes': (szt, [c_int, c_int, c_int, c_int, c_int]),
    'femasr_window_attention': (c_int, [vp, vp, c_int, c_int, c_int, c_int, c_int, c_int, vp, vp]),
    'femasr_vq': (c_int, [vp, vp, c_i64, c_int, vp, vp, vp, c_int, vp, vp, vp]),
    'femasr_row_sqsum': (c_int, [vp, vp, c_i64, c_int, vp]),
    'femasr_vq_twopass_ok': (c_int, [c_int, c_int]),
    'femasr_vq_aux_bytes': (szt, [c_int, c_int]),
    'femasr_vq_prepare': (c_int, [vp, vp, vp, c_int, c_int, vp]),
    'femasr_vq_scratch_bytes': (szt, [c_i64, c_int]),
    'femasr_vq_twopass': (c_int, [vp, vp, c_i64, c_int, vp, vp, vp, c_int, vp, vp, vp]),
    'femasr_vq_candidates': (c_int, [vp, vp, c_i64, c_int, vp, vp, c_int, vp, vp]),
    'femasr_codebook_gather': (c_int, [vp, vp, c_i64, c_int, vp, c_int, vp]),
    'femasr_extract_tiles': (c_int, [vp, vp, c_int, c_int, c_int, c_int, vp, c_int, c_int, c_int, vp]),
    'femasr_paste_tiles': (c_int, [vp, vp, c_int, c_int, c_int, c_int, c_int, vp, c_int, c_int, c_int, vp]),
    'femasr_extract_tiles_u8': (c_int, [vp, vp, c_int, c_int, c_int, vp, c_int, c_int, c_int, vp]),
    'femasr_paste_tiles_u8': (c_int, [vp, vp, c_int, c_int, c_int, c_int, vp, c_int, c_int, c_int, vp]),
    'femasr_blend_tiles': (c_int, [vp, vp, vp, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, vp]),
    'femasr_blend_tiles_u8': (c_int, [vp, vp, vp, c_int, c_int, c_int, c_int, c_int, c_int, c_int, vp]),
    'femasr_concat_resize': (c_int, [vp, vp, c_int, vp, c_int, c_int, c_int, c_int, c_int, c_int, vp]),
    'femasr_repack_oihw': (c_int, [vp, vp, c_int, c_int, c_int, c_int, vp]),
    'femasr_packed_weight_floats': (szt, [c_int, c_int, c_int, c_int]),
    'femasr_up2_weight_floats': (szt, [c_int, c_int]),
    'femasr_wino_weight_floats': (szt, [c_int, c_int]),
    'femasr_repack_oihw_wino': (c_int, [vp, vp, c_int, c_int, vp]),
    'femasr_wino_up2_weight_floats': (szt, [c_int, c_int]),
    'femasr_repack_oihw_wino_up2': (c_int, [vp, vp, c_int, c_int, vp]),
    'femasr_repack_oihw_up2': (c_int, [vp, vp, c_int, c_int, vp]),
    'femasr_packed_weight_bf16x3_bytes': (szt, [c_int, c_int, c_int, c_int]),
    'femasr_repack_oihw_bf16x3': (c_int, [vp, vp, c_int, c_int, c_int, c_int, vp]),
    'femasr_packed_weight_f16_bytes': (szt, [c_int, c_int, c_int, c_int]),
    'femasr_repack_oihw_f16': (c_int, [vp, vp, c_int, c_int, c_int, c_int, vp]),
    'femasr_packed_weight_k1_f16_bytes': (szt, [c_int, c_int]),
    'femasr_repack_k1_f16': (c_int, [vp, vp, c_int, c_int, vp]),
    'femasr_set_decoder_math': (c_int, [vp, c_int]),
    'femasr_set_linear_math': (c_int, [vp, c_int]),
    'femasr_packed_weight_bf16s_bytes': (szt, [c_int, c_int]),
    'femasr_repack_k1_bf16s': (c_int, [vp, vp, c_int, c_int, vp]),
    'femasr_packed_weight_conv3x3_bf16s_bytes': (szt, [c_int, c_int]),
    'femasr_repack_oihw_bf16s': (c_int, [vp, vp, c_int, c_int, vp]),
    'femasr_gn_silu_apply': (c_int, [vp, vp, c_int, c_int, c_int, c_int, vp, vp, vp]),
    'femasr_image_u8_to_f32': (c_int, [vp, vp, c_int, c_int, c_int, vp]),
    'femasr_image_f32_to_u8': (c_int, [vp, vp, c_int, c_int, c_int, vp]),
    'femasr_lpips_create': (c_int, [c_int, c_int, ctypes.POINTER(vp)]),
    'femasr_lpips_destroy': (None, [vp]),
    'femasr_lpips_set_weight': (c_int, [vp, ctypes.c_char_p, vp, ctypes.POINTER(c_i64), c_int]),
    'femasr_lpips_finalize_weights': (c_int, [vp]),
    'femasr_lpips_workspace_bytes': (c_int, [vp, c_int, c_int, c_int, ctypes.POINTER(szt)]),
    'femasr_lpips_forward': (c_int, [vp, vp, vp, vp, c_int, c_int, c_int, vp, vp, vp, szt]),
    'femasr_lpips_scale_input': (c_int, [vp, vp, vp, c_int, c_int, c_int, vp]),
    'femasr_lpips_tap_partials': (c_int, [c_int, c_int]),
    'femasr_lpips_tap': (c_int, [vp, vp, c_int, c_int, c_int, c_int, vp, c_int, vp, vp]),
    'femasr_lpips_finalize': (c_int, [vp, vp, c_int, c_int, ctypes.POINTER(ctypes.c_int32), vp, vp]),
    'femasr_psnr_ssim_workspace_bytes': (c_int, [c_int, c_int, c_int, c_int, c_int, ctypes.POINTER(szt)]),
    'femasr_psnr_ssim': (c_int, [vp, vp, vp, c_int, c_int, c_int, c_int, c_int, vp, vp, vp, vp, szt]),
    'femasr_ssim_window': (c_int, [ctypes.POINTER(ctypes.c_double)]),
    'femasr_imresize_workspace_bytes': (c_int, [c_int, c_int, c_int, c_int, c_int, ctypes.POINTER(szt)]),
    'femasr_imresize': (c_int, [vp, vp, c_int, c_int, c_int, c_int, c_int, c_int, vp, vp, c_int, vp, vp, c_int, vp, vp, szt]),
    'femasr_niqe_workspace_bytes': (c_int, [c_int, c_int, c_int, c_int, ctypes.POINTER(szt)]),
    'femasr_niqe_plane_offsets': (c_int, [c_int, c_int, c_int, c_int, ctypes.POINTER(szt * 4)]),
    'femasr_niqe_features': (c_int, [vp, vp, c_int, c_int, c_int, c_int, vp, vp, vp, vp, c_int, vp, vp, c_int, vp, vp, vp, szt]),
    'femasr_color_fix_workspace_bytes': (c_int, [c_int, c_int, c_int, c_int, c_int, c_int, ctypes.POINTER(szt)]),
    'femasr_color_fix': (c_int, [vp, vp, vp, c_int, c_int, c_int, c_int, c_int, c_int, c_int, vp, vp, c_int, vp, vp, c_int, vp, vp, szt]),
    'femasr_color_fix_u8': (c_int, [vp, vp, vp, c_int, c_int, c_int, c_int, c_int, c_int, c_int, vp, vp, c_int, vp, vp, c_int, vp, vp, szt]),
    'femasr_dihedral_expand': (c_int, [vp, vp, c_int, c_int, c_int, c_int, vp, vp]),
    'femasr_dihedral_expand_u8': (c_int, [vp, vp, c_int, c_int, c_int, vp, vp]),
    'femasr_dihedral_merge': (c_int, [vp, vp, vp, c_int, c_int, c_int, c_int, vp]),
    'femasr_dihedral_merge_u8': (c_int, [vp, vp, vp, c_int, c_int, c_int, vp]),
    'femasr_png_filter_rgb8': (c_int, [vp, vp, c_int, c_int, c_int, c_int, vp]),
    'femasr_png_filter_u8': (c_int, [vp, vp, c_int, c_int, c_int, c_int, c_int, vp]),
    'femasr_channels_split_u8': (c_int, [vp, vp, c_int, c_int, c_int, c_int, vp, vp]),
    'femasr_channels_merge_u8': (c_int, [vp, vp, vp, vp, c_int, c_int, c_int, c_int, vp, vp, c_int, vp, vp, c_int, vp]),
    'femasr_clock_probe': (c_int, [vp, c_int, vp]),
    'femasr_clock_probe_entries': (c_int, []),
}
# the network as an encoder and the code-usage histogram: include/femasr_hip_encode.h (included by femasr_hip.h; part of the interface)
ENCODE_SIGNATURES = {
    'femasr_encode_workspace_bytes': (c_int, [vp, c_int, c_int, c_int, c_int, ctypes.POINTER(szt)]),
    'femasr_encode': (c_int, [vp, vp, vp, c_int, c_int, c_int, c_int, c_int, c_int, vp, vp, szt]),
    'femasr_index_histogram_workspace_bytes': (c_int, [c_int, c_i64, c_int, ctypes.POINTER(szt)]),
    'femasr_index_histogram': (c_int, [vp, vp, c_int, c_i64, c_int, vp, vp, vp, szt]),
}
# the bicubic resample of uint8 images to an arbitrary size: include/femasr_hip_resample.h (included by femasr_hip.h; part of the interface)
RESAMPLE_SIGNATURES = {
    'femasr_resample_u8': (c_int, [vp, vp, c_int, c_int, c_int, vp, c_int, c_int, vp, vp, c_int, vp, vp, c_int]),
    'femasr_resample_tile': (c_int, []),
}
# the fast JPEG output - coefficients on the GPU, Huffman coding on the host: include/femasr_hip_jpeg.h (included by femasr_hip.h; part of the interface)
JPEG_SIGNATURES = {
    'femasr_jpeg_coefficients_u8': (c_int, [vp, c_int, c_int, c_int, c_int, vp, vp, vp, vp, vp, vp]),
    'femasr_jpeg_entropy_rows': (ctypes.c_longlong, [vp, vp, vp, c_int, c_int, c_int, c_int, c_int, c_int, vp, szt]),
    'femasr_jpeg_entropy_bound': (szt, [c_int, c_int, c_int, c_int]),
}
# synthesis of low-quality inputs - blur, resample, noise, quantisation, JPEG decode: include/femasr_hip_degrade.h (included by femasr_hip.h; part of the interface)
c_u64 = ctypes.c_uint64
DEGRADE_SIGNATURES = {
    'femasr_degrade_blur_f32': (c_int, [vp, vp, c_int, c_int, vp, c_int, c_int, vp]),
    'femasr_degrade_resize_f32': (c_int, [vp, vp, c_int, c_int, vp, c_int, c_int, vp, vp, c_int, vp, vp, c_int, vp, vp]),
    'femasr_degrade_noise_f32': (c_int, [vp, vp, vp, ctypes.c_longlong, c_u64, c_int, ctypes.POINTER(ctypes.c_double), c_u64]),
    'femasr_degrade_quantize_u8': (c_int, [vp, vp, vp, ctypes.c_longlong]),
    'femasr_degrade_unit_f32': (c_int, [vp, vp, c_int, c_int, c_int, vp]),
    'femasr_jpeg_decode_u8': (c_int, [vp, vp, vp, vp, c_int, c_int, c_int, c_int, vp, vp, vp, c_int]),
}
# DISTS - handle, forward, the backbone's stage maps, the L2-pool and moments units: include/femasr_hip_dists.h (included by femasr_hip.h; part of the interface)
DISTS_SIGNATURES = {
    'femasr_dists_create': (c_int, [c_int, ctypes.POINTER(vp)]),
    'femasr_dists_destroy': (None, [vp]),
    'femasr_dists_set_weight': (c_int, [vp, ctypes.c_char_p, vp, ctypes.POINTER(c_i64), c_int]),
    'femasr_dists_finalize_weights': (c_int, [vp]),
    'femasr_dists_workspace_bytes': (c_int, [vp, c_int, c_int, c_int, ctypes.POINTER(szt)]),
    'femasr_dists_forward': (c_int, [vp, vp, vp, vp, c_int, c_int, c_int, vp, szt, vp, vp]),
    'femasr_dists_features': (c_int, [vp, vp, vp, vp, c_int, c_int, c_int, vp, szt, vp]),
    'femasr_dists_l2pool': (c_int, [vp, vp, c_int, c_int, c_int, c_int, vp]),
    'femasr_dists_moments_workspace_bytes': (c_int, [c_int, c_int, c_int, c_int, ctypes.POINTER(szt)]),
    'femasr_dists_moments': (c_int, [vp, vp, c_int, c_int, c_int, c_int, vp, szt, vp]),
    'femasr_dists_moments_input': (c_int, [vp, vp, vp, c_int, c_int, c_int, vp, szt, vp]),
}
# test / measurement hooks: include/femasr_hip_debug.h (exported by the library, not part of the drop-in interface)
DEBUG_SIGNATURES = {
    'femasr_debug_set_wino_limits': (c_int, [vp, c_int, c_int]),
    'femasr_debug_mfma_bf16': (c_int, [vp, vp, vp, vp, c_int, vp]),
    'femasr_gemm_force_config': (c_int, [c_int]),
    'femasr_conv_small_launch_blocks': (c_int, [c_int]),
    'femasr_debug_conv_variant_name': (c_int, [ctypes.POINTER(ConvArgs), ctypes.c_char_p, c_int]),
    'femasr_debug_weight_image_bytes': (c_int, [vp, c_int, ctypes.POINTER(szt)]),
    'femasr_debug_math_eval': (c_int, [vp, c_int, vp, ctypes.c_longlong, vp]),
}

_lib = None


def load():
    """Load the shared library and bind every declared symbol; raises if anything is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(SO_PATH):
        raise FemasrError(
            f'{SO_PATH} not found: the HIP extension is not built. Run `python femasr_amd/csrc/build.py` '
            '(needs hipcc; cross-compiles gfx950 without a GPU). There is no CPU fallback.')
    lib = ctypes.CDLL(SO_PATH)
    lib.femasr_version.restype = c_int
    if lib.femasr_version() != ABI_VERSION:
        raise FemasrError(f'{SO_PATH} reports ABI version {lib.femasr_version()}, this binding is written for {ABI_VERSION} '
                          '(femasr_conv_args layout): rebuild with `python femasr_amd/csrc/build.py --force`')
    for name, (res, args) in list(SIGNATURES.items()) + list(ENCODE_SIGNATURES.items()) + list(RESAMPLE_SIGNATURES.items()) + list(JPEG_SIGNATURES.items()) + list(DEGRADE_SIGNATURES.items()) + list(DISTS_SIGNATURES.items()) + list(DEBUG_SIGNATURES.items()):
        fn = getattr(lib, name)      # AttributeError if the symbol is not exported
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(rc):
    if rc != 0:
        msg = load().femasr_last_error()
        raise FemasrError(f'libfemasr_hip error {rc}: {msg.decode() if msg else "?"}')


def ptr(t):
    """Device pointer of a torch tensor (or None)."""
    return None if t is None else ctypes.c_void_p(t.data_ptr())
