"""ctypes loader for libvitadapter_hip.so (the C ABI in include/vitadapter_hip.h).

The library is the product: there is NO fallback.  If it has not been built
(`python vit-adapter_amd/build.py`), importing this module raises ImportError.
"""
import ctypes
import os

# torch MUST be imported before the library is loaded: the PyTorch-ROCm wheel bundles its own
# libamdhip64.so, and the kernels have to be registered with (and launched through) the same
# HIP runtime instance that owns torch's streams and allocations.  Loading our library first
# would pull in /opt/rocm's runtime as a second instance ("no ROCm-capable device" at launch).
import torch  # noqa: F401

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, 'lib', 'libvitadapter_hip.so')
ABI_VERSION = 37

if not os.path.exists(LIB_PATH):
    raise ImportError(
        'libvitadapter_hip.so is missing (%s): build it with `python vit-adapter_amd/build.py` '
        '(hipcc --offload-arch=gfx950).  There is no CPU or PyTorch fallback.' % LIB_PATH)

lib = ctypes.CDLL(LIB_PATH)

_int, _i64, _f, _p, _str, _pi64 = (ctypes.c_int, ctypes.c_int64, ctypes.c_float, ctypes.c_void_p, ctypes.c_char_p,
                                   ctypes.POINTER(ctypes.c_int64))

# name -> (restype, argtypes) of every entry point include/vitadapter_hip.h declares, in the header's order, the fp16 twins
# excepted: those take their parent's signature (F16_TWINS).  tests/test_binding_table_cpu.py holds each entry to its
# prototype: a c_int where the library reads an int64_t is a garbage dimension inside a kernel.
SIGNATURES = {
    'vah_abi_version': (_int, []),
    'vah_last_error': (_str, []),
    'vah_msda_forward_f32': (_int, [_p, _p, _p, _p, _p, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _p, _p]),
    'vah_msda_forward_f64': (_int, [_p, _p, _p, _p, _p, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _p, _p]),
    'vah_msda_backward_f32': (_int, [_p, _p, _p, _p, _p, _p, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _p, _p, _p, _p]),
    'vah_msda_backward_f64': (_int, [_p, _p, _p, _p, _p, _p, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _p, _p, _p, _p]),
    'vah_msda_fused_supported': (_int, [_i64, _i64, _i64]),
    'vah_msda_fused_forward': (_int, [_p, _int, _p, _p, _p, _p, _int, _i64, _i64, _p, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _p, _p]),
    'vah_msda_fused_backward': (_int, [_p, _int, _p, _p, _p, _p, _int, _p, _i64, _p, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _p, _p, _p, _p]),
    'vah_msda_fused_forward_nref': (_int, [_p, _int, _p, _p, _p, _p, _int, _i64, _i64, _p, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _p,
                                           _p]),
    'vah_msda_fused_backward_nref': (_int, [_p, _int, _p, _p, _p, _p, _int, _p, _i64, _i64, _p, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _p, _p, _p,
                                            _p]),
    'vah_msda_win_ws_bytes': (_i64, [_i64, _i64]),
    'vah_msda_fused_forward_win': (_int, [_p, _int, _p, _p, _p, _p, _int, _i64, _i64, _p, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _p, _i64, _int,
                                          _p, _p]),
    'vah_msda_tile_ws_bytes': (_i64, [_i64, _i64, _i64, _i64, _i64, _i64]),
    'vah_msda_backward_tiled_f32': (_int, [_p, _p, _p, _p, _p, _p, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _p, _p, _p, _p, _i64, _p]),
    'vah_msda_fused_backward_tiled': (_int, [_p, _int, _p, _p, _p, _p, _int, _i64, _i64, _p, _i64, _p, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _p,
                                             _int, _p, _p, _int, _i64, _i64, _p, _i64, _p]),
    'vah_msda_fused_backward_tiled_nref': (_int, [_p, _int, _p, _p, _p, _p, _int, _i64, _i64, _p, _i64, _i64, _p, _i64, _i64, _i64, _i64, _i64, _i64,
                                                  _i64, _p, _int, _p, _p, _int, _i64, _i64, _p, _i64, _p]),
    'vah_attn_padded_len': (_i64, [_i64]),
    'vah_attn_fwd_bf16': (_int, [_p, _p, _p, _i64, _i64, _i64, _i64, _i64, _f, _p, _p, _i64, _p, _p]),
    'vah_attn_win_fwd_bf16': (_int, [_p, _p, _p, _i64, _i64, _i64, _i64, _i64, _i64, _f, _p, _p, _i64, _p, _p]),
    'vah_attn_bwd_workspace_bytes': (_i64, [_i64, _i64, _i64]),
    'vah_attn_bwd_bf16': (_int, [_p, _p, _p, _i64, _i64, _p, _p, _i64, _p, _i64, _i64, _i64, _f, _p, _p, _p, _p, _i64, _i64, _p]),
    'vah_attn_bias_fwd_bf16': (_int, [_p, _p, _p, _i64, _i64, _i64, _i64, _i64, _f, _p, _i64, _p, _i64, _p, _p]),
    'vah_attn_bias_bwd_bf16': (_int, [_p, _p, _p, _i64, _i64, _p, _p, _i64, _p, _i64, _i64, _i64, _f, _p, _p, _i64, _p, _p, _p, _p, _p, _i64, _i64,
                                      _p]),
    'vah_relpos_bias_build': (_int, [_p, _p, _i64, _i64, _i64, _i64, _p, _p, _p]),
    'vah_relpos_bias_grad_ws_floats': (_i64, [_i64, _i64]),
    'vah_relpos_bias_grad': (_int, [_p, _p, _i64, _i64, _i64, _i64, _i64, _p, _p, _p]),
    'vah_attn_win_bwd_bf16': (_int, [_p, _p, _p, _i64, _p, _p, _i64, _p, _i64, _i64, _i64, _i64, _i64, _f, _p, _p, _p, _p, _i64, _p]),
    'vah_reduce_ws_floats': (_i64, [_i64]),
    'vah_layernorm_fwd_f32_bf16': (_int, [_p, _p, _p, _i64, _i64, _f, _p, _p, _p, _p]),
    'vah_layernorm_bwd_f32_bf16': (_int, [_p, _p, _p, _p, _p, _p, _i64, _i64, _p, _p, _p, _p, _p]),
    'vah_residual_layernorm_fwd': (_int, [_p, _p, _p, _p, _i64, _i64, _i64, _p, _p, _f, _p, _p, _p, _p, _p]),
    'vah_residual_layernorm_bwd': (_int, [_p, _p, _p, _p, _p, _p, _p, _p, _p, _i64, _i64, _i64, _p, _p, _p, _p, _p, _p, _p]),
    'vah_layernorm_dual_fwd': (_int, [_p, _p, _p, _p, _p, _i64, _i64, _f, _p, _p, _p, _p, _p]),
    'vah_layernorm_dual_bwd': (_int, [_p, _p, _p, _p, _p, _p, _p, _p, _i64, _i64, _p, _p, _p, _p]),
    'vah_colsum_bf16': (_int, [_p, _i64, _i64, _p, _p, _p]),
    'vah_colsum_bf16_partials': (_int, [_p, _i64, _i64, _p, _pi64, _p]),
    'vah_residual_layernorm_bwd_bsum': (_int, [_p, _p, _p, _p, _p, _p, _p, _p, _p, _i64, _i64, _i64, _p, _p, _p, _p, _p, _p, _p, _pi64, _p]),
    'vah_scale_residual_bwd_bsum': (_int, [_p, _p, _p, _p, _i64, _i64, _i64, _p, _p, _p, _p, _pi64, _p]),
    'vah_gelu_bwd_bsum_bf16': (_int, [_p, _p, _i64, _i64, _p, _p, _pi64, _p]),
    'vah_colsum_f32': (_int, [_p, _i64, _i64, _i64, _i64, _p, _p, _p]),
    'vah_bn_tail_ws_floats': (_i64, [_i64]),
    'vah_bn_tail_supported': (_int, [_i64, _i64, _i64, _i64, _int, _int]),
    'vah_bn_tail_stats': (_int, [_p, _int, _p, _int, _p, _int, _i64, _i64, _i64, _i64, _p, _p, _p, _p]),
    'vah_bn_tail_apply': (_int, [_p, _int, _p, _int, _p, _int, _i64, _i64, _i64, _i64, _p, _p, _p, _p, _int, _p, _p, _int, _p]),
    'vah_bn_tail_bwd_stats': (_int, [_p, _int, _p, _int, _p, _int, _i64, _i64, _i64, _i64, _p, _p, _p, _p, _int, _p, _p, _int, _p, _p, _p]),
    'vah_bn_tail_bwd_apply': (_int, [_p, _int, _p, _int, _p, _int, _i64, _i64, _i64, _i64, _p, _p, _p, _p, _int, _p, _p, _int, _p, _p, _p, _p, _p,
                                     _p]),
    'vah_bn_finalize_stats': (_int, [_p, _i64, _f, _f, _p, _p, _p, _p, _p]),
    'vah_pixel_shuffle2_bf16': (_int, [_p, _i64, _i64, _i64, _i64, _p, _int, _p, _p]),
    'vah_transpose_tokens': (_int, [_p, _i64, _i64, _i64, _i64, _i64, _p, _int, _int, _p, _p]),
    'vah_maxpool3s2_fwd_bf16': (_int, [_p, _i64, _i64, _i64, _p, _p, _p]),
    'vah_maxpool3s2_bwd_bf16': (_int, [_p, _p, _i64, _i64, _i64, _p, _p]),
    'vah_conv_taps_nhwc_bf16': (_int, [_p, _i64, _i64, _i64, _i64, _p, _i64, _int, _p, _p, _int, _p, _i64, _i64, _i64, _i64, _int, _int, _int, _p]),
    'vah_conv3x3_dgrad_nhwc_bf16': (_int, [_p, _i64, _i64, _i64, _i64, _p, _i64, _int, _p, _i64, _i64, _p]),
    'vah_conv3x3_wgrad_ws_floats': (_i64, [_i64, _i64]),
    'vah_conv3x3_wgrad_nhwc_bf16': (_int, [_p, _i64, _i64, _i64, _i64, _p, _i64, _i64, _i64, _int, _p, _i64, _p, _p]),
    'vah_image_to_nhwc16_bf16': (_int, [_p, _i64, _i64, _i64, _p, _p]),
    'vah_patchify_bf16': (_int, [_p, _i64, _i64, _i64, _i64, _i64, _p, _p]),
    'vah_bn_nhwc_ws_floats': (_i64, [_i64]),
    'vah_bn_nhwc_stats': (_int, [_p, _i64, _i64, _p, _p, _p]),
    'vah_bn_nhwc_apply': (_int, [_p, _i64, _i64, _p, _p, _p, _p, _int, _p, _p]),
    'vah_bn_nhwc_bwd_stats': (_int, [_p, _p, _i64, _i64, _p, _p, _p, _p, _int, _p, _p, _p]),
    'vah_bn_nhwc_bwd_apply': (_int, [_p, _p, _i64, _i64, _p, _p, _p, _p, _int, _p, _p, _p, _p]),
    'vah_maxpool3s2_nhwc_fwd_bf16': (_int, [_p, _i64, _i64, _i64, _i64, _p, _p, _p]),
    'vah_maxpool3s2_nhwc_bwd_bf16': (_int, [_p, _p, _i64, _i64, _i64, _i64, _p, _p]),
    'vah_gemm_set_tuning': (_int, [_int, _int]),
    'vah_gemm_bf16': (_int, [_int, _int, _i64, _i64, _i64, _p, _i64, _p, _i64, _p, _i64, _int, _int, _p, _int, _p, _i64, _p]),
    'vah_gemm_bf16_fin': (_int, [_int, _int, _i64, _i64, _i64, _p, _i64, _p, _i64, _p, _i64, _int, _p, _i64, _p, _i64, _i64, _p, _p]),
    'vah_gemm_library_version': (_i64, []),
    'vah_gemm_rejected_candidates': (_i64, []),
    'vah_gemm_table_dump': (_i64, [_str, _i64]),
    'vah_gemm_table_load': (_int, [_str]),
    'vah_scale_residual_fwd': (_int, [_p, _p, _p, _p, _i64, _i64, _i64, _p, _p]),
    'vah_scale_residual_bwd': (_int, [_p, _p, _p, _p, _i64, _i64, _i64, _p, _p, _p, _p]),
    'vah_dwconv3x3_tokens_bf16': (_int, [_p, _p, _p, _i64, _i64, _i64, _i64, _int, _p, _p]),
    'vah_dwconv3x3_tokens_wgrad_bf16': (_int, [_p, _p, _i64, _i64, _i64, _i64, _p, _p, _p, _p]),
    'vah_prof_enable': (_int, [_int]),
    'vah_prof_filter': (_int, [_str]),
    'vah_prof_report': (_i64, [_str, _i64]),
}

# The fp16 twins, bf16 spelling -> fp16 name: the bf16 signature with _Float16 in the 16-bit operands.  Five groups:
# the attention / relative-position kernels (csrc/attn_*.hip, csrc/relpos.hip)
ATTN_F16_TWINS = {
    'vah_attn_fwd_bf16': 'vah_attn_fwd_f16', 'vah_attn_bwd_bf16': 'vah_attn_bwd_f16',
    'vah_attn_win_fwd_bf16': 'vah_attn_win_fwd_f16', 'vah_attn_win_bwd_bf16': 'vah_attn_win_bwd_f16',
    'vah_attn_bias_fwd_bf16': 'vah_attn_bias_fwd_f16', 'vah_attn_bias_bwd_bf16': 'vah_attn_bias_bwd_f16',
    'vah_relpos_bias_build': 'vah_relpos_bias_build_f16', 'vah_relpos_bias_grad': 'vah_relpos_bias_grad_f16',
}
# the row-streaming kernels of csrc/fused_ops.hip
FUSED_F16_TWINS = {
    'vah_layernorm_fwd_f32_bf16': 'vah_layernorm_fwd_f32_f16', 'vah_layernorm_bwd_f32_bf16': 'vah_layernorm_bwd_f32_f16',
    'vah_residual_layernorm_fwd': 'vah_residual_layernorm_fwd_f16', 'vah_residual_layernorm_bwd': 'vah_residual_layernorm_bwd_f16',
    'vah_layernorm_dual_fwd': 'vah_layernorm_dual_fwd_f16', 'vah_layernorm_dual_bwd': 'vah_layernorm_dual_bwd_f16',
    'vah_scale_residual_fwd': 'vah_scale_residual_fwd_f16', 'vah_scale_residual_bwd': 'vah_scale_residual_bwd_f16',
    'vah_dwconv3x3_tokens_bf16': 'vah_dwconv3x3_tokens_f16', 'vah_dwconv3x3_tokens_wgrad_bf16': 'vah_dwconv3x3_tokens_wgrad_f16',
}
# the Linear path: the GEMM dispatcher (csrc/gemm.hip) and its satellites in csrc/fused_ops.hip - column sums, GELU
# backward, and the `_bsum` forms of the two residual backward kernels (named after their `_f16` parents)
LINEAR_F16_TWINS = {
    'vah_gemm_bf16': 'vah_gemm_f16', 'vah_gemm_bf16_fin': 'vah_gemm_f16_fin',
    'vah_colsum_bf16': 'vah_colsum_f16', 'vah_colsum_bf16_partials': 'vah_colsum_f16_partials',
    'vah_gelu_bwd_bsum_bf16': 'vah_gelu_bwd_bsum_f16',
    'vah_residual_layernorm_bwd_bsum': 'vah_residual_layernorm_bwd_f16_bsum',
    'vah_scale_residual_bwd_bsum': 'vah_scale_residual_bwd_f16_bsum',
}
# the SpatialPriorModule kernels (csrc/conv.hip, csrc/spm_nhwc.hip); the workspace queries and vah_bn_finalize_stats are shared
SPM_F16_TWINS = {
    'vah_conv_taps_nhwc_bf16': 'vah_conv_taps_nhwc_f16', 'vah_conv3x3_dgrad_nhwc_bf16': 'vah_conv3x3_dgrad_nhwc_f16',
    'vah_conv3x3_wgrad_nhwc_bf16': 'vah_conv3x3_wgrad_nhwc_f16', 'vah_image_to_nhwc16_bf16': 'vah_image_to_nhwc16_f16',
    'vah_bn_nhwc_stats': 'vah_bn_nhwc_stats_f16', 'vah_bn_nhwc_apply': 'vah_bn_nhwc_apply_f16',
    'vah_bn_nhwc_bwd_stats': 'vah_bn_nhwc_bwd_stats_f16', 'vah_bn_nhwc_bwd_apply': 'vah_bn_nhwc_bwd_apply_f16',
    'vah_maxpool3s2_nhwc_fwd_bf16': 'vah_maxpool3s2_nhwc_fwd_f16', 'vah_maxpool3s2_nhwc_bwd_bf16': 'vah_maxpool3s2_nhwc_bwd_f16',
}
# the output-tail kernels (csrc/tail_ops.hip); in the twins the `*_bf16` flags read "fp16 (1) or fp32 (0)".
# vah_bn_tail_supported, vah_bn_tail_ws_floats and vah_bn_finalize_stats are shared
TAIL_F16_TWINS = {
    'vah_bn_tail_stats': 'vah_bn_tail_stats_f16', 'vah_bn_tail_apply': 'vah_bn_tail_apply_f16',
    'vah_bn_tail_bwd_stats': 'vah_bn_tail_bwd_stats_f16', 'vah_bn_tail_bwd_apply': 'vah_bn_tail_bwd_apply_f16',
    'vah_transpose_tokens': 'vah_transpose_tokens_f16', 'vah_maxpool3s2_fwd_bf16': 'vah_maxpool3s2_fwd_f16',
    'vah_maxpool3s2_bwd_bf16': 'vah_maxpool3s2_bwd_f16', 'vah_pixel_shuffle2_bf16': 'vah_pixel_shuffle2_f16',
}
F16_TWINS = {**ATTN_F16_TWINS, **FUSED_F16_TWINS, **LINEAR_F16_TWINS, **SPM_F16_TWINS, **TAIL_F16_TWINS}

# every symbol include/vitadapter_hip.h declares (checked by tests/test_capi_symbols.py): none without a signature
EXPORTS = tuple(SIGNATURES) + tuple(F16_TWINS.values())

_PARENT = {f16: b16 for b16, f16 in F16_TWINS.items()}
for _name in EXPORTS:
    _fn = getattr(lib, _name)
    _fn.restype, _fn.argtypes = SIGNATURES[_PARENT.get(_name, _name)]        # a twin: its parent's signature

# name -> (restype, argtypes) of every entry point include/vitadapter_hip_msda_box.h declares (the fused MSDeformAttn core
# with reference boxes): the *_nref signatures with one int64 ref_comps directly after ref_batch.  The dtype is an
# argument, so there are no fp16 twins.  tests/test_msda_box_abi_cpu.py holds each entry to its prototype.
BOX_SIGNATURES = {
    'vah_msda_fused_forward_box': (_int, [_p, _int, _p, _p, _p, _p, _int, _i64, _i64, _p, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _i64,
                                          _i64, _p, _p]),
    'vah_msda_fused_backward_tiled_box': (_int, [_p, _int, _p, _p, _p, _p, _int, _i64, _i64, _p, _i64, _i64, _i64, _p, _i64, _i64, _i64, _i64, _i64,
                                                 _i64, _i64, _p, _int, _p, _p, _int, _i64, _i64, _p, _i64, _p]),
}
for _name, (_res, _args) in BOX_SIGNATURES.items():
    _fn = getattr(lib, _name)
    _fn.restype, _fn.argtypes = _res, _args

# name -> (restype, argtypes) of every entry point include/vitadapter_hip_group_norm.h declares (GroupNorm on channels-last
# rows, csrc/group_norm.hip).  A tensor operand is (pointer, dtype code, row stride, image stride); the dtype is an
# argument, so there are no fp16 twins.  tests/test_group_norm_abi_cpu.py holds each entry to its prototype.
_t = [_p, _int, _i64, _i64]
GN_SIGNATURES = {
    'vah_group_norm_supported': (_int, [_i64, _i64]),
    'vah_group_norm_ws_floats': (_i64, [_i64, _i64, _i64, _i64]),
    'vah_group_norm_stats': (_int, _t + [_i64, _i64, _i64, _i64, _f, _p, _p, _p, _i64, _p]),
    'vah_group_norm_apply': (_int, _t + [_i64, _i64, _i64, _i64, _p, _p, _p, _p, _int, _p] + _t + [_p]),
    'vah_group_norm_bwd_stats': (_int, _t + _t + [_i64, _i64, _i64, _i64, _p, _p, _p, _p, _int, _p, _p, _p, _p, _i64, _p]),
    'vah_group_norm_bwd_apply': (_int, _t + _t + [_i64, _i64, _i64, _i64, _p, _p, _p, _p, _int, _p] + _t + [_p]),
}
for _name, (_res, _args) in GN_SIGNATURES.items():
    _fn = getattr(lib, _name)
    _fn.restype, _fn.argtypes = _res, _args

# name -> (restype, argtypes) of every entry point include/vitadapter_hip_resize.h declares (bilinear resize on channels-last
# rows and its adjoint, csrc/resize_rows.hip), tensor operands as above.  tests/test_resize_rows_abi_cpu.py holds each entry
# to its prototype.
RESIZE_SIGNATURES = {
    'vah_resize_rows_ws_bytes': (_i64, [_i64, _i64, _i64, _i64]),
    'vah_resize_rows_forward': (_int, _t + [_i64, _i64, _i64, _i64, _i64, _i64, _int] + _t + [_p, _i64, _p]),
    'vah_resize_rows_backward': (_int, _t + [_i64, _i64, _i64, _i64, _i64, _i64, _int] + _t + [_p, _i64, _p]),
}
for _name, (_res, _args) in RESIZE_SIGNATURES.items():
    _fn = getattr(lib, _name)
    _fn.restype, _fn.argtypes = _res, _args

# name -> (restype, argtypes) of every entry point include/vitadapter_hip_masked_attn.h declares (masked cross-attention of
# Mask2Former's query decoder, csrc/masked_attn.hip), tensor operands as above with (token stride, image stride).
# tests/test_masked_attn_abi_cpu.py holds each entry to its prototype.
_mca_dims = [_i64, _i64, _i64, _i64, _i64, _f]              # N, H, Lq, Lk, head_dim, scale
MCA_SIGNATURES = {
    'vah_mca_splits': (_i64, [_i64]),
    'vah_mca_ws_bytes': (_i64, [_i64, _i64, _i64, _i64]),
    'vah_mca_pack_mask': (_int, _t + [_i64, _i64, _i64, _p, _p]),
    'vah_mca_forward': (_int, _t + _t + _t + [_p] + _mca_dims + _t + [_p, _p, _i64, _p]),
    'vah_mca_backward': (_int, _t + _t + _t + [_p] + _t + _t + [_p] + _mca_dims + _t + _t + _t + [_p, _i64, _p]),
}
for _name, (_res, _args) in MCA_SIGNATURES.items():
    _fn = getattr(lib, _name)
    _fn.restype, _fn.argtypes = _res, _args

# name -> (restype, argtypes) of every entry point include/vitadapter_hip_points.h declares (point sampling and the
# matching cost of Mask2Former's training head, csrc/point_loss.hip).  A map operand is (pointer[, dtype code], map stride,
# row stride, maps, height, width).  tests/test_points_abi_cpu.py holds each entry to its prototype.
POINTS_SIGNATURES = {
    'vah_pts_sample': (_int, [_p, _int, _i64, _i64, _i64, _i64, _i64, _p, _i64, _i64, _p, _p, _i64, _p, _p]),
    'vah_pts_match_cost': (_int, [_p, _p, _p, _p, _p, _i64, _i64, _i64, _i64, _i64, _i64, _f, _f, _f, _f, _p, _p]),
}
for _name, (_res, _args) in POINTS_SIGNATURES.items():
    _fn = getattr(lib, _name)
    _fn.restype, _fn.argtypes = _res, _args

# name -> (restype, argtypes) of every entry point include/vitadapter_hip_point_mask_loss.h declares (the sampled BCE / dice
# of the matched masks of Mask2Former's training head and their backward, csrc/point_mask_loss.hip).  A map operand is
# (pointer[, dtype code], map stride, row stride, maps, height, width).  tests/test_point_mask_loss_abi_cpu.py holds each
# entry to its prototype.
PML_SIGNATURES = {
    'vah_pml_ws_bytes': (_i64, [_i64, _i64, _i64, _i64]),
    'vah_pml_forward': (_int, [_p, _i64, _i64, _i64, _i64, _i64, _p, _int, _i64, _i64, _i64, _i64, _i64, _p, _i64, _p, _p, _i64, _f,
                               _p, _p, _p, _p, _p, _p, _i64, _p]),
    'vah_pml_backward': (_int, [_p, _p, _p, _p, _p, _p, _i64, _i64, _i64, _i64, _f, _p, _p, _i64, _p]),
}
for _name, (_res, _args) in PML_SIGNATURES.items():
    _fn = getattr(lib, _name)
    _fn.restype, _fn.argtypes = _res, _args

# name -> (restype, argtypes) of every entry point include/vitadapter_hip_seg.h declares (the logit tail of the Mask2Former
# segmentor, csrc/seg_logits.hip).  An fp32 NCHW operand is (pointer, image stride, plane stride, row stride), a label map
# (pointer, image stride, row stride).  tests/test_seg_logits_abi_cpu.py holds each entry to its prototype.
_pl = [_p, _i64, _i64, _i64]
SEG_SIGNATURES = {
    'vah_seg_resize_add': (_int, _pl + [_i64, _i64, _i64, _i64, _i64, _i64, _int] + _pl + [_i64, _i64, _i64, _i64, _int, _p]),
    'vah_seg_finish': (_int, _pl + [_i64, _i64, _i64, _i64, _p, _p, _int, _i64, _i64, _int, _int] + _pl + [_int, _p, _i64, _i64, _p]),
    'vah_seg_argmax': (_int, _pl + [_i64, _i64, _i64, _i64, _f, _p, _i64, _i64, _p]),
}
for _name, (_res, _args) in SEG_SIGNATURES.items():
    _fn = getattr(lib, _name)
    _fn.restype, _fn.argtypes = _res, _args

# name -> (restype, argtypes) of every entry point include/vitadapter_hip_seg_loss.h declares (the training loss of the
# UperNet heads, csrc/seg_ce_loss.hip).  The logits are (pointer, dtype code, image stride, plane stride, row stride), the
# gradient and the label map as above.  tests/test_seg_ce_loss_abi_cpu.py holds each entry to its prototype.
_sce = [_p, _int, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _p, _i64, _i64, _i64, _i64, _int, _i64, _p]
SCE_SIGNATURES = {
    'vah_sce_ws_bytes': (_i64, [_i64, _i64, _i64, _i64, _i64, _i64]),
    'vah_sce_forward': (_int, _sce + [_p, _p, _p, _p, _i64, _p]),
    'vah_sce_backward': (_int, _sce + [_p, _p] + _pl + [_p, _i64, _p]),
}
for _name, (_res, _args) in SCE_SIGNATURES.items():
    _fn = getattr(lib, _name)
    _fn.restype, _fn.argtypes = _res, _args

# name -> (restype, argtypes) of every entry point include/vitadapter_hip_epoch.h declares: the one-launch 16-bit parameter
# copies of a forward epoch (csrc/epoch_copies.hip), the weight-gradient GEMM whose reduction launch stores through a row map
# (csrc/gemm.hip; `applied` is a host int the call writes) and the BatchNorm finalize launch that also does the module's
# bookkeeping (csrc/tail_ops.hip).  tests/test_epoch_abi_cpu.py holds each entry to its prototype.
_pint = ctypes.POINTER(ctypes.c_int)
_fin_rowmap = [_int, _int, _i64, _i64, _i64, _p, _i64, _p, _i64, _p, _i64, _int, _p, _i64, _p, _i64, _i64, _p, _p, _pint, _p]
EPOCH_SIGNATURES = {
    'vah_epoch_job_bytes': (_i64, []),
    'vah_epoch_chunk_elems': (_i64, []),
    'vah_epoch_copies': (_int, [_p, _i64, _p, _i64, _int, _p, _i64, _p, _i64, _p]),
    'vah_gemm_bf16_fin_rowmap': (_int, _fin_rowmap),
    'vah_gemm_f16_fin_rowmap': (_int, _fin_rowmap),
    'vah_bn_finalize_stats_book': (_int, [_p, _i64, _f, _f, _f, _p, _p, _p, _p, _p, _p]),
}
for _name, (_res, _args) in EPOCH_SIGNATURES.items():
    _fn = getattr(lib, _name)
    _fn.restype, _fn.argtypes = _res, _args

# name -> (restype, argtypes) of every entry point include/vitadapter_hip_seg_eval.h declares (the class counts of the mIoU
# evaluation, csrc/seg_eval.hip).  A label map is (pointer[, dtype code], image stride, row stride).
# tests/test_seg_eval_abi_cpu.py holds each entry to its prototype.
SEGEVAL_SIGNATURES = {
    'vah_segeval_ws_bytes': (_i64, [_i64, _i64, _i64, _i64]),
    'vah_segeval_update': (_int, [_p, _i64, _i64, _p, _int, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _int, _p, _i64, _p, _p, _i64, _p]),
}
for _name, (_res, _args) in SEGEVAL_SIGNATURES.items():
    _fn = getattr(lib, _name)
    _fn.restype, _fn.argtypes = _res, _args

# name -> (restype, argtypes) of every entry point include/vitadapter_hip_seg_target.h declares (Mask2Former's training
# targets from a label map, csrc/seg_target.hip).  The label map is (pointer, dtype code, image stride, row stride).
# tests/test_seg_targets_abi_cpu.py holds each entry to its prototype.
_lm = [_p, _int, _i64, _i64]
SEGTGT_SIGNATURES = {
    'vah_segtgt_ws_bytes': (_i64, [_i64, _i64, _i64]),
    'vah_segtgt_scan': (_int, _lm + [_i64, _i64, _i64, _i64, _p, _p, _p, _p, _p, _i64, _p]),
    'vah_segtgt_masks': (_int, _lm + [_i64, _i64, _i64, _p, _p, _p, _p, _i64, _p, _p, _p, _p]),
}
for _name, (_res, _args) in SEGTGT_SIGNATURES.items():
    _fn = getattr(lib, _name)
    _fn.restype, _fn.argtypes = _res, _args

# name -> (restype, argtypes) of every entry point include/vitadapter_hip_assign.h declares (the assignment step of
# Mask2Former's matching, csrc/assign.hip): cost, gt_offsets, L, N, Q, Gmax, table, status, stream.
# tests/test_hungarian_abi_cpu.py holds the entry to its prototype.
ASSIGN_SIGNATURES = {
    'vah_assign_solve': (_int, [_p, _p, _i64, _i64, _i64, _i64, _p, _p, _p]),
}
for _name, (_res, _args) in ASSIGN_SIGNATURES.items():
    _fn = getattr(lib, _name)
    _fn.restype, _fn.argtypes = _res, _args

if lib.vah_abi_version() != ABI_VERSION:
    raise ImportError('libvitadapter_hip.so ABI %d != binding ABI %d: rebuild the library'
                      % (lib.vah_abi_version(), ABI_VERSION))


class _NoSwitch:
    """Context manager that does nothing (the tensor's device is already current)."""

    def __enter__(self):
        return None

    def __exit__(self, *exc):
        return False


_NO_SWITCH = _NoSwitch()


def on(device):
    """``with on(t.device):`` - make ``device`` current for the HIP calls inside.  torch.cuda.device costs ~5 us of
    host time per use (index normalisation + two exchange calls); a training step enters it ~400 times, always for
    the device that already is current: in that case nothing is switched."""
    import torch
    if device.index is None or torch.cuda.current_device() == device.index:
        return _NO_SWITCH
    return torch.cuda.device(device)


def raw_stream(device):
    """hipStream_t (as an int) of torch's current stream on ``device``.  torch._C._cuda_getCurrentRawStream skips the
    Stream object torch.cuda.current_stream builds (~5 us of host time per kernel launch, ~200 launches per step)."""
    import torch
    idx = device.index if device.index is not None else torch.cuda.current_device()
    try:
        return torch._C._cuda_getCurrentRawStream(idx)
    except AttributeError:                 # other torch builds
        return torch.cuda.current_stream(device).cuda_stream


def check(rc, what):
    """Turn a non-zero ABI return code into RuntimeError (the reference only printf()s)."""
    if rc != 0:
        msg = lib.vah_last_error().decode('utf-8', 'replace')
        raise RuntimeError('%s failed (code %d): %s' % (what, rc, msg))


_SYM = {(b16, torch.bfloat16): getattr(lib, b16) for b16 in SIGNATURES}
_SYM.update(((b16, torch.float16), getattr(lib, f16)) for b16, f16 in F16_TWINS.items())


def sym(name, dtype):
    """The entry point ``name`` (its bf16 spelling) for 16-bit operands of ``dtype``: itself (bf16) or its fp16 twin."""
    try:
        return _SYM[name, dtype]
    except KeyError:
        raise ValueError('no entry point %s for %s operands' % (name, dtype)) from None


def call(name, dtype, *args):
    """sym(name, dtype)(*args), a non-zero return code raised under the name of the symbol that ran."""
    fn = sym(name, dtype)
    check(fn(*args), fn.__name__)


def prof_enable(on, prefix=''):
    """Time the launches of the entry points whose profile name starts with ``prefix``."""
    lib.vah_prof_filter(prefix.encode())
    lib.vah_prof_enable(1 if on else 0)


def prof_report():
    """-> {kernel_name: dict(calls, total_ms, bytes, def_bytes, flops)}; synchronises the recorded events.
    bytes = algorithmic bytes for the IO dtypes the launches ran with, def_bytes = the operator's
    fp32-definition bytes, flops = matrix-core work (0 for the HBM-bound entry points)."""
    need = lib.vah_prof_report(None, 0)
    buf = ctypes.create_string_buffer(int(need) + 64)
    lib.vah_prof_report(buf, len(buf))
    out = {}
    for line in buf.value.decode().splitlines():
        name, calls, ms, nbytes, dbytes, flops = line.split()
        out[name] = dict(calls=int(calls), total_ms=float(ms), bytes=int(nbytes), def_bytes=int(dbytes),
                         flops=int(flops))
    return out


GEMM_EPI_NONE, GEMM_EPI_BIAS = 0, 1


def gemm_table_dump():
    """The GEMM algorithm cache as text: a '#hipblaslt <version>' line, then one problem per line
    (see include/vitadapter_hip.h; the line of an fp16 problem starts with 'f16 ')."""
    n = lib.vah_gemm_table_dump(None, 0)
    buf = ctypes.create_string_buffer(int(n))
    lib.vah_gemm_table_dump(buf, n)
    return '#hipblaslt %d\n' % lib.vah_gemm_library_version() + buf.value.decode()


def gemm_table_load(text):
    """Load a dumped table; a table of another hipBLASLt build is ignored (returns 0): its
    algorithm indices mean nothing here and every problem is simply timed again."""
    first = text.split('\n', 1)[0].split()
    if len(first) == 2 and first[0] == '#hipblaslt' and int(first[1]) != lib.vah_gemm_library_version():
        return 0
    n = lib.vah_gemm_table_load(text.encode())
    if n < 0:
        check(n, 'gemm_table_load')
    return n
