"""ctypes loader for librubiks_hip.so (the C ABI declared in include/rubiks_hip.h).

There is deliberately NO fallback: if the HIP library has not been built, or a tensor is
not on a GPU, the operators raise.  Build with `python -c "import __graft_entry__ as g;
g.build()"` or `rubiksnet_amd/csrc/build.sh`.
"""
import ctypes
import os
import threading

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# RK_HIP_LIB: another build of the same library (kernel A/B runs of tools/; never a different implementation)
LIB_PATH = os.environ.get("RK_HIP_LIB") or os.path.join(_HERE, "csrc", "librubiks_hip.so")

_lock = threading.Lock()
_lib = None

_i = ctypes.c_int
_p = ctypes.c_void_p
_sz = ctypes.c_size_t

# name -> (restype, argtypes); mirrors include/rubiks_hip.h one to one
_DIMS3 = [_i] * 5 + [_i] * 6          # N,T,C,H,W, sT,sH,sW, pT,pH,pW
_DIMS2 = [_i] * 4 + [_i] * 4          # N,C,H,W, sH,sW,pH,pW
SIGNATURES = {
    "rk_version": (_i, []),
    "rk_error_string": (ctypes.c_char_p, [_i]),
    "rk_out_len": (_i, [_i, _i, _i]),
    "rk_device_count": (_i, []),
    "rk_debug_peek_launch_tag": (ctypes.c_uint, []),
    "rk_debug_set_finalize_spins": (_i, [_i]),
    "rk_debug_pw_gemm_plan": (_i, [_i] * 14 + [_p]),
    "rk_debug_pw_wgrad_plan": (_i, [_i] * 5),
    "rk_debug_3d_plan": (_i, [_i] * 20 + [_p]),
    "rk_debug_2d_plan": (_i, [_i] * 15 + [_p]),
    "rk3d_debug_finalize_only_f32": (_i, [_p, _sz, _i, _i, _p, _i, ctypes.c_float, _p]),
    "rk_fin_status_register": (_i, [_p]),
    "rk3d_debug_finalize_only_status_f32": (_i, [_p, _sz, _i, _i, _p, _i, ctypes.c_float, _p, _p]),
    "rk3d_forward_f32": (_i, [_p, _p, _p] + _DIMS3 + [_i, _p]),
    "rk3d_forward_f64": (_i, [_p, _p, _p] + _DIMS3 + [_i, _p]),
    "rk3d_backward_workspace_bytes": (_sz, _DIMS3 + [_i]),
    "rk3d_backward_f32": (_i, [_p] * 5 + _DIMS3 + [_i, ctypes.c_float, _i, _p, _sz, _p]),
    "rk3d_backward_f64": (_i, [_p] * 5 + _DIMS3 + [_i, ctypes.c_double, _i, _p, _sz, _p]),
    # 16-bit activations, fp32 shift table / d(shift)
    "rk3d_forward_bf16_sf32": (_i, [_p, _p, _p] + _DIMS3 + [_i, _p]),
    "rk3d_forward_f16_sf32": (_i, [_p, _p, _p] + _DIMS3 + [_i, _p]),
    "rk3d_backward_bf16_sf32": (_i, [_p] * 5 + _DIMS3 + [_i, ctypes.c_float, _i, _p, _sz, _p]),
    "rk3d_backward_f16_sf32": (_i, [_p] * 5 + _DIMS3 + [_i, ctypes.c_float, _i, _p, _sz, _p]),
    "rk3d_sf32_streams": (_i, _DIMS3 + [_i, _i]),
    "rk3d_backward_partials_f32": (_i, [_p] * 4 + _DIMS3 + [_i, _p, _sz, ctypes.POINTER(ctypes.c_int), _p]),
    "rk3d_backward_finalize_f32": (_i, [_p, _i, _i, _p, _i, ctypes.c_float, _p]),
    "rk2d_backward_workspace_bytes": (_sz, _DIMS2 + [_i]),
    "rk2d_backward_bn_workspace_bytes": (_sz, _DIMS2),
    "rk2d_bn_fused_shape": (_i, [_i] * 9),
    "rk2d_forward_bn_f32": (_i, [_p] * 4 + _DIMS2 + [_i, _p]),
    "rk2d_forward_bn_bf16_sf32": (_i, [_p] * 4 + _DIMS2 + [_i, _p]),
    "rk2d_backward_bn_f32": (_i, [_p] * 9 + _DIMS2 + [_i, _i, _p, _sz, _p]),
    "rk2d_backward_bn_bf16_sf32": (_i, [_p] * 9 + _DIMS2 + [_i, _i, _p, _sz, _p]),
    "rk_tshift3_backward_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "rk_tshift3_bn_forward_f32": (_i, [_p, _p, _p, _p, _i, _i, _i, _i, _p]),
    "rk_tshift3_bn_forward_bf16": (_i, [_p, _p, _p, _p, _i, _i, _i, _i, _p]),
    "rk_tshift3_bn_backward_f32": (_i, [_p, _p, _p, _p, _p, _p, _p, _p, _p, _i, _i, _i, _i, _p, _sz, _p]),
    "rk_tshift3_bn_backward_bf16": (_i, [_p, _p, _p, _p, _p, _p, _p, _p, _p, _i, _i, _i, _i, _p, _sz, _p]),
    "rk_bn_relu_gather2_f32": (_i, [_p, _p, _p, _i, _i, _i, _i, _p]),
    "rk_bn_relu_gather2_bf16": (_i, [_p, _p, _p, _i, _i, _i, _i, _p]),
    "rk_tshift3_bn_backward_fork_f32": (_i, [_p] * 12 + [_i] * 5 + [_p, _sz, _p]),
    "rk_tshift3_bn_backward_fork_bf16": (_i, [_p] * 12 + [_i] * 5 + [_p, _sz, _p]),
    "rk_tshift3_bn_backward_fin_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "rk_tshift3_bn_backward_fin_f32": (_i, [_p] * 11 + [_i, _i, _i, _i, _p, _sz, _p]),
    "rk_tshift3_bn_backward_fin_bf16": (_i, [_p] * 11 + [_i, _i, _i, _i, _p, _sz, _p]),
    "rk_soft_taps_forward_f32": (_i, [_p, _p, _p, _i, _p]),
    "rk_soft_taps_backward_f32": (_i, [_p, _p, _p, _p, _p, _i, _p]),
    "rk_soft_taps_many_forward_f32": (_i, [_p, _i, _p, _i, _p]),
    "rk_soft_taps_many_backward_f32": (_i, [_p, _i, _p, _p, _p, _i, _p]),
    "rk_bn_workspace_bytes": (_sz, [_i, _i, _i]),
    "rk_pw_gemm_f32": (_i, [_p, _p, _p, _p, _i, _i, _i, _i, _i, _p]),
    "rk_pw_gemm_bf16": (_i, [_p, _p, _p, _p, _i, _i, _i, _i, _i, _p]),
    "rk_pw_packed_bytes": (_sz, [_i, _i]),
    "rk_pw_pack_bf16": (_i, [_p, _i, _i, _p, _p, _p]),
    "rk_pw_pack_many_bf16": (_i, [_p, _i, _p, _i, _p]),
    "rk_scatter2x2_add_bf16": (_i, [_p, _p, _p, ctypes.c_longlong, _i, _i, _p]),
    "rk_stem16_supported": (_i, [_i] * 5),
    "rk_stem_conv3x3s2_bf16out": (_i, [_p, _p, _p, _i, _i, _i, _i, _i, _p]),
    "rk_stem_wgrad16_workspace_bytes": (_sz, [_i] * 5),
    "rk_stem_wgrad3x3s2_bf16": (_i, [_p, _p, _p, _i, _i, _i, _i, _i, _p, _sz, _p]),
    "rk_pw_odd16_supported": (_i, [_i, _i, _i, _i]),
    "rk_pw_gemm_packed_odd_bf16": (_i, [_p, _p, _p, _p, _i, _i, _i, _i, _p]),
    "rk_pw_wgrad_odd16_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "rk_pw_wgrad_odd16_bf16": (_i, [_p, _p, _p, _i, _i, _i, _i, _p, _sz, _p]),
    "rk_pw_gemm_packed_bf16": (_i, [_p, _p, _p, _p, _i, _i, _i, _i, _p]),
    "rk_pw16_stat_tiles": (_i, [_i, _i]),
    "rk_pw_gemm_packed_stats_bf16": (_i, [_p, _p, _p, _p, _i, _i, _i, _i, _p, _i, _p]),
    "rk_pw_wgrad16_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "rk_pw_wgrad16_bf16": (_i, [_p, _p, _p, _i, _i, _i, _i, _p, _sz, _p]),
    "rk_stem_conv3x3s2_f32": (_i, [_p, _p, _p, _i, _i, _i, _i, _i, _p]),
    "rk_stem_wgrad3x3s2_f32": (_i, [_p, _p, _p, _i, _i, _i, _i, _i, _p, _sz, _p]),
    "rk_pw_s2_forward_f32": (_i, [_p, _p, _p, _i, _i, _i, _i, _i, _p]),
    "rk_pw_s2_forward_fused_f32": (_i, [_p, _p, _p, _i, _i, _i, _i, _i, _p, _p, _i, _p]),
    "rk_pw_s2_dgrad_f32": (_i, [_p, _p, _p, _i, _i, _i, _i, _i, _p]),
    "rk_pw_s2_wgrad_f32": (_i, [_p, _p, _p, _i, _i, _i, _i, _i, _p, _sz, _p]),
    "rk_bn_fold_f32": (_i, [_p, _p, _p, _p, ctypes.c_float, _p, _p, _i, _p]),
    "rk_bn_fold_many_f32": (_i, [_p, _i, _p, ctypes.c_longlong, _i, _p]),
    "rk_pw_gemm_fused_f32": (_i, [_p, _p, _p, _p, _i, _i, _i, _i, _i, _p, _p, _i, _p, _p, _i, _p]),
    "rk_pw_wgrad_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    # second-generation fp32 kernels (rk_pw2.hip): tuning / test hooks with an explicit kernel configuration
    "rk_pw2_gemm_cfg_f32": (_i, [_p, _p, _p, _p, _i, _i, _i, _i, _i, _p, _p, _i, _i, _i, _i, _p]),
    "rk_pw4_gemm_f32": (_i, [_p, _p, _p, _p, _i, _i, _i, _i, _i, _p, _p, _i, _i, _p, _p, _p, _p, _i, _p]),
    "rk_pw2_wgrad_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "rk_pw2_wgrad_cfg_f32": (_i, [_p, _p, _p, _i, _i, _i, _i, _p, _sz, _p, _p, _i, _i, _i, _i, _p]),
    "rk_pw_wgrad_f32": (_i, [_p, _p, _p, _i, _i, _i, _i, _p, _sz, _p]),
    "rk_pw_wgrad_bf16": (_i, [_p, _p, _p, _i, _i, _i, _i, _p, _sz, _p]),
    # planes with H * W % 4 != 0 (7x7)
    "rk_pw_gemm_odd_f32": (_i, [_p, _p, _p, _p, _i, _i, _i, _i, _i, _p]),
    "rk_pw_wgrad_odd_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "rk_pw_wgrad_odd_f32": (_i, [_p, _p, _p, _i, _i, _i, _i, _p, _sz, _p]),
    "rk_pw_s2_forward_odd_f32": (_i, [_p, _p, _p, _i, _i, _i, _i, _i, _p]),
    "rk_pw_s2_dgrad_odd_f32": (_i, [_p, _p, _p, _i, _i, _i, _i, _i, _p]),
    "rk_pw_s2_wgrad_odd_f32": (_i, [_p, _p, _p, _i, _i, _i, _i, _i, _p, _sz, _p]),
    # training-mode fusion of the block's BatchNorms into the GEMMs (include/rubiks_hip.h)
    "rk3d_forward_bn_f32": (_i, [_p, _p, _p, _p] + _DIMS3 + [_i, _p]),
    "rk3d_backward_bn_workspace_bytes": (_sz, _DIMS3),
    "rk3d_backward_bn_f32": (_i, [_p] * 9 + _DIMS3 + [_i, ctypes.c_float, _i, _p, _sz, _p]),
    "rk_pw_tiles": (_i, [_i, _i]),
    "rk_pw_gemm_tiles": (_i, [_p, _i, _i, _i, _i, _i]),
    "rk_pw_gemm_stats_f32": (_i, [_p, _p, _p, _p, _i, _i, _i, _i, _i, _p, _p, _i, _p, _i, _p]),
    "rk_stem_conv3x3s2_stats_f32": (_i, [_p, _p, _p, _i, _i, _i, _i, _i, _p, _i, _p]),
    "rk_pw_gemm_bnbwd_f32": (_i, [_p, _p, _p, _p, _i, _i, _i, _i, _i, _p, _p, _p, _i, _p]),
    "rk_pw_wgrad_pro_f32": (_i, [_p, _p, _p, _i, _i, _i, _i, _p, _p, _i, _p, _sz, _p]),
    "rk_pw_s2_wgrad_pro_f32": (_i, [_p, _p, _p, _i, _i, _i, _i, _i, _p, _p, _i, _p, _sz, _p]),
    "rk_bn_finish_tiles_f32": (_i, [_p, _i, ctypes.c_longlong, _p, _p, _p, _p, _p, _p, _p, _p, _p, _i, ctypes.c_float,
                                    ctypes.c_float, _p, _p]),
    "rk_bn_tile_stats_f32": (_i, [_p, _p, _i, _i, _i, _p]),
    "rk_bn_apply_affine_f32": (_i, [_p, _p, _p, _p, _i, _i, _i, _i, _p]),
    "rk_bn_apply_affine_bf16": (_i, [_p, _p, _p, _p, _i, _i, _i, _i, _p]),
    "rk_bn_bwd_finish_tiles_f32": (_i, [_p, _i, ctypes.c_longlong, _p, _p, _p, _i, _p]),
    "rk_bn_bwd_dx_pre_f32": (_i, [_p, _p, _p, _p, _p, _p, _p, _p, _i, _i, _i, _p]),
    "rk_bn_bwd_dx_pre_bf16": (_i, [_p, _p, _p, _p, _p, _p, _p, _p, _i, _i, _i, _p]),
    "rk_bn_stats_finish_f32": (_i, [_p, _p, _p, _p, _p, _p, _p, _p, _i, _i, _i, ctypes.c_float, ctypes.c_float, _p, _p, _sz, _p]),
    "rk_bn_stats_finish_bf16": (_i, [_p, _p, _p, _p, _p, _p, _p, _p, _i, _i, _i, ctypes.c_float, ctypes.c_float, _p, _p, _sz, _p]),
    "rk_bn_stats_finish_abmi_f32": (_i, [_p] * 9 + [_i, _i, _i, ctypes.c_float, ctypes.c_float, _p, _p, _sz, _p]),
    "rk_bn_stats_finish_abmi_bf16": (_i, [_p] * 9 + [_i, _i, _i, ctypes.c_float, ctypes.c_float, _p, _p, _sz, _p]),
}
SIGNATURES["rk_se_mlp_forward_f32"] = (_i, [_p, _p, _p, _p, _p, _i, _i, _i, _p])
SIGNATURES["rk_se_mlp_backward_f32"] = (_i, [_p] * 11 + [_i, _i, _i, _p])
SIGNATURES["rk_se_dgate_f32"] = (_i, [_p, _p, _p, _i, _i, _i, _p])
SIGNATURES["rk_se_scale_add_f32"] = (_i, [_p, _p, _p, ctypes.c_float, _p, _i, _i, _i, _p])
# the one-launch optimizer step (rk_optim.hip): jobs, n, chunks, host hyper-parameter records, groups, partials, count,
# max_norm, norm_out, zero_grads, stream
SIGNATURES["rk_debug_optim_chunks"] = (_i, [_p, _i, _p])
SIGNATURES["rk_optim_sqnorm_workspace_bytes"] = (_sz, [_i])
SIGNATURES["rk_optim_sqnorm_many_f32"] = (_i, [_p, _i, _i, _p, _p])
SIGNATURES["rk_optim_sgd_many_f32"] = (_i, [_p, _i, _i, _p, _i, _p, _i, ctypes.c_float, _p, _i, _p])
SIGNATURES["rk_optim_adam_many_f32"] = (_i, [_p, _i, _i, _p, _i, _p, _i, ctypes.c_float, _p, _i, _p])
# the extended step: rule, then as above up to zero_grads, then ema pointers, ema_decay, 1 - ema_decay, guard, skipped, stream
SIGNATURES["rk_optim_step_ext_f32"] = (_i, [_i, _p, _i, _i, _p, _i, _p, _i, ctypes.c_float, _p, _i, _p, ctypes.c_float,
                                            ctypes.c_float, _i, _p, _p])
# the streaming metrics launch (rk_metrics.hip): logits, labels, state, videos, views, classes, confusion, ntopk, k0..k3,
# consensus, pred, rank, loss (each may be NULL), stream
SIGNATURES["rk_metrics_state_bytes"] = (_sz, [_i, _i])
for _sfx in ("f32", "bf16", "f16"):
    SIGNATURES["rk_metrics_update_" + _sfx] = (_i, [_p, _p, _p] + [_i] * 9 + [_p] * 5)
# baseline JPEG decode (rk_jpeg.hip): host frame table, n -> bytes; streams, stream_bytes, frames, qtabs, htabs, nq, nh, n,
# rgb, rgb_bytes, workspace, workspace_bytes, status, stream
SIGNATURES["rk_jpeg_workspace_bytes"] = (_sz, [_p, _i])
SIGNATURES["rk_jpeg_decode_u8"] = (_i, [_p, ctypes.c_longlong, _p, _p, _p, _i, _i, _i, _p, ctypes.c_longlong, _p, _sz, _p, _p])
# resident frames decoded by scan index: streams, stream_bytes, frames, htabs, nq, nh, n, seg_mcus, entry_off, entries,
# n_entries, status, stream / host frame table, n, host pick, m, max_segments -> bytes / streams, stream_bytes, frames, qtabs,
# htabs, nq, nh, n, entries, n_entries, entry_off, seg_mcus, build_status, pick, rgb_off, m, max_segments, rgb, rgb_bytes,
# workspace, workspace_bytes, status, stream
SIGNATURES["rk_jpeg_build_index"] = (_i, [_p, ctypes.c_longlong, _p, _p, _i, _i, _i, _p, _p, _p, ctypes.c_longlong, _p, _p])
SIGNATURES["rk_jpeg_chunked_workspace_bytes"] = (_sz, [_p, _i, _i])
# ... entries, n_entries, chunk_bytes, max_rounds, workspace, workspace_bytes, status, route, stream
SIGNATURES["rk_jpeg_build_index_chunked"] = (_i, [_p, ctypes.c_longlong, _p, _p, _i, _i, _i, _p, _p, _p, ctypes.c_longlong, _i, _i,
                                                  _p, _sz, _p, _p, _p])
SIGNATURES["rk_jpeg_indexed_workspace_bytes"] = (_sz, [_p, _i, _p, _i, _i])
SIGNATURES["rk_jpeg_decode_indexed_u8"] = (_i, [_p, ctypes.c_longlong, _p, _p, _p, _i, _i, _i, _p, ctypes.c_longlong, _p, _p, _p, _p,
                                                _p, _i, _i, _p, ctypes.c_longlong, _p, _sz, _p, _p])
# resident frames as packed coefficients: streams, stream_bytes, frames, htabs, nq, nh, n, entries, n_entries, entry_off, seg_mcus,
# build_status, max_segments, workspace, workspace_bytes, status, block_off, block_cap, first_block, region_off, stream / frames,
# n, max_segments, workspace, workspace_bytes, status, block_off, block_cap, first_block, region_off, blob, blob_bytes, stream /
# host frame table, n, host pick, m -> bytes / blob, blob_bytes, frames, qtabs, nq, n, region_off, build_status, pick, rgb_off, m,
# rgb, rgb_bytes, workspace, workspace_bytes, status, stream
SIGNATURES["rk_jpeg_coef_sizes"] = (_i, [_p, ctypes.c_longlong, _p, _p, _i, _i, _i, _p, ctypes.c_longlong, _p, _p, _p, _i, _p, _sz, _p,
                                         _p, ctypes.c_longlong, _p, _p, _p])
SIGNATURES["rk_jpeg_coef_pack"] = (_i, [_p, _i, _i, _p, _sz, _p, _p, ctypes.c_longlong, _p, _p, _p, ctypes.c_longlong, _p])
SIGNATURES["rk_jpeg_coef_workspace_bytes"] = (_sz, [_p, _i, _p, _i])
SIGNATURES["rk_jpeg_decode_coef_u8"] = (_i, [_p, ctypes.c_longlong, _p, _p, _i, _i, _p, _p, _p, _p, _i, _p, ctypes.c_longlong, _p, _sz,
                                             _p, _p])
# the same three with a trailing record_format (behind the stream); format, nblocks, &least, &most -> status
for _name, _as in (("rk_jpeg_coef_sizes", "rk_jpeg_coef_sizes_as"), ("rk_jpeg_coef_pack", "rk_jpeg_coef_pack_as"),
                   ("rk_jpeg_decode_coef_u8", "rk_jpeg_decode_coef_as_u8")):
    SIGNATURES[_as] = (_i, SIGNATURES[_name][1] + [_i])
SIGNATURES["rk_jpeg_coef_region_bounds"] = (_i, [_i, ctypes.c_longlong, _p, _p])
for _sfx in ("f32", "bf16"):
    SIGNATURES["rk_clip_u8_to_chw_" + _sfx] = (_i, [_p, _p, _p, _p, _i, _i, _i, _i, _p])
    SIGNATURES["rk_clip_resample_u8_" + _sfx] = (_i, [_p] * 5 + [_i] * 7 + [_p])     # B,T,Hs,Ws,V,Sh,Sw
    # arena, arena_bytes, clips, frame_idx, boxes, mean3, std3, out, B, V, T, Sh, Sw, stream
    SIGNATURES["rk_clip_resample_ragged_u8_" + _sfx] = (_i, [_p, ctypes.c_longlong] + [_p] * 6 + [_i] * 5 + [_p])
    SIGNATURES["rk_se_squeeze_" + _sfx] = (_i, [_p, _p, _i, _i, _i, _p])
    SIGNATURES["rk_se_scale_" + _sfx] = (_i, [_p, _p, _p, _i, _i, _i, _p])
    SIGNATURES["rk_se_scale_backward_" + _sfx] = (_i, [_p, _p, _p, _p, _p, _i, _i, _i, _p])
    SIGNATURES["rk_bn_relu_forward_" + _sfx] = (
        _i, [_p] * 8 + [_i, _i, _i, ctypes.c_float, ctypes.c_float, _i, _i, _p, _sz, _p])
    SIGNATURES["rk_bn_relu_forward_counted_" + _sfx] = (
        _i, [_p] * 8 + [_i, _i, _i, ctypes.c_float, ctypes.c_float, _i, _p, _p, _sz, _p])
    SIGNATURES["rk_bn_relu_backward_" + _sfx] = (_i, [_p] * 10 + [_i, _i, _i, _i, _p, _sz, _p])
for _sfx in ("f32", "f64", "f16", "bf16"):
    SIGNATURES["rk2d_forward_" + _sfx] = (_i, [_p, _p, _p] + _DIMS2 + [_i, _p])
    SIGNATURES["rk2d_backward_" + _sfx] = (_i, [_p] * 5 + _DIMS2 + [_i, _i, _i, _p, _sz, _p])
    if _sfx in ("f16", "bf16"):          # 16-bit activations, fp32 shift table / d(shift)
        SIGNATURES["rk2d_forward_%s_sf32" % _sfx] = SIGNATURES["rk2d_forward_" + _sfx]
        SIGNATURES["rk2d_backward_%s_sf32" % _sfx] = SIGNATURES["rk2d_backward_" + _sfx]
    SIGNATURES["rk_tshift3_forward_" + _sfx] = (_i, [_p, _p, _p, _i, _i, _i, _i, _p])
    SIGNATURES["rk_tshift3_backward_" + _sfx] = (_i, [_p] * 5 + [_i, _i, _i, _i, _p, _sz, _p])


class RubiksHipError(RuntimeError):
    """A librubiks_hip entry point returned a negative RK_ERR_* code."""


def lib():
    """Load (once) and return the ctypes handle; raises if the library is not built."""
    global _lib
    if _lib is None:
        with _lock:
            if _lib is None:
                if not os.path.exists(LIB_PATH):
                    raise RuntimeError(
                        "librubiks_hip.so not found at %s -- the HIP extension is not built and there is "
                        "no CPU fallback. Run `python -c \"import __graft_entry__ as g; g.build()\"`." % LIB_PATH
                    )
                handle = ctypes.CDLL(LIB_PATH)
                for name, (res, args) in SIGNATURES.items():
                    fn = getattr(handle, name)   # AttributeError here = ABI mismatch, loudly
                    fn.restype = res
                    fn.argtypes = args
                _lib = handle
    return _lib


def check(rc, what):
    if rc != 0:
        msg = lib().rk_error_string(int(rc)).decode()
        raise RubiksHipError("%s failed: %s (code %d)" % (what, msg, rc))


def call(name, *args):
    """`lib().name(*args)`; a non-zero status raises RubiksHipError naming the entry point."""
    rc = getattr(lib(), name)(*args)
    if rc != 0:
        check(rc, name)


def launch(name, dev, *args, after=()):
    """`call` with device `dev` current and its current stream's handle as the last argument (`after`: what the entry
    point takes behind the stream)."""
    with torch.cuda.device(dev):
        call(name, *args, torch.cuda.current_stream(dev).cuda_stream, *after)


def ptr(t):
    return t.data_ptr() if t is not None else None


def workspace(query_name, dev, *dims):
    """(uint8 scratch tensor on `dev`, its size in bytes as the `*_workspace_bytes` query `query_name` gives it)."""
    nbytes = int(getattr(lib(), query_name)(*dims))
    return torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev), nbytes


def dtype_suffix(dtype):
    return {
        torch.float32: "f32",
        torch.float64: "f64",
        torch.float16: "f16",
        torch.bfloat16: "bf16",
    }.get(dtype)
