"""ctypes binding of libdram_hip.so (C ABI: include/dram_hip.h).

The library is the product: there is no CPU or PyTorch fallback.  Importing this
module without the built library raises ImportError with the build command.
"""
import ctypes
import os
from ctypes import c_char_p, c_float, c_int, c_int64, c_size_t, c_void_p

# torch FIRST: it bundles its own libamdhip64.so (soname libamdhip64.so.7).  Loaded after torch, libdram_hip.so binds
# to that already-mapped runtime, i.e. to the one that owns the device buffers and streams it is handed.  Loaded
# before torch, the dynamic loader resolves the soname to /opt/rocm's copy instead and torch then maps its own on
# top: two HIP runtimes in one process, and every launch from this library fails ("no ROCm-capable device").
import torch  # noqa: F401  (import order matters, see above)

_HERE = os.path.dirname(os.path.abspath(__file__))
# (DRAM_HIP_LIB: another build of the same library -- diagnostics / A-B experiments only)
LIB_PATH = os.environ.get("DRAM_HIP_LIB") or os.path.join(os.path.dirname(_HERE), "libdram_hip.so")

P, I, L, F, Z = c_void_p, c_int, c_int64, c_float, c_size_t

# name -> (restype, argtypes); mirrors include/dram_hip.h one to one
SIGNATURES = {
    "dram_last_error": (c_char_p, []),
    "dram_abi_version": (I, []),
    "dram_conv3d_k3_packed_floats": (Z, [I, I]),
    "dram_conv3d_k3_pack_weights": (I, [P, P, I, I, I, P]),
    "dram_conv3d_k3_fwd_ex": (I, [P, I, P, I, I, I, I, I, I, I, P, P, P, I, P, I, I, I, I, I, I, I, I, I, I, I, P]),
    "dram_conv3d_k3_wgrad_ws_bytes": (Z, [I, I, I, I, I, I]),
    "dram_conv3d_fwd": (I, [P, P, P, P] + [I] * 15 + [P]),
    "dram_conv3d_bwd_data": (I, [P, P, P] + [I] * 15 + [P]),
    "dram_conv3d_wgrad_ws_bytes": (Z, [I] * 15),
    "dram_conv3d_wgrad": (I, [P, P, P, P, Z] + [I] * 15 + [P]),
    "dram_conv3d_gen_launch_counts": (I, [P, I]),
    "dram_channel_sum_ws_bytes": (Z, [I, I, L]),
    "dram_channel_sum": (I, [P, P, P, Z, I, I, L, P]),
    "dram_norm_ws_bytes": (Z, [I, I, L]),
    "dram_norm_fwd_train": (I, [P, P, P, P, P, P, P, P, P, F, F, I, I, I, I, I, L, P, Z, P]),
    "dram_bn_fwd_eval": (I, [P, P, P, P, P, P, P, P, P, F, I, I, I, L, P]),
    "dram_norm_bwd": (I, [P, P, P, P, P, P, P, P, P, I, I, I, I, I, I, L, P, Z, P]),
    "dram_norm_bwd_head_ok": (I, [I]),
    "dram_norm_bwd_head": (I, [P, P, I, P, P, P, P, P, P, P, P, I, I, I, I, I, I, L, P, Z, P]),
    "dram_norm_bwd_pool_add": (I, [P, P, P, I, I, I, P, P, P, P, P, P, P, P, I, I, I, I, I, I, P, Z, P]),
    "dram_bn_stats": (I, [P, P, I, I, L, P, Z, P]),
    "dram_bn_bwd_sums": (I, [P, P, P, P, P, P, I, I, I, L, P, Z, P]),
    "dram_bn_bwd_apply_sums": (I, [P, P, P, P, P, P, P, ctypes.c_double, P, I, I, I, L, P, Z, P]),
    "dram_relu_fwd": (I, [P, P, L, P]),
    "dram_relu_bwd": (I, [P, P, P, L, P]),
    "dram_maxpool3d_2_fwd": (I, [P, P, P, I, I, I, I, I, P]),
    "dram_maxpool3d_2_bwd": (I, [P, P, P, I, I, I, I, I, P]),
    "dram_maxpool3d_fwd": (I, [P, P, P] + [I] * 14 + [P]),
    "dram_maxpool3d_bwd": (I, [P, P, P] + [I] * 14 + [P]),
    "dram_upsample_trilinear_ac_fwd": (I, [P, P, I, I, I, I, I, I, I, I, P]),
    "dram_upsample_trilinear_ac_bwd": (I, [P, P, I, I, I, I, I, I, I, I, P]),
    "dram_upsample_trilinear_ac_bwd_ws_bytes": (Z, [I, I, I, I, I, I, I, I]),
    "dram_upsample_trilinear_ac_bwd_ws": (I, [P, P, P, Z, I, I, I, I, I, I, I, I, P]),
    "dram_upsample_trilinear_ac_bwd_choice": (I, [I, I, I, Z, I, I, I, I, I, I, I, I, P]),
    "dram_crop_concat_fwd": (I, [P, P, P, I, I, I, I, I, I, I, I, I, I, I, I, P]),
    "dram_crop_concat_bwd": (I, [P, P, P, I, I, I, I, I, I, I, I, I, I, I, I, P]),
    "dram_conv3d_k1_fwd": (I, [P, P, P, P, I, I, I, L, P]),
    "dram_conv3d_k1_bwd_ws_bytes": (Z, [I, I, I, L]),
    "dram_conv3d_k1_bwd": (I, [P, P, P, P, P, P, P, Z, I, I, I, L, P]),
    "dram_conv3d_k1_fwd_choice": (I, [I, I, L]),
    "dram_conv3d_k1_bwd_choice": (I, [I, I, I, I, I, L, I]),
    "dram_masked_mean_ws_bytes": (Z, [I, I, L]),
    "dram_masked_mean_fwd": (I, [P, P, P, P, P, Z, I, I, L, P]),
    "dram_masked_mean_bwd": (I, [P, P, P, P, I, I, L, P]),
    "dram_label_bboxes": (I, [P, P, I, I, I, I, P]),
    "dram_lobe_chunks": (I, [P, P, P, P, I, I, I, I, I, F, F, P]),
    "dram_lobe_paste": (I, [P, P, P, P, I, I, I, I, I, P]),
    "dram_lobe_chunk_masks": (I, [P, P, P, I, I, I, I, I, P]),
    "dram_lobe_cam_max": (I, [P, P, P, I, I, I, P, P, P]),
    "dram_lobe_cam_paste": (I, [P, P, P, P, P, P, I, I, I, I, I, I, P]),
    "dram_lung_hist256": (I, [P, P, P, P, L, P]),
    "dram_threshold_mask": (I, [P, P, F, L, P]),
    "dram_scan_hist256": (I, [P, P, P, I, I, L, P]),
    "dram_lesion_post": (I, [P, P, P, P, P, F, I, I, ctypes.c_double, L, P]),
    "dram_mask_overlap": (I, [P, P, P, L, P]),
    "dram_resample_volume": (I, [P, P, I, I, I, I, I, I, I, I, P, P, P]),
    "dram_intreg_loss_ws_bytes": (Z, [I, L]),
    "dram_intreg_loss_state_floats": (I, [I]),
    "dram_intreg_loss_fwd": (I, [P, P, P, P, P, P, P, F, P, P, P, Z, I, L, P]),
    "dram_intreg_loss_bwd": (I, [P, P, P, P, P, P, P, P, P, F, P, P, I, L, P]),
    "dram_intreg_enc_loss_ws_bytes": (Z, [I, L]),
    "dram_intreg_enc_loss_state_floats": (I, [I]),
    "dram_intreg_enc_loss_fwd": (I, [P, P, P, P, P, P, P, Z, I, L, P]),
    "dram_intreg_enc_loss_bwd": (I, [P, P, P, P, P, P, P, I, L, P]),
    "dram_intreg_targets_ws_bytes": (Z, [I, L]),
    "dram_intreg_targets": (I, [P, P, P, P, ctypes.c_double, P, P, P, P, Z, I, L, P]),
    "dram_prelu_fwd": (I, [P, P, P, I, I, I, L, P]),
    "dram_prelu_bwd_ws_bytes": (Z, [I, I, L]),
    "dram_prelu_bwd": (I, [P, P, P, P, P, P, Z, I, I, I, L, P]),
    "dram_global_max_fwd": (I, [P, P, P, I, L, P]),
    "dram_global_max_bwd": (I, [P, P, P, I, L, P]),
    "dram_dropout": (I, [P, P, L, ctypes.c_uint, F, ctypes.c_ulonglong, ctypes.c_ulonglong, P]),
    "dram_resize_trilinear_fwd": (I, [P, P, I, I, I, I, I, I, I, I, F, F, F, P]),
    "dram_resize_trilinear_bwd": (I, [P, P, I, I, I, I, I, I, I, I, F, F, F, P]),
    "dram_resize_nearest": (I, [P, P, I, I, I, I, I, I, I, I, F, F, F, P]),
    "dram_spatial_permute_flip": (I, [P, P, I, I, I, I, I, P, P, P]),
    "dram_pcm_attention_split_fwd": (I, [P, P, P, I, I, I, I, P, I, I, I, I, I, P]),
    "dram_pcm_attention_split_bwd": (I, [P, P, P, P, P, I, I, I, I, P, P, P, P, I, I, I, I, I, P]),
    "dram_pcm_attention_sum_fwd": (I, [P, P, P, I, I, P, I, I, I, I, I, P]),
    "dram_pcm_attention_sum_bwd": (I, [P, P, P, P, P, I, I, P, P, P, I, I, I, I, I, P]),
    "dram_pcm_aggregate_fwd": (I, [P, P, P, I, P, I, I, I, I, I, P]),
    "dram_pcm_aggregate_bwd": (I, [P, P, P, P, I, P, P, I, I, I, I, I, P]),
    # fused conv -> norm -> ReLU -> conv chains ("lazy" tensors)
    "dram_conv3d_k3_stats_parts": (I, [I, I, I, I, I]),
    "dram_conv3d_k3_fwd_fused": (I, [P, I, P, I, P, I, P, I, I, I, I, I, I, I, P, P, P, P, I, I, I, I, I, I, P]),
    "dram_conv3d_k3_wgrad_lazy_ok": (I, [I, I, I, I, I, I, I]),
    "dram_conv3d_k3_wgrad_fused": (I, [P, I, P, I, P, I, P, I, I, I, I, I, I, I, P, P, P, Z, I, I, I, I, I, P]),
    "dram_conv3d_k3_fwd_choice_src": (I, [I, I, I, I, I, I, I, I, I, I, I, I, I, I, I, I, I, c_char_p, Z]),
    "dram_conv3d_k3_wgrad_choice": (I, [I, I, I, I, I, I, I, I, c_char_p, Z]),
    "dram_conv3d_k3_kernel_rows": (I, [c_char_p, Z]),
    "dram_conv3d_k3_launch_counts": (I, [P, I]),
    "dram_norm_parts_ws_bytes": (Z, [I, I, I]),
    "dram_norm_finalize_parts": (I, [P, I, P, P, P, P, P, P, P, F, F, I, I, I, I, L, P, Z, P]),
    "dram_bn_parts_stats": (I, [P, I, P, I, I, L, P, Z, P]),
    "dram_bn_eval_coef": (I, [P, P, P, P, P, P, P, F, I, I, P]),
    "dram_row_affine_act": (I, [P, P, P, I, L, L, P]),
    "dram_maxpool3d_2_fwd_lazy": (I, [P, P, I, P, P, I, I, I, I, I, P]),
    "dram_maxpool3d_2_bwd_acc": (I, [P, P, P, I, I, I, I, I, P]),
    "dram_upsample_trilinear_ac_fwd_lazy": (I, [P, P, I, P, I, I, I, I, I, I, I, I, P]),
    "dram_conv3d_k1_fwd_lazy": (I, [P, P, I, P, P, P, I, I, I, L, P]),
    "dram_conv3d_k1_bwd_lazy": (I, [P, P, P, I, P, P, P, P, P, Z, I, I, I, L, P]),
    # affine-consistency losses
    "dram_sigmoid_fwd": (I, [P, P, L, P]),
    "dram_sigmoid_bwd": (I, [P, P, P, L, P]),
    "dram_masked_smooth_l1_ws_bytes": (Z, [I, I, L]),
    "dram_masked_smooth_l1_fwd": (I, [P, P, P, P, P, Z, I, I, L, P]),
    "dram_masked_smooth_l1_bwd": (I, [P, P, P, P, P, P, P, I, I, L, P]),
    # segmentation losses with a given target
    "dram_seg_loss_ws_bytes": (Z, [L]),
    "dram_seg_loss_state_floats": (I, []),
    "dram_seg_loss_chunk": (I, []),
    "dram_boot_bce_fwd": (I, [P, P, P, I, I, L, ctypes.c_double, P, P, P, Z, P]),
    "dram_boot_bce_bwd": (I, [P, P, P, I, I, L, ctypes.c_double, P, P, P, P]),
    "dram_bce_smooth_fwd": (I, [P, P, I, L, ctypes.c_double, P, P, P, Z, P]),
    "dram_bce_smooth_bwd": (I, [P, P, I, L, ctypes.c_double, P, P, P, P]),
    # per-sample Tversky + focal loss on logits with a given target
    "dram_seg_overlap_ws_bytes": (Z, [I, L]),
    "dram_seg_overlap_state_floats": (I, [I]),
    "dram_seg_overlap_fwd": (I, [P, P, P, I, I, I, L] + [ctypes.c_double] * 5 + [P, P, P, Z, P]),
    "dram_seg_overlap_bwd": (I, [P, P, P, I, I, I, L, ctypes.c_double, ctypes.c_double, P, P, P, P]),
    "dram_affine_sample_fwd": (I, [P, P, P, I, I, I, I, I, P]),
    "dram_affine_sample_bwd": (I, [P, P, P, I, I, I, I, I, P]),
    # measured ceilings (bench.py)
    "dram_calibrate_hbm_copy": (I, [P, P, Z, P]),
    "dram_calibrate_mfma_f32": (I, [P, I, I, P, P]),
    # training-time augmentation pool
    "dram_aug_minmax": (I, [P, P, P, I, L, P]),
    "dram_aug_gaussian_blur": (I, [P, P, P, P, I, I, I, I, I, I, P]),
    "dram_aug_mask_out": (I, [P, P, P, P, P, P, I, I, I, I, I, I, P]),
    "dram_aug_gaussian_noise": (I, [P, P, P, P, P, P, I, P, I, L, P]),
    "dram_aug_permute_flip": (I, [P, P, I, P, P, P, I, I, I, I, I, I, P]),
    "dram_aug_row_mean_ws_bytes": (Z, [I, L]),
    "dram_aug_row_mean": (I, [P, P, P, I, L, P, Z, P]),
    "dram_aug_intensity_map": (I, [P, P, I, P, P, P, I, P, I, I, L, P]),
    "dram_aug_row_mean_std_ws_bytes": (Z, [I, L]),
    "dram_aug_row_mean_std": (I, [P, P, P, I, L, P, Z, P]),
    "dram_aug_slab_project": (I, [P, P, P, P, I, P, I, I, I, I, I, P]),
    "dram_aug_keep_region": (I, [P, P, I, P, P, P, I, I, I, I, I, I, P]),
    "dram_aug_pad_min_ws_bytes": (Z, [I, I, I, I, I]),
    "dram_aug_pad_min": (I, [P, I, P, I, I, I, I, P, Z, P]),
    "dram_aug_crop_resample": (I, [P, P, I, I, P, P, Z, P, I, I, I, I, I, P]),
    "dram_aug_minmax_u8": (I, [P, P, P, I, L, P]),
    "dram_aug_spline_ws_bytes": (Z, [I, I, I, I]),
    "dram_aug_spline_prefilter": (I, [P, P, P, I, I, I, I, I, P, Z, P]),
    "dram_aug_spline_resample": (I, [P, P, I, I, P, P, P, Z, P, I, I, I, I, I, P]),
    # device chunk loader
    "dram_chunk_hist256": (I, [P, P, P, I, P, I, I, P]),
    "dram_otsu256": (I, [P, I, ctypes.c_double, P, P]),
    "dram_chunk_prepare": (I, [P, P, P, P, P, I, I, I, I, F, F, I, I, P, P, P, P, P]),
    # lesion-wise report: connected components, their statistics, LUT relabelling, per-lobe burden
    "dram_cc_ws_bytes": (Z, [I, I, I]),
    "dram_cc_label": (I, [P, P, P, I, I, I, I, P, Z, P]),
    "dram_cc_stats": (I, [P, P, I, P, P, P, I, I, I, P]),
    "dram_cc_relabel": (I, [P, P, I, P, P, L, P]),
    "dram_lobe_burden": (I, [P, P, P, L, P]),
    # lesion density report: per-label moments and histograms of the scan, their percentiles and band counts
    "dram_label_density_plan": (I, [I, I, I]),
    "dram_label_density": (I, [P, P, I, P, I, P, P, P, P, P, P, I, I, I, L, P]),
    "dram_hist_summary": (I, [P, I, I, I, I, P, I, P, I, P, P, P]),
    # lesion distribution report: per-label reduction of a depth map and of the voxel positions
    "dram_label_depth_plan": (I, [I, I, I, I]),
    "dram_label_depth": (I, [P, P, I, P, I, P, P, P, P, P, P, I, I, P, P, I, I, I, I, I, I, P]),
    # lesion shape report: per-label 2x2x2 configuration histogram and second-order moments
    "dram_label_shape_plan": (I, [I, I]),
    "dram_label_shape": (I, [P, I, I, P, P, I, I, I, P]),
    # lesion texture report: per-label grey-level co-occurrence tables in the 13 directions
    "dram_label_glcm_plan": (I, [I, I, I, I]),
    "dram_label_glcm": (I, [P, P, I, P, I, I, I, I, I, P, I, I, I, P]),
    # heat-map evaluation curves: the joint histogram of score bin x class x region
    "dram_score_hist_plan": (I, [I, I, I]),
    "dram_score_hist": (I, [P, P, P, P, I, I, P, P, L, P]),
    # surface-distance metrics: exact Euclidean distance transform, mask surface, compaction over a surface
    "dram_edt_max_dim": (I, []),
    "dram_edt_ws_bytes": (Z, [I, I, I]),
    "dram_edt": (I, [P, P] + [ctypes.c_double] * 3 + [I, I, I, P, Z, P]),
    "dram_mask_surface": (I, [P, P, P, I, I, I, P]),
    "dram_surface_gather": (I, [P, P, P, P, L, L, P]),
    # pseudo-vessel mask: Hessian of Gaussian, Frangi's c, eigenvalues and vesselness, mask
    "dram_vessel_max_radius": (I, []),
    "dram_hessian_ws_bytes": (Z, [I, I, I]),
    "dram_hessian": (I, [P, I, F, F, P, P, P, I, I, I, P, P, Z, P]),
    "dram_hessian_norm_max": (I, [P, P, L, P, P]),
    "dram_vesselness": (I, [P, L, ctypes.c_double, ctypes.c_double, P, P, I, P, P]),
    "dram_vessel_mask": (I, [P, P, F, P, L, P]),
    # heat-map refinement: the masked 3-D guided filter
    "dram_guided_max_radius": (I, []),
    "dram_guided_ws_bytes": (Z, [I, I, I]),
    "dram_guided_filter": (I, [P, I, ctypes.c_double, ctypes.c_double, P, P, P, ctypes.c_double, I, I, I, P, P, P, Z, P]),
    # result contact sheet: planes of the zoomed coordinate mask, the rendered sheet (layers: host array of dram_sheet_layer)
    "dram_sheet_occupancy": (I, [P, I, I, I, I, I, I, I, P, P]),
    "dram_sheet_render": (I, [P, I, I, I, P, P, I, P, I, I, I, I, I, I, I, I, I, I, ctypes.c_double, P, P]),
    # test-time augmentation for the per-lobe inference (views: host array of V x {perm[3], flip[3]})
    "dram_tta_expand": (I, [P, P, I, I, P, I, P]),
    "dram_tta_combine": (I, [P, P, P, I, I, P, I, P]),
    "dram_lobe_paste_prob": (I, [P, P, P, P, P, P, I, I, I, I, I, P]),
    # optimiser update (table: host array of dram_optim_tensor)
    "dram_optim_table_capacity": (I, []),
    "dram_optim_adam": (I, [P, I] + [ctypes.c_double] * 5 + [I, I, I, P]),
    "dram_optim_sgd": (I, [P, I] + [ctypes.c_double] * 4 + [I, I, P]),
    "dram_optim_radam": (I, [P, I] + [ctypes.c_double] * 5 + [I, I, P]),
    "dram_optim_adabound": (I, [P, I] + [ctypes.c_double] * 4 + [I] + [ctypes.c_double] * 2 + [P]),
    # global-norm gradient clipping over the same tables
    "dram_optim_grad_norm_partials": (Z, [P, I]),
    "dram_optim_grad_norm": (I, [P, I, I, P, L, P]),
    "dram_optim_grad_norm_finish": (I, [P, L, I, ctypes.c_double, P, P]),
    "dram_optim_adam_scaled": (I, [P, I] + [ctypes.c_double] * 5 + [I, I, I, P, P]),
    "dram_optim_sgd_scaled": (I, [P, I] + [ctypes.c_double] * 4 + [I, I, P, P]),
    "dram_optim_radam_scaled": (I, [P, I] + [ctypes.c_double] * 5 + [I, I, P, P]),
    "dram_optim_adabound_scaled": (I, [P, I] + [ctypes.c_double] * 4 + [I] + [ctypes.c_double] * 2 + [P, P]),
    "dram_optim_grad_scale": (I, [P, I, P, P]),
}


class DramHipError(RuntimeError):
    """A libdram_hip.so entry point returned a DRAM_E* status."""


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: the HIP library is the only implementation of this path "
            f"(no CPU fallback). Build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            f"or `make -C bodyct-dram_amd/csrc`.")
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)   # AttributeError if the library does not export a declared symbol
        fn.restype = res
        fn.argtypes = args
    return lib


lib = _load()


def call(name, *args):
    """Call an int-returning entry point; raise DramHipError on a non-zero status."""
    rc = getattr(lib, name)(*args)
    if rc != 0:
        msg = lib.dram_last_error()
        raise DramHipError(f"{name} failed ({rc}): {msg.decode() if msg else '?'}")
