"""ctypes binding of libgradtts_gfx950.so (C ABI: include/gradtts_abi.h).

PyTorch is only plumbing here: it owns device memory (packed weights, workspace, tensors) and the stream.
There is NO fallback: if the library is missing or a call fails, a RuntimeError is raised.
"""
import ctypes
import math
import weakref
import os
import threading

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("GTTS_LIB", os.path.join(_HERE, "libgradtts_gfx950.so"))   # GTTS_LIB: tuning variants

PREC_BF16X3 = 0
PREC_BF16 = 1
PREC_BF16_STORE = 2
PREC_F16F8 = 3          # fp16 hi*hi + both cross terms in one fp8 MFMA on the 3x3 Block convolutions (ABI 5); fp32-grade like bf16x3

_lib = None
_lock = threading.Lock()


class UnetCfg(ctypes.Structure):
    _fields_ = [("dim", ctypes.c_int), ("n_feats", ctypes.c_int), ("n_spks", ctypes.c_int),
                ("spk_emb_dim", ctypes.c_int), ("groups", ctypes.c_int), ("pe_scale", ctypes.c_float),
                ("beta_min", ctypes.c_float), ("beta_max", ctypes.c_float), ("precision", ctypes.c_int),
                ("keep_intermediates", ctypes.c_int), ("arch", ctypes.c_int), ("dim_cond", ctypes.c_int),
                ("use_ref_t", ctypes.c_int), ("c_dim", ctypes.c_int), ("vc_beta_min", ctypes.c_double),
                ("vc_beta_max", ctypes.c_double), ("conv_ws", ctypes.c_int)]


class EncCfg(ctypes.Structure):
    _fields_ = [("mode", ctypes.c_int), ("n_vocab", ctypes.c_int), ("n_feats", ctypes.c_int), ("channels", ctypes.c_int),
                ("filter_channels", ctypes.c_int), ("filter_channels_dp", ctypes.c_int), ("n_heads", ctypes.c_int),
                ("n_layers", ctypes.c_int), ("kernel_size", ctypes.c_int), ("window_size", ctypes.c_int)]


class VocCfg(ctypes.Structure):
    _fields_ = [("n_mels", ctypes.c_int), ("upsample_initial_channel", ctypes.c_int), ("n_ups", ctypes.c_int),
                ("upsample_rates", ctypes.c_int * 8), ("upsample_kernel_sizes", ctypes.c_int * 8),
                ("n_kernels", ctypes.c_int), ("resblock_kernel_sizes", ctypes.c_int * 8),
                ("resblock_dilations", (ctypes.c_int * 3) * 8), ("resblock_type", ctypes.c_int)]


class MelCfg(ctypes.Structure):
    _fields_ = [("n_fft", ctypes.c_int), ("num_mels", ctypes.c_int), ("sampling_rate", ctypes.c_int), ("hop_size", ctypes.c_int),
                ("win_size", ctypes.c_int), ("fmin", ctypes.c_double), ("fmax", ctypes.c_double)]


class FglCfg(ctypes.Structure):
    _fields_ = [("n_fft", ctypes.c_int), ("n_mels", ctypes.c_int), ("hop_size", ctypes.c_int), ("momentum", ctypes.c_double)]


class SpkCfg(ctypes.Structure):
    _fields_ = [("n_mels", ctypes.c_int), ("hidden", ctypes.c_int), ("layers", ctypes.c_int), ("embed", ctypes.c_int)]


class WavCfg(ctypes.Structure):
    _fields_ = [("source_sr", ctypes.c_int), ("sampling_rate", ctypes.c_int), ("n_fft", ctypes.c_int), ("hop_size", ctypes.c_int),
                ("n_mels", ctypes.c_int), ("lowpass_filter_width", ctypes.c_int), ("rolloff", ctypes.c_double),
                ("fmin", ctypes.c_double), ("fmax", ctypes.c_double)]


class PackItem(ctypes.Structure):           # gtts_pack_item
    _fields_ = [("w", ctypes.c_void_p), ("packed", ctypes.c_void_p), ("kind", ctypes.c_int), ("cin", ctypes.c_int),
                ("cout", ctypes.c_int), ("transposed", ctypes.c_int)]


# Every handle family spells its life-cycle entry points gtts_<family>_<op>, except three names the plan has had since ABI 1.
_PLAN_NAMES = {"packed_bytes": "gtts_packed_weight_bytes", "pack": "gtts_pack_weights", "workspace_bytes": "gtts_workspace_bytes"}


def _sym(family, op):
    if family == "plan" and op in _PLAN_NAMES:
        return _PLAN_NAMES[op]
    return "gtts_%s_%s" % (family, op)


def lib():
    """Load the HIP library (once).  Fails loudly when it has not been built."""
    global _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                "libgradtts_gfx950.so is not built (%s). Run `python -c 'import __graft_entry__ as g; g.build()'` "
                "or `python speech-backbones_amd/build.py`. There is no CPU/PyTorch fallback for the sampling path."
                % LIB_PATH)
        L = ctypes.CDLL(LIB_PATH)
        vp, i, f, sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_size_t
        L.gtts_abi_version.restype = i
        L.gtts_last_error.restype = ctypes.c_char_p
        # the handle families with parameters (_Native): create takes the family's configuration, gtts_pack_weights also the frequency table
        for fam, cfg, extra in (("plan", [ctypes.POINTER(UnetCfg)], [vp]), ("voc", [ctypes.POINTER(VocCfg)], []),
                                ("enc", [ctypes.POINTER(EncCfg)], []), ("postnet", [i, i, i], []),
                                ("spk", [ctypes.POINTER(SpkCfg)], [])):
            fn = {op: getattr(L, _sym(fam, op)) for op in ("create", "destroy", "num_params", "param_info", "packed_bytes", "pack",
                                                            "workspace_bytes")}
            fn["create"].argtypes = cfg + [ctypes.POINTER(vp)]
            fn["destroy"].argtypes, fn["destroy"].restype = [vp], None
            fn["num_params"].argtypes = [vp]
            fn["param_info"].argtypes = [vp, i, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(i), ctypes.POINTER(i * 4)]
            fn["packed_bytes"].argtypes, fn["packed_bytes"].restype = [vp], sz
            fn["pack"].argtypes = [vp, ctypes.POINTER(vp), i] + extra + [vp, vp]
            fn["workspace_bytes"].argtypes, fn["workspace_bytes"].restype = [vp, i, i], sz
        L.gtts_plan_set_streams.argtypes = [vp, ctypes.POINTER(vp), i]
        L.gtts_plan_set_graph.argtypes = [vp, i]
        L.gtts_mas_maximum_path_cpu.argtypes = [vp, vp, vp, vp, vp, i, i, i]
        L.gtts_bcast_weights.argtypes = [vp, sz, i, vp, vp]
        L.gtts_estimator_forward.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp, sz, i, i, vp]
        L.gtts_euler_step.argtypes = [vp, vp, vp, vp, vp, f, f, i, i, i, vp]
        L.gtts_reverse_diffusion.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp, sz, i, i, i, i, i, vp]
        L.gtts_mas_scratch_bytes.argtypes = [i, i, i]
        L.gtts_mas_scratch_bytes.restype = sz
        L.gtts_mas_maximum_path.argtypes = [vp, vp, vp, vp, vp, vp, i, i, i, vp]
        L.gtts_expand_alignment.argtypes = [vp, vp, vp, vp, vp, f, vp, vp, vp, i, i, i, i, vp]
        L.gtts_log_prior.argtypes = [vp, vp, vp, i, i, i, i, vp]
        L.gtts_diffusion_noising.argtypes = [vp, vp, vp, vp, vp, f, f, vp, vp, i, i, i, vp]
        L.gtts_score_loss_partials.argtypes = [i, i, i]
        L.gtts_score_loss_partials.restype = sz
        L.gtts_score_loss.argtypes = [vp, vp, vp, f, f, f, vp, vp, i, i, i, vp]
        L.gtts_conv3x3_packed_bytes.argtypes = [i, i]
        L.gtts_conv3x3_packed_bytes.restype = sz
        L.gtts_conv3x3_pack.argtypes = [vp, vp, i, i, i, vp]
        L.gtts_conv3x3_masked.argtypes = [vp, vp, i, vp, vp, vp, vp, vp, i, i, i, i, i, vp]
        L.gtts_conv3x3_wgrad_workspace_bytes.argtypes = [i, i, i, i, i]
        L.gtts_conv3x3_wgrad_workspace_bytes.restype = sz
        L.gtts_conv3x3_wgrad.argtypes = [vp, vp, i, vp, vp, vp, vp, vp, sz, i, i, i, i, i, vp]
        L.gtts_conv1x1_packed_bytes.argtypes = [i, i]
        L.gtts_conv1x1_packed_bytes.restype = sz
        L.gtts_conv1x1_pack.argtypes = [vp, vp, i, i, i, vp]
        L.gtts_conv1x1_masked.argtypes = [vp, vp, vp, vp, vp, i, i, i, i, i, vp]
        L.gtts_conv1x1_wgrad_workspace_bytes.argtypes = [i, i, i, i, i]
        L.gtts_conv1x1_wgrad_workspace_bytes.restype = sz
        L.gtts_conv1x1_wgrad.argtypes = [vp, vp, vp, vp, vp, vp, sz, i, i, i, i, i, vp]
        L.gtts_conv_resample_packed_bytes.argtypes = [i, i, i]
        L.gtts_conv_resample_packed_bytes.restype = sz
        L.gtts_conv_resample_pack.argtypes = [vp, vp, i, i, i, vp]
        L.gtts_conv_resample.argtypes = [vp, vp, vp, vp, vp, i, i, i, i, i, i, vp]
        L.gtts_conv_train_kernel_name.argtypes = [i, i, i, i, i, i, i, i, ctypes.c_char_p, sz]
        L.gtts_add_masked.argtypes = [vp, vp, vp, vp, i, i, i, i, i, vp]
        L.gtts_conv_wgrad_small_scratch_floats.argtypes = [i, i, i, i]
        L.gtts_conv_wgrad_small_scratch_floats.restype = sz
        L.gtts_conv_wgrad_small.argtypes = [vp, vp, vp, vp, vp, vp, i, i, i, i, i, i, vp]
        L.gtts_conv_dgrad_small.argtypes = [vp, vp, vp, vp, i, i, i, i, i, i, vp]
        L.gtts_diffusion_noising_backward.argtypes = [vp, vp, vp, f, f, vp, vp, i, i, i, vp]
        L.gtts_align_index.argtypes = [vp, vp, vp, vp, i, i, i, vp]
        L.gtts_duration_loss.argtypes = [vp, vp, vp, vp, vp, i, i, vp]
        L.gtts_align_gather_partials.argtypes, L.gtts_align_gather_partials.restype = [i, i, i], sz
        L.gtts_align_gather_forward.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, i, i, i, i, i, vp]
        L.gtts_align_gather_backward.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp, i, i, i, i, vp]
        L.gtts_zero_insert2.argtypes = [vp, vp, i, i, i, i, vp]
        L.gtts_space_to_depth2.argtypes = [vp, vp, i, i, i, i, vp]
        L.gtts_final_conv_forward.argtypes = [vp, vp, vp, vp, vp, i, i, i, i, vp]
        L.gtts_final_conv_scratch_floats.argtypes = [i, i, i, i]
        L.gtts_final_conv_scratch_floats.restype = sz
        L.gtts_final_conv_backward.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, i, i, i, i, vp]
        L.gtts_attn_train_scratch_floats.argtypes = [i, i]
        L.gtts_attn_train_scratch_floats.restype = sz
        L.gtts_attn_train_forward.argtypes = [vp, vp, vp, vp, vp, i, i, vp]
        L.gtts_attn_train_backward.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, i, i, vp]
        L.gtts_rezero_forward.argtypes = [vp, vp, vp, vp, sz, vp]
        L.gtts_rezero_scratch_bytes.argtypes = [sz]
        L.gtts_rezero_scratch_bytes.restype = sz
        L.gtts_rezero_backward.argtypes = [vp, vp, vp, vp, vp, vp, sz, vp]
        L.gtts_gn_mish_forward.argtypes = [vp, vp, vp, vp, vp, vp, vp, i, i, i, i, i, f, vp]
        L.gtts_gn_mish_stats_floats.argtypes = [i, i]
        L.gtts_gn_mish_stats_floats.restype = sz
        L.gtts_gn_mish_scratch_bytes.argtypes = [i, i]
        L.gtts_gn_mish_scratch_bytes.restype = sz
        L.gtts_gn_mish_backward.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i, i, i, i, i, vp]
        L.gtts_enc_attention_path.argtypes = [vp, i]
        L.gtts_enc_forward.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, sz, i, i, vp]
        L.gtts_enc_layernorm.argtypes = [vp, vp, vp, vp, vp, vp, vp, i, i, i, f, i, i, vp]
        L.gtts_enc_attention.argtypes = [vp, vp, vp, vp, vp, vp, vp, i, i, i, i, i, i, vp]
        L.gtts_enc_attention_path_for.argtypes = [i, i, i, i]
        L.gtts_enc_attention_train_ok.argtypes = [i, i, i, i]
        L.gtts_enc_attention_train_scratch_bytes.argtypes, L.gtts_enc_attention_train_scratch_bytes.restype = [i, i, i, i, i], sz
        L.gtts_enc_attention_train_forward.argtypes = [vp] * 9 + [i] * 5 + [vp]
        L.gtts_enc_attention_train_backward.argtypes = [vp] * 15 + [i] * 5 + [vp]
        L.gtts_enc_layernorm_backward_scratch_floats.argtypes, L.gtts_enc_layernorm_backward_scratch_floats.restype = [i, i, i], sz
        L.gtts_enc_layernorm_backward.argtypes = [vp] * 12 + [i, i, i, f, i, i, vp]
        L.gtts_postnet_forward.argtypes = [vp, vp, vp, vp, vp, vp, sz, i, i, vp]
        L.gtts_conv1d_create.argtypes = [i, i, i, i, i, i, ctypes.POINTER(vp)]
        L.gtts_conv1d_destroy.argtypes, L.gtts_conv1d_destroy.restype = [vp], None
        L.gtts_conv1d_packed_bytes.argtypes, L.gtts_conv1d_packed_bytes.restype = [vp], sz
        L.gtts_conv1d_pack.argtypes = [vp, vp, vp, vp]
        L.gtts_conv1d_forward.argtypes = [vp, vp, vp, vp, vp, vp, vp, i, f, f, vp, vp, i, i, vp]
        L.gtts_conv1d_instance.argtypes = [vp, i, i, i, i, i, ctypes.POINTER(i * 5)]
        L.gtts_conv1d_pack_dgrad.argtypes = [vp, vp, vp, vp]
        L.gtts_conv1d_wgrad_workspace_bytes.argtypes, L.gtts_conv1d_wgrad_workspace_bytes.restype = [vp, i, i], sz
        L.gtts_conv1d_wgrad.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, sz, i, i, vp]
        L.gtts_conv1d_wgrad_info.argtypes = [vp, i, i, ctypes.POINTER(i * 6)]
        L.gtts_voc_hop.argtypes = [vp]
        L.gtts_voc_forward.argtypes = [vp, vp, vp, vp, vp, sz, i, i, vp]
        L.gtts_plan_num_tensors.argtypes = [vp]
        L.gtts_plan_tensor_info.argtypes = [vp, i, i, i, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(sz),
                                            ctypes.POINTER(i * 4)]
        L.gtts_vc_workspace_bytes.argtypes = [vp, i, i, i]
        L.gtts_vc_workspace_bytes.restype = sz
        L.gtts_vc_estimator_forward.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, sz, i, i, i, vp]
        L.gtts_vc_reverse_diffusion.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, sz, i, i, i, i, i, i, i, vp]
        L.gtts_vc_tensor_info.argtypes = [vp, i, i, i, i, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(sz),
                                          ctypes.POINTER(i * 4)]
        L.gtts_plan_num_ops.argtypes = [vp]
        L.gtts_plan_op_info.argtypes = [vp, i, i, i, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(ctypes.c_char_p),
                                        ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double)]
        L.gtts_profile_enable.argtypes = [vp, i]
        L.gtts_profile_collect.argtypes = [vp, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_longlong)]
        L.gtts_profile_timeline.argtypes = [vp, i, ctypes.POINTER(i), ctypes.POINTER(i), ctypes.POINTER(ctypes.c_double),
                                            ctypes.POINTER(ctypes.c_double), ctypes.POINTER(i)]
        L.gtts_pack_batch_desc_bytes.argtypes = [i]
        L.gtts_pack_batch_desc_bytes.restype = sz
        L.gtts_pack_batch_describe.argtypes = [ctypes.POINTER(PackItem), i, vp, ctypes.POINTER(i)]
        L.gtts_pack_batch.argtypes = [vp, i, i, vp]
        L.gtts_ubench_mfma_out_floats.argtypes = [i]
        L.gtts_ubench_mfma_out_floats.restype = sz
        L.gtts_ubench_mfma.argtypes = [vp, sz, vp, i, i, ctypes.POINTER(ctypes.c_double), vp]
        L.gtts_ubench_hbm.argtypes = [vp, vp, vp, sz, i, i, ctypes.POINTER(ctypes.c_double), vp]
        L.gtts_workspace_status.argtypes = [vp, ctypes.POINTER(ctypes.c_uint), ctypes.POINTER(f), vp]
        L.gtts_in_glu_stats_floats.argtypes = [i, i]
        L.gtts_in_glu_stats_floats.restype = sz
        L.gtts_in_glu_scratch_floats.argtypes = [i, i]
        L.gtts_in_glu_scratch_floats.restype = sz
        L.gtts_in_glu_forward.argtypes = [vp, vp, vp, vp, vp, i, i, i, i, f, vp]
        L.gtts_in_glu_backward.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp, i, i, i, i, vp]
        L.gtts_in_glu_tb_forward.argtypes = [vp, vp, vp, vp, vp, vp, i, i, i, i, f, vp]
        L.gtts_in_glu_tb_backward.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i, i, i, i, vp]
        L.gtts_cond_field_forward.argtypes = [vp, vp, vp, vp, i, i, i, i, i, vp]
        L.gtts_cond_field_backward.argtypes = [vp, vp, vp, i, i, i, i, i, vp]
        L.gtts_masked_mean_forward.argtypes = [vp, vp, vp, i, i, i, i, vp]
        L.gtts_masked_mean_backward.argtypes = [vp, vp, vp, i, i, i, i, vp]
        L.gtts_conv3x3_narrow_workspace_bytes.argtypes, L.gtts_conv3x3_narrow_workspace_bytes.restype = [i, i, i, i, i, i], sz
        L.gtts_conv3x3_narrow_forward.argtypes = [vp, vp, vp, vp, vp, vp, vp, sz, i, i, i, i, i, vp]
        L.gtts_conv3x3_narrow_dgrad.argtypes = [vp, vp, vp, vp, vp, vp, sz, i, i, i, i, i, vp]
        L.gtts_conv3x3_narrow_wgrad.argtypes = [vp, vp, vp, vp, vp, vp, vp, sz, i, i, i, i, i, vp]
        L.gtts_conv7x7_packed_bytes.argtypes = [i, i]
        L.gtts_conv7x7_packed_bytes.restype = sz
        L.gtts_conv7x7_pack.argtypes = [vp, vp, i, i, i, vp]
        L.gtts_conv7x7_masked.argtypes = [vp, vp, vp, vp, vp, vp, i, i, i, i, i, vp]
        L.gtts_conv7x7_wgrad_workspace_bytes.argtypes = [i, i, i, i, i]
        L.gtts_conv7x7_wgrad_workspace_bytes.restype = sz
        L.gtts_conv7x7_wgrad.argtypes = [vp, vp, vp, vp, vp, vp, sz, i, i, i, i, i, vp]
        L.gtts_postnet_expand.argtypes = [vp, vp, vp, vp, vp, i, i, i, i, vp]
        L.gtts_postnet_collapse.argtypes = [vp, vp, vp, vp, vp, i, i, i, i, vp]
        L.gtts_postnet_chan_dot_scratch_floats.argtypes = [i, i, i, i]
        L.gtts_postnet_chan_dot_scratch_floats.restype = sz
        L.gtts_postnet_chan_dot.argtypes = [vp, vp, vp, vp, vp, vp, i, i, i, i, vp]
        L.gtts_mel_create.argtypes = [ctypes.POINTER(MelCfg), ctypes.POINTER(vp)]
        L.gtts_mel_destroy.argtypes, L.gtts_mel_destroy.restype = [vp], None
        L.gtts_mel_frames.argtypes = [vp, i]
        L.gtts_mel_packed_bytes.argtypes, L.gtts_mel_packed_bytes.restype = [vp], sz
        L.gtts_mel_pack.argtypes = [vp, vp, vp]
        L.gtts_mel_filterbank.argtypes = [vp, vp]
        L.gtts_mel_forward.argtypes = [vp, vp, vp, vp, vp, i, i, vp]
        L.gtts_mel_backward_workspace_bytes.argtypes, L.gtts_mel_backward_workspace_bytes.restype = [vp, i, i], sz
        L.gtts_mel_backward.argtypes = [vp, vp, vp, vp, vp, vp, vp, sz, i, i, vp]
        L.gtts_fgl_create.argtypes = [ctypes.POINTER(FglCfg), ctypes.POINTER(vp)]
        L.gtts_fgl_destroy.argtypes, L.gtts_fgl_destroy.restype = [vp], None
        L.gtts_fgl_samples.argtypes = [vp, i]
        L.gtts_fgl_packed_bytes.argtypes, L.gtts_fgl_packed_bytes.restype = [vp], sz
        L.gtts_fgl_pack.argtypes = [vp, vp, vp, vp]
        L.gtts_fgl_workspace_bytes.argtypes, L.gtts_fgl_workspace_bytes.restype = [vp, i, i], sz
        L.gtts_fgl_init.argtypes = [vp, vp, vp, vp, vp, vp, sz, i, i, vp]
        L.gtts_fgl_step.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, sz, i, i, vp]
        L.gtts_fgl_forward.argtypes = [vp, vp, vp, vp, vp, sz, i, i, i, vp]
        L.gtts_spk_forward.argtypes = [vp, vp, vp, i, i, i, i, i, vp, vp, vp, vp, sz, vp]
        L.gtts_spktrain_packed_bytes.argtypes, L.gtts_spktrain_packed_bytes.restype = [vp], sz
        for op in ("saved_bytes", "workspace_bytes"):
            fn = getattr(L, "gtts_spktrain_" + op)
            fn.argtypes, fn.restype = [vp, i, i], sz
        L.gtts_spktrain_pack.argtypes = [vp, ctypes.POINTER(vp), i, vp, vp]
        L.gtts_spktrain_forward.argtypes = [vp, vp, vp, i, i, vp, vp, sz, vp]
        L.gtts_spktrain_backward.argtypes = [vp, vp, vp, vp, vp, sz, ctypes.POINTER(vp), i, vp, sz, i, i, vp]
        L.gtts_ge2e_workspace_bytes.argtypes, L.gtts_ge2e_workspace_bytes.restype = [i, i, i], sz
        L.gtts_ge2e_loss.argtypes = [vp, vp, vp, i, i, i, vp, vp, vp, vp, vp, vp, sz, vp]
        L.gtts_wav_create.argtypes = [ctypes.POINTER(WavCfg), ctypes.POINTER(vp)]
        L.gtts_wav_destroy.argtypes, L.gtts_wav_destroy.restype = [vp], None
        for op in ("resampled_length", "frames", "tiles"):
            getattr(L, "gtts_wav_" + op).argtypes = [vp, i]
        L.gtts_wav_span.argtypes = [vp]
        L.gtts_wav_taps.argtypes = [vp, vp, vp]
        L.gtts_wav_filterbank.argtypes = [vp, vp]
        L.gtts_wav_packed_bytes.argtypes, L.gtts_wav_packed_bytes.restype = [vp], sz
        L.gtts_wav_pack.argtypes = [vp, vp, vp]
        L.gtts_wav_workspace_bytes.argtypes, L.gtts_wav_workspace_bytes.restype = [vp, i, i], sz
        L.gtts_wav_resample.argtypes = [vp, vp, vp, vp, vp, i, i, vp]
        L.gtts_wav_normalize.argtypes = [vp, vp, vp, ctypes.c_double, i, vp, vp, sz, i, i, vp]
        L.gtts_wav_powmel.argtypes = [vp, vp, vp, vp, i, i, vp]
        if L.gtts_abi_version() != 7:
            raise RuntimeError("libgradtts_gfx950.so ABI version mismatch")
        _lib = L
        return _lib


class RangeError(RuntimeError):
    """GTTS_E_RANGE: a value lies outside what the plan's precision represents (f16f8: a 3x3 conv weight with |w| >= 63.97)."""


def _check(rc, what):
    if rc != 0:
        exc = RangeError if rc == -7 else RuntimeError
        raise exc("%s failed (%d): %s" % (what, rc, lib().gtts_last_error().decode()))


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


class _NoSwitch:
    def __enter__(self):
        return None

    def __exit__(self, *exc):
        return False


_NO_SWITCH = _NoSwitch()


def _on(device):
    """Context that makes `device` current for the launches inside -- free when it already is (the training wrappers run
    ~600 launches per step; torch.cuda.device() costs more host time than the launch it guards)."""
    if device.index is None or device.index == torch.cuda.current_device():
        return _NO_SWITCH
    return torch.cuda.device(device)


def _ptr(t):
    return ctypes.c_void_p(0 if t is None else t.data_ptr())


def _launch(device, name, *args):
    """THE call of an entry point that takes a stream: with `device` current (as _on makes it), gtts_<...> `name` on tensors and None
    as pointers, every other argument (ints, floats, ctypes values) as it is, and the current stream last; a failure raises through
    _check under the same name."""
    if device.type != "cuda":
        raise RuntimeError("%s launches on a HIP device (got %s); there is no CPU fallback" % (name, device))
    fn = getattr(_lib or lib(), name)
    args = [a.data_ptr() if isinstance(a, torch.Tensor) else a for a in args]
    index, current = device.index, torch.cuda.current_device()
    if index is None or index == current:                    # (the free path of _on, without its context)
        rc = fn(*args, _raw_stream(current))
    else:
        with torch.cuda.device(device):
            rc = fn(*args, _raw_stream(index))
    if rc:
        _check(rc, name)


def _raw_stream(index):
    """The current stream of device `index` as the address the entry points take -- what _stream gives, without building the
    torch.cuda.Stream object in between (a microsecond of host time per launch, which pays for the argument checks of a wrapper)."""
    return _RAW_STREAM(index)


# (torch keeps the raw getter under torch._C; a build without it takes the public road)
_RAW_STREAM = getattr(torch._C, "_cuda_getCurrentRawStream", None) or (lambda index: torch.cuda.current_stream(index).cuda_stream)


class ArgumentError(ValueError, RuntimeError):
    """An argument that a wrapper refuses before anything is launched: ONE type for every family.  The wrappers no longer tell a
    ValueError family (decoder, PostNet, condition path) from a RuntimeError one (encoders, glue): this type is both, so every
    `except` and every test written against either keeps catching what it caught; new code catches ArgumentError."""


def _in(op, name, t, shape=None, dev=None, strict=False, optional=False, dtype=torch.float32):
    """THE rule for a tensor the wrapper `op` passes to a kernel as the input `name`; returns the tensor the kernel reads.
    None is accepted (and returned) where the argument is `optional`.  dev: the call's device; None for the call's first tensor, which
    has to live on a HIP device (there is no CPU fallback).  Coercing (default): `dtype` and a contiguous layout are produced, by a copy
    only where the tensor does not have them.  strict (the encoder ops, which take views into larger allocations as they are): both
    are required, nothing is converted or copied.  shape: a tuple is the exact shape; an int the element count (where callers pass
    different views of the same memory: a weight given flat or as [1,C,1,1]); None: not checked (the tensor the sizes are read from)."""
    if t is None:
        if optional:
            return None
        raise ArgumentError("%s: %s is required (got None)" % (op, name))
    if (not t.is_cuda) if dev is None else (t.device != dev):
        if t.is_cuda:
            raise ArgumentError("%s: %s lives on %s, the call runs on %s" % (op, name, t.device, dev))
        raise ArgumentError("%s: %s must live on a HIP device (got %s); the kernels need HIP tensors, there is no CPU fallback" %
                            (op, name, t.device))
    if strict:
        if t.dtype != dtype or not t.is_contiguous():
            raise ArgumentError("%s: %s must be a contiguous %s tensor on %s" % (op, name, dtype, t.device))
    else:
        if t.dtype != dtype:
            t = t.to(dtype)
        t = t.contiguous()
    if shape is not None:
        if shape.__class__ is int:
            if t.numel() != shape:
                raise ArgumentError("%s: %s has %d elements (shape %s), expected %d" % (op, name, t.numel(), tuple(t.shape), shape))
        elif t.shape != shape:
            raise ArgumentError("%s: %s has shape %s, expected %s" % (op, name, tuple(t.shape), tuple(shape)))
    return t


def _f32c(t, name):
    """The handle methods' coercion (they keep their own checks and messages)."""
    if t is None:
        return None
    if not t.is_cuda:
        raise RuntimeError("%s must live on a HIP device (got %s); the sampling path has no CPU fallback" %
                           (name, t.device))
    if t.dtype != torch.float32:
        t = t.float()
    return t.contiguous()


def _rebuild(cls, kw):
    return cls(**kw)


class _Native:
    """Owner of one native handle of the family gtts_<_family>_*.  A handle is host metadata: copies and pickles rebuild it from its
    constructor arguments (EMA deep copies, torch.save(model) of a module that already ran)."""
    _family = None

    def _open(self, kw, *create_args):
        """kw: the constructor arguments a copy is rebuilt from; create_args: what gtts_<family>_create takes before the handle."""
        self._kw = kw
        self._h = ctypes.c_void_p()
        self._ws = {}               # the single live workspace: {(shape..., str(device)): uint8 tensor}
        self._call("create", *create_args, ctypes.byref(self._h))

    def _fn(self, op):
        return getattr(lib(), _sym(self._family, op))

    def _call(self, op, *args):
        _check(self._fn(op)(*args), _sym(self._family, op))

    def _launch(self, device, op, *args):
        """_launch of this family's entry point `op`, which takes the handle first."""
        _launch(device, _sym(self._family, op), self._h, *args)

    def __reduce__(self):
        return (_rebuild, (type(self), self._kw))

    def __deepcopy__(self, memo):
        return type(self)(**self._kw)

    def __del__(self):
        try:
            if self._h:
                self._fn("destroy")(self._h)
                self._h = None
        except Exception:
            pass

    # ---- state_dict layout
    def param_layout(self):
        out = []
        for k in range(self._fn("num_params")(self._h)):
            name, rank, dims = ctypes.c_char_p(), ctypes.c_int(), (ctypes.c_int * 4)()
            self._call("param_info", self._h, k, ctypes.byref(name), ctypes.byref(rank), ctypes.byref(dims))
            out.append((name.value.decode(), tuple(dims[:rank.value])))
        return out

    def packed_bytes(self):
        return int(self._fn("packed_bytes")(self._h))

    # ---- weights
    def _params(self, state, device, hint=""):
        """The fp32 device tensors of param_layout(), checked against it, and their pointer array (which does not own them)."""
        keep = []
        for name, shape in self.param_layout():
            if name not in state:
                raise RuntimeError("state_dict is missing '%s'%s" % (name, hint))
            t = state[name].detach().to(device=device, dtype=torch.float32).contiguous()
            if tuple(t.shape) != shape:
                raise RuntimeError("parameter %s has shape %s, expected %s" % (name, tuple(t.shape), shape))
            keep.append(t)
        return keep, (ctypes.c_void_p * len(keep))(*[t.data_ptr() for t in keep])

    def _pack(self, params, device, *extra):
        keep, arr = params
        blob = torch.empty(self.packed_bytes(), dtype=torch.uint8, device=device)
        self._launch(blob.device, "pack", arr, len(keep), *extra, blob)
        torch.cuda.current_stream(blob.device).synchronize()     # sources in `keep` may be temporaries
        return blob

    def pack(self, state, device):
        """state: mapping name -> tensor with the names of param_layout() (the reference module's state_dict)."""
        return self._pack(self._params(state, device), device)

    # ---- workspace
    def workspace_bytes(self, B, T):
        return int(self._fn("workspace_bytes")(self._h, int(B), int(T)))

    def _one_workspace(self, key, device, nbytes):
        ws = self._ws.get(key)
        if ws is None:
            self._ws.clear()      # one shape at a time: the caching allocator recycles the old block
            ws = torch.empty(nbytes(), dtype=torch.uint8, device=device)
            self._ws[key] = ws
        return ws

    def workspace(self, B, T, device):
        return self._one_workspace((int(B), int(T), str(device)), device, lambda: self.workspace_bytes(B, T))


class Plan(_Native):
    """Host-side plan of one score U-Net (mirrors GradLogPEstimator2d.__init__, diffusion.py:129-172)."""
    _family = "plan"

    def __init__(self, dim=64, n_feats=80, n_spks=1, spk_emb_dim=64, groups=8, pe_scale=1000.0, beta_min=0.05,
                 beta_max=20.0, precision=PREC_BF16X3, keep_intermediates=False, arch=0, dim_cond=128, use_ref_t=True,
                 c_dim=256, streams=None, conv_ws=None):
        """arch=0: Grad-TTS GradLogPEstimator2d; arch=1: DiffVC GradLogPEstimator (dim = dim_base).

        conv_ws: which kernel runs the wide Block 3x3 convolutions in bf16x3 (gtts_unet_cfg.conv_ws).  False: the uniform-wave
        kernel of conv_mfma.hip, which shares CUs with other streams' kernels.  True: the persistent wave-specialised kernel of
        conv_ws.hip -- 11 % faster per launch, but it owns every CU's registers while it runs.  None (default): True where these
        convolutions dominate (dim >= 128: the DiffVC decoder, +6 % end to end), False on the Grad-TTS dim-64 network, where a
        third of the call is bandwidth-bound kernels that three sub-batch streams hide under the convolutions of another
        sub-batch (measured on one box: 7.05 ms per U-Net call against 7.47 with the persistent kernel on two streams).

        precision PREC_F16F8 (the drop-in modules' default): the 128-channel-and-wider Block convolutions run the f16 + fp8 split on
        the persistent kernel (conv_ws defaults to True), unsplit -- measured on one box, ms per U-Net call at B = 16: 6.68 against
        7.16 for bf16x3 on three streams; with the persistent kernel two sub-batch streams are slower (6.80 vs 6.64), and sub-batch
        streams confined to disjoint halves of the CUs (hipExtStreamCreateWithCUMask) slower still (7.07; bf16x3: 7.70 vs 7.16).

        streams: number of sub-batches gtts_reverse_diffusion runs side by side on torch side streams owned by this
        object and registered with gtts_plan_set_streams (0 / 1: no split; $GTTS_STREAMS overrides the default).  Default 3;
        2 with conv_ws in bf16x3 (8 + 8 utterances fill the chip in whole rounds of persistent workgroups); 0 with PREC_F16F8."""
        if conv_ws is None:
            conv_ws = int(dim) >= 128 or int(precision) == PREC_F16F8
        conv_ws = bool(conv_ws) and int(precision) in (PREC_BF16X3, PREC_F16F8)
        self.conv_ws = conv_ws
        self.cfg = UnetCfg(int(dim), int(n_feats), int(n_spks), int(spk_emb_dim), int(groups), float(pe_scale),
                           float(beta_min), float(beta_max), int(precision), 1 if keep_intermediates else 0, int(arch),
                           int(dim_cond), 1 if use_ref_t else 0, int(c_dim), float(beta_min), float(beta_max),
                           1 if conv_ws else 0)
        self._open(dict(dim=dim, n_feats=n_feats, n_spks=n_spks, spk_emb_dim=spk_emb_dim, groups=groups, pe_scale=pe_scale,
                        beta_min=beta_min, beta_max=beta_max, precision=precision, keep_intermediates=keep_intermediates, arch=arch,
                        dim_cond=dim_cond, use_ref_t=use_ref_t, c_dim=c_dim, streams=streams, conv_ws=conv_ws),
                   ctypes.byref(self.cfg))
        if streams is None:
            streams = int(os.environ.get("GTTS_STREAMS", ("0" if int(precision) == PREC_F16F8 else "2") if conv_ws else "3"))
        self._nstreams = 0 if int(streams) < 2 else min(int(streams), 4)
        self._side = None           # (device, [torch.cuda.Stream])
        self._graph = False
        self._gstream = None
        self._stage = {}            # graph mode: persistent argument buffers (stable addresses -> graph cache hits)

    def set_graph(self, on=True):
        """hipGraph replay of whole reverse_diffusion calls (launch-bound small batches).  Inputs are copied into
        persistent buffers owned by this object so that every call presents the same addresses to the library."""
        _check(lib().gtts_plan_set_graph(self._h, 1 if on else 0), "gtts_plan_set_graph")
        self._graph = bool(on)
        self._stage = {}
        self._gstream = None        # capture / replay stream (stream capture is not allowed on the default stream)

    def _use_streams(self, device):
        """Register this plan's side streams for `device` (created once; they belong to this object)."""
        if self._nstreams < 2:
            return
        if self._side is not None and self._side[0] == device:
            return
        side = [torch.cuda.Stream(device=device) for _ in range(self._nstreams)]
        arr = (ctypes.c_void_p * len(side))(*[s.cuda_stream for s in side])
        _check(lib().gtts_plan_set_streams(self._h, arr, len(side)), "gtts_plan_set_streams")
        self._side = (device, side)
        self._ws.clear()            # the workspace size depends on the number of sub-batches

    def workspace_bytes(self, B, T):
        n = super().workspace_bytes(B, T)
        if n == 0:
            raise RuntimeError("gtts_workspace_bytes: %s" % lib().gtts_last_error().decode())
        return n

    def range_status(self, device=None):
        """(events, max |x|) of the activation range record of the last estimator / sampler call, as gtts_workspace_status counts
        them (gradtts_abi.h).  PREC_F16F8: staging lanes x launches that split an activation with |x| >= 1024, which keeps fp16-grade
        cross terms only.  Every precision: (samples x Block convolutions) whose GroupNorm statistics came out non-finite; max |x| is
        then inf.  (0, 0.0) before the first call.  Synchronises the current stream."""
        ws = None
        for key, w in self._ws.items():
            if device is None or key[-1] == str(device):
                ws = w
        if ws is None:
            return 0, 0.0
        n, mx = ctypes.c_uint(0), ctypes.c_float(0.0)
        _launch(ws.device, "gtts_workspace_status", ws, ctypes.byref(n), ctypes.byref(mx))
        return int(n.value), float(mx.value)

    # ---- weights
    def pack(self, state, device):
        """state: mapping name -> tensor with the estimator-level names of the reference state_dict.
        PREC_F16F8: raises RangeError when a 3x3 Block-convolution weight does not fit the format (|w| >= 63.97)."""
        params = self._params(state, device)
        half = self.cfg.dim // 2
        # exactly SinusoidalPosEmb's frequency table, computed on the host CPU like the reference (diffusion.py:121-122)
        freq = torch.exp(torch.arange(half).float() * -(math.log(10000) / (half - 1))).to(device)
        return self._pack(params, device, freq)

    # ---- GradLogPEstimator2d.forward
    def estimator_forward(self, blob, x, mask, mu, t, spk=None):
        x, mask, mu, t, spk = (_f32c(x, "x"), _f32c(mask, "mask"), _f32c(mu, "mu"), _f32c(t, "t"),
                               _f32c(spk, "spk"))
        B, F, T = x.shape
        if F != self.cfg.n_feats:
            raise RuntimeError("expected %d mel bins, got %d" % (self.cfg.n_feats, F))
        if mask.numel() != B * T or mu.shape != x.shape or t.numel() != B:
            raise RuntimeError("shape mismatch: x %s mask %s mu %s t %s" % (tuple(x.shape), tuple(mask.shape),
                                                                         tuple(mu.shape), tuple(t.shape)))
        out = torch.empty_like(x)
        ws = self.workspace(B, T, x.device)
        _launch(x.device, "gtts_estimator_forward", self._h, blob, x, mask, mu, t, spk, out, ws, ws.numel(), B, T)
        return out

    # ---- Diffusion.reverse_diffusion (whole loop)
    def reverse_diffusion(self, blob, z, mask, mu, n_timesteps, spk=None, noise=None):
        z, mask, mu, spk, noise = (_f32c(z, "z"), _f32c(mask, "mask"), _f32c(mu, "mu"), _f32c(spk, "spk"),
                                   _f32c(noise, "noise"))
        B, F, T = z.shape
        if F != self.cfg.n_feats:
            raise RuntimeError("expected %d mel bins, got %d" % (self.cfg.n_feats, F))
        if mask.numel() != B * T or mu.shape != z.shape:
            raise RuntimeError("shape mismatch: z %s mask %s mu %s" % (tuple(z.shape), tuple(mask.shape), tuple(mu.shape)))
        if noise is not None and tuple(noise.shape) != (int(n_timesteps), B, F, T):
            raise RuntimeError("noise must be [n_timesteps, B, F, T]")
        self._use_streams(z.device)
        ws = self.workspace(B, T, z.device)
        if self._graph:
            key = (B, T, str(z.device), spk is not None, None if noise is None else tuple(noise.shape))
            st = self._stage.get(key)
            if st is None:
                self._stage.clear()
                st = {"z": torch.empty_like(z), "mask": torch.empty_like(mask), "mu": torch.empty_like(mu),
                      "out": torch.empty_like(z), "spk": None if spk is None else torch.empty_like(spk),
                      "noise": None if noise is None else torch.empty_like(noise)}
                self._stage[key] = st
            for k, v in (("z", z), ("mask", mask), ("mu", mu), ("spk", spk), ("noise", noise)):
                if v is not None:
                    st[k].copy_(v)
            z, mask, mu, spk, noise, out = st["z"], st["mask"], st["mu"], st["spk"], st["noise"], st["out"]
        else:
            out = torch.empty_like(z)

        def run():          # on the stream that is current where it is called
            _launch(z.device, "gtts_reverse_diffusion", self._h, blob, z, mask, mu, spk, noise, out, ws, ws.numel(), B, T, int(n_timesteps),
                    0, int(n_timesteps))
        with torch.cuda.device(z.device):
            if not self._graph:
                run()
                return out
            cur = torch.cuda.current_stream()
            if self._gstream is None or self._gstream.device != z.device:
                self._gstream = torch.cuda.Stream(device=z.device)
            self._gstream.wait_stream(cur)
            with torch.cuda.stream(self._gstream):
                run()
            cur.wait_stream(self._gstream)
            return out.clone()

    # ---- DiffVC (arch=1)
    def vc_workspace(self, B, T, Tr, device):
        def nbytes():
            n = int(lib().gtts_vc_workspace_bytes(self._h, int(B), int(T), int(Tr)))
            if n == 0:
                raise RuntimeError("gtts_vc_workspace_bytes: %s" % lib().gtts_last_error().decode())
            return n
        return self._one_workspace(("vc", int(B), int(T), int(Tr), str(device)), device, nbytes)

    def vc_estimator_forward(self, blob, x, x_mask, mean, xt_ref, ref_mask, c, t):
        """DiffVC GradLogPEstimator.forward(x, x_mask, mean, ref, ref_mask, c, t) (DiffVC/model/diffusion.py:61-106)."""
        x, x_mask, mean, xt_ref, ref_mask, c, t = (_f32c(v, n) for v, n in (
            (x, "x"), (x_mask, "x_mask"), (mean, "mean"), (xt_ref, "ref"), (ref_mask, "ref_mask"), (c, "c"), (t, "t")))
        B, F, T = x.shape
        Tr = int(ref_mask.shape[-1]) if ref_mask is not None else T
        out = torch.empty_like(x)
        ws = self.vc_workspace(B, T, Tr, x.device)
        _launch(x.device, "gtts_vc_estimator_forward", self._h, blob, x, x_mask, mean, xt_ref, ref_mask, c, t, out, ws, ws.numel(), B, T, Tr)
        return out

    def vc_reverse_diffusion(self, blob, z, mask, mean, ref, ref_mask, mean_ref, c, n_timesteps, mode, noise=None,
                             noise_chunk_bytes=256 << 20):
        """DiffVC Diffusion.reverse_diffusion (DiffVC/model/diffusion.py:164-196); mode in {'pf','em','ml'}.

        noise (em / ml): a [n_timesteps, B, F, T] tensor, or a callable `draw(k)` returning the next k steps' N(0,1)
        draws as [k, B, F, T] -- then the loop runs in step ranges of at most noise_chunk_bytes of noise, so long
        schedules never hold more than one chunk (the reference holds one [B,F,T] draw at a time)."""
        modes = {"pf": 0, "em": 1, "ml": 2}
        if mode not in modes:
            raise RuntimeError("mode must be one of pf / em / ml")
        draw = noise if callable(noise) else None
        z, mask, mean, ref, ref_mask, mean_ref, c = (_f32c(v, n) for v, n in (
            (z, "z"), (mask, "mask"), (mean, "mean"), (ref, "ref"), (ref_mask, "ref_mask"), (mean_ref, "mean_ref"), (c, "c")))
        B, F, T = z.shape
        N = int(n_timesteps)
        Tr = int(ref_mask.shape[-1]) if ref_mask is not None else T
        if draw is None:
            noise = _f32c(noise, "noise")
            if mode != "pf" and (noise is None or tuple(noise.shape) != (N, B, F, T)):
                raise RuntimeError("em / ml sampling needs noise of shape [n_timesteps, B, F, T] (or a callable)")
        out = torch.empty_like(z)
        ws = self.vc_workspace(B, T, Tr, z.device)
        per = max(1, int(noise_chunk_bytes) // max(1, B * F * T * 4)) if (draw is not None and mode != "pf") else N
        with torch.cuda.device(z.device):
            i0 = 0
            while i0 < N:
                i1 = min(N, i0 + per)
                nz = None
                if mode != "pf":
                    nz = _f32c(draw(i1 - i0), "noise") if draw is not None else noise[i0:i1]
                    if tuple(nz.shape) != (i1 - i0, B, F, T):
                        raise RuntimeError("noise chunk must be [%d, B, F, T]" % (i1 - i0))
                _launch(z.device, "gtts_vc_reverse_diffusion", self._h, blob, z, mask, mean, ref, ref_mask, mean_ref, c, nz, out, ws,
                        ws.numel(), B, T, Tr, N, modes[mode], i0, i1)
                i0 = i1
        return out

    def vc_tensors(self, B, T, Tr, device):
        """Named intermediates of the last DiffVC estimator call (keep_intermediates plans); ref tensors use T_ref."""
        ws = self.vc_workspace(B, T, Tr, device)
        return ws, {name: (off, dims) for name, off, dims in self._tensor_infos("gtts_vc_tensor_info", B, T, Tr)}

    # ---- measurement (bench.py): per-op HIP-event timing
    def ops(self, B, T):
        """[(label, kernel, algorithmic flops, algorithmic bytes)] of the launches of one estimator call."""
        L = lib()
        out = []
        for k in range(L.gtts_plan_num_ops(self._h)):
            label, kern, fl, by = ctypes.c_char_p(), ctypes.c_char_p(), ctypes.c_double(), ctypes.c_double()
            _check(L.gtts_plan_op_info(self._h, k, int(B), int(T), ctypes.byref(label), ctypes.byref(kern),
                                       ctypes.byref(fl), ctypes.byref(by)), "gtts_plan_op_info")
            out.append((label.value.decode(), kern.value.decode(), fl.value, by.value))
        return out

    def profile(self, on):
        """on = True / 1: per-op durations (the sampler runs unsplit); on = 2: timeline mode (sub-batch streams stay on, see
        profile_timeline); False / 0: off."""
        _check(lib().gtts_profile_enable(self._h, 2 if on == 2 else (1 if on else 0)), "gtts_profile_enable")

    def profile_timeline(self, cap=1 << 18):
        """[(op index, stream index, start ms, end ms)] of every launch recorded in timeline mode; clears the record."""
        op, st = (ctypes.c_int * cap)(), (ctypes.c_int * cap)()
        t0, t1 = (ctypes.c_double * cap)(), (ctypes.c_double * cap)()
        n = ctypes.c_int(0)
        _check(lib().gtts_profile_timeline(self._h, cap, op, st, t0, t1, ctypes.byref(n)), "gtts_profile_timeline")
        return [(op[k], st[k], t0[k], t1[k]) for k in range(n.value)]

    def profile_collect(self):
        """(ms per op, launches per op) accumulated since profiling was enabled; clears the record."""
        n = lib().gtts_plan_num_ops(self._h)
        ms = (ctypes.c_double * n)()
        cnt = (ctypes.c_longlong * n)()
        _check(lib().gtts_profile_collect(self._h, ms, cnt), "gtts_profile_collect")
        return list(ms), list(cnt)

    # ---- debugging: named intermediates (keep_intermediates plans)
    def tensors(self, B, T, device):
        if int(self.cfg.precision) == PREC_BF16_STORE:
            raise RuntimeError("Plan.tensors(): the named-intermediate views are fp32; a keep_intermediates plan with bf16 "
                               "activation storage stores 2-byte activations -- use PREC_BF16 / PREC_BF16X3 for tap tests")
        ws = self.workspace(B, T, device)
        out = {}
        for name, off, dims in self._tensor_infos("gtts_plan_tensor_info", B, T):
            n = dims[0] * dims[1] * dims[2] * dims[3]
            if n > 0:
                out[name] = ws[off: off + 4 * n].view(torch.float32).view(*dims)
        return out

    def _tensor_infos(self, entry, *shape):
        """(name, workspace byte offset, dims [4]) of every named intermediate at `shape` = (B, T[, T_ref])."""
        info = getattr(lib(), entry)
        for k in range(lib().gtts_plan_num_tensors(self._h)):
            name, off, dims = ctypes.c_char_p(), ctypes.c_size_t(), (ctypes.c_int * 4)()
            _check(info(self._h, k, *[int(v) for v in shape], ctypes.byref(name), ctypes.byref(off), ctypes.byref(dims)), entry)
            yield name.value.decode(), off.value, tuple(dims)


class Vocoder(_Native):
    """HiFi-GAN generator on the HIP kernels (csrc/voc.hip): Generator(h).forward of Grad-TTS/hifi-gan/models.py:77-120."""
    _family = "voc"

    def __init__(self, upsample_rates=(8, 8, 2, 2), upsample_kernel_sizes=(16, 16, 4, 4), upsample_initial_channel=512,
                 resblock_kernel_sizes=(3, 7, 11), resblock_dilation_sizes=((1, 3, 5), (1, 3, 5), (1, 3, 5)), resblock="1",
                 n_mels=80):
        cfg = VocCfg()
        cfg.n_mels = int(n_mels)
        cfg.upsample_initial_channel = int(upsample_initial_channel)
        cfg.n_ups = len(upsample_rates)
        cfg.n_kernels = len(resblock_kernel_sizes)
        cfg.resblock_type = int(resblock)
        if cfg.n_ups > 8 or cfg.n_kernels > 8:
            raise RuntimeError("at most 8 upsamplers / ResBlock kernels")
        for k, (u, ks) in enumerate(zip(upsample_rates, upsample_kernel_sizes)):
            cfg.upsample_rates[k] = int(u)
            cfg.upsample_kernel_sizes[k] = int(ks)
        want = 3 if str(resblock) == "1" else 2       # ResBlock1 walks three dilations, ResBlock2 two (models.py:11-74)
        for k, (ks, dil) in enumerate(zip(resblock_kernel_sizes, resblock_dilation_sizes)):
            cfg.resblock_kernel_sizes[k] = int(ks)
            if len(dil) != want:
                raise RuntimeError("resblock_dilation_sizes[%d] has %d entries; the HIP ResBlock%s runs exactly %d (the torch "
                                   "module would accept any count, the kernel does not)" % (k, len(dil), resblock, want))
            for j in range(3):
                cfg.resblock_dilations[k][j] = int(dil[j]) if j < len(dil) else 1
        self.cfg = cfg
        self._open(dict(upsample_rates=tuple(upsample_rates), upsample_kernel_sizes=tuple(upsample_kernel_sizes),
                        upsample_initial_channel=int(upsample_initial_channel), resblock_kernel_sizes=tuple(resblock_kernel_sizes),
                        resblock_dilation_sizes=tuple(tuple(d) for d in resblock_dilation_sizes), resblock=str(resblock),
                        n_mels=int(n_mels)), ctypes.byref(cfg))
        self.hop = int(lib().gtts_voc_hop(self._h))

    @classmethod
    def from_config(cls, h):
        """h: the AttrDict of hifigan-config.json (Grad-TTS/inference.py:57-59)."""
        return cls(h["upsample_rates"], h["upsample_kernel_sizes"], h["upsample_initial_channel"],
                   h["resblock_kernel_sizes"], h["resblock_dilation_sizes"], h["resblock"], h.get("num_mels", 80))

    def pack(self, state, device):
        """state: name -> tensor with weight normalisation folded (`<module>.weight`, `<module>.bias`)."""
        return self._pack(self._params(state, device, " (call remove_weight_norm() or fold weight_g / weight_v)"), device)

    def forward(self, blob, mel):
        mel = _f32c(mel, "mel")
        B, F, T = mel.shape
        if F != self.cfg.n_mels:
            raise RuntimeError("expected %d mel bins, got %d" % (self.cfg.n_mels, F))
        ws = self.workspace(B, T, mel.device)
        wav = torch.empty((B, 1, T * self.hop), dtype=torch.float32, device=mel.device)
        self._launch(mel.device, "forward", blob, mel, wav, ws, ws.numel(), B, T)
        return wav


class Conv1dOp(_Native):
    """One layer of the shared 1-D convolution kernel (csrc/conv1d.h) -- the kernel of every dense layer of the vocoder and of both
    encoders -- for its per-layer tests.  mode 0: Conv1d(cin, cout, K, dilation, 'same' padding); mode 1: ConvTranspose1d(cin, cout,
    K = 2 S, stride S, padding S / 2).  The handle has no parameters of its own: pack() takes the reference module's weight."""
    _family = "conv1d"

    def __init__(self, mode, cin, cout, K, dilation=1, S=1):
        self.mode, self.cin, self.cout, self.K, self.S = int(mode), int(cin), int(cout), int(K), int(S)
        kw = dict(mode=int(mode), cin=int(cin), cout=int(cout), K=int(K), dilation=int(dilation), S=int(S))
        self._open(kw, *[kw[k] for k in ("mode", "cin", "cout", "K", "dilation", "S")])

    def instance(self, B, Lin, res=False, accmode=0, out_mask=False):
        """(MT, TPS, AITER, KCH, epilogue) of the kernel instance forward() launches at this shape (a host call; epilogue 0: buffer
        descriptors, 1 / 2: ConvTranspose1d 16-byte / two 8-byte stores, 3: generic); raises where forward() would refuse."""
        info = (ctypes.c_int * 5)()
        self._call("instance", self._h, int(B), int(Lin), int(bool(res)), int(accmode), int(bool(out_mask)), ctypes.byref(info))
        return tuple(info)

    def pack(self, weight, device):
        """weight: Conv1d [cout, cin, K] / ConvTranspose1d [cin, cout, K]."""
        want = (self.cout, self.cin, self.K) if self.mode == 0 else (self.cin, self.cout, self.K)
        if tuple(weight.shape) != want:
            raise RuntimeError("weight has shape %s, expected %s" % (tuple(weight.shape), want))
        w = weight.detach().to(device=device, dtype=torch.float32).contiguous()
        if not w.is_cuda:
            raise RuntimeError("the weights are packed for a HIP device (got %s)" % w.device)
        blob = torch.empty(self.packed_bytes(), dtype=torch.uint8, device=w.device)
        self._launch(w.device, "pack", w, blob)
        torch.cuda.current_stream(w.device).synchronize()
        return blob

    def _pack_source(self, weight, blob, shape):
        """What the unsynchronised packs take: the weight as it is (contiguous fp32 on a HIP device, no temporary copy that could die
        before the launch runs) and a blob of packed_bytes() on its device (made here when None)."""
        if tuple(weight.shape) != shape:
            raise RuntimeError("weight has shape %s, expected %s" % (tuple(weight.shape), shape))
        if not weight.is_cuda or weight.dtype != torch.float32 or not weight.is_contiguous():
            raise RuntimeError("weight must be a contiguous fp32 tensor on a HIP device")
        if blob is None:
            blob = torch.empty(self.packed_bytes(), dtype=torch.uint8, device=weight.device)
        elif blob.device != weight.device or blob.dtype != torch.uint8 or blob.numel() < self.packed_bytes() or not blob.is_contiguous():
            raise RuntimeError("blob must hold packed_bytes() = %d bytes on %s" % (self.packed_bytes(), weight.device))
        return blob

    def pack_into(self, weight, blob=None):
        """pack() on the current stream WITHOUT a synchronise (the training path): weight [cout, cin, K] as it is, into `blob`."""
        if self.mode != 0:
            raise RuntimeError("pack_into serves Conv1d (mode 0) handles")
        blob = self._pack_source(weight, blob, (self.cout, self.cin, self.K))
        self._launch(weight.device, "pack", weight, blob)
        return blob

    def pack_dgrad(self, weight, blob=None):
        """On the TRANSPOSED handle Conv1dOp(0, cout, cin, K, dilation): packs the forward module's weight [cout, cin, K] = [self.cin,
        self.cout, K] as W'[ci][co][t] = W[co][ci][K-1-t], one launch, no synchronise.  forward() of this handle on dy is then the data
        gradient (in_mask = the forward's output mask, out_mask = its input mask, a zero bias)."""
        blob = self._pack_source(weight, blob, (self.cin, self.cout, self.K))
        self._launch(weight.device, "pack_dgrad", weight, blob)
        return blob

    def wgrad_info(self, B, L):
        """(tile rows, tile columns, positions per chunk, slices, chunks per slice, empty slices) of wgrad() at this shape: a host call."""
        info = (ctypes.c_int * 6)()
        self._call("wgrad_info", self._h, int(B), int(L), ctypes.byref(info))
        return tuple(info)

    def wgrad_workspace_bytes(self, B, L):
        n = int(self._fn("wgrad_workspace_bytes")(self._h, int(B), int(L)))
        if n == 0:
            raise RuntimeError("gtts_conv1d_wgrad_workspace_bytes refused: %s" % lib().gtts_last_error().decode())
        return n

    def wgrad(self, x, dy, in_mask=None, out_mask=None, want_bias=True, dw=None, db=None, workspace=None):
        """(dw [cout, cin, K], db [cout] or None) of the layer y = (conv(x * in_mask) + bias) * out_mask for x [B, cin, L], dy [B, cout, L],
        masks [B, L] or None.  Contiguous fp32 tensors on x's HIP device, passed as they are; dw / db / workspace are made when None."""
        if not x.is_cuda:
            raise RuntimeError("x must live on a HIP device (got %s); there is no CPU fallback" % x.device)
        B, cin, L = x.shape
        if cin != self.cin:
            raise RuntimeError("expected %d input channels, got %d" % (self.cin, cin))
        if dw is None:
            dw = torch.empty((self.cout, self.cin, self.K), dtype=torch.float32, device=x.device)
        if db is None and want_bias:
            db = torch.empty((self.cout,), dtype=torch.float32, device=x.device)
        _enc_in("Conv1dOp.wgrad", x.device, ("x", x, (B, cin, L), False), ("dy", dy, (B, self.cout, L), False), ("in_mask", in_mask, (B, L), True),
                ("out_mask", out_mask, (B, L), True), ("dw", dw, (self.cout, self.cin, self.K), False), ("db", db, (self.cout,), True))
        if workspace is None:
            workspace = torch.empty(self.wgrad_workspace_bytes(B, L), dtype=torch.uint8, device=x.device)
        elif workspace.device != x.device or not workspace.is_contiguous():
            raise RuntimeError("workspace must be a contiguous tensor on %s" % x.device)
        self._launch(x.device, "wgrad", x, in_mask, dy, out_mask, dw, db, workspace, workspace.numel() * workspace.element_size(), B, L)
        return dw, db

    def forward(self, blob, bias, x, out=None, res=None, accsrc=None, accmode=0, div=1.0, slope=1.0, in_mask=None, out_mask=None):
        """x [B, cin, Lin] -> [B, cout, Lin * S] (written into `out` when given).  Every tensor must be contiguous fp32 on x's HIP
        device: views into larger allocations are passed as they are, nothing is copied."""
        if not x.is_cuda:
            raise RuntimeError("x must live on a HIP device (got %s); there is no CPU fallback" % x.device)
        B, cin, Lin = x.shape
        if cin != self.cin:
            raise RuntimeError("expected %d input channels, got %d" % (self.cin, cin))
        if out is None:
            out = torch.empty((B, self.cout, Lin * self.S), dtype=torch.float32, device=x.device)
        shapes = {"bias": (self.cout,), "out": (B, self.cout, Lin * self.S), "res": (B, self.cout, Lin * self.S),
                  "accsrc": (B, self.cout, Lin * self.S), "in_mask": (B, Lin), "out_mask": (B, Lin * self.S)}
        given = {"x": x, "bias": bias, "out": out, "res": res, "accsrc": accsrc, "in_mask": in_mask, "out_mask": out_mask}
        for name, t in given.items():
            if t is None:
                continue
            if t.device != x.device or t.dtype != torch.float32 or not t.is_contiguous():
                raise RuntimeError("%s must be a contiguous fp32 tensor on %s" % (name, x.device))
            if name in shapes and tuple(t.shape) != shapes[name]:
                raise RuntimeError("%s has shape %s, expected %s" % (name, tuple(t.shape), shapes[name]))
        self._launch(x.device, "forward", blob, bias, x, out, res, accsrc, int(accmode), float(div), float(slope), in_mask, out_mask, B, Lin)
        return out


class Encoder(_Native):
    """Grad-TTS TextEncoder (mode 'text') / DiffVC MelEncoder (mode 'mel') on the HIP kernels (csrc/enc.hip)."""
    _family = "enc"

    def __init__(self, mode="text", n_vocab=149, n_feats=80, channels=192, filter_channels=768, filter_channels_dp=256,
                 n_heads=2, n_layers=6, kernel_size=3, window_size=4):
        self.mode = mode
        self.cfg = EncCfg({"text": 0, "mel": 1}[mode], int(n_vocab), int(n_feats), int(channels), int(filter_channels),
                          int(filter_channels_dp), int(n_heads), int(n_layers), int(kernel_size), int(window_size or 0))
        self._open(dict(mode=mode, n_vocab=n_vocab, n_feats=n_feats, channels=channels, filter_channels=filter_channels,
                        filter_channels_dp=filter_channels_dp, n_heads=n_heads, n_layers=n_layers, kernel_size=kernel_size,
                        window_size=window_size), ctypes.byref(self.cfg))

    def attention_path(self, L):
        """Which attention kernel forward() runs at sequence length L: 16 (16 queries per workgroup), 8 (the 8-query kernel: long
        sequences, windows above 7, head widths not divisible by 4) or 0 (forward() refuses L: no kernel holds its probabilities)."""
        return int(lib().gtts_enc_attention_path(self._h, int(L)))

    def forward(self, blob, x, x_mask):
        """text: x = ids [B,L] int64 -> (mu [B,n_feats,L], logw [B,1,L]);  mel: x = mel [B,n_feats,L] -> [B,n_feats,L].
        x_mask [B,1,L] or [B,L] float."""
        if not x.is_cuda:
            raise RuntimeError("the encoder kernels need HIP tensors (got %s); there is no CPU fallback here" % x.device)
        m = _f32c(x_mask, "x_mask")
        if self.mode == "text":
            ids = x.to(torch.int64).contiguous()
            B, L = ids.shape
            mel = None
        else:
            mel = _f32c(x, "mel")
            B, _, L = mel.shape
            ids = None
        if m.numel() != B * L:
            raise RuntimeError("x_mask must have B*L elements")
        dev = x.device
        mu = torch.empty((B, self.cfg.n_feats, L), dtype=torch.float32, device=dev)
        logw = torch.empty((B, 1, L), dtype=torch.float32, device=dev) if self.mode == "text" else None
        ws = self.workspace(B, L, dev)
        self._launch(dev, "forward", blob, ids, mel, m, mu, logw, ws, ws.numel(), B, L)
        return (mu, logw) if self.mode == "text" else mu


def enc_attention_path(channels, n_heads, window, L):
    """Which attention kernel an encoder of these channels, heads and window runs at length L (16, 8, or 0: refused) -- a host
    call, the decision of Encoder.attention_path without a handle."""
    return int(lib().gtts_enc_attention_path_for(int(channels), int(n_heads), int(window or 0), int(L)))


def _enc_in(op, dev, *args):
    """_in in its strict mode for (name, tensor, shape, optional) of a stand-alone encoder op: views into larger allocations are
    passed as they are, nothing is converted or copied."""
    for name, t, shape, optional in args:
        _in(op, name, t, shape, dev, True, optional)


def enc_layernorm(a, gamma, beta, bres=None, a_mask=None, out_mask=None, eps=1e-4, relu_in=False, relu_out=False, out=None):
    """The encoders' LayerNorm kernel on its own: relu_out?(LN_c(relu_in?(a) * a_mask + bres)) * out_mask.  a, bres [B,C,L]; gamma,
    beta [C]; masks [B,L]; written into `out` when given.  The launch gtts_enc_forward makes, for the per-op tests."""
    op = "enc_layernorm"
    _in(op, "a", a, strict=True)
    dev, (B, C, L) = a.device, a.shape
    _enc_in(op, dev, ("bres", bres, (B, C, L), True), ("gamma", gamma, (C,), False), ("beta", beta, (C,), False),
            ("a_mask", a_mask, (B, L), True), ("out_mask", out_mask, (B, L), True))
    out = _out(op, out, "out", (B, C, L), dev)
    _launch(dev, "gtts_enc_layernorm", a, bres, gamma, beta, a_mask, out_mask, out, B, C, L, float(eps), int(bool(relu_in)),
            int(bool(relu_out)))
    return out


def enc_attention(q, k, v, mask, emb_rel_k=None, emb_rel_v=None, n_heads=2, window=0, path=0, out=None):
    """The encoders' windowed relative-position attention kernel on its own: q, k, v [B,C,L], mask [B,L], emb_rel_k / emb_rel_v
    [2 window + 1, C / n_heads] (window 0: none) -> [B,C,L].  path 0: the kernel Encoder.forward would run; 16 / 8: that kernel
    (refused where it cannot serve the shape).  The launch gtts_enc_forward makes, for the per-op tests."""
    op = "enc_attention"
    _in(op, "q", q, strict=True)
    dev, (B, C, L) = q.device, q.shape
    window = int(window or 0)
    rel = (2 * window + 1, C // max(int(n_heads), 1))
    _enc_in(op, dev, ("k", k, (B, C, L), False), ("v", v, (B, C, L), False), ("mask", mask, (B, L), False),
            ("emb_rel_k", emb_rel_k, rel, not window), ("emb_rel_v", emb_rel_v, rel, not window))
    out = _out(op, out, "out", (B, C, L), dev)
    _launch(dev, "gtts_enc_attention", q, k, v, mask, emb_rel_k, emb_rel_v, out, B, C, L, int(n_heads), window, int(path))
    return out


# ---- training of the two ops (csrc/enc_train.hip)
def enc_attention_train_ok(channels, n_heads, window, L):
    """Whether the training attention kernels hold this shape (a host call): 1 / 0."""
    return int(lib().gtts_enc_attention_train_ok(int(channels), int(n_heads), int(window or 0), int(L)))


def _att_train_in(op, q, k, v, mask, emb_rel_k, emb_rel_v, drop, n_heads, window):
    """The inputs the two training attention calls share, checked: (device, B, C, L, H, shape of the relative embeddings)."""
    _in(op, "q", q, strict=True)
    dev, (B, C, L), H = q.device, q.shape, max(int(n_heads), 1)
    rel = (2 * window + 1, C // H)
    _enc_in(op, dev, ("k", k, (B, C, L), False), ("v", v, (B, C, L), False), ("mask", mask, (B, L), False),
            ("emb_rel_k", emb_rel_k, rel, not window), ("emb_rel_v", emb_rel_v, rel, not window), ("drop", drop, (B, H, L, L), True))
    return dev, B, C, L, H, rel


def enc_attention_train_forward(q, k, v, mask, emb_rel_k=None, emb_rel_v=None, drop=None, n_heads=2, window=0, out=None, stat=None):
    """enc_attention for training: `drop` [B,H,L,L] (0 or 1 / (1 - p)) multiplies the probabilities after the softmax; returns
    (out [B,C,L], stat [B,H,L,2]: each query row's score maximum and reciprocal exponential sum, what the backward recomputes from)."""
    op, window = "enc_attention_train_forward", int(window or 0)
    dev, B, C, L, H, _ = _att_train_in(op, q, k, v, mask, emb_rel_k, emb_rel_v, drop, n_heads, window)
    out, stat = _out(op, out, "out", (B, C, L), dev), _out(op, stat, "stat", (B, H, L, 2), dev)
    _launch(dev, "gtts_enc_attention_train_forward", q, k, v, mask, emb_rel_k, emb_rel_v, drop, out, stat, B, C, L, int(n_heads), window)
    return out, stat


def enc_attention_train_backward(q, k, v, mask, emb_rel_k, emb_rel_v, drop, stat, dout, n_heads=2, window=0, grads=None):
    """(dq, dk, dv, dek, dev) of enc_attention_train_forward from its inputs, `drop` and `stat` (dek = dev = None without a window).
    grads: optional dict of preallocated outputs by those names."""
    op, window = "enc_attention_train_backward", int(window or 0)
    dev, B, C, L, H, rel = _att_train_in(op, q, k, v, mask, emb_rel_k, emb_rel_v, drop, n_heads, window)
    _enc_in(op, dev, ("stat", stat, (B, H, L, 2), False), ("dout", dout, (B, C, L), False))
    g = grads or {}
    dq, dk, dv = (_out(op, g, n, (B, C, L), dev) for n in ("dq", "dk", "dv"))
    dek, dev_ = (_out(op, g, n, rel, dev) for n in ("dek", "dev")) if window else (None, None)
    need = int(lib().gtts_enc_attention_train_scratch_bytes(B, C, L, int(n_heads), window))
    scratch = torch.empty(max(need, 4) // 4, dtype=torch.float32, device=dev)
    _launch(dev, "gtts_enc_attention_train_backward", q, k, v, mask, emb_rel_k, emb_rel_v, drop, stat, dout, dq, dk, dv, dek, dev_, scratch,
            B, C, L, int(n_heads), window)
    return dq, dk, dv, dek, dev_


def enc_layernorm_backward(dout, a, gamma, beta, bres=None, a_mask=None, out_mask=None, eps=1e-4, relu_in=False, relu_out=False,
                           grads=None):
    """(da, dbres, dgamma, dbeta) of enc_layernorm (dbres None without bres).  grads: optional dict of preallocated outputs."""
    op = "enc_layernorm_backward"
    _in(op, "a", a, strict=True)
    dev, (B, C, L) = a.device, a.shape
    _enc_in(op, dev, ("dout", dout, (B, C, L), False), ("bres", bres, (B, C, L), True), ("gamma", gamma, (C,), False),
            ("beta", beta, (C,), False), ("a_mask", a_mask, (B, L), True), ("out_mask", out_mask, (B, L), True))
    g = grads or {}
    da, dgamma, dbeta = _out(op, g, "da", (B, C, L), dev), _out(op, g, "dgamma", (C,), dev), _out(op, g, "dbeta", (C,), dev)
    dbres = _out(op, g, "dbres", (B, C, L), dev) if bres is not None else None
    need = int(lib().gtts_enc_layernorm_backward_scratch_floats(B, C, L))
    scratch = torch.empty(max(need, 1), dtype=torch.float32, device=dev)
    _launch(dev, "gtts_enc_layernorm_backward", dout, a, bres, gamma, beta, a_mask, out_mask, da, dbres, dgamma, dbeta, scratch, B, C, L,
            float(eps), int(bool(relu_in)), int(bool(relu_out)))
    return da, dbres, dgamma, dbeta


class PostNetPlan(_Native):
    """DiffVC PostNet (DiffVC/model/postnet.py:40-53) on the HIP kernels (csrc/postnet.hip)."""
    _family = "postnet"

    def __init__(self, dim=128, n_feats=80, groups=8):
        self.dim, self.n_feats = int(dim), int(n_feats)
        self._open(dict(dim=int(dim), n_feats=int(n_feats), groups=int(groups)), int(dim), int(n_feats), int(groups))

    def forward(self, blob, x, mask):
        """x [B,n_feats,T], mask [B,1,T] -> [B,n_feats,T]."""
        x, mask = _f32c(x, "x"), _f32c(mask, "mask")
        B, F, T = x.shape
        if F != self.n_feats or mask.numel() != B * T:
            raise RuntimeError("shape mismatch: x %s mask %s" % (tuple(x.shape), tuple(mask.shape)))
        ws = self.workspace(B, T, x.device)
        out = torch.empty_like(x)
        self._launch(x.device, "forward", blob, x, mask, out, ws, ws.numel(), B, T)
        return out


class MelPlan(_Native):
    """Log-mel front end on the HIP kernel (csrc/mel.hip): mel_spectrogram(..., center=False) of Grad-TTS/hifi-gan/meldataset.py:51-74.
    The handle has no parameters: its blob holds the window, the twiddles and the filterbank, computed on the host in float64."""
    _family = "mel"

    def __init__(self, n_fft=1024, num_mels=80, sampling_rate=22050, hop_size=256, win_size=1024, fmin=0.0, fmax=8000.0):
        self.cfg = MelCfg(int(n_fft), int(num_mels), int(sampling_rate), int(hop_size), int(win_size), float(fmin), float(fmax))
        self.n_fft, self.num_mels, self.hop_size = int(n_fft), int(num_mels), int(hop_size)
        self.pad = (self.n_fft - self.hop_size) // 2
        self._open(dict(n_fft=int(n_fft), num_mels=int(num_mels), sampling_rate=int(sampling_rate), hop_size=int(hop_size),
                        win_size=int(win_size), fmin=float(fmin), fmax=float(fmax)), ctypes.byref(self.cfg))

    def frames(self, L):
        """T for rows of L samples; raises when L <= (n_fft - hop_size) / 2 (no reflection) or no whole frame fits."""
        T = int(self._fn("frames")(self._h, int(L)))
        if T < 0:
            _check(T, "gtts_mel_frames")
        return T

    def filterbank(self):
        """W [num_mels, n_fft / 2 + 1] fp32 on the CPU (a host call: no device is touched)."""
        W = torch.empty((self.num_mels, self.n_fft // 2 + 1), dtype=torch.float32)
        self._call("filterbank", self._h, _ptr(W))
        return W

    def pack(self, device):
        blob = torch.empty(self.packed_bytes(), dtype=torch.uint8, device=device)
        if not blob.is_cuda:
            raise RuntimeError("the mel tables are packed for a HIP device (got %s)" % blob.device)
        self._launch(blob.device, "pack", blob)
        torch.cuda.current_stream(blob.device).synchronize()
        return blob

    def forward(self, blob, y, lengths=None):
        """y [B, L] -> log-mel [B, num_mels, frames(L)] in one launch; lengths: optional [B] ints on y's device -- row b is the
        utterance y[b, :lengths[b]], frames beyond its own count are 0."""
        y = _f32c(y, "y")
        if y.dim() != 2:
            raise RuntimeError("y must be [B, L] (got %s)" % (tuple(y.shape),))
        B, L = y.shape
        if lengths is not None:
            if not torch.is_tensor(lengths) or lengths.device != y.device or lengths.numel() != B:
                raise RuntimeError("lengths must be a [B] integer tensor on y's HIP device")
            lengths = lengths.to(torch.int32).contiguous()
        out = torch.empty((B, self.num_mels, self.frames(L)), dtype=torch.float32, device=y.device)
        self._launch(y.device, "forward", blob, y, lengths, out, B, L)
        return out

    def backward_workspace_bytes(self, B, L):
        """Bytes of the windowed frame gradients [B, frames(L), n_fft] the backward writes between its two launches."""
        self.frames(L)
        return int(self._fn("backward_workspace_bytes")(self._h, int(B), int(L)))

    def backward(self, blob, y, dmel, lengths=None):
        """The input gradient of forward (csrc/mel_train.hip): y [B, L], dmel [B, num_mels, frames(L)] -> dwav [B, L] fp32; the same
        lengths as the forward's (gradient 0 at and beyond a row's length).  No floating-point atomics: two calls give the same bits."""
        if y.dim() != 2:
            raise RuntimeError("y must be [B, L] (got %s)" % (tuple(y.shape),))
        B, L = y.shape
        if dmel.device != y.device or tuple(dmel.shape) != (B, self.num_mels, self.frames(L)):
            raise RuntimeError("dmel must be [%d, %d, %d] on y's device (got %s on %s)" %
                               (B, self.num_mels, self.frames(L), tuple(dmel.shape), dmel.device))
        y, dmel = _f32c(y, "y"), _f32c(dmel, "dmel")
        if lengths is not None:
            if not torch.is_tensor(lengths) or lengths.device != y.device or lengths.numel() != B:
                raise RuntimeError("lengths must be a [B] integer tensor on y's HIP device")
            lengths = lengths.to(torch.int32).contiguous()
        ws = torch.empty(self.backward_workspace_bytes(B, L), dtype=torch.uint8, device=y.device)
        dwav = torch.empty((B, L), dtype=torch.float32, device=y.device)
        self._launch(y.device, "backward", blob, y, lengths, dmel, dwav, ws, ws.numel(), B, L)
        return dwav


class FglPlan(_Native):
    """Fast Griffin-Lim on the HIP kernels (csrc/fgl.hip): FastGL of DiffVC/model/utils.py:42-110, log-mel [B, n_mels, T] -> waveform
    [B, hop_size (T - 1)].  The handle has no parameters of its own: its blob holds the window, the twiddles and the caller's
    pseudo-inverse of the mel filterbank."""
    _family = "fgl"

    def __init__(self, n_fft=1024, n_mels=80, hop_size=256, momentum=0.99):
        self.cfg = FglCfg(int(n_fft), int(n_mels), int(hop_size), float(momentum))
        self.n_fft, self.n_mels, self.hop_size, self.momentum = int(n_fft), int(n_mels), int(hop_size), float(momentum)
        self.bins = self.n_fft // 2 + 1
        self._open(dict(n_fft=int(n_fft), n_mels=int(n_mels), hop_size=int(hop_size), momentum=float(momentum)), ctypes.byref(self.cfg))

    def samples(self, T):
        """L = hop_size (T - 1) for mels of T frames; raises when that is <= n_fft / 2 (no reflection), naming the smallest T."""
        L = int(self._fn("samples")(self._h, int(T)))
        if L < 0:
            _check(L, "gtts_fgl_samples")
        return L

    def pack(self, inv_basis, device):
        """inv_basis: the pseudo-inverse of the mel filterbank, [n_fft / 2 + 1, n_mels] (any device; it is read on the host)."""
        P = inv_basis.detach().to(device="cpu", dtype=torch.float32).contiguous()
        if tuple(P.shape) != (self.bins, self.n_mels):
            raise RuntimeError("inv_basis must be [%d, %d] (got %s)" % (self.bins, self.n_mels, tuple(P.shape)))
        blob = torch.empty(self.packed_bytes(), dtype=torch.uint8, device=device)
        if not blob.is_cuda:
            raise RuntimeError("the Griffin-Lim tables are packed for a HIP device (got %s)" % blob.device)
        self._launch(blob.device, "pack", P, blob)
        return blob

    def _mel(self, s):
        s = _f32c(s, "logmel")
        if s.dim() != 3 or s.shape[1] != self.n_mels:
            raise RuntimeError("logmel must be [B, %d, T] (got %s)" % (self.n_mels, tuple(s.shape)))
        return s, int(s.shape[0]), int(s.shape[2]), self.samples(s.shape[2])

    def init(self, blob, s):
        """logmel [B, n_mels, T] -> (c [B, K, T], x0 [B, L])."""
        s, B, T, L = self._mel(s)
        ws = self.workspace(B, T, s.device)
        c = torch.empty((B, self.bins, T), dtype=torch.float32, device=s.device)
        x0 = torch.empty((B, L), dtype=torch.float32, device=s.device)
        self._launch(s.device, "init", blob, s, c, x0, ws, ws.numel(), B, T)
        return c, x0

    def step(self, blob, c, x, a_prev):
        """One iteration: c [B, K, T], x [B, L], a_prev complex64 [B, K, T] -> (x_out [B, L], a complex64 [B, K, T])."""
        c, x = _f32c(c, "c"), _f32c(x, "x")
        if c.dim() != 3 or c.shape[1] != self.bins:
            raise RuntimeError("c must be [B, %d, T] (got %s)" % (self.bins, tuple(c.shape)))
        B, _, T = c.shape
        L = self.samples(T)
        if tuple(x.shape) != (B, L):
            raise RuntimeError("x must be [%d, %d] (got %s)" % (B, L, tuple(x.shape)))
        if not a_prev.is_cuda or a_prev.dtype != torch.complex64 or tuple(a_prev.shape) != tuple(c.shape):
            raise RuntimeError("a_prev must be a complex64 %s on the HIP device (got %s %s on %s)" %
                               (tuple(c.shape), a_prev.dtype, tuple(a_prev.shape), a_prev.device))
        a_prev = a_prev.contiguous()
        ws = self.workspace(B, T, c.device)
        x_out, a = torch.empty_like(x), torch.empty_like(a_prev)
        self._launch(c.device, "step", blob, c, x, a_prev, x_out, a, ws, ws.numel(), B, T)
        return x_out, a

    def forward(self, blob, s, n_iters=32):
        """logmel [B, n_mels, T] -> waveform [B, L] after n_iters iterations, one launch each (n_iters = 0: the initial reconstruction)."""
        s, B, T, L = self._mel(s)
        ws = self.workspace(B, T, s.device)
        wav = torch.empty((B, L), dtype=torch.float32, device=s.device)
        self._launch(s.device, "forward", blob, s, wav, ws, ws.numel(), B, T, int(n_iters))
        return wav


class WavPlan(_Native):
    """Waveform front end of the DiffVC speaker encoder on the HIP kernels (csrc/wav.hip): the batch functions of
    DiffVC/speaker_encoder/encoder/audio.py -- torchaudio's default Resample, normalize_volume_batch, the 40-band power mel
    [B, T, n_mels] that SpkPlan.forward reads.  The handle has no parameters: its blob holds the resampling taps, the windowed DFT table
    and the filterbank, computed on the host in float64."""
    _family = "wav"

    def __init__(self, source_sr=22050, sampling_rate=16000, n_fft=400, hop_size=160, n_mels=40, lowpass_filter_width=6, rolloff=0.99,
                 fmin=0.0, fmax=8000.0):
        kw = dict(source_sr=int(source_sr), sampling_rate=int(sampling_rate), n_fft=int(n_fft), hop_size=int(hop_size),
                  n_mels=int(n_mels), lowpass_filter_width=int(lowpass_filter_width), rolloff=float(rolloff), fmin=float(fmin),
                  fmax=float(fmax))
        self.cfg = WavCfg(*kw.values())
        self.source_sr, self.sampling_rate, self.n_fft, self.hop_size, self.n_mels = list(kw.values())[:5]
        self._open(kw, ctypes.byref(self.cfg))

    def _count(self, op, L):
        v = int(self._fn(op)(self._h, int(L)))
        if v < 0:
            _check(v, _sym(self._family, op))
        return v

    def resampled_length(self, L):
        """ceil(n L / o) for the reduced rates o -> n; raises on L < 1."""
        return self._count("resampled_length", L)

    def frames(self, L):
        """T = 1 + L // hop_size; raises when L <= n_fft / 2 (no reflection)."""
        return self._count("frames", L)

    def tiles(self, L):
        """Tile sums of squares per row of L samples (what resample leaves and normalize takes)."""
        return self._count("tiles", L)

    def taps(self):
        """(first [n] int32, taps [n, span] fp32) on the CPU: the taps the kernel keeps of every phase (a host call)."""
        n = self.sampling_rate // math.gcd(self.source_sr, self.sampling_rate)
        first = torch.empty(n, dtype=torch.int32)
        taps = torch.empty((n, int(self._fn("span")(self._h))), dtype=torch.float32)
        self._call("taps", self._h, _ptr(first), _ptr(taps))
        return first, taps

    def filterbank(self):
        """W [n_mels, n_fft / 2 + 1] fp32 on the CPU (a host call: no device is touched)."""
        W = torch.empty((self.n_mels, self.n_fft // 2 + 1), dtype=torch.float32)
        self._call("filterbank", self._h, _ptr(W))
        return W

    def pack(self, device):
        blob = torch.empty(self.packed_bytes(), dtype=torch.uint8, device=device)
        if not blob.is_cuda:
            raise RuntimeError("the waveform front end's tables are packed for a HIP device (got %s)" % blob.device)
        self._launch(blob.device, "pack", blob)
        torch.cuda.current_stream(blob.device).synchronize()
        return blob

    @staticmethod
    def _rows(wavs):
        wavs = _f32c(wavs, "wavs")
        if wavs.dim() != 2:
            raise RuntimeError("wavs must be [B, L] (got %s)" % (tuple(wavs.shape),))
        return wavs, int(wavs.shape[0]), int(wavs.shape[1])

    def resample(self, blob, wavs):
        """wavs [B, L] at source_sr -> (out [B, resampled_length(L)] at sampling_rate, partials [B, tiles] for normalize); one launch."""
        wavs, B, L = self._rows(wavs)
        Lo = self.resampled_length(L)
        out = torch.empty((B, Lo), dtype=torch.float32, device=wavs.device)
        partials = torch.empty((B, self.tiles(Lo)), dtype=torch.float32, device=wavs.device)
        self._launch(wavs.device, "resample", blob, wavs, out, partials, B, L)
        return out, partials

    def normalize(self, blob, wavs, target_dBFS, increase_only=False, decrease_only=False, partials=None):
        """normalize_volume_batch: wavs [B, L] -> [B, L].  partials: what resample returned beside THESE wavs (one launch); None: the
        tile sums are formed first in the cached workspace (two launches, the same bits).  blob is not read (no table is needed)."""
        if increase_only and decrease_only:
            raise ValueError("Both increase only and decrease only are set")
        wavs, B, L = self._rows(wavs)
        ws = None
        if partials is None:
            ws = self._one_workspace((B, L, str(wavs.device)), wavs.device, lambda: max(self.workspace_bytes(B, L), 256))
        elif (not partials.is_cuda or partials.dtype != torch.float32 or not partials.is_contiguous()
              or tuple(partials.shape) != (B, self.tiles(L))):
            raise RuntimeError("partials must be the fp32 [%d, %d] tensor resample returned beside these wavs" % (B, self.tiles(L)))
        out = torch.empty_like(wavs)
        self._launch(wavs.device, "normalize", wavs, partials, float(target_dBFS), 1 if increase_only else 2 if decrease_only else 0,
                     out, ws, 0 if ws is None else ws.numel(), B, L)
        return out

    def powmel(self, blob, wavs):
        """wavs [B, L] at sampling_rate -> power mel [B, frames(L), n_mels] in one launch."""
        wavs, B, L = self._rows(wavs)
        out = torch.empty((B, self.frames(L), self.n_mels), dtype=torch.float32, device=wavs.device)
        self._launch(wavs.device, "powmel", blob, wavs, out, B, L)
        return out


class SpkPlan(_Native):
    """DiffVC speaker encoder (DiffVC/speaker_encoder/encoder/model.py:43-63) on the HIP kernels (csrc/spk.hip): LSTM stack, Linear,
    ReLU, L2 normalisation, and the mean + renormalisation over an utterance's partials."""
    _family = "spk"

    def __init__(self, n_mels=40, hidden=256, layers=3, embed=256):
        self.cfg = SpkCfg(int(n_mels), int(hidden), int(layers), int(embed))
        self.n_mels, self.hidden, self.layers, self.embed = int(n_mels), int(hidden), int(layers), int(embed)
        self._open(dict(n_mels=int(n_mels), hidden=int(hidden), layers=int(layers), embed=int(embed)), ctypes.byref(self.cfg))

    def forward(self, blob, frames, P=1, S=0, T=None, want_hidden=False, want_utt=False):
        """frames [U, T_total, n_mels] -> embeds [U * P, embed]: sequence u * P + p is frames[u, p * S : p * S + T] (the slicing is load
        addressing in the kernel; P = 1, S = 0, T = None: every row of frames is one sequence).  want_hidden: also h_T of the last
        layer [U * P, hidden]; want_utt: also the normalised mean over each utterance's P embeddings [U, embed].  Returns embeds, or
        (embeds[, hidden][, utt]) in that order."""
        frames = _f32c(frames, "frames")
        if frames.dim() != 3 or frames.shape[2] != self.n_mels:
            raise RuntimeError("frames must be [U, T_total, %d] (got %s)" % (self.n_mels, tuple(frames.shape)))
        U, T_total, _ = frames.shape
        P, S = int(P), int(S)
        T = T_total if T is None else int(T)
        dev = frames.device
        N = U * max(P, 0)
        nbytes = self.workspace_bytes(N, T) if N > 0 and T > 0 else 0
        ws = self._one_workspace((N, T, str(dev)), dev, lambda: max(nbytes, 256))
        embeds = torch.empty((max(N, 0), self.embed), dtype=torch.float32, device=dev)
        hidden = torch.empty((max(N, 0), self.hidden), dtype=torch.float32, device=dev) if want_hidden else None
        utt = torch.empty((U, self.embed), dtype=torch.float32, device=dev) if want_utt else None
        self._launch(dev, "forward", blob, frames, U, T_total, P, S, T, embeds, hidden, utt, ws, ws.numel())
        out = [embeds] + ([hidden] if want_hidden else []) + ([utt] if want_utt else [])
        return out[0] if len(out) == 1 else tuple(out)

    # ---- training (csrc/spk_train.hip)
    def pack_train(self, state, device):
        """The weights in the orders the backward reads (W_hh^T and W_ih^T as MFMA fragments, linear.weight): a blob of its own beside
        pack()'s, from the same state."""
        keep, arr = self._params(state, device)
        blob = torch.empty(int(lib().gtts_spktrain_packed_bytes(self._h)), dtype=torch.uint8, device=device)
        _launch(blob.device, "gtts_spktrain_pack", self._h, arr, len(keep), blob)
        torch.cuda.current_stream(blob.device).synchronize()     # sources in `keep` may be temporaries
        return blob

    def saved_bytes(self, N, T):
        return int(lib().gtts_spktrain_saved_bytes(self._h, int(N), int(T)))

    def train_workspace_bytes(self, N, T):
        return int(lib().gtts_spktrain_workspace_bytes(self._h, int(N), int(T)))

    def forward_train(self, blob, frames):
        """frames [N, T, n_mels] -> (embeds [N, embed], saved): the embeddings of forward(), bit for bit, and the uint8 tensor of
        saved_bytes(N, T) bytes that backward() takes (gates, cell states and hidden sequences of every layer, h_T, the head before
        its norm).  No workspace: every intermediate is part of `saved`."""
        frames = _f32c(frames, "frames")
        if frames.dim() != 3 or frames.shape[2] != self.n_mels:
            raise RuntimeError("frames must be [N, T, %d] (got %s)" % (self.n_mels, tuple(frames.shape)))
        N, T, _ = frames.shape
        dev = frames.device
        embeds = torch.empty((N, self.embed), dtype=torch.float32, device=dev)
        saved = torch.empty(max(self.saved_bytes(N, T) if N > 0 and T > 0 else 0, 256), dtype=torch.uint8, device=dev)
        _launch(dev, "gtts_spktrain_forward", self._h, blob, frames, N, T, embeds, saved, saved.numel())
        return embeds, saved

    def backward(self, blob_train, frames, d_embeds, saved):
        """The gradients of every parameter, in param_layout() order and of the parameters' shapes, for the upstream d_embeds [N, embed].
        `saved` comes from forward_train on the same frames and is consumed (the gate gradients are written over the gates)."""
        frames, d_embeds = _f32c(frames, "frames"), _f32c(d_embeds, "d_embeds")
        N, T, _ = frames.shape
        dev = frames.device
        if tuple(d_embeds.shape) != (N, self.embed):
            raise RuntimeError("d_embeds must be [%d, %d] (got %s)" % (N, self.embed, tuple(d_embeds.shape)))
        grads = [torch.empty(shape, dtype=torch.float32, device=dev) for _, shape in self.param_layout()]
        arr = (ctypes.c_void_p * len(grads))(*[g.data_ptr() for g in grads])
        nbytes = self.train_workspace_bytes(N, T) if N > 0 and T > 0 else 0
        cache = self.__dict__.setdefault("_ws_train", {})      # beside forward()'s workspace: a training loop alternates the two
        ws = cache.get((N, T, str(dev)))
        if ws is None:
            cache.clear()
            ws = cache[(N, T, str(dev))] = torch.empty(max(nbytes, 256), dtype=torch.uint8, device=dev)
        _launch(dev, "gtts_spktrain_backward", self._h, blob_train, frames, d_embeds, saved, saved.numel(), arr, len(grads), ws, ws.numel(), N, T)
        return grads


_GE2E_WS = {}       # the single live workspace of ge2e_loss: {(S, U, E, str(device)): uint8 tensor}


def ge2e_loss(embeds, w, b, want_grad=True):
    """GE2E similarity matrix, loss and gradient in one launch (csrc/spk_train.hip).  embeds [S, U, E], w and b one-element tensors on
    the same HIP device -> (sim [S * U, S], loss [1], d_embeds [S, U, E], dw [1], db [1]) for a loss gradient of 1; with
    want_grad=False the three gradients are None and their phases are skipped."""
    op = "ge2e_loss"
    embeds = _in(op, "embeds", embeds)
    if embeds.dim() != 3:
        raise ArgumentError("embeds must be [speakers, utterances, embed] (got %s)" % (tuple(embeds.shape),))
    dev, (S, U, E) = embeds.device, embeds.shape
    w, b = _in(op, "w", w, 1, dev), _in(op, "b", b, 1, dev)
    key = (S, U, E, str(dev))
    ws = _GE2E_WS.get(key)
    if ws is None:
        _GE2E_WS.clear()
        ws = torch.empty(max(int(lib().gtts_ge2e_workspace_bytes(S, U, E)), 256), dtype=torch.uint8, device=dev)
        _GE2E_WS[key] = ws
    sim = torch.empty((S * U, S), dtype=torch.float32, device=dev)
    loss = torch.empty(1, dtype=torch.float32, device=dev)
    d_embeds = torch.empty_like(embeds) if want_grad else None
    dw = torch.empty(1, dtype=torch.float32, device=dev) if want_grad else None
    db = torch.empty(1, dtype=torch.float32, device=dev) if want_grad else None
    _launch(dev, "gtts_ge2e_loss", embeds, w, b, S, U, E, sim, loss, d_embeds, dw, db, ws, ws.numel())
    return sim, loss, d_embeds, dw, db


def euler_step(xt, mu, est, mask, beta_t, h, noise=None):
    """In-place update of xt [B,F,T] (one step of Diffusion.reverse_diffusion, diffusion.py:264-274): mu, est and noise (or None) of
    xt's shape, mask [B,T] in any view of B * T elements ([B,1,T])."""
    op = "euler_step"
    if not xt.is_cuda or xt.dtype != torch.float32 or not xt.is_contiguous():
        raise ArgumentError("xt must be a contiguous fp32 HIP tensor (updated in place)")
    dev, (B, F, T) = xt.device, xt.shape
    mu, est, mask = _in(op, "mu", mu, (B, F, T), dev), _in(op, "est", est, (B, F, T), dev), _in(op, "mask", mask, B * T, dev)
    noise = _in(op, "noise", noise, (B, F, T), dev, optional=True)
    _launch(dev, "gtts_euler_step", xt, mu, est, mask, noise, float(beta_t), float(h), B, F, T)
    return xt


def mas_maximum_path(value, mask):
    """monotonic_align.maximum_path(value, mask) (value, mask: [b, t_x, t_y]).

    HIP tensors run the GPU kernel.  Host tensors run the library's C++ twin gtts_mas_maximum_path_cpu -- the
    reference's wrapper accepts tensors on any device and always runs its Cython kernel on the host
    (monotonic_align/__init__.py:8-23); both are bit-identical to it."""
    v = value.detach().float().contiguous()
    m = mask.detach().to(device=v.device, dtype=torch.float32).contiguous()
    b, tx, ty = v.shape
    if m.shape != (b, tx, ty):
        raise ArgumentError("mas_maximum_path: mask has shape %s, expected %s" % (tuple(m.shape), (b, tx, ty)))
    t_x = m.sum(1)[:, 0].to(torch.int32).contiguous()       # __init__.py:20-21
    t_y = m.sum(2)[:, 0].to(torch.int32).contiguous()
    path = torch.empty((b, tx, ty), dtype=torch.int32, device=v.device)
    if not v.is_cuda:
        _check(lib().gtts_mas_maximum_path_cpu(_ptr(v), _ptr(m), _ptr(t_x), _ptr(t_y), _ptr(path), b, tx, ty),
               "gtts_mas_maximum_path_cpu")
        return path.to(dtype=value.dtype)
    scratch = torch.empty(int(lib().gtts_mas_scratch_bytes(b, tx, ty)), dtype=torch.uint8, device=v.device)
    _launch(v.device, "gtts_mas_maximum_path", v, m, t_x, t_y, path, scratch, b, tx, ty)
    return path.to(dtype=value.dtype)


# ---- training hot path (csrc/train.hip): raw kernels; the autograd wiring lives in model/_train_ops.py
_MAX_TENSOR_ELEMS = 1 << 29      # per call: B * max(cin, cout) * H * W (32-bit byte offsets inside the kernels; train_wgrad.hip)


def conv_size_ok(B, cin, cout, H, W):
    """The training kernels address one call's tensors with 32-bit byte offsets: larger shapes must take the torch path."""
    return int(B) * max(int(cin), int(cout)) * int(H) * int(W) < _MAX_TENSOR_ELEMS


def _tiles(c):
    """Whole output tiles of the MFMA convolution kernels: 64 channels, or a multiple of 128."""
    return c == 64 or (c > 64 and c % 128 == 0)


def _dgrad_small_ok(need_dgrad, shape):
    """gtts_conv_dgrad_small stages whole rows with their halo in LDS: at most 2289 columns."""
    return not need_dgrad or shape is None or int(shape[2]) <= 2289


def conv3x3_supported(cin, cout, need_dgrad=True, shape=None):
    """Channel counts (and, with shape = (B, H, W), tensor sizes) the training conv kernels take (forward / data gradient /
    weight gradient).  The first layer (the stacked 2- or 3-plane input) has its own weight-gradient and data-gradient kernels
    (gtts_conv_wgrad_small, gtts_conv_dgrad_small)."""
    if shape is not None and not conv_size_ok(shape[0], cin, cout, shape[1], shape[2]):
        return False
    if cin in (2, 3):
        return _tiles(cout) and _dgrad_small_ok(need_dgrad, shape)
    if conv3x3_narrow(cin, cout):
        return cin == 32 or not need_dgrad
    return cin % 32 == 0 and cout % 32 == 0 and _tiles(cin) and _tiles(cout)


def conv3x3_narrow(cin, cout):
    """RefBlock's narrow layers (DiffVC/model/modules.py:128-157 at base 32): 1 or 32 input channels, which fit no 64-channel tile and
    have kernels of their own (csrc/train_narrow.hip; cin 1: no data gradient -- its input is data)."""
    return int(cin) in (1, 32) and int(cout) in (64, 128)


_PACKED = {}       # (id(weight), transposed, kind) -> (weakref to the weight, its version, pack generation, packed blob)
_PACK_GEN = 0      # a packed copy is shared only by the forward and the backward of ONE estimator call (new_pack_generation)
_CONSTS = {}       # (device, kind, n) -> ones / zeros of the data-gradient call


def new_pack_generation():
    """Called at every entry of the training estimator (model/_train_ops.py): packed weight copies made before this point are
    not reused.  Tensor._version does not see writes through `p.data` (EMA swaps, manual SGD, `p.data = t`); with the generation
    in the validity check a stale pack cannot outlive the step that made it, at the price of one re-pack (microseconds) per
    convolution and step."""
    global _PACK_GEN
    _PACK_GEN += 1


def clear_packed_cache():
    """Drop every cached packed training weight (Diffusion.invalidate_packed and the load_state_dict hook call this)."""
    global _PACK_GEN
    _PACK_GEN += 1
    _PACKED.clear()


# kind -> (family of gtts_<family>_packed_bytes / gtts_<family>_pack, `up` of the resampling family (None: the family takes
# `transposed` there), gtts_pack_item.kind (None: not part of the batched pack)).  "dn" Downsample forward, "up" Upsample forward,
# "dn_T" Downsample's data gradient.
_PACK_KINDS = {"3x3": ("conv3x3", None, 0), "1x1": ("conv1x1", None, 1), "7x7": ("conv7x7", None, None),
               "dn": ("conv_resample", 0, 2), "up": ("conv_resample", 1, 3), "dn_T": ("conv_resample", 1, 4)}
_PACK_TAPS = {"3x3": 9, "1x1": 1, "7x7": 49, "dn": 9, "up": 16, "dn_T": 9}      # elements of a kind's weight per (cin, cout) pair


def _packed_nbytes(kind, cin, cout):
    family, up, _ = _PACK_KINDS[kind]
    return int(getattr(lib(), "gtts_%s_packed_bytes" % family)(int(cin), int(cout), *(() if up is None else (up,))))


def _packed_weight(weight, cin, cout, transposed, kind):
    """Packed (fragment-order, bf16 hi / lo) copy of a convolution weight, cached per Parameter OBJECT and version: the entry is
    valid only while the very same tensor object is alive and unmodified (an optimizer step bumps `_version`; a data pointer
    alone can be recycled by the caching allocator for a different weight of the same shape)."""
    key = (id(weight), bool(transposed), kind)
    hit = _PACKED.get(key)
    if (hit is not None and hit[0]() is weight and hit[1] == int(weight._version) and hit[2] == _PACK_GEN and
            hit[3].device == weight.device):
        return hit[3]
    family, up, _ = _PACK_KINDS[kind]
    # "dn_T": an Upsample of dy with the forward weight [cout][cin][3][3] zero-padded to [.][.][4][4] (ConvTranspose2d layout:
    # [in = cout][out = cin])
    src = torch.nn.functional.pad(weight, (0, 1, 0, 1)).contiguous() if kind == "dn_T" else weight
    packed = torch.empty(_packed_nbytes(kind, cin, cout), dtype=torch.uint8, device=weight.device)
    _launch(weight.device, "gtts_%s_pack" % family, src, packed, cin, cout, (1 if transposed else 0) if up is None else up)
    if len(_PACKED) >= 512:          # (two entries per convolution: ~100 for the Grad-TTS U-Net); dead entries go with the sweep
        for k in [k for k, v in _PACKED.items() if v[0]() is None]:
            del _PACKED[k]
        if len(_PACKED) >= 512:
            _PACKED.clear()
    _PACKED[key] = (weakref.ref(weight), int(weight._version), _PACK_GEN, packed)
    return packed


class PackSpecs(list):
    """[(weight, cin, cout, transposed, kind)] of one module tree, plus the batched-pack plan built for it (device descriptor table +
    the blobs it fills).  The plan hangs off THIS list, and the list off the estimator it was built from (_train_ops._pack_specs), so
    weights, blobs and table die with the estimator; there is no module-global table of plans."""
    plan = None


def _build_pack_plan(specs, dev, sig):
    L = lib()
    n = len(specs)
    items = (PackItem * n)()
    blobs = []
    with _on(dev):
        for k, (w, ci, co, t, kind) in enumerate(specs):
            # (the packing kernel reads the weight where it lies, at every later step too: nothing may be converted or copied)
            _in("prepack", "weight %d" % k, w, int(ci) * int(co) * _PACK_TAPS[kind], dev, strict=True)
            blob = torch.empty(_packed_nbytes(kind, ci, co), dtype=torch.uint8, device=dev)
            blobs.append(blob)
            items[k].w, items[k].packed = w.data_ptr(), blob.data_ptr()
            items[k].kind, items[k].cin, items[k].cout, items[k].transposed = _PACK_KINDS[kind][2], int(ci), int(co), 1 if t else 0
        nbytes = int(L.gtts_pack_batch_desc_bytes(n))
        host = (ctypes.c_ubyte * nbytes)()
        grid = ctypes.c_int(0)
        _check(L.gtts_pack_batch_describe(items, n, ctypes.cast(host, ctypes.c_void_p), ctypes.byref(grid)), "gtts_pack_batch_describe")
        desc = torch.frombuffer(bytearray(host), dtype=torch.uint8).to(dev)
    # (weights are referenced weakly here: the spec list is what keeps them alive)
    return {"desc": desc, "n": n, "grid": int(grid.value), "sig": sig,
            "entries": [((id(w), bool(t), kind), weakref.ref(w), blob) for (w, ci, co, t, kind), blob in zip(specs, blobs)]}


def prepack(specs):
    """All weight packs of one training step in ONE launch (gtts_pack_batch).  specs: [(weight, cin, cout, transposed, kind)] with the
    meanings of _packed_weight (cin / cout of the convolution being packed).  With a PackSpecs list the blobs are allocated once and
    re-filled in place at every call (a plain list gets a plan per call); the per-weight cache entries are stamped with the current pack
    generation, so the autograd Functions of this step find them and nothing older survives.  Call after new_pack_generation(), on
    the stream the step runs on."""
    if not specs:
        return
    dev = specs[0][0].device
    sig = tuple([w.data_ptr() for w, *_ in specs])          # (cheap per-step check: the addresses the descriptor table holds)
    plan = getattr(specs, "plan", None)
    if plan is None or plan["sig"] != sig or plan["n"] != len(specs):
        plan = _build_pack_plan(specs, dev, sig)
        if isinstance(specs, PackSpecs):
            specs.plan = plan
    _launch(dev, "gtts_pack_batch", plan["desc"], plan["n"], plan["grid"])
    gen = _PACK_GEN
    for (key, ref, blob), spec in zip(plan["entries"], specs):
        w = spec[0]
        _PACKED[key] = (ref if ref() is w else weakref.ref(w), w._version, gen, blob)


def _const(device, kind, *shape):
    key = (str(device), kind) + shape
    v = _CONSTS.get(key)
    if v is None:
        v = (torch.ones if kind == "ones" else torch.zeros)(shape, dtype=torch.float32, device=device)
        _CONSTS[key] = v
    return v


def _out(op, given, name, shape, dev, dtype=torch.float32):
    """THE rule for a result of the wrapper `op`: the caller's preallocated tensor -- `given`, or `given[name]` of a dict; tests place
    them between guard margins -- has to be a contiguous `dtype` tensor of exactly `shape` on `dev`; without one a fresh tensor is made."""
    t = given.get(name) if isinstance(given, dict) else given
    if t is None:
        return torch.empty(shape, dtype=dtype, device=dev)
    if t.shape != shape or t.dtype != dtype or t.device != dev or not t.is_contiguous():
        raise ArgumentError("%s: output %s must be a contiguous %s tensor of shape %s on %s" % (op, name, dtype, tuple(shape), dev))
    return t


def _scratch(op, out, nbytes, dev):
    """The workspace of a weight-gradient call: `out["workspace"]` (fp32, exactly the bytes the call asks for) or a fresh one."""
    if out is None or out.get("workspace") is None:
        return torch.empty(nbytes, dtype=torch.uint8, device=dev)
    return _out(op, out, "workspace", (nbytes // 4,), dev)


def _i32(op, name, t, shape, dev):
    """_in for an int32 tensor the caller may give as a list of ints."""
    if not torch.is_tensor(t):
        t = torch.tensor(t, dtype=torch.int32)
    return _in(op, name, t.to(device=dev, dtype=torch.int32), shape, dev, dtype=torch.int32)


# kind -> (kernel size, the entry points take a second source x1 / c0, the forward entry point takes an output mask, the names of
# the forward / data-gradient entry point, of the weight gradient and of its workspace size)
_CONV_KINDS = {kind: (ksize, two, om, "gtts_conv%s_masked" % kind, "gtts_conv%s_wgrad" % kind, "gtts_conv%s_wgrad_workspace_bytes" % kind)
               for kind, ksize, two, om in (("3x3", 3, True, True), ("7x7", 7, False, True), ("1x1", 1, False, False))}


_TRAIN_NAME_KINDS = {"3x3": (0, 0), "1x1": (1, 0), "7x7": (2, 0), "dn": (3, 0), "up": (3, 1)}


def conv_train_kernel_name(kind, B, cin, cout, H, W, c0=0):
    """The kernel instance a forward / data-gradient convolution of the training path runs at this shape, as a demangler prints it
    (gtts_conv_train_kernel_name: the launching dispatch describing itself; works without a GPU).  kind: "3x3", "1x1", "7x7", "dn"
    (Downsample) or "up" (Upsample; Downsample's data gradient is an "up" call on the halved plane); B, cin, cout, H, W of the call
    asked about (a data gradient: the forward's cin and cout swapped); c0 in (0, cin): the 3x3 call reads two sources."""
    k, up = _TRAIN_NAME_KINDS[kind]
    buf = ctypes.create_string_buffer(256)
    _check(lib().gtts_conv_train_kernel_name(k, int(B), int(cin), int(c0), int(cout), int(H), int(W), up, buf, len(buf)),
           "gtts_conv_train_kernel_name")
    return buf.value.decode()


def _conv_run(op, kind, x, mask_cols, weight, bias, transposed, x1=None, out_mask=None, out=None, xname="x"):
    """The forward (transposed False) or data-gradient (True: x is dy, weight the forward's) call of a packed convolution kind for the
    wrapper `op`, every tensor checked: x [B,c0,H,W], x1 [B,c1,H,W] or None, masks [B,W], weight [cout,c0+c1,k,k] (transposed:
    [c0,cout,k,k]), bias [cout]."""
    ksize, two, om, name, _, _ = _CONV_KINDS[kind]
    x = _in(op, xname, x)
    dev, (B, c0, H, W) = x.device, x.shape
    c1 = 0 if x1 is None else x1.shape[1]
    x1 = _in(op, "x1", x1, (B, c1, H, W), dev, optional=True)
    cin, cout = c0 + c1, weight.shape[1 if transposed else 0]
    weight = _in(op, "weight", weight, (cin, cout, ksize, ksize) if transposed else (cout, cin, ksize, ksize), dev)
    mask_cols, bias = _in(op, "mask_cols", mask_cols, (B, W), dev), _in(op, "bias", bias, (cout,), dev)
    out_mask = _in(op, "mask_cols", out_mask, (B, W), dev, optional=True)
    y = _out(op, out, "out", (B, cout, H, W), dev)
    packed = _packed_weight(weight, cin, cout, transposed, kind)
    _launch(dev, name, *((x, x1, c0) if two else (x,)), mask_cols, *((out_mask,) if om else ()), packed, bias, y, B, cin, cout, H, W)
    return y


def _conv_dgrad(op, kind, dy, weight, mask_cols, out=None):
    B, W = dy.shape[0], dy.shape[-1]
    return _conv_run(op, kind, dy, _const(dy.device, "ones", B, W), weight, _const(dy.device, "zeros", int(weight.shape[1])), True,
                     out_mask=mask_cols, out=out, xname="dy")


def _wgrad_in(op, x, mask_cols, dy, x1=None, mask_optional=False):
    """The tensors a weight-gradient wrapper takes, checked: x [B,c0,H,W], x1 [B,c1,H,W] or None, mask_cols [B,W], dy [B,cout,H,W];
    returns them with the device and B, cin = c0 + c1, cout, H, W."""
    x = _in(op, "x", x)
    dev, (B, c0, H, W) = x.device, x.shape
    c1 = 0 if x1 is None else x1.shape[1]
    x1 = _in(op, "x1", x1, (B, c1, H, W), dev, optional=True)
    mask_cols = _in(op, "mask_cols", mask_cols, (B, W), dev, optional=mask_optional)
    cout = dy.shape[1]
    return x, mask_cols, _in(op, "dy", dy, (B, cout, H, W), dev), x1, dev, B, c0 + c1, cout, H, W


def _tiled_wgrad(op, kind, x, mask_cols, dy, x1=None, want_bias=True, out=None):
    """(dW [cout,cin,k,k], db [cout] or None) by the kind's LDS-tiled deterministic reduction (train_wgrad.hip, train_wgrad7.hip).
    `out`: optional dict of preallocated dw / db / workspace (fp32, gtts_conv<kind>_wgrad_workspace_bytes / 4 floats)."""
    ksize, two, _, _, name, ws_name = _CONV_KINDS[kind]
    x, mask_cols, dy, x1, dev, B, cin, cout, H, W = _wgrad_in(op, x, mask_cols, dy, x1, kind == "1x1")
    dw = _out(op, out, "dw", (cout, cin, ksize, ksize), dev)
    db = _out(op, out, "db", (cout,), dev) if want_bias else None
    nws = int(getattr(lib(), ws_name)(B, cin, cout, H, W))
    ws = _scratch(op, out, nws, dev)
    _launch(dev, name, *((x, x1, x.shape[1]) if two else (x,)), mask_cols, dy, dw, db, ws, nws, B, cin, cout, H, W)
    return dw, db


def _wgrad_small(op, x, mask_cols, dy, ksize, want_bias=True, out=None):
    """The first layer's weight gradient (cin 2 or 3: its own kernel).  `out`: optional dict of preallocated dw / db / workspace
    (gtts_conv_wgrad_small_scratch_floats floats)."""
    x, mask_cols, dy, _, dev, B, cin, cout, H, W = _wgrad_in(op, x, mask_cols, dy)
    dw = _out(op, out, "dw", (cout, cin, ksize, ksize), dev)
    db = _out(op, out, "db", (cout,), dev) if want_bias else None
    scratch = _out(op, out, "workspace", (int(lib().gtts_conv_wgrad_small_scratch_floats(B, cin, cout, ksize)),), dev)
    _launch(dev, "gtts_conv_wgrad_small", x, mask_cols, dy, dw, db, scratch, B, cin, cout, H, W, ksize)
    return dw, db


def conv3x3_masked(x, mask_cols, weight, bias, x1=None, out=None):
    """Conv2d_3x3(cat(x, x1) * mask) + bias (Block.forward, diffusion.py:56-57; the concatenation of the up path, :166, is read in
    place): x [B,c0,H,W], x1 [B,c1,H,W] or None, mask_cols [B,W], weight [cout,c0+c1,3,3], bias [cout].  `out`: optional preallocated
    result."""
    if x1 is None and conv3x3_narrow(weight.shape[1], weight.shape[0]):
        return conv3x3_narrow_forward(x, mask_cols, weight, bias, out=None if out is None else {"out": out})
    return _conv_run("conv3x3_masked", "3x3", x, mask_cols, weight, bias, False, x1, out=out)


def conv3x3_dgrad(dy, weight, mask_cols=None, out=None):
    """Gradient of conv3x3_masked w.r.t. (x * mask): a 3x3 convolution of dy [B,cout,H,W] with the transposed, flipped weights
    [cout,cin,3,3]; with mask_cols [B,W] the gradient w.r.t. x itself (the mask is applied in the kernel's epilogue).  `out`: optional
    preallocated result."""
    if conv3x3_narrow(weight.shape[1], weight.shape[0]):
        return conv3x3_narrow_dgrad(dy, weight, mask_cols, out=None if out is None else {"dx": out})
    return _conv_dgrad("conv3x3_dgrad", "3x3", dy, weight, mask_cols, out=out)


def conv3x3_wgrad(x, mask_cols, dy, x1=None, out=None):
    """(dW [cout,cin,3,3], db [cout]) of conv3x3_masked: x [B,c0,H,W], mask_cols [B,W], dy [B,cout,H,W] (x1 [B,c1,H,W]: second source
    of a concatenated input, c0 a multiple of 64).  `out`: optional dict of preallocated dw / db / workspace."""
    cin, cout = int(x.shape[1]) + (int(x1.shape[1]) if x1 is not None else 0), int(dy.shape[1])
    if cin in (2, 3) and x1 is None:
        return _wgrad_small("conv3x3_wgrad", x, mask_cols, dy, 3, out=out)
    if x1 is None and conv3x3_narrow(cin, cout):
        return conv3x3_narrow_wgrad(x, mask_cols, dy, out=out)
    if cin % 64 or cout % 64:
        raise ArgumentError("conv3x3_wgrad: cin and cout must be multiples of 64, or cin 2 or 3 from one source (got cin %d, cout %d)"
                         % (cin, cout))
    return _tiled_wgrad("conv3x3_wgrad", "3x3", x, mask_cols, dy, x1, out=out)


def _narrow_ws(op, out, B, cin, cout, H, W, which, dev):
    nws = int(lib().gtts_conv3x3_narrow_workspace_bytes(B, cin, cout, H, W, which))
    if nws == 0:
        raise ArgumentError("the narrow 3x3 kernels take cin 1 or 32 (the data gradient: 32) and cout 64 or 128 (got cin %d, cout %d, B %d, "
                         "%d x %d)" % (cin, cout, B, H, W))
    return _scratch(op, out, nws, dev), nws


def conv3x3_narrow_forward(x, mask_cols, weight, bias, out_mask=None, out=None):
    """Conv2d_3x3(x * mask) + bias [times out_mask] for RefBlock's narrow layers (cin 1 or 32, cout 64 or 128) on csrc/train_narrow.hip:
    x [B,cin,H,W], mask_cols / out_mask [B,W], weight [cout,cin,3,3] as the module holds it, bias [cout].  `out`: optional dict of a
    preallocated out / workspace (fp32, gtts_conv3x3_narrow_workspace_bytes / 4 floats)."""
    op = "conv3x3_narrow_forward"
    x = _in(op, "x", x)
    dev, (B, cin, H, W), cout = x.device, x.shape, int(weight.shape[0])
    weight, bias = _in(op, "weight", weight, (cout, cin, 3, 3), dev), _in(op, "bias", bias, (cout,), dev)
    mask_cols, out_mask = _in(op, "mask_cols", mask_cols, (B, W), dev), _in(op, "out_mask", out_mask, (B, W), dev, optional=True)
    y = _out(op, out, "out", (B, cout, H, W), dev)
    ws, nws = _narrow_ws(op, out, B, cin, cout, H, W, 0, dev)
    _launch(dev, "gtts_conv3x3_narrow_forward", x, mask_cols, out_mask, weight, bias, y, ws, nws, B, cin, cout, H, W)
    return y


def conv3x3_narrow_dgrad(dy, weight, mask_cols=None, out_mask=None, out=None):
    """dx [B,cin,H,W] of conv3x3_narrow_forward (cin 32) from dy [B,cout,H,W] and weight [cout,cin,3,3]: mask_cols [B,W] (None: ones) is
    the forward's input mask, out_mask [B,W] its output mask.  `out`: optional dict of a preallocated dx / workspace."""
    op = "conv3x3_narrow_dgrad"
    dy = _in(op, "dy", dy)
    dev, (B, cout, H, W), cin = dy.device, dy.shape, int(weight.shape[1])
    weight = _in(op, "weight", weight, (cout, cin, 3, 3), dev)
    mask_cols = _const(dev, "ones", B, W) if mask_cols is None else _in(op, "mask_cols", mask_cols, (B, W), dev)
    out_mask = _in(op, "out_mask", out_mask, (B, W), dev, optional=True)
    dx = _out(op, out, "dx", (B, cin, H, W), dev)
    ws, nws = _narrow_ws(op, out, B, cin, cout, H, W, 1, dev)
    _launch(dev, "gtts_conv3x3_narrow_dgrad", dy, out_mask, mask_cols, weight, dx, ws, nws, B, cin, cout, H, W)
    return dx


def conv3x3_narrow_wgrad(x, mask_cols, dy, out_mask=None, want_bias=True, out=None):
    """(dW [cout,cin,3,3], db [cout] or None) of conv3x3_narrow_forward: x [B,cin,H,W], mask_cols / out_mask [B,W], dy [B,cout,H,W].
    `out`: optional dict of preallocated dw / db / workspace."""
    op = "conv3x3_narrow_wgrad"
    x, mask_cols, dy, _, dev, B, cin, cout, H, W = _wgrad_in(op, x, mask_cols, dy)
    out_mask = _in(op, "out_mask", out_mask, (B, W), dev, optional=True)
    dw = _out(op, out, "dw", (cout, cin, 3, 3), dev)
    db = _out(op, out, "db", (cout,), dev) if want_bias else None
    ws, nws = _narrow_ws(op, out, B, cin, cout, H, W, 2, dev)
    _launch(dev, "gtts_conv3x3_narrow_wgrad", x, mask_cols, out_mask, dy, dw, db, ws, nws, B, cin, cout, H, W)
    return dw, db


def conv7x7_supported(cin, cout, need_dgrad=True, shape=None):
    """Channel counts (and, with shape = (B, H, W), tensor sizes) the 7x7 training kernels take (DiffVC PostNet Block): forward,
    data gradient and weight gradient all work on whole 64-channel tiles."""
    if shape is not None and not conv_size_ok(shape[0], cin, cout, shape[1], shape[2]):
        return False
    return int(cin) > 0 and int(cout) > 0 and int(cin) % 64 == 0 and int(cout) % 64 == 0


def conv7x7_masked(x, mask_cols, weight, bias, out=None):
    """Conv2d_7x7(x * mask, padding 3) + bias (PostNet Block, DiffVC/model/postnet.py:21-23): x [B,cin,H,W], mask_cols [B,W],
    weight [cout,cin,7,7], bias [cout].  `out`: optional preallocated result."""
    return _conv_run("conv7x7_masked", "7x7", x, mask_cols, weight, bias, False, out=out)


def conv7x7_dgrad(dy, weight, mask_cols=None, out=None):
    """Gradient of conv7x7_masked w.r.t. (x * mask): a 7x7 convolution of dy [B,cout,H,W] with the transposed, flipped weights
    [cout,cin,7,7]; with mask_cols [B,W] the gradient w.r.t. x itself (the mask is applied in the kernel's epilogue).  `out`: optional
    preallocated result."""
    return _conv_dgrad("conv7x7_dgrad", "7x7", dy, weight, mask_cols, out=out)


def conv7x7_wgrad(x, mask_cols, dy, out=None):
    """(dW [cout,cin,7,7], db [cout]) of conv7x7_masked (train_wgrad7.hip: deterministic split-bf16 MFMA reduction): x [B,cin,H,W],
    mask_cols [B,W], dy [B,cout,H,W].  `out`: optional dict of preallocated dw / db / workspace."""
    return _tiled_wgrad("conv7x7_wgrad", "7x7", x, mask_cols, dy, out=out)


def postnet_expand(x, mask, w, bias=None, out=None):
    """out [B,C,F,T] = w[c] * x[b,f,t] * mask[b,t] + bias[c] (PostNet init_conv; final_conv's data gradient with bias None): x [B,F,T],
    mask [B,T], w and bias C elements each (the weight flat or as the module's [C,1,1,1]: the element count decides).  `out`: optional
    preallocated result."""
    op = "postnet_expand"
    x = _in(op, "x", x)
    dev, (B, F, T), C = x.device, x.shape, int(w.numel())
    mask, w = _in(op, "mask", mask, (B, T), dev), _in(op, "w", w, C, dev)
    bias = _const(dev, "zeros", C) if bias is None else _in(op, "bias", bias, C, dev)
    out = _out(op, out, "out", (B, C, F, T), dev)
    _launch(dev, "gtts_postnet_expand", x, mask, w, bias, out, B, C, F, T)
    return out


def postnet_collapse(x, mask, w, bias=None, out=None):
    """out [B,F,T] = sum_c w[c] * x[b,c,f,t] * mask[b,t] + bias (PostNet final_conv; init_conv's data gradient with bias None):
    x [B,C,F,T], mask [B,T], w C elements (flat or [1,C,1,1]: the element count decides), bias one element.  `out`: optional
    preallocated result."""
    op = "postnet_collapse"
    x = _in(op, "x", x)
    dev, (B, C, F, T) = x.device, x.shape
    mask, w = _in(op, "mask", mask, (B, T), dev), _in(op, "w", w, C, dev)
    bias = _const(dev, "zeros", 1) if bias is None else _in(op, "bias", bias, 1, dev)
    out = _out(op, out, "out", (B, F, T), dev)
    _launch(dev, "gtts_postnet_collapse", x, mask, w, bias, out, B, C, F, T)
    return out


def postnet_chan_dot(a, v, mask, want_dot=True, want_sum=True, out=None):
    """(dot [C], sum [C]) over a [B,C,F,T]: dot[c] = sum a[b,c] * v[b] * mask[b,t] (v [B,F,T], mask [B,T]; v / mask None: 1), sum[c] =
    sum a[b,c] (fixed-order reduction; an output not wanted is None).  `out`: optional dict of preallocated dot / sum / workspace
    (gtts_postnet_chan_dot_scratch_floats floats)."""
    op = "postnet_chan_dot"
    a = _in(op, "a", a)
    dev, (B, C, F, T) = a.device, a.shape
    v, mask = _in(op, "v", v, (B, F, T), dev, optional=True), _in(op, "mask", mask, (B, T), dev, optional=True)
    dot = _out(op, out, "dot", (C,), dev) if want_dot else None
    sm = _out(op, out, "sum", (C,), dev) if want_sum else None
    scratch = _out(op, out, "workspace", (int(lib().gtts_postnet_chan_dot_scratch_floats(B, C, F, T)),), dev)
    _launch(dev, "gtts_postnet_chan_dot", a, v, mask, dot, sm, scratch, B, C, F, T)
    return dot, sm


def conv1x1_supported(cin, cout, need_dgrad=True, shape=None):
    """Channel counts (and, with shape = (B, H, W), tensor sizes) the 1x1 training kernels take: forward cout (and, for the
    data gradient, cin) a whole number of the kernel's output tiles; the weight gradient whole 64 x 64 tiles."""
    if shape is not None and not conv_size_ok(shape[0], cin, cout, shape[1], shape[2]):
        return False
    if cin in (2, 3):                             # first layer: own weight-gradient and data-gradient kernels
        return _tiles(cout) and _dgrad_small_ok(need_dgrad, shape)
    return _tiles(cout) and cin % 64 == 0 and (_tiles(cin) or not need_dgrad)


def conv1x1_masked(x, mask_cols, weight, bias, out=None):
    """Conv2d_1x1(x * mask) + bias (res_conv / to_qkv / to_out, diffusion.py:70,87-88): x [B,cin,H,W], mask_cols [B,W] or None,
    weight [cout,cin,1,1], bias [cout] or None.  `out`: optional preallocated result."""
    if mask_cols is None:
        mask_cols = _const(x.device, "ones", int(x.shape[0]), int(x.shape[3]))
    if bias is None:
        bias = _const(x.device, "zeros", int(weight.shape[0]))
    return _conv_run("conv1x1_masked", "1x1", x, mask_cols, weight, bias, False, out=out)


def conv1x1_dgrad(dy, weight, mask_cols=None, out=None):
    """Gradient of conv1x1_masked w.r.t. x: the 1x1 convolution of dy * mask (columns do not mix) with the transposed weight: dy
    [B,cout,H,W], weight [cout,cin,1,1], mask_cols [B,W] or None.  `out`: optional preallocated result."""
    if mask_cols is None:
        mask_cols = _const(dy.device, "ones", int(dy.shape[0]), int(dy.shape[3]))
    return _conv_run("conv1x1_dgrad", "1x1", dy, mask_cols, weight, _const(dy.device, "zeros", int(weight.shape[1])), True, out=out, xname="dy")


def conv1x1_wgrad(x, mask_cols, dy, want_bias=True, out=None):
    """(dW [cout,cin,1,1], db [cout] or None) of conv1x1_masked: x [B,cin,H,W], mask_cols [B,W] or None, dy [B,cout,H,W].  `out`:
    optional dict of preallocated dw / db / workspace."""
    if x.shape[1] in (2, 3):
        return _wgrad_small("conv1x1_wgrad", x, _const(x.device, "ones", int(x.shape[0]), int(x.shape[3])) if mask_cols is None else mask_cols,
                            dy, 1, want_bias, out=out)
    return _tiled_wgrad("conv1x1_wgrad", "1x1", x, mask_cols, dy, want_bias=want_bias, out=out)


def add_masked(a, b, mask_cols, channels=None, out=None):
    """a + b * mask (a None: b * mask; mask_cols None: a + b) over [B,C,H,W] with mask_cols [B,W].  channels = (c_begin, c_end):
    b is that channel range of a wider contiguous tensor [B,Cb,H,W] (read in place; the result and a have c_end - c_begin channels).
    `out`: optional preallocated result."""
    op = "add_masked"
    b = _in(op, "b", b)
    dev, (B, Cb, H, W) = b.device, b.shape
    c0, c1 = (0, Cb) if channels is None else channels
    if not 0 <= c0 < c1 <= Cb:
        raise ArgumentError("add_masked: channels %s lie outside b's %d" % ((c0, c1), Cb))
    a = _in(op, "a", a, (B, c1 - c0, H, W), dev, optional=True)
    mask_cols = _in(op, "mask_cols", mask_cols, (B, W), dev, optional=True)
    out = _out(op, out, "out", (B, c1 - c0, H, W), dev)
    _launch(dev, "gtts_add_masked", a, ctypes.c_void_p(b.data_ptr() + 4 * c0 * H * W), mask_cols, out, B, c1 - c0, H, W,
            0 if channels is None else Cb)
    return out


def zero_insert2(x, out=None):
    """[B,C,h,w] -> [B,C,2h,2w] with x at the even positions and zeros elsewhere.  `out`: optional preallocated result."""
    x = _in("zero_insert2", "x", x)
    B, C, h, w = x.shape
    out = _out("zero_insert2", out, "out", (B, C, 2 * h, 2 * w), x.device)
    _launch(x.device, "gtts_zero_insert2", x, out, B, C, h, w)
    return out


def space_to_depth2(x, out=None):
    """[B,C,2h,2w] -> [B,4C,h,w]: channel block (pr * 2 + pc) holds rows 2y + 1 - pr and columns 2x + 1 - pc.  `out`: optional
    preallocated result."""
    x = _in("space_to_depth2", "x", x)
    B, C, H2, W2 = x.shape
    if H2 % 2 or W2 % 2:
        raise ArgumentError("space_to_depth2: even height and width expected, got %d x %d" % (H2, W2))
    out = _out("space_to_depth2", out, "out", (B, 4 * C, H2 // 2, W2 // 2), x.device)
    _launch(x.device, "gtts_space_to_depth2", x, out, B, C, H2 // 2, W2 // 2)
    return out


def final_conv_forward(x, weight, bias, mask_cols, out=None):
    """(Conv2d_1x1(x * mask) + bias) * mask for the 64 -> 1 final convolution (diffusion.py:175-176): x [B,C,H,W], weight C elements
    (the module's [1,C,1,1] or flat: the element count decides), bias one element, mask_cols [B,W] -> [B,1,H,W].  `out`: optional
    preallocated result."""
    op = "final_conv_forward"
    x = _in(op, "x", x)
    dev, (B, C, H, W) = x.device, x.shape
    weight, bias, mask_cols = _in(op, "weight", weight, C, dev), _in(op, "bias", bias, 1, dev), _in(op, "mask_cols", mask_cols, (B, W), dev)
    out = _out(op, out, "out", (B, 1, H, W), dev)
    _launch(dev, "gtts_final_conv_forward", x, weight, bias, mask_cols, out, B, C, H, W)
    return out


def final_conv_backward(x, weight, mask_cols, dout, out=None):
    """(dx, dweight [1,C,1,1], dbias [1]) of final_conv_forward: x [B,C,H,W], weight C elements, mask_cols [B,W], dout [B,1,H,W].
    `out`: optional dict of preallocated dx / dw / db / workspace (gtts_final_conv_scratch_floats floats)."""
    op = "final_conv_backward"
    x = _in(op, "x", x)
    dev, (B, C, H, W) = x.device, x.shape
    weight, mask_cols, dout = _in(op, "weight", weight, C, dev), _in(op, "mask_cols", mask_cols, (B, W), dev), _in(op, "dout", dout, (B, 1, H, W), dev)
    dx, dw, db = _out(op, out, "dx", (B, C, H, W), dev), _out(op, out, "dw", (1, C, 1, 1), dev), _out(op, out, "db", (1,), dev)
    scratch = _out(op, out, "workspace", (int(lib().gtts_final_conv_scratch_floats(B, C, H, W)),), dev)
    _launch(dev, "gtts_final_conv_backward", x, weight, mask_cols, dout, dx, dw, db, scratch, B, C, H, W)
    return dx, dw, db


def resample_supported(cin, cout, H, W, up, B=1):
    # largest tensor of the call and of its gradients: Upsample's output (and its space_to_depth planes) is 4 cout planes of H x W
    if not conv_size_ok(B, 4 * max(cin, cout) if up else max(cin, cout), 1, H, W):
        return False
    return _tiles(cin) and _tiles(cout) and (up or (H % 2 == 0 and W % 2 == 0))


def conv_resample(x, mask_cols, weight, bias, up, dgrad_of_down=False, out=None):
    """Downsample (up False: Conv2d 3x3 stride 2 pad 1, weight [cout,cin,3,3]) or Upsample (up True: ConvTranspose2d 4x4 stride 2
    pad 1, weight [cin,cout,4,4]) of x * mask (diffusion.py:19-34): x [B,cin,H,W], mask_cols [B,W], bias [cout] or None.
    dgrad_of_down: x is the gradient of a Downsample output and weight that Downsample's forward weight [cin,cout,3,3]; the result is
    its data gradient (an Upsample with the zero-padded kernel).  `out`: optional preallocated result."""
    op = "conv_resample"
    x = _in(op, "x", x)
    dev, (B, cin, H, W) = x.device, x.shape
    if dgrad_of_down:
        cout, kind, up, wshape = int(weight.shape[1]), "dn_T", True, (cin, int(weight.shape[1]), 3, 3)
    elif up:
        cout, kind, wshape = int(weight.shape[1]), "up", (cin, int(weight.shape[1]), 4, 4)
    else:
        cout, kind, wshape = int(weight.shape[0]), "dn", (int(weight.shape[0]), cin, 3, 3)
    mask_cols, weight = _in(op, "mask_cols", mask_cols, (B, W), dev), _in(op, "weight", weight, wshape, dev)
    bias = _const(dev, "zeros", cout) if bias is None else _in(op, "bias", bias, (cout,), dev)
    y = _out(op, out, "out", (B, cout, 2 * H, 2 * W) if up else (B, cout, H // 2, W // 2), dev)
    packed = _packed_weight(weight, cin, cout, False, kind)
    _launch(dev, "gtts_conv_resample", x, mask_cols, packed, bias, y, B, cin, cout, H, W, 1 if up else 0)
    return y


def attn_train_forward(qkv, out=None):
    """LinearAttention core (diffusion.py:90-100) on to_qkv's output qkv [B,384,H,W]: (out [B,128,H,W], ctx [B,4,32,32],
    stat [B,4,32,2] = softmax row maxima and reciprocal sums).  `out`: optional dict of preallocated out / ctx / stat."""
    op = "attn_train_forward"
    qkv = _in(op, "qkv", qkv)
    dev, (B, C3, H, W) = qkv.device, qkv.shape
    if C3 != 384:
        raise ArgumentError("attn_train_forward: to_qkv output must have 3 x 4 heads x 32 = 384 channels, got %d" % C3)
    res, ctx, stat = _out(op, out, "out", (B, 128, H, W), dev), _out(op, out, "ctx", (B, 4, 32, 32), dev), _out(op, out, "stat", (B, 4, 32, 2), dev)
    scratch = torch.empty(int(lib().gtts_attn_train_scratch_floats(B, H * W)), dtype=torch.float32, device=dev)
    _launch(dev, "gtts_attn_train_forward", qkv, res, ctx, stat, scratch, B, H * W)
    return res, ctx, stat


def attn_train_backward(qkv, dout, ctx, stat, out=None):
    """d qkv of attn_train_forward given d out: qkv [B,384,H,W], dout [B,128,H,W], ctx [B,4,32,32] and stat [B,4,32,2] as the forward
    left them.  `out`: optional dict with a preallocated dqkv."""
    op = "attn_train_backward"
    qkv = _in(op, "qkv", qkv)
    dev, (B, C3, H, W) = qkv.device, qkv.shape
    if C3 != 384:
        raise ArgumentError("attn_train_backward: to_qkv output must have 3 x 4 heads x 32 = 384 channels, got %d" % C3)
    dout = _in(op, "dout", dout, (B, 128, H, W), dev)
    ctx, stat = _in(op, "ctx", ctx, (B, 4, 32, 32), dev), _in(op, "stat", stat, (B, 4, 32, 2), dev)
    dqkv = _out(op, out, "dqkv", (B, 384, H, W), dev)
    dctx = torch.empty((B, 4, 32, 32), dtype=torch.float32, device=dev)
    rdot = torch.empty((B, 4, 32), dtype=torch.float32, device=dev)
    scratch = torch.empty(int(lib().gtts_attn_train_scratch_floats(B, H * W)), dtype=torch.float32, device=dev)
    _launch(dev, "gtts_attn_train_backward", qkv, dout, ctx, stat, dqkv, dctx, rdot, scratch, B, H * W)
    return dqkv


def rezero_forward(f, g, x, out=None):
    """f * g + x (Rezero + Residual, diffusion.py:40-46,103-108); x of f's shape, g a 1-element device tensor.  `out`: optional dict
    with a preallocated y."""
    op = "rezero_forward"
    f = _in(op, "f", f)
    dev, shape = f.device, f.shape
    x, g = _in(op, "x", x, shape, dev), _in(op, "g", g, 1, dev)
    y = _out(op, out, "y", shape, dev)
    _launch(dev, "gtts_rezero_forward", f, x, g, y, f.numel())
    return y


def rezero_backward(dy, f, g, out=None):
    """(d f = dy * g, d g = sum(dy * f)) of rezero_forward: dy of f's shape.  `out`: optional dict of preallocated df / dg."""
    op = "rezero_backward"
    f = _in(op, "f", f)
    dev, shape = f.device, f.shape
    dy, g = _in(op, "dy", dy, shape, dev), _in(op, "g", g, 1, dev)
    df, dg = _out(op, out, "df", shape, dev), _out(op, out, "dg", g.shape, dev)
    scratch = torch.empty(int(lib().gtts_rezero_scratch_bytes(f.numel())), dtype=torch.uint8, device=dev)
    _launch(dev, "gtts_rezero_backward", dy, f, g, df, dg, scratch, f.numel())
    return df, dg


def gn_mish_forward(y, gamma, beta, mask_cols, groups, eps, tb=None, out=None):
    """(Mish(GroupNorm(y)) * mask [+ tb[:, :, None, None]], stats: (mean, rstd) pairs followed by reduction scratch) -- Block.forward
    after the convolution (diffusion.py:53-58) and, with tb [B,C], ResnetBlock's time term (diffusion.py:75-76): y [B,C,H,W], gamma and
    beta [C], mask_cols [B,W].  `out`: optional dict of preallocated out / stats."""
    op = "gn_mish_forward"
    y = _in(op, "y", y)
    dev, (B, C, H, W) = y.device, y.shape
    gamma, beta = _in(op, "gamma", gamma, (C,), dev), _in(op, "beta", beta, (C,), dev)
    mask_cols, tb = _in(op, "mask_cols", mask_cols, (B, W), dev), _in(op, "tb", tb, (B, C), dev, optional=True)
    res = _out(op, out, "out", (B, C, H, W), dev)
    stats = _out(op, out, "stats", (int(lib().gtts_gn_mish_stats_floats(B, int(groups))),), dev)
    _launch(dev, "gtts_gn_mish_forward", y, gamma, beta, mask_cols, tb, res, stats, B, C, H, W, int(groups), float(eps))
    return res, stats


def gn_mish_backward(dout, y, gamma, beta, mask_cols, stats, groups, want_dtb=False, out=None):
    """(dy, dgamma, dbeta[, dtb [B,C]]) of gn_mish_forward: dout of y's shape, stats as the forward left them
    (gtts_gn_mish_stats_floats floats).  `out`: optional dict of preallocated dy / dgamma / dbeta / dtb."""
    op = "gn_mish_backward"
    y = _in(op, "y", y)
    dev, (B, C, H, W) = y.device, y.shape
    dout, gamma, beta = _in(op, "dout", dout, (B, C, H, W), dev), _in(op, "gamma", gamma, (C,), dev), _in(op, "beta", beta, (C,), dev)
    mask_cols = _in(op, "mask_cols", mask_cols, (B, W), dev)
    stats = _in(op, "stats", stats, int(lib().gtts_gn_mish_stats_floats(B, int(groups))), dev)
    dy, dg, db = _out(op, out, "dy", (B, C, H, W), dev), _out(op, out, "dgamma", (C,), dev), _out(op, out, "dbeta", (C,), dev)
    dtb = _out(op, out, "dtb", (B, C), dev) if want_dtb else None
    scratch = torch.empty(int(lib().gtts_gn_mish_scratch_bytes(B, C)), dtype=torch.uint8, device=dev)
    _launch(dev, "gtts_gn_mish_backward", dout, y, gamma, beta, mask_cols, stats, dy, dg, db, dtb, scratch, B, C, H, W, int(groups))
    return (dy, dg, db, dtb) if want_dtb else (dy, dg, db)


def in_glu_forward(y, gamma, beta, eps=1e-5, tb=None, out=None):
    """(IN(y[:, :C]) * sigmoid(IN(y[:, C:])) [+ tb[:, :, None, None]], stats) -- InstanceNorm2d(affine) + GLU(dim=1) of DiffVC's RefBlock
    (modules.py:128-157) and, with tb [B,C], its time-bias add (modules.py:159,162): y [B,2C,H,W], gamma and beta [2C].  `out`: optional
    dict of preallocated out / stats."""
    op = "in_glu_forward"
    y = _in(op, "y", y)
    dev, (B, C2, H, W) = y.device, y.shape
    C = C2 // 2
    gamma, beta = _in(op, "gamma", gamma, (C2,), dev), _in(op, "beta", beta, (C2,), dev)
    tb = _in(op, "tb", tb, (B, C), dev, optional=True)
    res = _out(op, out, "out", (B, C, H, W), dev)
    stats = _out(op, out, "stats", (int(lib().gtts_in_glu_stats_floats(B, C)),), dev)
    if tb is None:
        _launch(dev, "gtts_in_glu_forward", y, gamma, beta, res, stats, B, C, H, W, float(eps))
    else:
        _launch(dev, "gtts_in_glu_tb_forward", y, gamma, beta, tb, res, stats, B, C, H, W, float(eps))
    return res, stats


def in_glu_backward(dout, y, gamma, beta, stats, want_dtb=False, out=None):
    """(dy, dgamma, dbeta[, dtb [B,C]]) of in_glu_forward: dout [B,C,H,W], y [B,2C,H,W], stats as the forward left them
    (gtts_in_glu_stats_floats floats).  `out`: optional dict of preallocated dy / dgamma / dbeta / dtb."""
    op = "in_glu_backward"
    y = _in(op, "y", y)
    dev, (B, C2, H, W) = y.device, y.shape
    C = C2 // 2
    dout, gamma, beta = _in(op, "dout", dout, (B, C, H, W), dev), _in(op, "gamma", gamma, (C2,), dev), _in(op, "beta", beta, (C2,), dev)
    stats = _in(op, "stats", stats, int(lib().gtts_in_glu_stats_floats(B, C)), dev)
    dy, dg, db = _out(op, out, "dy", (B, C2, H, W), dev), _out(op, out, "dgamma", (C2,), dev), _out(op, out, "dbeta", (C2,), dev)
    dtb = _out(op, out, "dtb", (B, C), dev) if want_dtb else None
    scratch = torch.empty(int(lib().gtts_in_glu_scratch_floats(B, C)), dtype=torch.float32, device=dev)
    if want_dtb:
        _launch(dev, "gtts_in_glu_tb_backward", dout, y, gamma, beta, stats, dy, dg, db, dtb, scratch, B, C, H, W)
    else:
        _launch(dev, "gtts_in_glu_backward", dout, y, gamma, beta, stats, dy, dg, db, scratch, B, C, H, W)
    return (dy, dg, db, dtb) if want_dtb else (dy, dg, db)


def cond_field(U, mask_cols, H, base=None, out=None):
    """base + the bias field of a condition vector convolved over the [H, W] plane (gtts_cond_field_forward): U [B,taps,C] with taps 9
    ((kh, kw) order, 3x3 with padding 1) or 1 (1x1), mask_cols [B,W], base [B,C,H,W] or None -> [B,C,H,W].  `out`: optional dict of a
    preallocated out."""
    op = "cond_field"
    U = _in(op, "U", U)
    dev, (B, taps, C), H, W = U.device, U.shape, int(H), int(mask_cols.shape[-1])
    mask_cols, base = _in(op, "mask_cols", mask_cols, (B, W), dev), _in(op, "base", base, (B, C, H, W), dev, optional=True)
    res = _out(op, out, "out", (B, C, H, W), dev)
    _launch(dev, "gtts_cond_field_forward", U, mask_cols, base, res, B, C, H, W, int(taps))
    return res


def cond_field_backward(dy, mask_cols, taps, out=None):
    """S [B,taps,C]: the gradient of cond_field w.r.t. U (the gradient w.r.t. base is dy itself): dy [B,C,H,W], mask_cols [B,W].
    `out`: optional dict of a preallocated S."""
    op = "cond_field_backward"
    dy = _in(op, "dy", dy)
    dev, (B, C, H, W) = dy.device, dy.shape
    mask_cols = _in(op, "mask_cols", mask_cols, (B, W), dev)
    S = _out(op, out, "S", (B, int(taps), C), dev)
    _launch(dev, "gtts_cond_field_backward", dy, mask_cols, S, B, C, H, W, int(taps))
    return S


def masked_mean(y, mask_cols, out=None):
    """p [B,C] = sum_{h,w} y mask / (sum_w mask H): RefBlock's masked mean over the plane (modules.py:165-166).  y [B,C,H,W], mask_cols
    [B,W].  `out`: optional dict of a preallocated p."""
    op = "masked_mean"
    y = _in(op, "y", y)
    dev, (B, C, H, W) = y.device, y.shape
    mask_cols = _in(op, "mask_cols", mask_cols, (B, W), dev)
    p = _out(op, out, "p", (B, C), dev)
    _launch(dev, "gtts_masked_mean_forward", y, mask_cols, p, B, C, H, W)
    return p


def masked_mean_backward(dp, mask_cols, H, out=None):
    """dy [B,C,H,W] of masked_mean: dp [B,C] broadcast over the live columns of mask_cols [B,W].  `out`: optional dict of a
    preallocated dy."""
    op = "masked_mean_backward"
    dp = _in(op, "dp", dp)
    dev, (B, C), H, W = dp.device, dp.shape, int(H), int(mask_cols.shape[-1])
    mask_cols = _in(op, "mask_cols", mask_cols, (B, W), dev)
    dy = _out(op, out, "dy", (B, C, H, W), dev)
    _launch(dev, "gtts_masked_mean_backward", dp, mask_cols, dy, B, C, H, W)
    return dy


def diffusion_noising(x0, mu, z, mask, t, beta_min, beta_max, out=None):
    """Diffusion.forward_diffusion given the N(0,1) draw z: (xt, z * mask)   (diffusion.py:244-252): x0, mu, z [B,F,T], mask B * T
    elements ([B,1,T] or [B,T]: the element count decides), t B elements.  `out`: optional dict of preallocated xt / zm."""
    op = "diffusion_noising"
    x0 = _in(op, "x0", x0)
    dev, (B, F, T) = x0.device, x0.shape
    mu, z = _in(op, "mu", mu, (B, F, T), dev), _in(op, "z", z, (B, F, T), dev)
    mask, t = _in(op, "mask", mask, B * T, dev), _in(op, "t", t, B, dev)
    xt, zm = _out(op, out, "xt", (B, F, T), dev), _out(op, out, "zm", (B, F, T), dev)
    _launch(dev, "gtts_diffusion_noising", x0, mu, z, mask, t, float(beta_min), float(beta_max), xt, zm, B, F, T)
    return xt, zm


def score_loss(eps, z_masked, t, beta_min, beta_max, inv_denom, want_grad=True, out=None):
    """Diffusion.loss_t's reduction: (sum((eps s + z)^2) * inv_denom as a 0-d tensor, d loss / d eps or None): eps, z_masked [B,F,T],
    t B elements.  inv_denom: a Python float, or a 0-d device tensor (then nothing here synchronises with the host: the kernel runs
    with a unit normaliser and loss and gradient are scaled by tensor ops).  `out`: optional dict of preallocated partials / grad."""
    if torch.is_tensor(inv_denom):
        loss, g = score_loss(eps, z_masked, t, beta_min, beta_max, 1.0, want_grad, out)
        return loss * inv_denom, (g * inv_denom if g is not None else None)
    op = "score_loss"
    eps = _in(op, "eps", eps)
    dev, (B, F, T) = eps.device, eps.shape
    z_masked, t = _in(op, "z_masked", z_masked, (B, F, T), dev), _in(op, "t", t, B, dev)
    part = _out(op, out, "partials", (int(lib().gtts_score_loss_partials(B, F, T)),), dev)
    g = _out(op, out, "grad", (B, F, T), dev) if want_grad else None
    _launch(dev, "gtts_score_loss", eps, z_masked, t, float(beta_min), float(beta_max), float(inv_denom), part, g, B, F, T)
    return part.sum() * inv_denom, g


def conv_dgrad_small(dy, weight, mask_cols=None, out=None):
    """The first layer's data gradient (cin 2 or 3, its own kernel): dx [B,cin,H,W] of Conv2d_kxk(x * mask) for k = 3 (padding 1) or 1,
    dy [B,cout,H,W], weight [cout,cin,k,k] (not packed), mask_cols [B,W] or None."""
    op = "conv_dgrad_small"
    dy = _in(op, "dy", dy)
    dev, (B, cout, H, W) = dy.device, dy.shape
    cin, ksize = int(weight.shape[1]), int(weight.shape[2])
    weight = _in(op, "weight", weight, (cout, cin, ksize, ksize), dev)
    mask_cols = _const(dev, "ones", B, W) if mask_cols is None else _in(op, "mask_cols", mask_cols, (B, W), dev)
    dx = _out(op, out, "dx", (B, cin, H, W), dev)
    _launch(dev, "gtts_conv_dgrad_small", dy, weight, mask_cols, dx, B, cin, cout, H, W, ksize)
    return dx


def diffusion_noising_backward(dxt, mask, t, beta_min, beta_max, want_dx0=True, want_dmu=True, out=None):
    """(dx0, dmu) of diffusion_noising (an output not wanted is None): dxt [B,F,T], mask B * T elements, t B elements."""
    op = "diffusion_noising_backward"
    dxt = _in(op, "dxt", dxt)
    dev, (B, F, T) = dxt.device, dxt.shape
    mask, t = _in(op, "mask", mask, B * T, dev), _in(op, "t", t, B, dev)
    dx0 = _out(op, out, "dx0", (B, F, T), dev) if want_dx0 else None
    dmu = _out(op, out, "dmu", (B, F, T), dev) if want_dmu else None
    _launch(dev, "gtts_diffusion_noising_backward", dxt, mask, t, float(beta_min), float(beta_max), dx0, dmu, B, F, T)
    return dx0, dmu


def align_index(path, out=None):
    """The alignment path [B,t_x,T] of monotonic_align.maximum_path as indices: (idx [B,T] int32 token of each frame or -1,
    dur [B,t_x] fp32 frames per token, first [B,t_x] int32 first frame of each token's run or -1)."""
    op = "align_index"
    path = _in(op, "path", path)
    dev, (B, tx, T) = path.device, path.shape
    idx, dur, first = _out(op, out, "idx", (B, T), dev, torch.int32), _out(op, out, "dur", (B, tx), dev), _out(op, out, "first", (B, tx), dev, torch.int32)
    _launch(dev, "gtts_align_index", path, idx, dur, first, B, tx, T)
    return idx, dur, first


def duration_loss(logw, dur, x_mask, want_grad=True, out=None):
    """(sum((logw - log(1e-8 + dur) * x_mask)^2) as a 0-d tensor, its gradient w.r.t. logw or None): utils.py:42-44 without the
    normaliser, which the caller keeps as a device scalar.  dur [B,t_x]; logw, x_mask: B * t_x elements each ([B,1,t_x] as the
    modules hold them: the element count decides)."""
    op = "duration_loss"
    lw = _in(op, "logw", logw)
    dev, B, tx = lw.device, int(dur.shape[0]), int(dur.shape[-1])
    lw, d, m = _in(op, "logw", lw, B * tx, dev), _in(op, "dur", dur, B * tx, dev), _in(op, "x_mask", x_mask, B * tx, dev)
    part = _out(op, out, "partials", (B,), dev)
    g = _out(op, out, "grad", lw.shape, dev) if want_grad else None
    _launch(dev, "gtts_duration_loss", lw, d, m, part, g, B, tx)
    return part.sum(), g


def align_gather(mu_x, y, idx, start, kept, S, out=None):
    """Training crop + aligned prior mean (tts.py:146-172) in one gather: (y_c [B,F,S], mu_y [B,F,S], sum over the live elements of
    0.5 ((y_c - mu_y)^2 + log 2 pi) as a 0-d tensor) from mu_x [B,F,t_x], y [B,F,T], idx [B,T] int32.  start, kept: [B] integer
    tensors (or lists); S: output frames."""
    op = "align_gather"
    mx = _in(op, "mu_x", mu_x)
    dev, (B, F, tx), T, S = mx.device, mx.shape, int(y.shape[2]), int(S)
    yy = _in(op, "y", y, (B, F, T), dev)
    if idx.dtype != torch.int32:
        raise ArgumentError("align_gather: idx must be int32 (got %s)" % idx.dtype)
    idx, st, kp = _in(op, "idx", idx, (B, T), dev, dtype=torch.int32), _i32(op, "start", start, (B,), dev), _i32(op, "kept", kept, (B,), dev)
    y_c, mu_y = _out(op, out, "y_c", (B, F, S), dev), _out(op, out, "mu_y", (B, F, S), dev)
    part = _out(op, out, "partials", (int(lib().gtts_align_gather_partials(B, F, S)),), dev)
    _launch(dev, "gtts_align_gather_forward", mx, yy, idx, st, kp, y_c, mu_y, part, B, F, tx, T, S)
    return y_c, mu_y, part.sum()


def align_gather_backward(g_mu_y, mu_y, y_c, scale, dur, first, start, kept, out=None):
    """dmu_x [B,F,t_x] of align_gather: per token the sum, over its live output frames, of g_mu_y + scale * (mu_y - y_c).  g_mu_y
    [B,F,S] or None; scale: a one-element device tensor, (gradient of the prior loss) / (sum(kept) F), or None (then mu_y, y_c [B,F,S]
    are unused and may be None); dur [B,t_x] fp32 and first [B,t_x] int32 as align_index left them."""
    op = "align_gather_backward"
    dur = _in(op, "dur", dur)
    dev, (B, tx) = dur.device, dur.shape
    ref = g_mu_y if g_mu_y is not None else mu_y
    if ref is None or ref.dim() != 3 or ref.shape[0] != B:
        raise ArgumentError("align_gather_backward: g_mu_y or mu_y must be [B,F,S] with dur's B = %d" % B)
    F, S = ref.shape[1], ref.shape[2]
    g, sc = _in(op, "g_mu_y", g_mu_y, (B, F, S), dev, optional=True), _in(op, "scale", scale, 1, dev, optional=True)
    my, yc = (_in(op, n, t, (B, F, S), dev, optional=sc is None) for n, t in (("mu_y", mu_y), ("y_c", y_c)))
    if first.dtype != torch.int32:
        raise ArgumentError("align_gather_backward: first must be int32 (got %s)" % first.dtype)
    first, st, kp = _in(op, "first", first, (B, tx), dev, dtype=torch.int32), _i32(op, "start", start, (B,), dev), _i32(op, "kept", kept, (B,), dev)
    dmu_x = _out(op, out, "dmu_x", (B, F, tx), dev)
    _launch(dev, "gtts_align_gather_backward", g, my, yc, sc, dur, first, st, kp, dmu_x, B, F, tx, S)
    return dmu_x


def log_prior(mu_x, y):
    """MAS score matrix of GradTTS.compute_loss (tts.py:130-139): [B,F,t_x], [B,F,T] -> [B,t_x,T], one launch."""
    op = "log_prior"
    mx = _in(op, "mu_x", mu_x.detach())
    dev, (B, F, tx), T = mx.device, mx.shape, y.shape[2]
    yy = _in(op, "y", y.detach(), (B, F, T), dev)
    out = torch.empty((B, tx, T), dtype=torch.float32, device=dev)
    _launch(dev, "gtts_log_prior", mx, yy, out, B, F, tx, T)
    return out


def expand_alignment(duration, x_mask, y_lengths, mu_x, T, noise=None, temperature=1.0):
    """generate_path + mu_y = attn^T . mu_x + z = mu_y + noise / temperature in one launch (tts.py:84-94).

    duration, x_mask: [B, t_x]; y_lengths: [B] integer; mu_x: [B, F, t_x]; noise: [B, F, T] or None.
    Returns (attn [B, t_x, T], mu_y [B, F, T], z [B, F, T] or None), bit-identical to the reference's CPU path."""
    op = "expand_alignment"
    mx = _in(op, "mu_x", mu_x)
    dev, (B, F, tx), T = mx.device, mx.shape, int(T)
    d, m = _in(op, "duration", duration, (B, tx), dev), _in(op, "x_mask", x_mask, (B, tx), dev)
    yl, nz = _i32(op, "y_lengths", y_lengths, (B,), dev), _in(op, "noise", noise, (B, F, T), dev, optional=True)
    attn = torch.empty((B, tx, T), dtype=torch.float32, device=dev)
    mu_y = torch.empty((B, F, T), dtype=torch.float32, device=dev)
    z = torch.empty((B, F, T), dtype=torch.float32, device=dev) if nz is not None else None
    _launch(dev, "gtts_expand_alignment", d, m, yl, mx, nz, float(temperature), attn, mu_y, z, B, F, tx, T)
    return attn, mu_y, z


def measured_ceilings(device, seconds=2.0):
    """Measured ceilings of this chip (bench.py roofline): bf16 MFMA TFLOP/s on random / zero operands and HBM GB/s for a
    16-byte copy, triad and read-only sweep.  About `seconds` of GPU time in total.  Returns a dict."""
    L = lib()
    out = {}
    with _on(device):
        props = torch.cuda.get_device_properties(device)
        cus = int(props.multi_processor_count)
        wgs = cus * 2                                   # 2 workgroups x 4 waves per CU = 2 waves per SIMD
        g = torch.Generator(device="cpu").manual_seed(0)
        rnd = torch.randn(1 << 20, generator=g).to(torch.bfloat16).to(device)
        zero = torch.zeros(1 << 20, dtype=torch.bfloat16, device=device)
        sink = torch.empty(int(L.gtts_ubench_mfma_out_floats(wgs)), dtype=torch.float32, device=device)
        flops = ctypes.c_double(0.0)

        def timed(fn, reps):
            fn()
            torch.cuda.synchronize(device)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                fn()
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1) * 1e-3 / reps

        iters = 4000                                    # 32 k MFMAs per wave: ~0.55 ms per launch at peak
        for name, src in (("random", rnd), ("zero", zero)):
            fn = lambda: _launch(device, "gtts_ubench_mfma", src, ctypes.c_size_t(src.numel() * 2), sink, wgs, iters, ctypes.byref(flops))
            t1 = timed(fn, 3)
            reps = max(3, int(seconds * 0.3 / max(t1, 1e-6)))      # long enough for the clock to settle at its power budget
            t = timed(fn, reps)
            out["mfma_bf16_tflops_%s" % name] = flops.value / t * 1e-12
        fn = lambda: _launch(device, "gtts_ubench_mfma", rnd, ctypes.c_size_t(rnd.numel() * 2), sink, wgs, -iters, ctypes.byref(flops))
        t1 = timed(fn, 3)
        out["mfma_bf16_16x16x32_tflops_random"] = flops.value / timed(fn, max(3, int(seconds * 0.3 / max(t1, 1e-6)))) * 1e-12
        # what the vendor's GEMM library reaches on the same chip with the same kind of data (hipBLASLt through torch.matmul,
        # 8192^3 bf16): the practical ceiling of an LDS-fed MFMA kernel, beside the register-only stream above
        m = 8192
        ga = torch.randn(m, m, generator=g).to(torch.bfloat16).to(device)
        gb = torch.randn(m, m, generator=g).to(torch.bfloat16).to(device)
        t = timed(lambda: torch.matmul(ga, gb), 10)
        out["gemm_bf16_tflops_random_hipblaslt"] = 2.0 * m ** 3 / t * 1e-12
        del ga, gb
        n = 1 << 28                                     # 1 GiB per buffer: four times the Infinity Cache
        a = torch.empty(n, dtype=torch.float32, device=device).normal_()
        b = torch.empty(n, dtype=torch.float32, device=device).normal_()
        c = torch.empty(n, dtype=torch.float32, device=device)
        nbytes = ctypes.c_double(0.0)
        for name, mode in (("copy", 0), ("triad", 1), ("read", 2)):
            best = 0.0
            for nt in (0, 4):                           # plain and nontemporal accesses, a few grid sizes: keep the best
                for wpc in (4, 8, 16):
                    fn = lambda: _launch(device, "gtts_ubench_hbm", a, b, c, ctypes.c_size_t(n), mode + nt, cus * wpc, ctypes.byref(nbytes))
                    t = timed(fn, 3)
                    gbs = nbytes.value / t * 1e-9
                    out.setdefault("hbm_detail", {})["%s_%s_wg%d" % (name, "nt" if nt else "plain", wpc)] = round(gbs, 1)
                    best = max(best, gbs)
            out["hbm_%s_gbs" % name] = best
        out["cus"] = cus
    return out
