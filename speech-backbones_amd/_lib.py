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


def _f32c(t, name):
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
        with torch.cuda.device(blob.device):
            self._call("pack", self._h, arr, len(keep), *extra, _ptr(blob), _stream())
            torch.cuda.current_stream().synchronize()     # sources in `keep` may be temporaries
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
        with torch.cuda.device(ws.device):
            _check(lib().gtts_workspace_status(_ptr(ws), ctypes.byref(n), ctypes.byref(mx), _stream()), "gtts_workspace_status")
        return int(n.value), float(mx.value)

    # ---- weights
    def pack(self, state, device):
        """state: mapping name -> tensor with the estimator-level names of the reference state_dict.
        PREC_F16F8: raises RangeError when a 3x3 Block-convolution weight does not fit the format (|w| >= 63.97)."""
        params = self._params(state, device)
        half = self.cfg.dim // 2
        # exactly SinusoidalPosEmb's frequency table, computed on the host CPU like the reference (diffusion.py:121-122)
        freq = torch.exp(torch.arange(half).float() * -(math.log(10000) / (half - 1))).to(device)
        return self._pack(params, device, _ptr(freq))

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
        with torch.cuda.device(x.device):
            _check(lib().gtts_estimator_forward(self._h, _ptr(blob), _ptr(x), _ptr(mask), _ptr(mu), _ptr(t), _ptr(spk),
                                                _ptr(out), _ptr(ws), ws.numel(), B, T, _stream()),
                   "gtts_estimator_forward")
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
            _check(lib().gtts_reverse_diffusion(self._h, _ptr(blob), _ptr(z), _ptr(mask), _ptr(mu), _ptr(spk),
                                                _ptr(noise), _ptr(out), _ptr(ws), ws.numel(), B, T, int(n_timesteps),
                                                0, int(n_timesteps), _stream()), "gtts_reverse_diffusion")
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
        with torch.cuda.device(x.device):
            _check(lib().gtts_vc_estimator_forward(self._h, _ptr(blob), _ptr(x), _ptr(x_mask), _ptr(mean), _ptr(xt_ref),
                                                   _ptr(ref_mask), _ptr(c), _ptr(t), _ptr(out), _ptr(ws), ws.numel(), B, T, Tr,
                                                   _stream()), "gtts_vc_estimator_forward")
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
                _check(lib().gtts_vc_reverse_diffusion(self._h, _ptr(blob), _ptr(z), _ptr(mask), _ptr(mean), _ptr(ref),
                                                       _ptr(ref_mask), _ptr(mean_ref), _ptr(c), _ptr(nz), _ptr(out), _ptr(ws),
                                                       ws.numel(), B, T, Tr, N, modes[mode], i0, i1, _stream()),
                       "gtts_vc_reverse_diffusion")
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
        with torch.cuda.device(mel.device):
            _check(lib().gtts_voc_forward(self._h, _ptr(blob), _ptr(mel), _ptr(wav), _ptr(ws), ws.numel(), B, T, _stream()),
                   "gtts_voc_forward")
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
        with torch.cuda.device(w.device):
            self._call("pack", self._h, _ptr(w), _ptr(blob), _stream())
            torch.cuda.current_stream().synchronize()
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
        with _on(weight.device):
            self._call("pack", self._h, _ptr(weight), _ptr(blob), _stream())
        return blob

    def pack_dgrad(self, weight, blob=None):
        """On the TRANSPOSED handle Conv1dOp(0, cout, cin, K, dilation): packs the forward module's weight [cout, cin, K] = [self.cin,
        self.cout, K] as W'[ci][co][t] = W[co][ci][K-1-t], one launch, no synchronise.  forward() of this handle on dy is then the data
        gradient (in_mask = the forward's output mask, out_mask = its input mask, a zero bias)."""
        blob = self._pack_source(weight, blob, (self.cin, self.cout, self.K))
        with _on(weight.device):
            self._call("pack_dgrad", self._h, _ptr(weight), _ptr(blob), _stream())
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
        _enc_op_tensors({"x": x, "dy": dy, "in_mask": in_mask, "out_mask": out_mask, "dw": dw, "db": db},
                        {"x": (B, cin, L), "dy": (B, self.cout, L), "in_mask": (B, L), "out_mask": (B, L), "dw": (self.cout, self.cin, self.K),
                         "db": (self.cout,)}, x.device)
        if workspace is None:
            workspace = torch.empty(self.wgrad_workspace_bytes(B, L), dtype=torch.uint8, device=x.device)
        elif workspace.device != x.device or not workspace.is_contiguous():
            raise RuntimeError("workspace must be a contiguous tensor on %s" % x.device)
        with _on(x.device):
            self._call("wgrad", self._h, _ptr(x), _ptr(in_mask), _ptr(dy), _ptr(out_mask), _ptr(dw), _ptr(db), _ptr(workspace),
                       workspace.numel() * workspace.element_size(), B, L, _stream())
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
        with _on(x.device):
            self._call("forward", self._h, _ptr(blob), _ptr(bias), _ptr(x), _ptr(out), _ptr(res), _ptr(accsrc), int(accmode), float(div),
                       float(slope), _ptr(in_mask), _ptr(out_mask), B, Lin, _stream())
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
        with torch.cuda.device(dev):
            _check(lib().gtts_enc_forward(self._h, _ptr(blob), _ptr(ids), _ptr(mel), _ptr(m), _ptr(mu), _ptr(logw), _ptr(ws),
                                          ws.numel(), B, L, _stream()), "gtts_enc_forward")
        return (mu, logw) if self.mode == "text" else mu


def _enc_op_tensors(given, shapes, dev):
    """The stand-alone encoder ops take views into larger allocations as they are: nothing is converted or copied."""
    for name, t in given.items():
        if t is None:
            continue
        if t.device != dev or t.dtype != torch.float32 or not t.is_contiguous():
            raise RuntimeError("%s must be a contiguous fp32 tensor on %s" % (name, dev))
        if tuple(t.shape) != shapes[name]:
            raise RuntimeError("%s has shape %s, expected %s" % (name, tuple(t.shape), shapes[name]))


def enc_attention_path(channels, n_heads, window, L):
    """Which attention kernel an encoder of these channels, heads and window runs at length L (16, 8, or 0: refused) -- a host
    call, the decision of Encoder.attention_path without a handle."""
    return int(lib().gtts_enc_attention_path_for(int(channels), int(n_heads), int(window or 0), int(L)))


def enc_layernorm(a, gamma, beta, bres=None, a_mask=None, out_mask=None, eps=1e-4, relu_in=False, relu_out=False, out=None):
    """The encoders' LayerNorm kernel on its own: relu_out?(LN_c(relu_in?(a) * a_mask + bres)) * out_mask.  a, bres [B,C,L]; gamma,
    beta [C]; masks [B,L]; written into `out` when given.  The launch gtts_enc_forward makes, for the per-op tests."""
    if not a.is_cuda:
        raise RuntimeError("the encoder kernels need HIP tensors (got %s); there is no CPU fallback here" % a.device)
    B, C, L = a.shape
    if out is None:
        out = torch.empty((B, C, L), dtype=torch.float32, device=a.device)
    _enc_op_tensors(dict(a=a, bres=bres, gamma=gamma, beta=beta, a_mask=a_mask, out_mask=out_mask, out=out),
                    dict(a=(B, C, L), bres=(B, C, L), gamma=(C,), beta=(C,), a_mask=(B, L), out_mask=(B, L), out=(B, C, L)), a.device)
    with _on(a.device):
        _check(lib().gtts_enc_layernorm(_ptr(a), _ptr(bres), _ptr(gamma), _ptr(beta), _ptr(a_mask), _ptr(out_mask), _ptr(out), B, C, L,
                                        float(eps), int(bool(relu_in)), int(bool(relu_out)), _stream()), "gtts_enc_layernorm")
    return out


def enc_attention(q, k, v, mask, emb_rel_k=None, emb_rel_v=None, n_heads=2, window=0, path=0, out=None):
    """The encoders' windowed relative-position attention kernel on its own: q, k, v [B,C,L], mask [B,L], emb_rel_k / emb_rel_v
    [2 window + 1, C / n_heads] (window 0: none) -> [B,C,L].  path 0: the kernel Encoder.forward would run; 16 / 8: that kernel
    (refused where it cannot serve the shape).  The launch gtts_enc_forward makes, for the per-op tests."""
    if not q.is_cuda:
        raise RuntimeError("the encoder kernels need HIP tensors (got %s); there is no CPU fallback here" % q.device)
    B, C, L = q.shape
    window = int(window or 0)
    if out is None:
        out = torch.empty((B, C, L), dtype=torch.float32, device=q.device)
    rel = (2 * window + 1, C // max(int(n_heads), 1))
    _enc_op_tensors(dict(q=q, k=k, v=v, mask=mask, emb_rel_k=emb_rel_k, emb_rel_v=emb_rel_v, out=out),
                    dict(q=(B, C, L), k=(B, C, L), v=(B, C, L), mask=(B, L), emb_rel_k=rel, emb_rel_v=rel, out=(B, C, L)), q.device)
    with _on(q.device):
        _check(lib().gtts_enc_attention(_ptr(q), _ptr(k), _ptr(v), _ptr(mask), _ptr(emb_rel_k), _ptr(emb_rel_v), _ptr(out), B, C, L,
                                        int(n_heads), window, int(path), _stream()), "gtts_enc_attention")
    return out


# ---- training of the two ops (csrc/enc_train.hip)
def enc_attention_train_ok(channels, n_heads, window, L):
    """Whether the training attention kernels hold this shape (a host call): 1 / 0."""
    return int(lib().gtts_enc_attention_train_ok(int(channels), int(n_heads), int(window or 0), int(L)))


def _att_train_shapes(q, n_heads, window):
    B, C, L = q.shape
    H = max(int(n_heads), 1)
    rel = (2 * window + 1, C // H)
    return B, C, L, H, dict(q=(B, C, L), k=(B, C, L), v=(B, C, L), mask=(B, L), emb_rel_k=rel, emb_rel_v=rel, drop=(B, H, L, L),
                            out=(B, C, L), stat=(B, H, L, 2), dout=(B, C, L), dq=(B, C, L), dk=(B, C, L), dv=(B, C, L), dek=rel, dev=rel)


def enc_attention_train_forward(q, k, v, mask, emb_rel_k=None, emb_rel_v=None, drop=None, n_heads=2, window=0, out=None, stat=None):
    """enc_attention for training: `drop` [B,H,L,L] (0 or 1 / (1 - p)) multiplies the probabilities after the softmax; returns
    (out [B,C,L], stat [B,H,L,2]: each query row's score maximum and reciprocal exponential sum, what the backward recomputes from)."""
    if not q.is_cuda:
        raise RuntimeError("the encoder kernels need HIP tensors (got %s); there is no CPU fallback here" % q.device)
    window = int(window or 0)
    B, C, L, H, shapes = _att_train_shapes(q, n_heads, window)
    if out is None:
        out = torch.empty((B, C, L), dtype=torch.float32, device=q.device)
    if stat is None:
        stat = torch.empty((B, H, L, 2), dtype=torch.float32, device=q.device)
    _enc_op_tensors(dict(q=q, k=k, v=v, mask=mask, emb_rel_k=emb_rel_k, emb_rel_v=emb_rel_v, drop=drop, out=out, stat=stat), shapes, q.device)
    with _on(q.device):
        _check(lib().gtts_enc_attention_train_forward(_ptr(q), _ptr(k), _ptr(v), _ptr(mask), _ptr(emb_rel_k), _ptr(emb_rel_v), _ptr(drop),
                                                      _ptr(out), _ptr(stat), B, C, L, int(n_heads), window, _stream()),
               "gtts_enc_attention_train_forward")
    return out, stat


def enc_attention_train_backward(q, k, v, mask, emb_rel_k, emb_rel_v, drop, stat, dout, n_heads=2, window=0, grads=None):
    """(dq, dk, dv, dek, dev) of enc_attention_train_forward from its inputs, `drop` and `stat` (dek = dev = None without a window).
    grads: optional dict of preallocated outputs by those names."""
    if not q.is_cuda:
        raise RuntimeError("the encoder kernels need HIP tensors (got %s); there is no CPU fallback here" % q.device)
    window = int(window or 0)
    B, C, L, H, shapes = _att_train_shapes(q, n_heads, window)
    g = dict(grads or {})
    for n in ("dq", "dk", "dv") + (("dek", "dev") if window else ()):
        if g.get(n) is None:
            g[n] = torch.empty(shapes[n], dtype=torch.float32, device=q.device)
    if not window:
        g["dek"] = g["dev"] = None
    _enc_op_tensors(dict(q=q, k=k, v=v, mask=mask, emb_rel_k=emb_rel_k, emb_rel_v=emb_rel_v, drop=drop, stat=stat, dout=dout, **g),
                    shapes, q.device)
    need = int(lib().gtts_enc_attention_train_scratch_bytes(B, C, L, int(n_heads), window))
    scratch = torch.empty(max(need, 4) // 4, dtype=torch.float32, device=q.device)
    with _on(q.device):
        _check(lib().gtts_enc_attention_train_backward(_ptr(q), _ptr(k), _ptr(v), _ptr(mask), _ptr(emb_rel_k), _ptr(emb_rel_v), _ptr(drop),
                                                       _ptr(stat), _ptr(dout), _ptr(g["dq"]), _ptr(g["dk"]), _ptr(g["dv"]), _ptr(g["dek"]),
                                                       _ptr(g["dev"]), _ptr(scratch), B, C, L, int(n_heads), window, _stream()),
               "gtts_enc_attention_train_backward")
    return g["dq"], g["dk"], g["dv"], g["dek"], g["dev"]


def enc_layernorm_backward(dout, a, gamma, beta, bres=None, a_mask=None, out_mask=None, eps=1e-4, relu_in=False, relu_out=False,
                           grads=None):
    """(da, dbres, dgamma, dbeta) of enc_layernorm (dbres None without bres).  grads: optional dict of preallocated outputs."""
    if not a.is_cuda:
        raise RuntimeError("the encoder kernels need HIP tensors (got %s); there is no CPU fallback here" % a.device)
    B, C, L = a.shape
    shapes = dict(dout=(B, C, L), a=(B, C, L), bres=(B, C, L), gamma=(C,), beta=(C,), a_mask=(B, L), out_mask=(B, L), da=(B, C, L),
                  dbres=(B, C, L), dgamma=(C,), dbeta=(C,))
    g = dict(grads or {})
    for n in ("da", "dgamma", "dbeta") + (("dbres",) if bres is not None else ()):
        if g.get(n) is None:
            g[n] = torch.empty(shapes[n], dtype=torch.float32, device=a.device)
    if bres is None:
        g["dbres"] = None
    _enc_op_tensors(dict(dout=dout, a=a, bres=bres, gamma=gamma, beta=beta, a_mask=a_mask, out_mask=out_mask, **g), shapes, a.device)
    need = int(lib().gtts_enc_layernorm_backward_scratch_floats(B, C, L))
    scratch = torch.empty(max(need, 1), dtype=torch.float32, device=a.device)
    with _on(a.device):
        _check(lib().gtts_enc_layernorm_backward(_ptr(dout), _ptr(a), _ptr(bres), _ptr(gamma), _ptr(beta), _ptr(a_mask), _ptr(out_mask),
                                                 _ptr(g["da"]), _ptr(g["dbres"]), _ptr(g["dgamma"]), _ptr(g["dbeta"]), _ptr(scratch), B, C, L,
                                                 float(eps), int(bool(relu_in)), int(bool(relu_out)), _stream()),
               "gtts_enc_layernorm_backward")
    return g["da"], g["dbres"], g["dgamma"], g["dbeta"]


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
        with torch.cuda.device(x.device):
            _check(lib().gtts_postnet_forward(self._h, _ptr(blob), _ptr(x), _ptr(mask), _ptr(out), _ptr(ws), ws.numel(), B, T,
                                              _stream()), "gtts_postnet_forward")
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
        with torch.cuda.device(blob.device):
            self._call("pack", self._h, _ptr(blob), _stream())
            torch.cuda.current_stream().synchronize()
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
        with _on(y.device):
            self._call("forward", self._h, _ptr(blob), _ptr(y), _ptr(lengths), _ptr(out), B, L, _stream())
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
        with _on(y.device):
            self._call("backward", self._h, _ptr(blob), _ptr(y), _ptr(lengths), _ptr(dmel), _ptr(dwav), _ptr(ws), ws.numel(), B, L,
                       _stream())
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
        with torch.cuda.device(blob.device):
            self._call("pack", self._h, _ptr(P), _ptr(blob), _stream())
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
        with _on(s.device):
            self._call("init", self._h, _ptr(blob), _ptr(s), _ptr(c), _ptr(x0), _ptr(ws), ws.numel(), B, T, _stream())
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
        with _on(c.device):
            self._call("step", self._h, _ptr(blob), _ptr(c), _ptr(x), _ptr(a_prev), _ptr(x_out), _ptr(a), _ptr(ws), ws.numel(), B, T,
                       _stream())
        return x_out, a

    def forward(self, blob, s, n_iters=32):
        """logmel [B, n_mels, T] -> waveform [B, L] after n_iters iterations, one launch each (n_iters = 0: the initial reconstruction)."""
        s, B, T, L = self._mel(s)
        ws = self.workspace(B, T, s.device)
        wav = torch.empty((B, L), dtype=torch.float32, device=s.device)
        with _on(s.device):
            self._call("forward", self._h, _ptr(blob), _ptr(s), _ptr(wav), _ptr(ws), ws.numel(), B, T, int(n_iters), _stream())
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
        with torch.cuda.device(blob.device):
            self._call("pack", self._h, _ptr(blob), _stream())
            torch.cuda.current_stream().synchronize()
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
        with _on(wavs.device):
            self._call("resample", self._h, _ptr(blob), _ptr(wavs), _ptr(out), _ptr(partials), B, L, _stream())
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
        with _on(wavs.device):
            self._call("normalize", self._h, _ptr(wavs), _ptr(partials), float(target_dBFS), 1 if increase_only else 2 if decrease_only else 0,
                       _ptr(out), _ptr(ws), 0 if ws is None else ws.numel(), B, L, _stream())
        return out

    def powmel(self, blob, wavs):
        """wavs [B, L] at sampling_rate -> power mel [B, frames(L), n_mels] in one launch."""
        wavs, B, L = self._rows(wavs)
        out = torch.empty((B, self.frames(L), self.n_mels), dtype=torch.float32, device=wavs.device)
        with _on(wavs.device):
            self._call("powmel", self._h, _ptr(blob), _ptr(wavs), _ptr(out), B, L, _stream())
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
        with _on(dev):
            self._call("forward", self._h, _ptr(blob), _ptr(frames), U, T_total, P, S, T, _ptr(embeds), _ptr(hidden), _ptr(utt),
                       _ptr(ws), ws.numel(), _stream())
        out = [embeds] + ([hidden] if want_hidden else []) + ([utt] if want_utt else [])
        return out[0] if len(out) == 1 else tuple(out)

    # ---- training (csrc/spk_train.hip)
    def pack_train(self, state, device):
        """The weights in the orders the backward reads (W_hh^T and W_ih^T as MFMA fragments, linear.weight): a blob of its own beside
        pack()'s, from the same state."""
        keep, arr = self._params(state, device)
        blob = torch.empty(int(lib().gtts_spktrain_packed_bytes(self._h)), dtype=torch.uint8, device=device)
        with torch.cuda.device(blob.device):
            _check(lib().gtts_spktrain_pack(self._h, arr, len(keep), _ptr(blob), _stream()), "gtts_spktrain_pack")
            torch.cuda.current_stream().synchronize()     # sources in `keep` may be temporaries
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
        with _on(dev):
            _check(lib().gtts_spktrain_forward(self._h, _ptr(blob), _ptr(frames), N, T, _ptr(embeds), _ptr(saved), saved.numel(),
                                                _stream()), "gtts_spktrain_forward")
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
        with _on(dev):
            _check(lib().gtts_spktrain_backward(self._h, _ptr(blob_train), _ptr(frames), _ptr(d_embeds), _ptr(saved), saved.numel(), arr,
                                           len(grads), _ptr(ws), ws.numel(), N, T, _stream()), "gtts_spktrain_backward")
        return grads


_GE2E_WS = {}       # the single live workspace of ge2e_loss: {(S, U, E, str(device)): uint8 tensor}


def ge2e_loss(embeds, w, b, want_grad=True):
    """GE2E similarity matrix, loss and gradient in one launch (csrc/spk_train.hip).  embeds [S, U, E], w and b one-element tensors on
    the same HIP device -> (sim [S * U, S], loss [1], d_embeds [S, U, E], dw [1], db [1]) for a loss gradient of 1; with
    want_grad=False the three gradients are None and their phases are skipped."""
    embeds, w, b = _f32c(embeds, "embeds"), _f32c(w, "w"), _f32c(b, "b")
    if embeds.dim() != 3:
        raise RuntimeError("embeds must be [speakers, utterances, embed] (got %s)" % (tuple(embeds.shape),))
    if w.numel() != 1 or b.numel() != 1 or w.device != embeds.device or b.device != embeds.device:
        raise RuntimeError("w and b must be one-element tensors on %s" % embeds.device)
    S, U, E = embeds.shape
    dev = embeds.device
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
    with _on(dev):
        _check(lib().gtts_ge2e_loss(_ptr(embeds), _ptr(w), _ptr(b), S, U, E, _ptr(sim), _ptr(loss), _ptr(d_embeds), _ptr(dw), _ptr(db),
                                    _ptr(ws), ws.numel(), _stream()), "gtts_ge2e_loss")
    return sim, loss, d_embeds, dw, db


def euler_step(xt, mu, est, mask, beta_t, h, noise=None):
    """In-place update of xt (one step of Diffusion.reverse_diffusion, diffusion.py:264-274)."""
    if not xt.is_cuda or xt.dtype != torch.float32 or not xt.is_contiguous():
        raise RuntimeError("xt must be a contiguous fp32 HIP tensor (updated in place)")
    mu, est, mask, noise = _f32c(mu, "mu"), _f32c(est, "est"), _f32c(mask, "mask"), _f32c(noise, "noise")
    B, F, T = xt.shape
    with torch.cuda.device(xt.device):
        _check(lib().gtts_euler_step(_ptr(xt), _ptr(mu), _ptr(est), _ptr(mask), _ptr(noise), float(beta_t), float(h),
                                     B, F, T, _stream()), "gtts_euler_step")
    return xt


def mas_maximum_path(value, mask):
    """monotonic_align.maximum_path(value, mask) (value, mask: [b, t_x, t_y]).

    HIP tensors run the GPU kernel.  Host tensors run the library's C++ twin gtts_mas_maximum_path_cpu -- the
    reference's wrapper accepts tensors on any device and always runs its Cython kernel on the host
    (monotonic_align/__init__.py:8-23); both are bit-identical to it."""
    v = value.detach().float().contiguous()
    m = mask.detach().to(device=v.device, dtype=torch.float32).contiguous()
    b, tx, ty = v.shape
    t_x = m.sum(1)[:, 0].to(torch.int32).contiguous()       # __init__.py:20-21
    t_y = m.sum(2)[:, 0].to(torch.int32).contiguous()
    path = torch.empty((b, tx, ty), dtype=torch.int32, device=v.device)
    if not v.is_cuda:
        _check(lib().gtts_mas_maximum_path_cpu(_ptr(v), _ptr(m), _ptr(t_x), _ptr(t_y), _ptr(path), b, tx, ty),
               "gtts_mas_maximum_path_cpu")
        return path.to(dtype=value.dtype)
    scratch = torch.empty(int(lib().gtts_mas_scratch_bytes(b, tx, ty)), dtype=torch.uint8, device=v.device)
    with torch.cuda.device(v.device):
        _check(lib().gtts_mas_maximum_path(_ptr(v), _ptr(m), _ptr(t_x), _ptr(t_y), _ptr(path), _ptr(scratch), b, tx,
                                           ty, _stream()), "gtts_mas_maximum_path")
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
    _check(getattr(lib(), "gtts_%s_pack" % family)(_ptr(src), _ptr(packed), cin, cout, (1 if transposed else 0) if up is None else up,
                                                   _stream()), "gtts_%s_pack" % family)
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
    L = lib()
    dev = specs[0][0].device
    sig = tuple([w.data_ptr() for w, *_ in specs])          # (cheap per-step check: the addresses the descriptor table holds)
    plan = getattr(specs, "plan", None)
    if plan is None or plan["sig"] != sig or plan["n"] != len(specs):
        plan = _build_pack_plan(specs, dev, sig)
        if isinstance(specs, PackSpecs):
            specs.plan = plan
    with _on(dev):
        _check(L.gtts_pack_batch(_ptr(plan["desc"]), plan["n"], plan["grid"], _stream()), "gtts_pack_batch")
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


def _out(out, name, shape, dtype, device, exc=RuntimeError):
    """A preallocated output of the caller's (`out` dict, tests place them between guard margins) or a fresh one."""
    t = None if out is None else out.get(name)
    if t is None:
        return torch.empty(shape, dtype=dtype, device=device)
    if tuple(t.shape) != tuple(shape) or t.dtype != dtype or t.device != device or not t.is_contiguous():
        raise exc("output %s must be a contiguous %s tensor of shape %s on %s" % (name, dtype, tuple(shape), device))
    return t


def _given(t, name, shape, device, dtype=torch.float32):
    """The caller's preallocated tensor `t` for the result `name` (tests place it between guard margins), or a fresh one: ValueError
    unless it is contiguous, of that shape and dtype, and on that device."""
    return _out(None if t is None else {name: t}, name, shape, dtype, device, exc=ValueError)


def _scratch(out, nbytes, device):
    """The workspace of a weight-gradient call: `out["workspace"]` (fp32, exactly the bytes the call asks for) or a fresh one."""
    if out is None or out.get("workspace") is None:
        return torch.empty(nbytes, dtype=torch.uint8, device=device)
    return _out(out, "workspace", (nbytes // 4,), torch.float32, device, exc=ValueError)


def _i32c(t, name, device):
    if not torch.is_tensor(t):
        t = torch.tensor(t, dtype=torch.int32)
    return t.to(device=device, dtype=torch.int32).contiguous()


def _hip_only(t, what):
    if not t.is_cuda:
        raise RuntimeError("%s needs HIP tensors (got %s); there is no CPU fallback" % (what, t.device))


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


def _conv_run(kind, x, mask_cols, weight, bias, transposed, x1=None, out_mask=None, out=None):
    _, two, om, name, _, _ = _CONV_KINDS[kind]
    B, c0, H, W = x.shape
    cin = c0 + (int(x1.shape[1]) if x1 is not None else 0)
    cout = weight.shape[1] if transposed else weight.shape[0]
    y = _given(out, "out", (B, cout, H, W), x.device)
    src = (_ptr(x), _ptr(x1), c0, _ptr(mask_cols)) if two else (_ptr(x), _ptr(mask_cols))
    with _on(x.device):
        packed = _packed_weight(weight, cin, cout, transposed, kind)
        _check(getattr(lib(), name)(*src, *((_ptr(out_mask),) if om else ()), _ptr(packed), _ptr(bias), _ptr(y), B, cin, cout, H, W,
                                    _stream()), name)
    return y


def _conv_dgrad(kind, dy, weight, mask_cols, out=None):
    dy, weight = _f32c(dy, "dy"), _f32c(weight, "weight")
    B, cout, H, W = dy.shape
    return _conv_run(kind, dy, _const(dy.device, "ones", B, W), weight, _const(dy.device, "zeros", int(weight.shape[1])), True,
                     out_mask=_f32c(mask_cols, "mask"), out=out)


def _tiled_wgrad(kind, x, mask_cols, dy, x1=None, want_bias=True, out=None):
    """(dW [cout,cin,k,k], db [cout] or None) by the kind's LDS-tiled deterministic reduction (train_wgrad.hip, train_wgrad7.hip).
    `out`: optional dict of preallocated dw / db / workspace (fp32, gtts_conv<kind>_wgrad_workspace_bytes / 4 floats)."""
    ksize, two, _, _, name, ws_name = _CONV_KINDS[kind]
    B, c0, H, W = x.shape
    cin = c0 + (int(x1.shape[1]) if x1 is not None else 0)
    cout = int(dy.shape[1])
    dw = _out(out, "dw", (cout, cin, ksize, ksize), torch.float32, x.device, exc=ValueError)
    db = _out(out, "db", (cout,), torch.float32, x.device, exc=ValueError) if want_bias else None
    src = (_ptr(x), _ptr(x1), c0) if two else (_ptr(x),)
    with _on(x.device):
        L = lib()
        nws = int(getattr(L, ws_name)(B, cin, cout, H, W))
        ws = _scratch(out, nws, x.device)
        _check(getattr(L, name)(*src, _ptr(mask_cols), _ptr(dy), _ptr(dw), _ptr(db), _ptr(ws), nws, B, cin, cout, H, W, _stream()), name)
    return dw, db


def _wgrad_small(x, mask_cols, dy, ksize, want_bias=True, out=None):
    """The first layer's weight gradient (cin 2 or 3: its own kernel).  `out`: optional dict of preallocated dw / db / workspace
    (gtts_conv_wgrad_small_scratch_floats floats)."""
    B, cin, H, W = x.shape
    cout = int(dy.shape[1])
    dw = _out(out, "dw", (cout, cin, ksize, ksize), torch.float32, x.device, exc=ValueError)
    db = _out(out, "db", (cout,), torch.float32, x.device, exc=ValueError) if want_bias else None
    with _on(x.device):
        scratch = _out(out, "workspace", (int(lib().gtts_conv_wgrad_small_scratch_floats(B, cin, cout, ksize)),), torch.float32, x.device,
                       exc=ValueError)
        _check(lib().gtts_conv_wgrad_small(_ptr(x), _ptr(mask_cols), _ptr(dy), _ptr(dw), _ptr(db), _ptr(scratch), B, cin, cout, H, W, ksize,
                                           _stream()), "gtts_conv_wgrad_small")
    return dw, db


def conv3x3_masked(x, mask_cols, weight, bias, x1=None, out=None):
    """Conv2d_3x3(cat(x, x1) * mask) + bias (Block.forward, diffusion.py:56-57; the concatenation of the up path, :166, is read in
    place): x [B,c0,H,W], x1 [B,c1,H,W] or None, mask_cols [B,W], weight [cout,c0+c1,3,3].  `out`: optional preallocated result."""
    x, mask_cols, weight, bias = _f32c(x, "x"), _f32c(mask_cols, "mask"), _f32c(weight, "weight"), _f32c(bias, "bias")
    if x1 is None and conv3x3_narrow(weight.shape[1], weight.shape[0]):
        return conv3x3_narrow_forward(x, mask_cols, weight, bias, out=None if out is None else {"out": out})
    return _conv_run("3x3", x, mask_cols, weight, bias, False, _f32c(x1, "x1"), out=out)


def conv3x3_dgrad(dy, weight, mask_cols=None, out=None):
    """Gradient of conv3x3_masked w.r.t. (x * mask): a 3x3 convolution of dy with the transposed, flipped weights; with
    mask_cols [B,W] the gradient w.r.t. x itself (the mask is applied in the kernel's epilogue).  `out`: optional preallocated result."""
    if conv3x3_narrow(weight.shape[1], weight.shape[0]):
        return conv3x3_narrow_dgrad(dy, weight, mask_cols, out=None if out is None else {"dx": out})
    return _conv_dgrad("3x3", dy, weight, mask_cols, out=out)


def conv3x3_wgrad(x, mask_cols, dy, x1=None, out=None):
    """(dW [cout,cin,3,3], db [cout]) of conv3x3_masked (x1: second source of a concatenated input, c0 a multiple of 64).  `out`:
    optional dict of preallocated dw / db / workspace."""
    x, mask_cols, dy, x1 = _f32c(x, "x"), _f32c(mask_cols, "mask"), _f32c(dy, "dy"), _f32c(x1, "x1")
    cin, cout = int(x.shape[1]) + (int(x1.shape[1]) if x1 is not None else 0), int(dy.shape[1])
    if cin in (2, 3) and x1 is None:
        return _wgrad_small(x, mask_cols, dy, 3, out=out)
    if x1 is None and conv3x3_narrow(cin, cout):
        return conv3x3_narrow_wgrad(x, mask_cols, dy, out=out)
    if cin % 64 or cout % 64:
        raise ValueError("conv3x3_wgrad: cin and cout must be multiples of 64, or cin 2 or 3 from one source (got cin %d, cout %d)"
                         % (cin, cout))
    return _tiled_wgrad("3x3", x, mask_cols, dy, x1, out=out)


def _narrow_ws(out, B, cin, cout, H, W, op, device):
    nws = int(lib().gtts_conv3x3_narrow_workspace_bytes(B, cin, cout, H, W, op))
    if nws == 0:
        raise ValueError("the narrow 3x3 kernels take cin 1 or 32 (the data gradient: 32) and cout 64 or 128 (got cin %d, cout %d, B %d, "
                         "%d x %d)" % (cin, cout, B, H, W))
    return _scratch(out, nws, device), nws


def conv3x3_narrow_forward(x, mask_cols, weight, bias, out_mask=None, out=None):
    """Conv2d_3x3(x * mask) + bias [times out_mask] for RefBlock's narrow layers (cin 1 or 32, cout 64 or 128) on csrc/train_narrow.hip:
    x [B,cin,H,W], mask_cols / out_mask [B,W], weight [cout,cin,3,3] as the module holds it.  `out`: optional dict of a preallocated
    out / workspace (fp32, gtts_conv3x3_narrow_workspace_bytes / 4 floats)."""
    _hip_only(x, "conv3x3_narrow_forward")
    x, mask_cols, weight, bias = _f32c(x, "x"), _f32c(mask_cols, "mask"), _f32c(weight, "weight"), _f32c(bias, "bias")
    B, cin, H, W = x.shape
    cout = int(weight.shape[0])
    if tuple(weight.shape) != (cout, cin, 3, 3) or tuple(mask_cols.shape) != (B, W) or tuple(bias.shape) != (cout,):
        raise ValueError("conv3x3_narrow_forward: x %s, weight %s, bias %s and mask %s do not match" %
                         (tuple(x.shape), tuple(weight.shape), tuple(bias.shape), tuple(mask_cols.shape)))
    y = _out(out, "out", (B, cout, H, W), torch.float32, x.device, exc=ValueError)
    with _on(x.device):
        ws, nws = _narrow_ws(out, B, cin, cout, H, W, 0, x.device)
        _check(lib().gtts_conv3x3_narrow_forward(_ptr(x), _ptr(mask_cols), _ptr(_f32c(out_mask, "out_mask")), _ptr(weight), _ptr(bias), _ptr(y),
                                                 _ptr(ws), nws, B, cin, cout, H, W, _stream()), "gtts_conv3x3_narrow_forward")
    return y


def conv3x3_narrow_dgrad(dy, weight, mask_cols=None, out_mask=None, out=None):
    """dx [B,cin,H,W] of conv3x3_narrow_forward (cin 32): mask_cols (None: ones) is the forward's input mask, out_mask its output mask.
    `out`: optional dict of a preallocated dx / workspace."""
    _hip_only(dy, "conv3x3_narrow_dgrad")
    dy, weight = _f32c(dy, "dy"), _f32c(weight, "weight")
    B, cout, H, W = dy.shape
    cin = int(weight.shape[1])
    if tuple(weight.shape) != (cout, cin, 3, 3):
        raise ValueError("conv3x3_narrow_dgrad: weight %s does not match dy %s" % (tuple(weight.shape), tuple(dy.shape)))
    mask_cols = _const(dy.device, "ones", B, W) if mask_cols is None else _f32c(mask_cols, "mask")
    dx = _out(out, "dx", (B, cin, H, W), torch.float32, dy.device, exc=ValueError)
    with _on(dy.device):
        ws, nws = _narrow_ws(out, B, cin, cout, H, W, 1, dy.device)
        _check(lib().gtts_conv3x3_narrow_dgrad(_ptr(dy), _ptr(_f32c(out_mask, "out_mask")), _ptr(mask_cols), _ptr(weight), _ptr(dx), _ptr(ws),
                                               nws, B, cin, cout, H, W, _stream()), "gtts_conv3x3_narrow_dgrad")
    return dx


def conv3x3_narrow_wgrad(x, mask_cols, dy, out_mask=None, want_bias=True, out=None):
    """(dW [cout,cin,3,3], db [cout] or None) of conv3x3_narrow_forward.  `out`: optional dict of preallocated dw / db / workspace."""
    _hip_only(x, "conv3x3_narrow_wgrad")
    x, mask_cols, dy = _f32c(x, "x"), _f32c(mask_cols, "mask"), _f32c(dy, "dy")
    B, cin, H, W = x.shape
    cout = int(dy.shape[1])
    if tuple(dy.shape) != (B, cout, H, W) or tuple(mask_cols.shape) != (B, W):
        raise ValueError("conv3x3_narrow_wgrad: x %s, dy %s and mask %s do not match" % (tuple(x.shape), tuple(dy.shape), tuple(mask_cols.shape)))
    dw = _out(out, "dw", (cout, cin, 3, 3), torch.float32, x.device, exc=ValueError)
    db = _out(out, "db", (cout,), torch.float32, x.device, exc=ValueError) if want_bias else None
    with _on(x.device):
        ws, nws = _narrow_ws(out, B, cin, cout, H, W, 2, x.device)
        _check(lib().gtts_conv3x3_narrow_wgrad(_ptr(x), _ptr(mask_cols), _ptr(_f32c(out_mask, "out_mask")), _ptr(dy), _ptr(dw), _ptr(db),
                                               _ptr(ws), nws, B, cin, cout, H, W, _stream()), "gtts_conv3x3_narrow_wgrad")
    return dw, db


def conv7x7_supported(cin, cout, need_dgrad=True, shape=None):
    """Channel counts (and, with shape = (B, H, W), tensor sizes) the 7x7 training kernels take (DiffVC PostNet Block): forward,
    data gradient and weight gradient all work on whole 64-channel tiles."""
    if shape is not None and not conv_size_ok(shape[0], cin, cout, shape[1], shape[2]):
        return False
    return int(cin) > 0 and int(cout) > 0 and int(cin) % 64 == 0 and int(cout) % 64 == 0


def conv7x7_masked(x, mask_cols, weight, bias, out=None):
    """Conv2d_7x7(x * mask, padding 3) + bias (PostNet Block, DiffVC/model/postnet.py:21-23): x [B,cin,H,W], mask_cols [B,W],
    weight [cout,cin,7,7].  `out`: optional preallocated result."""
    x, mask_cols, weight, bias = _f32c(x, "x"), _f32c(mask_cols, "mask"), _f32c(weight, "weight"), _f32c(bias, "bias")
    return _conv_run("7x7", x, mask_cols, weight, bias, False, out=out)


def conv7x7_dgrad(dy, weight, mask_cols=None, out=None):
    """Gradient of conv7x7_masked w.r.t. (x * mask): a 7x7 convolution of dy with the transposed, flipped weights; with mask_cols
    [B,W] the gradient w.r.t. x itself (the mask is applied in the kernel's epilogue).  `out`: optional preallocated result."""
    return _conv_dgrad("7x7", dy, weight, mask_cols, out=out)


def conv7x7_wgrad(x, mask_cols, dy, out=None):
    """(dW [cout,cin,7,7], db [cout]) of conv7x7_masked (train_wgrad7.hip: deterministic split-bf16 MFMA reduction).  `out`: optional
    dict of preallocated dw / db / workspace."""
    return _tiled_wgrad("7x7", _f32c(x, "x"), _f32c(mask_cols, "mask"), _f32c(dy, "dy"), out=out)


def postnet_expand(x, mask, w, bias=None, out=None):
    """out [B,C,F,T] = w[c] * x[b,f,t] * mask[b,t] + bias[c] (PostNet init_conv; final_conv's data gradient with bias None).  `out`:
    optional preallocated result."""
    x, mask, w = _f32c(x, "x"), _f32c(mask, "mask"), _f32c(w, "weight")
    B, F, T = x.shape
    C = int(w.numel())
    bias = _const(x.device, "zeros", C) if bias is None else _f32c(bias, "bias")
    out = _given(out, "out", (B, C, F, T), x.device)
    with _on(x.device):
        _check(lib().gtts_postnet_expand(_ptr(x), _ptr(mask), _ptr(w), _ptr(bias), _ptr(out), B, C, F, T, _stream()), "gtts_postnet_expand")
    return out


def postnet_collapse(x, mask, w, bias=None, out=None):
    """out [B,F,T] = sum_c w[c] * x[b,c,f,t] * mask[b,t] + bias (PostNet final_conv; init_conv's data gradient with bias None).  `out`:
    optional preallocated result."""
    x, mask, w = _f32c(x, "x"), _f32c(mask, "mask"), _f32c(w, "weight")
    B, C, F, T = x.shape
    bias = _const(x.device, "zeros", 1) if bias is None else _f32c(bias, "bias")
    out = _given(out, "out", (B, F, T), x.device)
    with _on(x.device):
        _check(lib().gtts_postnet_collapse(_ptr(x), _ptr(mask), _ptr(w), _ptr(bias), _ptr(out), B, C, F, T, _stream()), "gtts_postnet_collapse")
    return out


def postnet_chan_dot(a, v, mask, want_dot=True, want_sum=True, out=None):
    """(dot [C], sum [C]) over a [B,C,F,T]: dot[c] = sum a[b,c] * v[b] * mask[b,t] (v [B,F,T], v / mask None: 1), sum[c] = sum a[b,c]
    (fixed-order reduction; an output not wanted is None).  `out`: optional dict of preallocated dot / sum / workspace
    (gtts_postnet_chan_dot_scratch_floats floats)."""
    a, v, mask = _f32c(a, "a"), _f32c(v, "v"), _f32c(mask, "mask")
    B, C, F, T = a.shape
    dot = _out(out, "dot", (C,), torch.float32, a.device, exc=ValueError) if want_dot else None
    sm = _out(out, "sum", (C,), torch.float32, a.device, exc=ValueError) if want_sum else None
    with _on(a.device):
        scratch = _out(out, "workspace", (int(lib().gtts_postnet_chan_dot_scratch_floats(B, C, F, T)),), torch.float32, a.device,
                       exc=ValueError)
        _check(lib().gtts_postnet_chan_dot(_ptr(a), _ptr(v), _ptr(mask), _ptr(dot), _ptr(sm), _ptr(scratch), B, C, F, T, _stream()),
               "gtts_postnet_chan_dot")
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
    x, weight = _f32c(x, "x"), _f32c(weight, "weight")
    B, W = int(x.shape[0]), int(x.shape[3])
    mask_cols = _const(x.device, "ones", B, W) if mask_cols is None else _f32c(mask_cols, "mask")
    bias = _const(x.device, "zeros", int(weight.shape[0])) if bias is None else _f32c(bias, "bias")
    return _conv_run("1x1", x, mask_cols, weight, bias, False, out=out)


def conv1x1_dgrad(dy, weight, mask_cols=None, out=None):
    """Gradient of conv1x1_masked w.r.t. x: the 1x1 convolution of dy * mask (columns do not mix) with the transposed weight.  `out`:
    optional preallocated result."""
    dy, weight = _f32c(dy, "dy"), _f32c(weight, "weight")
    B, W = int(dy.shape[0]), int(dy.shape[3])
    mask_cols = _const(dy.device, "ones", B, W) if mask_cols is None else _f32c(mask_cols, "mask")
    return _conv_run("1x1", dy, mask_cols, weight, _const(dy.device, "zeros", int(weight.shape[1])), True, out=out)


def conv1x1_wgrad(x, mask_cols, dy, want_bias=True, out=None):
    """(dW [cout,cin,1,1], db [cout] or None) of conv1x1_masked.  `out`: optional dict of preallocated dw / db / workspace."""
    x, mask_cols, dy = _f32c(x, "x"), _f32c(mask_cols, "mask"), _f32c(dy, "dy")
    if x.shape[1] in (2, 3):
        return _wgrad_small(x, _const(x.device, "ones", int(x.shape[0]), int(x.shape[3])) if mask_cols is None else mask_cols, dy, 1, want_bias,
                            out=out)
    return _tiled_wgrad("1x1", x, mask_cols, dy, want_bias=want_bias, out=out)


def add_masked(a, b, mask_cols, channels=None, out=None):
    """a + b * mask (a None: b * mask; mask_cols None: a + b) over [B,C,H,W] with mask_cols [B,W].  channels = (c_begin, c_end):
    b is that channel range of a wider contiguous tensor (read in place; the result is contiguous).  `out`: optional preallocated result."""
    a, b, mask_cols = _f32c(a, "a"), _f32c(b, "b"), _f32c(mask_cols, "mask")
    B, Cb, H, W = b.shape
    c0, c1 = (0, Cb) if channels is None else channels
    out = _given(out, "out", (B, c1 - c0, H, W), b.device)
    with _on(b.device):
        _check(lib().gtts_add_masked(_ptr(a), ctypes.c_void_p(b.data_ptr() + 4 * c0 * H * W), _ptr(mask_cols), _ptr(out), B, c1 - c0, H, W,
                                     0 if channels is None else Cb, _stream()), "gtts_add_masked")
    return out


def zero_insert2(x, out=None):
    """[B,C,h,w] -> [B,C,2h,2w] with x at the even positions and zeros elsewhere.  `out`: optional preallocated result."""
    x = _f32c(x, "x")
    B, C, h, w = x.shape
    out = _given(out, "out", (B, C, 2 * h, 2 * w), x.device)
    with _on(x.device):
        _check(lib().gtts_zero_insert2(_ptr(x), _ptr(out), B, C, h, w, _stream()), "gtts_zero_insert2")
    return out


def space_to_depth2(x, out=None):
    """[B,C,2h,2w] -> [B,4C,h,w]: channel block (pr * 2 + pc) holds rows 2y + 1 - pr and columns 2x + 1 - pc.  `out`: optional
    preallocated result."""
    x = _f32c(x, "x")
    B, C, H2, W2 = x.shape
    if H2 % 2 or W2 % 2:
        raise ValueError("space_to_depth2: even height and width expected, got %d x %d" % (H2, W2))
    out = _given(out, "out", (B, 4 * C, H2 // 2, W2 // 2), x.device)
    with _on(x.device):
        _check(lib().gtts_space_to_depth2(_ptr(x), _ptr(out), B, C, H2 // 2, W2 // 2, _stream()), "gtts_space_to_depth2")
    return out


def final_conv_forward(x, weight, bias, mask_cols, out=None):
    """(Conv2d_1x1(x * mask) + bias) * mask for the 64 -> 1 final convolution (diffusion.py:175-176): [B,1,H,W].  `out`: optional
    preallocated result."""
    x, weight, bias, mask_cols = _f32c(x, "x"), _f32c(weight, "weight"), _f32c(bias, "bias"), _f32c(mask_cols, "mask")
    B, C, H, W = x.shape
    out = _given(out, "out", (B, 1, H, W), x.device)
    with _on(x.device):
        _check(lib().gtts_final_conv_forward(_ptr(x), _ptr(weight), _ptr(bias), _ptr(mask_cols), _ptr(out), B, C, H, W, _stream()),
               "gtts_final_conv_forward")
    return out


def final_conv_backward(x, weight, mask_cols, dout, out=None):
    """(dx, dweight [1,C,1,1], dbias [1]) of final_conv_forward.  `out`: optional dict of preallocated dx / dw / db / workspace
    (gtts_final_conv_scratch_floats floats)."""
    x, weight, mask_cols, dout = _f32c(x, "x"), _f32c(weight, "weight"), _f32c(mask_cols, "mask"), _f32c(dout, "dout")
    B, C, H, W = x.shape
    dx = _out(out, "dx", (B, C, H, W), torch.float32, x.device, exc=ValueError)
    dw = _out(out, "dw", (1, C, 1, 1), torch.float32, x.device, exc=ValueError)
    db = _out(out, "db", (1,), torch.float32, x.device, exc=ValueError)
    with _on(x.device):
        scratch = _out(out, "workspace", (int(lib().gtts_final_conv_scratch_floats(B, C, H, W)),), torch.float32, x.device, exc=ValueError)
        _check(lib().gtts_final_conv_backward(_ptr(x), _ptr(weight), _ptr(mask_cols), _ptr(dout), _ptr(dx), _ptr(dw), _ptr(db),
                                              _ptr(scratch), B, C, H, W, _stream()), "gtts_final_conv_backward")
    return dx, dw, db


def resample_supported(cin, cout, H, W, up, B=1):
    # largest tensor of the call and of its gradients: Upsample's output (and its space_to_depth planes) is 4 cout planes of H x W
    if not conv_size_ok(B, 4 * max(cin, cout) if up else max(cin, cout), 1, H, W):
        return False
    return _tiles(cin) and _tiles(cout) and (up or (H % 2 == 0 and W % 2 == 0))


def conv_resample(x, mask_cols, weight, bias, up, dgrad_of_down=False, out=None):
    """Downsample (up False: Conv2d 3x3 stride 2 pad 1, weight [cout,cin,3,3]) or Upsample (up True: ConvTranspose2d 4x4 stride 2
    pad 1, weight [cin,cout,4,4]) of x * mask (diffusion.py:19-34).  dgrad_of_down: x is the gradient of a Downsample output and
    weight that Downsample's forward weight; the result is its data gradient (an Upsample with the zero-padded kernel).  `out`: optional
    preallocated result."""
    x, mask_cols, weight = _f32c(x, "x"), _f32c(mask_cols, "mask"), _f32c(weight, "weight")
    B, cin, H, W = x.shape
    if dgrad_of_down:
        cout, kind, up = int(weight.shape[1]), "dn_T", True
    else:
        cout, kind = (int(weight.shape[1]), "up") if up else (int(weight.shape[0]), "dn")
    bias = _const(x.device, "zeros", cout) if bias is None else _f32c(bias, "bias")
    y = _given(out, "out", (B, cout, 2 * H, 2 * W) if up else (B, cout, H // 2, W // 2), x.device)
    with _on(x.device):
        packed = _packed_weight(weight, cin, cout, False, kind)
        _check(lib().gtts_conv_resample(_ptr(x), _ptr(mask_cols), _ptr(packed), _ptr(bias), _ptr(y), B, cin, cout, H, W, 1 if up else 0,
                                        _stream()), "gtts_conv_resample")
    return y


def attn_train_forward(qkv, out=None):
    """LinearAttention core (diffusion.py:90-100) on to_qkv's output qkv [B,384,H,W]: (out [B,128,H,W], ctx [B,4,32,32],
    stat [B,4,32,2] = softmax row maxima and reciprocal sums).  `out`: optional dict of preallocated out / ctx / stat."""
    qkv = _f32c(qkv, "qkv")
    B, C3, H, W = qkv.shape
    if C3 != 384:
        raise ValueError("attn_train_forward: to_qkv output must have 3 x 4 heads x 32 = 384 channels, got %d" % C3)
    N = H * W
    res = _out(out, "out", (B, 128, H, W), torch.float32, qkv.device)
    ctx = _out(out, "ctx", (B, 4, 32, 32), torch.float32, qkv.device)
    stat = _out(out, "stat", (B, 4, 32, 2), torch.float32, qkv.device)
    with _on(qkv.device):
        scratch = torch.empty(int(lib().gtts_attn_train_scratch_floats(B, N)), dtype=torch.float32, device=qkv.device)
        _check(lib().gtts_attn_train_forward(_ptr(qkv), _ptr(res), _ptr(ctx), _ptr(stat), _ptr(scratch), B, N, _stream()),
               "gtts_attn_train_forward")
    return res, ctx, stat


def attn_train_backward(qkv, dout, ctx, stat, out=None):
    """d qkv of attn_train_forward given d out.  `out`: optional dict with a preallocated dqkv."""
    qkv, dout = _f32c(qkv, "qkv"), _f32c(dout, "dout")
    B, C3, H, W = qkv.shape
    N = H * W
    dqkv = _out(out, "dqkv", tuple(qkv.shape), torch.float32, qkv.device)
    dctx = torch.empty((B, 4, 32, 32), dtype=torch.float32, device=qkv.device)
    rdot = torch.empty((B, 4, 32), dtype=torch.float32, device=qkv.device)
    with _on(qkv.device):
        scratch = torch.empty(int(lib().gtts_attn_train_scratch_floats(B, N)), dtype=torch.float32, device=qkv.device)
        _check(lib().gtts_attn_train_backward(_ptr(qkv), _ptr(dout), _ptr(ctx), _ptr(stat), _ptr(dqkv), _ptr(dctx), _ptr(rdot),
                                              _ptr(scratch), B, N, _stream()), "gtts_attn_train_backward")
    return dqkv


def rezero_forward(f, g, x, out=None):
    """f * g + x (Rezero + Residual, diffusion.py:40-46,103-108); g a 1-element device tensor.  `out`: optional dict with a
    preallocated y."""
    f, x, g = _f32c(f, "f"), _f32c(x, "x"), _f32c(g, "g")
    y = _out(out, "y", tuple(f.shape), torch.float32, f.device)
    with _on(f.device):
        _check(lib().gtts_rezero_forward(_ptr(f), _ptr(x), _ptr(g), _ptr(y), f.numel(), _stream()), "gtts_rezero_forward")
    return y


def rezero_backward(dy, f, g, out=None):
    """(d f = dy * g, d g = sum(dy * f)) of rezero_forward.  `out`: optional dict of preallocated df / dg."""
    dy, f, g = _f32c(dy, "dy"), _f32c(f, "f"), _f32c(g, "g")
    df = _out(out, "df", tuple(f.shape), torch.float32, f.device)
    dg = _out(out, "dg", tuple(g.shape), torch.float32, f.device)
    with _on(f.device):
        scratch = torch.empty(int(lib().gtts_rezero_scratch_bytes(f.numel())), dtype=torch.uint8, device=f.device)
        _check(lib().gtts_rezero_backward(_ptr(dy), _ptr(f), _ptr(g), _ptr(df), _ptr(dg), _ptr(scratch), f.numel(), _stream()),
               "gtts_rezero_backward")
    return df, dg


def gn_mish_forward(y, gamma, beta, mask_cols, groups, eps, tb=None, out=None):
    """(Mish(GroupNorm(y)) * mask [+ tb[:, :, None, None]], stats: (mean, rstd) pairs followed by reduction scratch) -- Block.forward
    after the convolution (diffusion.py:53-58) and, with tb [B,C], ResnetBlock's time term (diffusion.py:75-76).  `out`: optional dict of
    preallocated out / stats."""
    y, gamma, beta, mask_cols, tb = _f32c(y, "y"), _f32c(gamma, "gamma"), _f32c(beta, "beta"), _f32c(mask_cols, "mask"), _f32c(tb, "tb")
    B, C, H, W = y.shape
    res = _out(out, "out", (B, C, H, W), torch.float32, y.device)
    stats = _out(out, "stats", (int(lib().gtts_gn_mish_stats_floats(B, int(groups))),), torch.float32, y.device)
    with _on(y.device):
        _check(lib().gtts_gn_mish_forward(_ptr(y), _ptr(gamma), _ptr(beta), _ptr(mask_cols), _ptr(tb), _ptr(res), _ptr(stats), B, C,
                                          H, W, int(groups), float(eps), _stream()), "gtts_gn_mish_forward")
    return res, stats


def gn_mish_backward(dout, y, gamma, beta, mask_cols, stats, groups, want_dtb=False, out=None):
    """(dy, dgamma, dbeta[, dtb [B,C]]) of gn_mish_forward.  `out`: optional dict of preallocated dy / dgamma / dbeta / dtb."""
    dout, y = _f32c(dout, "dout"), _f32c(y, "y")
    B, C, H, W = y.shape
    dy = _out(out, "dy", (B, C, H, W), torch.float32, y.device)
    dg = _out(out, "dgamma", (C,), torch.float32, y.device)
    db = _out(out, "dbeta", (C,), torch.float32, y.device)
    dtb = _out(out, "dtb", (B, C), torch.float32, y.device) if want_dtb else None
    scratch = torch.empty(int(lib().gtts_gn_mish_scratch_bytes(B, C)), dtype=torch.uint8, device=y.device)
    with _on(y.device):
        _check(lib().gtts_gn_mish_backward(_ptr(dout), _ptr(y), _ptr(_f32c(gamma, "gamma")), _ptr(_f32c(beta, "beta")),
                                           _ptr(_f32c(mask_cols, "mask")), _ptr(stats), _ptr(dy), _ptr(dg), _ptr(db), _ptr(dtb),
                                           _ptr(scratch), B, C, H, W, int(groups), _stream()), "gtts_gn_mish_backward")
    return (dy, dg, db, dtb) if want_dtb else (dy, dg, db)


def in_glu_forward(y, gamma, beta, eps=1e-5, tb=None, out=None):
    """(IN(y[:, :C]) * sigmoid(IN(y[:, C:])) [+ tb[:, :, None, None]], stats) -- InstanceNorm2d(affine) + GLU(dim=1) of DiffVC's RefBlock
    (modules.py:128-157) and, with tb [B,C], its time-bias add (modules.py:159,162).  `out`: optional dict of preallocated out / stats."""
    y, gamma, beta, tb = _f32c(y, "y"), _f32c(gamma, "gamma"), _f32c(beta, "beta"), _f32c(tb, "tb")
    B, C2, H, W = y.shape
    C = C2 // 2
    if tb is not None and tuple(tb.shape) != (B, C):
        raise ValueError("tb %s does not match y %s" % (tuple(tb.shape), tuple(y.shape)))
    res = _out(out, "out", (B, C, H, W), torch.float32, y.device)
    stats = _out(out, "stats", (int(lib().gtts_in_glu_stats_floats(B, C)),), torch.float32, y.device)
    with _on(y.device):
        if tb is None:
            _check(lib().gtts_in_glu_forward(_ptr(y), _ptr(gamma), _ptr(beta), _ptr(res), _ptr(stats), B, C, H, W, float(eps), _stream()),
                   "gtts_in_glu_forward")
        else:
            _check(lib().gtts_in_glu_tb_forward(_ptr(y), _ptr(gamma), _ptr(beta), _ptr(tb), _ptr(res), _ptr(stats), B, C, H, W, float(eps),
                                                _stream()), "gtts_in_glu_tb_forward")
    return res, stats


def in_glu_backward(dout, y, gamma, beta, stats, want_dtb=False, out=None):
    """(dy, dgamma, dbeta[, dtb [B,C]]) of in_glu_forward.  `out`: optional dict of preallocated dy / dgamma / dbeta / dtb."""
    dout, y, gamma, beta = _f32c(dout, "dout"), _f32c(y, "y"), _f32c(gamma, "gamma"), _f32c(beta, "beta")
    B, C2, H, W = y.shape
    C = C2 // 2
    dy = _out(out, "dy", (B, C2, H, W), torch.float32, y.device)
    dg = _out(out, "dgamma", (C2,), torch.float32, y.device)
    db = _out(out, "dbeta", (C2,), torch.float32, y.device)
    dtb = _out(out, "dtb", (B, C), torch.float32, y.device) if want_dtb else None
    scratch = torch.empty(int(lib().gtts_in_glu_scratch_floats(B, C)), dtype=torch.float32, device=y.device)
    with _on(y.device):
        if want_dtb:
            _check(lib().gtts_in_glu_tb_backward(_ptr(dout), _ptr(y), _ptr(gamma), _ptr(beta), _ptr(stats), _ptr(dy), _ptr(dg), _ptr(db),
                                                 _ptr(dtb), _ptr(scratch), B, C, H, W, _stream()), "gtts_in_glu_tb_backward")
        else:
            _check(lib().gtts_in_glu_backward(_ptr(dout), _ptr(y), _ptr(gamma), _ptr(beta), _ptr(stats), _ptr(dy), _ptr(dg), _ptr(db),
                                              _ptr(scratch), B, C, H, W, _stream()), "gtts_in_glu_backward")
    return (dy, dg, db, dtb) if want_dtb else (dy, dg, db)


def cond_field(U, mask_cols, H, base=None, out=None):
    """base + the bias field of a condition vector convolved over the [H, W] plane (gtts_cond_field_forward): U [B,taps,C] with taps 9
    ((kh, kw) order, 3x3 with padding 1) or 1 (1x1), mask_cols [B,W], base [B,C,H,W] or None -> [B,C,H,W].  `out`: optional dict of a
    preallocated out."""
    _hip_only(U, "cond_field")
    U, mask_cols, base = _f32c(U, "U"), _f32c(mask_cols, "mask"), _f32c(base, "base")
    B, taps, C = U.shape
    W = int(mask_cols.shape[-1])
    if tuple(mask_cols.shape) != (B, W) or (base is not None and tuple(base.shape) != (B, C, int(H), W)):
        raise ValueError("cond_field: U %s, mask %s and base %s do not match" % (tuple(U.shape), tuple(mask_cols.shape),
                                                                                 None if base is None else tuple(base.shape)))
    res = _out(out, "out", (B, C, int(H), W), torch.float32, U.device, exc=ValueError)
    with _on(U.device):
        _check(lib().gtts_cond_field_forward(_ptr(U), _ptr(mask_cols), _ptr(base), _ptr(res), B, C, int(H), W, int(taps), _stream()),
               "gtts_cond_field_forward")
    return res


def cond_field_backward(dy, mask_cols, taps, out=None):
    """S [B,taps,C]: the gradient of cond_field w.r.t. U (the gradient w.r.t. base is dy itself).  `out`: optional dict of a preallocated S."""
    _hip_only(dy, "cond_field_backward")
    dy, mask_cols = _f32c(dy, "dy"), _f32c(mask_cols, "mask")
    B, C, H, W = dy.shape
    if tuple(mask_cols.shape) != (B, W):
        raise ValueError("cond_field_backward: dy %s and mask %s do not match" % (tuple(dy.shape), tuple(mask_cols.shape)))
    S = _out(out, "S", (B, int(taps), C), torch.float32, dy.device, exc=ValueError)
    with _on(dy.device):
        _check(lib().gtts_cond_field_backward(_ptr(dy), _ptr(mask_cols), _ptr(S), B, C, H, W, int(taps), _stream()), "gtts_cond_field_backward")
    return S


def masked_mean(y, mask_cols, out=None):
    """p [B,C] = sum_{h,w} y mask / (sum_w mask H): RefBlock's masked mean over the plane (modules.py:165-166).  y [B,C,H,W], mask_cols
    [B,W].  `out`: optional dict of a preallocated p."""
    _hip_only(y, "masked_mean")
    y, mask_cols = _f32c(y, "y"), _f32c(mask_cols, "mask")
    B, C, H, W = y.shape
    if tuple(mask_cols.shape) != (B, W):
        raise ValueError("masked_mean: y %s and mask %s do not match" % (tuple(y.shape), tuple(mask_cols.shape)))
    p = _out(out, "p", (B, C), torch.float32, y.device, exc=ValueError)
    with _on(y.device):
        _check(lib().gtts_masked_mean_forward(_ptr(y), _ptr(mask_cols), _ptr(p), B, C, H, W, _stream()), "gtts_masked_mean_forward")
    return p


def masked_mean_backward(dp, mask_cols, H, out=None):
    """dy [B,C,H,W] of masked_mean: dp [B,C] broadcast over the live columns.  `out`: optional dict of a preallocated dy."""
    _hip_only(dp, "masked_mean_backward")
    dp, mask_cols = _f32c(dp, "dp"), _f32c(mask_cols, "mask")
    B, C = dp.shape
    W = int(mask_cols.shape[-1])
    if tuple(mask_cols.shape) != (B, W):
        raise ValueError("masked_mean_backward: dp %s and mask %s do not match" % (tuple(dp.shape), tuple(mask_cols.shape)))
    dy = _out(out, "dy", (B, C, int(H), W), torch.float32, dp.device, exc=ValueError)
    with _on(dp.device):
        _check(lib().gtts_masked_mean_backward(_ptr(dp), _ptr(mask_cols), _ptr(dy), B, C, int(H), W, _stream()), "gtts_masked_mean_backward")
    return dy


def diffusion_noising(x0, mu, z, mask, t, beta_min, beta_max, out=None):
    """Diffusion.forward_diffusion given the N(0,1) draw z: (xt, z * mask)   (diffusion.py:244-252).  `out`: optional dict of
    preallocated xt / zm."""
    x0, mu, z, mask, t = (_f32c(v, n) for v, n in ((x0, "x0"), (mu, "mu"), (z, "z"), (mask, "mask"), (t, "t")))
    B, F, T = x0.shape
    xt, zm = _out(out, "xt", (B, F, T), torch.float32, x0.device), _out(out, "zm", (B, F, T), torch.float32, x0.device)
    with _on(x0.device):
        _check(lib().gtts_diffusion_noising(_ptr(x0), _ptr(mu), _ptr(z), _ptr(mask), _ptr(t), float(beta_min), float(beta_max),
                                            _ptr(xt), _ptr(zm), B, F, T, _stream()), "gtts_diffusion_noising")
    return xt, zm


def score_loss(eps, z_masked, t, beta_min, beta_max, inv_denom, want_grad=True, out=None):
    """Diffusion.loss_t's reduction: (sum((eps s + z)^2) * inv_denom as a 0-d tensor, d loss / d eps or None).
    inv_denom: a Python float, or a 0-d device tensor (then nothing here synchronises with the host: the kernel runs with a
    unit normaliser and loss and gradient are scaled by tensor ops).  `out`: optional dict of preallocated partials / grad."""
    if torch.is_tensor(inv_denom):
        loss, g = score_loss(eps, z_masked, t, beta_min, beta_max, 1.0, want_grad, out)
        return loss * inv_denom, (g * inv_denom if g is not None else None)
    eps, z_masked, t = _f32c(eps, "eps"), _f32c(z_masked, "z"), _f32c(t, "t")
    B, F, T = eps.shape
    n = int(lib().gtts_score_loss_partials(B, F, T))
    part = _out(out, "partials", (n,), torch.float32, eps.device)
    g = _out(out, "grad", (B, F, T), torch.float32, eps.device) if want_grad else None
    with _on(eps.device):
        _check(lib().gtts_score_loss(_ptr(eps), _ptr(z_masked), _ptr(t), float(beta_min), float(beta_max), float(inv_denom),
                                     _ptr(part), _ptr(g), B, F, T, _stream()), "gtts_score_loss")
    return part.sum() * inv_denom, g


def conv_dgrad_small(dy, weight, mask_cols=None, out=None):
    """The first layer's data gradient (cin 2 or 3, its own kernel): dx [B,cin,H,W] of Conv2d_kxk(x * mask) for k = 3 (padding 1) or 1,
    dy [B,cout,H,W], weight [cout,cin,k,k] (not packed), mask_cols [B,W] or None."""
    _hip_only(dy, "conv_dgrad_small")
    dy, weight = _f32c(dy, "dy"), _f32c(weight, "weight")
    B, cout, H, W = dy.shape
    cin, ksize = int(weight.shape[1]), int(weight.shape[2])
    if weight.shape[0] != cout or weight.shape[3] != ksize:
        raise RuntimeError("weight %s does not match dy %s" % (tuple(weight.shape), tuple(dy.shape)))
    mask_cols = _const(dy.device, "ones", B, W) if mask_cols is None else _f32c(mask_cols, "mask")
    dx = _out(out, "dx", (B, cin, H, W), torch.float32, dy.device)
    with _on(dy.device):
        _check(lib().gtts_conv_dgrad_small(_ptr(dy), _ptr(weight), _ptr(mask_cols), _ptr(dx), B, cin, cout, H, W, ksize, _stream()),
               "gtts_conv_dgrad_small")
    return dx


def diffusion_noising_backward(dxt, mask, t, beta_min, beta_max, want_dx0=True, want_dmu=True, out=None):
    """(dx0, dmu) of diffusion_noising (an output not wanted is None)."""
    _hip_only(dxt, "diffusion_noising_backward")
    dxt, mask, t = _f32c(dxt, "dxt"), _f32c(mask, "mask"), _f32c(t, "t")
    B, F, T = dxt.shape
    dx0 = _out(out, "dx0", (B, F, T), torch.float32, dxt.device) if want_dx0 else None
    dmu = _out(out, "dmu", (B, F, T), torch.float32, dxt.device) if want_dmu else None
    with _on(dxt.device):
        _check(lib().gtts_diffusion_noising_backward(_ptr(dxt), _ptr(mask), _ptr(t), float(beta_min), float(beta_max), _ptr(dx0), _ptr(dmu),
                                                     B, F, T, _stream()), "gtts_diffusion_noising_backward")
    return dx0, dmu


def align_index(path, out=None):
    """The alignment path [B,t_x,T] of monotonic_align.maximum_path as indices: (idx [B,T] int32 token of each frame or -1,
    dur [B,t_x] fp32 frames per token, first [B,t_x] int32 first frame of each token's run or -1)."""
    _hip_only(path, "align_index")
    path = _f32c(path, "path")
    B, tx, T = path.shape
    idx = _out(out, "idx", (B, T), torch.int32, path.device)
    dur = _out(out, "dur", (B, tx), torch.float32, path.device)
    first = _out(out, "first", (B, tx), torch.int32, path.device)
    with _on(path.device):
        _check(lib().gtts_align_index(_ptr(path), _ptr(idx), _ptr(dur), _ptr(first), B, tx, T, _stream()), "gtts_align_index")
    return idx, dur, first


def duration_loss(logw, dur, x_mask, want_grad=True, out=None):
    """(sum((logw - log(1e-8 + dur) * x_mask)^2) as a 0-d tensor, its gradient w.r.t. logw or None): utils.py:42-44 without the
    normaliser, which the caller keeps as a device scalar.  logw, dur, x_mask: B * t_x elements each."""
    _hip_only(logw, "duration_loss")
    lw, d, m = _f32c(logw, "logw"), _f32c(dur, "dur"), _f32c(x_mask, "x_mask")
    B, tx = int(d.shape[0]), int(d.shape[-1])
    if lw.numel() != B * tx or m.numel() != B * tx:
        raise RuntimeError("logw, dur and x_mask must hold [B, t_x] = [%d, %d] elements each" % (B, tx))
    part = _out(out, "partials", (B,), torch.float32, lw.device)
    g = _out(out, "grad", tuple(lw.shape), torch.float32, lw.device) if want_grad else None
    with _on(lw.device):
        _check(lib().gtts_duration_loss(_ptr(lw), _ptr(d), _ptr(m), _ptr(part), _ptr(g), B, tx, _stream()), "gtts_duration_loss")
    return part.sum(), g


def align_gather(mu_x, y, idx, start, kept, S, out=None):
    """Training crop + aligned prior mean (tts.py:146-172) in one gather: (y_c [B,F,S], mu_y [B,F,S], sum over the live elements of
    0.5 ((y_c - mu_y)^2 + log 2 pi) as a 0-d tensor).  start, kept: [B] integer tensors (or lists); S: output frames."""
    _hip_only(mu_x, "align_gather")
    mx, yy = _f32c(mu_x, "mu_x"), _f32c(y, "y")
    B, F, tx = mx.shape
    T, S = int(yy.shape[2]), int(S)
    if tuple(yy.shape[:2]) != (B, F) or tuple(idx.shape) != (B, T) or idx.dtype != torch.int32:
        raise RuntimeError("mu_x [B,F,t_x], y [B,F,T] and idx [B,T] int32 disagree: %s, %s, %s" % (tuple(mx.shape), tuple(yy.shape), tuple(idx.shape)))
    st, kp = _i32c(start, "start", mx.device), _i32c(kept, "kept", mx.device)
    y_c = _out(out, "y_c", (B, F, S), torch.float32, mx.device)
    mu_y = _out(out, "mu_y", (B, F, S), torch.float32, mx.device)
    part = _out(out, "partials", (int(lib().gtts_align_gather_partials(B, F, S)),), torch.float32, mx.device)
    with _on(mx.device):
        _check(lib().gtts_align_gather_forward(_ptr(mx), _ptr(yy), _ptr(idx.contiguous()), _ptr(st), _ptr(kp), _ptr(y_c), _ptr(mu_y), _ptr(part),
                                               B, F, tx, T, S, _stream()), "gtts_align_gather_forward")
    return y_c, mu_y, part.sum()


def align_gather_backward(g_mu_y, mu_y, y_c, scale, dur, first, start, kept, out=None):
    """dmu_x [B,F,t_x] of align_gather: per token the sum, over its live output frames, of g_mu_y + scale * (mu_y - y_c).  g_mu_y
    [B,F,S] or None; scale: a one-element device tensor, (gradient of the prior loss) / (sum(kept) F), or None (then mu_y, y_c unused)."""
    _hip_only(dur, "align_gather_backward")
    g, my, yc, sc = _f32c(g_mu_y, "g_mu_y"), _f32c(mu_y, "mu_y"), _f32c(y_c, "y_c"), _f32c(scale, "scale")
    ref = g if g is not None else my
    B, F, S = ref.shape
    tx = int(dur.shape[1])
    st, kp = _i32c(start, "start", dur.device), _i32c(kept, "kept", dur.device)
    dmu_x = _out(out, "dmu_x", (B, F, tx), torch.float32, dur.device)
    with _on(dur.device):
        _check(lib().gtts_align_gather_backward(_ptr(g), _ptr(my), _ptr(yc), _ptr(sc), _ptr(_f32c(dur, "dur")), _ptr(first.contiguous()), _ptr(st),
                                                _ptr(kp), _ptr(dmu_x), B, F, tx, S, _stream()), "gtts_align_gather_backward")
    return dmu_x


def log_prior(mu_x, y):
    """MAS score matrix of GradTTS.compute_loss (tts.py:130-139): [B,F,t_x], [B,F,T] -> [B,t_x,T], one launch."""
    _hip_only(mu_x, "log_prior")
    mx, yy = _f32c(mu_x.detach(), "mu_x"), _f32c(y.detach(), "y")
    B, F, tx = mx.shape
    if yy.shape[0] != B or yy.shape[1] != F:
        raise RuntimeError("mu_x [B,F,t_x] and y [B,F,T] disagree: %s vs %s" % (tuple(mx.shape), tuple(yy.shape)))
    T = yy.shape[2]
    out = torch.empty((B, tx, T), dtype=torch.float32, device=mx.device)
    with _on(mx.device):
        _check(lib().gtts_log_prior(_ptr(mx), _ptr(yy), _ptr(out), B, F, tx, T, _stream()), "gtts_log_prior")
    return out


def expand_alignment(duration, x_mask, y_lengths, mu_x, T, noise=None, temperature=1.0):
    """generate_path + mu_y = attn^T . mu_x + z = mu_y + noise / temperature in one launch (tts.py:84-94).

    duration, x_mask: [B, t_x]; y_lengths: [B] integer; mu_x: [B, F, t_x]; noise: [B, F, T] or None.
    Returns (attn [B, t_x, T], mu_y [B, F, T], z [B, F, T] or None), bit-identical to the reference's CPU path."""
    _hip_only(mu_x, "expand_alignment")
    d, m, mx = _f32c(duration, "duration"), _f32c(x_mask, "x_mask"), _f32c(mu_x, "mu_x")
    B, F, tx = mx.shape
    if d.shape != (B, tx) or m.shape != (B, tx):
        raise RuntimeError("duration / x_mask must be [B, t_x] = [%d, %d]" % (B, tx))
    yl = y_lengths.to(device=mx.device, dtype=torch.int32).contiguous()
    nz = _f32c(noise, "noise")
    if nz is not None and nz.shape != (B, F, T):
        raise RuntimeError("noise must be [B, F, T]")
    attn = torch.empty((B, tx, T), dtype=torch.float32, device=mx.device)
    mu_y = torch.empty((B, F, T), dtype=torch.float32, device=mx.device)
    z = torch.empty((B, F, T), dtype=torch.float32, device=mx.device) if nz is not None else None
    with _on(mx.device):
        _check(lib().gtts_expand_alignment(_ptr(d), _ptr(m), _ptr(yl), _ptr(mx), _ptr(nz), float(temperature), _ptr(attn),
                                           _ptr(mu_y), _ptr(z), B, F, tx, int(T), _stream()), "gtts_expand_alignment")
    return attn, mu_y, z


def measured_ceilings(device, seconds=2.0):
    """Measured ceilings of this chip (bench.py roofline): bf16 MFMA TFLOP/s on random / zero operands and HBM GB/s for a
    16-byte copy, triad and read-only sweep.  About `seconds` of GPU time in total.  Returns a dict."""
    L = lib()
    out = {}
    with _on(device):
        st = _stream()
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
            fn = lambda: _check(L.gtts_ubench_mfma(_ptr(src), ctypes.c_size_t(src.numel() * 2), _ptr(sink), wgs, iters,
                                                   ctypes.byref(flops), st), "gtts_ubench_mfma")
            t1 = timed(fn, 3)
            reps = max(3, int(seconds * 0.3 / max(t1, 1e-6)))      # long enough for the clock to settle at its power budget
            t = timed(fn, reps)
            out["mfma_bf16_tflops_%s" % name] = flops.value / t * 1e-12
        fn = lambda: _check(L.gtts_ubench_mfma(_ptr(rnd), ctypes.c_size_t(rnd.numel() * 2), _ptr(sink), wgs, -iters,
                                               ctypes.byref(flops), st), "gtts_ubench_mfma")
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
                    fn = lambda: _check(L.gtts_ubench_hbm(_ptr(a), _ptr(b), _ptr(c), ctypes.c_size_t(n), mode + nt, cus * wpc,
                                                          ctypes.byref(nbytes), st), "gtts_ubench_hbm")
                    t = timed(fn, 3)
                    gbs = nbytes.value / t * 1e-9
                    out.setdefault("hbm_detail", {})["%s_%s_wg%d" % (name, "nt" if nt else "plain", wpc)] = round(gbs, 1)
                    best = max(best, gbs)
            out["hbm_%s_gbs" % name] = best
        out["cus"] = cus
    return out
