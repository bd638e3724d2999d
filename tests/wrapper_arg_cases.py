"""The case table of tests/test_gpu_wrapper_args.py: for every module-level function of the binding that launches a kernel, valid
arguments at the smallest shape the wrapper accepts and, for each tensor argument, one mismatch (a wrong trailing dimension, a wrong
channel count, a missing batch row).  No kernel runs on these tensors: the test replaces the binding's launch call with a recorder.

A case: id; fn (the wrapper); entry (the entry point a valid call reaches last); args(L, dev) -> keyword arguments; bad:
{tensor argument: wrong shape, or (wrong shape, the text the refusal names instead of the argument)} -- a wrong first tensor, the one the
wrapper reads its sizes from, shows as a mismatch of the next argument checked, and a wrong weight of the single-channel convolutions,
which define the channel count, as one of the bias; call(L, kw): how the wrapper takes them when not as keywords; stop: the recorder ends
the call at the first launch (a wrapper that goes on to time what it launched).  A wrapper with one tensor has no mismatch to make."""
import torch

I32, I64 = torch.int32, torch.int64


def Z(dev, *shape, dtype=torch.float32):
    return torch.zeros(shape, dtype=dtype, device=dev)


def _enc_att(dev, train):
    kw = dict(q=Z(dev, 2, 4, 8), k=Z(dev, 2, 4, 8), v=Z(dev, 2, 4, 8), mask=Z(dev, 2, 8), emb_rel_k=Z(dev, 3, 2), emb_rel_v=Z(dev, 3, 2),
              n_heads=2, window=1)
    if train:
        kw["drop"] = Z(dev, 2, 2, 8, 8)
    if train == 2:
        kw.update(stat=Z(dev, 2, 2, 8, 2), dout=Z(dev, 2, 4, 8))
    return kw


_ENC_ATT_BAD = dict(q=((1, 4, 8), "k"), k=(2, 4, 7), v=(2, 3, 8), mask=(2, 7), emb_rel_k=(3, 3), emb_rel_v=(2, 2))
_LN = lambda dev: dict(a=Z(dev, 2, 4, 8), gamma=Z(dev, 4), beta=Z(dev, 4), bres=Z(dev, 2, 4, 8), a_mask=Z(dev, 2, 8), out_mask=Z(dev, 2, 8))
_LN_BAD = dict(a=((1, 4, 8), "bres"), gamma=(5,), beta=(3,), bres=(2, 4, 7), a_mask=(1, 8), out_mask=(2, 7))


def _conv(k, cin=64, cout=64):
    """x, dy on 4 x 8 planes, B 2: the tiled convolutions' smallest shape (one 64-channel tile)."""
    return lambda L, dev: dict(x=Z(dev, 2, cin, 4, 8), mask_cols=Z(dev, 2, 8), weight=Z(dev, cout, cin, k, k), bias=Z(dev, cout))


def _dgrad(k, cin=64, cout=64):
    return lambda L, dev: dict(dy=Z(dev, 2, cout, 4, 8), weight=Z(dev, cout, cin, k, k), mask_cols=Z(dev, 2, 8))


def _wgrad(cin=64, cout=64):
    return lambda L, dev: dict(x=Z(dev, 2, cin, 4, 8), mask_cols=Z(dev, 2, 8), dy=Z(dev, 2, cout, 4, 8))


_CONV_BAD = dict(x=((2, 32, 4, 8), "weight"), mask_cols=(2, 7), weight=(64, 64, 2, 2), bias=(63,))
_DGRAD_BAD = dict(dy=((2, 128, 4, 8), "weight"), weight=(64, 64, 2, 2), mask_cols=(1, 8))
_WGRAD_BAD = dict(x=((1, 64, 4, 8), "mask_cols"), mask_cols=(2, 7), dy=(2, 64, 4, 7))
_NOISE = lambda L, dev: dict(x0=Z(dev, 2, 4, 8), mu=Z(dev, 2, 4, 8), z=Z(dev, 2, 4, 8), mask=Z(dev, 2, 1, 8), t=Z(dev, 2), beta_min=0.05,
                             beta_max=20.0)
_GATHER_BACK = lambda L, dev: dict(g_mu_y=Z(dev, 2, 4, 8), mu_y=Z(dev, 2, 4, 8), y_c=Z(dev, 2, 4, 8), scale=Z(dev, 1), dur=Z(dev, 2, 3),
                                   first=Z(dev, 2, 3, dtype=I32), start=Z(dev, 2, dtype=I32), kept=Z(dev, 2, dtype=I32))

CASES = [
    dict(id="enc_layernorm", fn="enc_layernorm", entry="gtts_enc_layernorm", args=lambda L, dev: _LN(dev), bad=_LN_BAD),
    dict(id="enc_attention", fn="enc_attention", entry="gtts_enc_attention", args=lambda L, dev: _enc_att(dev, 0), bad=_ENC_ATT_BAD),
    dict(id="enc_attention_train_forward", fn="enc_attention_train_forward", entry="gtts_enc_attention_train_forward",
         args=lambda L, dev: _enc_att(dev, 1), bad=dict(_ENC_ATT_BAD, drop=(2, 2, 8, 7))),
    dict(id="enc_attention_train_backward", fn="enc_attention_train_backward", entry="gtts_enc_attention_train_backward",
         args=lambda L, dev: _enc_att(dev, 2), bad=dict(_ENC_ATT_BAD, drop=(2, 1, 8, 8), stat=(2, 2, 8, 1), dout=(2, 4, 7))),
    dict(id="enc_layernorm_backward", fn="enc_layernorm_backward", entry="gtts_enc_layernorm_backward",
         args=lambda L, dev: dict(_LN(dev), dout=Z(dev, 2, 4, 8)), bad=dict(_LN_BAD, a=((1, 4, 8), "dout"), dout=(2, 4, 7))),
    dict(id="ge2e_loss", fn="ge2e_loss", entry="gtts_ge2e_loss", args=lambda L, dev: dict(embeds=Z(dev, 2, 2, 4), w=Z(dev, 1), b=Z(dev, 1)),
         bad=dict(embeds=(2, 4), w=(2,), b=(2,))),
    dict(id="euler_step", fn="euler_step", entry="gtts_euler_step",
         args=lambda L, dev: dict(xt=Z(dev, 2, 4, 8), mu=Z(dev, 2, 4, 8), est=Z(dev, 2, 4, 8), mask=Z(dev, 2, 1, 8), beta_t=7.3, h=0.1,
                                  noise=Z(dev, 2, 4, 8)),
         bad=dict(xt=((1, 4, 8), "mu"), mu=(2, 4, 7), est=(2, 3, 8), mask=(2, 1, 7), noise=(1, 4, 8))),
    dict(id="mas_maximum_path", fn="mas_maximum_path", entry="gtts_mas_maximum_path",
         args=lambda L, dev: dict(value=Z(dev, 2, 3, 5), mask=Z(dev, 2, 3, 5)), bad=dict(value=((2, 3, 4), "mask"), mask=(2, 2, 5))),
    dict(id="conv3x3_masked", fn="conv3x3_masked", entry="gtts_conv3x3_masked",
         args=lambda L, dev: dict(_conv(3, 128)(L, dev), x=Z(dev, 2, 64, 4, 8), x1=Z(dev, 2, 64, 4, 8)), bad=dict(_CONV_BAD, x1=(2, 64, 4, 7))),
    dict(id="conv3x3_masked-first", fn="conv3x3_masked", entry="gtts_conv3x3_masked", args=_conv(3, 2),
         bad=dict(x=((2, 3, 4, 8), "weight"), mask_cols=(2, 7), weight=(64, 2, 3, 2), bias=(63,))),
    dict(id="conv3x3_dgrad", fn="conv3x3_dgrad", entry="gtts_conv3x3_masked", args=_dgrad(3), bad=_DGRAD_BAD),
    dict(id="conv3x3_wgrad", fn="conv3x3_wgrad", entry="gtts_conv3x3_wgrad",
         args=lambda L, dev: dict(_wgrad(128)(L, dev), x=Z(dev, 2, 64, 4, 8), x1=Z(dev, 2, 64, 4, 8)),
         bad=dict(x=((1, 64, 4, 8), "x1"), mask_cols=(2, 7), dy=(2, 64, 4, 7), x1=(2, 64, 3, 8))),
    dict(id="conv3x3_wgrad-first", fn="conv3x3_wgrad", entry="gtts_conv_wgrad_small", args=_wgrad(2),
         bad=dict(x=((1, 2, 4, 8), "mask_cols"), mask_cols=(2, 7), dy=(2, 64, 4, 7))),
    dict(id="conv3x3_narrow_forward", fn="conv3x3_narrow_forward", entry="gtts_conv3x3_narrow_forward",
         args=lambda L, dev: dict(_conv(3, 32)(L, dev), out_mask=Z(dev, 2, 8)),
         bad=dict(x=((2, 16, 4, 8), "weight"), mask_cols=(2, 7), weight=(64, 32, 3, 2), bias=(63,), out_mask=(1, 8))),
    dict(id="conv3x3_narrow_dgrad", fn="conv3x3_narrow_dgrad", entry="gtts_conv3x3_narrow_dgrad",
         args=lambda L, dev: dict(_dgrad(3, 32)(L, dev), out_mask=Z(dev, 2, 8)),
         bad=dict(dy=((2, 128, 4, 8), "weight"), weight=(64, 32, 3, 2), mask_cols=(1, 8), out_mask=(2, 7))),
    dict(id="conv3x3_narrow_wgrad", fn="conv3x3_narrow_wgrad", entry="gtts_conv3x3_narrow_wgrad",
         args=lambda L, dev: dict(_wgrad(32)(L, dev), out_mask=Z(dev, 2, 8)),
         bad=dict(x=((1, 32, 4, 8), "mask_cols"), mask_cols=(2, 7), dy=(2, 64, 4, 7), out_mask=(2, 9))),
    dict(id="conv7x7_masked", fn="conv7x7_masked", entry="gtts_conv7x7_masked", args=_conv(7), bad=_CONV_BAD),
    dict(id="conv7x7_dgrad", fn="conv7x7_dgrad", entry="gtts_conv7x7_masked", args=_dgrad(7), bad=_DGRAD_BAD),
    dict(id="conv7x7_wgrad", fn="conv7x7_wgrad", entry="gtts_conv7x7_wgrad", args=_wgrad(), bad=_WGRAD_BAD),
    dict(id="postnet_expand", fn="postnet_expand", entry="gtts_postnet_expand",
         args=lambda L, dev: dict(x=Z(dev, 2, 4, 8), mask=Z(dev, 2, 8), w=Z(dev, 64, 1, 1, 1), bias=Z(dev, 64)),
         bad=dict(x=((1, 4, 8), "mask"), mask=(2, 7), w=((63,), "bias"), bias=(63,))),
    dict(id="postnet_collapse", fn="postnet_collapse", entry="gtts_postnet_collapse",
         args=lambda L, dev: dict(x=Z(dev, 2, 64, 4, 8), mask=Z(dev, 2, 8), w=Z(dev, 1, 64, 1, 1), bias=Z(dev, 1)),
         bad=dict(x=((2, 32, 4, 8), "w"), mask=(2, 7), w=(1, 63, 1, 1), bias=(2,))),
    dict(id="postnet_chan_dot", fn="postnet_chan_dot", entry="gtts_postnet_chan_dot",
         args=lambda L, dev: dict(a=Z(dev, 2, 64, 4, 8), v=Z(dev, 2, 4, 8), mask=Z(dev, 2, 8)),
         bad=dict(a=((1, 64, 4, 8), "v"), v=(2, 4, 7), mask=(2, 7))),
    dict(id="conv1x1_masked", fn="conv1x1_masked", entry="gtts_conv1x1_masked", args=_conv(1), bad=_CONV_BAD),
    dict(id="conv1x1_dgrad", fn="conv1x1_dgrad", entry="gtts_conv1x1_masked", args=_dgrad(1), bad=_DGRAD_BAD),
    dict(id="conv1x1_wgrad", fn="conv1x1_wgrad", entry="gtts_conv1x1_wgrad", args=_wgrad(), bad=_WGRAD_BAD),
    dict(id="conv1x1_wgrad-first", fn="conv1x1_wgrad", entry="gtts_conv_wgrad_small", args=_wgrad(2),
         bad=dict(x=((1, 2, 4, 8), "mask_cols"), mask_cols=(2, 7), dy=(2, 64, 4, 7))),
    dict(id="add_masked", fn="add_masked", entry="gtts_add_masked",
         args=lambda L, dev: dict(a=Z(dev, 2, 64, 4, 8), b=Z(dev, 2, 64, 4, 8), mask_cols=Z(dev, 2, 8)),
         bad=dict(a=(2, 64, 4, 7), b=((2, 32, 4, 8), "a"), mask_cols=(1, 8))),
    dict(id="add_masked-slice", fn="add_masked", entry="gtts_add_masked",
         args=lambda L, dev: dict(a=None, b=Z(dev, 2, 128, 4, 8), mask_cols=Z(dev, 2, 8), channels=(64, 128)),
         bad=dict(b=((2, 64, 4, 8), "channels"), mask_cols=(2, 7))),
    dict(id="zero_insert2", fn="zero_insert2", entry="gtts_zero_insert2", args=lambda L, dev: dict(x=Z(dev, 2, 64, 2, 4)), bad={}),
    dict(id="space_to_depth2", fn="space_to_depth2", entry="gtts_space_to_depth2", args=lambda L, dev: dict(x=Z(dev, 2, 64, 4, 8)),
         bad=dict(x=((2, 64, 3, 8), "even height"))),
    dict(id="final_conv_forward", fn="final_conv_forward", entry="gtts_final_conv_forward",
         args=lambda L, dev: dict(x=Z(dev, 2, 64, 4, 8), weight=Z(dev, 1, 64, 1, 1), bias=Z(dev, 1), mask_cols=Z(dev, 2, 8)),
         bad=dict(x=((2, 32, 4, 8), "weight"), weight=(1, 63, 1, 1), bias=(2,), mask_cols=(2, 7))),
    dict(id="final_conv_backward", fn="final_conv_backward", entry="gtts_final_conv_backward",
         args=lambda L, dev: dict(x=Z(dev, 2, 64, 4, 8), weight=Z(dev, 1, 64, 1, 1), mask_cols=Z(dev, 2, 8), dout=Z(dev, 2, 1, 4, 8)),
         bad=dict(x=((2, 32, 4, 8), "weight"), weight=(63,), mask_cols=(1, 8), dout=(2, 1, 4, 7))),
    dict(id="conv_resample-down", fn="conv_resample", entry="gtts_conv_resample", args=lambda L, dev: dict(_conv(3)(L, dev), up=False),
         bad=_CONV_BAD),
    dict(id="conv_resample-up", fn="conv_resample", entry="gtts_conv_resample", args=lambda L, dev: dict(_conv(4)(L, dev), up=True),
         bad=dict(_CONV_BAD, weight=(64, 64, 3, 3))),
    dict(id="conv_resample-dgrad_of_down", fn="conv_resample", entry="gtts_conv_resample",
         args=lambda L, dev: dict(_conv(3)(L, dev), bias=None, up=True, dgrad_of_down=True),
         bad=dict(x=((2, 32, 4, 8), "weight"), mask_cols=(2, 7), weight=(64, 64, 4, 4))),
    dict(id="attn_train_forward", fn="attn_train_forward", entry="gtts_attn_train_forward", args=lambda L, dev: dict(qkv=Z(dev, 2, 384, 2, 4)),
         bad=dict(qkv=((2, 383, 2, 4), "384 channels"))),
    dict(id="attn_train_backward", fn="attn_train_backward", entry="gtts_attn_train_backward",
         args=lambda L, dev: dict(qkv=Z(dev, 2, 384, 2, 4), dout=Z(dev, 2, 128, 2, 4), ctx=Z(dev, 2, 4, 32, 32), stat=Z(dev, 2, 4, 32, 2)),
         bad=dict(qkv=((2, 384, 2, 3), "dout"), dout=(2, 127, 2, 4), ctx=(1, 4, 32, 32), stat=(2, 4, 32, 1))),
    dict(id="rezero_forward", fn="rezero_forward", entry="gtts_rezero_forward",
         args=lambda L, dev: dict(f=Z(dev, 2, 64, 2, 4), g=Z(dev, 1), x=Z(dev, 2, 64, 2, 4)), bad=dict(f=((1, 64, 2, 4), "x"), g=(2,), x=(2, 64, 2, 3))),
    dict(id="rezero_backward", fn="rezero_backward", entry="gtts_rezero_backward",
         args=lambda L, dev: dict(dy=Z(dev, 2, 64, 2, 4), f=Z(dev, 2, 64, 2, 4), g=Z(dev, 1)), bad=dict(dy=(2, 64, 2, 3), f=((1, 64, 2, 4), "dy"), g=(2,))),
    dict(id="gn_mish_forward", fn="gn_mish_forward", entry="gtts_gn_mish_forward",
         args=lambda L, dev: dict(y=Z(dev, 2, 64, 4, 8), gamma=Z(dev, 64), beta=Z(dev, 64), mask_cols=Z(dev, 2, 8), groups=8, eps=1e-5, tb=Z(dev, 2, 64)),
         bad=dict(y=((2, 32, 4, 8), "gamma"), gamma=(63,), beta=(65,), mask_cols=(2, 7), tb=(2, 63))),
    dict(id="gn_mish_backward", fn="gn_mish_backward", entry="gtts_gn_mish_backward",
         args=lambda L, dev: dict(dout=Z(dev, 2, 64, 4, 8), y=Z(dev, 2, 64, 4, 8), gamma=Z(dev, 64), beta=Z(dev, 64), mask_cols=Z(dev, 2, 8),
                                  stats=Z(dev, int(L.lib().gtts_gn_mish_stats_floats(2, 8))), groups=8),
         bad=dict(dout=(2, 64, 4, 7), y=((1, 64, 4, 8), "dout"), gamma=(63,), beta=(65,), mask_cols=(2, 7), stats=(3,))),
    dict(id="in_glu_forward", fn="in_glu_forward", entry="gtts_in_glu_tb_forward",
         args=lambda L, dev: dict(y=Z(dev, 2, 64, 4, 8), gamma=Z(dev, 64), beta=Z(dev, 64), tb=Z(dev, 2, 32)),
         bad=dict(y=((2, 32, 4, 8), "gamma"), gamma=(32,), beta=(65,), tb=(2, 64))),
    dict(id="in_glu_backward", fn="in_glu_backward", entry="gtts_in_glu_backward",
         args=lambda L, dev: dict(dout=Z(dev, 2, 32, 4, 8), y=Z(dev, 2, 64, 4, 8), gamma=Z(dev, 64), beta=Z(dev, 64),
                                  stats=Z(dev, int(L.lib().gtts_in_glu_stats_floats(2, 32)))),
         bad=dict(dout=(2, 64, 4, 8), y=((2, 32, 4, 8), "dout"), gamma=(32,), beta=(65,), stats=(3,))),
    dict(id="cond_field", fn="cond_field", entry="gtts_cond_field_forward",
         args=lambda L, dev: dict(U=Z(dev, 2, 9, 64), mask_cols=Z(dev, 2, 8), H=4, base=Z(dev, 2, 64, 4, 8)),
         bad=dict(U=((1, 9, 64), "mask_cols"), mask_cols=(1, 8), base=(2, 64, 4, 7))),
    dict(id="cond_field_backward", fn="cond_field_backward", entry="gtts_cond_field_backward",
         args=lambda L, dev: dict(dy=Z(dev, 2, 64, 4, 8), mask_cols=Z(dev, 2, 8), taps=9), bad=dict(dy=((1, 64, 4, 8), "mask_cols"), mask_cols=(2, 7))),
    dict(id="masked_mean", fn="masked_mean", entry="gtts_masked_mean_forward",
         args=lambda L, dev: dict(y=Z(dev, 2, 64, 4, 8), mask_cols=Z(dev, 2, 8)), bad=dict(y=((1, 64, 4, 8), "mask_cols"), mask_cols=(2, 7))),
    dict(id="masked_mean_backward", fn="masked_mean_backward", entry="gtts_masked_mean_backward",
         args=lambda L, dev: dict(dp=Z(dev, 2, 64), mask_cols=Z(dev, 2, 8), H=4), bad=dict(dp=((1, 64), "mask_cols"), mask_cols=(3, 8))),
    dict(id="diffusion_noising", fn="diffusion_noising", entry="gtts_diffusion_noising", args=_NOISE,
         bad=dict(x0=((1, 4, 8), "mu"), mu=(2, 4, 7), z=(2, 3, 8), mask=(2, 1, 7), t=(3,))),
    dict(id="score_loss", fn="score_loss", entry="gtts_score_loss",
         args=lambda L, dev: dict(eps=Z(dev, 2, 4, 8), z_masked=Z(dev, 2, 4, 8), t=Z(dev, 2), beta_min=0.05, beta_max=20.0, inv_denom=0.5),
         bad=dict(eps=((1, 4, 8), "z_masked"), z_masked=(2, 4, 7), t=(1,))),
    dict(id="conv_dgrad_small", fn="conv_dgrad_small", entry="gtts_conv_dgrad_small", args=_dgrad(3, 2),
         bad=dict(dy=((2, 128, 4, 8), "weight"), weight=(64, 2, 3, 2), mask_cols=(1, 8))),
    dict(id="diffusion_noising_backward", fn="diffusion_noising_backward", entry="gtts_diffusion_noising_backward",
         args=lambda L, dev: dict(dxt=Z(dev, 2, 4, 8), mask=Z(dev, 2, 1, 8), t=Z(dev, 2), beta_min=0.05, beta_max=20.0),
         bad=dict(dxt=((1, 4, 8), "mask"), mask=(2, 1, 7), t=(3,))),
    dict(id="align_index", fn="align_index", entry="gtts_align_index", args=lambda L, dev: dict(path=Z(dev, 2, 3, 8)), bad={}),
    dict(id="duration_loss", fn="duration_loss", entry="gtts_duration_loss",
         args=lambda L, dev: dict(logw=Z(dev, 2, 1, 3), dur=Z(dev, 2, 3), x_mask=Z(dev, 2, 1, 3)),
         bad=dict(logw=(2, 1, 4), dur=((2, 4), "logw"), x_mask=(2, 1, 2))),
    dict(id="align_gather", fn="align_gather", entry="gtts_align_gather_forward",
         args=lambda L, dev: dict(mu_x=Z(dev, 2, 4, 3), y=Z(dev, 2, 4, 8), idx=Z(dev, 2, 8, dtype=I32), start=Z(dev, 2, dtype=I32),
                                  kept=Z(dev, 2, dtype=I32), S=8),
         bad=dict(mu_x=((1, 4, 3), "y"), y=(2, 3, 8), idx=(2, 7), start=(3,), kept=(1,))),
    dict(id="align_gather_backward", fn="align_gather_backward", entry="gtts_align_gather_backward", args=_GATHER_BACK,
         bad=dict(g_mu_y=((2, 4, 7), "mu_y"), mu_y=(2, 4, 7), y_c=(2, 3, 8), scale=(2,), dur=(1, 3), first=(2, 2), start=(3,), kept=(1,))),
    dict(id="log_prior", fn="log_prior", entry="gtts_log_prior", args=lambda L, dev: dict(mu_x=Z(dev, 2, 4, 3), y=Z(dev, 2, 4, 8)),
         bad=dict(mu_x=((1, 4, 3), "y"), y=(2, 3, 8))),
    dict(id="expand_alignment", fn="expand_alignment", entry="gtts_expand_alignment",
         args=lambda L, dev: dict(duration=Z(dev, 2, 3), x_mask=Z(dev, 2, 3), y_lengths=Z(dev, 2, dtype=I64), mu_x=Z(dev, 2, 4, 3), T=8,
                                  noise=Z(dev, 2, 4, 8)),
         bad=dict(duration=(2, 4), x_mask=(1, 3), y_lengths=(3,), mu_x=((2, 4, 4), "duration"), noise=(2, 4, 7))),
    dict(id="prepack", fn="prepack", entry="gtts_pack_batch", args=lambda L, dev: dict(weight=Z(dev, 64, 64, 3, 3)),
         call=lambda L, kw: L.prepack([(kw["weight"], 64, 64, False, "3x3"), (kw["weight"], 64, 64, True, "3x3")]), bad=dict(weight=(64, 64, 3, 2))),
    dict(id="measured_ceilings", fn="measured_ceilings", entry="gtts_ubench_mfma", args=lambda L, dev: dict(device=dev, seconds=0.0),
         bad={}, stop=True),
]
