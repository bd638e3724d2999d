"""Shared by the tests that compare with tests/golden/live_*.npz and by tests/golden/make_golden_live.py, which writes them:
the inputs both sides draw, and the checks of a module's layout and initialisation against the reference's."""
import glob
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# DiffVC shell, small but structurally complete: n_feats 80, 2 transformer layers, dec_dim 64
VC_ARGS = dict(n_feats=80, channels=48, filters=96, heads=2, layers=2, kernel=3, dropout=0.0, window_size=4, enc_dim=32,
               spk_dim=128, use_ref_t=True, dec_dim=64, beta_min=0.05, beta_max=20.0)

# host threads live_*.npz were written with: the CPU convolutions' sums, and so the last bits of a gradient, depend on it
GOLDEN_THREADS = 8

_LIVE = None


# file of each group of arrays (by key prefix), so that no single fixture file grows large
GROUPS = (("vc_fwd_out", "vc"), ("vc_fwd_", "vc_forward"), ("vc_", "vc"), ("grad_", "grads"), ("gradtts_", "gradtts"),
          ("textenc_", "gradtts"), ("hifigan_", "hifigan"), ("", "oracle"))


def group_of(key):
    return next(g for prefix, g in GROUPS if key.startswith(prefix))


def live():
    """Every array of tests/golden/live_*.npz in one dict."""
    global _LIVE
    if _LIVE is None:
        _LIVE = {}
        for f in sorted(glob.glob(os.path.join(GOLDEN, "live_*.npz"))):
            _LIVE.update(np.load(f))
    return _LIVE


def encode_layout(sd):
    return np.array(list(sd)), np.array([",".join(str(d) for d in v.shape) for v in sd.values()])


def layout(G, tag):
    """[(name, shape)] of a state_dict stored with encode_layout."""
    return [(str(n), tuple(int(d) for d in str(s).split(",") if d)) for n, s in zip(G[tag + "_names"], G[tag + "_shapes"])]


def assert_reference_init(sd, G, tag):
    """Same names and shapes as the reference's state_dict, and per tensor the same |.|-sum of its seeded default init."""
    assert [(k, tuple(v.shape)) for k, v in sd.items()] == layout(G, tag)
    for (k, v), want in zip(sd.items(), G[tag + "_abssum"]):
        assert abs(float(v.double().abs().sum()) - float(want)) <= 1e-12 * max(1.0, float(want)), k


def sample_index(n, k=64):
    """Positions of the stored entries of a tensor with n elements: all of them up to k, else k evenly spaced."""
    return np.unique(np.linspace(0, n - 1, min(n, k)).round().astype(np.int64))


def hifigan_attr(cfg):
    return dict(cfg, upsample_rates=list(cfg["upsample_rates"]), upsample_kernel_sizes=list(cfg["upsample_kernel_sizes"]),
                resblock_kernel_sizes=list(cfg["resblock_kernel_sizes"]),
                resblock_dilation_sizes=[list(d) for d in cfg["resblock_dilation_sizes"]])


def vc_forward_inputs():
    g = torch.Generator().manual_seed(5)
    x = torch.randn(3, 80, 50, generator=g)
    x_len = torch.tensor([50, 37, 42])                    # longest 50 -> padded to 52
    x_ref = torch.randn(3, 80, 36, generator=g)
    r_len = torch.tensor([36, 20, 29])
    c = torch.randn(3, 256, generator=g)
    return x, x_len, x_ref, r_len, c


def vc_loss_inputs():
    g = torch.Generator().manual_seed(8)
    x = torch.randn(2, 80, 32, generator=g)
    x_len = torch.tensor([32, 24])
    x_ref = torch.randn(2, 80, 32, generator=g)
    c = torch.randn(2, 256, generator=g)
    return x, x_len, x_ref, c


def _mask(xl, yl, tx, ty):
    from oracle import gradtts_oracle as O
    return (O.sequence_mask(xl, tx).unsqueeze(-1) * O.sequence_mask(yl, ty).unsqueeze(1)).float()


def mas_random_cases():
    g = torch.Generator().manual_seed(11)
    cases = []
    for b, tx, ty in [(4, 31, 90), (3, 1, 7), (2, 50, 50), (6, 13, 200)]:
        value = torch.randn(b, tx, ty, generator=g) * 4
        xl = torch.randint(1, tx + 1, (b,), generator=g)
        yl = torch.maximum(torch.randint(1, ty + 1, (b,), generator=g), xl)   # t_y >= t_x (defined regime)
        cases.append((value, _mask(xl, yl, tx, ty)))
    return cases


def mas_gpu_case():
    g = torch.Generator().manual_seed(42)
    value = torch.randn(8, 60, 333, generator=g) * 5
    xl = torch.randint(1, 61, (8,), generator=g)
    yl = torch.maximum(torch.randint(1, 334, (8,), generator=g), xl)
    return value, _mask(xl, yl, 60, 333)
