"""The algebra behind folding the level-0 attention output into the Downsample weights (csrc/attn.hip, attn_fold), restated in
torch float64 -- no GPU.

Reference form:  conv3x3s2(W, m * (x + M_b x + b')) + b_dn                      (attention apply pass, then the Downsample)
Folded form:     conv3x3s2(W'_b, m * x) + b_dn + sum_kx m(2 ox - 1 + kx) t[rowcase(oy)][kx][co]
    W'_b[co][ci][ky][kx] = W[co][ci][ky][kx] + sum_c W[co][c][ky][kx] M_b[c][ci]
    v[co][ky][kx]        = sum_c W[co][c][ky][kx] b'[c]
    t[0][kx][co] = v[co][1][kx] + v[co][2][kx]                    output row 0: tap row ky = 0 lies above the image
    t[1][kx][co] = v[co][0][kx] + v[co][1][kx] + v[co][2][kx]     every other row (the input height is even)
The bias table has exactly the kernel's layout [2 row cases][3 kx][C]."""
import pytest
import torch
import torch.nn.functional as F

TOL = 1e-12
SHAPES = [(3, 6, 13, [13, 8, 1]), (2, 8, 12, [12, 7])]      # odd width, a one-frame utterance, both parities of the mask edge


def _mask(lengths, W):
    return (torch.arange(W)[None, :] < torch.tensor(lengths)[:, None]).double()      # [B][W]


def _folded(x, m, Wd, b_dn, A_minus_I, bp):
    """The folded form, with the bias table in the kernel's layout."""
    B, C, H, Wi = x.shape
    Ho, Wo = (H + 1) // 2, (Wi + 1) // 2
    assert H % 2 == 0
    v = torch.einsum("ocyx,c->oyx", Wd, bp)                               # [co][ky][kx]
    table = torch.empty(2, 3, C, dtype=torch.float64)
    for kx in range(3):
        table[0, kx] = v[:, 1, kx] + v[:, 2, kx]
        table[1, kx] = (v[:, 0, kx] + v[:, 1, kx]) + v[:, 2, kx]
    out = torch.empty(B, C, Ho, Wo, dtype=torch.float64)
    for b in range(B):
        Wb = Wd + torch.einsum("ocyx,ci->oiyx", Wd, A_minus_I[b])
        y = F.conv2d((x[b] * m[b][None, None, :])[None], Wb, b_dn, stride=2, padding=1)[0]
        for oy in range(Ho):
            rc = 0 if oy == 0 else 1
            for ox in range(Wo):
                for kx in range(3):
                    gx = 2 * ox - 1 + kx
                    mk = m[b, gx] if 0 <= gx < Wi else 0.0
                    y[:, oy, ox] += mk * table[rc, kx]
        out[b] = y
    return out


@pytest.mark.parametrize("B,H,W,lengths", SHAPES)
def test_folded_downsample_equals_apply_then_downsample(B, H, W, lengths):
    C = 8
    g = torch.Generator().manual_seed(11 + W)
    x = torch.randn(B, C, H, W, generator=g, dtype=torch.float64)
    M = torch.randn(B, C, C, generator=g, dtype=torch.float64) * 0.5
    bp = torch.randn(C, generator=g, dtype=torch.float64)
    Wd = torch.randn(C, C, 3, 3, generator=g, dtype=torch.float64) * 0.3
    b_dn = torch.randn(C, generator=g, dtype=torch.float64)
    m = _mask(lengths, W)
    y = x + torch.einsum("bci,bihw->bchw", M, x) + bp[None, :, None, None]
    ref = F.conv2d(y * m[:, None, None, :], Wd, b_dn, stride=2, padding=1)
    got = _folded(x, m, Wd, b_dn, M, bp)
    err = float((got - ref).abs().max())
    print("B=%d H=%d W=%d lengths=%s: max |folded - reference| = %.3e (max |ref| %.3g)" % (B, H, W, lengths, err, float(ref.abs().max())))
    assert err <= TOL


def test_tap_forms_from_precomposed_output_projection():
    """What the fold kernel evaluates per tap: W'_b[tap] = W[tap] + g (W[tap] . Wout) . blockdiag(ctx^T) . Wq -- the same
    composition with the checkpoint-only product W[tap] . Wout formed first (at pack time) -- and v[tap] = W[tap] . bout."""
    C, heads, dh = 8, 4, 32
    g = torch.Generator().manual_seed(5)
    Wd = torch.randn(C, C, 3, 3, generator=g, dtype=torch.float64) * 0.3
    Wout = torch.randn(C, heads * dh, generator=g, dtype=torch.float64) * 0.1
    Wq = torch.randn(heads * dh, C, generator=g, dtype=torch.float64) * 0.3
    ctx = torch.randn(heads, dh, dh, generator=g, dtype=torch.float64) * 0.2      # [h][d][e]
    gz = 0.7
    U = torch.einsum("ohe,hde->ohd", Wout.view(C, heads, dh), ctx).reshape(C, heads * dh)
    M = gz * U @ Wq                                                               # attn.hip header: M_b
    want = Wd + torch.einsum("ocyx,ci->oiyx", Wd, M)
    WO = torch.einsum("ocyx,cj->yxoj", Wd, Wout)                                  # [ky][kx][co][128], pack time
    Ut = torch.einsum("yxohe,hde->yxohd", WO.view(3, 3, C, heads, dh), ctx).reshape(3, 3, C, heads * dh)
    got = Wd + gz * torch.einsum("yxoj,ji->oiyx", Ut, Wq)
    assert float((got - want).abs().max()) <= TOL
