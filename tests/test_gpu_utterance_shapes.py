"""GPU tests (-m gpu) of the once-per-utterance inference models at the shapes and on the paths they really run: the encoders
(csrc/enc.hip) on BOTH attention kernels and at both LDS limits, the PostNet (csrc/postnet.hip) at whole-utterance lengths, HiFi-GAN V1
(csrc/voc.hip, csrc/conv1d.h) at its real widths with partial tiles and at the benchmark batch, the cached workspaces of all three,
and the DiffVC decoder at odd (B, T, T_ref).

Reference: the CPU oracles of oracle/ run in float64 (state and inputs cast with .double(); the fp32 oracles sit 1e-7 ... 1e-6 from
them).  Bounds are the project's existing ones and nothing else: max|err| <= 1e-4 * max|ref| for encoders and PostNet, and on the
waveform additionally 1e-4 absolute; log-durations as tests/test_gpu_encoder.py bounds them (on the O(1) scale of the quantity).

Which encoder assertion covers which kernel.  Every encoder case first asserts Encoder.attention_path(L), which reports the very
decision gtts_enc_forward dispatches by (one function in enc.hip), so a case proves which kernel produced the output it checks:
  enc_attention16_kernel  L = 2432 (its last length: exactly 160 KB of LDS), B 16 x L 1024, window 7 (last slot of s_rel),
                          window 0 with dk 96 (its win = -1 branch), kernel size 5
  enc_attention_kernel    L = 2433 (first length after the hand-over: the same weights as the L = 2432 case, so the pair runs one
                          configuration through both kernels), L = 5024 (its last length: exactly 160 KB), the ragged B 2 x L 3000
                          batch, window 8, dk 10 (dk % 4 != 0) with window 4 and with window 0 (its win = -1 branch)
  neither                 L = 5025 is refused by the library; the drop-in modules run their torch composition there.

Run with -s to see the table of measured errors."""
import importlib
import time
import warnings

import pytest
import torch

from oracle import diffvc_oracle as V
from oracle import encoder_oracle as E
from oracle import hifigan_oracle as H
from oracle import postnet_oracle as P
from gpu_guards import S, dev  # noqa: F401

pytestmark = pytest.mark.gpu
REL = 1e-4


def f64(sd):
    return {k: v.double() for k, v in sd.items()}


def relerr(a, b):
    """max|a - b| / max|b| with b the float64 reference."""
    return float((a.double() - b).abs().max() / (b.abs().max() + 1e-30))


def abserr(a, b):
    return float((a.double() - b).abs().max())


def row(fmt, *args):
    print("\n[utterance-shapes] " + fmt % args, end="")


# ------------------------------------------------------------------------------------------------------------------ encoders
ENC_KW = dict(n_vocab=149, n_feats=80, channels=192, filter_channels=768, filter_channels_dp=256, n_heads=2, n_layers=6, kernel_size=3,
              window_size=4)


def _enc_setup(S, dev, mode, seed, kw=ENC_KW):
    sd = E.make_state(mode, kw["n_vocab"], kw["n_feats"], kw["channels"], kw["filter_channels"], kw["filter_channels_dp"],
                      kw["n_heads"], kw["n_layers"], kw["kernel_size"], kw["window_size"], seed=seed)
    enc = S.Encoder(mode, **dict(kw, filter_channels_dp=kw["filter_channels_dp"] if mode == "text" else 0,
                                 n_vocab=kw["n_vocab"] if mode == "text" else 0))
    return sd, enc, enc.pack(sd, dev)


_ENC = {}


def _real_encoder(S, dev, mode):
    """The real-width encoder (192 / 768, 6 layers, 2 heads, window 4), one per mode for the whole module."""
    if mode not in _ENC:
        sd, enc, blob = _enc_setup(S, dev, mode, seed=31 if mode == "text" else 32)
        _ENC[mode] = (sd, f64(sd), enc, blob)
    return _ENC[mode]


def _enc_inputs(mode, lens, L, seed):
    g = torch.Generator().manual_seed(seed)
    lens = torch.tensor(lens)
    B = len(lens)
    x = torch.randint(0, 149, (B, L), generator=g) if mode == "text" else torch.randn(B, 80, L, generator=g)
    mask = E.sequence_mask(lens, L).unsqueeze(1).float()
    return x, lens, mask


def _enc_check(tag, mode, sd64, enc, blob, dev, x, lens, mask, path, kw=ENC_KW):
    """One encoder case: the path first, then the kernels against the float64 oracle."""
    B, L = mask.shape[0], mask.shape[-1]
    assert enc.attention_path(L) == path, (tag, L, enc.attention_path(L))
    o = dict(n_heads=kw["n_heads"], window=kw["window_size"], k=kw["kernel_size"])
    if mode == "text":
        mu, logw = enc.forward(blob, x.to(dev), mask.to(dev))
        mu, logw = mu.cpu(), logw.cpu()
        t0 = time.time()
        mu_o, logw_o, mask_o = E.text_encoder_forward(sd64, x, lens, **o)
        t1 = time.time()
        assert torch.equal(mask_o.float(), mask)
        e_mu, e_lw = relerr(mu, mu_o), abserr(logw, logw_o)
        lw_bound = REL * max(1.0, float(logw_o.abs().max()))
        row("%-26s text B %2d L %4d path %2d: mu rel %.2e, logw abs %.2e (bound %.2e)   [oracle %.1f s]", tag, B, L, path, e_mu, e_lw,
            lw_bound, t1 - t0)
        assert torch.isfinite(mu).all() and torch.isfinite(logw).all()
        assert e_mu <= REL
        assert e_lw <= lw_bound
        # exactly zero at masked positions (proj_m(x) * x_mask, proj_w(...) * x_mask)
        assert float((mu * (1 - mask)).abs().max()) == 0.0 and float((logw * (1 - mask)).abs().max()) == 0.0
        return mu, logw
    out = enc.forward(blob, x.to(dev), mask.to(dev)).cpu()
    t0 = time.time()
    ref = E.mel_encoder_forward(sd64, x.double(), mask.double(), **o)
    t1 = time.time()
    e = relerr(out, ref)
    row("%-26s mel  B %2d L %4d path %2d: rel %.2e   [oracle %.1f s]", tag, B, L, path, e, t1 - t0)
    assert torch.isfinite(out).all()
    assert e <= REL
    return out


def _ragged16(L):
    """Sixteen utterance lengths up to L, the longest first (the batch is padded to it): odd ones, either side of tile edges, one of 16."""
    return [L, L - 1, L - 17, (3 * L) // 4 + 1, L // 2, L // 2 + 33, L // 4, 16, L - 64, L - 65, 700, 513, 512, 511, 301, 257]


LONG_CASES = [
    # tag, lengths, L, path
    ("last length of path 16", [2432], 2432, 16),
    ("first length of path 8", [2433], 2433, 8),
    ("largest accepted length", [5024], 5024, 8),
    ("DiffVC shape, ragged", _ragged16(1024), 1024, 16),
    ("ragged batch on path 8", [3000, 1497], 3000, 8),
]


@pytest.mark.parametrize("mode", ["mel", "text"])
@pytest.mark.parametrize("tag,lens,L,path", LONG_CASES, ids=[c[0].replace(" ", "_").replace(",", "") for c in LONG_CASES])
def test_encoder_long_inputs_on_both_attention_paths(S, dev, mode, tag, lens, L, path):
    """Real width, real lengths.  L = 2432 and 5024 need exactly 160 KB of dynamic LDS on their kernel (the largest launch each kernel
    is ever asked for); 2432 / 2433 run the same weights through enc_attention16_kernel and enc_attention_kernel."""
    sd, sd64, enc, blob = _real_encoder(S, dev, mode)
    x, lens_t, mask = _enc_inputs(mode, lens, L, seed=L + len(lens))
    _enc_check(tag, mode, sd64, enc, blob, dev, x, lens_t, mask, path)


def test_encoder_refuses_the_first_length_past_the_limit(S, dev):
    """L = 5025: attention_path says 0 and forward raises a clean error (nothing is launched)."""
    for mode in ("mel", "text"):
        sd, sd64, enc, blob = _real_encoder(S, dev, mode)
        assert enc.attention_path(5025) == 0
        x, lens, mask = _enc_inputs(mode, [5025], 5025, seed=1)
        with pytest.raises(RuntimeError, match="too long"):
            enc.forward(blob, x.to(dev), mask.to(dev))
    torch.cuda.synchronize()


EDGE_CFGS = {
    # name: (channels, heads, window, kernel size, expected path)
    "window8": (96, 4, 8, 3, 8),             # 17 relative positions: the 8-query kernel
    "window7": (96, 4, 7, 3, 16),            # 15 relative positions: the last slot of s_rel
    "window0_dk96": (192, 2, 0, 3, 16),      # no relative window: win = -1 in enc_attention16_kernel
    "window0_dk10": (80, 8, 0, 3, 8),        # ... and in enc_attention_kernel
    "dk10": (80, 8, 4, 3, 8),                # dk % 4 != 0
    "kernel5": (192, 2, 4, 5, 16),           # FFN / duration-predictor kernel size 5
}


@pytest.mark.parametrize("mode", ["mel", "text"])
@pytest.mark.parametrize("L", [1, 7, 65, 130])
@pytest.mark.parametrize("name", list(EDGE_CFGS))
def test_encoder_edge_configurations(S, dev, name, L, mode):
    """The fallback kernel and the edge configurations at small L (shorter than, around and beyond the relative window; one and
    three 64-key blocks), ragged with a one-token item."""
    C, heads, window, k, path = EDGE_CFGS[name]
    kw = dict(ENC_KW, channels=C, filter_channels=4 * C, filter_channels_dp=64, n_heads=heads, n_layers=2, kernel_size=k,
              window_size=window)
    sd, enc, blob = _enc_setup(S, dev, mode, seed=50 + len(name), kw=kw)
    lens = [1, 1] if L == 1 else [L, max(1, L // 2), 1]
    x, lens_t, mask = _enc_inputs(mode, lens, L, seed=L)
    _enc_check(name, mode, f64(sd), enc, blob, dev, x, lens_t, mask, path, kw=kw)


def test_drop_in_encoders_run_past_the_kernel_limit(S, dev):
    """MelEncoder / TextEncoder in eval mode under no_grad at a length the kernels refuse: the reference modules work at any length,
    so the drop-ins run their own torch composition (and warn once) instead of raising."""
    TE = importlib.import_module("speech-backbones_amd.model.text_encoder")
    ME = importlib.import_module("speech-backbones_amd.diffvc.model.encoder")
    L = 5025
    kw = dict(ENC_KW, n_layers=2)               # (real width and heads, so the limit is the real one; two layers of oracle time)
    TE._WARNED_TOO_LONG.clear()
    sdm = E.make_state("mel", kw["n_vocab"], 80, 192, 768, 256, 2, 2, 3, 4, seed=61)
    menc = ME.MelEncoder(80, 192, 768, 2, 2, 3, 0.1, window_size=4)
    menc.load_state_dict(sdm, strict=True)
    menc = menc.to(dev).eval()
    x, lens, mask = _enc_inputs("mel", [L, 2000], L, seed=3)
    with torch.no_grad():
        with pytest.warns(RuntimeWarning, match="too long for the attention kernel"):
            out = menc(x.to(dev), mask.to(dev)).cpu()
        with warnings.catch_warnings():
            warnings.simplefilter("error")                                  # said once
            again = menc(x.to(dev), mask.to(dev)).cpu()
        short = menc(x[:, :, :100].contiguous().to(dev), mask[:, :, :100].contiguous().to(dev))     # the kernels still serve the rest
    assert menc._hip_enc.attention_path(L) == 0 and menc._hip_blob is not None and short.shape == (2, 80, 100)
    e = relerr(out, E.mel_encoder_forward(f64(sdm), x.double(), mask.double()))
    row("%-26s mel  B %2d L %4d path  0: rel %.2e (torch composition)", "MelEncoder module", 2, L, e)
    assert e <= REL and torch.equal(out, again)

    sdt = E.make_state("text", 149, 80, 192, 768, 256, 2, 2, 3, 4, seed=62)
    tenc = TE.TextEncoder(149, 80, 192, 768, 256, 2, 2, 3, 0.1, 4)
    tenc.load_state_dict(sdt, strict=True)
    tenc = tenc.to(dev).eval()
    ids, lens, mask = _enc_inputs("text", [L, 2000], L, seed=4)
    with torch.no_grad():
        with pytest.warns(RuntimeWarning, match="too long for the attention kernel"):
            mu, logw, m = tenc(ids.to(dev), lens.to(dev))
    mu_o, logw_o, mask_o = E.text_encoder_forward(f64(sdt), ids, lens)
    e_mu, e_lw = relerr(mu.cpu(), mu_o), abserr(logw.cpu(), logw_o)
    row("%-26s text B %2d L %4d path  0: mu rel %.2e, logw abs %.2e (torch composition)", "TextEncoder module", 2, L, e_mu, e_lw)
    assert torch.equal(m.cpu(), mask_o.float())
    assert e_mu <= REL and e_lw <= REL * max(1.0, float(logw_o.abs().max()))
    assert float((mu.cpu() * (1 - mask)).abs().max()) == 0.0 and float((logw.cpu() * (1 - mask)).abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------------------------ PostNet
_PN = {}


def _postnet(S, dev):
    if not _PN:
        sd = P.make_state(128, seed=3)
        plan = S.PostNetPlan(128)
        _PN["v"] = (sd, f64(sd), plan, plan.pack(sd, dev))
    return _PN["v"]


@pytest.mark.parametrize("lens,T", [(_ragged16(1024), 1024), ([1021], 1021), ([257, 1, 128], 257)],
                         ids=["B16_T1024_ragged", "B1_T1021", "B3_T257_one_frame_item"])
def test_postnet_whole_utterances(S, dev, lens, T):
    """The DiffVC average-voice path feeds the PostNet the whole utterance (dim 128): the benchmark batch with ragged lengths, a length
    that is no multiple of any tile, and a batch with a single-frame item.  At B 16 an item run alone at the same T gives the same
    bits (GroupNorm statistics are per sample and reduced in a fixed order).

    The float64 oracle of the B 16 batch is computed for six of its items, one at a time (the model is per sample; 3 s of host time
    per item): the full-length one, L - 1, 769, the 16-frame one, 511 and 257 -- each on its own scale, which is the stricter reading
    of 1e-4 * max|ref|."""
    sd, sd64, plan, blob = _postnet(S, dev)
    B = len(lens)
    g = torch.Generator().manual_seed(T + B)
    x = torch.randn(B, 80, T, generator=g)
    mask = E.sequence_mask(torch.tensor(lens), T).unsqueeze(1).float()
    out = plan.forward(blob, x.to(dev), mask.to(dev))
    assert torch.isfinite(out).all()
    items = (0, 1, 3, 7, 13, 15) if B == 16 else range(B)
    t0 = time.time()
    if B == 16:
        errs = [relerr(out[b:b + 1].cpu(), P.postnet_forward(sd64, x[b:b + 1].double(), mask[b:b + 1].double())) for b in items]
    else:
        ref = P.postnet_forward(sd64, x.double(), mask.double())
        errs = [relerr(out.cpu(), ref)] + [relerr(out[b].cpu(), ref[b]) for b in items]
    row("%-26s      B %2d T %4d: rel %.2e (worst of items %s, each on its own scale)   [oracle %.1f s]", "PostNet", B, T, max(errs),
        list(items), time.time() - t0)
    assert max(errs) <= REL
    if B == 16:
        for b in (0, 6, 15):                                               # full length, a quarter, the shortest
            alone = plan.forward(blob, x[b:b + 1].contiguous().to(dev), mask[b:b + 1].contiguous().to(dev))
            same = torch.equal(alone[0], out[b])
            row("%-26s      item %2d alone == in the batch, bitwise: %s", "PostNet", b, same)
            assert same


# ------------------------------------------------------------------------------------------------------------------ HiFi-GAN V1
def _v1_loud():
    """V1 widths (512/256/128/64/32) with the conv_post gain raised as the SMALL fixture of tests/test_gpu_hifigan.py does, so that
    the output tanh saturates for part of the samples.  SMALL's factor 6 is not enough at V1's width (fan-in scaled weights over 32
    instead of 4 final channels: the oracle alone gives max|wav| 0.24 at T = 1); with 20 the oracle's waveform reaches 0.70 at T = 1
    and 0.99 at T = 37, where two thirds of the samples lie beyond 0.5."""
    sd = H.make_state(H.V1, seed=5, gain=1.0)
    sd["conv_post.weight"] = sd["conv_post.weight"] * 20.0
    return sd


_VOC = {}


def _vocoder(S, dev, loud):
    if loud not in _VOC:
        sd = _v1_loud() if loud else H.make_state(H.V1, seed=0)
        voc = S.Vocoder(**H.V1)
        _VOC[loud] = (sd, f64(sd), voc, voc.pack(sd, dev))
    return _VOC[loud]


@pytest.mark.parametrize("B,T", [(1, 1), (3, 37), (2, 129)])
def test_vocoder_v1_odd_lengths(S, dev, B, T):
    """HiFi-GAN V1 at its real widths and odd frame counts.  The layers run at T (conv_pre, 512 wide), 8 T (256), 64 T (128), 128 T
    (64) and 256 T (32, conv_post): with T odd the last tile is partial on every layer that can have one -- the stage-3 layers and
    conv_post run at 256 T, a whole number of 128- and 256-sample tiles, and cannot.  The oracle's per-stage taps are not compared:
    the vocoder's intermediates cannot be read through the ABI."""
    sd, sd64, voc, blob = _vocoder(S, dev, True)
    mel = H.make_mel(B, T, seed=T)
    t0 = time.time()
    ref = H.generator_forward(sd64, H.V1, mel.double())
    t1 = time.time()
    wav = voc.forward(blob, mel.to(dev)).cpu()
    ea, er = abserr(wav, ref), relerr(wav, ref)
    row("%-26s      B %2d T %4d: max|ref| %.3f, abs %.2e, rel %.2e   [oracle %.1f s]", "HiFi-GAN V1", B, T, float(ref.abs().max()), ea,
        er, t1 - t0)
    assert wav.shape == (B, 1, 256 * T) and torch.isfinite(wav).all()
    assert float(ref.abs().max()) > 0.3
    assert ea <= 1e-4 and er <= REL


def test_vocoder_v1_benchmark_shape(S, dev):
    """B 16, T 1024 (what bench.py --target hifigan times): finite and inside (-1, 1), bit-identical on rerun, first and last items
    bit-identical to single-item runs, one item against the float64 oracle."""
    sd, sd64, voc, blob = _vocoder(S, dev, False)
    mel = H.make_mel(16, 1024, seed=11)
    a = voc.forward(blob, mel.to(dev))
    b = voc.forward(blob, mel.to(dev))
    assert a.shape == (16, 1, 262144) and torch.isfinite(a).all() and float(a.abs().max()) < 1.0
    rerun = torch.equal(a, b)
    first = torch.equal(voc.forward(blob, mel[0:1].contiguous().to(dev))[0], a[0])
    last = torch.equal(voc.forward(blob, mel[15:16].contiguous().to(dev))[0], a[15])
    row("%-26s      B 16 T 1024: rerun bitwise %s, item 0 alone bitwise %s, item 15 alone bitwise %s", "HiFi-GAN V1", rerun, first, last)
    assert rerun and first and last
    t0 = time.time()
    ref = H.generator_forward(sd64, H.V1, mel[7:8].double())
    ea, er = abserr(a[7:8].cpu(), ref), relerr(a[7:8].cpu(), ref)
    row("%-26s      B 16 T 1024 item 7: max|ref| %.3f, abs %.2e, rel %.2e   [oracle %.1f s]", "HiFi-GAN V1", float(ref.abs().max()), ea,
        er, time.time() - t0)
    assert ea <= 1e-4 and er <= REL


# ------------------------------------------------------------------------------------------------------------------ workspaces
def _poison(obj):
    """Fill the object's cached workspace (one shape at a time) with 0xFF bytes: every float in it becomes a NaN."""
    assert len(obj._ws) == 1
    (ws,) = obj._ws.values()
    assert ws.dtype == torch.uint8 and ws.numel() > 0
    ws.fill_(0xFF)
    return ws


def test_results_do_not_depend_on_workspace_contents(S, dev):
    """Encoder, PostNetPlan and Vocoder cache their workspace and reuse it: forward, fill the cached tensor with 0xFF bytes, forward
    again on the same inputs -- the same workspace tensor is used and the output is bit-identical."""
    for mode, L, lens in (("mel", 300, [300, 130]), ("text", 300, [300, 130]), ("mel", 2500, [2500])):       # (2500: the 8-query kernel)
        sd, sd64, enc, blob = _real_encoder(S, dev, mode)
        x, lens_t, mask = _enc_inputs(mode, lens, L, seed=77)
        first = enc.forward(blob, x.to(dev), mask.to(dev))
        ws = _poison(enc)
        second = enc.forward(blob, x.to(dev), mask.to(dev))
        assert next(iter(enc._ws.values())) is ws
        outs = zip(first, second) if mode == "text" else [(first, second)]
        same = all(torch.equal(p, q) and bool(torch.isfinite(q).all()) for p, q in outs)
        row("%-26s %-4s L %4d path %2d: bitwise after 0xFF fill: %s", "workspace Encoder", mode, L, enc.attention_path(L), same)
        assert same
    sd, sd64, plan, blob = _postnet(S, dev)
    g = torch.Generator().manual_seed(5)
    x = torch.randn(3, 80, 333, generator=g)
    mask = E.sequence_mask(torch.tensor([333, 200, 1]), 333).unsqueeze(1).float()
    first = plan.forward(blob, x.to(dev), mask.to(dev))
    ws = _poison(plan)
    second = plan.forward(blob, x.to(dev), mask.to(dev))
    same = torch.equal(first, second) and bool(torch.isfinite(second).all()) and next(iter(plan._ws.values())) is ws
    row("%-26s      B  3 T  333: bitwise after 0xFF fill: %s", "workspace PostNetPlan", same)
    assert same
    sd, sd64, voc, blob = _vocoder(S, dev, True)
    mel = H.make_mel(2, 45, seed=8)
    first = voc.forward(blob, mel.to(dev))
    ws = _poison(voc)
    second = voc.forward(blob, mel.to(dev))
    same = torch.equal(first, second) and bool(torch.isfinite(second).all()) and next(iter(voc._ws.values())) is ws
    row("%-26s      B  2 T   45: bitwise after 0xFF fill: %s", "workspace Vocoder", same)
    assert same


# ------------------------------------------------------------------------------------------------------------------ DiffVC decoder
@pytest.mark.parametrize("prec", ["bf16x3", "f16f8"])
@pytest.mark.parametrize("B,T,Tr", [(1, 4, 8), (3, 100, 36), (5, 260, 132), (2, 128, 260)])
def test_vc_estimator_matches_oracle_odd_shapes(S, dev, B, T, Tr, prec):
    """DiffVC estimator at odd (B, T, T_ref) -- the smallest T, a reference longer and shorter than the target, widths that are no
    multiple of a tile -- with ragged target and reference masks, both precisions (mirrors test_estimator_matches_oracle_odd_shapes of
    tests/test_gpu_parity.py under the REL of tests/test_gpu_diffvc.py)."""
    sd = V.make_state(dim_base=64, dim_cond=128, use_ref_t=True, seed=B)
    plan = S.Plan(dim=64, arch=1, precision={"bf16x3": S.PREC_BF16X3, "f16f8": S.PREC_F16F8}[prec])
    blob = plan.pack(sd, dev)
    inp = V.make_inputs(B, T, Tr, seed=B * 100 + T, ragged=False)
    lens = torch.tensor([T - 1 if B == 1 else T] + [max(1, (T * (k + 1)) // (B + 1)) for k in range(B - 1)])
    rlens = torch.tensor([Tr - 3 if B == 1 else Tr] + [max(1, (Tr * (B - 1 - k)) // (B + 1) + 1) for k in range(B - 1)])
    mask = E.sequence_mask(lens, T).unsqueeze(1).float()
    ref_mask = E.sequence_mask(rlens, Tr).unsqueeze(1).float()
    t = torch.linspace(0.05, 0.95, B)
    xt_ref = torch.stack([V.compute_diffused_mean(inp["ref"], ref_mask, inp["mean_ref"], 0.6)], 1)
    ref = V.estimator_forward(f64(sd), inp["z"].double(), mask.double(), inp["mean"].double(), xt_ref.double(), ref_mask.double(),
                              inp["c"].double(), t.double())
    out = plan.vc_estimator_forward(blob, inp["z"].to(dev), mask.to(dev), inp["mean"].to(dev), xt_ref.to(dev), ref_mask.to(dev),
                                    inp["c"].to(dev), t.to(dev)).cpu()
    e = relerr(out, ref)
    row("%-26s %-6s B %d T %3d Tr %3d: rel %.2e", "DiffVC estimator", prec, B, T, Tr, e)
    assert torch.isfinite(out).all()
    assert e <= REL
    assert float((out * (1 - mask)).abs().max()) == 0.0
