"""GPU tests (-m gpu) of the speaker encoder's waveform front end (csrc/wav.hip) through WavPlan and through the drop-in
encoder/audio.py, against the float64 restatement on the CPU (tests/wav_oracle.py).

Bounds.  Resample and normalise: e_kernel <= 4 e_ref32 + 2e-6 on signals with |y| <~ 1, e_ref32 being the same recipe run in float32
torch on the CPU (both max-abs against float64).  Power mel: max |got - ref| <= 1e-5 max(ref) per case, the criterion
tests/test_spk_cpu.py already holds this front end to (a wrong window, pad, frame origin or filter costs >= 1e-2; a serial fp32 chain of
400 terms measures ~1e-6); its ratio to e_ref32 is printed, not asserted.  No cell is left out of any comparison.  With -s every parity
case prints e_kernel, e_ref32 and their ratio.  Batch independence, repeatability, shift invariance, partials or none: bit for bit."""
import numpy as np
import pytest
import torch

import spk_oracle as SO
import wav_oracle as WO
from gpu_guards import S, dev  # noqa: F401

pytestmark = pytest.mark.gpu
L37 = 441 * 37 + 100
L_RS_TILE = 1412            # resamples to 1025 samples: one past the resampler's tile of 1024 outputs
L_MEL_TILE = 160 * 32       # 33 frames: one past a tile of the mel kernel (16 frames)
RESAMPLE_CASES = [(22050, 16000, L) for L in (1, 5, 441, 442, 1000, L37, L_RS_TILE)] + \
                 [(s, r, L) for (s, r) in WO.RATIOS[1:] for L in (5, 1000)]
MEL_LENGTHS = (201, 400, 1600, 160 * 59 + 31, 16000, L_MEL_TILE)


@pytest.fixture(scope="module")
def plan(S, dev):
    """plan(source_sr, sr) -> (WavPlan, blob), made once per ratio."""
    made = {}

    def get(source_sr=22050, sr=16000):
        if (source_sr, sr) not in made:
            p = S.WavPlan(source_sr, sr, fmax=min(8000.0, sr / 2))
            made[(source_sr, sr)] = (p, p.pack(dev))
        return made[(source_sr, sr)]
    return get


def _row(tag, e_kernel, e_ref32):
    print("\n%-46s e_kernel %.2e  e_ref32 %.2e  ratio %.2f" % (tag, e_kernel, e_ref32, e_kernel / max(e_ref32, 1e-30)))


# ---- resample
@pytest.mark.parametrize("source_sr,sr,L", RESAMPLE_CASES)
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("name", ["noise", "speechlike"])
def test_resample_parity(plan, dev, name, B, source_sr, sr, L):
    p, blob = plan(source_sr, sr)
    ref, e_ref32 = WO.resample_reference(name, L, source_sr, sr)
    got, partials = p.resample(blob, WO.wave(name, L, source_sr)[:B].to(dev))
    assert tuple(got.shape) == (B, WO.resampled_length(L, source_sr, sr)) == tuple(ref[:B].shape) and got.dtype == torch.float32
    assert tuple(partials.shape) == (B, p.tiles(got.shape[1]))
    e_kernel = float((got.cpu().double() - ref[:B]).abs().max())
    _row("resample %d->%d L=%d B=%d %s" % (source_sr, sr, L, B, name), e_kernel, e_ref32)
    assert e_kernel <= 4 * e_ref32 + 2e-6
    # the tile sums beside the output are its squares
    want = got.cpu().double().pow(2).sum(1)
    assert float((partials.cpu().double().sum(1) - want).abs().max()) <= 1e-5 * max(float(want.max()), 1e-30)


@pytest.mark.parametrize("source_sr,sr", WO.RATIOS)
def test_resample_of_an_impulse_at_either_end(plan, dev, source_sr, sr):
    """A single 1.0 at sample 0 and at sample L - 1: the zero-padded ends."""
    p, blob = plan(source_sr, sr)
    x = torch.zeros(2, 1000)
    x[0, 0] = x[1, -1] = 1.0
    ref = WO.resample(x, source_sr, torch.float64, sr)
    e_ref32 = float((WO.resample(x, source_sr, torch.float32, sr).double() - ref).abs().max())
    got = p.resample(blob, x.to(dev))[0].cpu()
    e_kernel = float((got.double() - ref).abs().max())
    _row("impulse ends %d->%d" % (source_sr, sr), e_kernel, e_ref32)
    assert got.shape == ref.shape and e_kernel <= 4 * e_ref32 + 2e-6 and float(ref.abs().max()) > 0.3


# ---- normalise
def _levels(sr=16000, L=16000):
    x = WO.wave("harmonic", L, sr)                        # rows at about -13 dBFS
    return torch.stack([0.01 * x[0], 10 * x[1], torch.zeros_like(x[2])])      # -53 dBFS (raised), +7 dBFS (left alone), silence


@pytest.mark.parametrize("mode", ["increase_only", "decrease_only", "none"])
def test_normalize_levels_and_modes(plan, dev, mode):
    p, blob = plan()
    x = _levels()
    level = 10 * torch.log10(x[:2].double().pow(2).mean(1))
    assert float(level[0]) < -30.5 and float(level[1]) > -29.5              # no decision rests on rounding
    kw = {} if mode == "none" else {mode: True}
    ref = WO.normalize(x, -30, **kw)
    e_ref32 = float(torch.nan_to_num(WO.normalize(x, -30, dtype=torch.float32, **kw).double() - ref).abs().max())
    got = p.normalize(blob, x.to(dev), -30, **kw).cpu()
    assert torch.equal(torch.isnan(got), torch.isnan(ref))
    e_kernel = float(torch.nan_to_num(got.double() - ref).abs().max())
    _row("normalize %s" % mode, e_kernel, e_ref32)
    assert e_kernel <= 4 * e_ref32 + 2e-6
    if mode == "increase_only":
        assert not torch.equal(got[0], x[0]) and torch.equal(got[1], x[1]) and bool(torch.isnan(got[2]).all())      # 0 * inf, as the module's recipe
        assert abs(float(10 * torch.log10(got[0].double().pow(2).mean())) + 30) < 1e-3
    elif mode == "decrease_only":
        assert torch.equal(got[0], x[0]) and not torch.equal(got[1], x[1]) and bool((got[2] == 0).all())
    else:
        assert torch.equal(got, x)
    A = WO.audio()
    module = A.normalize_volume_batch(x, -30, **kw)         # the module's torch recipe on the CPU treats the three rows alike
    assert torch.equal(torch.isnan(got), torch.isnan(module)) and float(torch.nan_to_num(got - module).abs().max()) <= 2e-6


def test_normalize_with_and_without_the_resamplers_partials(plan, dev):
    p, blob = plan()
    for L in (5, L_RS_TILE, L37):
        x = (0.01 * WO.wave("speechlike", L, 22050)).to(dev)
        y, partials = p.resample(blob, x)
        with_p = p.normalize(blob, y, -30, increase_only=True, partials=partials)
        alone = p.normalize(blob, y, -30, increase_only=True)
        assert not torch.equal(with_p, y) and torch.equal(with_p, alone)


# ---- power mel
@pytest.mark.parametrize("L", MEL_LENGTHS)
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("name", ["speechlike", "noise", "quiet", "impulse", "zeros"])
def test_power_mel_parity(plan, dev, name, B, L):
    p, blob = plan()
    ref, e_ref32 = WO.powmel_reference(name, L)
    got = p.powmel(blob, WO.wave(name, L, 16000)[:B].to(dev)).cpu()
    assert tuple(got.shape) == (B, 1 + L // 160, 40) == tuple(ref[:B].shape) and got.dtype == torch.float32
    e_kernel, top = float((got.double() - ref[:B]).abs().max()), float(ref[:B].max())
    _row("powmel L=%d B=%d %s  max(ref) %.2e" % (L, B, name, top), e_kernel, e_ref32)
    assert bool(torch.isfinite(got).all()) and e_kernel <= 1e-5 * top
    if name == "zeros" or (name == "impulse" and L <= 500):
        assert bool((got == 0).all())
    else:
        assert top > 0


@pytest.mark.parametrize("n_fft,hop,n_mels", [(1024, 1024, 128), (64, 1, 3), (1022, 300, 80)], ids=["largest", "smallest", "odd-tiles"])
def test_power_mel_at_the_ends_of_the_supported_range(S, dev, n_fft, hop, n_mels):
    """n_fft = hop = 1024 with 128 bands is the largest LDS footprint (above the 48 KB a launch gets unasked) and walks the table in
    three groups of row tiles; 64 / 1 the smallest; 1022 leaves a partial k block and a partial row tile.  Same criterion as above
    (a serial fp32 chain of 1024 terms: about sqrt(1024 / 400) of the 1.1e-6 measured at 400)."""
    p = S.WavPlan(22050, 16000, n_fft, hop, n_mels)
    L = 5 * n_fft + 77 if hop > 1 else 300
    x = WO.wave("noise", L, 16000)
    s = torch.stft(x.double(), n_fft=n_fft, hop_length=hop, win_length=n_fft, window=torch.hann_window(n_fft, dtype=torch.float64),
                   center=True, pad_mode="reflect", return_complex=True)
    ref = torch.transpose(torch.matmul(p.filterbank().double(), s.real ** 2 + s.imag ** 2), 1, 2)
    got = p.powmel(p.pack(dev), x.to(dev)).cpu()
    assert tuple(got.shape) == tuple(ref.shape) == (3, 1 + L // hop, n_mels)
    e_kernel, top = float((got.double() - ref).abs().max()), float(ref.max())
    _row("powmel n_fft=%d hop=%d n_mels=%d  max(ref) %.2e" % (n_fft, hop, n_mels, top), e_kernel, 0.0)
    assert top > 0 and e_kernel <= 1e-5 * top


# ---- independence
def test_rows_do_not_depend_on_the_batch_and_calls_repeat(plan, dev):
    p, blob = plan()
    x22 = (0.01 * WO.wave("speechlike", L37, 22050)).to(dev)
    y, partials = p.resample(blob, x22)
    z = p.normalize(blob, y, -30, increase_only=True, partials=partials)
    x16 = WO.wave("noise", 160 * 59 + 31, 16000).to(dev)
    mel = p.powmel(blob, x16)
    again = p.resample(blob, x22)
    assert torch.equal(again[0], y) and torch.equal(again[1], partials)
    assert torch.equal(p.normalize(blob, y, -30, increase_only=True, partials=partials), z) and torch.equal(p.powmel(blob, x16), mel)
    for b in range(3):
        yb, pb = p.resample(blob, x22[b:b + 1])
        assert torch.equal(yb, y[b:b + 1]) and torch.equal(pb, partials[b:b + 1])
        assert torch.equal(p.normalize(blob, yb, -30, increase_only=True, partials=pb), z[b:b + 1])
        assert torch.equal(p.normalize(blob, yb, -30, increase_only=True), z[b:b + 1])
        assert torch.equal(p.powmel(blob, x16[b:b + 1]), mel[b:b + 1])


@pytest.mark.parametrize("name", ["speechlike", "noise"])
def test_interior_frames_do_not_depend_on_their_position(plan, dev, name):
    """Dropping five hops of samples moves every frame five places, into another MFMA column and another workgroup: frames whose
    samples touch no reflection must not change by a bit."""
    p, blob = plan()
    for L in (160 * 59 + 31, 16000):
        x = WO.wave(name, L, 16000).to(dev)
        whole, shifted = p.powmel(blob, x), p.powmel(blob, x[:, 160 * 5:].contiguous())
        assert shifted.shape[1] == whole.shape[1] - 5
        assert torch.equal(shifted[:, 2:-2], whole[:, 7:-2])


# ---- the drop-in
@pytest.fixture(scope="module")
def I(dev, tmp_path_factory):
    mod = SO.encoder_pkg()
    sd = SO.state("default")
    sd.update(similarity_weight=torch.tensor([10.]), similarity_bias=torch.tensor([-5.]))
    path = tmp_path_factory.mktemp("wav") / "encoder.pt"
    torch.save({"model_state": sd, "step": 3}, path)
    mod.load_model(path, device=dev)
    return mod


def test_drop_in_from_22050_hz_to_the_embedding(I, dev):
    A = I.audio
    x = 0.01 * WO.wave("harmonic", 22050 * 2, 22050)
    ref = WO.normalize(WO.resample(x, 22050), -30, increase_only=True)
    ref32 = WO.normalize(WO.resample(x, 22050, torch.float32), -30, increase_only=True, dtype=torch.float32)
    e_ref32 = float((ref32.double() - ref).abs().max())
    got = A.preprocess_wav_batch(x.to(dev), 22050)
    assert got.is_cuda and tuple(got.shape) == (3, 32000) and got.dtype == torch.float32
    e_kernel = float((got.cpu().double() - ref).abs().max())
    _row("preprocess_wav_batch [3, 44100]", e_kernel, e_ref32)
    assert e_kernel <= 4 * e_ref32 + 2e-6
    # plan and tables are cached per device
    key = (22050, str(got.device))
    ptr = A._blobs[key].data_ptr()
    assert torch.equal(A.preprocess_wav_batch(x.to(dev), 22050), got) and A._blobs[key].data_ptr() == ptr
    embeds = I.embed_utterance_batch(got)
    assert embeds.is_cuda and tuple(embeds.shape) == (3, 256)
    for b in range(3):
        want, _ = SO.utterance_recipe(SO.state("default"), ref[b].numpy(), pad_value=1.0)
        assert float(np.abs(embeds[b].cpu().numpy() - want).max()) <= 1e-3
    # CPU tensors and tensors that require grad take the module's torch ops
    cpu = A.preprocess_wav_batch(x, 22050)
    assert not cpu.is_cuda and float((cpu.double() - ref).abs().max()) <= 4 * e_ref32 + 2e-6
    xg = x.to(dev).requires_grad_()
    grad = A.preprocess_wav_batch(xg, 22050)
    assert grad.requires_grad and float((grad.detach().cpu().double() - ref).abs().max()) <= 4 * e_ref32 + 2e-6
    with torch.no_grad():
        assert torch.equal(A.preprocess_wav_batch(xg, 22050), got)            # autograd off: the kernels
    # a source rate outside the kernels' table (16010 Hz reduces to 1601 / 1600): the torch recipe on the device, not a refusal
    odd = A.preprocess_wav_batch(x[:, :3000].to(dev), 16010)
    assert odd.is_cuda and tuple(odd.shape) == (3, -(-1600 * 3000 // 1601))
    assert float((odd.cpu() - A.preprocess_wav_batch(x[:, :3000], 16010)).abs().max()) <= 2e-6
    y = A.resample_batch(x, 22050).to(dev)                # normalize_volume_batch on its own: the kernels, forming the tile sums itself
    assert torch.equal(A.normalize_volume_batch(y, -30, increase_only=True), A._plan().normalize(None, y, -30, increase_only=True))
    assert float((A.normalize_volume_batch(y, -30, increase_only=True).cpu().double() - ref).abs().max()) <= 4 * e_ref32 + 2e-6


def test_drop_in_mel_paths_agree(I, dev):
    A = I.audio
    x = WO.wave("speechlike", 16000, 16000)
    ref, _ = WO.powmel_reference("speechlike", 16000)
    bound = 1e-5 * float(ref.max())
    kernel = A.wav_to_mel_spectrogram_batch(x.to(dev))
    p = A._plan()
    assert torch.equal(kernel, p.powmel(A._blob(16000, dev), x.to(dev)))
    xg = x.to(dev).requires_grad_()
    for other in (A.wav_to_mel_spectrogram_batch(x), A.wav_to_mel_spectrogram_batch(xg), A.wav_to_mel_spectrogram_batch(x.double().to(dev))):
        assert float((other.detach().cpu().double() - ref).abs().max()) <= bound
    assert float((kernel.cpu().double() - ref).abs().max()) <= bound
    assert A.wav_to_mel_spectrogram_batch(xg).requires_grad and A.wav_to_mel_spectrogram_batch(x.double().to(dev)).dtype == torch.float64


def test_one_call_allocates_its_outputs_only(plan, dev):
    """Beyond the packed blob and the cached workspace a call allocates its outputs and nothing else, not even transiently."""
    p, blob = plan()
    x = (0.01 * WO.wave("noise", L37, 22050)).to(dev)
    y, partials = p.resample(blob, x)
    calls = (lambda: p.resample(blob, x), lambda: (p.normalize(blob, y, -30, True, partials=partials),),
             lambda: (p.normalize(blob, y, -30, True),), lambda: (p.powmel(blob, y),))
    for call in calls:
        call()                                             # (first call: code object load, workspace)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        before = torch.cuda.memory_allocated(dev)
        out = call()
        torch.cuda.synchronize()
        out_bytes = sum((o.numel() * 4 + 511) // 512 * 512 for o in out)      # the caching allocator hands out multiples of 512 bytes
        assert torch.cuda.memory_allocated(dev) - before == out_bytes
        assert torch.cuda.max_memory_allocated(dev) - before == out_bytes
        del out
        assert torch.cuda.memory_allocated(dev) == before
