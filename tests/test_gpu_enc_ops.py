"""GPU parity tests (-m gpu) of the encoders' fp32 VALU kernels (csrc/enc.hip), one op at a time through gtts_enc_layernorm and
gtts_enc_attention -- the two launch functions gtts_enc_forward itself calls -- against oracle/encoder_oracle.py in float64 on the
CPU.  The catalogue is tests/enc_op_cases.py; tests/test_enc_op_cases_cpu.py proves its paths, its score regimes and that the bound
below tells restated kernel mistakes from the kernels.

  error     e = max |got - ref64| / max |ref64| over ALL elements of the case: padded queries, padded keys' effect, the fully masked
            item and the length-1 item included.  e_ref32 = the same op in fp32 torch on the CPU against float64.
  bound     e <= 4 e_ref32 + 2e-6 (the project's fp32 elementwise rule) and e <= 1e-5 (its bound for fp32 reductions).  For the one
            case of enc_op_cases.SERIAL_SUM_CASES (L = 5024 on the 8-query kernel: 4.02e-06 against 3.56e-06) e_ref32 is the fp32
            restatement in that kernel's serial summation order, shown by the test to land within 2x of the kernel's error
  guards    every input lies inside a larger allocation whose margins hold NaN, `out` inside one filled with a sentinel: both
            kernels clamp out-of-range lanes onto valid memory, so a read outside a tensor shows as a NaN, a write as a disturbed
            sentinel, a skipped element as a surviving one
  linkage   after Encoder.forward the workspace's own Q, K, V / LayerNorm operands through the stand-alone entry points reproduce the
            workspace's A / x / H2 slots bit for bit: the entry points are the kernels the encoder runs, not twins
Run with -s for the table; the recorded figures are in profiles/enc_op_parity.txt."""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

import enc_op_cases as K
from gpu_guards import SENTINEL, Outputs, S, dev, guarded_inputs, table_row  # noqa: F401
from oracle import encoder_oracle as E

pytestmark = pytest.mark.gpu


def _run(dev, shape, margin, call):
    """`call(out)` between guards; the CPU result after checking the sentinel margins of `out` (written / finite: asserted by the
    tests, after their table row)."""
    o = Outputs(dev, margin)
    out = o.result("out", shape)
    got = call(out)
    assert got.data_ptr() == out.data_ptr()
    return o.collect(values=False)["out"]


def run_att(S, dev, c, d, path):
    B, C, L = d["q"].shape
    margin = 4 * L + 256                 # farther than any clamped lane could reach: a whole row of keys and a 64-key block
    t = guarded_inputs(d, ("q", "k", "v", "mask", "ek", "ev"), margin, dev)
    return _run(dev, (B, C, L), margin, lambda out: S.enc_attention(t["q"], t["k"], t["v"], t["mask"], t["ek"], t["ev"], n_heads=c.heads,
                                                                    window=c.window, path=path, out=out))


def run_ln(S, dev, c, d):
    B, C, L = d["a"].shape
    margin = 16 * L + 256                # a 16-position tile of every one of 16 channel lanes
    t = guarded_inputs(d, ("a", "bres", "gamma", "beta", "a_mask", "out_mask"), margin, dev)
    return _run(dev, (B, C, L), margin, lambda out: S.enc_layernorm(t["a"], t["gamma"], t["beta"], bres=t["bres"], a_mask=t["a_mask"],
                                                                    out_mask=t["out_mask"], eps=K.EPS, relu_in=c.relu_in,
                                                                    relu_out=c.relu_out, out=out))


@functools.lru_cache(maxsize=None)
def att_ref(cid):
    """(inputs, float64 reference, e_ref32) of one attention case: computed once per process, shared by every test, never modified."""
    c = K.ATT_BY_ID[cid]
    d = K.att_inputs(c)
    ref = K.att_reference(c, d)
    assert bool(torch.isfinite(ref).all())
    return d, ref, K.relerr(K.att_reference(c, d, torch.float32), ref)


@functools.lru_cache(maxsize=None)
def ln_ref(cid):
    c = K.LN_BY_ID[cid]
    d = K.ln_inputs(c)
    ref = K.ln_reference(c, d)
    assert bool(torch.isfinite(ref).all())
    return d, ref, K.relerr(K.ln_reference(c, d, torch.float32), ref)


_GOT = {}


def att_got(S, dev, cid, path):
    """The kernel's output for (case, path): run once, shared by the parity and the path-agreement tests."""
    if (cid, path) not in _GOT:
        _GOT[cid, path] = run_att(S, dev, K.ATT_BY_ID[cid], att_ref(cid)[0], path)
    return _GOT[cid, path]


def _row(kind, kernel, cid, shape, regime, maxref, e, e32, b):
    table_row((__name__, kind), "\n%-24s %-40s %-16s %-10s %9s %9s %9s %9s" % ("kernel", "case", "B,C,L", "regime", "max|ref|", "e", "e_ref32", "bound"),
              "%-24s %-40s %-16s %-10s %9.3f %9.2e %9.2e %9.2e" % (kernel, cid, "%d,%d,%d" % shape, regime, maxref, e, e32, b))


ATT_RUNS = [(c.id, p) for c in K.ATT_CASES for p in c.paths]
KERNEL = {8: "enc_attention_kernel", 16: "enc_attention16_kernel"}


@pytest.mark.parametrize("cid,path", ATT_RUNS, ids=["%s-path%d" % r for r in ATT_RUNS])
def test_attention_matches_float64(S, dev, cid, path):
    c = K.ATT_BY_ID[cid]
    d, ref, e32 = att_ref(cid)
    got = att_got(S, dev, cid, path)
    finite = bool(torch.isfinite(got).all())
    e = K.relerr(got, ref) if finite else float("nan")
    assert e32 <= K.E32_MAX
    regime = c.regime
    if cid in K.SERIAL_SUM_CASES and finite:
        # the 8-query kernel's one serial sum over L = 5024 keys per output element: e_ref32 is the fp32 restatement in the kernel's
        # own summation order (every 8th query row), once that restatement is shown to land within 2x of what the kernel does -- on
        # its own rows and against the error of the whole case
        rows = torch.arange(0, c.L, K.SERIAL_ROWS)
        nrm = ref.abs().max()
        e_ser = float((K.att_serial_fp32(c, d, rows).double() - ref[..., rows]).abs().max() / nrm)
        e_rows = float((got[..., rows].double() - ref[..., rows]).abs().max() / nrm)
        print("\n%s: e %.3e; rows 0, 8, 16, ...: kernel %.3e, serial-order fp32 restatement %.3e; fp32 torch %.3e" % (cid, e, e_rows, e_ser, e32))
        assert 0.5 * e_ser <= e_rows <= 2.0 * e_ser, (cid, e_rows, e_ser)
        assert 0.5 * e_ser <= e <= 2.0 * e_ser, (cid, e, e_ser)
        e32, regime = e_ser, c.regime + "/serial"
    b = K.bound(e32)
    _row("att", KERNEL[path], cid, tuple(ref.shape), regime, float(ref.abs().max()), e, e32, b)
    assert finite, "%s: non-finite output (a read outside an input, or a softmax that lost its maximum)" % cid
    assert not bool((got == SENTINEL).any()), "%s: an output element was never written" % cid
    assert e <= 4.0 * e32 + K.ELEMENTWISE_ABS, (cid, path, e, e32)
    assert e <= K.REDUCTION_REL, (cid, path, e)


BOTH = [c.id for c in K.ATT_CASES if set(c.paths) == {8, 16}]


@pytest.mark.parametrize("cid", BOTH)
def test_the_two_attention_kernels_agree(S, dev, cid):
    """Same inputs, same formulas, another association of the two long sums: each within the bound, and within twice the bound of
    each other."""
    d, ref, e32 = att_ref(cid)
    a, b = att_got(S, dev, cid, 8), att_got(S, dev, cid, 16)
    assert K.relerr(a, ref) <= K.bound(e32) and K.relerr(b, ref) <= K.bound(e32)
    diff = float((a.double() - b.double()).abs().max() / ref.abs().max())
    assert diff <= 2.0 * K.bound(e32), (cid, diff)


def test_attention_batch_items_do_not_see_each_other_and_runs_repeat(S, dev):
    """Item b of a batch equals, bit for bit, the same item run alone at B = 1; a second run of the batch is bit-identical."""
    n = 0
    for c in K.ATT_CASES:
        d = att_ref(c.id)[0]
        for path in c.paths:
            whole = att_got(S, dev, c.id, path)
            assert torch.equal(run_att(S, dev, c, d, path), whole), (c.id, path, "second run differs")
            for b in range(c.B if c.B > 1 else 0):
                alone = run_att(S, dev, c._replace(B=1, lens=(c.lens[b],)), K.att_slice(d, b), path)
                assert torch.equal(alone[0], whole[b]), (c.id, path, b)
                n += 1
    assert n >= 200


@pytest.mark.parametrize("cid", [c.id for c in K.LN_CASES])
def test_layernorm_matches_float64(S, dev, cid):
    c = K.LN_BY_ID[cid]
    d, ref, e32 = ln_ref(cid)
    got = run_ln(S, dev, c, d)
    finite = bool(torch.isfinite(got).all())
    e = K.relerr(got, ref) if finite else float("nan")
    flags = "+".join(k for k in K.FLAGS if getattr(c, k)) or "-"
    _row("ln", "enc_layernorm_kernel", cid, tuple(ref.shape), c.data, float(ref.abs().max()), e, e32, K.bound(e32))
    assert finite, "%s (%s): non-finite output (a read outside an input)" % (cid, flags)
    assert not bool((got == SENTINEL).any()), "%s: an output element was never written" % cid
    assert e32 <= K.E32_MAX
    assert e <= 4.0 * e32 + K.ELEMENTWISE_ABS, (cid, e, e32)
    assert e <= K.REDUCTION_REL, (cid, e)
    if c.out_mask:
        for b, n in enumerate(c.lens):
            assert n == c.L or float(got[b, :, n:].abs().max()) == 0.0, (cid, b)
    if c.data == "const":
        # equal inputs with a short mantissa: the sum is exact in any order, the mean is the value, every deviation 0, the output beta
        want = torch.relu(d["beta"]) if c.relu_out else d["beta"]
        for (b, t) in K.CONST_COLUMNS:
            assert torch.equal(got[b, :, t], want), (cid, b, t, float((got[b, :, t] - want).abs().max()))


def test_layernorm_batch_items_do_not_see_each_other_and_runs_repeat(S, dev):
    for c in K.LN_CASES:
        d = ln_ref(c.id)[0]
        whole = run_ln(S, dev, c, d)
        assert torch.equal(run_ln(S, dev, c, d), whole), (c.id, "second run differs")
        for b in range(c.B):
            alone = run_ln(S, dev, c._replace(B=1, lens=(c.lens[b],)), K.ln_slice(d, b))
            assert torch.equal(alone[0], whole[b]), (c.id, b)


# ------------------------------------------------------------------------------------------------------------------- linkage
def align256(n):
    return (n + 255) // 256 * 256


def slots(enc, B, L):
    """The workspace layout of gtts_enc_forward, restated once from csrc/enc.hip's comment above gtts_enc_workspace_bytes:
    X, Y, Z, Q, K, V, A of `channels` channels, then H and H2 of max(filter_channels, filter_channels_dp, channels) channels, each
    [B][channels][L] fp32 rounded up to 256 bytes.  Returns {name: (byte offset, channels)}."""
    C = enc.cfg.channels
    Hc = max(enc.cfg.filter_channels, enc.cfg.filter_channels_dp, C)
    sc, sh = align256(B * C * L * 4), align256(B * Hc * L * 4)
    lay = {n: (i * sc, C) for i, n in enumerate(("X", "Y", "Z", "Q", "K", "V", "A"))}
    lay["H"], lay["H2"] = (7 * sc, Hc), (7 * sc + sh, Hc)
    assert 7 * sc + 2 * sh == enc.workspace_bytes(B, L), "the slots do not sum to gtts_enc_workspace_bytes"
    return lay


def slot(ws, lay, name, B, L, channels=None):
    off, ch = lay[name]
    ch = channels or ch
    return ws[off:off + B * ch * L * 4].view(torch.float32).view(B, ch, L)


def _encoder(S, dev, mode, n_layers, seed):
    sd = E.make_state(mode, n_layers=n_layers, seed=seed)
    enc = S.Encoder("text", n_layers=n_layers) if mode == "text" else S.Encoder("mel", 0, 80, 192, 768, 0, 2, n_layers, 3, 4)
    return sd, enc, enc.pack(sd, dev)


@pytest.mark.parametrize("mode", ["text", "mel"])
@pytest.mark.parametrize("n_layers", [1, 6])
@pytest.mark.parametrize("B,L", [(2, 45), (1, 2433)])
def test_entry_points_are_the_kernels_the_encoder_runs(S, dev, mode, n_layers, B, L):
    """After Encoder.forward the workspace still holds the last layer's Q, K, V and A, the LN-1 output (X slot), the FFN output
    (Z slot) and the layer's result x (Y slot); the text encoder's H / H2 hold the DurationPredictor's second conv and LayerNorm."""
    sd, enc, blob = _encoder(S, dev, mode, n_layers, 40 + n_layers)
    path = enc.attention_path(L)
    assert path == (16 if L <= 2432 else 8)
    g = torch.Generator().manual_seed(L)
    lens = torch.tensor([L, max(1, L // 3)][:B])
    mask = E.sequence_mask(lens, L).float().to(dev)
    x = torch.randint(0, 149, (B, L), generator=g) if mode == "text" else torch.randn(B, 80, L, generator=g)
    enc.forward(blob, x.to(dev), mask)
    torch.cuda.synchronize()
    ws = enc.workspace(B, L, dev)
    lay = slots(enc, B, L)
    get = lambda n, ch=None: slot(ws, lay, n, B, L, ch).clone()
    p = "encoder.attn_layers.%d." % (n_layers - 1)
    ek, ev = sd[p + "emb_rel_k"][0].contiguous().to(dev), sd[p + "emb_rel_v"][0].contiguous().to(dev)
    A = S.enc_attention(get("Q"), get("K"), get("V"), mask, ek, ev, n_heads=2, window=4, path=0)
    assert torch.equal(A, get("A")), "gtts_enc_attention differs from the encoder's attention (path %d)" % path
    assert torch.equal(S.enc_attention(get("Q"), get("K"), get("V"), mask, ek, ev, n_heads=2, window=4, path=path), A)
    n2 = "encoder.norm_layers_2.%d." % (n_layers - 1)
    xs = S.enc_layernorm(get("X"), sd[n2 + "gamma"].to(dev), sd[n2 + "beta"].to(dev), bres=get("Z"))
    assert torch.equal(xs, get("Y")), "gtts_enc_layernorm differs from the encoder's norm_layers_2"
    assert bool(torch.isfinite(xs).all()) and float(xs.abs().max()) > 0.5
    if mode == "text":
        h2 = S.enc_layernorm(get("H", 256), sd["proj_w.norm_2.gamma"].to(dev), sd["proj_w.norm_2.beta"].to(dev), relu_in=True)
        assert torch.equal(h2, get("H2", 256)), "gtts_enc_layernorm differs from the DurationPredictor's norm_2"


@pytest.mark.parametrize("L", [1, 257])
def test_embedding_slot_without_layers(S, dev, L):
    """n_layers = 0: nothing overwrites the X slot after enc_embed_kernel; it is F.embedding(ids) * sqrt(C) in fp32, exactly."""
    sd, enc, blob = _encoder(S, dev, "text", 0, 50)
    B = 2
    ids = torch.randint(0, 149, (B, L), generator=torch.Generator().manual_seed(L))
    mask = E.sequence_mask(torch.tensor([L, max(1, L // 2)]), L).float().to(dev)
    enc.forward(blob, ids.to(dev), mask)
    torch.cuda.synchronize()
    X = slot(enc.workspace(B, L, dev), slots(enc, B, L), "X", B, L).cpu()
    want = (F.embedding(ids, sd["emb.weight"]) * math.sqrt(192)).transpose(1, 2)
    assert want.dtype == torch.float32 and torch.equal(X, want)
