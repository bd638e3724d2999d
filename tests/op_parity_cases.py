"""Case catalogue of tests/test_gpu_op_parity.py (helper module, imported by name like spk_oracle / mel_oracle; no GPU import).

A case is one estimator call: plan keyword arguments, B, T, the utterance lengths and, for DiffVC, T_ref.  The catalogue is the grid
of tests/golden/make_golden_op_table.py pruned by a cover rule: every kernel instance of tests/golden/op_table.json must be launched
by at least one case (tests/test_op_parity_cases_cpu.py proves it with Plan.ops, no GPU), and the four edge shapes below stay on
Grad-TTS bf16x3, Grad-TTS f16f8 (both with the uniform-wave and with the persistent convolution kernel) and DiffVC dim 64 bf16x3.

Edge shapes (level widths T, T/2, T/4; convolution tiles are 32 columns wide):
  (1, 4)    [3]             widths 4 / 2 / 1: one partial tile everywhere, a one-column plane at level 2; B = 1 small-launch tiling
  (2, 36)   [36, 19]        widths 36 / 18 / 9: a tile plus 4 columns, an utterance end inside a tile, the scalar tail at width 9
  (3, 132)  [132, 67, 1]    widths 132 / 66 / 33: one column past a tile at every level, and a one-frame utterance
  (16, 4)   [4, 3, 2, 1]*4  the regular (not half-height) tiling at the smallest planes: B decides the instance, not T
DiffVC dim 128 and 256 take (1, 4) and (2, 36) only (the float64 references grow with dim^2)."""
import collections

import torch

PREC_NAME = {0: "bf16x3", 1: "bf16", 2: "bf16_store", 3: "f16f8"}
EDGE_SHAPES = collections.OrderedDict([((1, 4), [3]), ((2, 36), [36, 19]), ((3, 132), [132, 67, 1]), ((16, 4), [4, 3, 2, 1] * 4)])
EXTRA_LENGTHS = {(5, 100): [100, 77, 51, 26, 1], (1, 92): [91], (1, 8): [7], (1, 256): [255]}
T_REF = {(1, 4): 24, (2, 36): 36, (3, 132): 24, (16, 4): 36, (1, 92): 24}

Case = collections.namedtuple("Case", "id arch dim prec conv_ws n_spks use_ref_t B T lengths T_ref")


def _case(arch, dim, prec, conv_ws, B, T, n_spks=1, use_ref_t=True):
    lengths = EDGE_SHAPES.get((B, T)) or EXTRA_LENGTHS[(B, T)]
    assert len(lengths) == B and max(lengths) <= T and T % 4 == 0
    if arch == 0:
        cid = "gradtts-%s-%s-spk%d-B%d-T%d" % (PREC_NAME[prec], "ws" if conv_ws else "mfma", n_spks, B, T)
        return Case(cid, 0, dim, prec, conv_ws, n_spks, True, B, T, list(lengths), None)
    cid = "diffvc%d-%s-%s-%s-B%d-T%d" % (dim, PREC_NAME[prec], "ws" if conv_ws else "mfma", "ref" if use_ref_t else "noref", B, T)
    return Case(cid, 1, dim, prec, conv_ws, 1, use_ref_t, B, T, list(lengths), T_REF[(B, T)])


# the configurations that keep all four edge shapes: (arch, dim, precision, conv_ws)
EDGE_CONFIGS = [(0, 64, 0, False), (0, 64, 0, True), (0, 64, 3, False), (0, 64, 3, True), (1, 64, 0, False)]

CASES = [_case(a, d, p, w, B, T) for (a, d, p, w) in EDGE_CONFIGS for (B, T) in EDGE_SHAPES]
CASES += [
    # ---- Grad-TTS dim 64
    _case(0, 64, 3, True, 5, 100),                    # batches of five or more: conv3x3_ws_kernel<1, 2, 2, 5, {1,2}, 3, float, 2>
    _case(0, 64, 0, False, 2, 36, n_spks=2),          # spk_mlp and the third input plane
    _case(0, 64, 1, False, 1, 4),                     # plain bf16 contractions
    _case(0, 64, 1, False, 2, 36, n_spks=2),
    _case(0, 64, 1, False, 3, 132),
    _case(0, 64, 1, False, 16, 4),
    _case(0, 64, 2, False, 1, 4),                     # bf16 storage: tail_identity_kernel<4, __bf16, 1> (not in the record's grid of shapes)
    _case(0, 64, 2, False, 1, 8),                     # tail_identity_kernel<8, __bf16, 1>
    _case(0, 64, 2, False, 1, 256),                   # tail_identity_kernel<8, __bf16, 4>
    _case(0, 64, 2, False, 2, 36, n_spks=2),          # prep_input_kernel<__bf16> with a speaker plane, the scalar bf16 tail
    _case(0, 64, 2, False, 3, 132),                   # tail_identity_kernel<4, __bf16, 4>
    _case(0, 64, 2, False, 16, 4),
    # ---- DiffVC dim 64
    _case(1, 64, 0, True, 2, 36),
    _case(1, 64, 0, False, 2, 36, use_ref_t=False),
    _case(1, 64, 1, False, 1, 4),
    _case(1, 64, 1, False, 2, 36),
    _case(1, 64, 1, False, 16, 4, use_ref_t=False),
    _case(1, 64, 3, False, 2, 36),
    _case(1, 64, 3, True, 3, 132),
    _case(1, 64, 3, True, 16, 4, use_ref_t=False),
    # ---- DiffVC dim 128
    _case(1, 128, 0, False, 1, 4),
    _case(1, 128, 0, False, 2, 36),
    _case(1, 128, 0, False, 1, 92),                   # tail_identity_kernel<4, float, 4>
    _case(1, 128, 0, True, 1, 4),
    _case(1, 128, 0, True, 2, 36, use_ref_t=False),
    _case(1, 128, 1, False, 1, 4),
    _case(1, 128, 1, False, 2, 36),
    _case(1, 128, 3, False, 2, 36),
    _case(1, 128, 3, True, 1, 4),
    _case(1, 128, 3, True, 2, 36),
    # ---- DiffVC dim 256
    _case(1, 256, 0, False, 1, 4),
    _case(1, 256, 0, True, 2, 36),
    _case(1, 256, 1, False, 1, 4),
    _case(1, 256, 1, False, 2, 36, use_ref_t=False),
    _case(1, 256, 3, False, 1, 4),
    _case(1, 256, 3, True, 2, 36),
]


def plan_kwargs(case):
    """Keyword arguments of Plan for a case, with the named intermediates kept."""
    kw = dict(dim=case.dim, precision=case.prec, conv_ws=case.conv_ws, keep_intermediates=True)
    if case.arch == 0:
        kw.update(n_spks=case.n_spks)
    else:
        kw.update(arch=1, use_ref_t=case.use_ref_t)
    return kw


# ---------------------------------------------------------------------------------------------------- who checks which op
# Check kinds of tests/test_gpu_op_parity.py, each with the op labels of Plan.ops it claims.  An op label must be claimed by exactly one
# kind; tests/test_op_parity_cases_cpu.py asserts that for every op of every case, and the GPU test asserts that what it checked is what
# its kinds claim.  The kinds in NOT_CHECKED_HERE are owned elsewhere or are not launched by an estimator call, for the reason given.
def _is_resnet_part(label, part):
    return label.endswith(part) and not label.startswith("ref.")


CLAIMS = collections.OrderedDict([
    ("stacked_input", lambda c, l, k: (l == "prep_input" and (c.arch == 0 or "prep_vc" in k)) or (l == "spk_mlp" and c.n_spks > 1)),
    ("time_bias", lambda c, l, k: l == "time_mlp"),
    ("block_conv", lambda c, l, k: _is_resnet_part(l, (".b1.conv", ".b2.conv")) or l == "final_block.conv"),
    ("groupnorm", lambda c, l, k: _is_resnet_part(l, ".gn")),
    ("tail_identity", lambda c, l, k: _is_resnet_part(l, ".tail")),       # also where the attention context pass applies it (marker)
    ("res_tail", lambda c, l, k: _is_resnet_part(l, ".res_tail")),
    ("downsample", lambda c, l, k: l in ("downs.0.3", "downs.1.3") or k.startswith("(fused into downs.")),
    ("upsample", lambda c, l, k: l in ("ups.0.3", "ups.1.3")),
    ("ref_conv", lambda c, l, k: l.startswith("ref.block") and l.endswith(".conv")),
    ("instnorm", lambda c, l, k: l.startswith("ref.block") and l.endswith(".in")),
    ("ref_pool", lambda c, l, k: l == "ref.pool"),
    ("cond", lambda c, l, k: l == "cond_block"),
    ("final", lambda c, l, k: l == "final_conv+euler"),
    ("attention", lambda c, l, k: l.endswith((".ctx", ".merge", ".fold", ".apply")) and not k.startswith("(fused into downs.")),
    ("sampler_only", lambda c, l, k: l == "xt=z*mask"),
    ("not_launched", lambda c, l, k: (l == "spk_mlp" and c.n_spks == 1) or (l == "prep_input" and c.arch == 1 and "prep_vc" not in k)),
])
NOT_CHECKED_HERE = {
    "attention": "context, merge, fold and apply of every attention are checked per op in float64 by tests/test_gpu_attention.py",
    "sampler_only": "z * mask opens a sampler call; an estimator call does not launch it (one exact fp32 product, tests/test_gpu_parity*.py)",
    "not_launched": "listed by Plan.ops for every plan, launched only by multi-speaker (spk_mlp) / Grad-TTS (prep_input_kernel) plans",
}


def claims(case, label, kernel):
    """The check kinds that claim one op of Plan.ops (exactly one, or the catalogue test fails)."""
    return [kind for kind, rule in CLAIMS.items() if rule(case, label, kernel)]


# What tests/test_gpu_parity_full.py, test_gpu_attention.py and test_gpu_op_parity.py share: the U-Net's op names, two bounds, the
# float64 attention and the reader of a plan's named intermediates.
REL = 1e-4          # bf16x3 contractions, fp32 accumulate (measured ~2e-5 per call)
FMT_FACTOR = 4.0    # bf16 / bf16_store: e_kernel <= FMT_FACTOR * e_fmt
RESNETS = ["downs.0.0", "downs.0.1", "downs.1.0", "downs.1.1", "downs.2.0", "downs.2.1", "mid_block1", "mid_block2",
           "ups.0.0", "ups.0.1", "ups.1.0", "ups.1.1"]
ATTNS = {"downs.0.2": "downs.0.1", "downs.1.2": "downs.1.1", "downs.2.2": "downs.2.1", "mid_attn": "mid_block1",
         "ups.0.2": "ups.0.1", "ups.1.2": "ups.1.1"}


def attention_f64(sd, a, X, bf16_operands=False, dtype=torch.float64):
    """(ctx [B,4,32,32], branch = g * LinearAttention(X) [B,C,H,W], max |k|) in float64.  bf16_operands: X and the two weights are
    rounded to bf16 first (the error the bf16 formats force); softmax and every sum stay float64.  dtype=torch.float32: the same
    chain in plain fp32, for the float32 reference's own context error."""
    p = a + ".fn.fn."
    B, C, H, W = X.shape
    rnd = (lambda v: v.float().to(torch.bfloat16).to(dtype)) if bf16_operands else (lambda v: v.to(dtype))
    x = rnd(X).reshape(B, C, H * W)
    wqkv = rnd(sd[p + "to_qkv.weight"]).reshape(384, C)
    wout = rnd(sd[p + "to_out.weight"]).reshape(C, 128)
    qkv = torch.einsum("oc,bcn->bon", wqkv, x).view(B, 3, 4, 32, H * W)
    q, k, v = qkv[:, 0], qkv[:, 1], qkv[:, 2]
    ctx = torch.einsum("bhdn,bhen->bhde", torch.softmax(k, -1), v)
    out = torch.einsum("bhde,bhdn->bhen", ctx, q).reshape(B, 128, H * W)
    y = torch.einsum("oc,bcn->bon", wout, out) + sd[p + "to_out.bias"].to(dtype)[None, :, None]
    return ctx, (y * sd[a + ".fn.g"].to(dtype)).view(B, C, H, W), float(k.abs().max())


def _reader(ws, infos, store_bf16=False):
    """name -> CPU fp32 copy of one named intermediate of the workspace.  With bf16 activation storage the activation tensors of
    plan.hip (kind TK_ACT: "x0", "<op>.raw", "<op>.out") are 2-byte; the per-sample ones ("<attn>.ctx", "<attn>.bfold") stay fp32.
    Plan.tensors has no view of 2-byte tensors, so the offsets are read as Plan.vc_tensors reads them."""
    def get(name):
        off, dims = infos[name]
        n = dims[0] * dims[1] * dims[2] * dims[3]
        if store_bf16 and (name == "x0" or name.endswith((".raw", ".out"))):
            return ws[off: off + 2 * n].view(torch.bfloat16).view(*dims).float().cpu()
        return ws[off: off + 4 * n].view(torch.float32).view(*dims).cpu()
    return get
