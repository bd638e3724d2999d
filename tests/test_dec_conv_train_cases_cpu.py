"""CPU: the catalogue of tests/dec_conv_train_cases.py proves what it claims without a GPU -- its formulas equal float64 autograd, the
`integers` cases are exact in fp32, every restated mistake is told from the contract by the bounds the GPU test applies, the documented
arithmetic itself stays inside them, the weight-gradient regimes and the kernel instances it claims are the ones the library chooses."""

import pytest
import torch

import dec_conv_train_cases as C
import wgrad_regimes as R
from abi_util import S

CONV_CASES = [c for c in C.CASES if c.op in C.CONV_OPS]
GLUE_CASES = [c for c in C.CASES if c.op in C.GLUE_OPS]


@pytest.fixture(scope="module")
def lib(S):
    return S._lib


def _held(ref):
    return [n for n in ("y", "dx", "dw", "db") if ref[n] is not None]


@pytest.mark.parametrize("cid", [c.id for c in CONV_CASES])
def test_formulas_equal_float64_autograd(cid):
    c, d, ref, M, base = C.references(cid)
    got = C.formulas(c, d)
    for n in _held(ref):
        assert float(ref[n].abs().max()) > 0.0, (cid, n)
        assert got[n].shape == ref[n].shape and C.relerr(got[n], ref[n]) <= 1e-12, (cid, n, C.relerr(got[n], ref[n]))
        assert bool((M[n] >= ref[n].abs() * (1 - 1e-12)).all()), (cid, n)         # M bounds |ref| element for element
    assert max(t.numel() for t in (d["x"], d["dy"], d["w"])) <= 2.2e6, cid


@pytest.mark.parametrize("cid", [c.id for c in CONV_CASES if c.kind == "integers"])
def test_integer_cases_are_exact_in_fp32(cid):
    """The premise of the zero-tolerance test, on the reference alone: fp32 autograd equals float64 autograd bit for bit."""
    c, d, ref, _, _ = C.references(cid)
    assert 9 * C.contraction(c) < 2 ** 24, cid
    for v in (d["x"], d["dy"], d["w"], d["bias"]):
        assert v is None or (bool((v == v.round()).all()) and float(v.abs().max()) <= 3.0)
    ref32 = C.reference(c, d, torch.float32)
    for n in _held(ref):
        assert ref32[n].dtype == torch.float32 and torch.equal(ref32[n].double(), ref[n]), (cid, n)


def test_every_kind_on_every_op_and_glue_references():
    for op in C.CONV_OPS + C.GLUE_OPS:
        assert {c.kind for c in C.CASES if c.op == op} == set(C.KINDS_OF[op]), op
    for c in GLUE_CASES:
        ref = C.glue_reference(c, C.make_inputs(c))
        assert ref.dtype == torch.float32 and float(ref.abs().max()) > 0.0, c.id
    # the pieces of ResampleConv.backward: zero-insertion and the four phases invert each other where they meet
    c = C.BY_ID["s2d-plain-b2-64to64-6x34"]
    b = C.make_inputs(c)["b"]
    P = C.glue_reference(c, dict(a=None, b=b, mask=None))
    assert torch.equal(P[:, 3 * 64:], b[:, :, 0::2, 0::2]) and torch.equal(P[:, :64], b[:, :, 1::2, 1::2])


@pytest.mark.parametrize("mistake", C.MISTAKES)
def test_each_geometry_mistake_is_caught(mistake):
    """Broken exact equality on an `integers` case, and the per-tensor bound broken with an error of at least 1e-3 on another kind."""
    exact = loose = None
    for c in CONV_CASES:
        if not C.applies(mistake, c) or (exact if c.kind == "integers" else loose):
            continue
        _, d, ref, M, base = C.references(c.id)
        got = C.formulas(c, d, mistake)
        for n in _held(ref):
            if c.kind == "integers" and not C.passes(c, n, got[n], ref[n], M[n], base[n]):
                exact = (c.id, n)
            if c.kind != "integers" and C.relerr(got[n], ref[n]) >= 1e-3 and not C.passes(c, n, got[n], ref[n], M[n], base[n]):
                loose = (c.id, n, C.relerr(got[n], ref[n]))
    print("\n%-28s exact equality broken on %s; bound broken on %s" % (mistake, exact, loose))
    assert exact is not None and loose is not None, (mistake, exact, loose)


def test_a_mistake_that_does_not_apply_changes_nothing():
    c = C.BY_ID["final-plain-b2-64to1-5x45"]
    d = C.make_inputs(c)
    a, b = C.formulas(c, d), C.formulas(c, d, "dgrad_taps_not_flipped")
    assert all(torch.equal(a[n], b[n]) for n in a)


def test_the_documented_arithmetic_passes_and_each_arithmetic_mistake_fails():
    """The unmodified emulation passes the per-element and the per-tensor bound on every case with room for the kernels' own summation
    order; each arithmetic mistake, emulated, breaks one of them on some case; fp32 torch leaves room under the cap of the fp32 tensors."""
    caught = {m: None for m in C.ARITHMETIC_MISTAKES}
    worst = dict(ratio=0.0, emul=0.0, ref32=0.0)
    for c in CONV_CASES:
        if c.kind == "integers":
            continue
        _, d, ref, M, base = C.references(c.id)
        emu = C.emulate(c, d)
        for n in _held(ref):
            if not C.split_bf16(c, n):
                worst["ref32"] = max(worst["ref32"], base[n])
                assert 4.0 * base[n] + C.ABS <= 0.25 * C.REL_CAP, (c.id, n, base[n])
                continue
            ratio = C.worst_ratio(emu[n], ref[n], M[n])
            worst.update(ratio=max(worst["ratio"], ratio / C.PER_ELEM), emul=max(worst["emul"], base[n]))
            assert C.passes(c, n, emu[n], ref[n], M[n], base[n]), (c.id, n)
            assert ratio <= 0.5 * C.PER_ELEM and C.EMUL_FACTOR * base[n] + C.ABS <= 0.8 * C.REL_CAP, (c.id, n, ratio / C.PER_ELEM, base[n])
        for m in C.ARITHMETIC_MISTAKES:
            if caught[m] is None:
                bad = C.emulate(c, d, m)
                hit = [n for n in bad if not C.passes(c, n, bad[n], ref[n], M[n], base[n])]
                if hit:
                    caught[m] = (c.id, hit)
    print("\nemulation: worst |err| / M = %.3f x 2^-14, worst e_emul %.2e, worst e_ref32 %.2e; caught: %s" % (
        worst["ratio"], worst["emul"], worst["ref32"], caught))
    assert all(v is not None for v in caught.values()), caught


def test_weight_gradient_regimes(lib):
    seen = set()
    for c in CONV_CASES:
        tag = next((t for t in sorted(C.SLICES, key=len, reverse=True) if c.id.endswith("-" + t)), None)
        if tag is None:
            continue
        r = R.regime(lib.lib(), C.REGIME_KIND[c.op], c.B, c.cin, c.cout, c.H, c.W)
        assert C.SLICES[tag](r), (c.id, R.describe(r))
        seen.add((c.op, tag))
    assert seen == {(op, tag) for op in C.REGIME_KIND for tag in C.SLICES}


# every PRO_MASK / EPI_PLAIN instance launch_conv can pick for the training entry points (conv_mfma.hip: <MODE, WM, WN, MF, KCH, PRO,
# EPI, NSPLIT, FULLC, storage, NF, 0>): 3x3 full and half height at both cout tilings, the ragged first-layer 3x3 and 1x1, both 1x1
# tilings, 7x7 (64-cout tile only), Downsample at both tilings, and the four-phase Upsample of conv_up.hip
_I = "gtts::conv_mfma_kernel<%s, 1, 0, 2, %d, float, 2, 0>"
REQUIRED = {"3x3 64 full": _I % ("0, 1, 4, 2, 1", 1), "3x3 64 half": _I % ("0, 2, 2, 1, 1", 1), "3x3 wide full": _I % ("0, 2, 2, 2, 1", 1),
            "3x3 wide half": _I % ("0, 4, 1, 1, 1", 1), "3x3 ragged": _I % ("0, 1, 4, 2, 1", 0), "1x1 ragged": _I % ("3, 1, 4, 2, 1", 0),
            "1x1 64": _I % ("3, 1, 4, 2, 1", 1), "1x1 wide": _I % ("3, 2, 2, 2, 1", 1), "7x7": _I % ("4, 1, 4, 2, 1", 1),
            "down 64": _I % ("1, 2, 2, 1, 1", 1), "down wide": _I % ("1, 2, 2, 2, 1", 1), "up": "gtts::conv_up4_kernel"}


def test_the_catalogue_reaches_every_training_instance(lib):
    reached = {}
    for c in CONV_CASES:
        for n, name in C.instances(c, lib.conv_train_kernel_name).items():
            reached.setdefault(name, (c.id, n))
    missing = {k: v for k, v in REQUIRED.items() if v not in reached}
    assert not missing, missing
    assert set(reached) == set(REQUIRED.values()), set(reached) - set(REQUIRED.values())
    # the full-height 3x3 instances are reached by the forward of the cases made for them (a data gradient is the same call)
    for cid, key in (("c3-plain-b4-64to64-121x33-full", "3x3 64 full"), ("c3-plain-b2-128to256-61x33-full", "3x3 wide full")):
        assert C.instances(C.BY_ID[cid], lib.conv_train_kernel_name)["y"] == REQUIRED[key], cid
    # The generic CONV_UP instance of conv_mfma.hip cannot be reached from gtts_conv_resample: conv_up4_eligible asks for bf16x3, fp32
    # storage, the mask prologue, the plain epilogue, one source, shared weights and bias, cin % 16 == 0, cout 64 or a multiple of 128 and
    # an output of twice the input -- conv_train_launch sets the first seven and the entry point refuses everything else.
    for cin, cout in ((16, 64), (64, 64), (48, 128), (128, 256), (512, 128)):
        for B, H, W in ((1, 1, 1), (2, 3, 17), (16, 40, 86), (1, 1, 2048)):
            assert lib.conv_train_kernel_name("up", B, cin, cout, H, W) == REQUIRED["up"]
    for cin, cout in ((8, 64), (64, 96), (24, 128)):
        with pytest.raises(RuntimeError):
            lib.conv_train_kernel_name("up", 2, cin, cout, 3, 17)
