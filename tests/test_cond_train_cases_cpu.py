"""CPU: the catalogue of tests/cond_train_cases.py is sound.  Its float64 restatements of the kernels' contract equal float64 autograd of
the torch composition; the GPU bound (e <= 4 e_ref32 + 2e-6 and e <= 1e-4) passes the contract and rejects every restated mistake at
least tenfold on at least one case; the integer-valued cases are exact in fp32; every shape the issue of this suite names is reached."""
import functools
import itertools

import pytest
import torch

import cond_train_cases as G

FAMILY = {"F": (G.F_CASES, G.f_inputs, G.f_composition, G.f_manual, ("out", "S"), G.F_MISTAKES),
          "P": (G.P_CASES, G.p_inputs, G.p_composition, G.p_manual, ("p", "dy", "tail"), G.P_MISTAKES),
          "G": (G.G_CASES, G.g_inputs, G.g_composition, G.g_manual, G.G_TENSORS, G.G_MISTAKES)}


@functools.lru_cache(maxsize=None)
def refs(fam, cid):
    cases, inputs, comp = FAMILY[fam][:3]
    c = next(k for k in cases if k.id == cid)
    d = inputs(c)
    return c, d, comp(c, d), comp(c, d, torch.float32)


@pytest.mark.parametrize("fam,cid", [(fam, c.id) for fam in "FPG" for c in FAMILY[fam][0]])
def test_restatement_equals_float64_autograd_of_the_composition(fam, cid):
    manual, names = FAMILY[fam][3:5]
    c, d, ref, r32 = refs(fam, cid)
    got = manual(c, d)
    for n in names:
        e = G.relerr(got[n], ref[n])
        assert e <= 1e-10, (cid, n, e)
        assert G.relerr(r32[n], ref[n]) <= 2e-6, (cid, n)        # the fp32 autograd the GPU bound is scaled by is an fp32-grade answer
        if getattr(c, "ints", False):
            # small integers: every product and every partial sum is exact in fp32 (p: one division of exact operands, rounded once)
            assert torch.equal(r32[n].double(), ref[n]) or n in ("p", "dy", "tail"), (cid, n)
            if n in ("p", "dy"):
                assert torch.equal(ref[n].float(), got[n].float()), (cid, n)


@pytest.mark.parametrize("fam,mistake", [(fam, m) for fam in "FPG" for m in FAMILY[fam][5]])
def test_the_bound_rejects_the_restated_mistake(fam, mistake):
    cases, _, _, manual, names, _ = FAMILY[fam]
    worst = 0.0
    for c0 in cases:
        if c0.H * c0.W > 2000:              # (the small planes show every mistake; the large ones only cost time)
            continue
        c, d, ref, r32 = refs(fam, c0.id)
        got = manual(c, d, mistake)
        for n in names:
            worst = max(worst, G.relerr(got[n], ref[n]) / G.bound(G.relerr(r32[n], ref[n])))
    assert worst >= 10.0, (mistake, worst)


def test_time_bias_before_the_glu_is_another_function():
    """The restated mistake is the float64 autograd of that other composition -- so the bound rejects the thing it names."""
    for c0 in G.G_CASES:
        c, d, _, _ = refs("G", c0.id)
        other, got = G.g_composition(c, d, mistake="tb_before_glu"), G.g_manual(c, d, "tb_before_glu")
        assert all(G.relerr(got[n], other[n]) <= 1e-10 for n in G.G_TENSORS), c.id


def test_the_catalogue_holds_what_the_kernels_can_get_wrong():
    for cases in (G.F_CASES, G.P_CASES):
        plain = [c for c in cases if not c.ints]
        assert {(c.H, c.W) for c in plain} == set(itertools.product((1, 2, 3, 80), (1, 2, 3, 5, 67, 130)))
        assert {c.B for c in plain} == {1, 3} and {c.C for c in plain} == {64, 256} and {c.mask for c in plain} == set(G.MASK_KINDS)
        assert {(c.B, c.C) for c in plain} == {(1, 64), (3, 64), (1, 256), (3, 256)}
        assert any(c.ints and c.H * c.W > 256 for c in cases) and any(c.ints and c.H * c.W < 64 for c in cases)
        # every mask kind meets a plane with both neighbours (W >= 3) and more than one row
        assert {c.mask for c in plain if c.W >= 3 and c.H >= 2} == set(G.MASK_KINDS)
    assert {(c.taps, c.base) for c in G.F_CASES} == {(9, True), (9, False), (1, True), (1, False)}
    assert len({c.id for c in G.F_CASES}) == len(G.F_CASES) and len({c.id for c in G.P_CASES}) == len(G.P_CASES)
    # masks: a sample of length 1, ragged tails, interior holes (a dead column with live neighbours on both sides)
    m = G.make_mask("len1", 3, 67)
    assert m.sum(1).tolist() == [67.0, 1.0, 34.0] and G.make_mask("len1", 1, 5).sum().item() == 1.0
    assert G.make_mask("ragged", 3, 130).sum(1).tolist() == [130.0, 66.0, 129.0]
    h = G.make_mask("holes", 3, 67)
    assert bool(((h[:, 1:-1] == 0) & (h[:, :-2] == 1) & (h[:, 2:] == 1)).any()) and bool((h.sum(1) >= 1).all())
    for kind in G.MASK_KINDS:
        for B, W in ((1, 1), (3, 1), (1, 2), (3, 3)):
            assert bool((G.make_mask(kind, B, W).sum(1) >= 1).all()), (kind, B, W)
    # narrow convolutions: the three layer kinds on the four planes, with and without the output mask
    assert {(c.cin, c.cout) for c in G.N_CASES} == {(1, 64), (32, 64), (32, 128)}
    for kind in ((1, 64), (32, 64), (32, 128)):
        assert {(c.H, c.W) for c in G.N_CASES if (c.cin, c.cout) == kind} == {(1, 1), (3, 5), (17, 130), (80, 36)}
    assert {c.omask for c in G.N_CASES} == {True, False}


@pytest.mark.parametrize("cid", [c.id for c in G.N_CASES if c.H * c.W <= 2500])
def test_narrow_convolution_reference_is_an_fp32_grade_answer(cid):
    c = G.N_BY_ID[cid]
    d = G.n_inputs(c)
    ref, r32 = G.n_composition(c, d), G.n_composition(c, d, torch.float32)
    for n in ("y", "dw", "db", "dx"):
        assert G.relerr(r32[n], ref[n]) <= 4e-6, (cid, n)
    # a masked input column carries no data gradient, and with the output mask a masked output column is zero
    dead = (1.0 - d["mask"])[:, None, None, :].double()
    assert float((ref["dx"] * dead).abs().max()) == 0.0 and (not c.omask or float((ref["y"] * dead).abs().max()) == 0.0)
