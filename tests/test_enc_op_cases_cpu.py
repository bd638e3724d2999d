"""CPU: the catalogue of tests/test_gpu_enc_ops.py (tests/enc_op_cases.py) is what it claims to be -- each attention case reaches the
kernel its `paths` name (gtts_enc_attention_path_for: the dispatch's own decision, host arithmetic), each score regime holds on the
float64 scores, the references are finite and two independent indexings of the relative window agree, fp32 torch stays within 2e-6
of float64 on every case, and the GPU bound tells every restated kernel mistake from the kernel on at least one case."""
import math

import pytest
import torch

import enc_op_cases as K


@pytest.fixture(scope="module")
def att():
    """{case id: (inputs, float64 reference)}, computed once; nothing below modifies it."""
    out = {}
    for c in K.ATT_CASES:
        d = K.att_inputs(c)
        out[c.id] = (d, K.att_reference(c, d))
    return out


@pytest.fixture(scope="module")
def ln():
    out = {}
    for c in K.LN_CASES:
        d = K.ln_inputs(c)
        out[c.id] = (d, K.ln_reference(c, d))
    return out


def test_case_ids_are_unique_and_shapes_small():
    ids = [c.id for c in K.ATT_CASES + K.LN_CASES]
    assert len(set(ids)) == len(ids)
    for c in K.ATT_CASES:
        assert c.B <= 3 and len(c.lens) == c.B and c.paths, c.id
        assert c.L <= 130 or (c.B == 1 and c.heads == 1 and c.dk == 96 and len(c.paths) == 1), c.id
    for c in K.LN_CASES:
        assert c.B == 2 and c.C <= 256 and c.L <= 130, c.id


# ------------------------------------------------------------------------------------------------------------------- attention
def test_every_attention_case_reaches_the_kernels_it_names(sba):
    assert K.lds16(96, 2432) == K.LDS < K.lds16(96, 2433) and K.lds8(96, 5024) == K.LDS < K.lds8(96, 5025)
    n = {8: 0, 16: 0}
    for c in K.ATT_CASES:
        elig = K.eligible_paths(c.dk, c.window, c.L)
        assert set(c.paths) <= set(elig), c.id
        chosen = sba.enc_attention_path(c.heads * c.dk, c.heads, c.window, c.L)            # what gtts_enc_forward would run
        assert chosen == (16 if 16 in elig else 8), (c.id, chosen)
        if c.L <= 130:
            assert c.paths == elig, c.id                                                   # every eligible kernel runs the case
        for p in c.paths:
            n[p] += 1
    assert n[8] == len(K.ATT_CASES) - 1 and n[16] >= 40
    by = {c.id: c for c in K.ATT_CASES}
    assert by["att-limit-h1-dk96-L2432-w4-init"].paths == (16,) and by["att-limit-h1-dk96-L5024-w4-init"].paths == (8,)
    assert sba.enc_attention_path(96, 1, 4, 2433) == 8 and sba.enc_attention_path(96, 1, 4, 5025) == 0
    for c in K.ATT_CASES:                                                                  # path 8 only: dk = 10 and window 8
        assert (16 in c.paths) == (c.dk % 4 == 0 and c.window <= 7 and c.L <= 2432), c.id


def test_attention_catalogue_keeps_its_edges():
    A = K.ATT_CASES
    for regime in ("init", "peaked"):
        assert set(c.L for c in A if c.regime == regime and (c.heads, c.dk, c.window, c.B) == (2, 48, 4, 3)) == set(K.LENGTHS)
    assert set(c.L for c in A if c.regime == "saturated") >= {5, 17, 64, 65, 130}
    assert set(c.dk for c in A) == {4, 10, 48, 96} and set(c.heads for c in A) == {1, 2, 8}
    assert set(c.window for c in A) == {0, 1, 4, 7, 8}
    assert any(c.window > c.L for c in A if 16 in c.paths) and any(c.window == 8 and c.window > c.L for c in A)
    assert any(1 in c.lens and c.L > 1 for c in A) and any(0 in c.lens for c in A)         # a length-1 item, a fully masked item
    assert all(c.lens[0] > 0 for c in A) and any(len(set(c.lens)) == 3 for c in A)
    for regime in ("init", "peaked", "saturated"):                                         # every regime on both kernels, with padding
        for p in (8, 16):
            assert any(c.regime == regime and p in c.paths and min(c.lens) < c.L for c in A), (regime, p)


def _row_stats(c, d):
    """Float64 scores of the valid rows (valid query), and the softmax of every row."""
    sc = K.att_direct(c, d, want="scores")
    valid = (d["mask"] > 0).view(c.B, 1, c.L).expand(c.B, c.heads, c.L)
    vk = (d["mask"] > 0).view(c.B, 1, 1, c.L)
    return sc, torch.softmax(sc, -1), valid, vk


def test_score_regimes_are_what_their_names_say(att):
    seen = {"init": 0, "peaked": 0, "saturated": 0}
    for c in K.ATT_SMALL:
        d = att[c.id][0]
        sc, p, valid, vk = _row_stats(c, d)
        real = sc[valid.unsqueeze(-1) & vk]                                                # scores no mask replaced
        pmax = p.max(-1).values[valid]
        seen[c.regime] += 1
        if c.regime == "init":
            if real.numel() > 8:
                assert 0.15 < float(real.std()) < 0.6, (c.id, float(real.std()))
            assert float(real.abs().max()) < 5.0, c.id
        elif c.regime == "peaked":
            assert float((pmax >= 0.9).double().mean()) >= 0.5, (c.id, float((pmax >= 0.9).double().mean()))
            assert 10.0 <= float(real.abs().max()) <= 30.0, (c.id, float(real.abs().max()))
        else:
            top2 = sc.topk(2, -1).values
            gap = (top2[..., 0] - top2[..., 1])[valid]
            assert int((gap > 100.0).sum()) >= 4 and float(real.max()) > 300.0, c.id
        # a fully masked item and padded queries: every score -1e4, the row uniform over all L keys
        dead = ~valid
        if bool(dead.any()):
            assert bool((sc[dead] == -1e4).all()) and bool((p[dead] == 1.0 / c.L).all()), c.id
    assert min(seen.values()) >= 6, seen


def test_padded_positions_hold_large_values(att):
    for c in K.ATT_CASES:
        d = att[c.id][0]
        pad = (d["mask"] == 0).unsqueeze(1).expand_as(d["q"])
        if not bool(pad.any()):
            continue
        for name, factor in (("q", 30.0), ("k", 30.0), ("v", 3.0)):
            x = d[name]
            assert float(x[pad].abs().median()) > factor * float(x[~pad].abs().median()), (c.id, name)
            assert bool(torch.isfinite(x).all())


def test_attention_references(att):
    """Finite, not degenerate, fp32 torch within 2e-6 -- and the reference's pad / reshape indexing agrees with the direct
    r = j - i + w form (two independent statements of the same window) to float64 rounding."""
    for c in K.ATT_CASES:
        d, ref = att[c.id]
        assert ref.shape == (c.B, c.heads * c.dk, c.L) and bool(torch.isfinite(ref).all()) and float(ref.abs().max()) > 0.05, c.id
        e32 = K.relerr(K.att_reference(c, d, torch.float32), ref)
        assert e32 <= K.E32_MAX, (c.id, e32)
        if c.L <= 130:
            assert K.relerr(K.att_direct(c, d), ref) <= 1e-12, c.id


def test_serial_restatement_is_the_same_attention(att):
    """att_serial_fp32 (the 8-query kernel's summation order on the CPU) is a restatement of the op, not another op."""
    for cid in ("att-len-h2-dk48-L65-w4-init", "att-len-h2-dk48-L17-w4-saturated", "att-win-h2-dk48-L17-w0-peaked"):
        c = K.ATT_BY_ID[cid]
        d, ref = att[cid]
        full = K.att_serial_fp32(c, d)
        assert K.relerr(full, ref) <= K.E32_MAX, cid
        rows = torch.arange(0, c.L, K.SERIAL_ROWS)                              # rows are independent: a subset is the same bits
        assert torch.equal(K.att_serial_fp32(c, d, rows), full[..., rows]), cid
    for cid in K.SERIAL_SUM_CASES:                                              # only where one chain runs over the kernel's longest L
        c = K.ATT_BY_ID[cid]
        assert c.paths == (8,) and K.lds8(c.dk, c.L) == K.LDS and c.regime == "init", cid


def test_bound_tells_restated_attention_mistakes_from_the_kernels(att):
    caught = {m: [] for m in K.ATT_MISTAKES}
    for c in K.ATT_SMALL:
        d, ref = att[c.id]
        b = K.bound(K.relerr(K.att_reference(c, d, torch.float32), ref))
        for m in K.ATT_MISTAKES:
            if K.exceeds(K.relerr(K.att_direct(c, d, mistake=m), ref), b):
                caught[m].append(c.id)
    print({m: len(v) for m, v in caught.items()})
    for m, ids in caught.items():
        assert ids, "no case of tests/enc_op_cases.py tells '%s' from the kernel" % m
    # what each mistake needs: a window (and more than one position), padding, more than one head, large scores
    windowed = [c.id for c in K.ATT_SMALL if c.window and c.L > 1]
    for m in ("rel-index+1", "rel-index-1", "no-rel-v", "rel-k-unscaled"):
        assert len(caught[m]) >= len(windowed) // 2, (m, len(caught[m]), len(windowed))
    assert set(caught["softmax32-no-max"]) >= set(c.id for c in K.ATT_SMALL if c.regime == "saturated")
    assert all(K.ATT_BY_ID[i].heads > 1 for i in caught["head-offset"])
    assert all(min(K.ATT_BY_ID[i].lens) < K.ATT_BY_ID[i].L for i in caught["no-key-mask"] + caught["no-query-mask"])


# ------------------------------------------------------------------------------------------------------------------- LayerNorm
def test_layernorm_catalogue_keeps_its_edges():
    Lc = K.LN_CASES
    flags = set((c.bres, c.a_mask, c.out_mask, c.relu_in, c.relu_out) for c in Lc if (c.B, c.C, c.L, c.data) == (2, 20, 17, "normal"))
    assert len(flags) == 32
    assert all(c.lens == (17, 6) for c in Lc if c.id.startswith("ln-flags"))
    want = {"prenet": (192, (False, False, False, False, True)), "norm1": (192, (True, True, False, False, False)),
            "norm2": (192, (True, False, False, False, False)), "durpred": (256, (False, False, False, True, False))}
    for site, (C, f) in want.items():
        got = [c for c in Lc if c.id.startswith("ln-%s-" % site)]
        assert set(c.L for c in got) == {1, 15, 16, 17, 130} and all(c.C == C for c in got), site
        assert all((c.bres, c.a_mask, c.out_mask, c.relu_in, c.relu_out) == f for c in got), site
    assert set(c.C for c in Lc) >= {1, 10, 16, 17, 80, 192, 256}
    assert set(c.data for c in Lc) == {"normal", "const", "lowvar", "offset"}
    assert any(c.data == "const" and c.relu_out for c in Lc) and any(c.data == "const" and not c.relu_out for c in Lc)


def test_layernorm_references_and_data_kinds(ln):
    for c in K.LN_CASES:
        d, ref = ln[c.id]
        assert ref.shape == (c.B, c.C, c.L) and bool(torch.isfinite(ref).all()) and float(ref.abs().max()) > 0.01, c.id
        e32 = K.relerr(K.ln_reference(c, d, torch.float32), ref)
        assert e32 <= K.E32_MAX, (c.id, e32)
        a = d["a"].double()
        if c.data == "const":
            beta = d["beta"].double()
            for (b, t), val in K.CONST_COLUMNS.items():
                assert bool((d["a"][b, :, t] == val).all())
                # the fp32 sum of C copies is exact in any order: val has a 2-bit mantissa, C <= 192 < 2^22
                assert float(torch.full((c.C,), val).sum()) == val * c.C and float(torch.tensor(val * c.C) / c.C) == val
                assert torch.equal(ref[b, :, t], torch.relu(beta) if c.relu_out else beta), (c.id, b, t)
            (b, t), val = K.CONST_AWKWARD
            assert bool((d["a"][b, :, t] == torch.tensor(val)).all())
            assert bool((beta > 0).any()) and bool((beta < 0).any())
        elif c.data == "lowvar":
            var = a.var(1, unbiased=False)
            assert 3e-6 < float(var.min()) and float(var.max()) < 3e-5 and float(a.mean(1).abs().max()) <= 0.06, c.id
        elif c.data == "offset":
            assert float((a.mean(1) / a.std(1)).min()) > 10.0, c.id


def test_bound_tells_restated_layernorm_mistakes_from_the_kernel(ln):
    caught = {m: [] for m in K.LN_MISTAKES}
    touched = {m: 0 for m in K.LN_MISTAKES}
    for c in K.LN_CASES:
        d, ref = ln[c.id]
        b = K.bound(K.relerr(K.ln_reference(c, d, torch.float32), ref))
        for m in K.LN_MISTAKES:
            wrong = K.ln_reference(c, d, mistake=m)
            if wrong is None:
                continue
            touched[m] += 1
            if K.exceeds(K.relerr(wrong, ref), b):
                caught[m].append(c.id)
    print({m: (len(v), touched[m]) for m, v in caught.items()})
    for m, ids in caught.items():
        assert ids, "no case of tests/enc_op_cases.py tells '%s' from the kernel" % m
    # the one-pass variance is what the offset cases are for; the flag mistakes show on every case they can touch
    assert set(caught["one-pass-fp32"]) >= set(c.id for c in K.LN_CASES if c.data == "offset")
    assert set(caught["eps-1e-5"]) >= set(c.id for c in K.LN_CASES if c.data == "lowvar")
    for m in ("unbiased", "relu-after", "mask-on-bres", "no-relu-out", "no-out-mask"):
        assert len(caught[m]) >= touched[m] - 2, (m, len(caught[m]), touched[m])


def test_bound_is_the_projects_rule():
    assert K.bound(0.0) == 2e-6 and K.bound(1e-6) == pytest.approx(6e-6) and K.bound(1e-5) == 1e-5
    assert K.exceeds(float("nan"), 1e-5) and K.exceeds(2e-5, 1e-5) and not K.exceeds(1e-6, 2e-6)
    assert math.isnan(K.relerr(torch.tensor([float("nan"), 1.0]), torch.tensor([1.0, 1.0])))
