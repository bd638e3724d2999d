"""CPU: the training catalogue tests/enc_train_op_cases.py is what tests/test_gpu_enc_train_ops.py takes it for -- the fp32 autograd
error e_ref32 of every held gradient stays under the cap its regime sets, the float64 restatement with the direct band index equals
attention_core's autograd, the backward formulas the kernels implement (att_backward_manual / ln_backward_manual) equal autograd, and
the GPU bound rejects every restated backward mistake on at least one case."""
import functools

import pytest
import torch

import enc_op_cases as K
import enc_train_op_cases as T


@functools.lru_cache(maxsize=None)
def att(cid):
    c = T.ATT_TRAIN_BY_ID[cid]
    d = T.att_train_inputs(c)
    return c, d, T.att_grads(c, d), T.att_grads(c, d, torch.float32)


@functools.lru_cache(maxsize=None)
def att_drop(cid):
    c = T.ATT_TRAIN_BY_ID[cid]
    d = T.att_train_inputs(c)
    drop = T.att_drop(c)
    return c, d, drop, T.att_grads(c, d, drop=drop), T.att_grads(c, d, torch.float32, drop=drop)


@functools.lru_cache(maxsize=None)
def ln(cid):
    c = K.LN_BY_ID[cid]
    d = K.ln_inputs(c)
    return c, d, T.ln_grads(c, d), T.ln_grads(c, d, torch.float32)


def test_catalogue_is_the_forward_catalogue_plus_one_long_case():
    assert T.ATT_TRAIN_CASES[:-1] == K.ATT_SMALL and len(K.ATT_SMALL) >= 60
    c = T.ATT_TRAIN_CASES[-1]
    assert (c.id, c.B, c.heads, c.dk, c.L, c.window, c.regime) == ("att-train-h1-dk96-L1025-w4-init", 1, 1, 96, 1025, 4, "init")
    assert c.L > 16 * 64 and c.lens[0] < c.L
    assert len(set(x.id for x in T.ATT_TRAIN_CASES)) == len(T.ATT_TRAIN_CASES)
    drops = [T.ATT_TRAIN_BY_ID[i] for i in T.DROP_IDS]
    assert set(x.regime for x in drops) == {"init", "peaked", "saturated"} and any(x.window == 0 for x in drops)
    assert any(min(x.lens) == 0 for x in drops) and any(x.dk % 4 for x in drops)
    m = T.att_drop(drops[0])
    assert set(m.unique().tolist()) == {0.0, float(torch.tensor(1.0) / 0.9)} and 0.85 < float((m > 0).float().mean()) < 0.95


@pytest.mark.parametrize("cid", [c.id for c in T.ATT_TRAIN_CASES])
def test_attention_fp32_autograd_stays_under_the_cap(cid):
    c, d, ref, r32 = att(cid)
    for n in T.ATT_GRADS:
        if ref[n] is None:
            assert not c.window and n in ("dek", "dev")
            continue
        assert bool(torch.isfinite(ref[n]).all()) and bool(torch.isfinite(r32[n]).all()), (cid, n)
        if T.held(c, n):
            e32 = T.relerr(r32[n], ref[n])
            print("%-44s %-4s max|ref| %9.3e  e_ref32 %9.2e" % (cid, n, float(ref[n].abs().max()), e32))
            assert e32 <= T.E32_CAP[c.regime], (cid, n, e32)


@pytest.mark.parametrize("cid", T.DROP_IDS)
def test_dropout_references(cid):
    c, d, drop, ref, r32 = att_drop(cid)
    for n in T.ATT_GRADS:
        if ref[n] is not None and T.held(c, n):
            assert T.relerr(r32[n], ref[n]) <= T.E32_CAP[c.regime], (cid, n)
    # the multiplier matters: the gradients differ from those without it by far more than the bound
    plain = att(cid)[2]
    assert T.relerr(ref["dv"], plain["dv"]) > 1e-3


def test_direct_restatement_is_attention_core_when_the_multiplier_is_all_ones():
    """att_direct_train (the dropout cases' reference) against attention_core's autograd at 1e-12: output and every gradient, with no
    multiplier and with a multiplier of ones."""
    for c in T.ATT_TRAIN_CASES:
        if c.L > 130:
            continue
        _, d, ref, _ = att(c.id)
        for drop in (None, torch.ones(c.B, c.heads, c.L, c.L)):
            got = T.att_grads(c, d, drop=drop, direct=True)
            for n in ("out",) + T.ATT_GRADS:
                if ref[n] is not None:
                    assert T.relerr(got[n], ref[n]) <= 1e-12, (c.id, n)


def test_the_kernels_backward_formulas_are_autograd():
    for c in T.ATT_TRAIN_CASES:
        if c.L > 130:
            continue
        _, d, ref, _ = att(c.id)
        got = T.att_backward_manual(c, d)
        for n in T.ATT_GRADS:
            if ref[n] is not None:
                assert T.relerr(got[n], ref[n]) <= 1e-11, (c.id, n, T.relerr(got[n], ref[n]))
    for cid in T.DROP_IDS:
        c, d, drop, ref, _ = att_drop(cid)
        got = T.att_backward_manual(c, d, drop=drop)
        for n in T.ATT_GRADS:
            if ref[n] is not None:
                assert T.relerr(got[n], ref[n]) <= 1e-11, (cid, n)
    for c in K.LN_CASES:
        _, d, ref, _ = ln(c.id)
        got = T.ln_backward_manual(c, d)
        for n in T.LN_GRADS:
            if ref[n] is not None:
                assert T.relerr(got[n], ref[n]) <= 1e-11, (c.id, n, T.relerr(got[n], ref[n]))


def _rejected(c, ref, r32, wrong, names, is_held):
    for n in names:
        if ref[n] is None or not is_held(n):
            continue
        if K.exceeds(T.relerr(wrong[n], ref[n]), T.bound(T.relerr(r32[n], ref[n]))):
            return True
    return False


def test_bound_tells_restated_attention_backward_mistakes_from_the_kernels():
    caught = {m: [] for m in T.ATT_TRAIN_MISTAKES}
    for c in T.ATT_TRAIN_CASES:
        if c.L > 130:
            continue
        _, d, ref, r32 = att(c.id)
        for m in T.ATT_TRAIN_MISTAKES:
            wrong = T.att_backward_manual(c, d, mistake=m)
            if wrong is not None and _rejected(c, ref, r32, wrong, T.ATT_GRADS, lambda n: T.held(c, n)):
                caught[m].append(c.id)
    for cid in T.DROP_IDS:
        c, d, drop, ref, r32 = att_drop(cid)
        wrong = T.att_backward_manual(c, d, drop=drop, mistake="drop-once")
        if _rejected(c, ref, r32, wrong, T.ATT_GRADS, lambda n: T.held(c, n)):
            caught["drop-once"].append(cid)
    print({m: len(v) for m, v in caught.items()})
    for m, ids in caught.items():
        assert ids, "no case tells '%s' from the kernels" % m
    assert all(min(T.ATT_TRAIN_BY_ID[i].lens) < T.ATT_TRAIN_BY_ID[i].L for i in caught["ds-kept-at-masked"])
    assert len(caught["drop-once"]) >= 4


def test_layernorm_fp32_autograd_stays_under_the_cap_and_mistakes_are_rejected():
    caught = {m: [] for m in T.LN_TRAIN_MISTAKES}
    touched = {m: 0 for m in T.LN_TRAIN_MISTAKES}
    for c in K.LN_CASES:
        _, d, ref, r32 = ln(c.id)
        for n in T.LN_GRADS:
            if ref[n] is None:
                assert n == "dbres" and not c.bres
                continue
            e32 = T.relerr(r32[n], ref[n])
            print("%-36s %-6s max|ref| %9.3e  e_ref32 %9.2e" % (c.id, n, float(ref[n].abs().max()), e32))
            cap = T.LN_E32_CAP_OFFSET_DGAMMA if (c.data == "offset" and n == "dgamma") else T.LN_E32_CAP
            assert e32 <= cap, (c.id, n, e32)
        for m in T.LN_TRAIN_MISTAKES:
            wrong = T.ln_backward_manual(c, d, mistake=m)
            if wrong is None:
                continue
            touched[m] += 1
            if _rejected(c, ref, r32, wrong, T.LN_GRADS, lambda n: True):
                caught[m].append(c.id)
    print({m: (len(v), touched[m]) for m, v in caught.items()})
    for m, ids in caught.items():
        assert ids, "no case tells '%s' from the kernel" % m


def test_bound_is_the_issues_rule():
    assert T.bound(0.0) == 2e-6 and T.bound(1e-6) == pytest.approx(6e-6) and T.bound(1.0) == 1e-4
    assert T.relerr(torch.zeros(3), torch.zeros(3)) == 0.0 and T.relerr(torch.tensor([0.0, 1e-30]), torch.zeros(2)) == float("inf")
    assert K.exceeds(float("nan"), 1.0)
