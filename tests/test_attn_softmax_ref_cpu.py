"""The softmax reference point of the context kernels (speech-backbones_amd/csrc/attn.hip: p = exp(k - m) of the online softmax of
LinearAttention, Grad-TTS/model/diffusion.py:95) restated in float32 numpy.

One-instruction form (before):  p = exp2(fma(k, log2e, -ml2)),  ml2 = fp32(m log2e).  The fma is exact, so the maximum element's
exponent is the rounding residual of m log2e: up to half an ulp of m log2e, which is +-512 at |m| ~ 1e10.  A residual above 128
overflows p, one below -149 flushes every p of the row to 0 (Z = 0, 1 / Z = inf) -- while exp(k - max) of the reference is exactly 1
at the maximum and fp32 itself is far from its range limit.
Form the kernels use:  p = exp2((k - m) log2e): k - m is exactly 0 at the maximum, at any magnitude."""
import numpy as np

LOG2E = np.float32(1.44269504088896340736)


def p_fma_form(k, m):
    """exp2(fma(k, log2e, -fp32(m log2e))): the fma as the float32 rounding of the float64 product minus ml2 (the product of two
    float32 is exact in float64)."""
    ml2 = np.float32(m * LOG2E)
    arg = (k.astype(np.float64) * np.float64(LOG2E) - np.float64(ml2)).astype(np.float32)
    with np.errstate(over="ignore", under="ignore"):
        return np.exp2(arg)


def p_exact_form(k, m):
    """exp2((k - m) log2e): a float32 subtraction, a float32 multiply."""
    with np.errstate(under="ignore"):
        return np.exp2((k - np.float32(m)) * LOG2E)


def rows_at(scale, n=400, width=64, seed=3):
    """n rows of `width` float32 scores around `scale`, neighbours a few ulps apart; the maximum sits at a random position."""
    g = np.random.default_rng(seed)
    m = (scale * (1.0 + 3.0 * g.random(n))).astype(np.float32)
    ulp = np.spacing(m)
    k = m[:, None] - ulp[:, None] * g.integers(1, 40, (n, width)).astype(np.float32)
    k[np.arange(n), g.integers(0, width, n)] = m
    return k.astype(np.float32), m


def test_fma_form_overflows_or_empties_rows_at_1e10():
    k, m = rows_at(1e10)
    assert np.all(k.max(1) == m) and np.all(np.isfinite(k))
    p = np.stack([p_fma_form(k[i], m[i]) for i in range(len(m))])
    overflow = np.isinf(p).any(1)
    empty = (p.sum(1) == 0.0)
    print("fma form at |k| ~ 1e10: %d of %d rows overflow, %d rows are all zero" % (overflow.sum(), len(m), empty.sum()))
    assert overflow.sum() >= len(m) // 10
    assert empty.sum() >= len(m) // 10


def test_exact_form_is_finite_and_one_at_the_maximum_at_any_magnitude():
    for scale in (1.0, 30.0, 1e4, 1.5e9, 1e10, 1e20, 1e37):
        for sign in (1.0, -1.0):
            k, m = rows_at(scale)
            if sign < 0:                         # negative scores of the same magnitude: the maximum is the one nearest zero
                k = -k
                m = k.max(1)
            p = np.stack([p_exact_form(k[i], m[i]) for i in range(len(m))])
            assert np.all(np.isfinite(p)), scale
            assert np.all(p.max(1) == 1.0), scale
            assert np.all(p[k == m[:, None]] == 1.0), scale
            assert np.all(p.sum(1) >= 1.0), scale


def test_both_forms_agree_with_float64_at_ordinary_magnitudes():
    """|k| <= 30 (the fixtures reach 7): the residual of the fma form is a common factor below 2e-6 there, which the normalisation
    removes; both forms give the float64 softmax to float32 accuracy."""
    g = np.random.default_rng(5)
    k = (g.standard_normal((200, 256)) * 8.0).clip(-30, 30).astype(np.float32)
    m = k.max(1)
    want = np.exp(k.astype(np.float64) - m[:, None].astype(np.float64))
    want /= want.sum(1, keepdims=True)
    for form in (p_fma_form, p_exact_form):
        p = np.stack([form(k[i], m[i]) for i in range(len(m))]).astype(np.float64)
        got = p / p.sum(1, keepdims=True)
        assert np.abs(got - want).max() <= 1e-5 * want.max(), form.__name__
