"""CPU: the catalogue of tests/dec_train_op_cases.py is sound.  The float64 restatements of the kernels' headers (forward and manual
backward formulas) equal float64 autograd of the plain torch expressions to 1e-12; the fp32 reference stays under the catalogue's caps
on every held (case, tensor), and four times a cap stays under the tensor's hard bound, so no case can fail on its reference alone; the
GPU bound rejects every restated mistake on at least one case; every case is reached."""
import functools

import pytest
import torch

import dec_train_op_cases as D

SEEN = set()


@functools.lru_cache(maxsize=None)
def refs(fam, cid):
    cases, inputs, reference, _, _ = D.FAMILIES[fam]
    c = next(k for k in cases if k.id == cid)
    d = inputs(c)
    ref = reference(c, d)
    return c, d, ref, D.errors(fam, reference(c, d, torch.float32), ref)


def _ids():
    return [(fam, c.id) for fam in D.FAMILIES for c in D.FAMILIES[fam][0]]


@pytest.mark.parametrize("fam,cid", _ids())
def test_restatement_equals_autograd_and_the_fp32_reference_stays_under_its_cap(fam, cid):
    manual = D.FAMILIES[fam][3]
    c, d, ref, e32 = refs(fam, cid)
    kind = D.kind_of(fam, c)
    if manual is not None:
        for n, e in D.errors(fam, manual(c, d), ref).items():
            assert e <= 1e-12, (cid, n, e)
    assert set(e32) == {n for n in D.HELD[fam] if ref.get(n) is not None}
    for n, e in e32.items():
        if D.is_held(fam, kind, n):
            assert e <= D.e32_cap(fam, kind, n), (cid, n, e)
    SEEN.add(cid)


def test_no_case_can_fail_on_its_reference_alone():
    """Four times every cap on e_ref32 lies under the tensor's hard cap; what `offset300` leaves unheld is what has no room for such a
    cap at twice the measured e_ref32."""
    for fam in D.FAMILIES:
        for c in D.FAMILIES[fam][0]:
            kind = D.kind_of(fam, c)
            for n in D.HELD[fam]:
                if D.is_held(fam, kind, n) and n not in ("stat_max", "dg_cs"):
                    assert 4.0 * D.e32_cap(fam, kind, n) <= D.cap(n), (fam, kind, n)
    for fam, names in (("GN", ("out", "dy", "dgamma", "dbeta")), ("IN", ("out",))):
        worst = {n: 0.0 for n in names}
        for c in D.FAMILIES[fam][0]:
            if c.kind == "offset300":
                e32 = refs(fam, c.id)[3]
                worst = {n: max(worst[n], e32[n]) for n in names}
        assert all(8.0 * worst[n] > D.cap(n) for n in names), (fam, worst)
        assert set(D.HELD[fam]) - set(D.HELD_ONLY[fam, "offset300"]) - {"dtb"} == set(names)


def test_the_catalogue_holds_what_the_kernels_can_get_wrong():
    shapes = {tuple(c[1:6]) for c in D.GN_CASES}
    assert shapes == {(2, 16, 5, 7, 8), (2, 8, 4, 9, 8), (3, 64, 8, 131, 8), (1, 32, 32, 32, 4), (1, 512, 1, 16, 8), (40, 8, 1, 4, 8)}
    for s in ((2, 16, 5, 7, 8), (2, 8, 4, 9, 8), (3, 64, 8, 131, 8)):
        assert {c.kind for c in D.GN_CASES if tuple(c[1:6]) == s and c.tb} == set(D.KINDS)
        assert any(tuple(c[1:6]) == s and not c.tb for c in D.GN_CASES)
    assert {(c.B, c.C, c.H, c.W) for c in D.IN_CASES} == {(2, 4, 5, 7), (1, 3, 16, 16), (2, 8, 8, 131)}
    assert all({c.kind for c in D.IN_CASES if (c.B, c.C, c.H, c.W) == s} == set(D.KINDS) for s in ((2, 4, 5, 7), (1, 3, 16, 16), (2, 8, 8, 131)))
    assert {"offset30", "offset300", "plain", "short", "saturated"} <= set(D.KINDS)
    assert D._lens(3, 131) == [131, 1, 66]
    # the saturated kind reaches both Mish tails and the clamp at 40
    c = D.GN_BY_ID["gn-b3-c64-8x131-g8-saturated-tb"]
    d = D.gn_inputs(c)
    z = torch.nn.functional.group_norm(d["y"].double(), c.groups, d["gamma"].double(), d["beta"].double(), D.EPS)
    assert float(z.max()) > 40.0 and float(z.min()) < -40.0
    # the short kind: a masked column holds the channel's bias alone
    d = D.gn_inputs(D.GN_BY_ID["gn-b2-c16-5x7-g8-short-tb"])
    assert bool((d["y"][1, :, :, 1:] == d["y"][1, :, :1, 1:2]).all()) and not bool((d["y"][0, :, :, 1:] == d["y"][0, :, :1, 1:2]).all())
    # attention: every N with the three regimes, the two slice-order regimes from 513 pixels on
    assert D.AT_NS == (1, 7, 64, 65, 257, 512, 513, 1025)
    assert {(c.N, c.regime) for c in D.AT_CASES} == ({(n, r) for n in D.AT_NS for r in ("flat", "peaked", "shifted")} |
                                                    {(n, r) for n in (513, 1025) for r in ("late-max", "early-max")})
    for c in D.AT_CASES:
        k = D._split(D.at_inputs(c)["qkv"])[1]
        if c.regime == "shifted":
            assert float(k[:, :, 1::2].min()) > 70.0 and float(k[:, :, 0::2].max()) < 10.0       # exp(80) overflows fp32 at 88.7 with the sum
        if c.regime in ("late-max", "early-max"):
            m = torch.stack([k[..., n0:n0 + D.AT_SLICE].max(-1).values for n0 in range(0, c.N, D.AT_SLICE)])
            top = m.argmax(0)
            assert bool((top == (m.shape[0] - 1 if c.regime == "late-max" else 0)).all())
            assert float((m.max(0).values - m.min(0).values).min()) > 90.0       # e^{m_s - M} underflows in fp32
    # at one pixel the softmax is 1 and dk is exactly zero in float64
    assert float(refs("AT", "attn-n1-flat")[2]["dk"].abs().max()) == 0.0 and refs("AT", "attn-n1-flat")[2]["dk_scale"] > 0.0
    # Rezero: below one float4 per workgroup, ragged blocks, and one float4 past a full grid of 2048 x 256
    assert {c.n for c in D.RZ_CASES} == {4, 1020, 1028, 2097156}
    # noising: the old shape and one whose last 256-block is ragged; both ends of t
    assert [(c.B, c.F, c.T) for c in D.NZ_CASES] == [(3, 80, 52), (2, 5, 51)] and 2 * 5 * 51 % 256 != 0
    for c in D.NZ_CASES:
        assert min(c.t) == 1e-5 and max(c.t) == 1.0


@pytest.mark.parametrize("fam,mistake", [(fam, m) for fam in D.FAMILIES for m in D.FAMILIES[fam][4]])
def test_the_bound_rejects_each_restated_mistake(fam, mistake):
    cases, _, _, manual, _ = D.FAMILIES[fam]
    broken = []
    for c in cases:
        c, d, ref, e32 = refs(fam, c.id)
        kind = D.kind_of(fam, c)
        for n, e in D.errors(fam, manual(c, d, mistake), ref).items():
            if D.is_held(fam, kind, n) and not D.passes(n, e, e32[n]):
                broken.append((c.id, n, e))
    assert broken, mistake
    assert max(e for _, _, e in broken) >= 1e-3, (mistake, broken)      # far outside the bound, not at its edge


def test_no_case_was_skipped():
    assert SEEN == {cid for _, cid in _ids()}, sorted({cid for _, cid in _ids()} - SEEN)
