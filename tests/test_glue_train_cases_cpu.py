"""CPU: the catalogue of tests/glue_train_cases.py is sound.  Its float64 restatements of the kernels' contract equal float64 autograd
of the repository's composition; the GPU bound (e <= 4 e_ref32 + 2e-6 and e <= 1e-4; torch.equal for copies and counts) passes the
contract and rejects every restated mistake at least tenfold on at least one case; every case is reached."""
import functools

import pytest
import torch

import glue_train_cases as G

FAMILY = {"A": (G.A_CASES, G.a_inputs, G.a_composition, G.a_manual, ("dx",), ()),
          "B": (G.B_CASES, G.b_inputs, G.b_composition, G.b_manual, ("dx0", "dmu"), ()),
          "C": (G.C_CASES, G.c_inputs, G.c_composition, G.c_manual, G.C_BOUNDED, ("y_c", "mu_y"))}
SEEN = set()


@functools.lru_cache(maxsize=None)
def refs(fam, cid):
    cases, inputs, comp, manual, _, _ = FAMILY[fam]
    c = next(k for k in cases if k.id == cid)
    d = inputs(c)
    return c, d, comp(c, d), comp(c, d, torch.float32)


def _ids():
    return [(fam, c.id) for fam in "ABC" for c in FAMILY[fam][0]]


@pytest.mark.parametrize("fam,cid", _ids())
def test_restatement_equals_float64_autograd_of_the_composition(fam, cid):
    _, _, _, manual, bounded, copies = FAMILY[fam]
    c, d, ref, r32 = refs(fam, cid)
    got = manual(c, d)
    for n in bounded:
        e = G.relerr(got[n], ref[n])
        assert e <= 1e-12, (cid, n, e)
        # the fp32 autograd the GPU bound is scaled by is itself an fp32-grade answer
        assert G.relerr(r32[n], ref[n]) <= 2e-6, (cid, n, G.relerr(r32[n], ref[n]))
    for n in copies:
        assert torch.equal(got[n], ref[n]), (cid, n)                     # exact in float64 ...
        assert torch.equal(got[n].float(), r32[n]), (cid, n)             # ... and in fp32: one term times 1.0 plus zeros
    if fam == "C":
        idx, dur, first = G.c_index(d)
        assert torch.equal(dur, d["path"].sum(-1)) and idx.dtype == torch.int32 and first.dtype == torch.int32
        for b in range(c.B):
            for i in range(c.tx):
                run = (idx[b] == i).nonzero().flatten().tolist()
                assert len(run) == int(dur[b, i]) and (run == list(range(int(first[b, i]), int(first[b, i]) + len(run))) if run else first[b, i] == -1)
    SEEN.add(cid)


def test_the_catalogue_holds_what_the_kernels_can_get_wrong():
    assert [tuple(c[1:]) for c in G.A_CASES] == [(1, 2, 5, 4, 64, 3), (2, 3, 7, 68, 64, 1), (2, 2, 80, 44, 128, 3), (3, 3, 80, 172, 64, 3),
                                                 (3, 2, 80, 172, 64, 1)]
    assert [(c.B, c.F, c.T) for c in G.B_CASES] == [(1, 80, 4), (3, 80, 44), (2, 5, 172)]
    assert [tuple(c[1:]) for c in G.C_CASES] == [(3, 80, 7, 23, None), (3, 80, 7, 23, 8), (3, 80, 7, 23, 16), (2, 80, 40, 130, 48), (1, 5, 1, 3, None)]
    # A: a full sample, one cut mid-row, one of length 1; more than one tile of 512 pixels; both kernel sizes and plane counts
    assert G._lens(3, 172) == [172, 87, 1]
    assert {(c.cin, c.k) for c in G.A_CASES} == {(2, 3), (3, 1), (3, 3), (2, 1)} and any(c.H * c.W > 512 for c in G.A_CASES)
    # B: every t regime
    ts = [t for c in G.B_CASES for t in c.t]
    assert min(ts) == pytest.approx(1e-5) and 0.5 in ts and max(ts) == pytest.approx(1.0 - 1e-5)
    # C: padded tokens and frames, a y_length below out_size, a start inside a token's run, a token left without a live frame
    cut = dead = short = 0
    for c in G.C_CASES:
        d = G.c_inputs(c)
        idx, dur, first = G.c_index(d)
        kept = G.c_kept(c, d).tolist()
        if c.B > 1:
            assert int(d["x_lengths"].min()) < c.tx and int(d["y_lengths"].min()) < c.T
        if c.out_size is None:
            continue
        short += any(int(n) < c.out_size for n in d["y_lengths"])
        for b in range(c.B):
            s = d["starts"][b]
            assert 0 <= s <= max(int(d["y_lengths"][b]) - c.out_size, 0)
            cut += s > 0 and int(idx[b, s - 1]) == int(idx[b, s])
            for i in range(int(d["x_lengths"][b])):
                dead += min(int(first[b, i]) + int(dur[b, i]) - s, kept[b]) <= max(int(first[b, i]) - s, 0)
    assert cut >= 2 and dead >= 2 and short >= 2, (cut, dead, short)


@pytest.mark.parametrize("mistake", sorted(G.MISTAKES))
def test_the_bound_rejects_each_restated_mistake_tenfold(mistake):
    fam = G.MISTAKES[mistake]
    cases, _, _, manual, bounded, copies = FAMILY[fam]
    worst = 0.0
    for c in cases:
        c, d, ref, r32 = refs(fam, c.id)
        bad = manual(c, d, mistake)
        for n in bounded:
            worst = max(worst, G.relerr(bad[n], ref[n]) / G.bound(G.relerr(r32[n], ref[n])))
        for n in copies:
            if not torch.equal(bad[n], ref[n]):
                worst = float("inf")
    assert worst >= 10.0, (mistake, worst)


def test_no_case_was_skipped():
    assert SEEN == {cid for _, cid in _ids()}, sorted({cid for _, cid in _ids()} - SEEN)
