"""CPU: the catalogue of tests/test_gpu_enc_conv_train_ops.py (tests/enc_conv_train_cases.py) reaches every regime of the Conv1d
weight-gradient launcher it claims -- Conv1dOp.wgrad_info and Conv1dOp.instance are the launchers' own arithmetic, host calls -- the
formulas of include/gradtts_abi.h equal float64 autograd, and the bound tells seven restated kernel mistakes from the kernels."""
import pytest
import torch

import enc_conv_train_cases as C


@pytest.fixture(scope="module")
def info(sba):
    return {c.id: sba.Conv1dOp(0, c.cin, c.cout, c.K, c.dil).wgrad_info(c.B, c.L) for c in C.CASES}


def test_case_ids_are_unique_and_shapes_small():
    ids = [c.id for c in C.CASES]
    assert len(set(ids)) == len(ids)
    for c in C.CASES:
        assert c.B <= 3 or c.id == "slice-empty", c.id                      # (25 chunks: the fewest that leave a slice of six empty)
        assert c.L <= 70 or c.id in ("slices-3", "slice-empty"), c.id
        assert c.cin <= 48 and c.cout <= 48 or c.B == 2 or c.id == "slice-empty", c.id      # real widths at B = 2 only


def test_the_tiling_is_the_one_the_catalogue_was_written_for(info):
    for cid, i in info.items():
        assert i[:3] == (C.TILE, C.TILE, C.CHUNK), (cid, i)


def test_catalogue_reaches_every_regime_it_claims(sba, info):
    by = C.BY_ID
    for cid, want in C.EXPECT.items():
        assert info[cid][3:] == want, (cid, info[cid])
    # partial output tiles in both dimensions, whole ones in both, and more than one tile in both
    assert any(c.cout % C.TILE and c.cin % C.TILE for c in C.CASES)
    assert any(c.cout % C.TILE == 0 and c.cin % C.TILE == 0 for c in C.CASES)
    assert any(c.cout > C.TILE and c.cout % C.TILE and c.cin > C.TILE and c.cin % C.TILE for c in C.CASES)      # a partial LAST tile behind whole ones
    assert any(c.cout == 1 for c in C.CASES) and any(c.cin == 80 for c in C.CASES)
    # more than one slice, more than one chunk per slice, an empty trailing slice
    assert any(i[3] > 1 for i in info.values()) and any(i[4] > 1 for i in info.values())
    assert info["slice-empty"][5] >= 1
    # L around the chunk: a partial only chunk, a whole one, a whole one followed by a single position
    for L in (C.CHUNK - 1, C.CHUNK, C.CHUNK + 1):
        assert any(c.L == L and c.B == 3 for c in C.CASES)
    assert any(c.L == 1 for c in C.CASES)
    # a halo that crosses the chunk edge and both ends of the sample, with a dilation
    assert any(c.dil == 3 and c.K == 5 and c.L > C.CHUNK for c in C.CASES)
    # every mask combination on one shape, ragged with a length-1 item
    combos = set((c.in_lens is not None, c.out_lens is not None) for c in C.CASES if c.id.startswith("mask-"))
    assert len(combos) == 4
    assert all(1 in (c.in_lens or c.out_lens) for c in C.CASES if c.id.startswith("mask-") and (c.in_lens or c.out_lens))
    assert any(not c.bias for c in C.CASES) and any(not c.x_grad for c in C.CASES)
    # the real widths
    have = set((c.cin, c.cout, c.K) for c in C.CASES)
    assert have >= {(192, 768, 3), (768, 192, 3), (192, 192, 5), (192, 80, 1), (80, 192, 1), (256, 1, 1), (256, 768, 3), (24, 48, 3)}
    # the forward kernel (forward and, on the channel-swapped handle, data gradient) is served for every case, on all three row tiles
    tiles = set()
    for c in C.CASES:
        tiles.add(sba.Conv1dOp(0, c.cin, c.cout, c.K, c.dil).instance(c.B, c.L, out_mask=c.out_lens is not None)[0])
        tiles.add(sba.Conv1dOp(0, c.cout, c.cin, c.K, c.dil).instance(c.B, c.L, out_mask=c.in_lens is not None)[0])
    assert tiles == {32, 64, 128}


@pytest.mark.parametrize("cid", [c.id for c in C.CASES])
def test_formulas_equal_float64_autograd(cid):
    c = C.BY_ID[cid]
    d = C.make_inputs(c)
    ref, f = C.reference(c, d), C.formulas(c, d)
    for k in ("dx", "dw", "db"):
        if ref[k] is None:
            assert f[k] is None
            continue
        assert bool(torch.isfinite(ref[k]).all()) and float(ref[k].abs().max()) > 0.0
        assert C.relerr(f[k], ref[k]) <= 1e-11, (cid, k, C.relerr(f[k], ref[k]))


SMALL = [c for c in C.CASES if c.cin * c.cout * c.K * c.B * c.L <= 5e7]


@pytest.mark.parametrize("mistake", C.MISTAKES)
def test_the_bound_tells_each_restated_mistake(mistake):
    """Each mistake moves dx, dw or db past the bound on at least one case (most of them on most)."""
    caught = []
    for c in SMALL:
        d = C.make_inputs(c)
        good, bad = C.formulas(c, d), C.formulas(c, d, mistake)
        worst = max(C.relerr(bad[k], good[k]) for k in ("dx", "dw", "db") if good[k] is not None)
        if worst > C.REL:
            caught.append((c.id, worst))
    print("%-22s caught on %d of %d cases" % (mistake, len(caught), len(SMALL)))
    assert caught, mistake
    assert all(e > 10 * C.REL for _, e in caught) or mistake == "last_chunk_dropped", caught      # nothing near the bound: a clear verdict


def test_db_bound_is_above_an_fp32_sum_and_below_a_dropped_term():
    """4 e_ref32 + 2e-6 holds for fp32 torch itself with room, and a single dropped position of db exceeds it."""
    for c in SMALL:
        if not c.bias:
            continue
        d = C.make_inputs(c)
        r64, r32 = C.reference(c, d)["db"], C.reference(c, d, torch.float32)["db"]
        e32 = C.relerr(r32, r64)
        assert e32 < 1e-5, (c.id, e32)
        dym = d["dy"].double() if d["out_mask"] is None else d["dy"].double() * d["out_mask"].double().unsqueeze(1)
        dropped = r64 - dym[0, :, 0]
        assert C.relerr(dropped, r64) > C.db_bound(e32), c.id
