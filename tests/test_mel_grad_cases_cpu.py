"""CPU tests of the log-mel gradient's yardstick (tests/mel_grad_cases.py): the hand-written float64 backward -- the formulas
csrc/mel_train.hip implements -- equals float64 autograd through the recipe on every catalogue case; every restated mistake exceeds the
bound the GPU test asserts on at least one case; the clip-side band removes at most 1 % of a case's cells; the half-clipped signal
leaves a part of the cells on the clip."""
import math

import pytest
import torch

import mel_grad_cases as C
import mel_oracle as MO

IDS = [C.case_id(c) for c in C.CASES]
# where the mistakes are looked for: three frames with both reflections, the clip, silence, ragged rows
PROBES = [("cfg1", 845, None, "noise"), ("cfg1", 845, None, "halfclip"), ("cfg1", 845, None, "zeros"), ("cfg1", 845, None, "speechlike"),
          (C.RAGGED[0], C.RAGGED[1], C.RAGGED[2], "noise")]


def test_the_catalogue_is_what_the_gpu_test_expects():
    assert len(C.CASES) == 8 * 6 and len(set(IDS)) == len(IDS)
    assert all(p in C.CASES for p in PROBES)
    assert MO.frames(MO.CFG1, 385) == 1 and MO.frames(MO.CFG1, 845) == 3 and MO.frames(MO.CFG1, C.L37) == 37
    for cfg in C.CFGS.values():                      # DC and Nyquist carry no filter weight in any configuration of the catalogue
        W = MO.filterbank64(cfg).to(torch.float32)
        assert float(W[:, 0].abs().max()) == 0.0 and float(W[:, -1].abs().max()) <= 1e-12      # (fmax = Nyquist: 8e-18 of rounding)


@pytest.mark.parametrize("case", C.CASES, ids=IDS)
def test_hand_written_backward_equals_autograd(case):
    r = C.reference(case)
    assert bool(torch.isfinite(r["ref"]).all())
    e = C.row_error(C.manual_grad(case), r["ref"])
    assert float(e.max()) <= 1e-10
    assert r["band"] <= C.CLIP_BAND_MAX_FRACTION
    tag, L, lens, name = case
    if name == "zeros":
        assert r["band"] == 0.0 and r["clipped"] == 1.0 and float(r["ref"].abs().max()) == 0.0
    if name in ("speechlike", "noise"):
        assert r["clipped"] == 0.0
    if name == "halfclip":
        assert 0.05 <= r["clipped"] <= 0.8
    if lens:
        for b, n in C.rows_of(case):
            assert float(r["ref"][b, n:].abs().max() if n < L else 0.0) == 0.0
    # the float32 run of the same recipe: what the GPU bound is a multiple of
    assert float(r["e_ref32"].max()) <= (3e-4 if name == "speechlike" else 5e-6)


@pytest.mark.parametrize("mistake", C.MISTAKES)
def test_every_restated_mistake_exceeds_the_gpu_bound_somewhere(mistake):
    margins = []
    for case in PROBES:
        r = C.reference(case)
        e = C.row_error(C.manual_grad(case, mistake), r["ref"])
        margins.append(max(float(e[b]) / C.gpu_bound(case, r["e_ref32"][b]) for b in range(MO.ROWS)))
    print("\n%-24s error / bound per probe: %s" % (mistake, " ".join("%.3g" % m for m in margins)))
    assert max(margins) > 1.0
    assert max(margins) > 4.0 or math.isinf(max(margins))          # not by a hair: at least four bounds on the best probe


def test_row_error_measure():
    ref = torch.tensor([[0.0, 2.0, -4.0], [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]], dtype=torch.float64)
    got = torch.tensor([[0.0, 2.0, -3.0], [0.0, 0.0, 0.0], [0.0, 1e-30, 0.0]], dtype=torch.float64)
    e = C.row_error(got, ref)
    assert float(e[0]) == 0.25 and float(e[1]) == 0.0 and math.isinf(float(e[2]))
    got[0, 0] = float("nan")
    assert math.isinf(float(C.row_error(got, ref)[0]))
