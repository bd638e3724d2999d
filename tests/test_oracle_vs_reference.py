"""CPU: the restatement against what the reference's Python returns on the same weights and inputs (its layout and outputs
stored in tests/golden/live_*.npz by tests/golden/make_golden_live.py).  Run live, on one machine with one thread count, the two are
bit-identical; against stored outputs the host's CPU convolutions reorder their sums with the thread count (measured here: up to
1.3e-6 of max |out|), so the stored comparison allows 1e-5."""
import torch

from live_golden import layout, live
from oracle import gradtts_oracle as O


def test_state_dict_layout_equals_reference():
    for n_spks in (1, 5):
        want = dict(layout(live(), "est_layout_s%d" % n_spks))
        got = {k: tuple(v.shape) for k, v in O.make_estimator_state(n_spks=n_spks).items()}
        assert got == want


def test_estimator_bit_identical_with_taps():
    torch.manual_seed(0)
    sd = O.make_estimator_state(seed=7)
    inp = O.make_inputs(2, 48, seed=3)
    t = torch.tensor([0.15, 0.95])
    taps = {}
    a = torch.from_numpy(live()["est_taps_out"])
    b = O.estimator_forward(sd, inp["z"], inp["mask"], inp["mu"], t, taps=taps)
    assert float((a - b).abs().max()) <= 1e-5 * float(a.abs().max())
    assert "downs.0.0.b1.raw" in taps and "ups.1.3.out" in taps and "final_block.raw" in taps


def test_reverse_diffusion_bit_identical():
    sd = O.make_estimator_state(seed=1)
    inp = O.make_inputs(1, 32, seed=4)
    a = torch.from_numpy(live()["rd3_out"])
    b = O.reverse_diffusion(sd, inp["z"], inp["mask"], inp["mu"], 3)
    assert float((a - b).abs().max()) <= 1e-5 * float(a.abs().max())
