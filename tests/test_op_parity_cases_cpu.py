"""The catalogue of tests/test_gpu_op_parity.py (tests/op_parity_cases.py) reaches every kernel instance of the U-Net's launch dispatch
and leaves no op without a checker -- proved here without a GPU: Plan.ops names the instance each op would launch (host arithmetic).

  * the kernel names of Plan(**kw).ops(B, T) over the catalogue contain every name of tests/golden/op_table.json (markers excluded);
  * every op label of every case is claimed by exactly one check kind (op_parity_cases.CLAIMS); the attention ops are counted as claimed
    by tests/test_gpu_attention.py, which owns them, and the three labels an estimator call never launches are named with the reason;
  * the edge shapes stay on the configurations that must keep them, and DiffVC dim 128, DiffVC in plain bf16 and every precision stay.
The counterpart of test_weight_gradient_cases_cover_every_regime for the inference path."""
import json
import os

import pytest

import op_parity_cases as C
from conftest import GOLDEN


@pytest.fixture(scope="module")
def tables(sba):
    """{case id: [(label, kernel)]} of the whole catalogue; one plan per configuration."""
    plans, out = {}, {}
    for case in C.CASES:
        kw = C.plan_kwargs(case)
        key = tuple(sorted(kw.items()))
        if key not in plans:
            plans[key] = sba.Plan(**kw)
        out[case.id] = [(label, kern) for label, kern, _, _ in plans[key].ops(case.B, case.T)]
    return out


def test_case_ids_are_unique_and_shapes_are_valid():
    ids = [c.id for c in C.CASES]
    assert len(set(ids)) == len(ids), sorted(i for i in ids if ids.count(i) > 1)
    for c in C.CASES:
        assert c.T % 4 == 0 and len(c.lengths) == c.B and 1 <= min(c.lengths) and max(c.lengths) <= c.T, c.id
        assert (c.T_ref in (24, 36)) == (c.arch == 1), c.id


def test_catalogue_launches_every_recorded_kernel_instance(tables):
    with open(os.path.join(GOLDEN, "op_table.json")) as f:
        recorded = set(k for k in json.load(f)["kernels"] if not k.startswith("("))
    assert len(recorded) == 98
    reached = set(k for ops in tables.values() for _, k in ops)
    missing = sorted(recorded - reached)
    print("%d cases reach %d kernel names, %d of them recorded" % (len(C.CASES), len(reached), len(reached & recorded)))
    assert not missing, "no case of tests/op_parity_cases.py launches:\n  " + "\n  ".join(missing)
    assert "gtts::tail_identity_kernel<4, __bf16, 1>" in reached      # bf16 storage at T = 4: outside the record's grid of shapes


def test_every_op_of_every_case_has_exactly_one_checker(tables):
    bad = []
    for case in C.CASES:
        for label, kern in tables[case.id]:
            kinds = C.claims(case, label, kern)
            if len(kinds) != 1:
                bad.append("%s: %s [%s] claimed by %s" % (case.id, label, kern, kinds or "no checker"))
    assert not bad, "\n".join(bad[:40])
    assert set(C.NOT_CHECKED_HERE) < set(C.CLAIMS)


def test_markers_are_claimed_by_the_op_they_name(sba):
    """'(fused into downs.0.3)' (plans without kept intermediates) belongs to the Downsample check, '(fused into the attention context
    pass)' to the identity-tail check, which reads the tensor the context pass writes."""
    case = C.CASES[0]
    kw = dict(C.plan_kwargs(case), keep_intermediates=False)
    markers = {label: kern for label, kern, _, _ in sba.Plan(**kw).ops(2, 36) if kern.startswith("(")}
    assert sorted(markers) == ["downs.0.1.tail", "downs.0.2.apply", "ups.1.1.tail"], markers
    assert C.claims(case, "downs.0.2.apply", markers["downs.0.2.apply"]) == ["downsample"]
    assert C.claims(case, "downs.0.1.tail", markers["downs.0.1.tail"]) == ["tail_identity"]


def test_catalogue_keeps_its_edge_shapes_and_configurations():
    have = set((c.arch, c.dim, c.prec, c.conv_ws, c.B, c.T, tuple(c.lengths)) for c in C.CASES)
    lost = []
    for arch, dim, prec, ws in [(0, 64, 0, False), (0, 64, 0, True), (0, 64, 3, False), (0, 64, 3, True), (1, 64, 0, False)]:
        for (B, T), lengths in (((1, 4), [3]), ((2, 36), [36, 19]), ((3, 132), [132, 67, 1]), ((16, 4), [4, 3, 2, 1] * 4)):
            if (arch, dim, prec, ws, B, T, tuple(lengths)) not in have:
                lost.append("arch %d dim %d %s conv_ws=%s at B %d, T %d, lengths %s" % (arch, dim, C.PREC_NAME[prec], ws, B, T, lengths))
    assert not lost, "edge shapes dropped from the catalogue:\n  " + "\n  ".join(lost)
    vc = [c for c in C.CASES if c.arch == 1]
    assert set(c.prec for c in vc if c.dim == 64) == {0, 1, 3}
    for dim in (128, 256):
        for prec in (0, 1, 3):
            shapes = set((c.B, c.T) for c in vc if c.dim == dim and c.prec == prec)
            assert {(1, 4), (2, 36)} <= shapes, "DiffVC dim %d %s lost one of (1, 4), (2, 36): has %s" % (dim, C.PREC_NAME[prec], sorted(shapes))
    assert any(not c.use_ref_t for c in vc) and set(c.T_ref for c in vc) == {24, 36}
    tts = [c for c in C.CASES if c.arch == 0]
    assert set(c.prec for c in tts) == {0, 1, 2, 3} and any(c.n_spks > 1 and c.prec == p for c in tts for p in (0,))
    assert any(c.n_spks > 1 and c.prec == 2 for c in tts)
