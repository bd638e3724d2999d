"""CPU tests of the guard harness the per-op GPU suites share (tests/gpu_guards.py) and of the catalogues' norms (tests/case_util.py):
every guard fires on the fault it is there for, and stays quiet without one.  Nothing here runs a kernel: a "kernel" is a line of
torch on CPU tensors that writes what a correct or a faulty one would."""
import math

import pytest
import torch

import case_util as U
import gpu_guards as G

CPU = torch.device("cpu")
MARGIN = 4
F32, I32 = torch.float32, torch.int32


def test_guarded_inputs_copy_the_tensor_between_poisoned_margins():
    d = dict(x=torch.arange(6, dtype=F32).view(2, 3), idx=torch.tensor([3, 1, 2], dtype=I32), none=None)
    t = G.guarded_inputs(d, ("x", "idx", "none"), MARGIN, CPU)
    assert t["none"] is None and set(t) == {"x", "idx", "none"}
    for n, is_guard in (("x", torch.isnan), ("idx", lambda m: m == G.INT_GUARD)):
        assert torch.equal(t[n], d[n]) and t[n].dtype == d[n].dtype and t[n].is_contiguous()
        whole = t[n].untyped_storage()
        assert whole.nbytes() == 4 * (d[n].numel() + 2 * MARGIN) and t[n].storage_offset() == MARGIN
        flat = torch.empty(0, dtype=d[n].dtype).set_(whole)
        assert bool(is_guard(flat[:MARGIN]).all()) and bool(is_guard(flat[MARGIN + d[n].numel():]).all())
    view, whole = G.guarded(d["x"], MARGIN, G.SENTINEL, CPU)
    assert view.data_ptr() == whole.data_ptr() + 4 * MARGIN and bool((whole[:MARGIN] == torch.tensor(G.SENTINEL)).all())


def outputs():
    """One fp32 result of 8 elements, one int32 result of 3 and a workspace of 5 floats, all written as a correct kernel would."""
    o = G.Outputs(CPU, MARGIN)
    o.result("y", (2, 4)).copy_(torch.arange(8, dtype=F32).view(2, 4))          # (0.0 among the values: a zero is a written element)
    o.result("idx", (3,), I32).copy_(torch.tensor([0, -1, 7], dtype=I32))
    o.space("ws", 5)                                                             # a workspace may stay as it was
    return o


def whole(o, name):
    return (o.results[name] if name in o.results else o.spaces[name])[1]


def test_collect_passes_on_complete_finite_results_and_returns_cpu_copies():
    o = outputs()
    assert o.view("y") is o.views()["y"] and o.view("nope") is None and set(o.views()) == {"y", "idx"}
    got = o.collect("case-1")
    assert set(got) == {"y", "idx"}
    assert torch.equal(got["y"], torch.arange(8, dtype=F32).view(2, 4)) and torch.equal(got["idx"], torch.tensor([0, -1, 7], dtype=I32))
    got["y"].fill_(1.0)                                                          # a copy: the guarded tensor does not follow
    assert float(o.view("y")[0, 0]) == 0.0
    o2 = G.Outputs(CPU, MARGIN).with_results(dict(a=(2,), b=(1, 2)), dtypes=dict(b=I32))
    assert o2.view("a").dtype == F32 and o2.view("b").dtype == I32 and o2.view("b").shape == (1, 2)


@pytest.mark.parametrize("name", ["y", "idx", "ws"])
@pytest.mark.parametrize("at", [MARGIN - 1, -1, 0, -MARGIN])
def test_collect_sees_a_write_outside(name, at):
    """One element of the leading or the trailing margin overwritten -- the one next to the tensor or the farthest -- of a result of
    either type or of a workspace."""
    o = outputs()
    whole(o, name)[at] = 1
    with pytest.raises(AssertionError, match="^case-1: a write outside %s$" % name):
        o.collect("case-1")
    with pytest.raises(AssertionError, match="^a write outside %s$" % name):
        o.collect(values=False)                                                  # the margins are checked either way


@pytest.mark.parametrize("name,fill", [("y", G.SENTINEL), ("idx", G.ISENTINEL)])
def test_collect_sees_an_element_never_written(name, fill):
    o = outputs()
    o.view(name).view(-1)[1] = fill
    with pytest.raises(AssertionError, match="^c: an element of %s was never written$" % name):
        o.collect("c")
    assert set(o.collect("c", values=False)) == {"y", "idx"}                     # the caller makes this check itself then


@pytest.mark.parametrize("bad", [math.nan, math.inf, -math.inf])
def test_collect_sees_a_non_finite_value(bad):
    o = outputs()
    o.view("y")[1, 3] = bad
    with pytest.raises(AssertionError, match=r"^non-finite y \(a read outside an input\)$"):
        o.collect()
    assert math.isnan(bad) or float(o.collect(values=False)["y"][1, 3]) == bad


def test_head_limits_the_finite_check_and_nothing_else():
    o = outputs()
    o.view("y").view(-1)[5] = math.nan                                           # behind the first 5 elements: scratch of another type
    assert math.isnan(float(o.collect(head=dict(y=5))["y"][1, 1]))
    with pytest.raises(AssertionError, match="non-finite y"):
        o.collect(head=dict(y=6))
    o.view("y").view(-1)[7] = G.SENTINEL                                         # ... which still has to be written
    with pytest.raises(AssertionError, match="an element of y was never written"):
        o.collect(head=dict(y=5))


def test_a_workspace_is_checked_at_its_margins_only():
    o = outputs()
    ws = o.spaces["ws"][0]
    assert bool((ws.view(I32) == G.WS_BITS).all())                               # never written: collect() accepts that
    ws[2] = 7.0
    assert "ws" not in o.collect()


def test_a_workspace_lies_over_nan_bits_and_its_margins_are_compared_as_bits():
    """Every word of a workspace and of its margins is 0xFFFFFFFF: a NaN to a kernel that reads scratch before writing it, whatever factor
    it multiplies it by.  A value comparison would call every margin word disturbed (NaN != NaN), or none if it skipped NaNs."""
    o = outputs()
    view, whole_ws, bits = o.spaces["ws"]
    assert bits == G.WS_BITS == -1 and whole_ws.dtype == F32 and view.dtype == F32 and whole_ws.numel() == 5 + 2 * MARGIN
    assert bool((whole_ws.view(I32) == -1).all()) and bool(torch.isnan(whole_ws).all())
    assert bool(torch.isnan(view * 0.0).all())                                   # what a finite fill could not show
    assert view.data_ptr() == whole_ws.data_ptr() + 4 * MARGIN
    o.collect("intact")                                                          # NaN margins, untouched: no write outside
    whole_ws.view(I32)[MARGIN - 1] = 0x7FC00000                                  # another NaN: the same to `==` on floats, other bits
    with pytest.raises(AssertionError, match="^c: a write outside ws$"):
        o.collect("c")
    o = outputs()
    o.spaces["ws"][1][-1] = G.SENTINEL                                           # the results' fill is a write into a workspace margin
    with pytest.raises(AssertionError, match="^a write outside ws$"):
        o.collect()
    # results keep SENTINEL, value and bits
    assert bool((whole(outputs(), "y")[:MARGIN] == torch.tensor(G.SENTINEL)).all()) and o.results["idx"][2] == G.ISENTINEL


def test_twice_compares_bits_and_names_the_tensor():
    calls = []

    def run(flip=None):
        calls.append(1)
        r = dict(a=torch.tensor([0.0, 1.5]), n=torch.tensor([1, 2], dtype=I32), s=torch.tensor(2.0))
        if flip and len(calls) % 2 == 0:
            flip(r)
        return r

    first = G.twice(run)
    assert len(calls) == 2 and torch.equal(first["a"], torch.tensor([0.0, 1.5]))
    assert G.same_bits(run(), run())

    def negative_zero(r):
        r["a"][0] = -0.0

    def one_ulp(r):
        r["a"] = r["a"].view(I32).add(torch.tensor([0, 1], dtype=I32)).view(F32)

    def scalar(r):
        r["s"] = torch.tensor(2.5)

    assert torch.equal(torch.tensor([0.0]), torch.tensor([-0.0]))                # what a value comparison would let through
    for flip, name in ((negative_zero, "a"), (one_ulp, "a"), (scalar, "s")):
        with pytest.raises(AssertionError, match="^case-7: %s differs between two calls on the same inputs$" % name):
            G.twice(lambda: run(flip), "case-7")
    assert not G.same_bits(dict(a=torch.tensor([0.0])), dict(a=torch.tensor([-0.0])))
    nan = dict(a=torch.tensor([math.nan]))
    assert G.same_bits(nan, dict(a=torch.tensor([math.nan])))                    # the same bits are the same result, a NaN included


def test_table_row_prints_its_header_once_per_key(capsys):
    G.table_row("test-key-1", "HEADER 1", "row a")
    G.table_row("test-key-1", "HEADER 1", "row b")
    G.table_row(("test-key-2", "ln"), "HEADER 2", "row c")
    G.table_row("test-key-1", "HEADER 1", "row d")
    assert capsys.readouterr().out == "HEADER 1\nrow a\nrow b\nHEADER 2\nrow c\nrow d\n"


# ------------------------------------------------------------------------------------------------------------------- case_util
def test_relerr_propagates_a_nan():
    ref = torch.tensor([1.0, -4.0])
    assert U.relerr(torch.tensor([1.0, -3.0]), ref) == 0.25
    assert math.isnan(U.relerr(torch.tensor([math.nan, -4.0]), ref)) and math.isnan(U.relerr(ref, torch.tensor([math.nan, 1.0])))
    assert U.relerr(torch.tensor([1.0, -4.0], dtype=torch.float32), ref.double()) == 0.0


def test_relerr_zero_exact_on_an_all_zero_reference_and_with_a_scale():
    zero = torch.zeros(3)
    assert U.relerr_zero_exact(torch.zeros(3), zero) == 0.0
    assert U.relerr_zero_exact(torch.tensor([0.0, 1e-30, 0.0]), zero) == math.inf
    assert U.relerr_zero_exact(torch.tensor([0.0, 0.5, 0.0]), zero, scale=2.0) == 0.25          # a scale of its own: no exact-zero rule
    assert U.relerr_zero_exact(torch.tensor([1.0, 3.0]), torch.tensor([1.0, 2.0])) == 0.5
    assert U.relerr_zero_exact(torch.tensor([1.0, 3.0]), torch.tensor([1.0, 2.0]), scale=4.0) == 0.25
    assert U.relerr_zero_exact(0.5, 1.0) == 0.5 and U.relerr_zero_exact([0.0], [0.0]) == 0.0     # plain numbers, as the loss heads pass


def test_relerr_floor_is_finite_on_an_all_zero_reference():
    e = U.relerr_floor(torch.tensor([0.0, 1e-3]), torch.zeros(2))
    assert math.isfinite(e) and e > 1e20
    assert U.relerr_floor(torch.zeros(2), torch.zeros(2)) == 0.0
    assert U.relerr_floor(torch.tensor([1.0, 3.0]), torch.tensor([1.0, 2.0])) == 0.5


def test_seq_mask():
    want = torch.tensor([[1.0, 1.0, 1.0], [1.0, 0.0, 0.0], [0.0, 0.0, 0.0]])
    for lens in ([3, 1, 0], (3, 1, 0), torch.tensor([3, 1, 0])):
        m = U.seq_mask(lens, 3)
        assert m.dtype == torch.float32 and torch.equal(m, want)
