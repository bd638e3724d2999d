"""CPU tests of the fresh-memory harness (tests/alloc_poison.py): the replacement of torch.empty fills what it says and counts it, the
real function comes back on exit, and `check` fires on a CPU restatement of each mistake it is there for -- and on a closure that allocates
nothing.  Nothing here runs a kernel: a "kernel" is a few lines of torch on CPU tensors that do what a correct or a faulty one would."""
import math

import pytest
import torch

import alloc_poison as P

CPU = torch.device("cpu")
F32, I32 = torch.float32, torch.int32


def raw_bytes(t):
    store = t.untyped_storage()
    return torch.tensor(list(bytes(store.tolist())), dtype=torch.uint8) if store.nbytes() else torch.zeros(0, dtype=torch.uint8)


def want_bytes(pattern, n):
    return torch.tensor([(pattern >> (8 * (k % 4))) & 0xFF for k in range(n)], dtype=torch.uint8)


@pytest.mark.parametrize("pattern", P.PATTERNS)
def test_the_replacement_fills_every_type_and_counts(monkeypatch, pattern):
    real, real_like = torch.empty, torch.empty_like
    with P.poisoned(monkeypatch, pattern, CPU) as tally:
        assert torch.empty is not real and torch.empty_like is not real_like
        made = [torch.empty(5, dtype=F32), torch.empty((2, 3), dtype=I32), torch.empty(7, dtype=torch.uint8), torch.empty(1, dtype=torch.uint8),
                torch.empty(3, dtype=torch.bfloat16), torch.empty(2, dtype=torch.complex64), torch.empty_like(torch.ones(3, 2)),
                torch.empty((4,), dtype=F32, device=CPU)]
        nothing = torch.empty(0, dtype=F32)                                       # an empty tensor is neither filled nor counted
        assert tally.count == len(made) and tally.nbytes == 20 + 24 + 7 + 1 + 6 + 16 + 24 + 16
    assert nothing.numel() == 0
    for t in made:
        n = t.untyped_storage().nbytes()
        assert n == t.numel() * t.element_size() and torch.equal(raw_bytes(t), want_bytes(pattern, n)), (t.dtype, hex(pattern))
    f, i, b7, bf, c = made[0], made[1], made[2], made[4], made[5]
    if pattern == P.NAN_BITS:
        assert bool(torch.isnan(f).all()) and bool((i == -1).all()) and bool((b7 == 0xFF).all()) and bool(torch.isnan(bf.float()).all())
        assert bool(torch.isnan(c.real).all()) and bool(torch.isnan(c.imag).all())
    elif pattern == P.INF_BITS:
        assert bool((f == math.inf).all())
    elif pattern == P.NEG_MAX_BITS:
        assert bool((f == -torch.finfo(F32).max).all()) and float(f.sum()) == -math.inf
    else:
        assert not bool(f.any()) and not bool(i.any())


def test_only_the_device_under_test_is_filled(monkeypatch):
    with P.poisoned(monkeypatch, P.NAN_BITS, torch.device("meta")) as tally:
        t = torch.empty(4, dtype=F32).fill_(1.0)
        assert tally.count == 0 and bool((t == 1.0).all())


def test_the_real_functions_come_back(monkeypatch):
    real, real_like = torch.empty, torch.empty_like
    with P.poisoned(monkeypatch, P.NAN_BITS, CPU):
        assert torch.empty is not real
    assert torch.empty is real and torch.empty_like is real_like
    with pytest.raises(RuntimeError, match="boom"):
        with P.poisoned(monkeypatch, P.INF_BITS, CPU):
            raise RuntimeError("boom")
    assert torch.empty is real and torch.empty_like is real_like
    # a library routine that allocates its own output still works afterwards
    spec = torch.stft(torch.arange(64, dtype=F32).sin(), 16, window=torch.hann_window(16), return_complex=True)
    assert bool(torch.isfinite(torch.view_as_real(spec)).all())


X = torch.arange(1.0, 7.0)


def correct():
    """Every buffer from torch.empty, every element written before it is read."""
    scratch = torch.empty(1, dtype=F32)
    scratch.zero_()
    scratch += X.sum()
    count = torch.empty(1, dtype=I32)
    count.fill_(0)
    count += 1
    out = torch.empty(8, dtype=F32)
    out[:6] = X * float(count[0])
    out[6:] = 0.0
    return dict(out=out, total=scratch, count=count)


def sum_into_uncleared_scratch():
    scratch = torch.empty(1, dtype=F32)
    scratch += X.sum()
    return scratch


def stray_read_times_zero_mask():
    buf = torch.empty(8, dtype=F32)
    buf[:6] = X
    mask = torch.tensor([1.0] * 6 + [0.0] * 2)
    return (buf * mask).sum().reshape(1)


def masked_tail_never_written():
    out = torch.empty(8, dtype=F32)
    out[:6] = X
    return out


def counter_read_before_it_is_set():
    """A last-arriver ticket that the call never cleared: the one arrival is `last` only over zero pages."""
    ticket = torch.empty(1, dtype=I32)
    ticket += 1
    return X * 2.0 if int(ticket[0]) == 1 else X * 0.0


def test_check_passes_on_a_correct_closure_and_prints_its_row(monkeypatch, capsys):
    base = P.check(correct, monkeypatch, CPU, family="cpu-correct", shape="(6,)")
    assert torch.equal(base["out"][:6], X) and int(base["count"][0]) == 1
    row = capsys.readouterr().out
    assert "cpu-correct" in row and "(6,)" in row and "3 allocations" in row and "%d bytes" % (4 + 4 + 32) in row
    assert torch.empty is P._REAL_EMPTY


@pytest.mark.parametrize("mistake,pattern,message", [
    (sum_into_uncleared_scratch, P.NAN_BITS, "non-finite out"),
    (sum_into_uncleared_scratch, P.INF_BITS, "non-finite out"),
    (sum_into_uncleared_scratch, P.NEG_MAX_BITS, "1 of 1 elements of out differ"),
    (stray_read_times_zero_mask, P.NAN_BITS, "non-finite out"),
    (stray_read_times_zero_mask, P.INF_BITS, "non-finite out"),
    (masked_tail_never_written, P.NAN_BITS, "non-finite out"),
    (masked_tail_never_written, P.INF_BITS, "non-finite out"),
    (masked_tail_never_written, P.NEG_MAX_BITS, r"2 of 8 elements of out differ from the zero-fill run \(first at 6\)"),
    (counter_read_before_it_is_set, P.NAN_BITS, "6 of 6 elements of out differ"),
    (counter_read_before_it_is_set, P.INF_BITS, "6 of 6 elements of out differ"),
    (counter_read_before_it_is_set, P.NEG_MAX_BITS, "6 of 6 elements of out differ"),
])
def test_check_fires_on_each_mistake(monkeypatch, mistake, pattern, message):
    with pytest.raises(AssertionError, match=message):
        P.check(mistake, monkeypatch, CPU, family=mistake.__name__, patterns=(P.ZERO, pattern))
    assert torch.empty is P._REAL_EMPTY and torch.empty_like is P._REAL_EMPTY_LIKE


@pytest.mark.parametrize("mistake", [sum_into_uncleared_scratch, stray_read_times_zero_mask, masked_tail_never_written, counter_read_before_it_is_set])
def test_check_with_all_patterns_fires_on_each_mistake(monkeypatch, mistake):
    with pytest.raises(AssertionError):
        P.check(mistake, monkeypatch, CPU, family=mistake.__name__)


def test_check_fires_on_a_closure_that_allocates_nothing(monkeypatch):
    with pytest.raises(AssertionError, match="took nothing from torch.empty"):
        P.check(lambda: torch.zeros(3) + X[:3], monkeypatch, CPU, family="vacuous")
    with pytest.raises(AssertionError, match="returned no tensor"):
        P.check(lambda: [torch.empty(2) is None or None], monkeypatch, CPU, family="no-result")


def test_check_compares_bits_not_values_and_takes_nested_results(monkeypatch):
    calls = []

    def signed_zero():
        calls.append(1)
        t = torch.empty(2, dtype=F32)
        t[0] = 0.0 if len(calls) == 1 else -0.0
        t[1] = 1.0
        return [t, None, (torch.tensor([1, 2]), dict(k=torch.tensor([True])))]

    with pytest.raises(AssertionError, match=r"1 of 2 elements of 0 differ"):
        P.check(signed_zero, monkeypatch, CPU, patterns=(P.ZERO, P.NAN_BITS))
    assert set(P._named(signed_zero())) == {"0", "2.0", "2.1.k"}
    resets = []
    P.check(correct, monkeypatch, CPU, reset=lambda: resets.append(1))
    assert len(resets) == len(P.PATTERNS)
