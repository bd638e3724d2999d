"""The guard harness of the per-op GPU parity suites (tests/test_gpu_*_ops.py, test_gpu_conv1d.py): inputs between margins that poison a
read outside them, outputs between margins and over a fill that show a write outside them and an element never written; bit-exact
repeats; the once-per-process table header; the fixtures that import the package.  Nothing here touches the GPU at import, and every
function takes the device it works on, so tests/test_gpu_guards_cpu.py proves on the CPU that each guard fires.

  inputs    fp32 between NaN margins, int32 between INT_GUARD: a kernel that reads outside a tensor computes a NaN or indexes far away
  outputs   filled with SENTINEL (int32: ISENTINEL), margins included: a surviving fill inside is an element never written, a disturbed
            one outside a write out of bounds.  "Never written" compares bit patterns.
  scratch   a workspace and its margins hold WS_BITS in every word (a NaN as fp32 and as bf16 halves, -1 as int32): a kernel that reads
            scratch it has not written, even under a factor 0, returns a NaN; the margins are compared as bits (NaN != NaN)."""
import importlib

import pytest
import torch

SENTINEL = -12345.675
ISENTINEL = -12345
NAN = float("nan")
INT_GUARD = 1 << 30
WS_BITS = -1                # 0xFFFFFFFF as int32: the fill of a workspace


def guarded(t, margin, fill, dev):
    """(view, whole): a contiguous copy of t on `dev` in the middle of a larger allocation of t's dtype filled with `fill`."""
    assert t.dtype in (torch.float32, torch.int32), t.dtype
    whole = torch.full((t.numel() + 2 * margin,), fill, dtype=t.dtype, device=dev)
    view = whole[margin:margin + t.numel()].view(t.shape)
    view.copy_(t)
    return view, whole


def guarded_inputs(d, names, margin, dev):
    """{name: view or None} of d's tensors on `dev`: fp32 between NaN margins, int32 between INT_GUARD; None stays None."""
    return {n: (None if d[n] is None else guarded(d[n], margin, NAN if d[n].dtype == torch.float32 else INT_GUARD, dev)[0]) for n in names}


class Outputs:
    """Sentinel-filled, guarded results and workspaces by name; `collect` checks them and returns CPU copies of the results."""

    def __init__(self, dev, margin):
        self.dev, self.margin, self.results, self.spaces = dev, margin, {}, {}

    def _new(self, shape, dtype, bits=None):
        """(view, whole, fill as int32 bits): filled with SENTINEL / ISENTINEL, or every word with `bits`."""
        assert dtype in (torch.float32, torch.int32), dtype
        numel = 1
        for s in shape:
            numel *= s
        if bits is None:
            fill = SENTINEL if dtype == torch.float32 else ISENTINEL
            whole = torch.full((numel + 2 * self.margin,), fill, dtype=dtype, device=self.dev)
            bits = int(torch.tensor(fill, dtype=dtype).view(torch.int32))
        else:
            whole = torch.full((numel + 2 * self.margin,), bits, dtype=torch.int32, device=self.dev).view(dtype)
        return whole[self.margin:self.margin + numel].view(shape), whole, bits

    def result(self, name, shape, dtype=torch.float32):
        self.results[name] = self._new(tuple(shape), dtype)
        return self.results[name][0]

    def with_results(self, shapes, dtypes=None):
        """result() for every {name: shape}; fp32 unless `dtypes` names another type.  Returns self."""
        for n, shape in shapes.items():
            self.result(n, shape, (dtypes or {}).get(n, torch.float32))
        return self

    def space(self, name, floats):
        """A workspace of `floats` fp32 over WS_BITS: only its margins are checked."""
        self.spaces[name] = self._new((floats,), torch.float32, WS_BITS)
        return self.spaces[name][0]

    def views(self):
        return {n: r[0] for n, r in self.results.items()}

    def view(self, name):
        return self.results[name][0] if name in self.results else None

    def collect(self, what="", head=None, values=True):
        """{name: CPU copy} of the results after asserting that both margins of every result and workspace still hold the fill and,
        with `values`, that no result element still has the fill's bits and every fp32 value is finite.  head: {name: n} -- only the
        first n elements of that result are values (behind them lies scratch of another type, which is only checked to be written)."""
        if torch.device(self.dev).type == "cuda":
            torch.cuda.synchronize()
        pre, head, got = "%s: " % what if what else "", head or {}, {}
        for store in (self.results, self.spaces):
            for n, (view, whole, fill) in store.items():
                w, m, k = whole.cpu(), self.margin, view.numel()
                ref, wb = torch.tensor(fill, dtype=torch.int32), w.view(torch.int32)
                assert bool((wb[:m] == ref).all()) and bool((wb[m + k:] == ref).all()), "%sa write outside %s" % (pre, n)
                if store is self.spaces:
                    continue
                got[n] = w[m:m + k].view(view.shape).clone()
                if not values:
                    continue
                assert not bool((got[n].view(torch.int32) == ref).any()), "%san element of %s was never written" % (pre, n)
                if w.dtype == torch.float32:
                    vals = got[n].reshape(-1)[:head[n]] if n in head else got[n]
                    assert bool(torch.isfinite(vals).all()), "%snon-finite %s (a read outside an input)" % (pre, n)
        return got


def same_bits(a, b):
    """Whether every tensor of dict a has the bits of its namesake in b (4-byte element types)."""
    return all(torch.equal(a[n].reshape(-1).view(torch.int32), b[n].reshape(-1).view(torch.int32)) for n in a)


def twice(run, what=""):
    """run() -> dict of CPU tensors, made twice; every tensor must repeat bit for bit.  Returns the first."""
    a, b = run(), run()
    for n in a:
        assert same_bits({n: a[n]}, b), "%s%s differs between two calls on the same inputs" % ("%s: " % what if what else "", n)
    return a


_ROWS_SEEN = set()


def table_row(key, header, line):
    """Print `header` the first time `key` is seen in this process, then `line`."""
    if key not in _ROWS_SEEN:
        _ROWS_SEEN.add(key)
        print(header)
    print(line)


# ------------------------------------------------------------------------------------------------------------------- fixtures
# Taken by a test module with `from gpu_guards import S, dev  # noqa: F401`.
@pytest.fixture(scope="module")
def S():
    """The product package."""
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return importlib.import_module("speech-backbones_amd")


@pytest.fixture(scope="module")
def L():
    """Its ctypes wrappers, _lib."""
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return importlib.import_module("speech-backbones_amd")._lib


@pytest.fixture(scope="module")
def TO():
    """model/_train_ops.py: the autograd Functions over the training kernels."""
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return importlib.import_module("speech-backbones_amd.model._train_ops")


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")
