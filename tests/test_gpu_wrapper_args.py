"""GPU: every module-level wrapper of the binding checks every tensor it passes before it launches.  The binding's one launch call is
replaced by a recorder that launches nothing, so a missing check shows as a failed assertion and never as a stray read: (a) the valid
call of tests/wrapper_arg_cases.py reaches the recorder with the expected entry point; (b) every mismatch raises the binding's
ArgumentError (one type for every wrapper family, a ValueError and a RuntimeError) with a message that names the argument, and the
recorder is not reached.  That the valid calls compute the right thing is what the per-op suites hold; that no wrapper is missing
from the table, tests/test_wrapper_args_cpu.py."""
import pytest
import torch

from conftest import pkg
from wrapper_arg_cases import CASES, Z


class _Reached(Exception):
    pass


@pytest.fixture(scope="module")
def L():
    return pkg()._lib


@pytest.fixture()
def launches(L, monkeypatch):
    names = type("Names", (list,), {"stop": False})()

    def record(device, name, *args):
        assert device.type == "cuda", (name, device)
        names.append(name)
        if names.stop:
            raise _Reached(name)

    monkeypatch.setattr(L, "_launch", record)
    yield names
    L.clear_packed_cache()      # (the blobs "packed" under the recorder hold nothing)


def _run(L, case, kw):
    if "call" in case:
        return case["call"](L, kw)
    return getattr(L, case["fn"])(**kw)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_every_tensor_is_checked_before_the_launch(case, L, launches):
    dev = torch.device("cuda", torch.cuda.current_device())
    launches.stop = bool(case.get("stop"))
    kw = case["args"](L, dev)
    if launches.stop:
        with pytest.raises(_Reached):
            _run(L, case, kw)
    else:
        _run(L, case, kw)
    assert launches and launches[-1] == case["entry"], (case["id"], list(launches))
    tensors = [n for n, v in kw.items() if torch.is_tensor(v)]
    assert set(case["bad"]) == set(tensors) or len(tensors) == 1, (case["id"], "a tensor argument without a mismatch", tensors)
    for name, wrong in case["bad"].items():
        shape, named = wrong if isinstance(wrong[0], tuple) else (wrong, name)
        del launches[:]
        with pytest.raises(L.ArgumentError) as ei:
            _run(L, case, dict(kw, **{name: Z(dev, *shape, dtype=kw[name].dtype)}))
        assert named in str(ei.value), (case["id"], name, str(ei.value))
        assert not launches, (case["id"], name, list(launches))
