"""What the host-side ABI tests (tests/test_abi.py, tests/test_*_abi_cpu.py) share: the error codes of include/gradtts_abi.h, the library's
exported symbols, the `S` fixture with its "run build() first" assertion, fake device addresses, and the header's prototypes as
argument kinds -- what ctypes has to be told about each entry point."""
import ctypes
import os
import re
import subprocess

import pytest

from conftest import ROOT, pkg

OK, E_NULL, E_SHAPE, E_CONFIG, E_HIP, E_PARAMS, E_WORKSPACE, E_RANGE = 0, -1, -2, -3, -4, -5, -6, -7      # GTTS_OK, GTTS_E_* of the header
HEADER = os.path.join(ROOT, "include", "gradtts_abi.h")


@pytest.fixture(scope="module")
def S():
    mod = pkg()
    assert os.path.exists(mod._lib.LIB_PATH), "run __graft_entry__.build() first"
    return mod


@pytest.fixture(scope="module")
def L(S):
    """The loaded library object."""
    return S._lib.lib()


def _fake(n=1):
    """n non-null host addresses: validation must fail before any of them is dereferenced or handed to the device."""
    return [ctypes.c_void_p(0x1000 * (i + 1)) for i in range(n)]


def nm(path=None):
    """What `nm -D --defined-only` prints for the built library."""
    return subprocess.check_output(["nm", "-D", "--defined-only", path or pkg()._lib.LIB_PATH]).decode()


def exported(path=None):
    """The gtts_* symbols the built library defines."""
    return set(re.findall(r"\bT (gtts_[a-z_0-9]+)", nm(path)))


def header_text():
    """include/gradtts_abi.h without comments and preprocessor lines (plain C is left)."""
    src = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    src = re.sub(r"//[^\n]*", " ", src)
    return "\n".join(ln for ln in src.splitlines() if not ln.lstrip().startswith("#"))


def declared():
    """Sorted names of every entry point the header declares."""
    return sorted(prototypes())


def _kind(decl):
    """The kind of one C parameter or return type: 'ptr' (any pointer, array parameter or gtts_stream_t), 'int', 'float', 'double',
    'size_t' or 'void'."""
    decl = decl.strip()
    if "*" in decl or "[" in decl or re.search(r"\bgtts_stream_t\b", decl):
        return "ptr"
    words = [w for w in re.findall(r"[A-Za-z_]\w*", decl) if w not in ("const", "extern", "unsigned", "signed")]
    kind = words[0] if words else "int"                                      # (`unsigned` alone is an int)
    if kind in ("size_t", "double", "float", "int", "void"):
        return kind
    raise ValueError("a parameter the ABI tests cannot map: %r" % decl)


def prototypes():
    """{entry point: (return kind, [argument kinds])} of every prototype in the header."""
    protos = {}
    for m in re.finditer(r"([^;{}()]*?)\b(gtts_\w+)\s*\(([^()]*)\)\s*;", header_text()):
        ret, name, params = m.group(1), m.group(2), m.group(3).strip()
        args = [] if params in ("", "void") else [_kind(p) for p in params.split(",")]
        assert name not in protos, "declared twice: %s" % name
        protos[name] = (_kind(ret), args)
    return protos


_CTYPES_KINDS = {ctypes.c_int: "int", ctypes.c_float: "float", ctypes.c_double: "double", ctypes.c_size_t: "size_t", None: "void"}


def ctypes_kind(t):
    """The same kinds for what a binding sets as argtypes / restype (every pointer type, c_void_p, c_char_p and arrays: 'ptr')."""
    if t in _CTYPES_KINDS:
        return _CTYPES_KINDS[t]
    if t in (ctypes.c_void_p, ctypes.c_char_p) or issubclass(t, (ctypes._Pointer, ctypes.Array)):
        return "ptr"
    raise ValueError("a ctypes type the ABI tests cannot map: %r" % (t,))
