"""The per-op table (Plan.ops / gtts_plan_op_info) against a record, and its kernel names against the library -- no GPU.

The launchers name the kernel instance they would launch (csrc/common.h: launch or describe), so a reported name follows the launch
dispatch by construction.  What is left to check: that the table is what it was (tests/golden/op_table.json, recorded from a build of
the commit before the table's code last changed -- see tests/golden/make_golden_op_table.py), and that every name is a kernel of the
library, spelled as a demangler and rocprofv3 spell it: a name that is not fails to join in a profile without any error."""
import importlib.util
import os
import json
import subprocess

import pytest

import abi_util
from conftest import GOLDEN, ROOT

_spec = importlib.util.spec_from_file_location("make_golden_op_table", os.path.join(GOLDEN, "make_golden_op_table.py"))
_gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_gen)


@pytest.fixture(scope="module")
def table(sba):
    return _gen.op_table(sba)


@pytest.fixture(scope="module")
def recorded():
    with open(os.path.join(GOLDEN, "op_table.json")) as f:
        return json.load(f)


def test_grid_is_the_recorded_grid(table, recorded):
    assert table["shapes"] == recorded["shapes"]
    assert sorted(table["cases"]) == sorted(recorded["cases"])
    assert len(table["cases"]) == 52 and len(table["shapes"]) == 12


def test_op_tables_match_the_record(table, recorded):
    """Labels, kernel names, flops and bytes of every op, string for string and bit for bit (repr of the doubles)."""
    diff = ["%s B=%d T=%d" % (cid, B, T) for cid in recorded["cases"]
            for (B, T), got, want in zip(_gen.SHAPES, table["cases"][cid], recorded["cases"][cid]) if got != want]
    assert not diff, "%d of %d op tables differ from the record, e.g. %s" % (len(diff), 52 * 12, diff[:5])


def test_kernel_names_match_the_record(table, recorded):
    assert table["kernels"] == recorded["kernels"]


def _library_kernels(path):
    """Names of the __global__ functions of the library: its host stubs, demangled, without `__device_stub__`, the return type that
    a template instance's name carries and the parameter list."""
    syms = [line.split()[-1] for line in abi_util.nm(path).splitlines()]
    stubs = [s for s in syms if "__device_stub__" in s]
    # binutils' demangler predates the Itanium ABI's code for __bf16 (DF16b); the vendor-extended spelling demangles to the same text
    plain = subprocess.run(["c++filt"], input="\n".join(stubs).replace("DF16b", "u6__bf16"), stdout=subprocess.PIPE, check=True,
                           universal_newlines=True).stdout.splitlines()
    names = set()
    for s in plain:
        s = s.replace("__device_stub__", "")
        if s.startswith("void "):
            s = s[len("void "):]
        depth = 0
        for k, ch in enumerate(s):      # cut the parameter list: the first '(' outside the template argument list
            depth += (ch == "<") - (ch == ">")
            if ch == "(" and depth == 0:
                s = s[:k]
                break
        names.add(s)
    return names


def test_every_reported_name_is_a_kernel_of_the_library(sba, table):
    have = _library_kernels(sba._lib.LIB_PATH)
    assert len(have) > 100, "no kernels found in %s (%d): nm / c++filt output changed?" % (sba._lib.LIB_PATH, len(have))
    names = [k for k in table["kernels"] if not k.startswith("(")]
    assert names
    missing = [k for k in names if k not in have]
    assert not missing, "reported but not in the library: %s" % missing


def test_plan_source_holds_no_kernel_instance_names():
    """The op program (csrc/plan.hip) keeps labels, the '(fused into ...)' markers and the flop / byte model; which template instance
    runs an op is the launchers' knowledge alone."""
    with open(os.path.join(ROOT, "speech-backbones_amd", "csrc", "plan.hip")) as f:
        src = f.read()
    assert "_kernel<" not in src
    assert "conv_kernel_name" not in src and "GTTS_ATTN_HPW" not in src
