"""Record the per-op tables (Plan.ops: label, kernel instance, algorithmic flops and bytes of every op of one U-Net call) over a grid
of plan configurations and shapes -> tests/golden/op_table.json.  No GPU: gtts_plan_op_info is host arithmetic.

The file is a record of what a KNOWN-GOOD build reports, so that a change to the launch dispatch or to the way names are derived from it
shows up as a difference (tests/test_op_table_cpu.py recomputes the table on the tree under test).  Regenerate it only for a change that
means to alter the table, and then from a build of the commit BEFORE the change plus a reviewed diff of the names -- for a refactor, from
the parent commit alone: check it out in a scratch worktree, build it there, and run this script with GTTS_LIB pointing at that library

    GTTS_LIB=<parent worktree>/speech-backbones_amd/libgradtts_gfx950.so python tests/golden/make_golden_op_table.py

Per configuration the file holds one SHA-256 per shape of the lines `label \\t kernel \\t repr(flops) \\t repr(bytes)`, and once the
sorted set of distinct kernel names of the whole grid (the "(fused into ...)" markers included)."""
import hashlib
import importlib
import itertools
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OUT = os.path.join(ROOT, "tests", "golden", "op_table.json")

SHAPES = [(B, T) for B in (1, 2, 16) for T in (32, 64, 172, 1024)]


def configs():
    """(id, Plan keyword arguments): Grad-TTS dim 64 in every precision, DiffVC at three widths; persistent convolution off and on."""
    for prec, ws, spk in itertools.product((0, 1, 2, 3), (False, True), (1, 2)):
        yield "gradtts dim=64 prec=%d ws=%d n_spks=%d" % (prec, ws, spk), dict(dim=64, precision=prec, conv_ws=ws, n_spks=spk)
    for dim, prec, ws, ref_t in itertools.product((64, 128, 256), (0, 1, 3), (False, True), (True, False)):
        yield ("diffvc dim=%d prec=%d ws=%d use_ref_t=%d" % (dim, prec, ws, ref_t),
               dict(arch=1, dim=dim, precision=prec, conv_ws=ws, use_ref_t=ref_t))


def op_table(S):
    """{"shapes", "cases": {config id: [digest per shape]}, "kernels": sorted distinct names} of the package S."""
    cases, kernels = {}, set()
    for cid, kw in configs():
        plan = S.Plan(**kw)
        digests = []
        for B, T in SHAPES:
            ops = plan.ops(B, T)
            kernels.update(k for _, k, _, _ in ops)
            text = "".join("%s\t%s\t%r\t%r\n" % op for op in ops)
            digests.append(hashlib.sha256(text.encode()).hexdigest())
        cases[cid] = digests
    return {"shapes": [list(s) for s in SHAPES], "cases": cases, "kernels": sorted(kernels)}


if __name__ == "__main__":
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    S = importlib.import_module("speech-backbones_amd")
    tab = op_table(S)
    with open(OUT, "w") as f:
        json.dump(tab, f, indent=0, sort_keys=True)
        f.write("\n")
    print("%s: library %s, %d configurations x %d shapes, %d distinct kernel names" % (
        OUT, S._lib.LIB_PATH, len(tab["cases"]), len(SHAPES), len(tab["kernels"])))
