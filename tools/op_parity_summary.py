"""Condense the -s output of tests/test_gpu_op_parity.py (one row per op and case, some 4 400 lines) into the tables of
profiles/op_parity.txt: the worst row per op kind and precision, per kernel instance and precision, and per case.

    python -m pytest tests/test_gpu_op_parity.py -q -m gpu -s > run.txt
    python tools/op_parity_summary.py run.txt > tables.txt

"worst e" is the largest e_kernel (own error, bound and place are that row's), e/bound the largest ratio; a GroupNorm / InstanceNorm row counts twice (scale, shift)."""
import collections
import re
import sys

ROW = re.compile(r"^\.?(?P<label>\S+)(?P<what> .*?)?\s+(?P<kernel>[a-z0-9_]+_kernel(?:<[^>]*>)?|\(fused[^)]*\))\s+(?P<shape>\d+(?:x\d+)*)\s+(?P<figs>e_kernel .*)$")
FIG = re.compile(r"e_kernel (\S+) (\S+)\s+(\S+) bound (\S+)")
VSFMT = re.compile(r"e_vs_fmt (\S+)")
KINDS = (("time_mlp", "time_mlp"), ("spk_mlp", "spk_mlp"), ("cond_block", "vc_cond"), ("ref.pool", "ref_pool"), ("prep_input", "exact copy"),
         (".in", "InstanceNorm"), (".gn", "GroupNorm"), (".res_tail", "tail (1x1 res_conv)"), (".tail", "tail (identity)"),
         ("final_conv+euler", "final_conv"))


def kind(label, what, kernel):
    if "copy" in what:
        return "exact copy"
    for key, name in KINDS:
        if label == key or (key.startswith(".") and label.endswith(key)):
            return name
    if label.startswith("ref."):
        return "RefBlock conv (IN-GLU prologue)"
    if label.endswith(".conv"):
        return "block conv 3x3"
    return "Upsample" if label.startswith("ups.") else "Downsample"


def rows(path):
    case = None
    for line in open(path):
        line = line.rstrip("\n")
        if line.lstrip(".").startswith("==== "):
            case = line.lstrip(".")[5:].strip()
            continue
        m = ROW.match(line)
        if not m or case is None:
            continue
        prec = case.split("-")[1]
        what = (m.group("what") or "").strip()
        k = kind(m.group("label"), what, m.group("kernel"))
        vs = VSFMT.search(line)
        for part, f in zip(("scale", "shift"), FIG.findall(m.group("figs"))):
            e, own_name, own, bound = float(f[0]), f[1], float(f[2]), float(f[3])
            yield dict(case=case, prec=prec, label=m.group("label"), kernel=m.group("kernel"), shape=m.group("shape"), e=e, own=own, bound=bound,
                       kind=k + (" " + part if k.endswith("Norm") else ""), ratio=e / bound if bound else (0.0 if e == 0 else float("inf")),
                       vs=float(vs.group(1)) if vs else None, failed="FAILS" in line)


def table(title, head, groups, fmt):
    print("\n==== " + title)
    print(head)
    for key in sorted(groups):
        g = groups[key]
        print(fmt(key, g, max(g, key=lambda r: r["e"]), max(r["ratio"] for r in g)))


def main(path):
    allrows = list(rows(path))
    kinds, kernels, cases = collections.defaultdict(list), collections.defaultdict(list), collections.OrderedDict()
    for r in allrows:
        kinds[(r["kind"], r["prec"])].append(r)
        kernels[(r["kernel"], r["prec"])].append(r)
        cases.setdefault(r["case"], []).append(r)
    own = lambda g: max((r["e"] / r["own"] for r in g if r["own"] > 0), default=0.0)
    vs = lambda g: max((r["vs"] for r in g if r["vs"] is not None), default=None)
    table("worst figure per op kind and precision (rows = comparisons; e/bound = worst e_kernel / bound; max e/own = worst e_kernel / own error)",
          "%-34s %-11s %5s  %-9s  %-9s  %-7s  %s" % ("op kind", "precision", "rows", "worst e", "own error", "e/bound", "max e/own"), kinds,
          lambda k, g, w, q: "%-34s %-11s %5d  %.2e   %.2e   %.3f    %.2f" % (k[0], k[1], len(g), w["e"], w["own"], q, own(g)))
    table("worst row per kernel instance and precision (cases = estimator calls that launch it; e_vs_fmt: worst over its rows, bf16 contractions only)",
          "%-58s %-10s %4s %5s  %-8s  %-8s  %-8s %-7s %-8s  %s" % ("kernel instance", "precision", "rows", "cases", "worst e", "own err", "bound", "e/bound", "e_vs_fmt", "worst at"), kernels,
          lambda k, g, w, q: "%-58s %-10s %4d %5d  %.2e  %.2e  %.2e %.3f   %-8s  %s %s %s" % (
              k[0], k[1], len(g), len({r["case"] for r in g}), w["e"], w["own"], w["bound"], q,
              "-" if vs(g) is None else "%.2e" % vs(g), w["case"], w["label"], w["shape"]))
    print("\n==== per case: op rows, worst e_kernel / bound and where")
    for c, g in cases.items():
        w = max(g, key=lambda r: (r["ratio"], r["e"]))
        print("%-40s %3d ops  e/bound %.3f  %s  %s%s" % (c, len({r["label"] for r in g}), w["ratio"], w["label"], w["kernel"], "  FAILED" if any(r["failed"] for r in g) else ""))
    print("comparisons: %d in %d cases, %d kernel instances; failed: %d" % (len(allrows), len(cases), len({r["kernel"] for r in allrows if not r["kernel"].startswith("(")}), sum(r["failed"] for r in allrows)))


if __name__ == "__main__":
    main(sys.argv[1])
