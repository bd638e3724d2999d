"""Which code paths of the weight-gradient kernels (csrc/train_wgrad.hip, csrc/train_wgrad7.hip) a shape reaches, read back from the
library instead of restated: `gtts_conv{3x3,1x1,7x7}_wgrad_workspace_bytes` returns (nslice * tiles * taps * 4096 + nslice * cout) * 4,
so nslice follows from the byte count; the chunk count is the kernels' documented tiling of the pixels (3x3: 2 rows x 32 columns,
1x1: 64 consecutive pixels of one sample's plane, 7x7: one row x 64 columns).  From the two:

  per          chunks per workgroup = ceil(nchunk / nslice): how often the staging loop (3x3: the double buffer) cycles
  empty        trailing slices with slice * per >= nchunk: workgroups that skip the loop and must still publish zeros
  groups       slices per slice-group of wgrad_reduce_kernel (8 groups of ceil(nslice / 8), the last ones shorter or empty)
  unrolled     some group holds >= 8 slices: the eight-loads-in-flight loop runs
  remainder    some group runs the unrolled loop AND the scalar loop after it (length >= 8, not a multiple of 8)

Shared by tests/test_train_abi_cpu.py (the formula) and tests/test_gpu_training_shapes.py (the regimes of its cases)."""

TAPS = {"3x3": 9, "1x1": 1, "7x7": 49}


def nchunk(kind, B, H, W):
    if kind == "3x3":
        return B * ((H + 1) // 2) * ((W + 31) // 32)
    if kind == "1x1":
        return B * ((H * W + 63) // 64)
    if kind == "7x7":
        return B * H * ((W + 63) // 64)
    raise KeyError(kind)


def workspace_bytes(L, kind, B, cin, cout, H, W):
    fn = {"3x3": L.gtts_conv3x3_wgrad_workspace_bytes, "1x1": L.gtts_conv1x1_wgrad_workspace_bytes,
          "7x7": L.gtts_conv7x7_wgrad_workspace_bytes}[kind]
    return int(fn(B, cin, cout, H, W))


def nslice_of(L, kind, B, cin, cout, H, W):
    """nslice the library chose for this call, from the workspace size (asserts the size has the documented form)."""
    nws = workspace_bytes(L, kind, B, cin, cout, H, W)
    tiles = (cin // 64) * (cout // 64)
    per_slice = (tiles * TAPS[kind] * 4096 + cout) * 4
    assert nws > 0 and nws % per_slice == 0, (kind, B, cin, cout, H, W, nws, per_slice)
    return nws // per_slice


def regime(L, kind, B, cin, cout, H, W):
    ns = nslice_of(L, kind, B, cin, cout, H, W)
    nc = nchunk(kind, B, H, W)
    assert 1 <= ns <= (nc + 3) // 4, (kind, ns, nc)
    per = (nc + ns - 1) // ns
    empty = sum(1 for s in range(ns) if s * per >= nc)
    gper = (ns + 7) // 8
    groups = [max(0, min(ns, (g + 1) * gper) - g * gper) for g in range(8)]
    assert sum(groups) == ns
    return {"nslice": ns, "nchunk": nc, "per": per, "empty": empty, "groups": groups,
            "unrolled": any(n >= 8 for n in groups), "all_unrolled": ns >= 64 and all(n >= 8 for n in groups if n),
            "remainder": any(n >= 8 and n % 8 for n in groups)}


def describe(r):
    return "nslice %d, %d chunks -> %d per workgroup, %d empty slices, reduce groups %s" % (
        r["nslice"], r["nchunk"], r["per"], r["empty"], r["groups"])
