"""CPU: the catalogue of tests/test_gpu_conv1d.py (tests/conv1d_cases.py) reaches every compiled instance of the shared 1-D convolution
kernel and every epilogue branch -- Conv1dOp.instance is the launcher's own selection, host arithmetic -- its references can carry a
comparison, the bound tells restated kernel mistakes from the kernel, and the host-side refusals refuse before any device call."""
import ctypes

import pytest
import torch

import conv1d_cases as C


@pytest.fixture(scope="module")
def selected(sba):
    return {c.id: sba.Conv1dOp(**C.op_kwargs(c)).instance(c.B, c.Lin, res=c.res, accmode=c.accmode, out_mask=c.out_lens is not None)
            for c in C.CASES}


def test_case_ids_are_unique_and_shapes_small():
    ids = [c.id for c in C.CASES]
    assert len(set(ids)) == len(ids)
    for c in C.CASES:
        assert c.B in (2, 3) or (c.B == 4 and (c.in_lens or c.out_lens)), c.id       # B = 4 only to hold the four mask lengths
        assert c.Lin <= 600 and c.cin <= 64 and c.cout <= 160, c.id


def test_catalogue_selects_every_instance_and_epilogue(selected):
    inst = set(s[:4] for s in selected.values())
    epi = set(s[4] for s in selected.values())
    print("%d cases: instances %s, epilogues %s" % (len(C.CASES), sorted(inst), sorted(C.EPI_NAME[e] for e in epi)))
    assert len(C.INSTANCES) == 9
    missing = [i for i in C.INSTANCES if i not in inst]
    assert not missing, "no case of tests/conv1d_cases.py selects (MT, TPS, AITER, KCH) = %s" % missing
    assert inst == set(C.INSTANCES)                          # and nothing the list does not know
    assert epi == {C.EPI_BUFFER, C.EPI_UP16, C.EPI_UP8, C.EPI_GENERIC}
    # every instance with whole row tiles and with its last row tile partial where the tile allows both at <= 160 rows
    for mt in (32, 64, 128):
        epis = set(s[4] for s in selected.values() if s[0] == mt)
        assert {C.EPI_BUFFER, C.EPI_GENERIC} <= epis, (mt, epis)


def test_named_cases_select_what_their_name_says(selected):
    for cid, (inst, epi) in C.EXPECT.items():
        assert selected[cid] == inst + (epi,), (cid, selected[cid])
    # both sides of each switch
    assert selected["switch-kch2-dil32"][3] == 2 and selected["switch-kch1-dil33"][3] == 1
    assert selected["inst-128-t3-a3-dil65"][2] == 3 and selected["switch-kch1-dil33"][2] == 2


def test_catalogue_keeps_its_edges():
    have = set((c.cout, c.Lin) for c in C.CASES if c.mode == 0 and c.K == 3 and c.dil == 1)
    for Lin in (1, 127, 128, 129, 259):
        assert (128, Lin) in have
    for Lin in (1, 255, 256, 257, 515):
        assert (32, Lin) in have
    for cout in (1, 4, 8, 31, 32, 33, 64, 96, 128, 160):
        assert (cout, 70) in have
    assert set(c.K for c in C.CASES if c.mode == 0) >= {1, 3, 5, 7, 11}
    assert set(c.S for c in C.CASES) == {1, 2, 4, 8}
    assert set(c.slope for c in C.CASES) == {1.0, 0.1, 0.0}
    assert set(c.cin % 16 for c in C.CASES) >= {0, 4, 8}
    assert any(c.K == 11 and c.dil == 5 and c.Lin == 3 for c in C.CASES) and any(c.K == 11 and c.dil == 5 and c.Lin == 7 for c in C.CASES)
    for lens in ("in_lens", "out_lens"):
        assert any(getattr(c, lens) and min(getattr(c, lens)) == 0 and 1 in getattr(c, lens) for c in C.CASES)
    assert set(c.accmode for c in C.CASES) == {0, 1, 2} and any(c.res and not c.accmode for c in C.CASES)


@pytest.fixture(scope="module")
def refs():
    out = {}
    for c in C.CASES:
        d = C.make_inputs(c)
        out[c.id] = (d, C.reference(c, d))
    return out


def test_references_are_finite_and_above_the_bias(refs):
    for c in C.CASES:
        ref = refs[c.id][1]
        assert bool(torch.isfinite(ref).all()) and float(ref.abs().max()) > 0.1, c.id
        assert ref.shape == (c.B, c.cout, c.Lin * c.S)


def test_bound_tells_restated_kernel_mistakes_from_the_kernel(refs):
    """What the GPU test's bound REL = 1e-4 would say to three mistakes, restated in float64 on the CPU:
      * the wl * xh MFMA dropped: the weights lose their low bf16 half, the layer is computed with bf16-rounded weights;
      * one tap offset shifted by one: the last tap reads one position late;
      * the residual add dropped.
    Each must exceed the bound on every case it can touch (so every such case of the GPU test turns red), while the float32 torch
    restatement of the true layer stays two orders below it."""
    n_shift = n_res = 0
    for c in C.CASES:
        d, ref = refs[c.id]
        e32 = C.relerr(C.reference(c, d, torch.float32), ref)
        assert e32 < 1e-6, (c.id, e32)
        e_lo = C.relerr(C.reference(c, d, w=C.bf16_round(d["w"])), ref)
        assert e_lo > C.REL, (c.id, e_lo)
        if c.mode == 0 and c.Lin > (c.K - 1) // 2 * c.dil + 1 and (c.in_lens is None or max(c.in_lens) == c.Lin):
            n_shift += 1
            assert C.relerr(C.reference(c, d, toff_shift=1), ref) > C.REL, c.id
        if c.res:
            n_res += 1
            assert C.relerr(C.reference(c, d, drop_res=True), ref) > C.REL, c.id
    assert n_shift >= 50 and n_res >= 8


# ---------------------------------------------------------------------------------------------- refusals (host side, no device call)
def test_create_refuses_what_no_instance_holds(sba):
    with pytest.raises(RuntimeError, match="halo"):
        sba.Conv1dOp(0, 16, 128, 3, dilation=129)            # halo 258 on the 128-row tile (limit 256)
    sba.Conv1dOp(0, 16, 128, 3, dilation=128)
    with pytest.raises(RuntimeError, match="halo"):
        sba.Conv1dOp(0, 16, 64, 3, dilation=65)              # halo 130 on the 64-row tile (limit 128)
    with pytest.raises(RuntimeError, match="halo"):
        sba.Conv1dOp(0, 16, 32, 11, dilation=13)             # 130 on the 32-row tile
    with pytest.raises(RuntimeError, match="taps"):
        sba.Conv1dOp(0, 16, 32, 13)                          # K > C1_MAXTAP = 12
    with pytest.raises(RuntimeError, match="power of two"):
        sba.Conv1dOp(1, 16, 16, 6, S=3)
    with pytest.raises(RuntimeError, match="odd kernel"):
        sba.Conv1dOp(0, 16, 32, 4)
    with pytest.raises(RuntimeError, match="2 \\* stride"):
        sba.Conv1dOp(1, 16, 16, 6, S=2)


def test_forward_refuses_a_sample_of_2_gib_before_any_launch(sba):
    """cout * Lout * 4 and the padded cin * Lin * 4 are 32-bit byte counts in the kernel: 2^31 bytes is refused with GTTS_E_SHAPE on the
    host.  The pointers are never read (there is no device here), so any non-null value stands for them."""
    L = sba._lib.lib()
    fake = ctypes.c_void_p(4096)

    def forward(op, B, Lin):
        return L.gtts_conv1d_forward(op._h, fake, fake, fake, fake, None, None, 0, 1.0, 1.0, None, None, B, Lin, None)
    out_big = sba.Conv1dOp(0, 16, 128, 3)
    assert out_big.instance(1, (1 << 22) - 1)[0] == 128                   # one position below: accepted (the query runs the same checks)
    assert forward(out_big, 1, 1 << 22) == -2                             # 128 * 2^22 * 4 = 2^31 bytes of output per sample
    assert b"2^31" in L.gtts_last_error()
    with pytest.raises(RuntimeError, match="2\\^31"):
        out_big.instance(1, 1 << 22)
    in_big = sba.Conv1dOp(0, 64, 8, 3)
    assert forward(in_big, 3, 1 << 23) == -2                              # 64 * 2^23 * 4 bytes of input per sample
    up = sba.Conv1dOp(1, 16, 16, 16, S=8)
    assert forward(up, 1, 1 << 22) == -2                                  # 16 * (8 * 2^22) * 4
    pad = sba.Conv1dOp(0, 4, 4, 3)
    assert forward(pad, 1, 1 << 25) == -2                                 # the staged chunk spans 16 channels: 16 * 2^25 * 4
    assert pad.instance(1, (1 << 25) - 1)[0] == 32


def test_conv1d_op_accepts_partial_chunks(sba):
    """cin % 16 != 0 is accepted (the pad channels of the last chunk are staged as zeros: tests/test_gpu_conv1d.py runs such layers
    between NaN margins); the packed size counts whole 16-channel chunks."""
    assert sba.Conv1dOp(0, 4, 4, 3).packed_bytes() == sba.Conv1dOp(0, 16, 4, 3).packed_bytes()
    assert sba.Conv1dOp(0, 20, 32, 7).instance(2, 70) == (32, 4, 3, 1, C.EPI_BUFFER)
    with pytest.raises(RuntimeError, match="HIP device"):
        sba.Conv1dOp(0, 4, 4, 3).forward(None, torch.zeros(4), torch.zeros(1, 4, 8))


def test_vocoder_refuses_a_layer_of_2_gib_before_its_first_launch(sba):
    """V1 at B = 1, T = 65536: ups.1 writes 128 channels x 2^22 samples = 2^31 bytes per sample.  gtts_voc_forward checks every layer of
    the call before the first launch (and before any other HIP call), so the refusal can be seen without a device."""
    L = sba._lib.lib()
    voc = sba.Vocoder()
    fake = ctypes.c_void_p(4096)
    nbytes = voc.workspace_bytes(1, 65536)
    assert L.gtts_voc_forward(voc._h, fake, fake, fake, fake, nbytes, 1, 65536, None) == -2
    msg = L.gtts_last_error()
    assert b"ups.1" in msg and b"2^31" in msg, msg
    # the earlier guard let this through: cout * Lout = 2^29 elements < 2^31
    assert 128 * 65536 * 64 == 1 << 29
