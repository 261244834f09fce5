"""The cycles pass alone (csrc/recon_out.hip: recon_cycles_kernel; include/sgvae.h: sgv_test_recon_cycles): the load cycles and the
rates over time of val = (tanh(GroupNorm(y)) - min_n) / scale_n, never stored.  Inputs, canary-framed buffers and the stored field F --
what the output pass (sgv_test_recon_physical, layout [B][T][N]) writes for the same inputs -- come from tests/recon_kernel_common.py;
a quarter of the scales are negative.  From T = 5 on one row of y is copied onto the next, so that F has a bitwise plateau.

All four outputs are held to the numpy emulation on F (tests/cycles_reference.py) bit for bit, in both dtypes; path, range_sum and
damage also to float64 within their a-priori bounds (cycles_reference.ratios).  No other tolerance anywhere.

Shapes (B, T, C, ldy).  T = 1, 2, 3 (the first range), 5; T = 33: longer than the ring of loads in flight (4 steps in bf16, 2 in fp32).
C = 8: a single octet, one thread; C = 72: G = 8 groups of 9 channels, octets straddle groups; C = 504, 512, 520: one octet below, at
and past a wave's 512-channel share; C = 2040, 2048, 2056: the same around a block's 2048-channel share.  ldy = C and C + 24 with
canary padding columns; B = 1 and 3.

Gates (cycles_reference.kernel_gates, from F, per channel): 0; a quarter of the node's peak-to-peak; fl(|F[0, 1] - F[0, 0]|), the
strict tie at the first step of sample 0; twice the peak-to-peak.  Exponents 1, 3 and 8."""
import os
import sys

import numpy as np
import pytest

import simulgen_vae_amd  # noqa: F401
from simulgen_vae_amd import engine as E

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cycles_reference as CR  # noqa: E402
from recon_kernel_common import _bf16, base_inputs, bits, canary_buffers, device_inputs, field, hook_inputs, margins_intact, padding_intact  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = [(1, 1, 8, 8), (3, 2, 8, 32), (1, 3, 8, 8), (3, 3, 72, 96), (3, 5, 72, 72), (3, 33, 72, 96), (1, 5, 504, 504), (3, 33, 512, 536),
         (1, 2, 520, 520), (3, 1, 520, 544), (1, 33, 2040, 2040), (3, 5, 2048, 2072), (1, 1, 2056, 2056), (3, 33, 2056, 2080),
         (1, 3, 2056, 2056)]          # (B, T, C, ldy)
DTYPES = pytest.mark.parametrize("dtype", [0, 1], ids=["f32", "bf16"])
GATES = ("zero", "quarter", "first", "twice")
SGV_ERR_ARG = -1
UNWRITTEN = -999          # no count or step is below -1
NAMES = ("reversals", "ranges", "rate_when", "rates")
GROUPS = {"turns": ("reversals", "ranges"), "rates": ("rate_when", "rates")}

_CASES = {}


def case(B, T, Cn, ldy, dtype):
    """inputs, the stored field F and the four gates of one (shape, dtype), computed once and left alone"""
    import torch
    key = (B, T, Cn, ldy, dtype)
    if key not in _CASES:
        c = base_inputs(B, T, Cn, dtype)
        if dtype == 1:
            c["y"] = _bf16(torch, c["y"])
        if T >= 5:
            c["y"][:, 2] = c["y"][:, 1]          # a plateau: the same y, the same constants, the same bits
        c["F"] = field(c, c["y"], ldy, dtype)
        c["gates"] = CR.kernel_gates(c["F"])
        for v in c.values():
            v.setflags(write=False)
        if T >= 5:
            assert np.array_equal(bits(c["F"][:, 2]), bits(c["F"][:, 1]))
        _CASES[key] = c
    return _CASES[key]


def sizes(b, Cn):
    return {"gate": Cn, "reversals": b * Cn, "ranges": b * 4 * Cn, "rate_when": b * 2 * Cn, "rates": b * 3 * Cn}


def shaped(bufs, b, Cn):
    sh = {"reversals": (b, Cn), "ranges": (b, 4, Cn), "rate_when": (b, 2, Cn), "rates": (b, 3, Cn)}
    return {k: bufs[k][1].cpu().numpy().reshape(sh[k]) for k in NAMES}


def launch(c, y, gate, m, ldy, dtype, want=("turns", "rates")):
    """one call of the hook on the samples y [b, T, C] with gate [C] and exponent m -> dict of the outputs of the groups in `want`;
    the outputs start as -999 / NaN, so every element must have been written, and nothing around them or in an absent group"""
    import torch
    lib = E.load_library()
    b, T, Cn = y.shape
    g = np.array(gate, np.float32)          # a writable copy
    d = device_inputs(c, y, ldy, dtype)
    bufs = canary_buffers(sizes(b, Cn), integer=("reversals", "rate_when"))
    bufs["gate"][1].copy_(torch.from_numpy(g).cuda())
    for k in NAMES:
        bufs[k][1].fill_(UNWRITTEN if k in ("reversals", "rate_when") else float("nan"))
    asked = [k for grp in want for k in GROUPS[grp]]
    out = E.CyclesOut(**{k: bufs[k][1].data_ptr() for k in asked})
    import ctypes
    rc = lib.sgv_test_recon_cycles(dtype, *hook_inputs(d, ldy), bufs["gate"][1].data_ptr(), m, ctypes.byref(out), b, T, Cn, None)
    assert rc == 0, lib.sgv_last_error().decode()
    assert margins_intact(bufs), "a margin around a buffer was written"
    assert padding_intact(d, Cn), "the padding columns of y were written"
    assert np.array_equal(bits(bufs["gate"][1].cpu().numpy()), bits(g)), "the gate was written"
    res = shaped(bufs, b, Cn)
    for k in NAMES:
        blank = (res[k] == UNWRITTEN) if res[k].dtype == np.int32 else np.isnan(res[k])
        if k in asked:
            assert not blank.any(), f"an element of {k} was not written"
        else:
            assert blank.all(), f"{k} was written although it was not asked for"
    return {k: res[k] for k in asked}


def same(a, b):
    return a.keys() == b.keys() and all(np.array_equal(bits(a[k]), bits(b[k])) for k in a)


@DTYPES
@pytest.mark.parametrize("B,T,Cn,ldy", CASES)
def test_cycles_equal_the_emulation_on_the_stored_field(B, T, Cn, ldy, dtype):
    c = case(B, T, Cn, ldy, dtype)
    F = c["F"]
    tag = f"B {B} T {T} C {Cn} ldy {ldy} {'bf16' if dtype else 'f32'}"
    worst = {}
    first = None
    for gi, name in enumerate(GATES):
        gate = c["gates"][gi]
        for m in (1, 3, 8):
            got = launch(c, c["y"], gate, m, ldy, dtype)
            want = CR.emulate(F, gate, m)
            for k in NAMES:
                assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (name, m, k)
                assert np.array_equal(bits(got[k]), bits(want[k])), (name, m, k)
            for k, v in CR.ratios(got, F, gate, m).items():
                worst[k] = max(worst.get(k, 0.0), v)
            if first is None:
                first = got
                assert same(launch(c, c["y"], gate, m, ldy, dtype), got)          # two launches are bitwise equal
            if m == 3:
                rev, opn = got["reversals"], got["ranges"][:, 3]
                if name == "quarter" and T == 33:
                    assert (rev > 3).any(), "a quarter of the peak-to-peak leaves many reversals"
                if name == "first" and T >= 2:
                    # the stored steps 0 and 1 of sample 0 alone: nothing turns at t = 1 (and the kernel equals the emulation on all of F)
                    assert not CR.emulate(F[:1, :2], gate, m)["reversals"].any(), "a gate equal to the first difference does not trigger"
                    if T == 2:
                        assert not rev[0].any()
                if name == "twice":
                    assert not rev.any() and np.array_equal(bits(opn), bits((F.max(axis=1) - F.min(axis=1)).astype(np.float32)))
    print(f"  {tag}: worst err / bound " + ", ".join(f"{k} {v:.4f}" for k, v in sorted(worst.items())))
    assert all(v <= 1.0 for v in worst.values()), worst


@DTYPES
@pytest.mark.parametrize("B,T,Cn,ldy", [(3, 33, 72, 96), (3, 33, 512, 536), (1, 2, 520, 520), (3, 1, 520, 544), (3, 5, 2048, 2072), (1, 33, 2040, 2040)])
def test_each_group_alone_gives_the_bits_it_gives_with_the_other(B, T, Cn, ldy, dtype):
    c = case(B, T, Cn, ldy, dtype)
    gate = c["gates"][1]
    both = launch(c, c["y"], gate, 3, ldy, dtype)
    for grp, names in GROUPS.items():
        alone = launch(c, c["y"], gate, 3, ldy, dtype, want=(grp,))          # launch() checks that the other group's buffers stay blank
        assert tuple(alone) == names and same(alone, {k: both[k] for k in names}), grp


@DTYPES
@pytest.mark.parametrize("T,Cn,ldy", [(2, 8, 32), (3, 72, 96), (5, 72, 72), (33, 512, 536), (1, 520, 544), (5, 2048, 2072), (33, 2056, 2080)])
def test_a_sample_does_not_depend_on_its_batch(T, Cn, ldy, dtype):
    """each sample of B = 3 launched alone, and the last two together, give the bits they have in the batch"""
    c = case(3, T, Cn, ldy, dtype)
    gate = c["gates"][1]
    whole = launch(c, c["y"], gate, 3, ldy, dtype)
    for b in range(3):
        assert same(launch(c, c["y"][b:b + 1], gate, 3, ldy, dtype), {k: v[b:b + 1] for k, v in whole.items()}), b
    assert same(launch(c, c["y"][1:], gate, 3, ldy, dtype), {k: v[1:] for k, v in whole.items()})


@DTYPES
@pytest.mark.parametrize("B,T,Cn,ldy", [(3, 33, 72, 96), (3, 33, 512, 536), (3, 5, 2048, 2072)])
def test_the_exponent_changes_the_damage_alone(B, T, Cn, ldy, dtype):
    c = case(B, T, Cn, ldy, dtype)
    gate = c["gates"][0]
    base = launch(c, c["y"], gate, 1, ldy, dtype)
    assert np.array_equal(bits(base["ranges"][:, 0]), bits(base["ranges"][:, 2]))          # m = 1: the damage is the range sum
    for m in (2, 8):
        out = launch(c, c["y"], gate, m, ldy, dtype)
        for k in ("reversals", "rate_when", "rates"):
            assert np.array_equal(bits(out[k]), bits(base[k])), (m, k)
        assert np.array_equal(bits(out["ranges"][:, [0, 1, 3]]), bits(base["ranges"][:, [0, 1, 3]]))
        assert not np.array_equal(bits(out["ranges"][:, 2]), bits(base["ranges"][:, 2]))


def test_rejected_arguments_launch_nothing():
    import ctypes
    import torch
    lib = E.load_library()
    B, T, Cn, ldy = 3, 5, 72, 96
    c = case(B, T, Cn, ldy, 0)
    d = device_inputs(c, c["y"], ldy, 0)
    sz = sizes(B, Cn)
    sz["gate"] += 8
    bufs = canary_buffers(sz, integer=("reversals", "rate_when"))
    ptr = {k: bufs[k][1].data_ptr() for k in bufs}
    hook = list(hook_inputs(d, ldy))

    def rejected(msg, inputs=None, gate=ptr["gate"], m=3, Bn=B, Tn=T, C_=Cn, no_out=False, **outs):
        a = hook if inputs is None else inputs
        o = {k: ptr[k] for k in NAMES}
        o.update(outs)
        out = None if no_out else ctypes.byref(E.CyclesOut(**{k: v for k, v in o.items() if v is not None}))
        assert lib.sgv_test_recon_cycles(0, *a, gate, m, out, Bn, Tn, C_, None) == SGV_ERR_ARG, msg
        assert msg in lib.sgv_last_error().decode(), lib.sgv_last_error().decode()

    for i in (0, 2, 3, 4, 5, 6):          # y, sums, gamma, beta, scale, min
        rejected("null argument", inputs=hook[:i] + [None] + hook[i + 1:])
    rejected("null argument", gate=None)
    rejected("null argument", no_out=True)
    rejected("no group of the outputs is given", reversals=None, ranges=None, rate_when=None, rates=None)
    for k in NAMES:
        rejected("half a group", **{k: None})
    rejected("half a group", reversals=None, rates=None)
    rejected("exponent = 0 is outside [1, 8]", m=0)
    rejected("exponent = 9 is outside [1, 8]", m=9)
    rejected("exponent = -3 is outside [1, 8]", m=-3)
    rejected("T = 65536 is beyond the limit of 65535 time steps", Tn=65536)
    rejected("misaligned pointer", gate=ptr["gate"] + 2)
    for k in NAMES:
        rejected("misaligned pointer", **{k: ptr[k] + 4})
        rejected("misaligned pointer", **{k: ptr[k] + 8})
    rejected("misaligned pointer", inputs=[hook[0] + 4] + hook[1:])
    rejected("C % 8 == 0 required", C_=76)
    rejected("C % 8 == 0 required", C_=0)
    rejected("B, T >= 1", Bn=0)
    rejected("B, T >= 1", Tn=0)
    rejected("row stride", inputs=hook[:1] + [64] + hook[2:])
    rejected("row stride", inputs=hook[:1] + [ldy + 4] + hook[2:])
    out = ctypes.byref(E.CyclesOut(**{k: ptr[k] for k in NAMES}))
    assert lib.sgv_test_recon_cycles(2, *hook, ptr["gate"], 3, out, B, T, Cn, None) == SGV_ERR_ARG          # an unknown dtype
    torch.cuda.synchronize()
    assert all(bool((buf == buf[0]).all()) for buf, _ in bufs.values()), "a rejected call wrote something"
    assert torch.isnan(d["sums"]).all(), "a rejected call computed the statistics"
    assert padding_intact(d, Cn)
    # and the gate may sit at any 4-byte boundary
    gate = c["gates"][1]
    sub = bufs["gate"][1][1:1 + Cn]
    assert sub.data_ptr() % 16 == 4
    sub.copy_(torch.from_numpy(np.array(gate)).cuda())
    assert lib.sgv_test_recon_cycles(0, *hook, sub.data_ptr(), 3, out, B, T, Cn, None) == 0, lib.sgv_last_error().decode()
    assert same(shaped(bufs, B, Cn), launch(c, c["y"], gate, 3, ldy, 0))
    assert margins_intact(bufs)
