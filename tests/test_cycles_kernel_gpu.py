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
import recon_kernel_common as H  # noqa: E402
from recon_kernel_common import DTYPES, bits, same  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = [(1, 1, 8, 8), (3, 2, 8, 32), (1, 3, 8, 8), (3, 3, 72, 96), (3, 5, 72, 72), (3, 33, 72, 96), (1, 5, 504, 504), (3, 33, 512, 536),
         (1, 2, 520, 520), (3, 1, 520, 544), (1, 33, 2040, 2040), (3, 5, 2048, 2072), (1, 1, 2056, 2056), (3, 33, 2056, 2080),
         (1, 3, 2056, 2056)]          # (B, T, C, ldy)
GATES = ("zero", "quarter", "first", "twice")
NAMES = ("reversals", "ranges", "rate_when", "rates")
GROUPS = {"turns": ("reversals", "ranges"), "rates": ("rate_when", "rates")}
PASS = H.Pass("cycles", lambda b, T, Cn, m: {"gate": (Cn,), "reversals": (b, Cn), "ranges": (b, 4, Cn), "rate_when": (b, 2, Cn), "rates": (b, 3, Cn)},
              NAMES, lambda a: (a["gate"], a["m"], H.struct(E.CyclesOut, a, NAMES)), integer=("reversals", "rate_when"))


def plateau(c):
    if c["y"].shape[1] >= 5:
        c["y"][:, 2] = c["y"][:, 1]          # the same y, the same constants, the same bits


def case(B, T, Cn, ldy, dtype):
    """inputs, the stored field F and the four gates of one (shape, dtype), computed once and left alone"""
    c = H.case(__name__, B, T, Cn, ldy, dtype, edit=plateau, extras=lambda c: {"gates": CR.kernel_gates(c["F"])})
    assert T < 5 or np.array_equal(bits(c["F"][:, 2]), bits(c["F"][:, 1]))
    return c


def launch(c, y, gate, m, ldy, dtype, want=("turns", "rates")):
    """one call of the hook on the samples y [b, T, C] with gate [C] and exponent m -> dict of the outputs of the groups in `want`"""
    asked = [k for grp in want for k in GROUPS[grp]]
    res = H.launch(PASS, c, y, ldy, dtype, {"gate": gate}, want=asked, m=m)
    return {k: res[k] for k in asked}


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
                assert not same(launch(c, c["y"], gate, m, ldy, dtype), got)          # two launches are bitwise equal
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
        assert tuple(alone) == names and not same(alone, {k: both[k] for k in names}), grp


@DTYPES
@pytest.mark.parametrize("T,Cn,ldy", [(2, 8, 32), (3, 72, 96), (5, 72, 72), (33, 512, 536), (1, 520, 544), (5, 2048, 2072), (33, 2056, 2080)])
def test_a_sample_does_not_depend_on_its_batch(T, Cn, ldy, dtype):
    """each sample of B = 3 launched alone, and the last two together, give the bits they have in the batch"""
    c = case(3, T, Cn, ldy, dtype)
    gate = c["gates"][1]
    H.assert_batch_independent(lambda y: launch(c, y, gate, 3, ldy, dtype), c["y"])


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
    import torch
    B, T, Cn, ldy = 3, 5, 72, 96
    c = case(B, T, Cn, ldy, 0)
    d = H.device_inputs(c, c["y"], ldy, 0)
    bufs = H.canary_buffers(dict(H.sizes(PASS, B, T, Cn, m=3), gate=Cn + 8), integer=PASS.integer)
    gate = c["gates"][1]
    sub = bufs["gate"][1][1:1 + Cn]          # the gate may sit at any 4-byte boundary: the good call has it there
    assert sub.data_ptr() % 16 == 4
    sub.copy_(torch.from_numpy(np.array(gate)).cuda())
    good = dict(H.hook_args(d, bufs, ldy, 0, B, T, Cn, m=3), gate=sub.data_ptr())
    bad = H.common_rejections(good)
    bad += [(dict(gate=None), "null argument"), (dict(no_struct=True), "null argument"), ({k: None for k in NAMES}, "no group of the outputs is given")]
    bad += [({k: None}, "half a group") for k in NAMES] + [(dict(reversals=None, rates=None), "half a group")]
    bad += [(dict(m=v), f"exponent = {v} is outside [1, 8]") for v in (0, 9, -3)]
    bad += [(dict(T=65536), "T = 65536 is beyond the limit of 65535 time steps"), (dict(gate=good["gate"] + 2), "misaligned pointer")]
    bad += [({k: good[k] + step}, "misaligned pointer") for k in NAMES for step in (4, 8)]
    H.reject_all(PASS, d, bufs, good, bad)
    assert not same(H.outputs_of(PASS, bufs, B, T, Cn, m=3), launch(c, c["y"], gate, 3, ldy, 0))
    assert H.margins_intact(bufs)
