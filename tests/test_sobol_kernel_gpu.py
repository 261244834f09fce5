"""The Sobol pass alone (csrc/recon_out.hip: recon_sobol_kernel; include/sgvae.h: sgv_test_recon_sobol): a launch holds nb blocks of
d + 2 members, A_j, B_j, AB_1_j .. AB_d_j; the values val[b, t, n] = (tanh(GroupNorm(y)) - min_n) / scale_n of the members are
combined per (t, n) into Welford mean / M2 over the A and B members and, per parameter i, the running sums of (xB - xAB_i)^2 and
(xA - xAB_i)^2 -- and never stored.  Inputs as tests/test_ensemble_kernel_gpu.py builds them (tests/recon_kernel_common.py); a quarter
of the scales are negative.

Bit for bit: the reference field F is what the existing output pass (sgv_test_recon_physical, layout [B][T][N]) stores for the same
inputs, and every output must equal tests/sobol_reference.py, the numpy float32 emulation of the kernel's arithmetic, run on F.
Against float64 on F: sobol_reference.sumsq_bound (nb terms) and welford_bound (2 nb values), no constant added; worst err / bound
seen on an MI355X stands in DESIGN.md section 20.

Shapes (nb, d, T, C, ldy): the smallest case; C = 40 has groups of 5 channels, so a thread's 8 channels lie in three groups (the
general path of the group table); (2, 3, 33, 72, 80) has padding columns, which hold a canary and must come back unchanged, and 33
rows leave row lanes ragged; d = 14 is a full batch of 16 in one block; 2080 channels are five column blocks, the last partly
filled; 5 blocks of 8 are 40 members, more than a launch holds, so the launcher cuts at a block boundary (the fp32 kernel
takes three blocks per launch, so it cuts the four blocks of (4, 2, 9, ..) too); d = 30 fills the member table."""
import os
import sys

import numpy as np
import pytest

import simulgen_vae_amd  # noqa: F401
from simulgen_vae_amd import engine as E

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sobol_reference as SR  # noqa: E402
import recon_kernel_common as H  # noqa: E402
from recon_kernel_common import DTYPES, bits  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1, 8, 8), (3, 2, 5, 40, 40), (2, 3, 33, 72, 80), (1, 14, 3, 72, 72), (4, 2, 9, 2080, 2080), (5, 6, 2, 72, 72),
          (1, 30, 2, 72, 72)]     # (nb, d, T, C, ldy)
BOTH = ("first", "total")
ARRAY = {"first": "first_sq", "total": "total_sq"}
SHAPE = pytest.mark.parametrize("nb,d,T,Cn,ldy", SHAPES)
PASS = H.Pass("sobol", lambda b, T, Cn, d, blocks_before: {"mean": (T, Cn), "m2": (T, Cn), "first_sq": (d, T, Cn), "total_sq": (d, T, Cn)}, SR.STATE,
              lambda a: (a["d"], a["blocks_before"], H.struct(E.SobolState, a, SR.STATE)))

_RUNS = {}


def case(nb, d, T, Cn, ldy, dtype):
    """inputs, the stored field F and the emulation's state of one (shape, dtype), computed once and left alone"""
    c = H.case((__name__, d), nb * (d + 2), T, Cn, ldy, dtype, extras=lambda c: {"want": SR.update(c["F"], d)})
    assert np.isfinite(c["F"]).all()
    return c


def launch(c, y, ldy, dtype, d, parts=BOTH, blocks_before=0, state=None):
    """one call of the hook on the members y [nb (d + 2), T, C] -> the state as a dict of numpy arrays.  state: the state to continue
    from (blocks_before > 0); else every array holds NaN first, which a launch from empty must not read.  The array of a part not
    asked for comes back as it was filled, and is checked not to have been written."""
    return H.launch(PASS, c, y, ldy, dtype, want=["mean", "m2"] + [ARRAY[p] for p in parts], state=state, d=d, blocks_before=blocks_before)


def same(a, b, names=SR.STATE):
    return H.same(a, b, names)


def run_once(nb, d, T, Cn, ldy, dtype):
    """the single launch from empty with both parts"""
    key = (nb, d, T, Cn, ldy, dtype)
    if key not in _RUNS:
        c = case(*key)
        _RUNS[key] = launch(c, c["y"], ldy, dtype, d)
    return _RUNS[key]


@DTYPES
@SHAPE
def test_from_empty_equals_the_emulation_on_the_stored_field(nb, d, T, Cn, ldy, dtype):
    c = case(nb, d, T, Cn, ldy, dtype)
    got = run_once(nb, d, T, Cn, ldy, dtype)          # the state was NaN before: a launch from empty does not read it
    bad = same(got, c["want"])
    for k in bad:
        i = np.flatnonzero(bits(got[k]).reshape(-1) != bits(c["want"][k]).reshape(-1))
        print(k, len(i), "mismatches, first:", got[k].reshape(-1)[i[:4]], c["want"][k].reshape(-1)[i[:4]])
    assert not bad, bad
    F = c["F"].reshape(nb, d + 2, T, Cn)
    if nb == 1:
        assert np.array_equal(bits(got["first_sq"]), bits(np.square(F[0, 1] - F[0, 2:]))) and np.array_equal(bits(got["total_sq"]), bits(np.square(F[0, 0] - F[0, 2:])))
    assert (got["first_sq"] >= 0).all() and (got["total_sq"] >= 0).all() and got["first_sq"].any() and got["total_sq"].any()


@DTYPES
@SHAPE
def test_within_the_a_priori_bounds_of_float64_on_the_stored_field(nb, d, T, Cn, ldy, dtype):
    c = case(nb, d, T, Cn, ldy, dtype)
    got, ref = run_once(nb, d, T, Cn, ldy, dtype), SR.exact(c["F"], d)
    with np.errstate(invalid="ignore", divide="ignore"):
        r_sq = max(np.nanmax(np.abs(got[k].astype(np.float64) - ref[k]) / SR.sumsq_bound(nb, ref[k])) for k in ("first_sq", "total_sq"))
        r_m2 = np.nanmax(np.abs(got["m2"].astype(np.float64) - ref["m2"]) / SR.welford_bound(2 * nb, ref["mean"], ref["m2"]))
    print(f"nb {nb} d {d} T {T} C {Cn} dtype {dtype}: worst err / bound  sums of squares {r_sq:.3f}  m2 {r_m2:.3f}")
    for k in ("m2", "first_sq", "total_sq"):          # where the exact sum is 0 (identical values) the kernel's is 0 too
        assert not got[k][ref[k] == 0].any()
    assert r_sq <= 1.0 and r_m2 <= 1.0


SPLITS = [((3, 2, 5, 40, 40), (1, 1, 1)), ((2, 3, 33, 72, 80), (1, 1)), ((4, 2, 9, 2080, 2080), (3, 1)), ((5, 6, 2, 72, 72), (1, 4)), ((5, 6, 2, 72, 72), (2, 3))]


@DTYPES
@pytest.mark.parametrize("shape,parts", SPLITS, ids=[f"{s[0]}x{s[1] + 2}={'+'.join(map(str, p))}" for s, p in SPLITS])
def test_any_split_of_the_blocks_gives_the_bits_of_one_launch(shape, parts, dtype):
    nb, d, T, Cn, ldy = shape
    assert sum(parts) == nb
    c = case(nb, d, T, Cn, ldy, dtype)
    state, lo = None, 0
    for n in parts:
        state = launch(c, c["y"][lo * (d + 2):(lo + n) * (d + 2)], ldy, dtype, d, blocks_before=lo, state=state)
        lo += n
    assert not same(state, run_once(nb, d, T, Cn, ldy, dtype))


@DTYPES
@SHAPE
def test_each_part_alone_gives_the_bits_of_the_full_call(nb, d, T, Cn, ldy, dtype):
    c = case(nb, d, T, Cn, ldy, dtype)
    full = run_once(nb, d, T, Cn, ldy, dtype)
    h = nb // 2          # the continuing launch (it reads the state) as well, where there are blocks for two
    for part in BOTH:
        names, other = ("mean", "m2", ARRAY[part]), ARRAY[BOTH[1 - BOTH.index(part)]]
        got = launch(c, c["y"], ldy, dtype, d, parts=(part,))
        assert not same(got, full, names), (part, same(got, full, names))
        assert np.isnan(got[other]).all()          # launch() has checked that it was not written; it still holds the fill
        if h:
            first = launch(c, c["y"][:h * (d + 2)], ldy, dtype, d, parts=(part,))
            rest = {k: (first[k] if k in names else full[k]) for k in SR.STATE}
            got = launch(c, c["y"][h * (d + 2):], ldy, dtype, d, parts=(part,), blocks_before=h, state=rest)
            assert not same(got, full), (part, same(got, full))      # the array not asked for was handed in complete and left alone


@DTYPES
@pytest.mark.parametrize("nb,d,T,Cn,ldy", [(3, 2, 5, 40, 40), (2, 3, 33, 72, 80), (4, 2, 9, 2080, 2080)])
def test_a_parameter_that_changes_nothing_or_everything_gives_exact_zeros(nb, d, T, Cn, ldy, dtype):
    c = dict(case(nb, d, T, Cn, ldy, dtype))
    y = np.array(c["y"]).reshape(nb, d + 2, T, Cn)
    y[:, 2] = y[:, 0]                             # AB_1 == A: identical rows and identical statistics, so identical values
    y[:, 2 + d - 1] = y[:, 1]                     # AB_d == B
    y = y.reshape(nb * (d + 2), T, Cn)
    got = launch(c, y, ldy, dtype, d)
    assert not got["total_sq"][0].any() and not got["first_sq"][d - 1].any()
    assert got["first_sq"][0].any() and got["total_sq"][d - 1].any()
    assert np.array_equal(bits(got["first_sq"][0]), bits(got["total_sq"][d - 1]))          # both sum (xA - xB)^2 in the same order
    assert not same(got, SR.update(H.field(c, y, ldy, dtype), d))


@DTYPES
@SHAPE
def test_two_launches_are_bitwise_equal(nb, d, T, Cn, ldy, dtype):
    c = case(nb, d, T, Cn, ldy, dtype)
    assert not same(launch(c, c["y"], ldy, dtype, d), run_once(nb, d, T, Cn, ldy, dtype))


def test_the_largest_count_is_accepted():
    nb, d, T, Cn, ldy, dtype = 3, 2, 5, 40, 40, 0
    c = case(nb, d, T, Cn, ldy, dtype)
    base = (1 << 23) - nb
    state = SR.empty_state(d, T, Cn)
    got = launch(c, c["y"], ldy, dtype, d, blocks_before=base, state=state)
    assert not same(got, SR.update(c["F"], d, state, base))


def test_rejected_arguments_write_nothing():
    nb, d, T, Cn, ldy, dtype = 3, 2, 5, 40, 40, 0
    B = nb * (d + 2)
    c = case(nb, d, T, Cn, ldy, dtype)
    dev = H.device_inputs(c, c["y"], ldy, dtype)
    bufs = H.canary_buffers(H.sizes(PASS, B, T, Cn, d=d, blocks_before=0))
    for _, v in bufs.values():
        v.fill_(float("nan"))
    good = H.hook_args(dev, bufs, ldy, dtype, B, T, Cn, d=d, blocks_before=0)
    bad = H.common_rejections(good) + [(dict(no_struct=True), "null argument")]
    bad += [(dict(mean=None), "mean and m2 are required"), (dict(m2=None), "mean and m2 are required"), (dict(first_sq=None, total_sq=None), "neither first_sq nor total_sq")]
    bad += [({k: good[k] + 4}, "misaligned pointer") for k in bufs]
    bad += [(dict(d=0), "n_params = 0 is outside [1, 30]"), (dict(d=-1), "outside [1, 30]"), (dict(d=31), "n_params = 31 is outside [1, 30]")]
    bad += [(dict(d=3), "not a positive multiple of n_params + 2 = 5"), (dict(B=B - 1), "not a positive multiple of n_params + 2 = 4"), (dict(d=B), "not a positive multiple")]
    bad += [(dict(blocks_before=v), "outside [0, 2^24]") for v in (-1, (1 << 23) - nb + 1, 1 << 40)]
    H.reject_all(PASS, dev, bufs, good, bad)
    assert not same(H.outputs_of(PASS, bufs, B, T, Cn, d=d, blocks_before=0), run_once(nb, d, T, Cn, ldy, dtype))
