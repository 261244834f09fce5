"""The ensemble pass alone (csrc/recon_out.hip: recon_ensemble_kernel; include/sgvae.h: sgv_test_recon_ensemble): the values
val[b, t, n] = (tanh(GroupNorm(y)) - min_n) / scale_n  of the members b of a launch are merged, member after member, into a running
state per (t, n) -- Welford mean / M2, max / min with the member's index, the count above a limit -- and never stored.  Inputs as
tests/test_summary_kernel_gpu.py builds them; a quarter of the scales are negative.

Everything here is bit for bit.  The reference field F is what the existing output pass (sgv_test_recon_physical, layout
[B][T][N]) stores for the same inputs: max / min / argmax / argmin / (F > limit).sum over axis 0 in numpy, and mean / M2 from
tests/ensemble_reference.py, the numpy float32 emulation of the kernel's arithmetic, run on F.  The limit of a case is the
per-node median of F, so that counts are neither 0 nor B everywhere.

Shapes (B, T, C, ldy): the smallest case; C = 40 has groups of 5 channels, so a thread's 8 channels lie in up to three groups (the
general path of the group table); (2, 33, 72, 80) has padding columns, which hold a canary and must come back unchanged, and 33
rows leave row lanes ragged; 16 members are a full batch (four rounds of loads); 2080 channels are five column blocks, the last
partly filled; 40 members are more than the block's table holds (32), so the launcher cuts the batch."""
import itertools
import os
import sys

import numpy as np
import pytest

import simulgen_vae_amd  # noqa: F401
from simulgen_vae_amd import engine as E

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ensemble_reference as ER  # noqa: E402
import recon_kernel_common as H  # noqa: E402
from recon_kernel_common import DTYPES, bits  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 8, 8), (3, 5, 40, 40), (2, 33, 72, 80), (16, 3, 72, 72), (4, 9, 2080, 2080)]     # (B, T, C, ldy)
GROUPS = {"moments": ("mean", "m2"), "extrema": ("max", "min", "arg_max", "arg_min"), "exceed": ("limit", "exceed")}
ALL = tuple(GROUPS)
STATE = ER.STATE                                   # the seven arrays the kernel writes
INT = ("arg_max", "arg_min", "exceed")
PASS = H.Pass("ensemble", lambda b, T, Cn, count_before: dict({k: (T, Cn) for k in STATE}, limit=(Cn,)), STATE,
              lambda a: (a["count_before"], H.struct(E.EnsembleState, a, STATE + ("limit",))), integer=INT)


def case(B, T, Cn, ldy, dtype):
    """inputs, the stored field F, the limit and the emulation's state of one (shape, dtype), computed once and left alone"""
    def extras(c):
        limit = np.median(c["F"].reshape(B * T, Cn), axis=0).astype(np.float32)
        return {"limit": limit, "want": ER.update(c["F"], limit=limit)}
    c = H.case(__name__, B, T, Cn, ldy, dtype, extras=extras)
    assert (c["scale"] < 0).any() or Cn == 8
    return c


def launch(c, y, ldy, dtype, groups=ALL, count_before=0, state=None, limit=None):
    """one call of the hook on the members y [b, T, C] -> the state as a dict of numpy arrays [T, C] (the arrays of groups not
    asked for come back as they were filled).  state: the state to continue from (count_before > 0), else every array holds
    NaN / UNWRITTEN first."""
    limit = (c["limit"] if limit is None else limit) if "exceed" in groups else None
    asked = [k for g in groups for k in GROUPS[g] if k != "limit"]
    return H.launch(PASS, c, y, ldy, dtype, {"limit": limit}, want=asked, state=state, count_before=count_before)


def same(a, b, names=STATE):
    return H.same(a, b, names)


_RUNS = {}


def run_once(B, T, Cn, ldy, dtype):
    """the single launch from empty with all groups"""
    key = (B, T, Cn, ldy, dtype)
    if key not in _RUNS:
        c = case(*key)
        _RUNS[key] = launch(c, c["y"], ldy, dtype)
    return _RUNS[key]


@DTYPES
@pytest.mark.parametrize("B,T,Cn,ldy", SHAPES + [(40, 2, 72, 72)])
def test_from_empty_equals_reductions_of_the_stored_field(B, T, Cn, ldy, dtype):
    c = case(B, T, Cn, ldy, dtype)
    got, F = run_once(B, T, Cn, ldy, dtype), c["F"]
    assert np.isfinite(F).all()
    assert np.array_equal(bits(got["max"]), bits(F.max(0))) and np.array_equal(bits(got["min"]), bits(F.min(0)))
    assert np.array_equal(got["arg_max"], np.argmax(F, 0)) and np.array_equal(got["arg_min"], np.argmin(F, 0))
    assert np.array_equal(got["exceed"], (F > c["limit"]).sum(0))
    assert 0 < got["exceed"].sum() < B * T * Cn or B == 1
    bad = same(got, c["want"])
    for k in bad:
        i = np.flatnonzero(bits(got[k]).reshape(-1) != bits(c["want"][k]).reshape(-1))
        print(k, len(i), "mismatches, first:", got[k].reshape(-1)[i[:4]], c["want"][k].reshape(-1)[i[:4]])
    assert not bad, bad
    if B == 1:
        assert np.array_equal(bits(got["mean"]), bits(F[0])) and not got["m2"].any()


SPLITS = [((16, 3, 72, 72), (5, 11)), ((3, 5, 40, 40), (1, 1, 1)), ((4, 9, 2080, 2080), (3, 1)), ((40, 2, 72, 72), (33, 7))]


@DTYPES
@pytest.mark.parametrize("shape,parts", SPLITS, ids=[f"{s[0]}={'+'.join(map(str, p))}" for s, p in SPLITS])
def test_any_split_of_the_members_gives_the_bits_of_one_launch(shape, parts, dtype):
    B, T, Cn, ldy = shape
    assert sum(parts) == B
    c = case(B, T, Cn, ldy, dtype)
    state, lo = None, 0
    for n in parts:
        state = launch(c, c["y"][lo:lo + n], ldy, dtype, count_before=lo, state=state)
        lo += n
    assert not same(state, run_once(B, T, Cn, ldy, dtype))


@DTYPES
def test_a_tie_keeps_the_earliest_member(dtype):
    B, T, Cn, ldy = 2, 33, 72, 80
    c = dict(case(B, T, Cn, ldy, dtype))
    y = np.array(c["y"])
    y[1] = y[0]                                   # identical rows and identical statistics: every (t, n) is a tie
    F = H.field(c, y, ldy, dtype)
    assert np.array_equal(bits(F[0]), bits(F[1]))
    got = launch(c, y, ldy, dtype)
    assert not got["arg_max"].any() and not got["arg_min"].any()
    assert np.array_equal(bits(got["max"]), bits(F[0])) and np.array_equal(bits(got["min"]), bits(F[0]))
    # across two launches the earlier launch's member stays
    first = launch(c, y[:1], ldy, dtype)
    second = launch(c, y[1:], ldy, dtype, count_before=1, state=first)
    assert not second["arg_max"].any() and not second["arg_min"].any()
    assert not same(second, got)
    # and a later member that is larger somewhere does take over there, with its own index
    y3 = np.concatenate([y, np.array(c["y"][1:2])])
    F3 = H.field(c, y3, ldy, dtype)
    got3 = launch(c, y3, ldy, dtype)
    assert np.array_equal(got3["arg_max"], np.argmax(F3, 0)) and np.array_equal(got3["arg_min"], np.argmin(F3, 0))
    assert set(np.unique(got3["arg_max"])) == {0, 2}


@DTYPES
@pytest.mark.parametrize("B,T,Cn,ldy", [(3, 5, 40, 40), (4, 9, 2080, 2080)])
def test_a_value_equal_to_the_limit_is_not_counted(B, T, Cn, ldy, dtype):
    c = case(B, T, Cn, ldy, dtype)
    F = c["F"]
    b0, t0 = B - 1, T // 2
    limit = np.array(F[b0, t0])                   # limit_n = F[b0, t0, n]
    got = launch(c, c["y"], ldy, dtype, groups=("exceed",), limit=limit)
    assert np.array_equal(got["exceed"], (F > limit).sum(0))
    others = (np.delete(F[:, t0], b0, axis=0) > limit).sum(0)
    assert np.array_equal(got["exceed"][t0], others)          # member b0 itself is not counted at (t0, n)
    above = launch(c, c["y"], ldy, dtype, groups=("exceed",), limit=np.nextafter(limit, np.float32(-np.inf)))
    assert np.array_equal(above["exceed"][t0], others + 1)    # one unit below the value it is


SUBSETS = [s for r in (1, 2) for s in itertools.combinations(ALL, r)]


@DTYPES
@pytest.mark.parametrize("B,T,Cn,ldy", SHAPES)
def test_every_subset_of_the_groups_gives_the_bits_of_the_full_call(B, T, Cn, ldy, dtype):
    c = case(B, T, Cn, ldy, dtype)
    full = run_once(B, T, Cn, ldy, dtype)
    h = B // 2          # the continuing launch (it reads the state) as well, where there are members for two
    for sub in SUBSETS:
        names = tuple(k for g in sub for k in GROUPS[g] if k != "limit")
        got = launch(c, c["y"], ldy, dtype, groups=sub)
        assert not same(got, full, names), (sub, same(got, full, names))
        for k in set(STATE) - set(names):          # launch() has checked that they were not written; they still hold the fill
            assert (got[k] == H.UNWRITTEN).all() if k in INT else np.isnan(got[k]).all()
        if h:
            first = launch(c, c["y"][:h], ldy, dtype, groups=sub)
            rest = {k: (first[k] if k in names else full[k]) for k in STATE}
            got = launch(c, c["y"][h:], ldy, dtype, groups=sub, count_before=h, state=rest)
            assert not same(got, full), (sub, same(got, full))      # the arrays not asked for were handed in complete and left alone


@DTYPES
@pytest.mark.parametrize("B,T,Cn,ldy", SHAPES)
def test_two_launches_are_bitwise_equal(B, T, Cn, ldy, dtype):
    c = case(B, T, Cn, ldy, dtype)
    assert not same(launch(c, c["y"], ldy, dtype), run_once(B, T, Cn, ldy, dtype))


def test_the_largest_count_is_accepted_and_the_index_is_the_members():
    B, T, Cn, ldy, dtype = 3, 5, 40, 40, 0
    c = case(B, T, Cn, ldy, dtype)
    base = (1 << 24) - B
    state = ER.empty_state(T, Cn)                 # as if 2^24 - 3 members had left nothing behind: every extremum is taken again
    got = launch(c, c["y"], ldy, dtype, count_before=base, state=state)
    want = ER.update(c["F"], state, base, limit=c["limit"])
    assert not same(got, want)
    assert np.array_equal(got["arg_max"], base + np.argmax(c["F"], 0)) and got["arg_max"].max() == (1 << 24) - 1


def test_rejected_arguments_write_nothing():
    import torch
    B, T, Cn, ldy, dtype = 3, 5, 40, 40, 0
    c = case(B, T, Cn, ldy, dtype)
    d = H.device_inputs(c, c["y"], ldy, dtype)
    bufs = H.canary_buffers(H.sizes(PASS, B, T, Cn, count_before=0), integer=INT)
    bufs["limit"][1].copy_(torch.from_numpy(np.array(c["limit"])).cuda())
    for name in STATE:
        bufs[name][1].fill_(H.UNWRITTEN if name in INT else float("nan"))
    good = H.hook_args(d, bufs, ldy, dtype, B, T, Cn, count_before=0)
    none = {k: None for k in bufs}
    bad = H.common_rejections(good)
    bad += [(dict(no_struct=True), "null argument"), (none, "no group of the state is given")]
    bad += [({k: None}, "half a group") for k in bufs]                                               # each array missing from its group
    bad += [(dict(none, **{k: good[k]}), "half a group") for k in bufs]                              # each array alone
    bad += [({k: good[k] + 4}, "misaligned pointer") for k in STATE] + [(dict(limit=good["limit"] + 2), "misaligned pointer")]
    bad += [(dict(count_before=v), "outside [0, 2^24]") for v in (-1, (1 << 24) - B + 1, 1 << 40)]
    H.reject_all(PASS, d, bufs, good, bad)
    assert not same(H.outputs_of(PASS, bufs, B, T, Cn, count_before=0), run_once(B, T, Cn, ldy, dtype))
