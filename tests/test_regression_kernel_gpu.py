"""The regression pass alone (csrc/recon_out.hip: recon_regress_kernel; include/sgvae.h: sgv_test_recon_regress): the values
val[b, t, n] = (tanh(GroupNorm(y)) - min_n) / scale_n  of the members b of a launch are merged, member after member, into a running
state per (t, n) -- Welford mean / M2 and the co-moments with K weights per member -- and never stored.  Inputs as
tests/test_ensemble_kernel_gpu.py builds them; a quarter of the scales are negative.  The weights are what
predict.regression_weights makes of random covariates, one of them scaled by 1000.

Everything here is bit for bit.  The reference field F is what the existing output pass (sgv_test_recon_physical, layout
[B][T][N]) stores for the same inputs, and the state is tests/regression_reference.py, the numpy float32 emulation of the kernel's
arithmetic, run on F; mean / M2 are also compared with what the ensemble pass (sgv_test_recon_ensemble, moments) leaves for the
same members.

Shapes (B, T, C, ldy): the ensemble pass's -- the smallest case; C = 40 with groups of 5 channels (octets in three groups);
(2, 33, 72, 80) with canary padding columns and ragged row lanes; 16 members; 2080 channels in five column blocks -- and 20 members,
more than a launch holds in either dtype (16 in bf16, 8 in fp32), and 40, more than the 32-member table of the other tails.
K = 1, 3 and 32 covariates."""
import os
import sys

import numpy as np
import pytest

import simulgen_vae_amd  # noqa: F401
from simulgen_vae_amd import engine as E
from simulgen_vae_amd.predict import regression_weights

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import regression_reference as RR  # noqa: E402
import recon_kernel_common as H  # noqa: E402
from recon_kernel_common import DTYPES, bits  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 8, 8), (3, 5, 40, 40), (2, 33, 72, 80), (16, 3, 72, 72), (4, 9, 2080, 2080), (20, 2, 72, 72), (40, 2, 72, 72)]     # (B, T, C, ldy)
KS = [1, 3, 32]
STATE = RR.STATE
KPAR = pytest.mark.parametrize("K", KS)
PASS = H.Pass("regress", lambda b, T, Cn, n_cov, count_before: {"mean": (T, Cn), "m2": (T, Cn), "comoment": (n_cov, T, Cn), "w": (b, n_cov)}, STATE,
              lambda a: (a["n_cov"], a["w"], a["count_before"], H.struct(E.RegressState, a, STATE)))
MOMENTS = H.Pass("ensemble", lambda b, T, Cn: {"mean": (T, Cn), "m2": (T, Cn)}, ("mean", "m2"), lambda a: (0, H.struct(E.EnsembleState, a, ("mean", "m2"))))


def case(B, T, Cn, ldy, dtype):
    """inputs and the stored field F of one (shape, dtype), computed once and left alone"""
    c = H.case(__name__, B, T, Cn, ldy, dtype)
    assert (c["scale"] < 0).any() or Cn == 8
    return c


_WEIGHTS = {}


def weights(B, K):
    """W fp32 [B, K]: the centred covariates of B members, covariate K - 1 a thousand times the others"""
    if (B, K) not in _WEIGHTS:
        Y = np.random.default_rng(7 * B + K).standard_normal((B, K))
        Y[:, K - 1] *= 1000.0
        W = regression_weights(Y)[0]
        W.setflags(write=False)
        _WEIGHTS[(B, K)] = W
    return _WEIGHTS[(B, K)]


_WANT = {}


def want(B, T, Cn, ldy, dtype, K):
    key = (B, T, Cn, ldy, dtype, K)
    if key not in _WANT:
        _WANT[key] = RR.update(case(B, T, Cn, ldy, dtype)["F"], weights(B, K))
    return _WANT[key]


def launch(c, y, W, ldy, dtype, count_before=0, state=None):
    """one call of the hook on the members y [b, T, C] with weights W [b, K] -> the state as a dict of numpy arrays.  state: the state
    to continue from (count_before > 0), else every array holds NaN first, which a launch from empty must not read."""
    return H.launch(PASS, c, y, ldy, dtype, {"w": W}, state=state, n_cov=W.shape[1], count_before=count_before)


def same(a, b, names=STATE):
    return H.same(a, b, names)


_RUNS = {}


def run_once(B, T, Cn, ldy, dtype, K):
    """the single launch from empty"""
    key = (B, T, Cn, ldy, dtype, K)
    if key not in _RUNS:
        c = case(B, T, Cn, ldy, dtype)
        _RUNS[key] = launch(c, c["y"], weights(B, K), ldy, dtype)
    return _RUNS[key]


@DTYPES
@KPAR
@pytest.mark.parametrize("B,T,Cn,ldy", SHAPES)
def test_from_empty_equals_the_emulation_on_the_stored_field(B, T, Cn, ldy, K, dtype):
    c = case(B, T, Cn, ldy, dtype)
    got, ref = run_once(B, T, Cn, ldy, dtype, K), want(B, T, Cn, ldy, dtype, K)
    assert np.isfinite(c["F"]).all() and all(np.isfinite(got[k]).all() for k in STATE)          # the NaN the arrays held was not read
    bad = same(got, ref)
    for k in bad:
        i = np.flatnonzero(bits(got[k]).reshape(-1) != bits(ref[k]).reshape(-1))
        print(k, len(i), "mismatches, first:", got[k].reshape(-1)[i[:4]], ref[k].reshape(-1)[i[:4]])
    assert not bad, bad
    if B == 1:
        assert np.array_equal(bits(got["mean"]), bits(c["F"][0])) and not got["m2"].any() and not got["comoment"].any()
    else:
        assert got["comoment"].any()


@DTYPES
@pytest.mark.parametrize("B,T,Cn,ldy", SHAPES)
def test_the_moments_are_the_ensemble_passes(B, T, Cn, ldy, dtype):
    c = case(B, T, Cn, ldy, dtype)
    ens = H.launch(MOMENTS, c, c["y"], ldy, dtype)
    assert not same(run_once(B, T, Cn, ldy, dtype, 3), ens, ("mean", "m2"))


CUTS = [((16, 3, 72, 72), tuple(range(1, 16))), ((20, 2, 72, 72), (1, 7, 8, 9, 16, 17, 19)), ((3, 5, 40, 40), (1, 2)), ((4, 9, 2080, 2080), (3,)),
        ((40, 2, 72, 72), (33,))]


@DTYPES
@pytest.mark.parametrize("shape,cuts", CUTS, ids=[str(s[0]) for s, _ in CUTS])
def test_every_cut_into_two_launches_gives_the_bits_of_one(shape, cuts, dtype):
    B, T, Cn, ldy = shape
    c = case(B, T, Cn, ldy, dtype)
    for K in (3, 32) if B == 16 else (3,):
        W, whole = weights(B, K), run_once(B, T, Cn, ldy, dtype, K)
        for cut in cuts:
            first = launch(c, c["y"][:cut], W[:cut], ldy, dtype)
            both = launch(c, c["y"][cut:], W[cut:], ldy, dtype, count_before=cut, state=first)
            assert not same(both, whole), (K, cut, same(both, whole))


@DTYPES
@KPAR
def test_a_state_that_is_not_zero_is_continued(K, dtype):
    B, T, Cn, ldy = 3, 5, 40, 40
    c = case(B, T, Cn, ldy, dtype)
    rng = np.random.default_rng(11)
    state = dict(mean=rng.standard_normal((T, Cn)).astype(np.float32), m2=rng.random((T, Cn)).astype(np.float32) * 9,
                 comoment=rng.standard_normal((K, T, Cn)).astype(np.float32) * 100)
    for cb in (5, (1 << 24) - B):                 # the largest count is accepted
        got = launch(c, c["y"], weights(B, K), ldy, dtype, count_before=cb, state=state)
        assert not same(got, RR.update(c["F"], weights(B, K), state, cb))


@DTYPES
@pytest.mark.parametrize("B,T,Cn,ldy", [(3, 5, 40, 40), (20, 2, 72, 72)])
def test_a_column_of_zero_weights_leaves_plus_zero(B, T, Cn, ldy, dtype):
    c = case(B, T, Cn, ldy, dtype)
    W = np.array(weights(B, 3))
    W[:, 1] = 0.0
    got = launch(c, c["y"], W, ldy, dtype)
    assert not bits(got["comoment"][1]).any()          # +0 everywhere, not -0
    assert not same(got, RR.update(c["F"], W))
    full = run_once(B, T, Cn, ldy, dtype, 3)
    assert np.array_equal(bits(got["comoment"][[0, 2]]), bits(full["comoment"][[0, 2]]))          # the other covariates do not notice


@DTYPES
@pytest.mark.parametrize("B,T,Cn,ldy", SHAPES)
def test_two_launches_are_bitwise_equal(B, T, Cn, ldy, dtype):
    c = case(B, T, Cn, ldy, dtype)
    assert not same(launch(c, c["y"], weights(B, 32), ldy, dtype), run_once(B, T, Cn, ldy, dtype, 32))


def test_rejected_arguments_write_nothing():
    import torch
    lib = E.load_library()
    B, T, Cn, ldy, dtype, K = 3, 5, 40, 40, 0, 3
    c = case(B, T, Cn, ldy, dtype)
    d = H.device_inputs(c, c["y"], ldy, dtype)
    bufs = H.canary_buffers(H.sizes(PASS, B, T, Cn, n_cov=K, count_before=0))
    bufs["w"][1].copy_(torch.from_numpy(np.array(weights(B, K)).reshape(-1)).cuda())
    for name in STATE:
        bufs[name][1].fill_(float("nan"))
    good = H.hook_args(d, bufs, ldy, dtype, B, T, Cn, n_cov=K, count_before=0)
    bad = H.common_rejections(good) + [(dict(w=None), "null argument"), (dict(no_struct=True), "null argument")]
    bad += [({k: None}, "mean, m2 and comoment are all required") for k in STATE]
    bad += [(dict(n_cov=0), "n_cov = 0 is outside [1, 32]"), (dict(n_cov=33), "n_cov = 33 is outside [1, 32]"), (dict(n_cov=-1), "is outside [1, 32]")]
    bad += [({k: good[k] + 4}, "misaligned pointer") for k in STATE] + [(dict(w=good["w"] + 2), "misaligned pointer")]
    bad += [(dict(count_before=v), "outside [0, 2^24]") for v in (-1, (1 << 24) - B + 1, 1 << 40)]
    H.reject_all(PASS, d, bufs, good, bad)
    assert not same(H.outputs_of(PASS, bufs, B, T, Cn, n_cov=K, count_before=0), run_once(B, T, Cn, ldy, dtype, K))
    # the weights need 4-byte alignment only
    w4 = torch.zeros(B * K + 1, device="cuda")
    w4[1:].copy_(bufs["w"][1])
    assert H.call(PASS, dict(good, w=w4.data_ptr() + 4)) == 0, lib.sgv_last_error().decode()
    assert not same(H.outputs_of(PASS, bufs, B, T, Cn, n_cov=K, count_before=0), run_once(B, T, Cn, ldy, dtype, K))
