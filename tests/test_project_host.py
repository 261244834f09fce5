"""The host side of the surrogate's linear functionals (simulgen-vae_amd/predict.py: functional_weights, region_weights, ProjectResult;
engine.py: the bindings of sgv_project and sgv_test_recon_project) and the numpy restatement of the project pass
(tests/project_reference.py).  No GPU.

The emulation is held to the a-priori bound of an fp32 summation in any order against float64,
|q - q64| <= (C + 2) 2^-24 sum_n |W[r, n] F[n]| (project_reference.bound), on random data at C = 520 and at the other widths of the
kernel tests: C = 520 lies in one wave's share, C = 1032 and C = 4104 cross the end of a wave's and of a block's share."""
import os
import re
import sys

import numpy as np
import pytest
import torch

import simulgen_vae_amd  # noqa: F401
from simulgen_vae_amd import engine as E
from simulgen_vae_amd.predict import ProjectResult, Surrogate, functional_weights, region_weights

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import project_reference as PR  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["sgv_project", "sgv_test_recon_project"]


# ---- functional_weights ----
def test_functional_weights_accepts_rows_and_a_single_vector():
    N = 24
    W = np.random.default_rng(0).standard_normal((3, N))
    for a in (W, W.astype(np.float32), W.astype(np.float16), W.tolist()):
        w = functional_weights(a, N)
        assert isinstance(w, np.ndarray) and w.dtype == np.float32 and w.shape == (3, N) and w.flags["C_CONTIGUOUS"]
        assert np.array_equal(w, np.asarray(a, np.float32))
    one = functional_weights(W[1], N)
    assert one.shape == (1, N) and np.array_equal(one[0], W[1].astype(np.float32))
    assert functional_weights(np.zeros((E.MAX_FUNCTIONALS, N)), N).shape == (32, N) and E.MAX_FUNCTIONALS == 32
    strided = functional_weights(np.asfortranarray(W), N)
    assert strided.flags["C_CONTIGUOUS"] and np.array_equal(strided, W.astype(np.float32))
    cpu = functional_weights(torch.from_numpy(W), N)          # a host tensor is host data
    assert isinstance(cpu, np.ndarray) and np.array_equal(cpu, W.astype(np.float32))


def test_functional_weights_names_what_is_wrong():
    N = 24
    with pytest.raises(ValueError, match=r"weights: an \[R, N\] or \[N\] array is required, got shape \(2, 3, 24\)"):
        functional_weights(np.zeros((2, 3, N)), N)
    with pytest.raises(ValueError, match=r"weights: an \[R, N\] or \[N\] array is required, got shape \(\)"):
        functional_weights(1.0, N)
    with pytest.raises(ValueError, match=r"weights: the last dimension is 23, expected N = 24 \(shape \(3, 23\)\)"):
        functional_weights(np.zeros((3, 23)), N)
    with pytest.raises(ValueError, match=r"weights: the last dimension is 25, expected N = 24"):
        functional_weights(np.zeros(25), N)
    with pytest.raises(ValueError, match=r"weights: R = 33 rows, between 1 and 32 are required"):
        functional_weights(np.zeros((33, N)), N)
    with pytest.raises(ValueError, match=r"weights: R = 0 rows, between 1 and 32 are required"):
        functional_weights(np.zeros((0, N)), N)
    for bad in (np.zeros((2, N), np.int32), np.zeros((2, N), bool), np.zeros((2, N), np.complex64)):
        with pytest.raises(ValueError, match=rf"weights: a floating dtype is required, not {bad.dtype}"):
            functional_weights(bad, N)
    W = np.zeros((3, N))
    W[2, 5] = np.inf
    W[1, 7] = np.nan          # the first in row-major order is named
    with pytest.raises(ValueError, match=r"weights\[1, 7\] = nan is not finite as float32"):
        functional_weights(W, N)
    W = np.zeros((3, N))
    W[2, 5] = 1e39
    with pytest.raises(ValueError, match=r"weights\[2, 5\] = 1e\+39 is not finite as float32"):
        functional_weights(W, N)
    assert "NOT read back" in functional_weights.__doc__


# ---- region_weights ----
def test_region_weights_rows_are_the_regions():
    lab = np.array([0, 2, -1, 1, 2, 2, -1, 0], np.int64)
    S = region_weights(lab, reduce="sum")
    assert S.dtype == np.float32 and S.shape == (3, 8)
    assert np.array_equal(S, np.array([[1, 0, 0, 0, 0, 0, 0, 1], [0, 0, 0, 1, 0, 0, 0, 0], [0, 1, 0, 0, 1, 1, 0, 0]], np.float32))
    nw = np.array([2.0, 1.0, 9.0, 4.0, 3.0, 0.5, 9.0, 6.0])
    S = region_weights(lab, node_weights=nw, reduce="sum")
    assert np.array_equal(S[0], np.array([2, 0, 0, 0, 0, 0, 0, 6], np.float32)) and np.array_equal(S[2], np.array([0, 1, 0, 0, 3, .5, 0, 0], np.float32))
    M = region_weights(lab, node_weights=nw)          # "mean" is the default
    assert np.array_equal(M[0], (np.array([2, 0, 0, 0, 0, 0, 0, 6]) / 8.0).astype(np.float32))
    assert np.array_equal(M[2], (np.array([0, 1, 0, 0, 3, .5, 0, 0]) / 4.5).astype(np.float32))
    assert not S[:, lab == -1].any() and not M[:, lab == -1].any()          # nodes in no region: weight 0 in every row
    # more regions than labels: allowed under "sum" (rows of zeros), and an int32 label vector
    assert np.array_equal(region_weights(lab.astype(np.int32), num_regions=5, reduce="sum")[3:], np.zeros((2, 8), np.float32))


def test_region_means_sum_to_one():
    """every entry is one rounding of w / sum to fp32, all entries positive: the row's sum is within 2^-24 of 1 (plus the float64 sum's own rounding)"""
    rng = np.random.default_rng(3)
    N = 5000
    lab = rng.integers(-1, 32, N)
    nw = np.exp(rng.uniform(np.log(1e-3), np.log(1e3), N))
    for w in (None, nw):
        M = region_weights(lab, node_weights=w)
        assert M.shape == (32, N) and not M[:, lab == -1].any()
        sums = M.astype(np.float64).sum(axis=1)
        assert np.all(np.abs(sums - 1.0) <= 2.0 ** -24 + N * 2.0 ** -53), np.abs(sums - 1.0).max()
        for r in (0, 31):
            assert not M[r, lab != r].any() and np.all(M[r, lab == r] > 0)


def test_region_weights_names_what_is_wrong():
    lab = np.array([0, 1, -1, 1])
    with pytest.raises(ValueError, match="reduce must be 'mean' or 'sum', not 'max'"):
        region_weights(lab, reduce="max")
    with pytest.raises(ValueError, match=r"labels: a 1-D array of N region labels is required, got shape \(2, 2\)"):
        region_weights(lab.reshape(2, 2))
    with pytest.raises(ValueError, match="labels: an integer dtype is required, not float64"):
        region_weights(lab.astype(np.float64))
    with pytest.raises(ValueError, match=r"labels\[2\] = -2 is below -1"):
        region_weights(np.array([0, 1, -2, 1]))
    with pytest.raises(ValueError, match=r"labels\[1\] = 1 is outside \[-1, num_regions = 1\)"):
        region_weights(lab, num_regions=1)
    with pytest.raises(ValueError, match="33 regions, at most 32 fit one call"):
        region_weights(np.arange(33))
    with pytest.raises(ValueError, match="33 regions, at most 32 fit one call"):
        region_weights(lab, num_regions=33)
    with pytest.raises(ValueError, match="0 regions, at least one is required"):
        region_weights(np.array([-1, -1]))
    with pytest.raises(ValueError, match="region 2 has no nodes"):
        region_weights(lab, num_regions=3)
    with pytest.raises(ValueError, match="region 1 has no nodes"):
        region_weights(np.array([0, 2, 2]))
    with pytest.raises(ValueError, match="region 1: its node weights sum to zero"):
        region_weights(lab, node_weights=np.array([1.0, 2.0, 1.0, -2.0]))
    with pytest.raises(ValueError, match=r"node_weights: shape \(3,\), expected \(N,\) = \(4,\)"):
        region_weights(lab, node_weights=np.ones(3))
    with pytest.raises(ValueError, match=r"node_weights\[3\] = inf is not finite"):
        region_weights(lab, node_weights=np.array([1.0, 1.0, 1.0, np.inf]))
    assert region_weights(lab, num_regions=3, reduce="sum").shape == (3, 4)          # an empty region is only refused for a mean


# ---- ProjectResult ----
def test_project_result_fields_peak_and_time_integral():
    assert ProjectResult.FIELDS == ("values",)
    rng = np.random.default_rng(5)
    v = rng.standard_normal((4, 9, 3)).astype(np.float32)
    v[0, 2, 0] = v[0, 6, 0] = 7.0          # a tie: the smallest t
    v[1, :, 1] = -1.5                      # every step ties
    v[2, 8, 2] = 9.0                       # the last step
    res = ProjectResult(values=torch.from_numpy(v))
    assert res.values.shape == (4, 9, 3)
    top, when = res.peak()
    assert top.dtype == torch.float32 and top.shape == (4, 3) and when.shape == (4, 3)
    assert np.array_equal(top.numpy(), v.max(axis=1))
    assert np.array_equal(when.numpy(), v.argmax(axis=1))          # numpy: the first occurrence
    assert int(when[0, 0]) == 2 and int(when[1, 1]) == 0 and int(when[2, 2]) == 8
    trapezoid = getattr(np, "trapezoid", None) or np.trapz
    for dt in (1.0, 0.025):
        got = res.time_integral(dt)
        assert got.dtype == torch.float32 and got.shape == (4, 3)
        want = trapezoid(v.astype(np.float64), dx=dt, axis=1)
        assert np.array_equal(got.numpy(), want.astype(np.float32)) or np.all(np.abs(got.numpy() - want) <= 2.0 ** -23 * np.abs(want) + 1e-300)
    one = ProjectResult(values=torch.from_numpy(v[:, :1]))
    assert not one.time_integral().any() and np.array_equal(one.peak()[0].numpy(), v[:, 0]) and not one.peak()[1].any()
    with pytest.raises(KeyError):
        ProjectResult()
    assert hasattr(Surrogate, "project")


def test_bindings():
    hdr = open(os.path.join(ROOT, "include", "sgvae.h")).read()
    for s in NEW_SYMBOLS:
        assert re.search(rf"\bint {s}\s*\(", hdr), s
        assert s in E.ABI_SYMBOLS
    lib = E.load_library()
    for s in NEW_SYMBOLS:
        assert hasattr(lib, s), s
    assert len(lib.sgv_project.argtypes) == 10 and len(lib.sgv_test_recon_project.argtypes) == 15
    # without an engine the call is an argument error that says who complains
    assert lib.sgv_project(None, None, None, 1, 1, None, None, None, 1, None) == -1 and "sgv_project" in lib.sgv_last_error().decode()
    assert lib.sgv_test_recon_project(0, None, 8, None, None, None, None, None, None, 1, None, 1, 1, 8, None) == -1
    assert "sgv_test_recon_project" in lib.sgv_last_error().decode()
    # the row offset of a study's noise
    assert re.search(r"\bint sgv_set_draw_row\s*\(", hdr) and "sgv_set_draw_row" in E.ABI_SYMBOLS and len(lib.sgv_set_draw_row.argtypes) == 2
    assert lib.sgv_set_draw_row(None, 0) == -1 and hasattr(E.Engine, "set_draw_row")


# ---- the emulation ----
def _random_case(C, R, rows=(2, 3), seed=0):
    rng = np.random.default_rng(seed + C)
    F = (rng.standard_normal(rows + (C,)) * np.exp(rng.uniform(-6, 6, C))).astype(np.float32)
    return F, PR.mixed_weights(R, C, seed)


def test_chain_order_takes_every_channel_once():
    for lo, hi in ((0, 8), (0, 16), (0, 520), (1024, 1032), (2048, 3072)):
        order = PR.chain_order(lo, hi)
        assert sorted(order) == list(range(lo, hi))
    assert PR.chain_order(0, 24) == [0, 8, 1, 9, 2, 10, 3, 11, 4, 12, 5, 13, 6, 14, 7, 15, 16, 17, 18, 19, 20, 21, 22, 23]
    assert PR.CHUNK == 4 * PR.WAVE_COLS and PR.WAVE_COLS % 16 == 0


@pytest.mark.parametrize("C,R", [(8, 1), (72, 3), (520, 32), (1032, 3), (4104, 2)])
def test_emulation_is_within_the_bound_of_float64(C, R):
    F, W = _random_case(C, R)
    q = PR.emulate(F, W)
    assert q.dtype == np.float32 and q.shape == (2, 3, R)
    ratio = PR.worst_ratio(q, F, W)
    print(f"  C = {C}, R = {R}: worst err / bound {ratio:.4f}")
    assert ratio <= 1.0
    assert W.size < 64 or ((W == 0).any() and (W > 0).any() and (W < 0).any())          # eight weights may all have one sign


def test_emulation_does_not_depend_on_the_cut_into_batches_or_on_the_other_rows():
    F, W = _random_case(520, 32, rows=(5, 4))
    whole = PR.emulate(F, W)
    for cut in (1, 2, 3):
        parts = np.concatenate([PR.emulate(F[lo:lo + cut], W) for lo in range(0, 5, cut)])
        assert np.array_equal(whole.view(np.int32), parts.view(np.int32))
    for r in (0, 17, 31):
        assert np.array_equal(PR.emulate(F, W[r:r + 1])[..., 0].view(np.int32), whole[..., r].view(np.int32))
    perm = np.random.default_rng(1).permutation(32)
    assert np.array_equal(PR.emulate(F, W[perm]).view(np.int32), whole[..., perm].view(np.int32))


@pytest.mark.parametrize("C", [520, 1032])
def test_one_hot_rows_pick_their_column_and_a_zero_row_gives_zero(C):
    F, _ = _random_case(C, 1)
    nodes = [0, C - 1, C - 5]
    W = np.zeros((5, C), np.float32)
    for k, n in enumerate(nodes):
        W[k, n] = 1.0
    W[4, 3] = -2.0
    q = PR.emulate(F, W)
    for k, n in enumerate(nodes):
        assert np.array_equal(q[..., k], F[..., n])
    assert np.array_equal(q[..., 3], np.zeros(F.shape[:-1], np.float32))
    assert np.array_equal(q[..., 4], -2.0 * F[..., 3])
    assert PR.worst_ratio(q, F, W) == 0.0
