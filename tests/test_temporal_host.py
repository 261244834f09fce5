"""The host side of the surrogate's temporal functionals (simulgen-vae_amd/predict.py: temporal_weights, fourier_rows, window_rows,
TemporalResult; engine.py: the bindings of sgv_temporal and sgv_test_recon_temporal) and the numpy restatement of the temporal pass
(tests/temporal_reference.py).  No GPU.

The emulation is held to the a-priori bound of an fp32 summation in any order against float64,
|q - q64| <= (T + 2) 2^-24 sum_t |W[r, t] F[t, n]| (temporal_reference.bound), on random data at the T of the kernel tests."""
import os
import re
import sys

import numpy as np
import pytest
import torch

import simulgen_vae_amd  # noqa: F401
from simulgen_vae_amd import engine as E
from simulgen_vae_amd.predict import Surrogate, TemporalResult, fourier_rows, temporal_weights, window_rows

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import temporal_reference as TR  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["sgv_temporal", "sgv_test_recon_temporal"]


# ---- temporal_weights ----
def test_temporal_weights_accepts_rows_and_a_single_vector():
    T = 12
    W = np.random.default_rng(0).standard_normal((3, T))
    for a in (W, W.astype(np.float32), W.astype(np.float16), W.tolist()):
        w = temporal_weights(a, T)
        assert isinstance(w, np.ndarray) and w.dtype == np.float32 and w.shape == (3, T) and w.flags["C_CONTIGUOUS"]
        assert np.array_equal(w, np.asarray(a, np.float32))
    one = temporal_weights(W[1], T)
    assert one.shape == (1, T) and np.array_equal(one[0], W[1].astype(np.float32))
    assert temporal_weights(np.zeros((E.MAX_TEMPORAL, T)), T).shape == (32, T) and E.MAX_TEMPORAL == 32
    strided = temporal_weights(np.asfortranarray(W), T)
    assert strided.flags["C_CONTIGUOUS"] and np.array_equal(strided, W.astype(np.float32))
    cpu = temporal_weights(torch.from_numpy(W), T)          # a host tensor is host data
    assert isinstance(cpu, np.ndarray) and np.array_equal(cpu, W.astype(np.float32))


def test_temporal_weights_names_what_is_wrong():
    T = 12
    with pytest.raises(ValueError, match=r"weights: an \[R, T\] or \[T\] array is required, got shape \(2, 3, 12\)"):
        temporal_weights(np.zeros((2, 3, T)), T)
    with pytest.raises(ValueError, match=r"weights: an \[R, T\] or \[T\] array is required, got shape \(\)"):
        temporal_weights(1.0, T)
    with pytest.raises(ValueError, match=r"weights: the last dimension is 11, expected T = 12 \(shape \(3, 11\)\)"):
        temporal_weights(np.zeros((3, 11)), T)
    with pytest.raises(ValueError, match=r"weights: the last dimension is 13, expected T = 12"):
        temporal_weights(np.zeros(13), T)
    with pytest.raises(ValueError, match=r"weights: R = 33 rows, between 1 and 32 are required"):
        temporal_weights(np.zeros((33, T)), T)
    with pytest.raises(ValueError, match=r"weights: R = 0 rows, between 1 and 32 are required"):
        temporal_weights(np.zeros((0, T)), T)
    for bad in (np.zeros((2, T), np.int32), np.zeros((2, T), bool), np.zeros((2, T), np.complex64)):
        with pytest.raises(ValueError, match=rf"weights: a floating dtype is required, not {bad.dtype}"):
            temporal_weights(bad, T)
    W = np.zeros((3, T))
    W[2, 5] = np.inf
    W[1, 7] = np.nan          # the first in row-major order is named
    with pytest.raises(ValueError, match=r"weights: row 1 is not finite as float32 at time step 7: weights\[1, 7\] = nan"):
        temporal_weights(W, T)
    W = np.zeros((3, T))
    W[2, 5] = 1e39
    with pytest.raises(ValueError, match=r"weights: row 2 is not finite as float32 at time step 5: weights\[2, 5\] = 1e\+39"):
        temporal_weights(W, T)
    assert "NOT read back" in temporal_weights.__doc__


# ---- fourier_rows ----
def _sinusoid(T, k, A, phi, dt):
    t = np.arange(T) * dt
    return A * np.cos(2.0 * np.pi * (k / (T * dt)) * t - phi)


@pytest.mark.parametrize("T,dt", [(200, 1.0), (33, 0.025), (12, 2.0)])
def test_fourier_rows_recover_amplitude_and_phase_at_bin_frequencies(T, dt):
    ks = [1, 3, T // 2 - 1]
    freqs = [k / (T * dt) for k in ks]
    W = fourier_rows(T, freqs, dt=dt)
    assert W.dtype == np.float32 and W.shape == (6, T) and W.flags["C_CONTIGUOUS"]
    for i, k in enumerate(ks):
        for A, phi in ((1.0, 0.0), (3.5, 0.7), (0.02, -2.4), (17.0, np.pi / 2)):
            x = _sinusoid(T, k, A, phi, dt)
            c, s = W[2 * i].astype(np.float64) @ x, W[2 * i + 1].astype(np.float64) @ x
            assert abs(np.hypot(c, s) - A) <= 1e-6 * A, (k, A, phi)
            dphi = np.arctan2(s, c) - phi
            assert abs((dphi + np.pi) % (2 * np.pi) - np.pi) <= 1e-6, (k, A, phi)
            # another bin's sinusoid is not seen: the rows are orthogonal on the grid, up to their fp32 rounding
            other = _sinusoid(T, ks[(i + 1) % 3], A, phi, dt)
            assert np.hypot(W[2 * i].astype(np.float64) @ other, W[2 * i + 1].astype(np.float64) @ other) <= 1e-6 * A
    # f = 0: the mean; the sine row is zero
    W0 = fourier_rows(T, [0.0], dt=dt)
    assert not W0[1].any() and abs(W0[0].astype(np.float64).sum() - 1.0) <= 1e-6
    # a scalar frequency, and float64 arithmetic rounded once
    one = fourier_rows(T, freqs[0], dt=dt)
    assert np.array_equal(one, W[:2])
    t = np.arange(T, dtype=np.float64)
    assert np.all(np.abs(W[0] - 2.0 / T * np.cos(2 * np.pi * ks[0] * t / T)) <= 2.0 ** -24 * 2.0 / T + 1e-15)


def test_fourier_rows_fold_the_window_and_renormalise():
    T, dt, k = 64, 0.5, 5
    hann = 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(T) / T)          # periodic Hann: its spectrum is zero two bins away and beyond
    W = fourier_rows(T, [k / (T * dt)], dt=dt, window=hann)
    plain = fourier_rows(T, [k / (T * dt)], dt=dt)
    assert np.all(np.abs(W - plain.astype(np.float64) * hann * T / hann.sum()) <= 2.0 ** -23 * np.abs(plain) * 2.0 + 1e-12)
    x = _sinusoid(T, k, 2.5, 1.1, dt)
    c, s = W[0].astype(np.float64) @ x, W[1].astype(np.float64) @ x
    assert abs(np.hypot(c, s) - 2.5) <= 1e-6 * 2.5 and abs(np.arctan2(s, c) - 1.1) <= 1e-6
    # Nyquist on an even grid: the cosine row alone, scaled by 1 / sum
    Wn = fourier_rows(T, [0.5 / dt], dt=dt)
    assert not Wn[1].any() and abs(Wn[0].astype(np.float64) @ _sinusoid(T, T // 2, 4.0, 0.0, dt) - 4.0) <= 4e-6


def test_fourier_rows_names_what_is_wrong():
    with pytest.raises(ValueError, match="fourier_rows: T = 0, at least one time step is required"):
        fourier_rows(0, [0.1])
    with pytest.raises(ValueError, match="fourier_rows: dt = 0.0 must be positive and finite"):
        fourier_rows(8, [0.1], dt=0.0)
    with pytest.raises(ValueError, match="fourier_rows: a list of frequencies is required"):
        fourier_rows(8, [])
    with pytest.raises(ValueError, match="fourier_rows: 17 frequencies give 34 rows, at most 32 fit one call"):
        fourier_rows(64, np.linspace(0.0, 0.4, 17))
    with pytest.raises(ValueError, match=r"fourier_rows: freqs\[1\] = -0.25 is outside \[0, 1 / \(2 dt\) = 0.5\]"):
        fourier_rows(8, [0.1, -0.25])
    with pytest.raises(ValueError, match=r"fourier_rows: freqs\[0\] = 0.3 is outside \[0, 1 / \(2 dt\) = 0.25\]"):
        fourier_rows(8, [0.3], dt=2.0)
    with pytest.raises(ValueError, match=r"fourier_rows: freqs\[2\] = nan is outside"):
        fourier_rows(8, [0.1, 0.2, np.nan])
    with pytest.raises(ValueError, match=r"fourier_rows: window has shape \(7,\), expected \(T,\) = \(8,\)"):
        fourier_rows(8, [0.1], window=np.ones(7))
    with pytest.raises(ValueError, match=r"fourier_rows: window\[3\] = inf is not finite"):
        fourier_rows(8, [0.1], window=np.array([1, 1, 1, np.inf, 1, 1, 1, 1.0]))
    with pytest.raises(ValueError, match="fourier_rows: the window sums to zero"):
        fourier_rows(8, [0.1], window=np.array([1, -1, 1, -1, 1, -1, 1, -1.0]))
    assert fourier_rows(64, np.linspace(0.0, 0.4, 16)).shape == (32, 64)


# ---- window_rows ----
def test_window_rows_are_means_over_their_windows():
    T = 33
    W = window_rows(T, [0, 1, 8, 20, 33])
    assert W.dtype == np.float32 and W.shape == (4, T)
    for i, (lo, hi) in enumerate(((0, 1), (1, 8), (8, 20), (20, 33))):
        assert not W[i, :lo].any() and not W[i, hi:].any() and np.all(W[i, lo:hi] == np.float32(1.0 / (hi - lo)))
        assert abs(W[i].astype(np.float64).sum() - 1.0) <= (hi - lo) * 2.0 ** -25          # hi - lo equal entries, one fp32 rounding of 1 / n each
    whole = window_rows(T, np.array([0, T], np.int32))
    assert whole.shape == (1, T) and np.all(whole == np.float32(1.0 / T))
    assert window_rows(64, np.arange(0, 65, 2)).shape == (32, 64)
    part = window_rows(T, [4, 9])          # the windows need not cover the time axis
    assert part.shape == (1, T) and np.count_nonzero(part) == 5


def test_window_rows_refuse_bad_edges():
    with pytest.raises(ValueError, match="window_rows: T = 0, at least one time step is required"):
        window_rows(0, [0, 1])
    with pytest.raises(ValueError, match=r"window_rows: edges must be a 1-D array, got shape \(2, 2\)"):
        window_rows(8, [[0, 1], [2, 3]])
    with pytest.raises(ValueError, match="window_rows: edges must be of an integer dtype, not float64"):
        window_rows(8, [0.0, 4.0])
    with pytest.raises(ValueError, match="window_rows: 1 edges, at least two are required"):
        window_rows(8, [0])
    with pytest.raises(ValueError, match="window_rows: 33 windows, at most 32 fit one call"):
        window_rows(64, np.arange(34))
    with pytest.raises(ValueError, match=r"window_rows: edges\[2\] = 9 is outside \[0, T = 8\]"):
        window_rows(8, [0, 4, 9])
    with pytest.raises(ValueError, match=r"window_rows: edges\[0\] = -1 is outside \[0, T = 8\]"):
        window_rows(8, [-1, 4])
    with pytest.raises(ValueError, match=r"window_rows: edges\[2\] = 4 is not above edges\[1\] = 4"):
        window_rows(8, [0, 4, 4, 8])
    with pytest.raises(ValueError, match=r"window_rows: edges\[1\] = 2 is not above edges\[0\] = 5"):
        window_rows(8, [5, 2])


# ---- TemporalResult ----
def test_temporal_result_amplitude_phase_and_peak():
    assert TemporalResult.FIELDS == ("values",)
    rng = np.random.default_rng(5)
    v = rng.standard_normal((4, 6, 9)).astype(np.float32)
    v[0, 0, 2] = v[0, 0, 6] = -7.0         # a tie of |value|: the smallest node, and the sign is kept
    v[1, 1, :] = 1.5                       # every node ties
    v[2, 5, 8] = 9.0                       # the last node
    res = TemporalResult(values=torch.from_numpy(v))
    amp, ph = res.amplitude(), res.phase()
    assert amp.dtype == torch.float32 and amp.shape == (4, 3, 9) and ph.shape == (4, 3, 9)
    assert np.allclose(amp.numpy(), np.hypot(v[:, 0::2], v[:, 1::2]), rtol=1e-6, atol=0)
    assert np.allclose(ph.numpy(), np.arctan2(v[:, 1::2], v[:, 0::2]), rtol=0, atol=1e-6)
    where, top = res.peak()
    assert where.dtype == torch.int64 and where.shape == (4, 6) and top.dtype == torch.float32 and top.shape == (4, 6)
    assert np.array_equal(where.numpy(), np.abs(v).argmax(axis=2))          # numpy: the first occurrence
    assert np.array_equal(top.numpy(), np.take_along_axis(v, np.abs(v).argmax(axis=2)[..., None], 2)[..., 0])
    assert int(where[0, 0]) == 2 and float(top[0, 0]) == -7.0 and int(where[1, 1]) == 0 and int(where[2, 5]) == 8
    odd = TemporalResult(values=torch.from_numpy(v[:, :5]))
    for fn in (odd.amplitude, odd.phase):
        with pytest.raises(ValueError, match=r"consecutive \(cos, sin\) pairs \(fourier_rows\): R = 5 is odd"):
            fn()
    assert odd.peak()[0].shape == (4, 5)
    with pytest.raises(KeyError):
        TemporalResult()
    assert hasattr(Surrogate, "temporal")


def test_amplitude_of_a_host_built_spectrum():
    """fourier_rows -> values -> amplitude() / phase() on a synthetic field: two nodes, two sinusoids each"""
    T, dt = 40, 0.1
    W = fourier_rows(T, [2 / (T * dt), 7 / (T * dt)], dt=dt)
    field = np.stack([_sinusoid(T, 2, 3.0, 0.4, dt) + _sinusoid(T, 7, 0.5, -1.0, dt), _sinusoid(T, 7, 2.0, 2.0, dt)], axis=1)[None]      # [1, T, 2]
    res = TemporalResult(values=torch.from_numpy(TR.emulate(field.astype(np.float32), W)))
    amp, ph = res.amplitude().numpy()[0], res.phase().numpy()[0]
    assert np.allclose(amp, [[3.0, 0.0], [0.5, 2.0]], rtol=2e-6, atol=2e-6)
    assert np.allclose([ph[0, 0], ph[1, 0], ph[1, 1]], [0.4, -1.0, 2.0], rtol=0, atol=5e-6)


def test_bindings():
    hdr = open(os.path.join(ROOT, "include", "sgvae.h")).read()
    for s in NEW_SYMBOLS:
        assert re.search(rf"\bint {s}\s*\(", hdr), s
        assert s in E.ABI_SYMBOLS
    lib = E.load_library()
    for s in NEW_SYMBOLS:
        assert hasattr(lib, s), s
    assert len(lib.sgv_temporal.argtypes) == 10 and len(lib.sgv_test_recon_temporal.argtypes) == 15
    # without an engine the call is an argument error that says who complains
    assert lib.sgv_temporal(None, None, None, 1, 1, None, None, None, 1, None) == -1 and "sgv_temporal" in lib.sgv_last_error().decode()
    assert lib.sgv_test_recon_temporal(0, None, 8, None, None, None, None, None, None, 1, None, 1, 1, 8, None) == -1
    assert "sgv_test_recon_temporal" in lib.sgv_last_error().decode()
    # the noise follows sgv_set_draw_row, and the header says so
    assert hasattr(E.Engine, "temporal") and "sgv_temporal" in hdr[hdr.index("Noise of a study"):hdr.index("int sgv_set_draw_row")]


# ---- the emulation ----
def _random_case(T, C, R, rows=(2,), seed=0):
    rng = np.random.default_rng(seed + 100 * T + C)
    F = (rng.standard_normal(rows + (T, C)) * np.exp(rng.uniform(-6, 6, C))).astype(np.float32)
    return F, TR.mixed_weights(R, T, seed)


@pytest.mark.parametrize("T,C,R", [(1, 8, 1), (2, 72, 3), (5, 264, 32), (33, 72, 3), (200, 16, 32)])
def test_emulation_is_within_the_bound_of_float64(T, C, R):
    F, W = _random_case(T, C, R)
    q = TR.emulate(F, W)
    assert q.dtype == np.float32 and q.shape == (2, R, C)
    ratio = TR.worst_ratio(q, F, W)
    print(f"  T = {T}, C = {C}, R = {R}: worst err / bound {ratio:.4f}")
    assert ratio <= 1.0
    assert W.size < 64 or ((W == 0).any() and (W > 0).any() and (W < 0).any())
    assert TR.BLOCK_COLS == 4 * TR.WAVE_COLS and TR.WAVE_COLS == 32 * 8


def test_emulation_does_not_depend_on_the_cut_into_batches_or_on_the_other_rows():
    F, W = _random_case(33, 72, 32, rows=(5,))
    whole = TR.emulate(F, W)
    for cut in (1, 2, 3):
        parts = np.concatenate([TR.emulate(F[lo:lo + cut], W) for lo in range(0, 5, cut)])
        assert np.array_equal(whole.view(np.int32), parts.view(np.int32))
    for r in (0, 17, 31):
        assert np.array_equal(TR.emulate(F, W[r:r + 1])[:, 0].view(np.int32), whole[:, r].view(np.int32))
    perm = np.random.default_rng(1).permutation(32)
    assert np.array_equal(TR.emulate(F, W[perm]).view(np.int32), whole[:, perm].view(np.int32))


@pytest.mark.parametrize("T", [1, 2, 5, 33])
def test_one_hot_rows_pick_their_time_step_and_a_zero_row_gives_zero(T):
    F, _ = _random_case(T, 72, 1)
    steps = [0, T - 1, T // 2]
    W = np.zeros((5, T), np.float32)
    for k, t in enumerate(steps):
        W[k, t] = 1.0
    W[4, T // 3] = -2.0
    q = TR.emulate(F, W)
    for k, t in enumerate(steps):
        assert np.array_equal(q[:, k], F[:, t])
    assert np.array_equal(q[:, 3], np.zeros_like(q[:, 3]))
    assert np.array_equal(q[:, 4], -2.0 * F[:, T // 3])
    assert TR.worst_ratio(q, F, W) == 0.0
