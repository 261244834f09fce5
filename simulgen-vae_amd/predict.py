"""Surrogate prediction: a trained VAE plus a trained latent conditioner as a simulator -- conditions in, `[T, N]` fields in
physical units out.  Not a mirror of anything in the reference, which has no such entry point; it is not
registered by install_reference_api().

Per batch: conditioner forward (eval mode) -> MinMaxScaler.inverse_transform of both latent heads (`ops.cols_sub_div`) -> the VAE
decoder (`Engine.generate`), whose last kernel applies tanh, the recon head's GroupNorm and the inverse of `data_scaler` in fp32 and
writes the field straight into the caller's buffer.  The three scalers are anything with `scale_` and `min_` arrays (sklearn's
MinMaxScaler, GpuMinMaxScaler, a namespace); sklearn itself is only needed to unpickle the files `from_files` reads.

Host waits: none between batches.  One in front of the first batch, and only with the image conditioner and conditions that are
already on the device: whether they are in [-1, 1] (the model then maps them to [0, 1]) is read back once, a full pass over
`[P, H*W]` on the caller's stream, instead of once per batch inside the model's forward; host conditions are ranged with numpy and
the parametric conditioner has no such test.  `predict_to_host` adds its one wait at the end.

    s = Surrogate.from_files("model_save", batch=16)
    fields = s.predict(conditions)                 # [P, T, N] fp32 on the device, physical units
    fields = s.predict_to_host(conditions)         # the same in pinned host memory, for P too large for the device
    summary = s.sweep(conditions, probes=[17, 4711])   # extrema per node / per time step, their indices, means, probe histories
                                                   # (DESIGN.md section 17): the fields are reduced by the pass that would store them
    score = s.score(conditions, truth)             # error against held-out fields [P, T, N]: per node / per time step max |e|, bias, MSE,
                                                   # per condition rmse / rel_l2 / max_abs, same fused pass
    ens = s.ensemble(conditions.repeat(1000, 1), limit=250.0, mode="random")   # statistics ACROSS draws per (time step, node): mean,
                                                   # ens.std(), envelope, which draw was worst, how often the limit is exceeded
                                                   # (DESIGN.md section 19); [T, N] running state instead of 1000 fields
    A, B = sobol_design(lo, hi, n=1000)            # two independent sample matrices [n, F] over the parameter ranges
    sens = s.sobol(A, B)                           # which input drives the response, where and when: sens.first_order() and
                                                   # sens.total_order() [F, T, N], Sobol indices by Jansen's estimators (DESIGN.md
                                                   # section 20); (2 + 2 F) running arrays [T, N] instead of n (F + 2) fields
    env = s.ensemble(draws, want=("extrema",), mode="random")       # percentile bands of a Monte-Carlo study in two passes: the
    dist = s.distribution(draws, env, bins=32, mode="random")       # envelope, then a histogram between it per (time step, node);
    p5, p50, p95 = dist.quantile([0.05, 0.5, 0.95])                 # integer counts [bins + 2, T, N] instead of the fields and a
                                                   # sort over them
    fit = s.regress(draws)                         # the linear response surface of the field on the inputs from the draws of such a
    beta, r2 = fit.coefficients(), fit.r2()        # study: coefficients [K, T, N] and the share of the variance they explain, from
                                                   # (2 + K) running arrays [T, N]; fit.covariance() with any scalar per draw
                                                   # (covariates=...)
    W = region_weights(part_of_node, node_weights=nodal_area)      # quantities of interest that are weighted sums over the mesh: the
    qoi = s.project(conditions, W)                 # area-weighted mean over every part, or any rows [R, N] (section forces, modal
    top, when = qoi.peak()                         # amplitudes): qoi.values [P, T, R] from the pass that would store the fields
                                                   # 
    spec = s.temporal(conditions, fourier_rows(T, [f1, f2], dt))   # quantities that are weighted sums over time, per node: Fourier
    amp, phi = spec.amplitude(), spec.phase()      # amplitude and phase at a few frequencies, window means (window_rows), time
                                                   # integrals, filtered values, any rows [R, T]: spec.values [P, R, N], 4 R N bytes
                                                   # per condition instead of 4 T N
    g = s.gram(conditions, node_weights=area)      # the temporal Gram matrix per condition, g.values [P, T, T]: energy histories,
    rows, lam, frac = g.modes(energy=0.99)         # autocorrelation / MAC, and the POD temporal modes of the whole study by
    pod = s.pod(conditions, rank=8, node_weights=area)   # numpy.linalg.eigh on the host; pod() chains gram -> modes -> temporal
                                                   # into a rank-R compression with coefficients [P, R, N]
    dur = s.exceedance(conditions, [allowable, 1.2 * allowable])   # what depends on the ORDER of the time steps: how long each node
    hot = dur.duration(dt), dur.longest_duration(dt)   # stays above a level, when it first crosses and is last above, one long
    node, steps = dur.worst()                      # excursion or many short ones (dur.runs), the accumulated excess: 24 L N bytes
                                                   # per condition instead of 4 T N
    cyc = s.cycles(conditions, gate=0.05 * allowable, exponent=3)   # fatigue and rate questions: the reversals of every node's
    dmg, node = cyc.damage(coefficient=Cf), cyc.worst()[0]   # history behind a hysteresis gate, the ranges between them, sum range^m,
    rate = cyc.peak_rate(dt)                       # the largest rise and fall and when: 40 N bytes per condition
"""
from __future__ import annotations

import contextlib
import inspect
import os
import pickle

import numpy as np

from .engine import (CYCLES_MAX_T, CYCLES_RANGES, CYCLES_RATES, MAX_CYCLES_EXPONENT, DISTRIBUTION_MAX_BINS, DISTRIBUTION_MIN_BINS, ENSEMBLE_GROUPS, ENSEMBLE_MAX_COUNT, EXCEEDANCE_MAX_T, EXCEEDANCE_SIDES, EXCEEDANCE_STATS, LAYOUTS, MAX_LEVELS, MAX_FUNCTIONALS, MAX_GRAM_T, MAX_PROBES, MAX_TEMPORAL, REGRESS_FIELDS, REGRESS_MAX_COVARIATES,
                     SOBOL_FIELDS, SOBOL_MAX_PARAMS, is_tensor_of)
from .engine import SOBOL_MAX_BLOCKS as SOBOL_MAX_COUNT          # base samples of one study

FILES = {"vae": "SimulGen-VAE", "conditioner": "LatentConditioner", "data_scaler": "scaler.pkl",
         "latent_scaler": "latent_vectors_scaler.pkl", "xs_scaler": "xs_scaler.pkl"}      # names the mirrors write under model_save/


def scaler_vectors(scaler, name, length, what):
    """(scale_, min_) of a fitted min-max scaler as float32 numpy vectors of `length` (= `what`) entries; ValueError naming the
    scaler and the first offending index otherwise.  numpy only."""
    try:
        scale, mn = np.asarray(scaler.scale_, np.float64).reshape(-1), np.asarray(scaler.min_, np.float64).reshape(-1)
    except AttributeError:
        raise ValueError(f"{name}: a fitted scaler with scale_ and min_ arrays is required") from None
    if scale.size != length or mn.size != length:
        raise ValueError(f"{name}: scale_ / min_ hold {scale.size} / {mn.size} entries, expected {what} = {length}")
    s32 = scale.astype(np.float32)
    bad = np.flatnonzero(~np.isfinite(s32) | (s32 == 0.0))
    if bad.size:
        raise ValueError(f"{name}: scale_[{int(bad[0])}] = {scale[bad[0]]!r} is zero or not finite (the inverse transform divides by it)")
    bad = np.flatnonzero(~np.isfinite(mn.astype(np.float32)))
    if bad.size:
        raise ValueError(f"{name}: min_[{int(bad[0])}] = {mn[bad[0]]!r} is not finite")
    return s32, mn.astype(np.float32)


@contextlib.contextmanager
def _engine_stream(stream):
    """The handoff of every surrogate call: `stream` (the engine's) waits for the caller's current stream, is the current stream
    inside the block, and the caller's stream waits for it afterwards, unless the two are one."""
    import torch
    cur = torch.cuda.current_stream()
    stream.wait_stream(cur)             # conditions / out may come from the caller's stream
    with torch.cuda.stream(stream):
        yield
    if cur != stream:
        cur.wait_stream(stream)


def _wanted(want, known, unknown, empty):
    """the names of `known` that the tuple `want` holds, in the order of `known`; ValueError(unknown) if it holds another name,
    ValueError(empty) if it holds none"""
    if any(w not in known for w in want):
        raise ValueError(unknown)
    want = tuple(k for k in known if k in want)
    if not want:
        raise ValueError(empty)
    return want


class _Result:
    """a result whose attributes are the names in its FIELDS, given by keyword"""

    def __init__(self, **kw):
        for k in self.FIELDS:
            setattr(self, k, kw[k])


class _StreamResult(_Result):
    """a result that keeps the engine stream (a torch stream): what is derived from its device tensors is computed there"""

    def __init__(self, stream=None, **kw):
        super().__init__(**kw)
        self._stream = stream

    def _on_stream(self, fn):
        with _engine_stream(self._stream) if self._stream is not None else contextlib.nullcontext():
            return fn()


class _RunningResult(_StreamResult):
    """a result whose device tensors (those of its STATE that are not None) ARE the running state of a study over `count` members"""
    PER_COUNT = 1          # values that enter the moments per unit of count

    def state(self):
        """the tensors of the running state by their names in the engine's entry point (Engine.ensemble, Engine.sobol)"""
        return {k: getattr(self, k) for k in self.STATE if getattr(self, k) is not None}

    def _dof(self, what, ddof):
        n = self.PER_COUNT * self.count
        if n - ddof <= 0:
            raise ValueError(f"{what}: {'count' if self.PER_COUNT == 1 else f'{self.PER_COUNT} count'} - ddof = {n} - {ddof} is not positive")
        return n - ddof

    @classmethod
    def require(cls, into):
        """the first check of `into=`, apart from continued(): what a caller compares of the earlier study comes between the two"""
        if not isinstance(into, cls):
            raise ValueError(f"into must be {'an' if cls.__name__[0] in 'AEIOU' else 'a'} {cls.__name__}, not {type(into).__name__}")

    def continued(self, spec):
        """(state(), count) for a call that goes on accumulating into this result, which must hold a contiguous CUDA tensor for
        every name of spec = {name: (shape, dtype)} and a count that is not negative"""
        state = self.state()
        for k, (shape, dtype) in spec.items():
            if not is_tensor_of(state.get(k), dtype, shape):
                raise ValueError(f"into.{k} must be a contiguous {dtype} CUDA tensor of shape {shape}")
        count = int(self.count)
        if count < 0:
            raise ValueError(f"into.count = {count} is negative")
        return state, count


def probe_nodes(nodes, num_node):
    """The probe list of Surrogate.sweep as an int32 vector: a 1-D array of integer dtype with 1 to MAX_PROBES entries, each in
    [0, num_node).  Duplicates are allowed and the order is kept.  ValueError naming the first bad position otherwise.  numpy only."""
    a = np.asarray(nodes)
    if a.ndim != 1:
        raise ValueError(f"probes: a 1-D array of node indices is required, got shape {a.shape}")
    if a.size < 1 or a.size > MAX_PROBES:
        raise ValueError(f"probes: {a.size} entries, between 1 and {MAX_PROBES} are required")
    if not np.issubdtype(a.dtype, np.integer):
        raise ValueError(f"probes: an integer dtype is required, not {a.dtype}")
    bad = np.flatnonzero((a < 0) | (a >= num_node))
    if bad.size:
        raise ValueError(f"probes[{int(bad[0])}] = {int(a[bad[0]])} is outside [0, {int(num_node)})")
    return a.astype(np.int32)


def truth_fields(truth, P, T, N):
    """The held-out fields of Surrogate.score: `truth` as given if it is a float32 array or tensor (host or device) of shape
    [P, T, N]; anything else array-like is looked at through np.asarray.  ValueError naming the offending dimension or the dtype
    otherwise.  numpy only: a tensor is judged by its shape and dtype attributes and not converted."""
    a = truth if hasattr(truth, "shape") and hasattr(truth, "dtype") else np.asarray(truth)
    shape = tuple(int(d) for d in a.shape)
    if len(shape) != 3:
        raise ValueError(f"truth: a [P, T, N] array is required, got shape {shape}")
    for name, got, want in (("P", shape[0], P), ("T", shape[1], T), ("N", shape[2], N)):
        if got != int(want):
            raise ValueError(f"truth: dimension {name} is {got}, expected {name} = {int(want)} (shape {shape}, wanted [P, T, N] = {[int(P), int(T), int(N)]})")
    if str(a.dtype).replace("torch.", "") != "float32":
        raise ValueError(f"truth: dtype float32 is required, not {a.dtype}")
    return a


def functional_weights(weights, num_node):
    """The weight rows of Surrogate.project as contiguous float32 [R, N]: `weights` of shape [R, N], or [N] for a single functional
    (then R = 1), 1 <= R <= MAX_FUNCTIONALS, N = num_node, of a floating dtype.  A CUDA tensor stays on the device and comes back as
    a contiguous float32 CUDA tensor; it is judged by its shape and dtype alone and NOT read back, so its entries are not looked at
    (a non-finite weight then gives non-finite values).  Anything else is looked at through np.asarray and comes back as a numpy
    array, every entry finite as float32.  ValueError naming the problem otherwise: a rank other than 1 or 2, a last dimension other
    than N, R outside its range, a dtype that is not floating, or -- host data -- an entry that is not finite (the first one is
    named).  numpy only for host data."""
    dev = _is_device_tensor(weights)
    a = weights if dev else np.asarray(weights)
    shape = tuple(int(d) for d in a.shape)
    if len(shape) not in (1, 2):
        raise ValueError(f"weights: an [R, N] or [N] array is required, got shape {shape}")
    if shape[-1] != int(num_node):
        raise ValueError(f"weights: the last dimension is {shape[-1]}, expected N = {int(num_node)} (shape {shape})")
    R = shape[0] if len(shape) == 2 else 1
    if R < 1 or R > MAX_FUNCTIONALS:
        raise ValueError(f"weights: R = {R} rows, between 1 and {MAX_FUNCTIONALS} are required (call twice for more)")
    if dev:
        if not a.dtype.is_floating_point:
            raise ValueError(f"weights: a floating dtype is required, not {a.dtype}")
        import torch
        return a.reshape(R, shape[-1]).to(dtype=torch.float32).contiguous()
    if not np.issubdtype(a.dtype, np.floating):
        raise ValueError(f"weights: a floating dtype is required, not {a.dtype}")
    a = a.reshape(R, shape[-1])
    with np.errstate(over="ignore"):          # a value beyond float32 becomes inf and is reported below
        w = np.ascontiguousarray(a, dtype=np.float32)
    bad = np.argwhere(~np.isfinite(w))
    if bad.size:
        r, n = (int(k) for k in bad[0])
        raise ValueError(f"weights[{r}, {n}] = {float(a[r, n])!r} is not finite as float32")
    return w


def region_weights(labels, num_regions=None, node_weights=None, reduce="mean"):
    """The weight rows of the most common functionals, means or sums over parts of the mesh, as float32 [R, N] on the host.
    labels: integer [N], the region of every node, -1 for a node in no region; num_regions: R (default: the largest label + 1);
    node_weights: [N], finite, the weight of every node inside its region -- a nodal area or mass -- default 1; reduce: "sum" (row
    r is node_weights on the nodes of region r and 0 elsewhere) or "mean" (that row divided by its sum, in float64, then rounded to
    float32, so row r gives the weighted mean over region r).  ValueError naming the problem otherwise: labels not 1-D or not of
    integer dtype, a label below -1 or >= num_regions, more than MAX_FUNCTIONALS regions or none, node_weights of another shape or
    with an entry that is not finite, and under "mean" a region without nodes or whose weights sum to zero.  numpy only."""
    if reduce not in ("mean", "sum"):
        raise ValueError(f"reduce must be 'mean' or 'sum', not {reduce!r}")
    lab = np.asarray(labels)
    if lab.ndim != 1:
        raise ValueError(f"labels: a 1-D array of N region labels is required, got shape {lab.shape}")
    if not np.issubdtype(lab.dtype, np.integer):
        raise ValueError(f"labels: an integer dtype is required, not {lab.dtype}")
    N = lab.size
    bad = np.flatnonzero(lab < -1)
    if bad.size:
        raise ValueError(f"labels[{int(bad[0])}] = {int(lab[bad[0]])} is below -1 (-1 means: in no region)")
    R = (int(lab.max()) + 1 if N else 0) if num_regions is None else int(num_regions)
    if R < 1:
        raise ValueError(f"region_weights: {R} regions, at least one is required")
    if R > MAX_FUNCTIONALS:
        raise ValueError(f"region_weights: {R} regions, at most {MAX_FUNCTIONALS} fit one call of project")
    bad = np.flatnonzero(lab >= R)
    if bad.size:
        raise ValueError(f"labels[{int(bad[0])}] = {int(lab[bad[0]])} is outside [-1, num_regions = {R})")
    if node_weights is None:
        nw = np.ones(N, np.float64)
    else:
        nw = np.asarray(node_weights, dtype=np.float64)
        if nw.shape != (N,):
            raise ValueError(f"node_weights: shape {nw.shape}, expected (N,) = {(N,)} as labels")
        bad = np.flatnonzero(~np.isfinite(nw))
        if bad.size:
            raise ValueError(f"node_weights[{int(bad[0])}] = {float(nw[bad[0]])!r} is not finite")
    W = np.zeros((R, N), np.float64)
    inside = np.flatnonzero(lab >= 0)
    W[lab[inside], inside] = nw[inside]
    if reduce == "mean":
        for r in range(R):
            if not np.any(lab == r):
                raise ValueError(f"region {r} has no nodes: its mean is not defined")
            total = W[r].sum()
            if total == 0.0:
                raise ValueError(f"region {r}: its node weights sum to zero, its mean is not defined")
            W[r] /= total
    return W.astype(np.float32)


class ProjectResult(_StreamResult):
    """Surrogate.project's result for P conditions: values [P, T, R] fp32, a device tensor that is the caller's --
    values[p, t, r] = sum over n of weights[r, n] * field[p, t, n], the time histories of R quantities of interest.  What is derived
    from it is computed on the engine stream."""
    FIELDS = ("values",)

    def peak(self):
        """(the maximum over t [P, R] fp32, its time step [P, R] int64); the smallest t on a tie"""
        import torch

        def fn():
            v = self.values
            T = v.shape[1]
            top = v.max(dim=1).values
            steps = torch.arange(T, device=v.device).view(1, T, 1)
            when = torch.where(v == top.unsqueeze(1), steps, T).min(dim=1).values
            return top, when
        return self._on_stream(fn)

    def time_integral(self, dt=1.0):
        """the trapezoid rule over t at spacing dt, summed in float64: [P, R] fp32 (zero for a single time step)"""
        def fn():
            v = self.values.double()
            return ((v[:, 1:] + v[:, :-1]).sum(dim=1) * (float(dt) / 2.0)).float()
        return self._on_stream(fn)


def temporal_weights(weights, T):
    """The weight rows of Surrogate.temporal as contiguous float32 [R, T]: `weights` of shape [R, T], or [T] for a single functional
    (then R = 1), 1 <= R <= MAX_TEMPORAL, T = num_time, of a floating dtype.  A CUDA tensor stays on the device and comes back as a
    contiguous float32 CUDA tensor; it is judged by its shape and dtype alone and NOT read back, so its entries are not looked at (a
    non-finite weight then gives non-finite values).  Anything else is looked at through np.asarray and comes back as a numpy array,
    every entry finite as float32.  ValueError naming the problem otherwise: a rank other than 1 or 2, a last dimension other than
    T, R outside its range, a dtype that is not floating, or -- host data -- an entry that is not finite (the first one is named by
    row and time step).  numpy only for host data."""
    dev = _is_device_tensor(weights)
    a = weights if dev else np.asarray(weights)
    shape = tuple(int(d) for d in a.shape)
    if len(shape) not in (1, 2):
        raise ValueError(f"weights: an [R, T] or [T] array is required, got shape {shape}")
    if shape[-1] != int(T):
        raise ValueError(f"weights: the last dimension is {shape[-1]}, expected T = {int(T)} (shape {shape})")
    R = shape[0] if len(shape) == 2 else 1
    if R < 1 or R > MAX_TEMPORAL:
        raise ValueError(f"weights: R = {R} rows, between 1 and {MAX_TEMPORAL} are required (call twice for more)")
    if dev:
        if not a.dtype.is_floating_point:
            raise ValueError(f"weights: a floating dtype is required, not {a.dtype}")
        import torch
        return a.reshape(R, shape[-1]).to(dtype=torch.float32).contiguous()
    if not np.issubdtype(a.dtype, np.floating):
        raise ValueError(f"weights: a floating dtype is required, not {a.dtype}")
    a = a.reshape(R, shape[-1])
    with np.errstate(over="ignore"):          # a value beyond float32 becomes inf and is reported below
        w = np.ascontiguousarray(a, dtype=np.float32)
    bad = np.argwhere(~np.isfinite(w))
    if bad.size:
        r, t = (int(k) for k in bad[0])
        raise ValueError(f"weights: row {r} is not finite as float32 at time step {t}: weights[{r}, {t}] = {float(a[r, t])!r}")
    return w


def fourier_rows(T, freqs, dt=1.0, window=None):
    """The weight rows of Fourier amplitudes at a few frequencies, float32 [2 F, T] on the host: for frequency f (in cycles per unit
    of dt, 0 <= f <= 1 / (2 dt)) row 2 i is c w[t] cos(2 pi f t dt) and row 2 i + 1 is c w[t] sin(2 pi f t dt), w the window
    (default: all ones) and c = 2 / sum(w), or 1 / sum(w) where the sine row vanishes (f = 0, and the Nyquist frequency of an even
    T): a sinusoid A cos(2 pi f t dt - phi) at an exact bin frequency f = k / (T dt) then gives (A cos phi, A sin phi), so
    TemporalResult.amplitude() is A and .phase() is phi.  window: an optional taper of length T, finite, with a non-zero sum; it
    is folded into the rows and the rows are renormalised by its sum, so the amplitude of a bin-centred sinusoid is still A (under
    a taper the neighbouring bins leak into it as they do into any windowed transform).  Computed in float64 and rounded to
    float32 once.  ValueError naming the problem otherwise: T < 1, no frequency or more than MAX_TEMPORAL / 2, a frequency that is
    not finite, negative or above Nyquist, dt that is not positive and finite, a window of another shape, with an entry that is not
    finite, or whose sum is zero.  numpy only."""
    T = int(T)
    if T < 1:
        raise ValueError(f"fourier_rows: T = {T}, at least one time step is required")
    dt = float(dt)
    if not (np.isfinite(dt) and dt > 0.0):
        raise ValueError(f"fourier_rows: dt = {dt!r} must be positive and finite")
    f = np.atleast_1d(np.asarray(freqs, dtype=np.float64))
    if f.ndim != 1 or f.size < 1:
        raise ValueError(f"fourier_rows: a list of frequencies is required, got shape {f.shape}")
    if 2 * f.size > MAX_TEMPORAL:
        raise ValueError(f"fourier_rows: {f.size} frequencies give {2 * f.size} rows, at most {MAX_TEMPORAL} fit one call of temporal")
    nyq = 0.5 / dt
    for i, fi in enumerate(f):
        if not np.isfinite(fi) or fi < 0.0 or fi > nyq * (1.0 + 1e-12):
            raise ValueError(f"fourier_rows: freqs[{i}] = {float(fi)!r} is outside [0, 1 / (2 dt) = {nyq!r}]")
    if window is None:
        w = np.ones(T, np.float64)
    else:
        w = np.asarray(window, dtype=np.float64)
        if w.shape != (T,):
            raise ValueError(f"fourier_rows: window has shape {w.shape}, expected (T,) = {(T,)}")
        bad = np.flatnonzero(~np.isfinite(w))
        if bad.size:
            raise ValueError(f"fourier_rows: window[{int(bad[0])}] = {float(w[bad[0]])!r} is not finite")
    total = w.sum()
    if total == 0.0:
        raise ValueError("fourier_rows: the window sums to zero, the rows cannot be normalised")
    steps = np.arange(T, dtype=np.float64)
    rows = np.empty((2 * f.size, T), np.float64)
    for i, fi in enumerate(f):
        cyc = fi * dt * steps          # cycles at every time step; reduced mod 1 in float64 before the 2 pi, exact at bin frequencies of moderate T
        ang = 2.0 * np.pi * (cyc - np.floor(cyc))
        s = np.sin(ang)
        alone = not np.any(np.abs(s) > 1e-9)          # f = 0 or Nyquist on the grid: the cosine row carries the whole amplitude
        c = (1.0 if alone else 2.0) / total
        rows[2 * i] = c * w * np.cos(ang)
        rows[2 * i + 1] = 0.0 if alone else c * w * s
    return rows.astype(np.float32)


def window_rows(T, edges):
    """The weight rows of means over time windows, float32 [len(edges) - 1, T] on the host: row i is 1 / (edges[i + 1] - edges[i])
    on the time steps edges[i] : edges[i + 1] and 0 elsewhere, so every row sums to 1 -- a coarse time history, or with two edges
    the mean over one window.  edges: integers, strictly increasing, within [0, T].  ValueError naming the problem otherwise: T < 1,
    edges not 1-D, not of integer dtype, fewer than two, more than MAX_TEMPORAL + 1, outside [0, T] or not strictly increasing (the
    first offending edge is named).  numpy only."""
    T = int(T)
    if T < 1:
        raise ValueError(f"window_rows: T = {T}, at least one time step is required")
    e = np.asarray(edges)
    if e.ndim != 1:
        raise ValueError(f"window_rows: edges must be a 1-D array, got shape {e.shape}")
    if not np.issubdtype(e.dtype, np.integer):
        raise ValueError(f"window_rows: edges must be of an integer dtype, not {e.dtype}")
    if e.size < 2:
        raise ValueError(f"window_rows: {e.size} edges, at least two are required")
    if e.size - 1 > MAX_TEMPORAL:
        raise ValueError(f"window_rows: {e.size - 1} windows, at most {MAX_TEMPORAL} fit one call of temporal")
    for i, v in enumerate(e):
        if v < 0 or v > T:
            raise ValueError(f"window_rows: edges[{i}] = {int(v)} is outside [0, T = {T}]")
        if i and v <= e[i - 1]:
            raise ValueError(f"window_rows: edges[{i}] = {int(v)} is not above edges[{i - 1}] = {int(e[i - 1])}: strictly increasing edges are required")
    rows = np.zeros((e.size - 1, T), np.float64)
    for i in range(e.size - 1):
        rows[i, int(e[i]):int(e[i + 1])] = 1.0 / float(int(e[i + 1]) - int(e[i]))
    return rows.astype(np.float32)


class TemporalResult(_StreamResult):
    """Surrogate.temporal's result for P conditions: values [P, R, N] fp32, a device tensor that is the caller's --
    values[p, r, n] = sum over t of weights[r, t] * field[p, t, n], R fields of quantities over time.  What is derived from it is
    computed on the engine stream."""
    FIELDS = ("values",)

    def _pairs(self):
        v = self.values
        if v.shape[1] % 2:
            raise ValueError(f"the rows are taken as consecutive (cos, sin) pairs (fourier_rows): R = {v.shape[1]} is odd")
        return v[:, 0::2], v[:, 1::2]

    def amplitude(self):
        """hypot(cos row, sin row) of every consecutive pair of rows: [P, R / 2, N] fp32; ValueError for an odd R"""
        def fn():
            c, s = self._pairs()
            return c.hypot(s)
        return self._on_stream(fn)

    def phase(self):
        """atan2(sin row, cos row) of every consecutive pair of rows, in (-pi, pi]: [P, R / 2, N] fp32 -- phi of A cos(w t - phi)
        under fourier_rows; ValueError for an odd R"""
        def fn():
            c, s = self._pairs()
            return s.atan2(c)
        return self._on_stream(fn)

    def peak(self):
        """(the node of the largest |value| [P, R] int64, that value with its sign [P, R] fp32); the smallest node on a tie"""
        import torch

        def fn():
            v = self.values
            N = v.shape[2]
            mag = v.abs()
            top = mag.max(dim=2).values
            nodes = torch.arange(N, device=v.device).view(1, 1, N)
            where = torch.where(mag == top.unsqueeze(2), nodes, N).min(dim=2).values
            return where, v.gather(2, where.clamp(max=N - 1).unsqueeze(2)).squeeze(2)
        return self._on_stream(fn)


def _gram_vector(v, N, name, nonneg):
    if v is None:
        return None
    dev = _is_device_tensor(v)
    a = v if dev else np.asarray(v)
    shape = tuple(int(d) for d in a.shape)
    if shape != (int(N),):
        raise ValueError(f"{name}: an [N] array with N = {int(N)} is required, got shape {shape}")
    if dev:
        if not a.dtype.is_floating_point:
            raise ValueError(f"{name}: a floating dtype is required, not {a.dtype}")
        import torch
        w = a.to(dtype=torch.float32).contiguous()
        if not bool(torch.isfinite(w).all()):
            raise ValueError(f"{name}: an entry is not finite as float32")
        if nonneg and bool((w < 0).any()):
            raise ValueError(f"{name}: an entry is negative; the weights of a Gram matrix are non-negative")
        return w
    if not np.issubdtype(a.dtype, np.floating):
        raise ValueError(f"{name}: a floating dtype is required, not {a.dtype}")
    with np.errstate(over="ignore"):          # a value beyond float32 becomes inf and is reported below
        w = np.ascontiguousarray(a, dtype=np.float32)
    bad = np.flatnonzero(~np.isfinite(w))
    if bad.size:
        raise ValueError(f"{name}[{int(bad[0])}] = {float(a[bad[0]])!r} is not finite as float32")
    if nonneg:
        bad = np.flatnonzero(w < 0)
        if bad.size:
            raise ValueError(f"{name}[{int(bad[0])}] = {float(a[bad[0]])!r} is negative; the weights of a Gram matrix are non-negative")
    return w


def gram_weights(node_weights, N):
    """The node weights of Surrogate.gram (a nodal mass or area) as contiguous float32 [N], or None for None (every weight 1).  A
    host array comes back as a numpy array, a CUDA tensor as a CUDA tensor; both are read: every entry finite as float32 and
    >= 0 (a CUDA tensor costs one host wait for that).  ValueError naming the problem otherwise: a shape other than [N], a dtype
    that is not floating, an entry that is not finite or negative (host data: the first one is named)."""
    return _gram_vector(node_weights, N, "node_weights", True)


def gram_offset(offset, N):
    """The reference field of Surrogate.gram (what is subtracted from every time step: a mean field, an initial state) as contiguous
    float32 [N], or None for None (no offset).  As gram_weights, without the sign condition."""
    return _gram_vector(offset, N, "offset", False)


def _host64(v):
    return (v.detach().cpu().numpy() if hasattr(v, "detach") else np.asarray(v)).astype(np.float64)


class GramResult(_StreamResult):
    """Surrogate.gram's result for P conditions: values [P, T, T] fp32, a device tensor that is the caller's --
    values[p, t, t'] = sum over n of w[n] (field[p, t, n] - m[n]) (field[p, t', n] - m[n]), bitwise symmetric -- and num_node = N.
    What is derived from it is computed on the host in float64 (numpy; the first call waits for the device and keeps the copy)."""
    FIELDS = ("values", "num_node")

    def __init__(self, **kw):
        super().__init__(**kw)
        self._g64 = None

    def host(self):
        """values as float64 [P, T, T] on the host"""
        if self._g64 is None:
            if self._stream is not None:
                self._stream.synchronize()
            self._g64 = _host64(self.values)
        return self._g64

    def energy(self):
        """[P, T]: the diagonal, the weighted energy of every time step about the offset"""
        return np.diagonal(self.host(), axis1=1, axis2=2).copy()

    def total(self):
        """[T, T]: the sum over the conditions, X X^T of the stacked snapshot matrix of the whole study"""
        return self.host().sum(axis=0)

    def correlation(self):
        """[P, T, T]: values[p, t, t'] / sqrt(values[p, t, t] values[p, t', t']), the temporal autocorrelation (squared: the MAC
        matrix between time steps); 0 where a diagonal entry is 0"""
        g = self.host()
        d = np.sqrt(np.clip(self.energy(), 0.0, None))
        den = d[:, :, None] * d[:, None, :]
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(den > 0, g / den, 0.0)

    def centered(self):
        """[P, T, T]: H G H with H = I - 1 1^T / T, the Gram matrix of the field minus its own mean over time"""
        g = self.host()
        T = g.shape[-1]
        H = np.eye(T) - np.full((T, T), 1.0 / T)
        return H @ g @ H

    def noise_floor(self):
        """(N + 3) 2^-24 trace(total()): for w >= 0 an upper bound of the Frobenius norm of the rounding error of total() -- every
        entry is within (N + 3) 2^-24 sum_n |w d_t d_t'| of the exact sum and Cauchy-Schwarz bounds that by the geometric mean of
        the two diagonal entries -- and by Weyl's inequality of the error of each of its eigenvalues"""
        return (int(self.num_node) + 3) * 2.0 ** -24 * float(np.trace(self.total()))

    def modes(self, rank=None, energy=None):
        """The POD temporal modes of the study (method of snapshots): eigh of total(), eigenvalues descending, negative ones clamped
        to 0, truncated to `rank` modes or to the smallest rank whose eigenvalues reach the fraction `energy` of their sum (give one
        of the two, or neither for all T).  Returns (rows [R, T] float32 -- orthonormal, ready for Surrogate.temporal --,
        eigenvalues [R] float64, the fraction of the energy they capture)."""
        if rank is not None and energy is not None:
            raise ValueError("modes: give rank or energy, not both")
        lam, vec = np.linalg.eigh(self.total())
        order = np.argsort(lam)[::-1]
        lam, vec = np.clip(lam[order], 0.0, None), vec[:, order]
        T = lam.size
        whole = float(lam.sum())
        if rank is not None:
            R = int(rank)
            if R < 1 or R > T:
                raise ValueError(f"modes: rank = {rank} is outside [1, T = {T}]")
        elif energy is not None:
            f = float(energy)
            if not (0.0 < f <= 1.0):
                raise ValueError(f"modes: energy = {energy!r} is outside (0, 1]")
            cum = np.cumsum(lam)
            R = T if whole == 0.0 else min(T, int(np.searchsorted(cum, f * whole * (1.0 - 1e-15))) + 1)
        else:
            R = T
        frac = 1.0 if whole == 0.0 else float(lam[:R].sum() / whole)
        return np.ascontiguousarray(vec[:, :R].T, dtype=np.float32), lam[:R].copy(), frac


class PodResult(_Result):
    """Surrogate.pod's result: rows [R, T] float32 (the temporal modes, host), eigenvalues [R] float64, fraction (of the energy the
    modes capture), coefficients [P, R, N] fp32 -- coefficients[p, r, n] = sum_t rows[r, t] (field[p, t, n] - m[n]), a device
    tensor that is the caller's -- and offset (m as float32 [N], or None)."""
    FIELDS = ("rows", "eigenvalues", "fraction", "coefficients", "offset")

    def reconstruct(self, p):
        """rows^T coefficients[p] + offset: the rank-R field of condition p, [T, N] float64, where the coefficients live"""
        c = self.coefficients[p]
        if hasattr(c, "detach"):
            import torch
            rows = torch.as_tensor(np.asarray(self.rows, np.float64), device=c.device)
            x = rows.t() @ c.to(torch.float64)
            if self.offset is not None:
                x += torch.as_tensor(self.offset, device=c.device).to(torch.float64)
            return x
        x = np.asarray(self.rows, np.float64).T @ np.asarray(c, np.float64)
        return x if self.offset is None else x + np.asarray(self.offset, np.float64)


def exceedance_levels(levels, N):
    """The levels of Surrogate.exceedance as contiguous float32 [L, N] in physical units, 1 <= L <= MAX_LEVELS: a scalar is one
    level for every node, a 1-D array of L entries is L levels, each broadcast over the nodes, an [L, N] array is taken node by
    node.  A CUDA tensor stays on the device and comes back as a contiguous float32 CUDA tensor; it is judged by its shape and
    dtype alone and NOT read back, so its entries are not looked at (nothing exceeds a NaN level).  Anything else is looked at
    through np.asarray and comes back as a numpy array, every entry finite as float32.  ValueError naming the problem otherwise:
    a rank above 2, a last dimension of an [L, N] array other than N, L outside its range, or -- host data -- an entry that is not
    finite (the first one is named).  numpy only for host data."""
    N = int(N)
    dev = _is_device_tensor(levels)
    a = levels if dev else np.asarray(levels, dtype=np.float64)
    shape = tuple(int(d) for d in a.shape)
    if len(shape) > 2:
        raise ValueError(f"levels: a scalar, an [L] vector or an [L, N] array is required, got shape {shape}")
    if len(shape) == 2 and shape[1] != N:
        raise ValueError(f"levels: the last dimension is {shape[1]}, expected N = {N} (shape {shape})")
    L = shape[0] if shape else 1
    if L < 1 or L > MAX_LEVELS:
        raise ValueError(f"levels: L = {L} levels, between 1 and {MAX_LEVELS} are required (call again for more"
                         + (f"; an [L] vector is L levels for every node, one level per node is [1, N] = [1, {N}])" if len(shape) == 1 else ")"))
    if dev:
        if not a.dtype.is_floating_point:
            raise ValueError(f"levels: a floating dtype is required, not {a.dtype}")
        import torch
        return a.to(dtype=torch.float32).reshape(L, -1).expand(L, N).contiguous()
    with np.errstate(over="ignore"):          # a value beyond float32 becomes inf and is reported below
        v = a.astype(np.float32).reshape(L, -1)
    bad = np.argwhere(~np.isfinite(v))
    if bad.size:
        l, n = (int(k) for k in bad[0])
        where = "levels" if not shape else f"levels[{l}]" if len(shape) == 1 else f"levels[{l}, {n}]"
        raise ValueError(f"{where} = {float(a.reshape(L, -1)[l, n])!r} is not finite as float32")
    return np.array(np.broadcast_to(v, (L, N)), order="C")          # a copy: the broadcast view is read-only


class ExceedanceResult(_StreamResult):
    """Surrogate.exceedance's result for P conditions against L levels: the level-crossing statistics of every node's T time steps,
    device tensors that are the caller's.  A step exceeds its level when the field is strictly above it (side "above") or below it
    ("below").  stats int32 [P, 5, L, N] with the views count (the steps that exceed), first and last (their smallest and largest
    time step, -1 if none), longest (the longest run of consecutive exceeding steps, 0 if none) and runs (the number of such
    maximal runs), each [P, L, N]; excess fp32 [P, L, N], the sum over the exceeding steps of field - level (level - field below),
    exactly 0 where nothing exceeds; levels fp32 [L, N] as they were used.  An output that was not asked for is None and its
    methods raise ValueError.  What is derived is plain torch on the small result, computed on the engine stream."""
    FIELDS = ("stats", "excess", "levels", "side", "T")

    def _plane(self, name):
        if self.stats is None:
            raise ValueError(f"{name}: the step statistics were not asked for (want=(\"steps\", ...))")
        return self.stats[:, EXCEEDANCE_STATS.index(name)]

    count = property(lambda self: self._plane("count"))
    first = property(lambda self: self._plane("first"))
    last = property(lambda self: self._plane("last"))
    longest = property(lambda self: self._plane("longest"))
    runs = property(lambda self: self._plane("runs"))

    def _excess(self, what):
        if self.excess is None:
            raise ValueError(f"{what}: the excess was not asked for (want=(..., \"excess\"))")
        return self.excess

    def ever(self):
        """count > 0: bool [P, L, N], whether the node exceeds the level at any time step"""
        return self._on_stream(lambda: self.count > 0)

    def fraction(self):
        """count / T: fp32 [P, L, N], the share of the time steps that exceed"""
        return self._on_stream(lambda: self.count.float() / float(self.T))

    def duration(self, dt=1.0):
        """count * dt: fp32 [P, L, N], the total time beyond the level"""
        return self._on_stream(lambda: self.count.float() * float(dt))

    def longest_duration(self, dt=1.0):
        """longest * dt: fp32 [P, L, N], the length of the longest uninterrupted excursion"""
        return self._on_stream(lambda: self.longest.float() * float(dt))

    def first_time(self, dt=1.0):
        """first * dt, NaN where the node never exceeds: fp32 [P, L, N]"""
        def fn():
            f = self.first
            return (f.float() * float(dt)).masked_fill(f < 0, float("nan"))
        return self._on_stream(fn)

    def excess_integral(self, dt=1.0):
        """excess * dt: fp32 [P, L, N], the rectangle-rule integral over time of the part of the field beyond the level"""
        return self._on_stream(lambda: self._excess("excess_integral") * float(dt))

    def mean_excess(self):
        """excess / count, 0 where count = 0: fp32 [P, L, N], how far beyond the level the node is while it exceeds"""
        def fn():
            c = self.count
            return (self._excess("mean_excess") / c.clamp(min=1).float()).masked_fill(c == 0, 0.0)
        return self._on_stream(fn)

    def worst(self):
        """(the node with the largest count [P, L] int64, that count [P, L] int32); the smallest node on a tie"""
        import torch

        def fn():
            c = self.count
            N = c.shape[2]
            top = c.max(dim=2).values
            nodes = torch.arange(N, device=c.device).view(1, 1, N)
            return torch.where(c == top.unsqueeze(2), nodes, N).min(dim=2).values, top
        return self._on_stream(fn)


def cycles_gate(gate, N):
    """The hysteresis gate of Surrogate.cycles as contiguous float32 [N] in physical units: a scalar is one gate for every node, an
    [N] array is taken node by node.  A CUDA tensor stays on the device and comes back as a contiguous float32 CUDA tensor; it is
    judged by its shape and dtype alone and NOT read back (a negative or NaN gate on the device is the caller's).  Anything else
    is looked at through np.asarray and comes back as a numpy array, every entry >= 0 as float32 and not NaN (inf is allowed:
    nothing turns).  ValueError naming the problem otherwise: a shape other than () or [N], or -- host data -- a negative or NaN
    entry (the first one is named).  numpy only for host data."""
    N = int(N)
    dev = _is_device_tensor(gate)
    a = gate if dev else np.asarray(gate, dtype=np.float64)
    shape = tuple(int(d) for d in a.shape)
    if shape not in ((), (N,)):
        raise ValueError(f"gate: a scalar or an [N] = [{N}] vector is required, got shape {shape}")
    if dev:
        if not a.dtype.is_floating_point:
            raise ValueError(f"gate: a floating dtype is required, not {a.dtype}")
        import torch
        return a.to(dtype=torch.float32).reshape(-1).expand(N).contiguous()
    with np.errstate(over="ignore"):
        v = a.astype(np.float32).reshape(-1)
    bad = np.flatnonzero(~(v >= 0))          # a NaN fails the comparison too
    if bad.size:
        n = int(bad[0])
        where = f"gate[{n}]" if shape else "gate"
        raise ValueError(f"{where} = {float(a.reshape(-1)[n])!r} is not a gate: a value >= 0 is required")
    return np.array(np.broadcast_to(v, (N,)), order="C")          # a copy: the broadcast view is read-only


class CyclesResult(_StreamResult):
    """Surrogate.cycles' result for P conditions: the load cycles and the rates of every node's T time steps, device tensors that are
    the caller's.  The turns (ASTM E1049 simple-range counting behind the hysteresis gate): reversals int32 [P, N], the confirmed
    turning points, and ranges fp32 [P, 4, N] with the views range_sum, range_max, damage_sum (the sum of range^exponent over the
    counted ranges) and open (the unfinished excursion at the end), each [P, N].  The rates: rate_when int32 [P, 2, N] with the views
    rise_when, fall_when (-1 at T = 1) and rates fp32 [P, 3, N] with the views rise, fall (the largest and the smallest first
    difference) and path (the sum of their magnitudes).  gate fp32 [N] as it was used, exponent, T.  A group that was not asked for
    is None and its methods raise ValueError.  What is derived is plain torch on the small result, computed on the engine stream."""
    FIELDS = ("reversals", "ranges", "rate_when", "rates", "gate", "exponent", "T")

    def _turns(self, name):
        if self.ranges is None:
            raise ValueError(f"{name}: the turns were not asked for (want=(\"turns\", ...))")
        return self.ranges[:, CYCLES_RANGES.index(name)] if name in CYCLES_RANGES else self.reversals

    def _rates(self, name):
        if self.rates is None:
            raise ValueError(f"{name}: the rates were not asked for (want=(..., \"rates\"))")
        return self.rates[:, CYCLES_RATES.index(name)] if name in CYCLES_RATES else self.rate_when[:, ("rise_when", "fall_when").index(name)]

    range_sum = property(lambda self: self._turns("range_sum"))
    range_max = property(lambda self: self._turns("range_max"))
    damage_sum = property(lambda self: self._turns("damage"))
    open = property(lambda self: self._turns("open"))
    rise = property(lambda self: self._rates("rise"))
    fall = property(lambda self: self._rates("fall"))
    path = property(lambda self: self._rates("path"))
    rise_when = property(lambda self: self._rates("rise_when"))
    fall_when = property(lambda self: self._rates("fall_when"))

    def half_cycles(self):
        """max(reversals - 1, 0): int32 [P, N], the number of counted ranges (half cycles)"""
        return self._on_stream(lambda: (self._turns("half_cycles") - 1).clamp(min=0))

    def mean_range(self):
        """range_sum / half_cycles, 0 where no range is counted: fp32 [P, N]"""
        def fn():
            k = (self._turns("mean_range") - 1).clamp(min=0)
            return (self.range_sum / k.clamp(min=1).float()).masked_fill(k == 0, 0.0)
        return self._on_stream(fn)

    def damage(self, coefficient=1.0, include_open=True):
        """0.5 (damage_sum + open^exponent) / coefficient: fp32 [P, N], Miner's sum for an S-N curve N(R) = coefficient / R^exponent,
        every counted range half a cycle; include_open counts the unfinished excursion at the end as one more half cycle"""
        def fn():
            d = self._turns("damage")
            if include_open:
                d = d + self.open ** int(self.exponent)
            return d * (0.5 / float(coefficient))
        return self._on_stream(fn)

    def peak_rate(self, dt=1.0):
        """max(|rise|, |fall|) / dt: fp32 [P, N], the largest rate of change in either direction"""
        return self._on_stream(lambda: self._rates("rise").abs().maximum(self.fall.abs()) / float(dt))

    def _time(self, name, dt):
        def fn():
            w = self._rates(name)
            return (w.float() * float(dt)).masked_fill(w < 0, float("nan"))
        return self._on_stream(fn)

    def rise_time(self, dt=1.0):
        """rise_when * dt, NaN at T = 1: fp32 [P, N], the end of the step with the largest rise"""
        return self._time("rise_when", dt)

    def fall_time(self, dt=1.0):
        """fall_when * dt, NaN at T = 1: fp32 [P, N], the end of the step with the largest fall"""
        return self._time("fall_when", dt)

    def path_length(self):
        """path: fp32 [P, N], the total variation of the node's history"""
        return self._on_stream(lambda: self._rates("path"))

    def worst(self, coefficient=1.0, include_open=True):
        """(the node with the largest damage(coefficient, include_open) [P] int64, that damage [P] fp32); the smallest node on a tie"""
        import torch

        def fn():
            d = self.damage(coefficient, include_open)
            N = d.shape[1]
            top = d.max(dim=1).values
            nodes = torch.arange(N, device=d.device).view(1, N)
            return torch.where(d == top.unsqueeze(1), nodes, N).min(dim=1).values, top
        return self._on_stream(fn)


class ScoreResult(_Result):
    """Surrogate.score's result for P conditions, device tensors; e = predicted field - truth.  node_max_abs / node_bias / node_mse
    [P, N] fp32 (max over time of |e|, mean of e, mean of e^2 per node) and t_worst [P, N] int32 (the time step of the largest |e|);
    frame_max_abs / frame_mse / frame_truth_ms [P, T] fp32 (max over the mesh of |e|, mean of e^2, mean of truth^2 per time step)
    and n_worst [P, T] int32 (the node of the largest |e|); per condition rmse = sqrt(mean_t frame_mse) and
    rel_l2 = sqrt(sum_t frame_mse / sum_t frame_truth_ms) [P] fp64 (inf / nan for a zero truth, as the division says) and
    max_abs = max_t frame_max_abs [P] fp32."""
    FIELDS = ("node_max_abs", "node_bias", "node_mse", "t_worst", "frame_max_abs", "frame_mse", "frame_truth_ms", "n_worst",
              "rmse", "rel_l2", "max_abs")


def exceed_limit(limit, N):
    """The limit of Surrogate.ensemble as a float32 vector of N entries in physical units: a scalar is broadcast to every node, a
    1-D array of N entries is taken node by node.  ValueError naming the problem otherwise: a rank above 1, a length other than N,
    or an entry that is not finite (the first one is named).  numpy only."""
    a = np.asarray(limit, dtype=np.float64)
    if a.ndim > 1:
        raise ValueError(f"limit: a scalar or a 1-D array of N = {int(N)} entries is required, got shape {a.shape}")
    if a.ndim == 1 and a.size != int(N):
        raise ValueError(f"limit: {a.size} entries, expected N = {int(N)} (or a scalar)")
    with np.errstate(over="ignore"):          # a value beyond float32 becomes inf and is reported below
        v = np.broadcast_to(a.astype(np.float32), (int(N),))
    bad = np.flatnonzero(~np.isfinite(v))
    if bad.size:
        where = f"limit[{int(bad[0])}]" if a.ndim == 1 else "limit"
        raise ValueError(f"{where} = {float(a.reshape(-1)[bad[0] if a.ndim == 1 else 0])!r} is not finite as float32")
    return np.array(v)          # a copy: the broadcast view is read-only


class EnsembleResult(_RunningResult):
    """Surrogate.ensemble's result: statistics over `count` members per (time step, node), device tensors [T, N] that ARE the running
    state (pass the result back as `into=` to go on accumulating).  mean, m2 fp32 (Welford: m2 is the sum of squared deviations
    from the mean); max, min fp32 with arg_max, arg_min int32 (the index, in call order, of the condition that produced the
    extremum; the earliest on a tie); exceed int32 (members with field > limit, strict) with limit fp32 [N].  Groups not asked for
    are None."""
    FIELDS = ("count", "mean", "m2", "max", "min", "arg_max", "arg_min", "exceed", "limit")
    GROUPS = ENSEMBLE_GROUPS
    STATE = tuple(k for names in ENSEMBLE_GROUPS.values() for k in names)

    def groups(self):
        """the groups this result holds, in the order of GROUPS"""
        return tuple(g for g, names in self.GROUPS.items() if getattr(self, names[0]) is not None)

    def var(self, ddof=0):
        """m2 / (count - ddof) [T, N] fp32"""
        if self.m2 is None:
            raise ValueError("var: the moments were not asked for")
        dof = self._dof("var", ddof)
        return self._on_stream(lambda: self.m2 / float(dof))

    def std(self, ddof=0):
        """sqrt(var(ddof))"""
        if self.m2 is None:
            raise ValueError("std: the moments were not asked for")
        dof = self._dof("std", ddof)
        return self._on_stream(lambda: (self.m2 / float(dof)).sqrt())

    def exceed_fraction(self):
        """exceed / count [T, N] fp32: how often the limit is exceeded"""
        if self.exceed is None:
            raise ValueError("exceed_fraction: no limit was given")
        if self.count < 1:
            raise ValueError("exceed_fraction: the ensemble is empty")
        return self._on_stream(lambda: self.exceed.float() / float(self.count))


def _is_device_tensor(v):
    """a CUDA tensor, judged by its attributes alone (numpy only: torch is not imported for the question)"""
    return hasattr(v, "data_ptr") and getattr(getattr(v, "device", None), "type", None) == "cuda"


def hist_range(range, T, N):
    """The bounds of Surrogate.distribution as (lo, hi), each [T, N] float32 in physical units.  `range` is an EnsembleResult that
    holds the extrema (its min and max tensors are returned as they are), or a pair (lo, hi) of scalars (every time step and
    node), of 1-D arrays of N entries (node by node, every time step) or of [T, N] arrays -- host forms, which come back as new
    numpy arrays -- or a pair of float32 CUDA tensors [T, N], which are returned as they are after a look at shape and dtype
    (their values are not read).  ValueError naming the problem otherwise: not a pair, a rank above 2 or a length other than N /
    a shape other than [T, N], an entry that is not finite as float32, or hi < lo (the first offender is named).  numpy only."""
    T, N = int(T), int(N)
    if isinstance(range, EnsembleResult):
        if range.min is None or range.max is None:
            raise ValueError("range: the EnsembleResult does not hold the extrema (want=('extrema',))")
        pair, names = (range.min, range.max), ("range.min", "range.max")
    else:
        if not isinstance(range, (tuple, list)) or len(range) != 2:
            raise ValueError("range: an EnsembleResult with the extrema or a pair (lo, hi) is required")
        pair, names = tuple(range), ("lo", "hi")
    if any(_is_device_tensor(v) for v in pair):
        for name, v in zip(names, pair):
            if not _is_device_tensor(v):
                raise ValueError(f"range: {name} is not a CUDA tensor, but the other bound is one")
            shape = tuple(int(d) for d in v.shape)
            if shape != (T, N):
                raise ValueError(f"range: {name} has shape {shape}, expected [T, N] = {[T, N]}")
            if str(v.dtype).replace("torch.", "") != "float32":
                raise ValueError(f"range: {name}: dtype float32 is required, not {v.dtype}")
            if hasattr(v, "is_contiguous") and not v.is_contiguous():
                raise ValueError(f"range: {name} must be contiguous")
        return pair
    out = []
    for name, v in zip(names, pair):
        a = np.asarray(v, dtype=np.float64)
        if a.ndim > 2:
            raise ValueError(f"range: {name}: a scalar, a 1-D array of N = {N} entries or a [T, N] = {[T, N]} array is required, got shape {a.shape}")
        if a.ndim == 1 and a.size != N:
            raise ValueError(f"range: {name}: {a.size} entries, expected N = {N} (or a scalar, or [T, N])")
        if a.ndim == 2 and a.shape != (T, N):
            raise ValueError(f"range: {name} has shape {a.shape}, expected [T, N] = {[T, N]}")
        with np.errstate(over="ignore"):          # a value beyond float32 becomes inf and is reported below
            v32 = np.broadcast_to(a.astype(np.float32), (T, N))
        bad = np.argwhere(~np.isfinite(v32))
        if bad.size:
            i = tuple(int(k) for k in bad[0])
            where = {0: name, 1: f"{name}[{i[1]}]", 2: f"{name}[{i[0]}, {i[1]}]"}[a.ndim]
            raise ValueError(f"range: {where} = {float(np.broadcast_to(a, (T, N))[i])!r} is not finite as float32")
        out.append(np.array(v32, order="C"))          # a dense copy: the broadcast view is read-only and has strides of 0
    lo, hi = out
    bad = np.argwhere(hi < lo)
    if bad.size:
        t, n = (int(k) for k in bad[0])
        raise ValueError(f"range: hi < lo at [t, n] = [{t}, {n}]: lo = {float(lo[t, n])!r}, hi = {float(hi[t, n])!r}")
    return lo, hi


def quantile_rank(q, count):
    """r = max(ceil(q count), 1): the q-quantile of `count` values is the r-th smallest (the empirical distribution function's
    inverse), 0 < q <= 1"""
    return max(int(np.ceil(np.float64(q) * int(count))), 1)


class DistributionResult(_RunningResult):
    """Surrogate.distribution's result: the histogram of `count` members per (time step, node) in `bins` uniform bins between lo and
    hi, device tensors.  counts int32 [bins + 2, T, N] IS the running state (pass the result back as `into=` to go on counting):
    row 0 the members below lo, rows 1 .. bins the bins, row bins + 1 the members above hi; every column sums to count.  lo, hi
    fp32 [T, N] are the bounds the call was given (the tensors of the EnsembleResult, if it was one)."""
    FIELDS = ("count", "bins", "lo", "hi", "counts")
    STATE = ("lo", "hi", "counts")
    CHUNK = 1 << 26          # elements of counts quantile() looks at in one piece: its temporaries take a few times 4 bytes each

    @property
    def under(self):
        """counts[0] [T, N] int32 (a view): members below lo"""
        return self.counts[0]

    @property
    def over(self):
        """counts[bins + 1] [T, N] int32 (a view): members above hi"""
        return self.counts[self.bins + 1]

    def fractions(self):
        """counts[1 : bins + 1] / count [bins, T, N] fp32: the share of the members in each bin"""
        if self.count < 1:
            raise ValueError("fractions: the distribution is empty")
        return self._on_stream(lambda: self.counts[1:self.bins + 1].float() / float(self.count))

    def quantile(self, q):
        """The q-quantile per (time step, node), fp32 [T, N] for a scalar q and [Q, T, N] for a sequence, 0 < q <= 1: with
        r = max(ceil(q count), 1) and j the first row of counts at which the running sum over the rows reaches r, lo for j = 0, hi
        for j = bins + 1 and otherwise lo + (j - 1 + (r - sum below row j) / counts[j]) (hi - lo) / bins, never above hi -- the r-th
        smallest member is in bin j, and the members of a bin are taken as evenly spread over it, so the result is within one bin
        width (hi - lo) / bins of that member.  Computed on the engine stream in torch, in pieces along T of at most CHUNK counts."""
        if self.count < 1:
            raise ValueError("quantile: the distribution is empty")
        qs = np.asarray(q, dtype=np.float64)
        if qs.ndim > 1 or qs.size < 1:
            raise ValueError(f"quantile: q must be a scalar or a non-empty 1-D sequence, got shape {qs.shape}")
        bad = np.flatnonzero(~((qs.reshape(-1) > 0.0) & (qs.reshape(-1) <= 1.0)))
        if bad.size:
            raise ValueError(f"quantile: q = {float(qs.reshape(-1)[bad[0]])!r} is outside (0, 1]")
        ranks = [quantile_rank(v, self.count) for v in qs.reshape(-1)]
        K = int(self.bins)

        def run():
            import torch
            T, N = self.lo.shape
            out = torch.empty((len(ranks), T, N), dtype=torch.float32, device=self.lo.device)
            step = max(1, self.CHUNK // ((K + 2) * N))
            fK = torch.full((), float(K), dtype=torch.float32, device=self.lo.device)          # a tensor: a true division, not a product with 1 / K
            for t0 in range(0, T, step):
                c = self.counts[:, t0:t0 + step]
                lo, hi = self.lo[t0:t0 + step], self.hi[t0:t0 + step]
                cum = c.cumsum(0, dtype=torch.int32)          # at most 2^24 members
                for i, r in enumerate(ranks):
                    j = (cum < r).sum(0).clamp_(max=K + 1)    # the first row whose running sum reaches r
                    below = torch.where(j > 0, cum.gather(0, (j - 1).clamp_(min=0)[None])[0], 0)
                    inside = c.gather(0, j[None])[0]
                    pos = (j - 1).float() + (r - below).float() / inside.float()
                    v = torch.minimum(lo + pos * (hi - lo) / fK, hi)
                    out[i, t0:t0 + step] = torch.where(j == 0, lo, torch.where(j == K + 1, hi, v))
            return out
        res = self._on_stream(run)
        return res[0] if qs.ndim == 0 else res

    def median(self):
        """quantile(0.5)"""
        return self.quantile(0.5)


def regression_covariates(covariates, P):
    """The covariates of Surrogate.regress as a float64 array [P, K]: one row per member, 1 <= K <= REGRESS_MAX_COVARIATES columns,
    every entry finite.  ValueError naming the problem otherwise: a rank other than 2, a number of rows other than P, K outside its
    range, or an entry that is not finite (the first one is named).  numpy only."""
    a = np.asarray(covariates, dtype=np.float64)
    if a.ndim != 2:
        raise ValueError(f"covariates: a [P, K] array is required, got shape {a.shape}")
    if a.shape[0] != int(P):
        raise ValueError(f"covariates: {a.shape[0]} rows, expected P = {int(P)} (one per condition)")
    if a.shape[1] < 1 or a.shape[1] > REGRESS_MAX_COVARIATES:
        raise ValueError(f"covariates: K = {a.shape[1]} columns, between 1 and {REGRESS_MAX_COVARIATES} are required")
    bad = np.argwhere(~np.isfinite(a))
    if bad.size:
        m, i = (int(k) for k in bad[0])
        raise ValueError(f"covariates[{m}, {i}] = {float(a[m, i])!r} is not finite")
    return a


def regression_weights(Y, mean=None, gram=None, count=0):
    """The host half of the regression pass, float64 and sequential: for member m of Y [P, K], k = count + m + 1,
        ybar_new = ybar + (y_m - ybar) / k;   w[m] = float32(y_m - ybar_new);   S = S + outer(y_m - ybar, y_m - ybar_new)
    -> (w float32 [P, K], ybar [K], S [K, K]).  w holds the covariates centred on the running mean that includes the member, which
    is what the kernel multiplies with the field's deviation from the mean before the member (the updating identity of the
    co-moment); S is the centred Gram matrix of the covariates, sum (y - ybar)(y - ybar)^T.  mean / gram: the ybar and S of the
    `count` members before these (None: zeros); the arguments are left alone.  Member by member, so any cut of Y into calls gives the
    same bits.  numpy only."""
    Y = np.asarray(Y, dtype=np.float64)
    if Y.ndim != 2:
        raise ValueError(f"regression_weights: Y must be [P, K], got shape {Y.shape}")
    K = Y.shape[1]
    ybar = np.zeros(K) if mean is None else np.array(mean, dtype=np.float64)
    S = np.zeros((K, K)) if gram is None else np.array(gram, dtype=np.float64)
    if ybar.shape != (K,) or S.shape != (K, K) or int(count) < 0:
        raise ValueError(f"regression_weights: mean {ybar.shape} / gram {S.shape} / count {count} do not fit K = {K} covariates")
    w = np.empty(Y.shape, np.float32)
    for m in range(Y.shape[0]):
        before = Y[m] - ybar
        ybar = ybar + before / float(int(count) + m + 1)
        after = Y[m] - ybar
        w[m] = after
        S = S + np.outer(before, after)
    return w, ybar, S


class RegressionResult(_RunningResult):
    """Surrogate.regress's result: the linear response surface of the field on K covariates over `count` members per (time step,
    node).  mean, m2 fp32 [T, N] (Welford, as EnsembleResult's) and comoment fp32 [K, T, N], sum (x - xbar)(y_i - ybar_i), are device
    tensors that ARE the running state (pass the result back as `into=` to go on accumulating); cov_mean [K] and cov_gram [K, K],
    float64 numpy arrays, are the mean and the centred Gram matrix sum (y - ybar)(y - ybar)^T of the covariates, kept on the host."""
    FIELDS = ("count", "mean", "m2", "comoment", "cov_mean", "cov_gram")
    STATE = REGRESS_FIELDS

    @property
    def n_cov(self):
        return int(self.comoment.shape[0])

    def var(self, ddof=0):
        """m2 / (count - ddof) [T, N] fp32"""
        dof = self._dof("var", ddof)
        return self._on_stream(lambda: self.m2 / float(dof))

    def std(self, ddof=0):
        """sqrt(var(ddof))"""
        dof = self._dof("std", ddof)
        return self._on_stream(lambda: (self.m2 / float(dof)).sqrt())

    def covariance(self, ddof=0):
        """comoment / (count - ddof) [K, T, N] fp32: the covariance of the field with each covariate"""
        dof = self._dof("covariance", ddof)
        return self._on_stream(lambda: self.comoment / float(dof))

    def _host(self, a, shape):
        import torch
        return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(self.comoment.device).reshape(shape)

    def correlation(self):
        """comoment_i / sqrt(m2 gram_ii) [K, T, N] fp32: Pearson's correlation of the field with each covariate; NaN or inf where
        the field or the covariate does not vary, as the division says"""
        diag = np.diag(np.asarray(self.cov_gram, np.float64))
        return self._on_stream(lambda: self.comoment / (self.m2[None] * self._host(diag, (-1, 1, 1))).sqrt())

    def gram_inverse(self):
        """The inverse of cov_gram [K, K], float64 on the host, through the unit-diagonal (correlation) form of the matrix.
        ValueError where the regression is not determined: count <= K, a covariate that does not vary (it is named), or a
        unit-diagonal Gram matrix that numpy.linalg.matrix_rank (default tolerance) finds rank-deficient."""
        K = self.n_cov
        G = np.asarray(self.cov_gram, np.float64)
        if self.count <= K:
            raise ValueError(f"coefficients: count = {self.count} members do not determine {K} coefficients and an intercept (count > K is required)")
        diag = np.diag(G)
        flat = np.flatnonzero(~(diag > 0.0))
        if flat.size:
            raise ValueError(f"coefficients: covariate {int(flat[0])} does not vary (gram[{int(flat[0])}, {int(flat[0])}] = {float(diag[flat[0]])!r})")
        s = 1.0 / np.sqrt(diag)
        R = G * s[:, None] * s[None, :]
        rank = int(np.linalg.matrix_rank(R))
        if rank < K:
            raise ValueError(f"coefficients: the covariates are linearly dependent (rank {rank} of {K})")
        return np.linalg.inv(R) * s[:, None] * s[None, :]

    def coefficients(self):
        """beta = gram^-1 comoment [K, T, N] fp32: the regression coefficients of the field on the covariates (with an intercept),
        per unit of each covariate.  The inverse is taken in float64 on the host (gram_inverse, which raises where the design is
        singular) and applied in fp32 on the engine stream."""
        ginv = self.gram_inverse()
        K = self.n_cov
        return self._on_stream(lambda: (self._host(ginv, (K, K)) @ self.comoment.reshape(K, -1)).reshape(self.comoment.shape))

    def intercept(self):
        """mean - sum_i beta_i cov_mean_i [T, N] fp32: the response surface is intercept + sum_i beta_i y_i"""
        beta = self.coefficients()
        return self._on_stream(lambda: self.mean - (self._host(self.cov_mean, (1, -1)) @ beta.reshape(self.n_cov, -1)).reshape(self.mean.shape))

    def r2(self):
        """sum_i beta_i comoment_i / m2 [T, N] fp32: the share of the variance over the members that the linear surface explains;
        NaN or inf where the field does not vary, as the division says"""
        beta = self.coefficients()
        return self._on_stream(lambda: (beta * self.comoment).sum(0) / self.m2)


def sobol_groups(groups, F):
    """The parameters of Surrogate.sobol as a list of d int64 index vectors into the F columns of a condition.  None: one parameter
    per column (d = F).  Otherwise a sequence of d non-empty 1-D integer index lists, each entry in [0, F); a column may appear in
    several groups (overlapping groups are allowed) and the order is kept.  ValueError naming the first bad group or index
    otherwise, and for d > SOBOL_MAX_PARAMS.  numpy only."""
    F = int(F)
    if groups is None:
        groups = [[c] for c in range(F)]
    try:
        groups = list(groups)
    except TypeError:
        raise ValueError(f"groups: a sequence of index lists is required, not {type(groups).__name__}") from None
    if len(groups) < 1:
        raise ValueError("groups: at least one group is required")
    if len(groups) > SOBOL_MAX_PARAMS:
        raise ValueError(f"groups: {len(groups)} groups, at most {SOBOL_MAX_PARAMS} parameters are supported")
    res = []
    for i, g in enumerate(groups):
        a = np.asarray(g)
        if a.ndim != 1 or a.size < 1:
            raise ValueError(f"groups[{i}]: a non-empty 1-D list of column indices is required, got shape {a.shape}")
        if not np.issubdtype(a.dtype, np.integer):
            raise ValueError(f"groups[{i}]: an integer dtype is required, not {a.dtype}")
        bad = np.flatnonzero((a < 0) | (a >= F))
        if bad.size:
            raise ValueError(f"groups[{i}][{int(bad[0])}] = {int(a[bad[0]])} is outside [0, {F})")
        res.append(a.astype(np.int64))
    return res


def sobol_design(lo, hi, n, seed=0):
    """Two independent sample matrices A, B [n, F] float32 for Surrogate.sobol, uniform in [lo[c], hi[c]] per column, from
    np.random.default_rng(seed) (A is drawn first).  ValueError for bounds of different lengths or not 1-D, a bound that is not
    finite (the first one is named), hi < lo, or n < 1.  numpy only."""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    if lo.ndim != 1 or hi.ndim != 1 or lo.size != hi.size or lo.size < 1:
        raise ValueError(f"sobol_design: lo and hi must be 1-D and of one length >= 1, got shapes {lo.shape} and {hi.shape}")
    for name, v in (("lo", lo), ("hi", hi)):
        bad = np.flatnonzero(~np.isfinite(v))
        if bad.size:
            raise ValueError(f"sobol_design: {name}[{int(bad[0])}] = {float(v[bad[0]])!r} is not finite")
    bad = np.flatnonzero(hi < lo)
    if bad.size:
        raise ValueError(f"sobol_design: hi[{int(bad[0])}] = {float(hi[bad[0]])!r} is below lo[{int(bad[0])}] = {float(lo[bad[0]])!r}")
    if int(n) != n or int(n) < 1:
        raise ValueError(f"sobol_design: n = {n!r}, at least one base sample is required")
    rng = np.random.default_rng(seed)
    A, B = (lo + (hi - lo) * rng.random((int(n), lo.size)) for _ in range(2))
    return A.astype(np.float32), B.astype(np.float32)


def sobol_members(A, B, groups):
    """The member matrix of a Sobol study, [n (d + 2), F] float32: base sample j yields the block A_j, B_j, AB_1_j .. AB_d_j, where
    AB_i_j is A_j with the columns of groups[i] (sobol_groups) taken from B_j.  What Surrogate.sobol builds on the device batch by
    batch; predict() on this matrix gives the fields the study reduces.  numpy only."""
    A, B = np.asarray(A, np.float32), np.asarray(B, np.float32)
    if A.ndim != 2 or A.shape != B.shape:
        raise ValueError(f"A and B must be [n, F] and of one shape, got {A.shape} and {B.shape}")
    groups = sobol_groups(groups, A.shape[1])
    M = np.repeat(A[:, None, :], len(groups) + 2, axis=1)
    M[:, 1] = B
    for i, g in enumerate(groups):
        M[:, 2 + i, g] = B[:, g]
    return np.ascontiguousarray(M.reshape(-1, A.shape[1]))


class SobolResult(_RunningResult):
    """Surrogate.sobol's result: the running sums of a Sobol sensitivity study over `count` base samples and `n_params` parameters,
    device tensors that ARE the running state (pass the result back as `into=` to go on accumulating).  mean, m2 fp32 [T, N]:
    Welford over the 2 count values of the A and B members; first_sq, total_sq fp32 [n_params, T, N]: sum_j (f(B_j) - f(AB_i_j))^2
    and sum_j (f(A_j) - f(AB_i_j))^2 (Jansen's estimators); one not asked for is None."""
    FIELDS = ("count", "n_params", "mean", "m2", "first_sq", "total_sq")
    PARTS = {"first": "first_sq", "total": "total_sq"}
    STATE = SOBOL_FIELDS
    PER_COUNT = 2

    def want(self):
        """the parts this result holds, in the order of PARTS"""
        return tuple(w for w, k in self.PARTS.items() if getattr(self, k) is not None)

    def var(self, ddof=0):
        """m2 / (2 count - ddof) [T, N] fp32: the variance of the response over the A and B samples"""
        dof = self._dof("var", ddof)
        return self._on_stream(lambda: self.m2 / float(dof))

    def first_order(self):
        """S_i = 1 - first_sq[i] / (2 count var) [n_params, T, N] fp32: the share of the variance parameter i explains on its own.
        Where the variance is 0 the result is inf or nan, as the division says."""
        if self.first_sq is None:
            raise ValueError("first_order: 'first' was not asked for")
        if self.count < 1:
            raise ValueError("first_order: the study is empty")
        return self._on_stream(lambda: 1.0 - self.first_sq / (float(2 * self.count) * (self.m2 / float(2 * self.count))))

    def total_order(self):
        """ST_i = total_sq[i] / (2 count var) [n_params, T, N] fp32: the share of the variance that involves parameter i at all
        (its own effect and every interaction).  Where the variance is 0 the result is inf or nan, as the division says."""
        if self.total_sq is None:
            raise ValueError("total_order: 'total' was not asked for")
        if self.count < 1:
            raise ValueError("total_order: the study is empty")
        return self._on_stream(lambda: self.total_sq / (float(2 * self.count) * (self.m2 / float(2 * self.count))))


class SweepResult(_Result):
    """Surrogate.sweep's result for P conditions, device tensors: node_max / node_min / node_mean [P, N] fp32 and t_max / t_min
    [P, N] int32 (extrema over time per node, the time step of each, the mean over time); frame_max / frame_min [P, T] fp32 and
    n_max / n_min [P, T] int32 (extrema over the mesh per time step and their node); probes [P, T, K] fp32 or None."""
    FIELDS = ("node_max", "node_min", "node_mean", "t_max", "t_min", "frame_max", "frame_min", "n_max", "n_min", "probes")


class Surrogate:
    def __init__(self, vae, conditioner, latent_scaler, xs_scaler, data_scaler, batch=16, seed=0):
        """vae: the mirror VAE; conditioner: LatentConditionerImg or the parametric LatentConditioner (put in eval mode);
        scalers: duck-typed (scale_, min_).  The engine runs at max_batch = batch and is seeded with `seed`.
        The engine is the VAE object's own, shared with everything else that uses that object: constructing a Surrogate re-seeds
        it (sgv_seed: the noise position goes back to 0), which changes the noise of any later training or sampling on the same
        VAE.  If the VAE rebuilds its engine later (a call with a larger batch), the next predict picks the new engine up and
        seeds it again with `seed`."""
        cfg = vae.cfg
        self.batch = int(batch)
        if self.batch < 1:
            raise ValueError(f"batch must be >= 1, not {batch}")
        self.size2, self.hier = int(conditioner.size2), int(conditioner.latent_dim)
        self.latent_end = int(conditioner.latent_dim_end)
        vecs = [scaler_vectors(latent_scaler, "latent_scaler", self.latent_end, "latent_dim_end"),
                scaler_vectors(xs_scaler, "xs_scaler", self.size2 * self.hier, "size2 * latent_dim"),
                scaler_vectors(data_scaler, "data_scaler", cfg.num_node, "num_node")]
        n_kl = len(cfg.num_filter_enc) - 1
        if self.latent_end != cfg.latent_dim or self.hier != cfg.hierarchical_dim or self.size2 != n_kl:
            raise ValueError(f"the conditioner predicts latents of ({self.latent_end}, {self.size2} x {self.hier}), the VAE decodes "
                             f"({cfg.latent_dim}, {n_kl} x {cfg.hierarchical_dim})")
        import torch
        self.torch = torch
        self.vae, self.conditioner = vae, conditioner.eval()
        self.N, self.T = cfg.num_node, cfg.num_time
        self.seed = int(seed)
        # whether the conditioner's forward can be told the input range instead of reading the batch's minimum back (image model)
        try:
            self._takes_remap = "remap" in inspect.signature(getattr(conditioner, "forward", conditioner)).parameters
        except (TypeError, ValueError):
            self._takes_remap = False
        self.eng = None
        self._engine()
        # the six vectors, uploaded once
        (self.lat_scale, self.lat_min), (self.xs_scale, self.xs_min), (self.data_scale, self.data_min) = (
            tuple(torch.from_numpy(a).cuda() for a in pair) for pair in vecs)

    def _engine(self):
        """the VAE's engine at max_batch >= batch; a new engine object (first use, or rebuilt by the VAE) is seeded and its streams wrapped"""
        eng = self.vae._eng(self.batch)
        if eng is not self.eng:
            t = self.torch
            self.eng = eng
            eng.seed(self.seed)
            self._stream = t.cuda.ExternalStream(eng.stream) if eng.stream else t.cuda.default_stream()
            self._copy_stream = None
        return eng

    @classmethod
    def from_files(cls, model_dir="model_save", **kw):
        """The files a training run of the mirrors leaves in `model_dir`; FileNotFoundError names the first one missing."""
        paths = {k: os.path.join(model_dir, v) for k, v in FILES.items()}
        for p in paths.values():
            if not os.path.exists(p):
                raise FileNotFoundError(f"Surrogate.from_files: {p} not found")
        import torch
        vae = torch.load(paths["vae"], map_location="cpu", weights_only=False)
        loaded = {}
        for k in ("conditioner", "latent_scaler", "xs_scaler", "data_scaler"):
            with open(paths[k], "rb") as f:
                loaded[k] = pickle.load(f)
        return cls(vae, loaded["conditioner"], loaded["latent_scaler"], loaded["xs_scaler"], loaded["data_scaler"], **kw)

    # ---- one batch: conditions [b, F] -> the decoder's latents (z [b, latent], xs [n_levels - 1, b, hier]) on the engine stream ----
    def _latents(self, cond, remap):
        from . import ops
        y = self.conditioner(cond, remap=remap) if self._takes_remap else self.conditioner(cond)
        y1, y2 = (y["latent_main"], y["xs"]) if isinstance(y, dict) else y          # a conditioner built with return_dict=True
        b = y1.shape[0]
        lat = ops.cols_sub_div(y1.contiguous(), self.lat_min, self.lat_scale)
        xs = ops.cols_sub_div(y2.reshape(b, -1).contiguous(), self.xs_min, self.xs_scale)
        # list order of ReconstructionEvaluator._reconstruct_from_latents: xs_list[k] = columns k*d .. (k+1)*d
        return lat, xs.view(b, self.size2, self.hier).transpose(0, 1).contiguous()

    # ... -> the field, written into `dst` ([b, T, N] or [b, N, T])
    def _generate(self, cond, dst, layout, fix, remap):
        lat, xs = self._latents(cond, remap)
        self.eng.generate(lat, xs, self.data_scale, self.data_min, out=dst, layout=layout, fix=fix)

    def _args(self, conditions, layout, mode):
        t = self.torch
        if layout not in LAYOUTS:
            raise ValueError(f"layout must be one of {sorted(LAYOUTS)}, not {layout!r}")
        if mode not in ("fix", "random"):
            raise ValueError(f"mode must be 'fix' or 'random', not {mode!r}")
        if not t.is_tensor(conditions):
            conditions = t.from_numpy(np.ascontiguousarray(conditions, dtype=np.float32))
        if conditions.dim() != 2:
            raise ValueError(f"conditions must be [P, F], got {tuple(conditions.shape)}")
        P = conditions.shape[0]
        shape = (P, self.T, self.N) if layout == "TN" else (P, self.N, self.T)
        # the image model maps inputs in [-1, 1] to [0, 1] when a batch's minimum is below -0.1, which it reads back per call;
        # decided here once for all of `conditions` instead (host data: no device involved; device data: one read, before
        # anything is enqueued), so that no batch makes the host wait for the stream
        remap = bool(P > 0 and float(conditions.min()) < -0.1) if self._takes_remap else None
        self._engine()
        return conditions, P, shape, remap

    def _batch(self, conditions, lo, hi):
        return conditions[lo:hi].to(device="cuda", dtype=self.torch.float32, non_blocking=True)

    @staticmethod
    def _batches(P, step):
        """(lo, hi) of the batches of `step` that P rows fall into; the last one may be ragged"""
        for lo in range(0, P, step):
            yield lo, min(P, lo + step)

    def _latent_batches(self, conditions, P, remap):
        """(lo, hi, lat, xs) batch by batch: rows lo .. hi of `conditions` and the decoder's latents for them"""
        for lo, hi in self._batches(P, self.batch):
            yield (lo, hi) + self._latents(self._batch(conditions, lo, hi), remap)

    def _condition_batches(self, conditions, P, remap):
        """_latent_batches for a pass that draws its noise per call (project, temporal, gram, exceedance, cycles): every batch draws from the
        streams of the call's first draw, condition p from their row p (Engine.set_draw_row) -- the noise one batch over all
        conditions would get, so the batch size does not show in the bits and the draw position ends where one call leaves it.
        The training state is read when the first batch is asked for.  The row is back at 0 once the generator is closed: callers wrap it in contextlib.closing, so that an exception in their
        loop body resets it at once."""
        eng = self.eng
        at = eng.train_state()
        try:
            for lo, hi, lat, xs in self._latent_batches(conditions, P, remap):
                eng.set_train_state(at["step"], at["seed"], at["draw"])
                eng.set_draw_row(lo)
                yield lo, hi, lat, xs
        finally:
            eng.set_draw_row(0)

    def _to_device(self, v, align16):
        """a validated host array or tensor on the device (None stays None), uploaded on the current stream.  align16: cloned when it
        is a view at an odd offset, for a kernel that loads 16 bytes at a time"""
        if v is None:
            return None
        t = self.torch
        if not t.is_tensor(v):
            v = t.from_numpy(v)
        v = v.to(device="cuda", non_blocking=True)
        return v.clone() if align16 and v.data_ptr() % 16 else v

    def predict(self, conditions, out=None, layout="TN", mode="fix"):
        """conditions [P, F] (host array or CUDA tensor, preprocessed as the conditioner's training set holds them) -> fp32 device
        tensor [P, T, N] (layout "TN") or [P, N, T] ("NT") in physical units.  mode "fix": the mean (the reference's "fix": the
        latents' noise times 1e-10, so bitwise-equal results need the same seed and call sequence); "random": sampled.
        Nothing makes the host wait between batches; with the image conditioner the input range is decided once for all of
        `conditions` in front of the first batch (see _args: for a CUDA tensor that is one device-to-host read), not per batch as
        the model's own forward does.  Host conditions in pageable memory are uploaded
        batch by batch with blocking copies; pass a pinned or a CUDA tensor to keep the host ahead."""
        t = self.torch
        conditions, P, shape, remap = self._args(conditions, layout, mode)
        if out is None:
            out = t.empty(shape, dtype=t.float32, device="cuda")
        elif not is_tensor_of(out, t.float32, shape):
            raise ValueError(f"out must be a contiguous float32 CUDA tensor of shape {shape}")
        with _engine_stream(self._stream):
            for lo, hi in self._batches(P, self.batch):
                self._generate(self._batch(conditions, lo, hi), out[lo:hi], layout, mode == "fix", remap)
        return out

    def sweep(self, conditions, probes=None, mode="fix"):
        """What a design study keeps of predict(conditions), without the fields: a SweepResult of device tensors -- per condition
        and node the extrema over time, when they happen and the mean; per condition and time step the extrema over the mesh and
        where they are; with `probes` (node indices, see probe_nodes) the time histories there.  The recon head's last pass reduces
        the values predict() would store (bit for bit the same, ties to the smallest index), so 20 N + 16 T bytes per condition
        leave the decoder instead of 4 T N.  Batching, streams, the single input-range decision and `mode` are predict()'s: no
        host wait between batches; the engine writes per-batch buffers and the copies into the [P, ...] results run on its stream."""
        t = self.torch
        conditions, P, _, remap = self._args(conditions, "TN", mode)
        want = ("node", "frame") + (("probes",) if probes is not None else ())
        if probes is not None:
            self.eng.set_probes(probe_nodes(probes, self.N))
        K = self.eng.n_probes if probes is not None else 0
        f32 = dict(dtype=t.float32, device="cuda")
        i32 = dict(dtype=t.int32, device="cuda")
        node, when = t.empty((3, P, self.N), **f32), t.empty((2, P, self.N), **i32)          # the results: the caller's stream owns them
        frame, where = t.empty((2, P, self.T), **f32), t.empty((2, P, self.T), **i32)
        hist = t.empty((P, self.T, K), **f32) if probes is not None else None
        with _engine_stream(self._stream):
            b0 = min(self.batch, max(P, 1))
            buf = dict(node_stats=t.empty((b0, 3, self.N), **f32), node_when=t.empty((b0, 2, self.N), **i32),
                       frame_stats=t.empty((b0, self.T, 2), **f32), frame_where=t.empty((b0, self.T, 2), **i32))
            for lo, hi, lat, xs in self._latent_batches(conditions, P, remap):
                out = {k: v[:hi - lo] for k, v in buf.items()}
                if hist is not None:
                    out["probes"] = hist[lo:hi]                  # [b, T, K] is the result's own layout: written in place
                self.eng.summarize(lat, xs, self.data_scale, self.data_min, fix=mode == "fix", want=want, out=out)
                node[:, lo:hi].copy_(out["node_stats"].transpose(0, 1))
                when[:, lo:hi].copy_(out["node_when"].transpose(0, 1))
                frame[:, lo:hi].copy_(out["frame_stats"].permute(2, 0, 1))
                where[:, lo:hi].copy_(out["frame_where"].permute(2, 0, 1))
        return SweepResult(node_max=node[0], node_min=node[1], node_mean=node[2], t_max=when[0], t_min=when[1],
                           frame_max=frame[0], frame_min=frame[1], n_max=where[0], n_min=where[1], probes=hist)

    def project(self, conditions, weights, mode="fix"):
        """Quantities of interest of predict(conditions) that are weighted sums over the mesh, without the fields: weights [R, N] or
        [N] (see functional_weights; region_weights builds the rows of means or sums over parts) -> a ProjectResult whose values
        [P, T, R] are sum_n weights[r, n] * field[p, t, n] -- resultant forces, weighted means, interpolated sensors, modal
        amplitudes.  The recon head's last pass multiplies the values predict() would store (bit for bit the same) into the weight
        rows on the matrix cores, fp32, in a fixed order inside fixed shares of the mesh, and adds the shares in float64: a value
        depends on its condition, time step and weight row alone, and the decoder's noise of condition p is row p of the streams
        one call over all conditions would draw from (Engine.set_draw_row; mode "fix" scales the noise by 1e-10, it does not remove
        it), so the batch size does not show in the bits in either mode, and 4 T R bytes per condition leave the decoder instead
        of 4 T N.  The weights are uploaded once per call and every batch is written straight
        into its rows of `values`.  Batching, streams, the single input-range decision and `mode` are sweep()'s: no host wait between
        batches.  values[:, t, :] is a [P, R] array of scalars per draw: what regress(covariates=...) takes."""
        t = self.torch
        conditions, P, _, remap = self._args(conditions, "TN", mode)
        w = functional_weights(weights, self.N)
        values = t.empty((P, self.T, w.shape[0]), dtype=t.float32, device="cuda")          # the result: the caller's stream owns it
        with _engine_stream(self._stream), contextlib.closing(self._condition_batches(conditions, P, remap)) as batches:
            w = self._to_device(w, align16=True)
            for lo, hi, lat, xs in batches:
                self.eng.project(lat, xs, self.data_scale, self.data_min, w, fix=mode == "fix", out=values[lo:hi])
        return ProjectResult(stream=self._stream, values=values)

    def temporal(self, conditions, weights, mode="fix"):
        """Quantities of predict(conditions) that are weighted sums over time, per node, without the fields: weights [R, T] or [T]
        (see temporal_weights; fourier_rows builds the rows of Fourier amplitudes, window_rows those of window means) -> a
        TemporalResult whose values [P, R, N] are sum_t weights[r, t] * field[p, t, n] -- spectral amplitudes, window means, time
        integrals, filtered values, amplitudes on temporal modes.  The recon head's last pass multiplies the values predict() would
        store (bit for bit the same) into the weight rows on the matrix cores, one fp32 fused multiply-add chain per value over t
        ascending: a value depends on its condition, weight row and node alone, and the decoder's noise is placed as in
        project() (_condition_batches), so the batch size does not show in the bits in either mode, and 4 R N bytes per condition
        leave the decoder instead of 4 T N.  The weights are uploaded once per
        call and every batch is written straight into its rows of `values`.  Batching, streams, the single input-range decision and
        `mode` are project()'s: no host wait between batches."""
        t = self.torch
        conditions, P, _, remap = self._args(conditions, "TN", mode)
        w = temporal_weights(weights, self.T)
        values = t.empty((P, w.shape[0], self.N), dtype=t.float32, device="cuda")          # the result: the caller's stream owns it
        with _engine_stream(self._stream), contextlib.closing(self._condition_batches(conditions, P, remap)) as batches:
            w = self._to_device(w, align16=False)
            for lo, hi, lat, xs in batches:
                self.eng.temporal(lat, xs, self.data_scale, self.data_min, w, fix=mode == "fix", out=values[lo:hi])
        return TemporalResult(stream=self._stream, values=values)

    def gram(self, conditions, node_weights=None, offset=None, mode="fix"):
        """The temporal Gram matrix of predict(conditions) per condition, without the fields: a GramResult whose values [P, T, T] are
        sum_n w[n] (field[p, t, n] - m[n]) (field[p, t', n] - m[n]), with node_weights w [N] (a nodal mass or area; see
        gram_weights) and offset m [N] (a reference field; see gram_offset), either None -- energy histories, autocorrelation and
        MAC between time steps, and, summed over the conditions, X X^T of the study, whose eigenvectors are its POD temporal modes
        (GramResult.modes).  num_time <= MAX_GRAM_T.  The recon head's last pass multiplies the values predict() would store (bit
        for bit the same) with themselves on the matrix cores in fp32, in a fixed order inside fixed shares of the mesh, and adds
        the shares in float64: a matrix depends on its condition alone, and the decoder's noise is placed as in project()
        (_condition_batches), so the batch size does not show in the bits in either mode, and 4 T T bytes per condition leave the
        decoder instead of 4 T N.  Batching, streams, the single
        input-range decision and `mode` are project()'s: no host wait between batches."""
        t = self.torch
        conditions, P, _, remap = self._args(conditions, "TN", mode)
        if self.T > MAX_GRAM_T:
            raise ValueError(f"gram: num_time = {self.T} is beyond the limit of {MAX_GRAM_T} time steps")
        w, m = gram_weights(node_weights, self.N), gram_offset(offset, self.N)
        values = t.empty((P, self.T, self.T), dtype=t.float32, device="cuda")          # the result: the caller's stream owns it
        with _engine_stream(self._stream), contextlib.closing(self._condition_batches(conditions, P, remap)) as batches:
            w, m = (self._to_device(v, align16=True) for v in (w, m))
            for lo, hi, lat, xs in batches:
                self.eng.gram(lat, xs, self.data_scale, self.data_min, node_weights=w, offset=m, fix=mode == "fix", out=values[lo:hi])
        return GramResult(stream=self._stream, values=values, num_node=self.N)

    def pod(self, conditions, rank=None, energy=None, node_weights=None, offset=None, mode="fix"):
        """A rank-R compression of predict(conditions) by the method of snapshots, the fields never stored: gram() gives the Gram
        matrices, GramResult.modes(rank, energy) the temporal modes rows [R, T] of the whole study, and temporal() the coefficients
        coefficients[p, r, n] = sum_t rows[r, t] (field[p, t, n] - m[n]), formed on the device in fp32 as temporal(rows)[p, r, n]
        - S_r m[n] with S_r = sum_t rows[r, t].  Every pass starts from the same draw position, so all of them see the same fields
        in either mode; the position ends where one pass leaves it.  More than MAX_TEMPORAL modes take several temporal passes.
        Returns a PodResult; PodResult.reconstruct(p) is rows^T coefficients[p] + m.  One host wait, for the Gram matrices."""
        t = self.torch
        eng = self.eng
        at = eng.train_state()
        g = self.gram(conditions, node_weights=node_weights, offset=offset, mode=mode)
        rows, lam, frac = g.modes(rank=rank, energy=energy)
        m = gram_offset(offset, self.N)
        parts = []
        for lo in range(0, rows.shape[0], MAX_TEMPORAL):
            eng.set_train_state(at["step"], at["seed"], at["draw"])
            parts.append(self.temporal(conditions, rows[lo:lo + MAX_TEMPORAL], mode=mode).values)
        with _engine_stream(self._stream):
            coeff = parts[0] if len(parts) == 1 else t.cat(parts, dim=1)
            if m is not None:
                m = self._to_device(m, align16=True)
                S = t.from_numpy(rows.astype(np.float64).sum(axis=1).astype(np.float32)).to(device="cuda")
                coeff -= S.view(1, -1, 1) * m.view(1, 1, -1)
        return PodResult(rows=rows, eigenvalues=lam, fraction=frac, coefficients=coeff, offset=m)

    def exceedance(self, conditions, levels, side="above", want=("steps", "excess"), mode="fix"):
        """What depends on the order of the time steps of predict(conditions), per node and level, without the fields: levels a
        scalar, an [L] vector or [L, N] in physical units, 1 <= L <= MAX_LEVELS (see exceedance_levels); side "above" or "below";
        want: "steps" for the integer statistics (count, first, last, longest, runs), "excess" for the accumulated excess -> an
        ExceedanceResult.  The recon head's last pass compares the values predict() would store (bit for bit the same) with the
        levels, strictly, one thread per node going through the time steps in order: the result is integer apart from the excess,
        which is one fp32 sum over t ascending, so it depends on its condition, level and node alone, and the decoder's noise is
        placed as in project() (_condition_batches): the batch size does not show in the bits in either mode, and 24 L N bytes per
        condition leave the decoder instead of 4 T N.  The levels are
        uploaded once per call and every batch is written straight into its rows of the result.  Batching, streams, the single
        input-range decision and `mode` are temporal()'s: no host wait between batches."""
        t = self.torch
        if side not in EXCEEDANCE_SIDES:
            raise ValueError(f"side must be one of {sorted(EXCEEDANCE_SIDES)}, not {side!r}")
        want = _wanted(want, ("steps", "excess"), f"want: a tuple of 'steps' and 'excess' is required, not {want!r}",
                       "want: nothing to compute")
        if self.T > EXCEEDANCE_MAX_T:
            raise ValueError(f"num_time = {self.T} is beyond the limit of {EXCEEDANCE_MAX_T} time steps of the exceedance pass")
        conditions, P, _, remap = self._args(conditions, "TN", mode)
        lv = exceedance_levels(levels, self.N)
        L = lv.shape[0]
        stats = t.empty((P, 5, L, self.N), dtype=t.int32, device="cuda") if "steps" in want else None          # the result: the caller's stream owns it
        excess = t.empty((P, L, self.N), dtype=t.float32, device="cuda") if "excess" in want else None
        with _engine_stream(self._stream), contextlib.closing(self._condition_batches(conditions, P, remap)) as batches:
            lv = self._to_device(lv, align16=False)
            for lo, hi, lat, xs in batches:
                self.eng.exceedance(lat, xs, self.data_scale, self.data_min, lv, side=side, fix=mode == "fix",
                                    stats=False if stats is None else stats[lo:hi], excess=False if excess is None else excess[lo:hi])
        return ExceedanceResult(stream=self._stream, stats=stats, excess=excess, levels=lv, side=side, T=self.T)

    def cycles(self, conditions, gate=0.0, exponent=3, want=("turns", "rates"), mode="fix"):
        """The load cycles and the rates of every node's time history in predict(conditions), without the fields: gate a scalar or
        [N] in physical units, >= 0 (see cycles_gate), the hysteresis below which a reversal is not counted; exponent the integer
        m of the damage sum, 1 <= m <= MAX_CYCLES_EXPONENT; want: "turns" for the reversals, the sum and the largest of the
        ranges between them, the damage sum of range^m and the open excursion (ASTM E1049 simple-range counting), "rates" for the
        largest rise and fall between two steps, their steps and the path length -> a CyclesResult.  The recon head's last pass walks
        the values predict() would store (bit for bit the same), one thread per node going through the time steps in order, every
        difference, product and sum rounded on its own in fp32: a value depends on its condition and node alone, and the decoder's
        noise is placed as in project() (_condition_batches): the batch size does not show in the bits in either mode, and 40 N
        bytes per condition leave the decoder instead of 4 T N.  The gate is uploaded once per call and every batch is written
        straight into its rows of the result.  Batching, streams, the single input-range decision and `mode` are temporal()'s: no
        host wait between batches."""
        t = self.torch
        want = _wanted(want, ("turns", "rates"), f"want: a tuple of 'turns' and 'rates' is required, not {want!r}", "want: nothing to compute")
        m = int(exponent)
        if m != exponent or m < 1 or m > MAX_CYCLES_EXPONENT:
            raise ValueError(f"exponent = {exponent!r} is not an integer in [1, {MAX_CYCLES_EXPONENT}]")
        if self.T > CYCLES_MAX_T:
            raise ValueError(f"num_time = {self.T} is beyond the limit of {CYCLES_MAX_T} time steps of the cycles pass")
        conditions, P, _, remap = self._args(conditions, "TN", mode)
        g = cycles_gate(gate, self.N)
        new = lambda on, dt, *shape: t.empty((P,) + shape, dtype=dt, device="cuda") if on else None          # the result: the caller's stream owns it
        reversals, ranges = new("turns" in want, t.int32, self.N), new("turns" in want, t.float32, 4, self.N)
        rate_when, rates = new("rates" in want, t.int32, 2, self.N), new("rates" in want, t.float32, 3, self.N)
        with _engine_stream(self._stream), contextlib.closing(self._condition_batches(conditions, P, remap)) as batches:
            g = self._to_device(g, align16=False)
            for lo, hi, lat, xs in batches:
                self.eng.cycles(lat, xs, self.data_scale, self.data_min, g, exponent=m, fix=mode == "fix",
                                turns=False if ranges is None else (reversals[lo:hi], ranges[lo:hi]),
                                rates=False if rates is None else (rate_when[lo:hi], rates[lo:hi]))
        return CyclesResult(stream=self._stream, reversals=reversals, ranges=ranges, rate_when=rate_when, rates=rates, gate=g, exponent=m, T=self.T)

    def score(self, conditions, truth, mode="fix"):
        """How wrong predict(conditions) is against held-out fields, without the fields: truth [P, T, N] fp32 in physical units (the
        data set's own order; a CUDA tensor, or a host array / CPU tensor that is moved batch by batch on the engine stream as the
        conditions are) -> a ScoreResult of device tensors.  The recon head's last pass subtracts the truth from the values
        predict() would store (one fp32 subtraction each) and reduces the error in a fixed order: bitwise reproducible, ties to the
        smallest index.  truth must be finite (not checked).  Batching, streams, the single input-range decision and `mode` are
        sweep()'s: no host wait between batches."""
        t = self.torch
        conditions, P, _, remap = self._args(conditions, "TN", mode)
        truth = truth_fields(truth, P, self.T, self.N)
        if not t.is_tensor(truth):
            truth = t.from_numpy(np.ascontiguousarray(truth))
        f32 = dict(dtype=t.float32, device="cuda")
        i32 = dict(dtype=t.int32, device="cuda")
        node, when = t.empty((3, P, self.N), **f32), t.empty((P, self.N), **i32)          # the results: the caller's stream owns them
        frame, where = t.empty((3, P, self.T), **f32), t.empty((P, self.T), **i32)
        with _engine_stream(self._stream):
            b0 = min(self.batch, max(P, 1))
            buf = dict(node_err=t.empty((b0, 3, self.N), **f32), frame_err=t.empty((b0, self.T, 3), **f32))
            for lo, hi, lat, xs in self._latent_batches(conditions, P, remap):
                out = {k: v[:hi - lo] for k, v in buf.items()}
                out.update(node_when=when[lo:hi], frame_where=where[lo:hi])          # the results' own layout: written in place
                self.eng.score(lat, xs, self.data_scale, self.data_min, self._batch(truth, lo, hi).contiguous(), fix=mode == "fix", out=out)
                node[:, lo:hi].copy_(out["node_err"].transpose(0, 1))
                frame[:, lo:hi].copy_(out["frame_err"].permute(2, 0, 1))
            mse64, tms64 = frame[1].double(), frame[2].double()
            rmse = mse64.mean(dim=1).sqrt()
            rel_l2 = (mse64.sum(dim=1) / tms64.sum(dim=1)).sqrt()
            max_abs = frame[0].max(dim=1).values
        return ScoreResult(node_max_abs=node[0], node_bias=node[1], node_mse=node[2], t_worst=when, frame_max_abs=frame[0],
                           frame_mse=frame[1], frame_truth_ms=frame[2], n_worst=where, rmse=rmse, rel_l2=rel_l2, max_abs=max_abs)

    def ensemble(self, conditions, limit=None, want=("moments", "extrema"), mode="fix", into=None):
        """Statistics over the fields of all `conditions` per (time step, node), without the fields: what a Monte-Carlo or
        design-space study asks of thousands of draws -> an EnsembleResult of device tensors [T, N].  want: "moments" (mean and m2,
        Welford's running update; result.var() / std()), "extrema" (the envelope max / min and arg_max / arg_min, the index into
        `conditions` in call order of the draw that produced each); with `limit` (a scalar or N values in physical units, see
        exceed_limit) also "exceed", the number of draws above the limit, which is in the result exactly when a limit is given.
        The recon head's last pass merges the values predict() would store into the result tensors themselves, member after member
        in fp32: they are the running state, updated in place batch after batch; there are no per-batch buffers and no copies, and
        the result does not depend on the batch size, bit for bit.  into: an earlier result to go on accumulating into (same groups,
        same limit; its tensors are updated and returned in a new result with the larger count): equal to one call on the
        concatenated conditions, bit for bit, wherever the cut falls.  Draws of ONE design are conditions.repeat(K, 1) with
        mode="random": the decoder's latents are then sampled per draw.  The decoder's noise of a draw follows its index in the
        ensemble, not its place in a batch (predict() draws per call): the same seed gives the same ensemble at any batch size, two
        studies on one seed share their random numbers, and predict() sees the same draws only while it makes a single call.
        Batching, streams, the single input-range decision and `mode` are sweep()'s: no host wait between batches, the last
        batch may be ragged."""
        t = self.torch
        conditions, P, _, remap = self._args(conditions, "TN", mode)
        want = tuple(want)
        groups = ENSEMBLE_GROUPS
        want = _wanted(want + (("exceed",) if limit is not None else ()), groups,          # a limit asks for "exceed" by itself
                       f"want must name groups of {tuple(groups)}, not {want!r}", f"want must name at least one of {tuple(groups)}")
        if limit is None and "exceed" in want:
            raise ValueError("want names 'exceed' but no limit is given")
        lim = None if limit is None else exceed_limit(limit, self.N)
        spec = {k: ((self.N,) if k == "limit" else (self.T, self.N), t.int32 if k in ("arg_max", "arg_min", "exceed") else t.float32)
                for g in want for k in groups[g]}          # the tensors of this ensemble
        state, count = {}, 0
        if into is not None:
            EnsembleResult.require(into)
            if into.groups() != want:
                raise ValueError(f"into holds the groups {into.groups()}, this call asks for {want}")
            state, count = into.continued(spec)
            if lim is not None and not np.array_equal(state["limit"].cpu().numpy(), lim):
                raise ValueError("into was accumulated against another limit")
        if count + P > ENSEMBLE_MAX_COUNT:
            raise ValueError(f"{count} + {P} members: an ensemble holds at most 2^24")
        with _engine_stream(self._stream):
            if into is None:
                for k, (shape, dtype) in spec.items():
                    state[k] = t.from_numpy(lim).cuda() if k == "limit" else t.empty(shape, dtype=dtype, device="cuda")
                if P == 0:          # the empty ensemble, as the first batch would have found it
                    for k, v in state.items():
                        if k != "limit":
                            v.fill_({"max": float("-inf"), "min": float("inf")}.get(k, 0))
            for lo, hi, lat, xs in self._latent_batches(conditions, P, remap):
                self.eng.ensemble(lat, xs, self.data_scale, self.data_min, state, count + lo, fix=mode == "fix")
        return EnsembleResult(stream=self._stream, count=count + P, **{k: state.get(k) for k in EnsembleResult.FIELDS if k != "count"})

    def distribution(self, conditions, range, bins=32, mode="fix", into=None):
        """The empirical distribution of the fields of all `conditions` per (time step, node), without the fields: percentile bands
        (result.quantile([0.05, 0.5, 0.95])) and the histogram behind them -> a DistributionResult of device tensors.  The second
        pass of a study: range gives the bounds between which `bins` uniform bins lie (DISTRIBUTION_MIN_BINS <= bins <=
        DISTRIBUTION_MAX_BINS), normally the EnsembleResult of ensemble(conditions, want=("extrema",), mode=mode) on the same seed,
        whose min / max tensors are used as they are, without a copy; or a pair (lo, hi) of scalars, of [N] arrays or of [T, N]
        arrays or CUDA tensors in physical units (hist_range).  The decoder's noise of a draw follows its index, as in ensemble(),
        so this pass regenerates the fields of the first one bit for bit and no draw falls outside its envelope: result.under and
        result.over are zero, in mode "random" too.  The recon head's last pass bins the values predict() would store and adds to
        result.counts, which is the running state: integer counts, exact and independent of order and batch size.  A value equal
        to hi is in the last bin; where hi == lo every value equal to them is in the first.  into: an earlier result to go on
        counting into (same bins, same bounds; its counts are updated and returned in a new result with the larger count): equal
        to one call on the concatenated conditions, bit for bit.  Batching, streams, the single input-range decision and `mode`
        are ensemble()'s: no host wait between batches, the last batch may be ragged."""
        t = self.torch
        conditions, P, _, remap = self._args(conditions, "TN", mode)
        K = int(bins)
        if K != bins or K < DISTRIBUTION_MIN_BINS or K > DISTRIBUTION_MAX_BINS:
            raise ValueError(f"bins = {bins!r} is outside [{DISTRIBUTION_MIN_BINS}, {DISTRIBUTION_MAX_BINS}]")
        lo, hi = hist_range(range, self.T, self.N)
        spec = {"lo": ((self.T, self.N), t.float32), "hi": ((self.T, self.N), t.float32), "counts": ((K + 2, self.T, self.N), t.int32)}
        state, count = None, 0
        if into is not None:
            DistributionResult.require(into)
            if int(into.bins) != K:
                raise ValueError(f"into holds {into.bins} bins, this call asks for {K}")
            state, count = into.continued(spec)
            for name, v in (("lo", lo), ("hi", hi)):
                same = v is state[name] or (t.equal(v, state[name]) if t.is_tensor(v) else np.array_equal(state[name].cpu().numpy(), v))
                if not same:
                    raise ValueError(f"into was counted between other bounds ({name} differs)")
        if count + P > ENSEMBLE_MAX_COUNT:
            raise ValueError(f"{count} + {P} members: a distribution holds at most 2^24")
        with _engine_stream(self._stream):
            if state is None:
                state = {"lo": lo if t.is_tensor(lo) else t.from_numpy(lo).cuda(), "hi": hi if t.is_tensor(hi) else t.from_numpy(hi).cuda(),
                         "counts": t.zeros(spec["counts"][0], dtype=t.int32, device="cuda")}          # the pass only ever adds
            for b_lo, b_hi, lat, xs in self._latent_batches(conditions, P, remap):
                self.eng.distribution(lat, xs, self.data_scale, self.data_min, state, count + b_lo, fix=mode == "fix")
        return DistributionResult(stream=self._stream, count=count + P, bins=K, lo=state["lo"], hi=state["hi"], counts=state["counts"])

    def regress(self, conditions, covariates=None, mode="fix", into=None):
        """The linear response surface of the fields of all `conditions` on K covariates per (time step, node), without the fields:
        what the draws of a Monte-Carlo or space-filling study say about which input drives the response -> a RegressionResult.
        result.coefficients() [K, T, N] are the regression coefficients, result.r2() [T, N] the share of the variance they explain:
        where it is close to 1 the coefficients are the sensitivities and no Sobol study is needed, where it is not, that is where
        to spend one.  covariates: [P, K] values per condition (regression_covariates; a host array or a tensor, 1 <= K <=
        REGRESS_MAX_COVARIATES), e.g. a probe history column of sweep(), to ask what co-varies with it; None: the columns of
        `conditions` themselves (conditions on the device are read back once for that).  The recon head's last pass merges the values
        predict() would store into mean, m2 (the moments of ensemble(), bit for bit) and the co-moments, the result tensors
        themselves; the covariates are centred on the host in float64 (regression_weights), which also keeps their mean and Gram
        matrix.  into: an earlier result of the same K to go on accumulating into (count, device state, cov_mean and cov_gram
        continue): equal to one call on the concatenated conditions, bit for bit, wherever the cut falls.  Batching, streams, the
        single input-range decision, `mode` and the noise that follows the member index are ensemble()'s."""
        t = self.torch
        conditions, P, _, remap = self._args(conditions, "TN", mode)
        if covariates is None:
            if int(conditions.shape[1]) > REGRESS_MAX_COVARIATES:
                raise ValueError(f"conditions have {int(conditions.shape[1])} columns, more than {REGRESS_MAX_COVARIATES}: give explicit covariates "
                                 f"[P, K] (covariates=...)")
            covariates = conditions
        if t.is_tensor(covariates):
            covariates = covariates.detach().cpu().numpy()
        Y = regression_covariates(covariates, P)
        K = Y.shape[1]
        spec = {"mean": ((self.T, self.N), t.float32), "m2": ((self.T, self.N), t.float32), "comoment": ((K, self.T, self.N), t.float32)}
        state, count, ybar, gram = {}, 0, None, None
        if into is not None:
            RegressionResult.require(into)
            if not t.is_tensor(into.comoment) or into.comoment.dim() != 3 or int(into.comoment.shape[0]) != K:
                raise ValueError(f"into holds {int(into.comoment.shape[0]) if t.is_tensor(into.comoment) and into.comoment.dim() == 3 else 'no'} covariates, "
                                 f"this call has {K}")
            state, count = into.continued(spec)
            ybar, gram = np.asarray(into.cov_mean, np.float64), np.asarray(into.cov_gram, np.float64)
            if ybar.shape != (K,) or gram.shape != (K, K):
                raise ValueError(f"into.cov_mean / into.cov_gram must be [K] / [K, K] with K = {K}, got {ybar.shape} / {gram.shape}")
        if count + P > ENSEMBLE_MAX_COUNT:
            raise ValueError(f"{count} + {P} members: a regression holds at most 2^24")
        w, ybar, gram = regression_weights(Y, ybar, gram, count)
        with _engine_stream(self._stream):
            if into is None:
                for k, (shape, dtype) in spec.items():
                    state[k] = (t.zeros if P == 0 else t.empty)(shape, dtype=dtype, device="cuda")
            w = t.from_numpy(w).cuda()
            for lo, hi, lat, xs in self._latent_batches(conditions, P, remap):
                self.eng.regress(lat, xs, self.data_scale, self.data_min, state, w[lo:hi], count + lo, fix=mode == "fix")
        return RegressionResult(stream=self._stream, count=count + P, mean=state["mean"], m2=state["m2"], comoment=state["comoment"],
                                cov_mean=ybar, cov_gram=gram)

    def sobol(self, A, B, groups=None, want=("first", "total"), into=None):
        """Variance-based global sensitivity of the response to its inputs per (time step, node), without the fields: which
        parameter drives the field, where on the mesh and when -> a SobolResult of device tensors.  A, B [n, F]: two independent
        sample matrices of conditions (sobol_design; host arrays or CUDA tensors, preprocessed as the conditioner's training set
        holds them).  groups: the d parameters as lists of column indices (sobol_groups; None: every column is a parameter).
        Base sample j is evaluated at A_j, B_j and AB_1_j .. AB_d_j (A_j with the columns of parameter i from B_j): n (d + 2) decoder
        passes, whose last pass keeps only running sums -- the result tensors themselves, updated in place batch after batch.
        want: "first" (result.first_order(): S_i, the share of the variance of the response that parameter i explains alone;
        sum_i S_i <= 1, the rest is interaction) and / or "total" (result.total_order(): ST_i >= S_i, the share that involves
        parameter i at all; ST_i = 0 means the parameter can be fixed).  Both are Jansen's estimators, sums of squared differences:
        non-negative, no centring, fp32-safe; their sampling error falls as 1 / sqrt(n), and an S_i of a weak parameter can come
        out slightly negative.  There is no `mode`: a sensitivity study needs a deterministic response, so the decoder always runs
        in the reference's "fix" mode, whose latent noise is scaled by 1e-10 -- numerically negligible but not bit-zero: it follows
        the member's index in the study (as in ensemble()), so the same seed gives the same bits at any batch size and for any cut
        into `into=` calls.  A batch takes self.batch // (d + 2) whole blocks.  into: an earlier result to go on accumulating into
        (same d, same want; its tensors are updated and returned in a new result with the larger count): equal to one call on
        the concatenated samples, bit for bit.  At most 2^23 base samples.  The single input-range decision of predict() is taken
        over A and B together; no host wait between batches."""
        t = self.torch
        A, n, _, remap_a = self._args(A, "TN", "fix")
        B, nb_, _, remap_b = self._args(B, "TN", "fix")
        if tuple(A.shape) != tuple(B.shape):
            raise ValueError(f"A and B must be of one shape [n, F], got {tuple(A.shape)} and {tuple(B.shape)}")
        remap = None if remap_a is None else (remap_a or remap_b)
        F = int(A.shape[1])
        groups = sobol_groups(groups, F)
        d = len(groups)
        want = tuple(want)
        want = _wanted(want, SobolResult.PARTS, f"want must name parts of {tuple(SobolResult.PARTS)}, not {want!r}",
                       f"want must name at least one of {tuple(SobolResult.PARTS)}")
        per = self.batch // (d + 2)
        if per < 1:
            raise ValueError(f"a block of d + 2 = {d + 2} members does not fit a batch of {self.batch}: build the Surrogate with batch >= {d + 2}")
        shapes = {"mean": (self.T, self.N), "m2": (self.T, self.N)}
        shapes.update({SobolResult.PARTS[w]: (d, self.T, self.N) for w in want})          # the tensors of this study
        state, count = {}, 0
        if into is not None:
            SobolResult.require(into)
            if int(into.n_params) != d:
                raise ValueError(f"into holds {into.n_params} parameters, this call has {d}")
            if into.want() != want:
                raise ValueError(f"into holds the parts {into.want()}, this call asks for {want}")
            state, count = into.continued({k: (shape, t.float32) for k, shape in shapes.items()})
        if count + n > SOBOL_MAX_COUNT:
            raise ValueError(f"{count} + {n} base samples: a study holds at most 2^23")
        take = np.zeros((d + 2, F), bool)          # which columns of a member come from B
        take[1] = True
        for i, g in enumerate(groups):
            take[2 + i, g] = True
        with _engine_stream(self._stream):
            if into is None:
                for k, shape in shapes.items():
                    state[k] = (t.zeros if n == 0 else t.empty)(shape, dtype=t.float32, device="cuda")
            take = t.from_numpy(take).cuda()[None]
            for lo, hi in self._batches(n, per):
                a, b = self._batch(A, lo, hi)[:, None, :], self._batch(B, lo, hi)[:, None, :]
                members = t.where(take, b, a).reshape((hi - lo) * (d + 2), F)          # A_j, B_j, AB_1_j .. AB_d_j per base sample
                lat, xs = self._latents(members, remap)
                self.eng.sobol(lat, xs, self.data_scale, self.data_min, state, d, count + lo, fix=True)
        return SobolResult(stream=self._stream, count=count + n, n_params=d, mean=state["mean"], m2=state["m2"],
                           first_sq=state.get("first_sq"), total_sq=state.get("total_sq"))

    def predict_to_host(self, conditions, out=None, layout="TN", mode="fix"):
        """The same result in pinned host memory: two device batch buffers alternate, each batch's device-to-host copy runs on the
        engine's copy stream behind the batch's last kernel, and the host waits once, at the end."""
        t = self.torch
        conditions, P, shape, remap = self._args(conditions, layout, mode)
        if out is None:
            out = t.empty(shape, dtype=t.float32, pin_memory=True)
        elif not (is_tensor_of(out, t.float32, shape, device="cpu") and out.is_pinned()):
            raise ValueError(f"out must be a contiguous pinned float32 CPU tensor of shape {shape}")
        if self._copy_stream is None:
            self._copy_stream = t.cuda.ExternalStream(self.eng.copy_stream())
        cs = self._copy_stream
        self._stream.wait_stream(t.cuda.current_stream())
        with t.cuda.stream(self._stream):
            bufs = [t.empty((self.batch,) + shape[1:], dtype=t.float32, device="cuda") for _ in range(min(2, (P + self.batch - 1) // self.batch))]
        copied = [None, None]
        for i, (lo, hi) in enumerate(self._batches(P, self.batch)):
            buf = bufs[i % 2][:hi - lo]
            with t.cuda.stream(self._stream):
                if copied[i % 2] is not None:
                    self._stream.wait_event(copied[i % 2])          # the buffer's previous copy has left it
                self._generate(self._batch(conditions, lo, hi), buf, layout, mode == "fix", remap)
                done = t.cuda.Event()
                done.record(self._stream)
            cs.wait_event(done)
            with t.cuda.stream(cs):
                out[lo:hi].copy_(buf, non_blocking=True)
                copied[i % 2] = t.cuda.Event()
                copied[i % 2].record(cs)
        cs.synchronize()                                             # the one host wait; the buffers are free again after it
        return out
