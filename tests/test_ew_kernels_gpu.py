"""Kernel-level parity of the non-GEMM kernels of the step (csrc/ew.hip) against tests/ew_reference.py (PyTorch float64 +
autograd on the CPU), through the sgv_test_* hooks: GroupNorm forward / backward on both dispatch paths, the recon loss for every
(dtype, loss kind, train), the latent / stage kernels on both sides of their clamps, ew_act and the Linear head / expand kernels.

Every case: seeded inputs (bf16-exact where a bf16 kernel reads them), outputs pre-filled with NaN, padded rows (ld > C) carrying a
canary that must survive, and a second launch that must be bitwise equal (no kernel of the step uses atomics).

Tolerances (none tuned on the kernels):
  * elementwise, stored in fp32: 2e-5 of the max-norm of the reference (the project's figure for fp32 kernels);
  * elementwise, stored in bf16: per element |got - ref| <= 2^-8 |ref| + 2e-5 max|ref| (fp32 compute, one rounding; half an ulp is
    2^-9, the factor 2 admits a rounding flipped by fp32 summation order);
  * reductions: relative to the sum of the magnitudes of their terms, max(4 x measured, 2^-22), `measured` being the error of a
    float32 re-summation of the same sum in two other orders (ew_reference.f32_sum_error), computed on the CPU at run time on the
    case's own inputs (slabs above 2M elements: on their first 2080 columns) and printed with every check; TOL below holds the
    floor and, for orientation, what `measured` comes to, tests/test_ew_reference_host.py keeps those figures honest.  Three
    departures from a bare re-ordering, each derived where it is made: sums of a handful of terms (GroupNorm backward, ew_act) are
    restated with the terms themselves evaluated in float32; the Linear sums take the worst of many outputs, as the check does;
    the conv-bias gradient is scaled by the terms of the closed form the kernels use for it;
  * kinks (ReLU at z = 0, sign(xhat - x) for MAE): the inputs are nudged until no element lies within 1e-4 of one, and the test
    asserts that none lies within 1e-5: nothing is left out of any check.  Planted clamp values of the latent / stage tests sit
    exactly on an edge or >= 0.1 away; see PLANTED and check_planted for how each of them is made to count.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import simulgen_vae_amd  # noqa: F401
from simulgen_vae_amd import engine as E

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ew_reference as R  # noqa: E402

pytestmark = pytest.mark.gpu

FLOOR = 2.0 ** -22
# reduction kind -> (orientation: the float32 re-summation error at (B, T, C) = (2, 200, 2080), an upper bound the host test checks;
# the floor of the tolerance).  check_red uses the floor and the value measured on the case itself, never the first column.
# Over all cases of this file `measured` stays <= 1.0e-6 (tolerance 4e-6), reached at (3, 1, 64, 8) with GELU where a group sum has
# eight float32-evaluated terms; elsewhere it is <= 3e-7 and mostly the floor decides.  The closed-form scale of dbias is at most
# 1.9 x sum |dY|, except at T = 1 (up to 23 x: T * m1 and m2 * xhat there are single terms that cancel against gamma * dz).
TOL = {
    "loss": (1e-7, FLOOR),      # one sum over all elements (loss sums, cdot, KL): 7e-8 measured
    "column": (3e-7, FLOOR),    # one sum per channel over the B*T rows (dgamma, dbeta, dbias): 2.3e-7 measured
    "group": (1e-7, FLOOR),     # one sum per (sample, group) over T x Cg (sums, sums2): 4e-8 measured
}
ELT32 = 2e-5
TANH_ERR = 2e-7     # absolute error of tanh_f (csrc/sgv_common.h)
CANARY = 768.0      # bf16-exact


def _torch():
    import torch
    return torch


def _bf16(a):
    torch = _torch()
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(torch.bfloat16).to(torch.float32).numpy()


class Map:
    """a [rows][ld] device map of the compute dtype with ld - C canary columns"""

    def __init__(self, rows, Cn, dtype, data=None, pad=8):
        torch = _torch()
        self.C, self.ld = Cn, Cn + pad
        self.t = torch.full((rows, self.ld), CANARY, dtype=torch.bfloat16 if dtype == 1 else torch.float32, device="cuda")
        if data is None:
            self.t[:, :Cn] = float("nan")
        else:
            self.t[:, :Cn] = torch.from_numpy(np.ascontiguousarray(data, np.float32).reshape(rows, Cn)).cuda().to(self.t.dtype)

    @property
    def p(self):
        return self.t.data_ptr()

    def get(self, shape=None):
        assert bool((self.t[:, self.C:].float() == CANARY).all()), "padding columns were overwritten"
        a = self.t[:, :self.C].float().cpu().numpy().astype(np.float64)
        return a.reshape(shape) if shape else a


def _f(a):
    torch = _torch()
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


def _nan(n, dt=None):
    torch = _torch()
    return torch.full((int(n),), float("nan"), dtype=dt or torch.float32, device="cuda")


def _p(t):
    return None if t is None else t.data_ptr()


def _h(t):
    return t.double().cpu().numpy()


def _ok(lib, rc):
    assert rc == 0, lib.sgv_last_error().decode()


def check_elt(got, ref, dtype, what):
    ref = np.asarray(ref, np.float64)
    got = np.asarray(got, np.float64).reshape(ref.shape)
    assert np.isfinite(got).all(), f"{what}: non-finite output (an element was not written?)"
    mx = np.abs(ref).max()
    tol = ELT32 * mx + (2.0 ** -8 * np.abs(ref) if dtype == 1 else 0.0)
    err = np.abs(got - ref)
    print(f"  {what}: max err {err.max():.3e} (max|ref| {mx:.3e}, worst err/tol {np.max(err / np.maximum(tol, 1e-300)):.3f})")
    assert np.all(err <= tol), f"{what}: {int((err > tol).sum())} elements off, worst {err.max():.3e} at {np.unravel_index(np.argmax(err - tol), ref.shape)}"


def check_red(got, ref, mag, measured, what, kind, extra=0.0):
    ref, mag = np.asarray(ref, np.float64), np.asarray(mag, np.float64)
    got = np.asarray(got, np.float64).reshape(ref.shape)
    assert np.isfinite(got).all(), f"{what}: non-finite"
    tol = max(4.0 * measured, TOL[kind][1])
    err = np.abs(got - ref) / np.maximum(mag, 1e-300)
    print(f"  {what}: err / sum of magnitudes {err.max():.3e} (tolerance {tol:.3e}, float32 re-summation {measured:.3e})")
    assert np.all(np.abs(got - ref) <= tol * mag + extra + 1e-300), f"{what}: {err.max():.3e} > {tol:.3e}"


def measure(y, dterm, G):
    """float32 re-summation errors of the three reduction kinds on this case's inputs (dterm: an [B, T, C] array of terms)"""
    B, T, Cn = y.shape
    if y.size > (2 << 20):                      # first sample, first group (at most 2080 columns of it)
        Cn = min(Cn // G, 2080)
        y, dterm, G, B = y[:1, :, :Cn], dterm[:1, :, :Cn], 1, 1
    return {"loss": R.f32_sum_error(dterm)[0], "column": R.f32_sum_error(dterm.reshape(B * T, Cn), axis=0)[0],
            "group": R.f32_sum_error(np.asarray(y, np.float64).reshape(B, T, G, Cn // G), axis=(1, 3))[0]}


def measure_bwd(m, ref, terms32, gamma, G):
    """dgamma / dbeta: the restatement evaluates the terms in float32 too (few rows per column: the terms' own rounding, not the
    order of the sum, is what such a sum carries); sums2 likewise (T = 1: eight terms per group, xhat = (y - mean) * rstd cancels
    in float32), on the first group.  Raises m["column"] and m["group"] to what that gives."""
    dz32, dzx32 = terms32
    dz64 = ref["dz"]
    B, T, Cn = dz64.shape
    rows = B * T
    cs = slice(0, Cn if dz64.size <= (2 << 20) else 2080)
    m["column"] = max(m["column"],
                      R.f32_sum_error(dz64[:, :, cs].reshape(rows, -1), 0, dz32[:, :, cs].reshape(rows, -1))[0],
                      R.f32_sum_error((dz64 * ref["xnorm"])[:, :, cs].reshape(rows, -1), 0, dzx32[:, :, cs].reshape(rows, -1))[0])
    w = min(Cn // G, 2080)
    g64 = (gamma.astype(np.float64) * dz64)[:, :, :w]
    g32 = (gamma * dz32)[:, :, :w]
    m["group"] = max(m["group"], R.f32_sum_error(g64, (1, 2), g32)[0],
                     R.f32_sum_error(g64 * ref["xnorm"][:, :, :w], (1, 2), (gamma * dzx32)[:, :, :w])[0])


def gn_inputs(seed, B, T, Cn, dtype):
    rng = np.random.default_rng(seed)
    y = (rng.standard_normal((B, T, Cn)) * 2 + 0.5).astype(np.float32)
    d = rng.standard_normal((B, T, Cn)).astype(np.float32)
    res = rng.standard_normal((B, T, Cn)).astype(np.float32)
    if dtype == 1:
        y, d, res = _bf16(y), _bf16(d), _bf16(res)
    gamma = (1 + 0.3 * rng.standard_normal(Cn)).astype(np.float32)
    beta = (0.3 * rng.standard_normal(Cn)).astype(np.float32)
    cbias = (0.3 * rng.standard_normal(Cn)).astype(np.float32)
    return y, d, res, gamma, beta, cbias


def off_the_kink(y, G, gamma, beta, dtype):
    """move the few elements whose z lies within 1e-4 of ReLU's kink; afterwards none is within 1e-5"""
    for _ in range(8):
        z = R.gn_forward(y, G, gamma, beta, 0)["z"]
        near = np.abs(z) < 1e-4
        if not near.any():
            break
        y = y.copy()
        y[near] += 0.5
        if dtype == 1:
            y = _bf16(y)
    assert not (np.abs(R.gn_forward(y, G, gamma, beta, 0)["z"]) < 1e-5).any()
    return y


# (B, T, C, G, forward path, backward path): 1 = the one-launch slab kernel, 0 = the multi-kernel chain.  From the dispatch code:
# forward slab: Cg % 8 == 0 and ceil(T / (256 / cv)) <= 16; backward slab: cv <= 32 and ceil(T / (512 / cv)) <= 8, cv = pow2 >= Cg / 8.
GN_SHAPES = [
    (2, 200, 128, 8, 1, 1),       # the engine's own widths: Cg 16
    (2, 200, 512, 8, 1, 1),       # Cg 64
    (2, 200, 512, 32, 1, 1),      # 32 groups of 16
    (2, 200, 1024, 8, 1, 1),      # Cg 128
    (2, 200, 1280, 8, 0, 0),      # Cg 160: 20 column vectors on 32 lanes, 25 rows per thread
    (2, 128, 1280, 8, 1, 1),      # the slab kernels' limits with idle column lanes: 16 rows per thread forward, 8 backward
    (2, 129, 1280, 8, 0, 0),      # one row more: 17 and 9
    (2, 64, 2048, 8, 1, 1),       # backward cv = 32
    (2, 64, 4096, 8, 1, 0),       # backward cv = 64: chain
    (3, 10, 72, 8, 0, 0),         # the fixture net: Cg = 9, not a multiple of 8
    (3, 1, 64, 8, 1, 1),          # T = 1
    (1, 37, 64, 8, 1, 1),         # B = 1, T not a multiple of the row lanes
    (2, 4096, 256, 32, 1, 1),     # image conditioner: Cg 8 at the slab limits (16 / 8 rows per thread)
    (1, 4104, 256, 32, 0, 0),     # ... one past them: narrow-group partials and the `lanes` finalize
    (2, 4096, 512, 32, 0, 0),     # Cg 16 on the chain
    (1, 16, 8 * 12296, 8, 0, 0),  # Cg 12296 > 12288: the spill loop of the finalize kernel
]
BIG = (2, 200, 95008, 8, 0, 0)    # the recon head's width: Cg 11876, 12 columns per thread in the finalize


def run_gn_case(shape, dtype, acts_f, acts_b):
    lib = E.load_library()
    torch = _torch()
    B, T, Cn, G, pf, pb = shape
    y, d, res, gamma, beta, cbias = gn_inputs(hash(shape) % (2 ** 31), B, T, Cn, dtype)
    if 3 in [a for a, _ in acts_f] or 3 in acts_b:
        y = off_the_kink(y, G, gamma, beta, dtype)
    rows = B * T
    nws = lib.sgv_test_gn_workspace_floats(B, T, Cn)
    work = _nan(nws)
    ym, dm, rm = Map(rows, Cn, dtype, y), Map(rows, Cn, dtype, d), Map(rows, Cn, dtype, res)
    gd, bd, cbd = _f(gamma), _f(beta), _f(cbias)
    path = C.c_int(-1)
    sums_ref = None
    for act, use_res in acts_f:
        rscale = 0.5 if use_res else 1.0
        ref = R.gn_forward(y, G, gamma, beta, act, res if use_res else None, rscale)
        m = measure(y, ref["out"], G)
        outs = []
        for rep in range(2):
            om, sums = Map(rows, Cn, dtype), _nan(B * G * 2, torch.float64)
            _ok(lib, lib.sgv_test_gn_fwd(dtype, act, ym.p, ym.ld, rm.p if use_res else None, rm.ld, rscale, om.p, om.ld, _p(gd), _p(bd),
                                         _p(sums), _p(work), nws, B, T, Cn, G, C.byref(path), None))
            outs.append((om.t.clone(), sums.clone()))
        assert path.value == pf, f"forward dispatch moved: path {path.value}"
        assert torch.equal(outs[0][0].view(torch.uint8), outs[1][0].view(torch.uint8)) and torch.equal(outs[0][1], outs[1][1]), "replay differs"
        print(f"gn_fwd {shape} dtype {dtype} act {act} res {use_res} path {path.value}")
        check_elt(om.get(), ref["out"].reshape(rows, Cn), dtype, "out")
        check_red(_h(sums), ref["sums"], ref["sums_mag"], m["group"], "sums", "group")
        sums_ref = ref["sums"]
    sums_d = torch.from_numpy(np.ascontiguousarray(sums_ref if sums_ref is not None else R.gn_stats(y, G)["sums"])).cuda()
    for i, act in enumerate(acts_b):
        rscale, gscale, accum = (0.5, 0.25, 1) if i % 2 else (1.0, 1.0, 0)
        ref = R.gn_backward(y, d, G, gamma, beta, act, rscale, gscale, cbias)
        m = measure(y, ref["dy"], G)
        measure_bwd(m, ref, R.gn_bwd_terms_f32(y, d, G, gamma, beta, act, rscale), gamma, G)
        outs = []
        for rep in range(2):
            dym, s2 = Map(rows, Cn, dtype), _nan(B * G * 2, torch.float64)
            if accum:
                aff = [torch.full((Cn,), v, device="cuda") for v in (1.0, -2.0, 3.0)]
            else:
                aff = [_nan(Cn) for _ in range(3)]
            cdot = _nan(1)
            _ok(lib, lib.sgv_test_gn_bwd(dtype, act, ym.p, ym.ld, dm.p, dm.ld, rscale, gscale, _p(gd), _p(bd), _p(sums_d), dym.p, dym.ld, _p(s2),
                                         _p(aff[0]), _p(aff[1]), _p(aff[2]), _p(cdot), _p(cbd), accum, _p(work), nws, B, T, Cn, G,
                                         C.byref(path), None))
            outs.append(torch.cat([dym.t.float().flatten(), s2.float(), aff[0], aff[1], aff[2], cdot]))
        assert path.value == pb, f"backward dispatch moved: path {path.value}"
        assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32)), "replay differs"
        print(f"gn_bwd {shape} dtype {dtype} act {act} rscale {rscale} gscale {gscale} accum {accum} path {path.value}")
        check_elt(dym.get(), ref["dy"].reshape(rows, Cn), dtype, "dy")
        check_red(_h(s2), ref["sums2"], ref["sums2_mag"], m["group"], "sums2", "group")
        base = (1.0, -2.0, 3.0) if accum else (0.0, 0.0, 0.0)
        for k, name in enumerate(("dgamma", "dbeta", "dbias")):
            check_red(_h(aff[k]) - base[k], ref[name], ref[name + "_mag"] + abs(base[k]), m["column"], name, "column")
        check_red(_h(cdot)[0], ref["cdot"], ref["cdot_mag"], m["loss"], "cdot", "loss")


@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("shape", GN_SHAPES, ids=lambda s: "x".join(map(str, s[:4])))
def test_groupnorm(shape, dtype):
    big = shape[0] * shape[1] * shape[2] > (1 << 20)
    run_gn_case(shape, dtype, ((1, 0), (3, 1)) if big else ((0, 0), (1, 1), (1, 0), (2, 0), (3, 1)), (1, 3) if big else (0, 1, 3))


@pytest.mark.parametrize("dtype", [0, 1])
def test_groupnorm_recon_width(dtype):
    """C = 95 008, G = 8 (Cg = 11 876, not a multiple of 8): the chain with the register form of the finalize; GELU, with the residual
    in bf16 and without it in fp32"""
    run_gn_case(BIG, dtype, ((1, dtype),), (1,))


RECON_SHAPES = [(3, 10, 72), (2, 200, 2080), (2, 200, 95008)]
_recon_cache = {}


def recon_inputs(shape, dtype):
    """bf16 kernels get bf16-exact maps, fp32 kernels the unrounded ones (all 24 mantissa bits in use); one set alive at a time"""
    if (shape, dtype) not in _recon_cache:
        _recon_cache.clear()
        B, T, Cn = shape
        rng = np.random.default_rng(Cn)
        y = (rng.standard_normal(shape) * 2 + 0.5).astype(np.float32)
        x = rng.uniform(-2, 2, shape).astype(np.float32)
        if dtype == 1:
            y, x = _bf16(y), _bf16(x)
        gamma = (1 + 0.3 * rng.standard_normal(Cn)).astype(np.float32)
        beta = (0.3 * rng.standard_normal(Cn)).astype(np.float32)
        cbias = (0.3 * rng.standard_normal(Cn)).astype(np.float32)
        for _ in range(8):                    # MAE's kink: move the targets that sit within 1e-4 of xhat
            d = R.recon_loss(y, x, 8, gamma, beta, 0, False)["diff"]
            near = (np.abs(d) < 1e-4) | (np.abs(np.abs(d) - 1) < 1e-4)
            if not near.any():
                break
            x[near] = x[near] + np.float32(0.25)
            if dtype == 1:
                x = _bf16(x)
        _recon_cache[(shape, dtype)] = (y, x, gamma, beta, cbias, {})
    return _recon_cache[(shape, dtype)]


@pytest.mark.parametrize("train", [1, 0])
@pytest.mark.parametrize("kind", [0, 1, 2, 3])
@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("shape", RECON_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_recon_loss(shape, kind, dtype, train):
    """one float64 reference per (shape, dtype, loss kind), shared by the train and eval cases (they follow each other)"""
    lib = E.load_library()
    torch = _torch()
    B, T, Cn = shape
    G, rows = 8, B * T
    y, x, gamma, beta, cbias, refs = recon_inputs(shape, dtype)
    gscale = 1e6 / (rows * Cn)
    if kind not in refs:
        refs.clear()
        refs[kind] = R.recon_loss(y, x, G, gamma, beta, kind, True, gscale, cbias)
        refs[kind]["m"] = measure(y, refs[kind]["diff"] ** 2, G)
        measure_bwd(refs[kind]["m"], refs[kind], R.gn_bwd_terms_f32(y, x, G, gamma, beta, 2, 1.0, kind), gamma, G)
    ref = refs[kind]
    m = ref["m"]
    ad = np.abs(ref["diff"])
    share = float(np.mean(ad > 1))
    assert 0.2 < share < 0.8, share                    # else smoothL1 / Huber are MSE / 2 and the test cannot tell
    assert not (ad < 1e-5).any() and not (np.abs(ad - 1) < 1e-5).any()
    nws = lib.sgv_test_gn_workspace_floats(B, T, Cn)
    work = _nan(nws)
    ym, xm = Map(rows, Cn, dtype, y), Map(rows, Cn, dtype, x)
    gd, bd, cbd = _f(gamma), _f(beta), _f(cbias)
    outs = []
    for rep in range(2):
        xh, dym = Map(rows, Cn, dtype), Map(rows, Cn, dtype)
        sums, ls, s2 = (_nan(n, torch.float64) for n in (B * G * 2, 2, B * G * 2))
        unit, cdot = _nan(3 * Cn), _nan(1)
        _ok(lib, lib.sgv_test_recon_loss(dtype, train, kind, ym.p, ym.ld, xm.p, xm.ld, xh.p, xh.ld, _p(gd), _p(bd), _p(sums), _p(ls),
                                         _p(s2) if train else None, _p(unit) if train else None, gscale, dym.p if train else None, dym.ld,
                                         _p(cdot) if train else None, _p(cbd), _p(work), nws, B, T, Cn, G, None))
        outs.append(torch.cat([xh.t.float().flatten(), dym.t.float().flatten(), sums.float(), ls.float(), s2.float(), unit, cdot]))
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32)), "replay differs"
    # the same call without xhat (what a training step does): every other output bitwise as before
    sums3, ls3, s23 = (_nan(n, torch.float64) for n in (B * G * 2, 2, B * G * 2))
    unit3, cdot3, dym3 = _nan(3 * Cn), _nan(1), Map(rows, Cn, dtype)
    _ok(lib, lib.sgv_test_recon_loss(dtype, train, kind, ym.p, ym.ld, xm.p, xm.ld, None, 0, _p(gd), _p(bd), _p(sums3), _p(ls3),
                                     _p(s23) if train else None, _p(unit3) if train else None, gscale, dym3.p if train else None, dym3.ld,
                                     _p(cdot3) if train else None, _p(cbd), _p(work), nws, B, T, Cn, G, None))
    no_xhat = torch.cat([dym3.t.float().flatten(), sums3.float(), ls3.float(), s23.float(), unit3, cdot3])
    assert torch.equal(no_xhat.view(torch.int32), outs[1][xh.t.numel():].view(torch.int32)), "outputs change when xhat is not asked for"
    print(f"recon {shape} kind {R.LOSSES[kind]} dtype {dtype} train {train}: share of |xhat - x| > 1: {share:.3f}")
    check_elt(xh.get(), ref["xhat"].reshape(rows, Cn), dtype, "xhat")
    check_red(_h(sums), ref["sums"], ref["sums_mag"], m["group"], "sums", "group")
    check_red(_h(ls)[0], ref["loss"], ref["loss_mag"], m["loss"], "loss sum", "loss")
    check_red(_h(ls)[1], ref["sq"], ref["sq"], m["loss"], "squared-error sum", "loss")
    if train:
        # Documented deviation: the kernels' tanh is one exp and one reciprocal, absolute error ~2e-7 (csrc/sgv_common.h), where the
        # float32 restatement has libm's.  A term dz = loss'(xhat - x) (1 - xhat^2) moves by at most TANH_ERR |d(dz)/d(xhat)| (the
        # derivative from autograd): the sums of dz get that much absolute room on top of their relative bound.
        S = TANH_ERR * ref["tanh_sens"]
        Sx, gam = S * np.abs(ref["xnorm"]), np.abs(gamma.astype(np.float64))
        gsum = lambda a: a.reshape(B, T, G, Cn // G).sum(axis=(1, 3))      # noqa: E731
        check_elt(dym.get(), ref["dy"].reshape(rows, Cn), dtype, "dy")
        check_red(_h(s2), ref["sums2"], ref["sums2_mag"], m["group"], "sums2", "group", np.stack((gsum(gam * S), gsum(gam * Sx)), -1))
        u = _h(unit).reshape(3, Cn)
        room = {"dgamma": Sx.sum(axis=(0, 1)), "dbeta": S.sum(axis=(0, 1)), "dbias_unit": 0.0}
        for k, name in enumerate(("dgamma", "dbeta", "dbias_unit")):
            check_red(u[k], ref[name], ref[name + "_mag"], m["column"], name, "column", room[name])
        check_red(_h(cdot)[0], ref["cdot"], ref["cdot_mag"], m["loss"], "cdot", "loss")


# Planted clamp values.  The set of the issue is split in two data sets so that each planted value can move a checked number:
#   "neg" (-40, -30, -29.9, 0): every KL term stays O(10), so the KL sum sees the lower clamps of lv and dlv; where the clamped
#       standard deviation is exp(-15) = 3e-7 the noise eps is 1e4, so that the reparameterisation term (3e-3 in z, 1.5e-3 |dz| in
#       the gradient) is far above its bound and a wrong `lv + dlv` mask or clamp shows;
#   "pos" (4.7, 29.9, 30, 40): exp(30) = 1e13 dominates the KL sum there (its upper clamps still show: exp(40) is 2e4 times that).
PLANTED = {1: (-40.0, -30.0, -29.9, 0.0), 2: (4.7, 29.9, 30.0, 40.0)}
BIG_EPS = 1e4


def planted_eps(eps, pos, vals):
    """eps = 1e4 where the planted log-variance is <= -29.9 (standard deviation 3e-7)"""
    for i, v in zip(pos, vals):
        if v <= -29.9:
            eps.reshape(-1)[i] = BIG_EPS * np.sign(eps.reshape(-1)[i])


def check_planted(got, ref, mag, dtype, pos, cancel, coef, what):
    """Gradient wrt the log-variances, flat positions `pos`: ordinary elements get the elementwise bound; every planted one is held
    to 2e-5 (bf16: + 2^-8) of the summed magnitudes of its two terms (reparameterisation, KL), tighter than the max-norm (the KL
    gradient reaches 1e13 at 30).  cancel: positions with lv = dlv >= 0, where the KL derivative 0.5 coef (1 - (dvar + df^2) ev /
    var^2) is the difference of two terms of size coef / 2 that agree to 1e-8: there, and only there, |coef| joins the scale.
    Returns the positions compared."""
    big = np.abs(ref) > 1e3                      # planted elements must not set the max-norm of the others
    assert set(np.flatnonzero(big.reshape(-1))) <= set(pos)
    check_elt(np.where(big, 0.0, got.reshape(ref.shape)), np.where(big, 0.0, ref), dtype, what)
    done = []
    for i in pos:
        g, r, sc = got.reshape(-1)[i], ref.reshape(-1)[i], mag.reshape(-1)[i] + (abs(coef) if i in cancel else 0.0)
        assert abs(g - r) <= (ELT32 + (2.0 ** -8 if dtype == 1 else 0.0)) * sc + 1e-30, f"{what}[{i}]: {g!r} vs {r!r} (scale {sc:.3e})"
        done.append(i)
    return done


@pytest.mark.parametrize("planted", [0, 1, 2])
@pytest.mark.parametrize("BZ", [(5, 7), (3, 32), (16, 33)])
def test_latent(BZ, planted):
    lib = E.load_library()
    torch = _torch()
    B, Z = BZ
    rng = np.random.default_rng(B * 100 + Z)
    lv, mu, eps, dz = (rng.standard_normal((B, Z)).astype(np.float32) for _ in range(4))
    vals = PLANTED.get(planted, ())
    pos = list(range(len(vals)))
    lv.reshape(-1)[pos] = np.array(vals, np.float32)
    planted_eps(eps, pos, vals)
    dz.reshape(-1)[pos] = 1.0
    last = np.concatenate([mu, lv], 1)
    coef = 0.37 / B
    ref = R.latent(last, eps, dz, coef)
    assert not (np.abs(np.abs(lv) - 30) < 0.09)[np.abs(lv) != 30].any() and not (np.abs(lv - 2 * np.log(10)) < 1e-3).any()
    last_d, eps_d, dz_d = _f(last), _f(eps), _f(dz)
    outs = []
    for rep in range(2):
        z, kl, dl = _nan(B * Z), _nan(1, torch.float64), _nan(2 * B * Z)
        _ok(lib, lib.sgv_test_latent(_p(last_d), _p(eps_d), _p(z), _p(kl), _p(dz_d), _p(dl), coef, B, Z, None))
        outs.append(torch.cat([z, kl.float(), dl]))
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32)), "replay differs"
    print(f"latent {BZ} planted {planted}")
    check_elt(_h(z), ref["z"].reshape(-1), 0, "z")
    check_red(_h(kl)[0], ref["kl"], ref["kl_mag"], R.f32_sum_error(np.float64(0.5) * (mu.astype(np.float64) ** 2))[0], "kl", "loss")
    idx = [(i // Z) * 2 * Z + Z + i % Z for i in pos]
    assert check_planted(_h(dl), ref["dlast"], ref["dlast_mag"], 0, idx, (), coef, "dlast") == idx
    g = dict(zip(vals, _h(dl).reshape(-1)[idx]))
    for v in vals:                               # beyond the clamp the gradient is exactly zero, on it and inside it is not
        assert (g[v] == 0) == (abs(v) > 30), (v, g[v])


@pytest.mark.parametrize("planted", [0, 1, 2])
@pytest.mark.parametrize("zmap", [0, 1])
@pytest.mark.parametrize("dtype,std_scale", [(0, 1.0), (1, 1.0), (0, 0.5), (1, 1e-10)])
@pytest.mark.parametrize("MC", [(30, 9), (600, 128), (37, 250)])
def test_stage(MC, dtype, std_scale, zmap, planted):
    """planted: the values go into lv at flat positions 0.. (dlv = -20 there in the "neg" set, so that exp(dlv) / (exp(lv) + 1e-8)
    stays small, and 0 in the "pos" set), into dlv at 16.. (lv = 0) and, halved into both, at 32.. (lv + dlv); mu = dmu at all of
    them ((mu - dmu) / var with var = 1e-8 would drown the other gradients)"""
    lib = E.load_library()
    torch = _torch()
    M, Cn = MC
    rng = np.random.default_rng(M * 1000 + Cn)
    lv, dlv, mu, dmu, eps, dzs, dec = (rng.standard_normal((M, Cn)).astype(np.float32) for _ in range(7))
    vals = PLANTED.get(planted, ())
    nv = len(vals)
    p_lv, p_dlv, p_sum = list(range(0, nv)), list(range(16, 16 + nv)), list(range(32, 32 + nv))
    if planted:
        v = np.array(vals, np.float32)
        lv.reshape(-1)[p_lv], dlv.reshape(-1)[p_lv] = v, (-20.0 if planted == 1 else 0.0)
        lv.reshape(-1)[p_dlv], dlv.reshape(-1)[p_dlv] = 0, v
        lv.reshape(-1)[p_sum], dlv.reshape(-1)[p_sum] = v / 2, v / 2
        dmu.reshape(-1)[p_lv + p_dlv + p_sum] = mu.reshape(-1)[p_lv + p_dlv + p_sum]
        planted_eps(eps, p_sum, vals)
        dzs.reshape(-1)[p_lv + p_dlv + p_sum] = 1.0
    if dtype == 1:
        dzs, dec = _bf16(dzs), _bf16(dec)
    kinks = (2 * np.log(10), 2 * np.log(10 / std_scale))      # where the standard deviation meets its upper clamp
    for k in kinks:                                            # ordinary values that land next to it move away by 0.25
        lv[np.abs(lv.astype(np.float64) + dlv - k) < 1e-3] += np.float32(0.25)
    pz, qz = np.concatenate([mu, lv], 1), np.concatenate([dmu, dlv], 1)
    inv_b, coef = 1.0 / 3, 0.21 / 3
    ref = R.stage(pz, qz, eps, dec, std_scale, inv_b, dzs, coef)
    s2 = lv.astype(np.float64) + dlv
    assert not (np.abs(s2 - 2 * np.log(10)) < 1e-3).any() and not (np.abs(s2 - 2 * np.log(10 / std_scale)) < 1e-3).any()
    if planted == 1:
        assert ref["kl_mag"] * 3 < 100 * M * Cn               # the KL terms stay O(10): the sum sees a wrong lower clamp (5 per element)
    pz_d, qz_d, eps_d = _f(pz), _f(qz), _f(eps)
    outs = []
    for rep in range(2):
        zs, gp, gq = Map(M, Cn, dtype), Map(M, 2 * Cn, dtype, pad=0), Map(M, 2 * Cn, dtype, pad=0)
        decm, dzm = Map(M, Cn, dtype, dec), Map(M, Cn, dtype, dzs)
        zm, kl, klp = (_nan(M * Cn) if zmap else None), _nan(1, torch.float64), _nan(2048, torch.float64)
        _ok(lib, lib.sgv_test_stage(dtype, _p(pz_d), _p(qz_d), _p(eps_d), decm.p, decm.ld, zs.p, zs.ld, _p(zm), std_scale, inv_b, _p(kl),
                                    _p(klp), dzm.p, dzm.ld, gp.p, gq.p, coef, M, Cn, None))
        outs.append(torch.cat([zs.t.float().flatten(), gp.t.float().flatten(), gq.t.float().flatten(), kl.float()] + ([zm] if zmap else [])))
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32)), "replay differs"
    print(f"stage {MC} dtype {dtype} std_scale {std_scale} zmap {zmap} planted {planted}")
    check_elt(zs.get(), ref["zs"], dtype, "zs_next")
    if zmap:
        check_elt(_h(zm), ref["z"].reshape(-1), 0, "zmap")
    check_red(_h(kl)[0], ref["kl"], ref["kl_mag"], R.f32_sum_error(np.float64(0.5) * (mu.astype(np.float64) - dmu) ** 2)[0], "kl", "loss")
    col = lambda i: (i // Cn) * 2 * Cn + Cn + i % Cn           # noqa: E731  flat position in the log-variance half of [M][2C]
    idx = [col(i) for i in p_lv + p_dlv + p_sum]
    cancel = [col(i) for i, v in zip(p_sum, vals) if v >= 0]
    assert check_planted(gp.get(), ref["g_p"], ref["g_p_mag"], dtype, idx, cancel, coef, "g_p") == idx
    assert check_planted(gq.get(), ref["g_q"], ref["g_q_mag"], dtype, idx, cancel, coef, "g_q") == idx
    if planted:
        gpf, gqf = gp.get().reshape(-1), gq.get().reshape(-1)
        for k, v in enumerate(vals):
            if abs(v) > 30:      # beyond a clamp: the KL term of that input and the reparameterisation term (lv + dlv is out too) vanish
                assert gpf[col(p_lv[k])] == 0 and gqf[col(p_dlv[k])] == 0, v
            elif v != 0:
                assert gpf[col(p_lv[k])] != 0 and gqf[col(p_dlv[k])] != 0, v
        if planted == 1:         # the reparameterisation term at lv + dlv = -40 (masked), -30 (on the edge: passes), -29.9
            rep = [abs(ref["g_p"].reshape(-1)[col(i)] - 0.5 * coef * (1 - 1 / (1 + 1e-8 / np.exp(float(v) / 2)) ** 2)) for i, v in zip(p_sum, vals)]
            bound = [ELT32 * ref["g_p_mag"].reshape(-1)[col(i)] for i in p_sum]
            assert rep[1] > 100 * bound[1] and rep[2] > 100 * bound[2], (rep, bound)    # a lost term would be 100 bounds away


@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("shape", [(2, 200, 128), (3, 37, 72), (1, 5, 2080)], ids=lambda s: "x".join(map(str, s)))
def test_act(shape, dtype):
    lib = E.load_library()
    torch = _torch()
    B, T, Cn = shape
    rows = B * T
    y, d, yf, _, _, cbias = gn_inputs(Cn + T, B, T, Cn, dtype)
    yf = (yf + np.float32(1e-3) * y).astype(np.float32)             # fp32 map of mode 2: not bf16-exact
    nws = lib.sgv_test_gn_workspace_floats(B, T, Cn)
    work, ym, dm, cbd, yfd = _nan(nws), Map(rows, Cn, dtype, y), Map(rows, Cn, dtype, d), _f(cbias), Map(rows, Cn, 0, yf)
    om = Map(rows, Cn, dtype)
    _ok(lib, lib.sgv_test_act(dtype, 0, ym.p, ym.ld, None, 0, 1.0, om.p, om.ld, None, None, None, None, 0, _p(work), nws, B, T, Cn, None))
    check_elt(om.get(), R.act_forward(y)["out"].reshape(rows, Cn), dtype, "gelu")
    for mode, with_db, with_dot, with_cb in [(1, 1, 1, 1), (1, 0, 0, 0), (1, 0, 1, 0), (1, 1, 0, 0), (2, 1, 1, 1), (2, 1, 0, 0), (2, 0, 1, 0)]:
        cb = cbias if with_cb else None
        ref = R.act_backward(y, d, 0.5, cb) if mode == 1 else R.colsum_dot(y, yf, cb)
        # the float32 restatement evaluates the terms in float32 too (five rows per column at T = 5: the terms' own rounding)
        if mode == 1:
            yt = torch.from_numpy(y).requires_grad_(True)
            torch.nn.functional.gelu(yt).sum().backward()
            t32 = (torch.from_numpy(d) * np.float32(0.5) * yt.grad).numpy()
        else:
            t32 = y
        t64 = ref["out"] if mode == 1 else y.astype(np.float64)
        w64 = (yf.astype(np.float64) if mode == 2 else y.astype(np.float64)) - (0.0 if cb is None else cb.astype(np.float64))
        m = {"column": R.f32_sum_error(t64.reshape(rows, Cn), 0, t32.reshape(rows, Cn))[0],
             "loss": R.f32_sum_error(t64 * w64, None, t32 * w64.astype(np.float32))[0]}
        outs = []
        for rep in range(2):
            om, db, cd = Map(rows, Cn, dtype), _nan(Cn), _nan(1)
            _ok(lib, lib.sgv_test_act(dtype, mode, ym.p, ym.ld, dm.p, dm.ld, 0.5, om.p, om.ld, _p(db) if with_db else None,
                                      _p(cd) if with_dot else None, _p(cbd) if with_cb else None, yfd.p, yfd.ld, _p(work), nws, B, T, Cn, None))
            outs.append(torch.cat([om.t.float().flatten(), db, cd]))
        assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32)), "replay differs"
        print(f"act {shape} dtype {dtype} mode {mode} dbias {with_db} cdot {with_dot} cbias {with_cb}")
        if mode == 1:
            check_elt(om.get(), ref["out"].reshape(rows, Cn), dtype, "out")
        else:
            assert bool(torch.isnan(om.t[:, :Cn]).all()), "mode 2 must not write out"
        if with_db:
            check_red(_h(db), ref["dbias"], ref["dbias_mag"], m["column"], "dbias", "column")
        else:
            assert bool(torch.isnan(db).all())
        if with_dot:
            check_red(_h(cd)[0], ref["cdot"], ref["cdot_mag"], m["loss"], "cdot", "loss")


def linear_measure(X, W, dY):
    """float32 re-summation error of the three sums of a Linear layer (over K, over the batch, over O): the worst of many outputs
    (all of them, or the first ones where there are millions), because the test takes the worst of all outputs too"""
    X, W, dY = (np.asarray(a, np.float64) for a in (X, W, dY))
    o4, k4 = min(W.shape[0], 4), min(W.shape[1], 4096)
    oK = min(W.shape[0], max(4, (1 << 22) // (X.shape[0] * W.shape[1])))      # about 4M terms
    mK = R.f32_sum_error(X[:, None, :] * W[None, :oK, :], axis=2)[0]
    mB = R.f32_sum_error(dY[:, :o4, None] * X[:, None, :k4], axis=0)[0]
    mO = R.f32_sum_error(dY[:, :, None] * W[None, :, :k4], axis=1)[0]
    return mK, mB, mO


@pytest.mark.parametrize("xdtype", [0, 1])
@pytest.mark.parametrize("BKO", [(1, 8, 1), (3, 1024, 16), (9, 95008, 64), (16, 4104, 16)])
def test_linear_head(BKO, xdtype):
    lib = E.load_library()
    torch = _torch()
    B, K, O = BKO
    rng = np.random.default_rng(K + O)
    X, add = (rng.standard_normal((B, K)).astype(np.float32) for _ in range(2))
    if xdtype == 1:
        X, add = _bf16(X), _bf16(add)
    W = (rng.standard_normal((O, K)) / np.sqrt(K)).astype(np.float32)
    bias, dY = rng.standard_normal(O).astype(np.float32), rng.standard_normal((B, O)).astype(np.float32)
    mK, mB, mO = linear_measure(X, W, dY)
    Xd, Wd, bd, dYd = Map(B, K, xdtype, X, pad=0), _f(W), _f(bias), _f(dY)
    addm = Map(B, K, xdtype, add, pad=0)
    part = _nan(128 * B * O)
    for sc, with_add, with_dx, with_dw in [(None, 0, 1, 1), (0.7, 1, 1, 1), (0.7, 0, 0, 1), (0.7, 1, 1, 0)]:
        scd = _f(np.array([sc], np.float32)) if sc is not None else None
        ref = R.linear(X, W, bias, sc or 1.0, dY, add if with_add else None)
        outs = []
        for rep in range(2):
            Y, dX, dW, db = _nan(B * O), Map(B, K, xdtype, pad=0), _nan(O * K), _nan(O)
            _ok(lib, lib.sgv_test_linear_head(xdtype, Xd.p, _p(Wd), _p(bd), _p(scd), _p(Y), _p(part), part.numel(), _p(dYd),
                                              addm.p if with_add else None, dX.p if with_dx else None, _p(dW) if with_dw else None,
                                              _p(db) if with_dw else None, B, K, O, None))
            outs.append(torch.cat([Y, dX.t.float().flatten(), dW, db]))
        assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32)), "replay differs"
        print(f"linear_head {BKO} xdtype {xdtype} scale {sc} addend {with_add} dX {with_dx} dW {with_dw}")
        check_red(_h(Y), ref["Y"], ref["Y_mag"], mK, "Y", "loss")
        if with_dx:
            if xdtype == 1:
                check_elt(dX.get(), ref["dX"], 1, "dX")
            else:
                check_red(dX.get(), ref["dX"], ref["dX_mag"], mO, "dX", "loss")
        else:
            assert bool(torch.isnan(dX.t).all())
        if not with_dw:
            assert bool(torch.isnan(dW).all()) and bool(torch.isnan(db).all())
            continue
        check_red(_h(dW), ref["dW"], ref["dW_mag"], mB, "dW", "loss")
        check_red(_h(db), ref["db"], ref["db_mag"], mB, "db", "loss")


@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("BKO", [(1, 8, 72), (5, 32, 200 * 128), (16, 64, 200 * 128), (5, 64, 10 * 72 + 8)])
def test_linear_expand(BKO, dtype):
    lib = E.load_library()
    torch = _torch()
    B, K, O = BKO
    rng = np.random.default_rng(K + O)
    X = rng.standard_normal((B, K)).astype(np.float32)
    W = (rng.standard_normal((O, K)) / np.sqrt(K)).astype(np.float32)
    bias, dY = rng.standard_normal(O).astype(np.float32), rng.standard_normal((B, O)).astype(np.float32)
    if dtype == 1:
        dY = _bf16(dY)
    mK, mB, mO = linear_measure(X, W, dY)
    Xd, Wd, bd, dYd = _f(X), _f(W), _f(bias), Map(B, O, dtype, dY, pad=0)
    for sc, with_dx in [(None, 1), (0.7, 1), (0.7, 0)]:
        scd = _f(np.array([sc], np.float32)) if sc is not None else None
        ref = R.linear(X, W, bias, sc or 1.0, dY)
        outs = []
        for rep in range(2):
            Y, dX, dW, db = Map(B, O, dtype, pad=0), _nan(B * K), _nan(O * K), _nan(O)
            _ok(lib, lib.sgv_test_linear_expand(dtype, _p(Xd), _p(Wd), _p(bd), _p(scd), Y.p, dYd.p, _p(dX) if with_dx else None, _p(dW), _p(db),
                                                B, K, O, None))
            outs.append(torch.cat([Y.t.float().flatten(), dX, dW, db]))
        assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32)), "replay differs"
        print(f"linear_expand {BKO} dtype {dtype} scale {sc} dX {with_dx}")
        if dtype == 1:
            check_elt(Y.get(), ref["Y"], 1, "Y")
        else:
            check_red(Y.get(), ref["Y"], ref["Y_mag"], mK, "Y", "loss")
        if with_dx:
            check_red(_h(dX), ref["dX"], ref["dX_mag"], mO, "dX", "loss")
        else:
            assert bool(torch.isnan(dX).all())
        check_red(_h(dW), ref["dW"], ref["dW_mag"], mB, "dW", "loss")
        check_red(_h(db), ref["db"], ref["db_mag"], mB, "db", "loss")


def test_hooks_reject_bad_arguments():
    lib = E.load_library()
    w = _nan(1 << 16)
    a = _nan(4096)
    path = C.c_int(0)
    for B, T, Cn, G, nws, y in [(1, 4, 12, 1, w.numel(), _p(a)), (1, 4, 64, 33, w.numel(), _p(a)), (1, 4, 64, 3, w.numel(), _p(a)),
                                (1, 4, 64, 8, 8, _p(a)), (1, 4, 64, 8, w.numel(), None)]:
        rc = lib.sgv_test_gn_fwd(0, 0, y, Cn, None, 0, 1.0, _p(a), Cn, _p(a), _p(a), _p(a), _p(w), nws, B, T, Cn, G, C.byref(path), None)
        assert rc == -1 and lib.sgv_last_error()
    assert lib.sgv_test_gn_bwd(0, 2, _p(a), 64, _p(a), 64, 1.0, 1.0, _p(a), _p(a), _p(a), _p(a), 64, _p(a), None, None, None, None, None, 0,
                               _p(w), w.numel(), 1, 4, 64, 8, C.byref(path), None) == -1
    from simulgen_vae_amd import ops
    assert ops.lib().sgv_op_gn_bwd(0, 2, _p(a), _p(a), _p(a), 1, 4, 64, 8, _p(a), _p(a), _p(a), _p(a), _p(w), _p(a), _p(a), None) != 0


def test_coverage_of_the_case_tables():
    """Coverage is a property of the case tables, and every case asserts what it was listed for: run_gn_case asserts the path each
    shape is listed with, test_recon_loss is parametrised over the full product, and the planted cases assert that every planted
    position was compared (check_planted returns them).  So this check needs no state from the other tests."""
    shapes = GN_SHAPES + [BIG]
    assert {s[4] for s in shapes} == {0, 1} and {s[5] for s in shapes} == {0, 1}
    marks = {m.args[0]: list(m.args[1]) for m in test_recon_loss.pytestmark if m.name == "parametrize"}
    assert marks["dtype"] == [0, 1] and marks["kind"] == [0, 1, 2, 3] and sorted(marks["train"]) == [0, 1]
    assert sorted(PLANTED[1] + PLANTED[2]) == sorted(R.LV_CLAMP_SET)
    for t in (test_latent, test_stage):
        assert [list(m.args[1]) for m in t.pytestmark if m.name == "parametrize" and m.args[0] == "planted"] == [[0, 1, 2]]
