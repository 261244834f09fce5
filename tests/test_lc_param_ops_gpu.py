"""The parameter side of the operator-level ABI (include/sgvae_ops.h; csrc/cnn.hip, csrc/pset.hip; simulgen_vae_amd/ops.py) against
float64 applied to the same fp32 inputs (tests/optim_reference.py, pinned to torch by tests/test_lc_param_reference_host.py): the
per-tensor spectral-norm chain (l2_normalize, dot, sgv_op_matvec_t, sn_power_iteration, sn_grad), conv_weight_pack / unpack, the
per-tensor optimizer tail (sumsq, clip_coef, adamw), multi_copy, cols_sub_div, gn_bwd(accumulate=False), the split-K combine behind
gemm_tn / conv2d_tn at chosen slab counts, and ops.ParamSet (the fused path) against float64 and against the per-tensor operators.

Every case: seeded inputs with magnitudes in [0.25, 1] x scale and random signs, outputs pre-filled with NaN, each output a slice
of a larger tensor whose other elements hold a canary that must survive bitwise (where the ops.* wrapper allocates the output
itself, the entry point is called on such a slice and the wrapper's own result must equal it bitwise), and a second launch on
restored inputs that must be bitwise equal (no operator here uses atomics).

Tolerances (none tuned on a kernel; U = 2^-24; helpers shared with tests/test_optim_kernels_gpu.py in tests/optim_checks.py,
whose docstring derives norm_bound, the sigma bound, e_g and check_update):
  * copies, permutations, pack / unpack, untouched buffers: bitwise;
  * fp32 reductions (matvec_t, the squared norm inside l2_normalize, the linear_fwd inside the power iteration, gemm_tn /
    conv2d_tn, the fused set's <G,W> and gradient norm): relative to the sum of the magnitudes of their terms,
    max(4 x measured, 2^-22), `measured` = ew_reference.f32_sum_error on the case's own terms, printed with every check; for
    gemm_tn at M = 65536 the terms of 16 outputs (the four corners and a seeded sample) are re-summed, not all 1152; bf16 cases
    take the terms of the rounded inputs;
  * sums accumulated in double (dot, sumsq): every product of two fp32 numbers is exact in double, so n 2^-53 x the sum of
    magnitudes covers any order of n additions; plus U |result| where the result is cast to fp32 (dot), plus 2^-53 |acc| for the
    one double addition onto the running total (sumsq);
  * l2_normalize: norm_bound with dx = 0 and the given eps; with the clamp active at eps = 0.5 the result is 2 x exactly;
  * per-tensor power iteration: v and u by norm_bound as in tests/test_optim_kernels_gpu.py.  sigma here is dot(u, W v) in
    double, not |s|^2 / max(|s|, eps):  |d sigma| <= sum(du |s| + |u| ds + du ds) + rows 2^-53 sum|u s| + U |sigma|  with ds the
    reduction bound of s = W v and du = norm_bound(s, ds);  1/sigma: 2 U / sigma (one division of the kernel's own sigma);
  * sn_grad_kernel: coef = gw * (1/sigma) is one fp32 product, formed here the same way in fp32 (exactly reproducible); then
    (G - coef u v) (1/sigma) is the operation sequence of e_g, so e_g = 2 U (|g| + |coef u v / sigma|) applies unchanged.  Against
    the full float64 chain the errors of the inputs are added: gw (a double-accumulated dot cast to fp32) and 1/sigma (U);
  * adamw_flat_kernel, read from csrc/cnn.hip: gi = g gs; pi = p (1 - lr wd); mi = m b1 + (1 - b1) gi; vi = v b2 + (1 - b2) gi gi;
    pi -= (lr / bc1) (mi / (sqrt(vi) / bc2s + eps)) -- the operations of SGV_ADAM1 in the same order, so check_update applies;
    bc1 = fl32(1 - b1^step), bc2s = fl32(sqrt(1 - b2^step)) are formed in double from the fp32 betas (the wrapper's own formula,
    not adam_coef's exact betas) and passed as the launch's own; one term is added to the increment, U lr wd |p|, the rounding of
    the product lr wd (the shared bound counts only the rounding of 1 - lr wd next to 1);
  * clip_coef: max_norm / (norm + 1e-6) formed in fp32 here; 2 U relative for the division;
  * cols_sub_div: one subtraction (U) and one division (2 U): (3 U + 2 U^2) |y|;
  * gn_bwd: the tolerance of test_groupnorm_relu in tests/test_ops_gpu.py (max(TOL[dt], 2e-4) relative, max norm), against
    float64 autograd;
  * ParamSet: the bounds above composed -- the set's sigma is |s|^2 / max(|s|, eps) (sigma_bound); <G,W>/sigma by the rule of
    check_dot in tests/test_optim_kernels_gpu.py; e_g gains |u v / sigma| e_cdot; the squared gradient norm is an fp32 reduction
    per 8192-element work item summed in double, with 2 |g| e_g + U g^2 per term, the norm itself |d n| <= d(n^2) / n + U n; the
    clip coefficient c = min(1, max_norm / (n + 1e-6)) moves by at most c (d n / n + 3 U) (the sum, the division, the cast), which
    enters e_g as |g| d c; the moments live inside the set, so the float64 moments are carried from step to step with their
    bounds (check_update's old_err).  The two GPU paths are bounded by the sum of their two bounds around the difference of
    their two float64 references: both start from the same numbers, but each reference takes its launch's own bias corrections
    (the set forms them from the exact betas, sgv_op_adamw from the fp32 ones), and from the second step on its path's own
    parameters and moments.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import simulgen_vae_amd  # noqa: F401
from simulgen_vae_amd import ops
from simulgen_vae_amd.ops import SgvError

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ew_reference as R  # noqa: E402
import optim_reference as O  # noqa: E402
from optim_checks import (B1, B2, LR, TINY, U, check_abs, check_red, check_update, mags, norm_bound, red_tol,  # noqa: E402
                          same, sigma_bound, sn_grad_bound, sq_err)

pytestmark = pytest.mark.gpu

CANARY = 768.0       # bf16-exact
PAD = 64             # canary elements on both sides of every buffer (256 bytes: the slice keeps the allocation's alignment)
D2 = 2.0 ** -53


class Buf:
    """n elements inside a larger tensor: PAD canary elements before and behind; data None: filled with NaN.  shift moves the
    slice by that many elements (off its 16-byte alignment)."""

    def __init__(self, data=None, n=None, dtype=torch.float32, shift=0):
        self.n = int(np.asarray(data).size if data is not None else n)
        self.lo = PAD + shift
        self.t = torch.full((self.lo + self.n + PAD,), CANARY, dtype=dtype, device="cuda")
        self.v = self.t[self.lo:self.lo + self.n]
        self.set(data)

    def set(self, data=None):
        if data is None:
            self.v.fill_(float("nan"))
        else:
            self.v.copy_(torch.from_numpy(np.ascontiguousarray(data).ravel()).to(self.t.dtype))

    def get(self, shape=None):
        assert bool((self.t[:self.lo].double() == CANARY).all()) and bool((self.t[self.lo + self.n:].double() == CANARY).all()), \
            "a canary next to a buffer was overwritten"
        a = self.v.double().cpu().numpy() if self.t.dtype == torch.float64 else self.v.float().cpu().numpy()
        return a.reshape(shape) if shape else a

    def bits(self):
        view = {torch.bfloat16: torch.int16, torch.float32: torch.int32, torch.float64: torch.int64}[self.t.dtype]
        return self.t.view(view).cpu().clone()


def raw(name, *args):
    rc = getattr(ops.lib(), name)(*args, ops._stream())
    if rc != 0:
        raise SgvError(f"{name} failed ({rc}): {ops.lib().sgv_last_error().decode()}")


def bits(t):
    return t.contiguous().view({torch.bfloat16: torch.int16, torch.float32: torch.int32, torch.float64: torch.int64}[t.dtype]).cpu()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ------------------------------------------------------------------------------------------------
# the spectral-norm chain, per tensor
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,cols", [(1, 1), (63, 5), (64, 256), (65, 257), (130, 300), (200, 1)])
def test_matvec_t(rows, cols):
    """out = W^T x: 1, 2, 3 and 4 row blocks of 64 (more than one goes through the partials and fin_rows), columns on both sides of 256"""
    rng = np.random.default_rng(1000 * rows + cols)
    W, x = mags(rng, (rows, cols)), mags(rng, rows)
    Wd, xd, out = dev(W), dev(x), Buf(n=cols)
    snaps = []
    for rep in range(2):
        out.set(None)
        raw("sgv_op_matvec_t", ops._p(Wd), ops._p(xd), ops._p(out.v), rows, cols)
        snaps.append(out.bits())
    assert same(snaps[:1], snaps[1:]), "replay differs"
    terms = O.f64(W) * O.f64(x)[:, None]
    m = R.f32_sum_error(terms, axis=0)[0]
    print(f"matvec_t {rows}x{cols}")
    check_red(out.get(), terms.sum(0), np.abs(terms).sum(0), m, "W^T x")


@pytest.mark.parametrize("n", [1, 3, 255, 256, 257, 1000])
def test_l2_normalize(n):
    rng = np.random.default_rng(n)
    x = mags(rng, n)
    xd, out = dev(x), Buf(n=n)
    raw("sgv_op_l2_normalize", ops._p(xd), ops._p(out.v), n, 1e-12)
    print(f"l2_normalize n={n}")
    tol_n = red_tol(sq_err(x))
    check_abs(out.get(), O.normalize(x), norm_bound(O.f64(x), 0.0, tol_n), "x / |x|")
    assert torch.equal(bits(ops.l2_normalize(xd)), bits(out.v)), "replay differs"
    # all zero: 0 / max(0, eps) = 0, not NaN
    out.set(None)
    z = torch.zeros(n, device="cuda")
    raw("sgv_op_l2_normalize", ops._p(z), ops._p(out.v), n, 1e-12)
    assert not out.get().any(), "the zero vector must give zeros"
    assert not ops.l2_normalize(z).cpu().numpy().any()
    # the clamp: |x| = 0.25 < eps = 0.5: out = x / 0.5, exactly 2 x
    h = (x * np.float32(0.25 / np.linalg.norm(O.f64(x)))).astype(np.float32)
    assert abs(np.linalg.norm(O.f64(h)) - 0.25) < 1e-6
    out.set(None)
    hd = dev(h)
    raw("sgv_op_l2_normalize", ops._p(hd), ops._p(out.v), n, 0.5)
    assert np.array_equal(out.get(), 2.0 * h), "with the clamp active the result is x / eps"
    assert torch.equal(bits(ops.l2_normalize(hd, eps=0.5)), bits(out.v))


def dot_bound(a, b):
    p = O.f64(a) * O.f64(b)
    return float(p.sum()), p.size * D2 * float(np.abs(p).sum()) + U * abs(float(p.sum()))


@pytest.mark.parametrize("n", [1, 7, 8192, 8193, 20000, 512 * 8192 + 5])
def test_dot(n):
    """one block up to 8192 elements (its partial goes straight into the scratch), 2 and 3 blocks, and the grid cap of 512: the
    last size needs the grid-stride loop"""
    rng = np.random.default_rng(n)
    a, b = mags(rng, n), mags(rng, n)
    ad, bd, out = dev(a), dev(b), Buf(n=4)
    raw("sgv_op_dot", ops._p(ad), ops._p(bd), ops._p(out.v), n)
    got = out.get()
    ref, tol = dot_bound(a, b)
    print(f"dot n={n}")
    check_abs(got[0], ref, tol, "a.b")
    check_abs(got[1], 1.0 / float(np.float32(got[0])), 2 * U / abs(got[0]), "1/(a.b) of the kernel's own a.b")
    assert torch.equal(bits(ops.dot(ad, bd)[:2]), bits(out.v[:2])), "replay differs"


def test_dot_rejects_a_misaligned_output():
    a = torch.ones(8, device="cuda")
    out = Buf(n=4, shift=1)
    before = out.bits()
    with pytest.raises(SgvError, match="8-byte aligned"):
        raw("sgv_op_dot", ops._p(a), ops._p(a), ops._p(out.v), 8)
    assert torch.equal(before, out.bits()), "a rejected call wrote"


def pi_bounds(W, u0, got_v):
    """float64 references and bounds of one power iteration on the plain matrix W: v from the inputs, s = W v and u from the
    kernel's own v"""
    W3 = O.as_taps(W)
    full = O.power_iteration(W3, u0, np.zeros(W.shape[1]), True)
    m_t = R.f32_sum_error(O.f64(W) * O.f64(u0)[:, None], axis=0)[0]
    dt = red_tol(m_t) * full["t_mag"]
    dv = norm_bound(full["t"], dt, red_tol(sq_err(full["t"])))
    s, s_mag = O.w_v(W3, got_v)
    m_s = R.f32_sum_error(O.f64(W) * O.f64(got_v)[None, :], axis=1)[0]
    ds = red_tol(m_s) * s_mag
    tol_ns = red_tol(sq_err(s))
    print(f"  float32 re-summation: t {m_t:.3e}, s {m_s:.3e}; |t| {np.linalg.norm(full['t']):.3e}, |s| {np.linalg.norm(s):.3e}")
    ds2 = ds + O.w_v(np.abs(O.f64(W3)), dv)[0]              # end to end: the bound of v carried through |W|
    return dict(full=full, dv=dv, s=s, ds=ds, tol_ns=tol_ns, du=norm_bound(s, ds, tol_ns), ds2=ds2, du2=norm_bound(full["s"], ds2, tol_ns))


def dot_sigma_bound(u, du, s, ds):
    """sigma = dot(u, s) accumulated in double from the kernel's fp32 u and s, cast to fp32"""
    u, s = np.abs(O.f64(u)), np.abs(O.f64(s))
    return float((du * s + u * ds + du * ds).sum()) + u.size * D2 * float((u * s).sum()) + U * float((u * s).sum())


@pytest.mark.parametrize("rows,cols", [(8, 12), (65, 257), (24, 72)])
def test_sn_power_iteration(rows, cols):
    rng = np.random.default_rng(100 * rows + cols)
    W, u0, v0 = mags(rng, (rows, cols)), mags(rng, rows, rows ** -0.5), mags(rng, cols, cols ** -0.5)
    Wb, ub, vb = Buf(W), Buf(u0), Buf(v0)
    Wm = Wb.v.view(rows, cols)
    snaps = []
    for rep in range(2):
        ub.set(u0)
        vb.set(None)                   # train: v is written before it is read
        sig = ops.sn_power_iteration(Wm, ub.v, vb.v, True)
        snaps.append([ub.bits(), vb.bits(), bits(sig[:2])])
    assert same(*snaps), "replay differs (train)"
    print(f"sn_power_iteration {rows}x{cols} train")
    got_v, got_u, got_sig = vb.get(), ub.get(), sig[:2].cpu().numpy()
    assert np.array_equal(Wb.get(), W.ravel()), "the weight was written"
    b = pi_bounds(W, u0, got_v)
    full = b["full"]
    check_abs(got_v, full["v"], b["dv"], "v vs float64 on the inputs")
    u_ref = O.normalize(b["s"])
    check_abs(got_u, u_ref, b["du"], "u vs float64 on the kernel's v")
    check_abs(got_sig[0], float((u_ref * b["s"]).sum()), dot_sigma_bound(u_ref, b["du"], b["s"], b["ds"]), "sigma vs float64 on the kernel's v")
    check_abs(got_sig[1], 1.0 / float(got_sig[0]), 2 * U / abs(got_sig[0]), "1/sigma")
    check_abs(got_u, full["u"], b["du2"], "u end to end")
    check_abs(got_sig[0], full["sigma"], dot_sigma_bound(full["u"], b["du2"], full["s"], b["ds2"]), "sigma end to end")
    ref = O.power_iteration(O.as_taps(W), u0, v0, True)
    check_abs(got_sig[0], ref["sigma"], dot_sigma_bound(full["u"], b["du2"], full["s"], b["ds2"]), "sigma vs optim_reference.power_iteration")
    # eval: u, v bitwise untouched, sigma from the given vectors
    ub.set(u0)
    vb.set(v0)
    before = [ub.bits(), vb.bits(), Wb.bits()]
    sig = ops.sn_power_iteration(Wm, ub.v, vb.v, False)
    assert same(before, [ub.bits(), vb.bits(), Wb.bits()]), "eval mode wrote u, v or W"
    ev = O.power_iteration(O.as_taps(W), u0, v0, False)
    m_s = R.f32_sum_error(O.f64(W) * O.f64(v0)[None, :], axis=1)[0]
    ds = red_tol(m_s) * ev["s_mag"]
    check_abs(sig[0].item(), ev["sigma"], dot_sigma_bound(u0, 0.0, ev["s"], ds), "sigma (eval)")


@pytest.mark.parametrize("rows,cols", [(1, 8), (5, 7), (24, 72), (33, 257)])
def test_sn_grad(rows, cols):
    rng = np.random.default_rng(10 * rows + cols)
    G, W = mags(rng, (rows, cols)), mags(rng, (rows, cols))
    u, v = mags(rng, rows, rows ** -0.5), mags(rng, cols, cols ** -0.5)
    sigma = np.float32(rng.uniform(0.8, 1.6))
    sig2 = np.array([sigma, np.float32(1.0) / sigma], np.float32)
    Gd, Wd, ud, vd, sd, out = dev(G), dev(W), dev(u), dev(v), dev(sig2), Buf(n=rows * cols)
    gw = ops.dot(Gd.reshape(-1), Wd.reshape(-1))                     # what ops.sn_grad computes first, read back
    raw("sgv_op_sn_grad", ops._p(Gd), ops._p(ud), ops._p(vd), ops._p(gw), ops._p(sd), ops._p(out.v), rows, cols)
    got = out.get((1, rows, cols))
    assert torch.equal(bits(ops.sn_grad(Gd, ud, vd, Wd, sd).reshape(-1)), bits(out.v)), "ops.sn_grad differs from the entry point on the same inputs"
    print(f"sn_grad {rows}x{cols}")
    gw0, inv = np.float32(gw[0].item()), sig2[1]
    ref_gw, tol_gw = dot_bound(G, W)
    check_abs(gw0, ref_gw, tol_gw, "<G, W>")
    cdot = float(np.float32(gw0 * inv))                                # the kernel's coef: one fp32 product
    go = O.chain_rule(O.as_taps(G), cdot, float(inv), u, v)
    e_g = sn_grad_bound(go, u, v, cdot, float(inv), (1, rows, cols))
    check_abs(got, go, e_g, "gradient wrt weight_orig vs float64 on the kernel's own <G,W> and 1/sigma")
    full = O.sn_backward(O.as_taps(G), O.as_taps(W), float(sigma), u, v)
    uv = np.abs(O.f64(u)[None, :, None] * O.f64(v)[None, None, :])
    e_full = (e_g + U * np.abs(O.f64(G))[None] * float(inv)                      # 1/sigma rounded, on the G term
              + uv * float(inv) ** 2 * tol_gw + uv * abs(ref_gw) * float(inv) ** 2 * 2.01 * U)      # <G,W>'s bound; 1/sigma twice on the u v^T term
    check_abs(got, full, e_full, "gradient vs the full float64 chain")


# ------------------------------------------------------------------------------------------------
# conv weight packing
# ------------------------------------------------------------------------------------------------
PACK_SHAPES = [(3, 1, 7, 7), (5, 3, 3, 3), (16, 8, 3, 3), (4, 2, 1, 1), (2, 5, 5, 3), (2, 3, 1, 4)]


@pytest.mark.parametrize("shape", PACK_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_conv_weight_pack_and_unpack(shape):
    cout, cin, kh, kw = shape
    rng = np.random.default_rng(sum(shape))
    w = mags(rng, shape)
    k = kh * kw * cin
    kp = (k + 7) // 8 * 8
    want = np.zeros((cout, kp), np.float32)
    want[:, :k] = torch.from_numpy(w).permute(0, 2, 3, 1).reshape(cout, -1).numpy()
    assert np.array_equal(want, O.conv_weight_pack(w))
    wd = dev(w)
    for dt, code in ((torch.float32, 0), (torch.bfloat16, 1)):
        out = Buf(n=cout * kp, dtype=dt)
        raw("sgv_op_conv_weight_pack", code, ops._p(wd), ops._p(out.v), cout, cin, kh, kw)
        got = out.get((cout, kp))
        assert not np.isnan(got).any(), "an element of the packed matrix was not written"
        assert torch.equal(bits(out.v), bits(torch.from_numpy(want).to(dt).reshape(-1))), f"pack {dt} is not the permutation (rounded to the dtype)"
        assert kp == k or not got[:, k:].any(), "the pad columns must be exactly zero"
        assert torch.equal(bits(ops.conv_weight_pack(wd, dt).reshape(-1)), bits(out.v)), "replay differs"
    back = Buf(n=w.size)
    packed = ops.conv_weight_pack(wd, torch.float32)
    raw("sgv_op_conv_weight_unpack", ops._p(packed), ops._p(back.v), cout, cin, kh, kw)
    assert np.array_equal(back.get(shape), w), "unpack(pack(w)) is not w"
    assert torch.equal(bits(ops.conv_weight_unpack(packed, shape)), bits(back.v.view(shape)))
    dirty = packed.clone()
    dirty[:, k:] = float("nan")
    got = ops.conv_weight_unpack(dirty, shape).cpu().numpy()
    assert np.array_equal(got, w), "unpack read a pad column"


# ------------------------------------------------------------------------------------------------
# the optimizer tail, per tensor
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 4095, 4096, 4097, 256 * 4096 + 3])
def test_sumsq(n):
    """4096 elements per block, the grid capped at 256 (the last size needs the grid-stride loop); the result is added onto
    the accumulator"""
    rng = np.random.default_rng(n)
    g = mags(rng, n)
    gd = dev(g)
    acc = Buf(np.zeros(1), dtype=torch.float64)
    assert acc.v.dtype == torch.float64
    ops.sumsq(gd, acc.v)
    first = acc.get()[0]
    S = float((O.f64(g) ** 2).sum())
    print(f"sumsq n={n}")
    check_abs(first, S, n * D2 * S, "sum g^2 onto 0")
    ops.sumsq(gd, acc.v)
    second = acc.get()[0]
    check_abs(second, first + S, n * D2 * S + D2 * (first + S), "a second call adds onto the first")
    assert second > 1.5 * first
    again = Buf(np.zeros(1), dtype=torch.float64)
    ops.sumsq(gd, again.v)
    assert again.get()[0] == first, "replay differs"


def test_clip_coef():
    """min(1, max_norm / (norm + 1e-6)) and the norm.  max_norm <= 0 means no clipping (coefficient 1) on both paths: the per-tensor
    path (LCOptimizer.clip_and_step with fused_params=False reads ops.clip_coef) and the fused one (ops.ParamSet.step, what
    production runs; pinned in test_param_set).  include/sgvae_ops.h states it for both."""
    def run(sumsq, max_norm):
        out = Buf(n=2)
        sq = dev(np.array([sumsq], np.float64))
        raw("sgv_op_clip_coef", ops._p(sq), C.c_float(max_norm), ops._p(out.v))
        got = out.get()
        assert torch.equal(bits(ops.clip_coef(sq, max_norm)), bits(out.v)), "replay differs"
        return got
    got = run(9.0, 10.0)
    assert got[0] == 1.0 and got[1] == 3.0, got
    for sumsq in (400.0, 401.5, 1e-30):
        got = run(sumsq, 10.0 if sumsq > 1 else 1e-20)
        tn = np.float32(np.sqrt(sumsq))
        assert got[1] == tn, (got, tn)
        want = np.float32(10.0 if sumsq > 1 else 1e-20) / np.float32(tn + np.float32(1e-6))
        assert want < 1.0
        check_abs(got[0], float(want), 2 * U * float(want), f"coefficient at sum g^2 = {sumsq}")
    for max_norm in (0.0, -1.0):
        got = run(401.5, max_norm)
        assert got[0] == 1.0 and got[1] == np.float32(np.sqrt(401.5)), f"max_norm = {max_norm} must mean no clipping, got {got}"


def op_coef(step):
    """sgv_op_adamw's bias corrections: in double from the fp32 betas"""
    return float(np.float32(1.0 - B1 ** step)), float(np.float32(np.sqrt(1.0 - B2 ** step)))


@pytest.mark.parametrize("gscale", [None, 0.37])
@pytest.mark.parametrize("wd", [0.0, 0.1])
@pytest.mark.parametrize("step", [1, 2, 1000])
def test_adamw(step, wd, gscale):
    wd = float(np.float32(wd))
    gs = None if gscale is None else float(np.float32(gscale))
    gs_dev = None if gscale is None else dev(np.array([gscale], np.float32))
    for n in (1, 255, 257, 70001):
        rng = np.random.default_rng(1000 * step + n + int(wd * 10) + (7 if gscale else 0))
        h = dict(p=mags(rng, n), g=mags(rng, n), m=mags(rng, n, 0.05), v=np.abs(mags(rng, n, 0.02)))
        if step == 1:
            h["m"], h["v"] = np.zeros(n, np.float32), np.zeros(n, np.float32)
        if n > 100:
            h["p"][n // 2] = 0.0          # the update at full fp32 precision
        b = {k: Buf(a) for k, a in h.items()}
        snaps = []
        for rep in range(2):
            for k in h:
                b[k].set(h[k])
            ops.adamw(b["p"].v, b["g"].v, b["m"].v, b["v"].v, LR, step, wd, gscale=gs_dev)
            snaps.append([x.bits() for x in b.values()])
        assert same(*snaps), "replay differs"
        print(f"adamw n={n} step {step} wd {wd} gscale {gscale}")
        got = {k: b[k].get() for k in ("p", "m", "v")}
        assert np.array_equal(b["g"].get(), h["g"]), "the gradient was written"
        r = check_update(f"n={n}", (1, 1, n), O.f64(h["g"]).reshape(1, 1, n), np.zeros((1, 1, n)), got, h, LR, wd, step, gs,
                         bc=op_coef(step), inc_extra=U * LR * wd * np.abs(O.f64(h["p"])).reshape(1, 1, n))
        if wd:          # the decay term alone is far above the bound: it cannot go missing unseen
            assert np.all(LR * wd * np.abs(h["p"][h["p"] != 0]) > 20 * r["e_inc"].ravel()[h["p"] != 0])


# ------------------------------------------------------------------------------------------------
# multi_copy, cols_sub_div, gn_bwd
# ------------------------------------------------------------------------------------------------
def test_multi_copy():
    """one launch over rows of 1, 3, 4, 1023 and 64*256*4 + 7 elements (past one sweep of the 64-block grid in float4s, with a
    scalar tail), plus rows whose source, destination or both sit one element off a 16-byte boundary (the scalar path)"""
    rng = np.random.default_rng(3)
    big = 64 * 256 * 4 + 7
    rows = [(1, 0, 0), (3, 0, 0), (4, 0, 0), (1023, 0, 0), (big, 0, 0), (1023, 1, 0), (big, 0, 1), (4, 1, 1), (1026, 1, 1)]
    gap = 8
    src_off, dst_off, so, do = [], [], gap, gap
    for cnt, s_shift, d_shift in rows:
        so = (so + 3) // 4 * 4 + s_shift
        do = (do + 3) // 4 * 4 + d_shift
        src_off.append(so)
        dst_off.append(do)
        so += cnt + gap
        do += cnt + gap
    src_h = mags(rng, so)
    src = dev(src_h)
    dst = torch.full((do,), CANARY, dtype=torch.float32, device="cuda")
    assert src.data_ptr() % 16 == 0 and dst.data_ptr() % 16 == 0
    pairs = [(src[a:a + c], dst[b:b + c]) for (c, _, _), a, b in zip(rows, src_off, dst_off)]
    assert [(s.data_ptr() % 16, d.data_ptr() % 16) for s, d in pairs[5:]] == [(4, 0), (0, 4), (4, 4), (4, 4)]
    want = np.full(do, CANARY, np.float32)
    for (c, _, _), a, b in zip(rows, src_off, dst_off):
        want[b:b + c] = src_h[a:a + c]
    snaps = []
    for rep in range(2):
        dst.fill_(CANARY)
        for _, d in pairs:
            d.fill_(float("nan"))
        keep = ops.multi_copy(pairs)
        snaps.append(bits(dst))
        del keep
    assert torch.equal(snaps[0], snaps[1]), "replay differs"
    assert np.array_equal(snaps[0].numpy().view(np.float32), want), "a destination differs from its source, or a canary between destinations was overwritten"
    assert np.array_equal(src.cpu().numpy(), src_h), "a source was written"


@pytest.mark.parametrize("rows,cols", [(1, 1), (9, 32), (7, 257)])
def test_cols_sub_div(rows, cols):
    rng = np.random.default_rng(rows * cols)
    x, mn, sc = mags(rng, (rows, cols)), mags(rng, cols), mags(rng, cols, 4.0)
    xd, md, sd, out = dev(x), dev(mn), dev(sc), Buf(n=rows * cols)
    raw("sgv_op_cols_sub_div", ops._p(xd), ops._p(md), ops._p(sd), ops._p(out.v), rows, cols)
    ref = (O.f64(x) - O.f64(mn)[None, :]) / O.f64(sc)[None, :]
    print(f"cols_sub_div {rows}x{cols}")
    check_abs(out.get((rows, cols)), ref, (3 * U + 2 * U * U) * np.abs(ref) + TINY, "(x - min) / scale")
    assert torch.equal(bits(ops.cols_sub_div(xd, md, sd).reshape(-1)), bits(out.v)), "replay differs"


GN_TOL = {torch.float32: 2e-5, torch.bfloat16: 2e-2}       # tests/test_ops_gpu.py


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("cfg", [(2, 32, 32, 36, 3), (3, 64, 32, 25, 0)])
def test_gn_bwd_set_and_accumulate(dt, cfg):
    """sgv_op_gn_bwd_set writes dgamma / dbeta into any buffer (NaN here); sgv_op_gn_bwd adds onto what is there (1.5 here)"""
    B, Cc, G, P, act = cfg
    g = torch.Generator().manual_seed(2)
    y = (torch.randn(B, Cc, P, generator=g) * 2 + 0.5).to(dt).double().requires_grad_()
    gamma = (torch.rand(Cc, generator=g) + 0.5).double().requires_grad_()
    beta = (torch.randn(Cc, generator=g) * 0.3).double().requires_grad_()
    o = F.group_norm(y, G, gamma, beta, 1e-5)
    if act == 3:
        o = F.relu(o)
    do = torch.randn(o.shape, generator=g).to(dt).double()
    o.backward(do)
    yd = y.detach().permute(0, 2, 1).contiguous().to(device="cuda", dtype=dt)
    dod = do.permute(0, 2, 1).contiguous().to(device="cuda", dtype=dt)
    gd, bd = gamma.detach().float().cuda(), beta.detach().float().cuda()
    _, sums = ops.gn_fwd(yd, G, gd, bd, act)
    tol = max(GN_TOL[dt], 2e-4)
    dgam, dbet = Buf(n=Cc), Buf(n=Cc)
    dy_set = ops.gn_bwd(yd, dod, G, gd, bd, sums, act, dgam.v, dbet.v, accumulate=False)
    e = (rel(dy_set.float().cpu().permute(0, 2, 1), y.grad), rel(torch.from_numpy(dgam.get()), gamma.grad), rel(torch.from_numpy(dbet.get()), beta.grad))
    print(f"gn_bwd set {cfg} {dt}: dy {e[0]:.3e} dgamma {e[1]:.3e} dbeta {e[2]:.3e} (tolerance {tol:.1e})")
    assert max(e) < tol, e
    agam, abet = Buf(np.full(Cc, 1.5, np.float32)), Buf(np.full(Cc, 1.5, np.float32))
    dy_acc = ops.gn_bwd(yd, dod, G, gd, bd, sums, act, agam.v, abet.v, accumulate=True)
    assert torch.equal(bits(dy_acc), bits(dy_set)), "dy differs between the two entry points"
    e = (rel(torch.from_numpy(agam.get()), gamma.grad + 1.5), rel(torch.from_numpy(abet.get()), beta.grad + 1.5))
    print(f"gn_bwd accumulate: dgamma {e[0]:.3e} dbeta {e[1]:.3e}")
    assert max(e) < tol, e
    # the accumulated result is the written one plus 1.5, to one fp32 rounding of the sum
    check_abs(agam.get(), O.f64(dgam.get()) + 1.5, U * (np.abs(O.f64(dgam.get())) + 1.5) * 2, "dgamma: accumulate vs set + 1.5")


# ------------------------------------------------------------------------------------------------
# the split-K combine behind gemm_tn / conv2d_tn
# ------------------------------------------------------------------------------------------------
def planned(dt, M, N1, N2, want):
    sk = int(ops.lib().sgv_op_gemm_tn_splitk(1 if dt == torch.bfloat16 else 0, M, N1, N2))
    assert sk == want, (f"sgv_op_gemm_tn_splitk({dt}, M={M}, N1={N1}, N2={N2}) = {sk}, this case was chosen for {want} slabs: the planner "
                        "changed, pick new shapes (1, a count > 4 that is no multiple of 4, and the cap of 256)")
    return sk


def check_tn(got, A, Bm, what):
    """got [N1][N2] against float64 A^T B of the (already rounded) operands; the float32 re-summation on 16 outputs when M is large"""
    A, Bm = O.f64(A), O.f64(Bm)
    M, N1 = A.shape
    N2 = Bm.shape[1]
    ref = A.T @ Bm
    mag = np.abs(A).T @ np.abs(Bm)
    if M * N1 * N2 <= 4e6:
        m = R.f32_sum_error(A[:, :, None] * Bm[:, None, :], axis=0)[0]
    else:
        rng = np.random.default_rng(M)
        ij = [(0, 0), (0, N2 - 1), (N1 - 1, 0), (N1 - 1, N2 - 1)] + [(int(rng.integers(N1)), int(rng.integers(N2))) for _ in range(12)]
        m = R.f32_sum_error(np.stack([A[:, i] * Bm[:, j] for i, j in ij], 1), axis=0)[0]
    check_red(got, ref, mag, m, what)


# (M, N1, N2, slabs in fp32, slabs in bf16): K-steps of 16 (fp32) / 32 (bf16) rows, at least 8 per slab, one 128x128 tile
TN_CASES = [(120, 16, 72, 1, 1), (1300, 16, 72, 10, 5), (1800, 24, 40, 14, 7), (65536, 16, 72, 256, 256)]


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("case", TN_CASES, ids=lambda c: "x".join(map(str, c[:3])))
def test_gemm_tn_split_k(dt, case):
    M, N1, N2, sk32, sk16 = case
    sk = planned(dt, M, N1, N2, sk32 if dt == torch.float32 else sk16)
    rng = np.random.default_rng(M + N1)
    A, Bm = torch.from_numpy(mags(rng, (M, N1))).to(dt), torch.from_numpy(mags(rng, (M, N2))).to(dt)
    Ad, Bd = A.cuda(), Bm.cuda()
    out = Buf(n=N1 * N2)
    slabs = Buf(n=sk * N1 * N2) if sk > 1 else None
    raw("sgv_op_gemm_tn", 1 if dt == torch.bfloat16 else 0, ops._p(Ad), ops._p(Bd), ops._p(out.v), M, N1, N2, ops._p(slabs.v) if slabs else None, sk)
    print(f"gemm_tn {M}x{N1}x{N2} {dt}: {sk} slabs")
    if slabs is not None:
        sl = slabs.get((sk, N1 * N2))
        assert np.isfinite(sl).all(), "a slab element was not written"
        check_red(out.get(), O.f64(sl).sum(0), np.abs(O.f64(sl)).sum(0), R.f32_sum_error(O.f64(sl), axis=0)[0],
                  "the combine against the float64 sum of the kernel's own slabs")
    check_tn(out.get((N1, N2)), A.float().numpy(), Bm.float().numpy(), "A^T B")
    assert torch.equal(bits(ops.gemm_tn(Ad, Bd).reshape(-1)), bits(out.v)), "replay differs"


# (B, H, W, Cin, Cout, k, slabs fp32, slabs bf16): M = B*H*W (stride 1, pad 1)
CONV_TN_CASES = [(1, 10, 10, 8, 16, 3, 1, 1), (1, 36, 36, 8, 16, 3, 10, 5), (4, 128, 128, 8, 16, 3, 256, 256)]


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("case", CONV_TN_CASES, ids=lambda c: "x".join(map(str, c[:6])))
def test_conv2d_tn_split_k(dt, case):
    B, H, W, Ci, Co, k, sk32, sk16 = case
    M, N2 = B * H * W, k * k * Ci
    sk = planned(dt, M, Co, N2, sk32 if dt == torch.float32 else sk16)
    rng = np.random.default_rng(M + 1)
    x = torch.from_numpy(mags(rng, (B, H, W, Ci))).to(dt)
    dy = torch.from_numpy(mags(rng, (B, H, W, Co))).to(dt)
    xd, dyd = x.cuda(), dy.cuda()
    got = ops.conv2d_tn(dyd, xd, k, k, 1, 1)
    assert torch.equal(bits(ops.conv2d_tn(dyd, xd, k, k, 1, 1)), bits(got)), "replay differs"
    print(f"conv2d_tn B={B} {H}x{W} Cin={Ci} Cout={Co} {k}x{k} {dt}: {sk} slabs")
    cols = F.unfold(x.double().permute(0, 3, 1, 2), k, padding=1)              # [B][(ci, kh, kw)][H*W]
    col = cols.view(B, Ci, k, k, H * W).permute(0, 4, 2, 3, 1).reshape(M, N2)    # [(b, oh, ow)][(kh, kw, ci)]
    check_tn(got.cpu().numpy(), dy.double().reshape(M, Co).numpy(), col.numpy(), "dY^T col")


# ------------------------------------------------------------------------------------------------
# ops.ParamSet: the fused path against float64 and against the per-tensor operators
# ------------------------------------------------------------------------------------------------
class RawDev:
    """a device address with the two methods ops.multi_copy reads"""

    def __init__(self, ptr, n):
        self.ptr, self.n = ptr, n

    def data_ptr(self):
        return self.ptr

    def numel(self):
        return self.n


ORDERS = {"normalised_first": [(8, 12), 4, (70, 260), 1028], "normalised_last": [4, 1028, (70, 260), (8, 12)]}


def make_entries(rng, order):
    ents = []
    for spec in order:
        sn = isinstance(spec, tuple)
        rows, cols = spec if sn else (0, 0)
        n = rows * cols if sn else spec
        e = dict(sn=sn, rows=rows, cols=cols, n=n, shape=(1, rows, cols) if sn else (1, 1, n), p0=mags(rng, n))
        e["p"], e["g"] = Buf(e["p0"]), Buf(n=n)
        if sn:
            e["u0"], e["v0"] = mags(rng, rows, rows ** -0.5), mags(rng, cols, cols ** -0.5)
            e["u"], e["v"] = Buf(e["u0"]), Buf(n=cols)
        ents.append(e)
    return ents


def pset_of(ents):
    return ops.ParamSet([dict(p=e["p"].v, g=e["g"].v, rows=e["rows"], cols=e["cols"], u=e["u"].v if e["sn"] else None,
                              v=e["v"].v if e["sn"] else None) for e in ents])


@pytest.mark.parametrize("order", list(ORDERS))
@pytest.mark.parametrize("mode", ["clip_at_step_2", "max_norm_0"])
def test_param_set(order, mode):
    rng = np.random.default_rng(len(order) + len(mode))
    wd = float(np.float32(0.1))
    ents = make_entries(rng, ORDERS[order])
    ps = pset_of(ents)
    # ---- power iteration; sigma through sigma_ptr ----
    ps.power_iteration(True)
    print(f"ParamSet {order} {mode}: power iteration")
    for k, e in enumerate(ents):
        if not e["sn"]:
            assert ps.sigma_ptr(k) == 0, "a plain entry has no sigma"
            continue
        sig = Buf(n=2)
        keep = ops.multi_copy([(RawDev(ps.sigma_ptr(k), 2), sig.v)])
        e["sig"], e["u1"], e["v1"] = sig.get(), e["u"].get(), e["v"].get()
        del keep
        W = e["p0"].reshape(e["rows"], e["cols"])
        assert np.array_equal(e["p"].get(), e["p0"]), "the power iteration wrote the weight"
        b = pi_bounds(W, e["u0"], e["v1"])
        full, s = b["full"], b["s"]
        check_abs(e["v1"], full["v"], b["dv"], f"entry {k} v vs float64 on the inputs")
        check_abs(e["u1"], O.normalize(s), b["du"], f"entry {k} u vs float64 on the kernel's v")
        sg = float((s * s).sum()) / max(float(np.linalg.norm(s)), O.SN_EPS)
        check_abs(e["sig"][0], sg, sigma_bound(s, b["ds"], b["tol_ns"]) * sg, f"entry {k} sigma vs float64 on the kernel's v")
        check_abs(e["sig"][1], 1.0 / float(e["sig"][0]), 2 * U / e["sig"][0], f"entry {k} 1/sigma")
        check_abs(e["u1"], full["u"], b["du2"], f"entry {k} u end to end")
        check_abs(e["sig"][0], full["sigma"], sigma_bound(full["s"], b["ds2"], b["tol_ns"]) * full["sigma"], f"entry {k} sigma end to end")
        # the per-tensor operator on a copy of the same tensors: u, v, sigma within the sum of the two bounds
        u2, v2 = dev(e["u0"]), torch.full((e["cols"],), float("nan"), device="cuda")
        sig2 = ops.sn_power_iteration(dev(W), u2, v2, True)
        check_abs(v2.cpu().numpy(), e["v1"], 2 * b["dv"], f"entry {k} v: per-tensor vs fused")
        check_abs(u2.cpu().numpy(), e["u1"], 2 * b["du2"], f"entry {k} u: per-tensor vs fused")
        check_abs(sig2[0].item(), e["sig"][0], sigma_bound(full["s"], b["ds2"], b["tol_ns"]) * full["sigma"]
                  + dot_sigma_bound(full["u"], b["du2"], full["s"], b["ds2"]), f"entry {k} sigma: per-tensor vs fused")
    # ---- the per-tensor path on copies, from the same u, v and sigma (its own power iteration is judged above) ----
    pt = [dict(p=dev(e["p0"]), m=torch.zeros(e["n"], device="cuda"), v=torch.zeros(e["n"], device="cuda")) for e in ents]
    # ---- three steps ----
    gscales = (1.0, 3.0, 1.0)
    n_all = sum(e["n"] for e in ents)
    # |g| of a tensor of n elements in [0.25, 1] is about 0.66 sqrt(n) (spectral-norm entries: divided by sigma, less the u v^T
    # part); the threshold sits between the scale-1 and the scale-3 norm; asserted below on the float64 norms
    max_norm = 0.0 if mode == "max_norm_0" else None
    mom = [dict(m=np.zeros(e["shape"]), v=np.zeros(e["shape"]), em=np.zeros(e["shape"]), ev=np.zeros(e["shape"])) for e in ents]
    clipped = []
    for step in (1, 2, 3):
        G = [mags(rng, e["n"], gscales[step - 1]) for e in ents]
        for e, g in zip(ents, G):
            e["g"].set(g)
        old = [e["p"].get().copy() for e in ents]
        old_pt = [t["p"].cpu().numpy() for t in pt]
        # float64 gradients wrt the original weights of both paths, and their bounds
        refs = []
        for k, (e, g) in enumerate(zip(ents, G)):
            both = []
            for p_now, fused in ((old[k], True), (old_pt[k], False)):
                g3 = O.f64(g).reshape(e["shape"])
                if not e["sn"]:
                    both.append((g3, np.zeros(e["shape"])))
                    continue
                inv = float(e["sig"][1])
                gw, gw_mag = O.grad_dot(g, p_now)
                uv = np.abs(O.f64(e["u1"])[None, :, None] * O.f64(e["v1"])[None, None, :]) * inv
                if fused:       # per-work-item fp32 partials times 1/sigma, added in fp32 (check_dot of tests/test_optim_kernels_gpu.py)
                    cdot = gw * inv
                    e_cdot = (red_tol(R.f32_sum_error(O.f64(g) * O.f64(p_now))[0]) + 2 * U) * gw_mag * inv
                else:           # double-accumulated dot cast to fp32, times 1/sigma in fp32
                    cdot = gw * inv
                    e_cdot = (e["n"] * D2 * gw_mag + U * abs(gw)) * inv + U * abs(cdot)
                go = O.chain_rule(g3, cdot, inv, e["u1"], e["v1"])
                both.append((go, sn_grad_bound(go, e["u1"], e["v1"], cdot, inv, e["shape"]) + uv * e_cdot))
            refs.append(both)
        # the norm of the chain-ruled gradients, as clip_grad_norm_ sees weight_orig.grad
        norm_ref, e_norm = [], []
        for which in (0, 1):
            terms = np.concatenate([(r[which][0] ** 2).ravel() for r in refs])
            extra = sum(float((2 * np.abs(r[which][0]) * r[which][1] + U * r[which][0] ** 2).sum()) for r in refs)
            S = float(terms.sum())
            m = R.f32_sum_error(terms)[0]
            e_sq = (red_tol(m) if which == 0 else n_all * D2) * S + extra
            norm_ref.append(np.sqrt(S))
            e_norm.append(e_sq / np.sqrt(S) + U * np.sqrt(S))
            if which == 0:
                print(f"  step {step}: gradient norm {np.sqrt(S):.6f}, float32 re-summation of its terms {m:.3e}")
        if max_norm is None:
            max_norm = float(np.float32(2.0 * norm_ref[0]))         # step 1 (scale 1) stays below it, step 2 (scale 3) goes above
        # ---- fused ----
        total = ps.step(LR, wd, max_norm)
        check_abs(total, norm_ref[0], e_norm[0], f"step {step} total norm (fused)")
        # ---- per tensor ----
        acc = torch.zeros(1, dtype=torch.float64, device="cuda")
        g_pt = []
        for k, (e, g) in enumerate(zip(ents, G)):
            gd = dev(g)
            if e["sn"]:
                gd = ops.sn_grad(gd.view(e["rows"], e["cols"]), dev(e["u1"]), dev(e["v1"]), pt[k]["p"].view(e["rows"], e["cols"]),
                                 dev(e["sig"])).reshape(-1)
            g_pt.append(gd)
            ops.sumsq(gd, acc)
        cf = ops.clip_coef(acc, max_norm)
        check_abs(cf[1].item(), norm_ref[1], e_norm[1], f"step {step} total norm (per tensor)")
        for k in range(len(ents)):
            ops.adamw(pt[k]["p"], g_pt[k], pt[k]["m"], pt[k]["v"], LR, step, wd, gscale=cf)
        # ---- the clip coefficient in float64, and what its error adds to every gradient ----
        c_ref, e_c = [], []
        for which in (0, 1):
            c = O.clip_coef(norm_ref[which], max_norm) if max_norm > 0 else 1.0
            c_ref.append(c)
            e_c.append(c * (e_norm[which] / norm_ref[which] + 3 * U) if c < 1.0 or norm_ref[which] + e_norm[which] > max_norm > 0 else 0.0)
        clipped.append(c_ref[0] < 1.0)
        assert abs(norm_ref[0] - max_norm) > 100 * e_norm[0], "the threshold sits too close to a norm for the case to be decided"
        for k, e in enumerate(ents):
            tag = f"step {step} entry {k} {e['shape']}"
            g0, eg0 = refs[k][0]
            r0 = check_update(tag + " fused", e["shape"], g0, eg0 + np.abs(g0) * e_c[0], dict(p=e["p"].get()),
                              dict(p=old[k], m=mom[k]["m"], v=mom[k]["v"]), LR, wd, step, c_ref[0],
                              inc_extra=U * LR * wd * np.abs(O.f64(old[k])).reshape(e["shape"]), old_err=dict(m=mom[k]["em"], v=mom[k]["ev"]))
            mom[k] = dict(m=r0["m"], v=r0["v"], em=r0["e_m"], ev=r0["e_v"])
            g1, eg1 = refs[k][1]
            got1 = {q: pt[k][q].cpu().numpy() for q in ("p", "m", "v")}
            m_in, v_in = e.get("pt_mv", (np.zeros(e["n"], np.float32), np.zeros(e["n"], np.float32)))
            r1 = check_update(tag + " per tensor", e["shape"], g1, eg1 + np.abs(g1) * e_c[1], got1, dict(p=old_pt[k], m=m_in, v=v_in),
                              LR, wd, step, c_ref[1], bc=op_coef(step), inc_extra=U * LR * wd * np.abs(O.f64(old_pt[k])).reshape(e["shape"]))
            e["pt_mv"] = (got1["m"], got1["v"])
            # the two GPU paths: the sum of their bounds around the difference of their float64 references (zero at step 1)
            inc0 = O.f64(e["p"].get()) - O.f64(old[k])
            inc1 = O.f64(got1["p"]) - O.f64(old_pt[k])
            d_ref = ((r0["p"] - O.f64(old[k]).reshape(e["shape"])) - (r1["p"] - O.f64(old_pt[k]).reshape(e["shape"]))).ravel()
            if step == 1:
                assert np.array_equal(old[k], old_pt[k]), "both paths start from the same numbers"
            check_abs(inc0 - inc1, d_ref, (r0["e_inc"] + r1["e_inc"]).ravel(), tag + " fused vs per tensor")
            if wd:
                nz = old[k] != 0
                assert np.all(LR * wd * np.abs(old[k][nz]) > 20 * r0["e_inc"].ravel()[nz]), "weight decay would hide inside the bound"
            assert np.array_equal(e["g"].get(), G[k]), "the set wrote a gradient buffer"
            if e["sn"]:
                assert np.array_equal(e["u"].get(), e["u1"]) and np.array_equal(e["v"].get(), e["v1"]), "the step wrote u or v"
    assert clipped == ([False, True, False] if mode == "clip_at_step_2" else [False, False, False]), clipped
    ps.close()


def test_param_set_rejects_bad_entries_before_any_launch():
    rng = np.random.default_rng(2)
    p, g, u, v = Buf(mags(rng, 32)), Buf(mags(rng, 32)), Buf(mags(rng, 4)), Buf(mags(rng, 8))
    p1, g1 = Buf(mags(rng, 32), shift=1), Buf(mags(rng, 32), shift=1)
    good = dict(p=p.v, g=g.v, rows=4, cols=8, u=u.v, v=v.v)
    ops.ParamSet([good]).close()
    bad = {
        "n % 4": dict(p=p.v[:30], g=g.v[:30]),
        "p off 16 bytes": dict(p=p1.v, g=g.v),
        "g off 16 bytes": dict(p=p.v, g=g1.v),
        "rows * cols != n": dict(good, rows=4, cols=4),
        "cols % 4": dict(p=p.v[:24], g=g.v[:24], rows=4, cols=6, u=u.v, v=v.v),
        "no u": dict(good, u=None),
        "no v": dict(good, v=None),
    }
    before = [x.bits() for x in (p, g, u, v, p1, g1)]
    for what, e in bad.items():
        with pytest.raises(SgvError, match="sgv_pset_create"):
            ops.ParamSet([good, e])
        print(f"  rejected: {what}")
    assert same(before, [x.bits() for x in (p, g, u, v, p1, g1)]), "a rejected create wrote to a buffer"
