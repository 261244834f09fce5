"""Kernel-level parity of csrc/optim.hip (spectral-norm power iteration, the <G,W> dot, both AdamW kernels, the gradient-norm pass,
the weight-copy kernels) against tests/optim_reference.py (float64), through the sgv_test_optset_* hook: the hook builds its
descriptor and work-item tables with the host helpers of csrc/sgv_ew.h the engine uses and calls the engine's launchers.

Every case: seeded inputs with magnitudes in [0.25, 1] x scale and random signs (nothing but the planted zeros is below 1e-30, so
no result depends on fp32 denormal handling), outputs pre-filled with NaN (the hook's own scratch too), 64 canary elements behind
every buffer that must survive, and a second launch on restored inputs that must be bitwise equal (nothing here uses atomics).

Tolerances (none tuned on the kernels; U = 2^-24 is the largest relative error of one correctly rounded fp32 operation):
  * copies (wc, wct) and untouched buffers: bitwise;
  * reductions (t = W^T u, s = W v, both squared norms, sigma, the dot, the gradient norm): relative to the sum of the magnitudes
    of their terms, max(4 x measured, 2^-22), `measured` = ew_reference.f32_sum_error on the case's own terms, printed with
    every check (the rule of tests/test_ew_kernels_gpu.py);
  * v = t / max(|t|, 1e-12) and u likewise (norm_bound): |dv_i| <= dt_i / N + |v_i| (tol_norm + |dt|_2 / N + 4 U), dt the reduction
    bound of t, N the clamped norm, |dt|_2 / N how far the kernel's norm moves because it is taken of the kernel's own t, 4 U for
    sqrt, the cast, the reciprocal and the product.  sigma = |s|^2 / max(|s|, 1e-12): 1.5 (tol_norm + 2 |ds|_2 / |s|) + 3 U
    relative (the factor 1.5 covers the clamped and the unclamped quotient).  u and sigma are compared with float64 applied to
    the kernel's own v (read back) and the operand the kernel read (the bf16 copy's values where it reads the copy: bf16 rounding
    is not part of any bound); the end-to-end float64 chain is compared too, with the bound of v propagated through |W| added;
  * elementwise AdamW, per element, from the operations of SGV_ADAM1 (check_update; fused multiply-adds only remove roundings):
      g (spectral-norm entries, g = (G - (u cdot) v) / sigma): e_g = 2 U (|g| + |u cdot v / sigma|)
          -- u * cdot, * v (carrying the first), the subtraction (carrying both), * 1/sigma: each product term is rounded twice,
             the difference twice; the float64 formula takes the kernel's own 1/sigma and summed dot, whose reductions are
             judged in their own checks;
      clip: g * gscale adds U |g gscale|;
      m: 3 U (|m| b1 + (1 - b1) |g|) + (1 - b1) e_g      -- two products, one sum (1 - b1 is exact in fp32);
      v: 3 U v_new + 2 (1 - b2) |g| e_g + (1 - b2) e_g^2  -- (1 - b2) g, * g, v b2, the sum: at most 3 roundings on positive terms;
      update = (lr / bc1) m / (sqrt(v) / bc2sqrt + eps): (lr / bc1) e_m / denom + |update| (e_v / (2 v_new) + 9 U)
          -- sqrt 2 U, / bc2sqrt 2 U, + eps U (5 U on the denominator), the quotient 2 U, lr / bc1 U, the product U;
      increment p_new - p_old: e_update + 2^-25 |p| (decay = 1 - lr wd rounded next to 1) + U |p decay| (the product) + U |p_new|
          (the final subtraction); the first two vanish for wd = 0.  The increment, not p_new, is compared: a check relative to
          |p| would hide the update.
    The float64 reference takes the launch's own fp32 arguments as exact numbers (lr, wd, eps, bc1, bc2sqrt, and b1 = fl32(0.9),
    b2 = fl32(0.999) -- the kernel forms 1 - b2 from the fp32 beta, 1.3e-5 below 0.001; tests/test_optim_reference_host.py pins
    the same formula to torch.optim.AdamW at the exact betas).
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
import optim_reference as O  # noqa: E402
from optim_checks import (B1, B2, EPS, LR, TINY, U, check_abs, check_red, check_update, coef, mags, norm_bound, red_tol,  # noqa: E402
                          same, sigma_bound, sn_grad_bound, sq_err)

pytestmark = pytest.mark.gpu

CANARY = 768.0       # bf16-exact
PAD = 64
F32, BF16 = 0, 1


def _torch():
    import torch
    return torch


def _ok(lib, rc):
    assert rc == 0, lib.sgv_last_error().decode()


class Buf:
    """device array of n elements followed by PAD canary elements; data None: filled with NaN"""

    def __init__(self, data=None, n=None, bf16=False):
        torch = _torch()
        self.n = int(np.asarray(data).size if data is not None else n)
        self.t = torch.full((self.n + PAD,), CANARY, dtype=torch.bfloat16 if bf16 else torch.float32, device="cuda")
        self.set(data)

    def set(self, data=None):
        torch = _torch()
        if data is None:
            self.t[:self.n] = float("nan")
        else:
            self.t[:self.n] = torch.from_numpy(np.ascontiguousarray(data, np.float32).ravel()).cuda().to(self.t.dtype)

    @property
    def p(self):
        return self.t.data_ptr()

    def get(self, shape=None):
        assert bool((self.t[self.n:].float() == CANARY).all()), "the canary behind a buffer was overwritten"
        a = self.t[:self.n].float().cpu().numpy()
        return a.reshape(shape) if shape else a

    def bits(self):
        torch = _torch()
        return self.t.view(torch.int16 if self.t.dtype == torch.bfloat16 else torch.int32).cpu().clone()


class Ent:
    """one tensor of an optimizer set: host copies of the inputs and the device buffers"""

    def __init__(self, rng, dtype, n=None, taps=1, rows=0, cols=0, tiled=False, wc=False, wct=False, g_bf16=False, active=True,
                 w_scale=1.0, g_ext=None, bf16_grad=False):
        self.dtype, self.taps, self.rows, self.cols, self.tiled, self.active = dtype, taps, rows, cols, tiled, active
        self.sn = rows > 0
        self.n = n if not self.sn else taps * rows * cols
        self.shape = (taps, rows, cols) if self.sn else (1, 1, self.n)
        n = self.n
        self.h = dict(p=mags(rng, n, w_scale), g=mags(rng, n), m=mags(rng, n, 0.05), v=np.abs(mags(rng, n, 0.02)))
        if bf16_grad:
            self.h["g"] = O.bf16_round(self.h["g"])
        self.b = {k: Buf(a) for k, a in self.h.items() if not (k == "g" and g_ext)}
        self.g_ext = g_ext              # (pointer, None): the gradient lives in a caller's arena
        if self.sn:
            sig = float(rng.uniform(0.8, 1.6))
            dot = np.zeros(32, np.float32)
            dot[0] = np.float32(O.grad_dot(self.h["g"], self.h["p"])[0] / sig)        # what the conv kernels would have left
            self.h.update(u=mags(rng, rows, rows ** -0.5), v_sn=mags(rng, taps * cols, (taps * cols) ** -0.5),
                          sigma=np.array([sig, 1.0 / sig], np.float32), dot=dot)
            for k in ("u", "v_sn", "sigma", "dot"):
                self.b[k] = Buf(self.h[k])
        self.b["wc"] = Buf(n=n, bf16=dtype == BF16) if wc else None
        self.b["wct"] = Buf(n=n, bf16=dtype == BF16) if wct else None
        self.b["g_bf16"] = Buf(n=n, bf16=True) if g_bf16 else None
        self.wc_init = None             # values to put into wc on restore (power-iteration tests), else NaN

    def restore(self):
        for k, a in self.h.items():
            if k in self.b:
                self.b[k].set(a)
        for k in ("wc", "wct"):
            if self.b[k] is not None:
                self.b[k].set(self.wc_init if k == "wc" else None)

    def centry(self):
        e = E.OptsetEntry()
        for k in ("p", "m", "v", "u", "v_sn", "sigma", "dot", "wc", "wct", "g_bf16"):
            setattr(e, k, self.b[k].p if self.b.get(k) is not None else None)
        e.g = self.g_ext if self.g_ext else self.b["g"].p
        e.n, e.taps, e.rows, e.cols, e.tiled, e.active = self.n, self.taps, self.rows, self.cols, int(self.tiled), int(self.active)
        return e

    def snapshot(self):
        return [b.bits() for b in self.b.values() if b is not None]


class Set:
    def __init__(self, dtype, ents):
        self.lib, self.ents, self.h = E.load_library(), ents, C.c_void_p()
        arr = (E.OptsetEntry * len(ents))(*[e.centry() for e in ents])
        _ok(self.lib, self.lib.sgv_test_optset_create(dtype, arr, len(ents), C.byref(self.h)))

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.lib.sgv_test_optset_destroy(self.h)

    def power_iteration(self, train, reuse=0):
        _ok(self.lib, self.lib.sgv_test_optset_power_iteration(self.h, train, reuse, None))

    def grad_dot(self):
        _ok(self.lib, self.lib.sgv_test_optset_grad_dot(self.h, None))

    def grad_norm(self):
        out = C.c_double(float("nan"))
        _ok(self.lib, self.lib.sgv_test_optset_grad_norm(self.h, C.byref(out), None))
        return out.value

    def adamw(self, lr, wd, step, gscale=None, source=0, g_base=None, g_wire=None, wire_elems=0):
        out = C.c_double(float("nan"))
        _ok(self.lib, self.lib.sgv_test_optset_adamw(self.h, lr, wd, step, gscale, source, g_base, g_wire, wire_elems, C.byref(out), None))
        return out.value

    def make_copies(self):
        _ok(self.lib, self.lib.sgv_test_optset_make_copies(self.h, None))

    def restore(self):
        for e in self.ents:
            e.restore()

    def snapshot(self):
        return [b for e in self.ents for b in e.snapshot()]


# ------------------------------------------------------------------------------------------------
# power iteration
# ------------------------------------------------------------------------------------------------
# (taps, rows, cols): what the case is for.  Row blocks are 64 rows, column blocks 1024 columns; sn_tsum_kernel walks the row
# blocks on 16 lanes (four chains while lane + 48 < blocks left), sn_ssum_kernel the taps * ceil(cols / 1024) partials on 4 lanes.
PI_SHAPES = [
    (1, 4, 4),          # smallest; both vectors far below 1024
    (1, 63, 12),        # one short row block; cols % 8 != 0: bf16 engines read the master
    (1, 64, 64),        # exactly one row block; taps * cols = 64: one full chunk of the t sum; bf16 copy read
    (1, 65, 68),        # one row past the block; taps * cols = 68: a second, short chunk
    (3, 130, 20),       # three taps, three row blocks, taps * cols = 60
    (2, 4, 1020),       # cols one vector below the column block
    (1, 4, 1024),       # exactly one column block; bf16 copy read over the whole block
    (1, 8, 1028),       # second column block of one vector
    (2, 4, 2052),       # 6 partials of W v (> 4 lanes); v has 4104 > 4096 elements
    (5, 4, 1028),       # taps * ceil(cols / 1024) = 10 partials
    (2, 6, 1032),       # bf16 copy read across a column-block edge (cols % 8 == 0, second block of 8)
    (1, 64 * 16 + 3, 8),    # 17 row blocks: single-chain loop, two trips on lane 0
    (1, 64 * 17 + 3, 8),    # 18
    (1, 64 * 48 + 3, 8),    # 49: lane 0 enters the four-chain loop
    (1, 64 * 49 + 3, 8),    # 50: lanes 0 and 1
    (1, 64 * 64 + 3, 8),    # 65: every lane in the four-chain loop, lane 0 has a remainder; u has 4099 > 4096 elements
    (1, 64 * 113 + 3, 8),   # 114: second trip of the four-chain loop on lanes 0 and 1
]


def pi_entry(rng, dtype, shape, wc_mode, w_scale=1.0, active=True):
    taps, rows, cols = shape
    e = Ent(rng, dtype, taps=taps, rows=rows, cols=cols, wc=wc_mode is not None, active=active, w_scale=w_scale)
    if wc_mode is not None:
        e.wc_init = O.bf16_round(2.0 * e.h["p"]) if dtype == BF16 else 2.0 * e.h["p"]      # deliberately NOT the copy of W
        e.restore()
    return e


def pi_operand(e):
    """the operand the W v pass must read: the copy for bf16 sets with a copy and cols % 8 == 0, else the master"""
    W = e.h["p"].reshape(e.shape)
    if e.dtype == BF16 and e.wc_init is not None and e.cols % 8 == 0:
        return e.wc_init.reshape(e.shape), True
    return W, False


def check_pi_train(e, got_v, got_u, got_sigma):
    W, u0 = e.h["p"].reshape(e.shape), e.h["u"]
    Wv, copy = pi_operand(e)
    full = O.power_iteration(W, u0, e.h["v_sn"], True, Wv)
    # v against float64 on the inputs
    m_t = R.f32_sum_error(O.f64(W) * O.f64(u0)[None, :, None], axis=1)[0]
    dt = red_tol(m_t) * full["t_mag"]
    tol_nt = red_tol(sq_err(full["t"]))
    dv = norm_bound(full["t"], dt, tol_nt)
    print(f"  t: float32 re-summation {m_t:.3e}; |t| {np.linalg.norm(full['t']):.3e}")
    check_abs(got_v, full["v"], dv, "v vs float64 on the inputs")
    # u, sigma against float64 on the kernel's own v and the operand it read
    s, s_mag = O.w_v(Wv, got_v)
    m_s = R.f32_sum_error(O.f64(Wv) * O.f64(got_v).reshape(e.taps, 1, e.cols), axis=(0, 2))[0]
    ds = red_tol(m_s) * s_mag
    tol_ns = red_tol(sq_err(s))
    print(f"  s: float32 re-summation {m_s:.3e}; |s| {np.linalg.norm(s):.3e}; W v read the {'bf16 copy' if copy else 'master'}")
    check_abs(got_u, O.normalize(s), norm_bound(s, ds, tol_ns), "u vs float64 on the kernel's v")
    sig = float((s * s).sum()) / max(float(np.linalg.norm(s)), O.SN_EPS)
    check_abs(got_sigma[0], sig, sigma_bound(s, ds, tol_ns) * abs(sig), "sigma vs float64 on the kernel's v")
    if sig > 0:
        check_abs(got_sigma[1], 1.0 / float(np.float32(got_sigma[0])), 2 * U / abs(got_sigma[0]), "1/sigma")
    # which operand: the other one gives a sigma a factor 2 away
    if e.wc_init is not None and sig > 0:
        other = O.power_iteration(W, u0, e.h["v_sn"], True, W if copy else e.wc_init.reshape(e.shape))["sigma"]
        assert abs(got_sigma[0] - other) > 0.25 * abs(sig), "the W v pass read the wrong operand"
    # end to end: the bound of v carried through |Wv|
    ds2 = ds + O.w_v(np.abs(O.f64(Wv)), dv)[0]
    check_abs(got_u, full["u"], norm_bound(full["s"], ds2, tol_ns), "u end to end")
    check_abs(got_sigma[0], full["sigma"], sigma_bound(full["s"], ds2, tol_ns) * abs(full["sigma"]), "sigma end to end")


def check_pi_eval(e, got_sigma):
    Wv, _ = pi_operand(e)
    u0 = O.f64(e.h["u"])
    s, s_mag = O.w_v(Wv, e.h["v_sn"])
    m_s = R.f32_sum_error(O.f64(Wv) * O.f64(e.h["v_sn"]).reshape(e.taps, 1, e.cols), axis=(0, 2))[0]
    m_d = R.f32_sum_error(u0 * s)[0]
    tol = red_tol(m_d) * float(np.abs(u0 * s).sum()) + float((np.abs(u0) * red_tol(m_s) * s_mag).sum()) + U * abs(float((u0 * s).sum()))
    print(f"  eval: float32 re-summation s {m_s:.3e}, u.s {m_d:.3e}")
    check_abs(got_sigma[0], float((u0 * s).sum()), tol, "sigma (eval)")


def run_pi(dtype, shape, wc_mode):
    rng = np.random.default_rng(hash((shape, dtype)) % (2 ** 31))
    e = pi_entry(rng, dtype, shape, wc_mode)
    with Set(dtype, [e]) as st:
        snaps = []
        for rep in range(2):
            st.restore()
            e.b["v_sn"].set(None)
            e.b["sigma"].set(None)
            st.power_iteration(1)
            snaps.append(st.snapshot())
        assert same(*snaps), "replay differs (train)"
        print(f"power iteration {shape} dtype {dtype} wc {wc_mode}")
        check_pi_train(e, e.b["v_sn"].get(), e.b["u"].get(), e.b["sigma"].get())
        # eval: sigma only, u and v bitwise untouched
        st.restore()
        e.b["sigma"].set(None)
        before = [e.b["u"].bits(), e.b["v_sn"].bits(), e.b["p"].bits()]
        st.power_iteration(0)
        assert same(before, [e.b["u"].bits(), e.b["v_sn"].bits(), e.b["p"].bits()]), "eval mode wrote u, v or W"
        check_pi_eval(e, e.b["sigma"].get())


@pytest.mark.parametrize("shape", PI_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("dtype", [F32, BF16])
def test_power_iteration(shape, dtype):
    run_pi(dtype, shape, "scaled" if dtype == BF16 else None)


@pytest.mark.parametrize("shape", [(1, 64, 64), (2, 6, 1032)], ids=lambda s: "x".join(map(str, s)))
def test_power_iteration_bf16_without_copy_reads_master(shape):
    run_pi(BF16, shape, None)


@pytest.mark.parametrize("dtype", [F32, BF16])
def test_power_iteration_clamp(dtype):
    """|t| and |s| both below 1e-12: v = t / 1e-12, u = s / 1e-12; every square stays a normal fp32 number"""
    rng = np.random.default_rng(77 + dtype)
    e = pi_entry(rng, dtype, (2, 64, 32), None, w_scale=1e-15)
    e.h["u"] = mags(rng, 64, 8.0)         # |u| about 40: |t| about 2e-13, |s| about 1e-15
    with Set(dtype, [e]) as st:
        st.restore()
        e.b["v_sn"].set(None)
        e.b["sigma"].set(None)
        st.power_iteration(1)
        v, u, sg = e.b["v_sn"].get(), e.b["u"].get(), e.b["sigma"].get()
        W = e.h["p"].reshape(e.shape)
        t = O.wt_u(W, e.h["u"])[0]
        s = O.w_v(W, v)[0]
        assert np.linalg.norm(t) < 5e-13 and np.linalg.norm(s) < 5e-13, "the case no longer sits below the clamp"
        assert min((t * t).min(), (s * s).min(), np.abs(O.f64(W) * O.f64(v).reshape(2, 1, 32)).min()) > 1e-37, "a term went denormal"
        print(f"clamp dtype {dtype}: |t| {np.linalg.norm(t):.3e} |s| {np.linalg.norm(s):.3e}")
        check_pi_train(e, v, u, sg)
        assert np.allclose(v, t / 1e-12, rtol=1e-5, atol=1e-5 * np.abs(v).max()) and np.allclose(u, s / 1e-12, rtol=1e-5, atol=1e-5 * np.abs(u).max()), "the clamp did not decide"


@pytest.mark.parametrize("dtype", [F32, BF16])
def test_power_iteration_zero_weight_and_inactive_entry(dtype):
    rng = np.random.default_rng(5 + dtype)
    z = pi_entry(rng, dtype, (2, 70, 12), None)
    z.h["p"] = np.zeros(z.n, np.float32)
    off = pi_entry(rng, dtype, (1, 65, 16), "scaled", active=False)
    on = pi_entry(rng, dtype, (1, 5, 8), None)
    with Set(dtype, [z, off, on]) as st:
        st.restore()
        z.b["v_sn"].set(None)
        z.b["sigma"].set(None)
        before = [off.b[k].bits() for k in ("u", "v_sn", "sigma")]
        st.power_iteration(1)
        assert not z.b["u"].get().any() and not z.b["v_sn"].get().any(), "zero weight: u and v must be exactly 0 (and not NaN)"
        assert z.b["sigma"].get()[0] == 0.0
        assert same(before, [off.b[k].bits() for k in ("u", "v_sn", "sigma")]), "an inactive entry was touched"
        check_pi_train(on, on.b["v_sn"].get(), on.b["u"].get(), on.b["sigma"].get())
        before = [off.b[k].bits() for k in ("u", "v_sn", "sigma")]
        st.power_iteration(0)
        assert same(before, [off.b[k].bits() for k in ("u", "v_sn", "sigma")]), "an inactive entry was touched (eval)"


# ------------------------------------------------------------------------------------------------
# <G, W>
# ------------------------------------------------------------------------------------------------
def check_dot(e, got_dot):
    is_ = float(e.h["sigma"][1])
    ref, mag = O.grad_dot(e.h["g"], e.h["p"])
    m = R.f32_sum_error(O.f64(e.h["g"]) * O.f64(e.h["p"]))[0]
    # every work item's partial is multiplied by 1/sigma (one rounding), the partials are added in fp32
    check_red(got_dot[0], ref * is_, mag * abs(is_), m, f"dot[0] n={e.n}", extra=2 * U * mag * abs(is_))


def test_grad_dot():
    """n on both sides of one and of three 8192-element work items; slot 0 takes the whole value, the other slots are left alone"""
    rng = np.random.default_rng(11)
    ents = [Ent(rng, F32, taps=1, rows=r, cols=c) for r, c in ((23, 356), (64, 128), (3, 2732), (5, 4916))]
    assert [e.n for e in ents] == [8188, 8192, 8196, 3 * 8192 + 4]
    for e in ents:
        e.h["dot"] = np.concatenate([[np.nan], mags(rng, 31)]).astype(np.float32)
    with Set(F32, ents) as st:
        snaps = []
        for rep in range(2):
            st.restore()
            st.grad_dot()
            snaps.append(st.snapshot())
        assert same(*snaps), "replay differs"
        for e in ents:
            d = e.b["dot"].get()
            check_dot(e, d)
            assert np.array_equal(d[1:], e.h["dot"][1:]), "slots 1..31 were written"


# ------------------------------------------------------------------------------------------------
# AdamW
# ------------------------------------------------------------------------------------------------
def ref_grad(e, g, dot_got, sigma_got):
    """float64 gradient wrt the original weight from the kernel's own summed dot and 1/sigma, and its error bound e_g"""
    g = O.f64(g).reshape(e.shape)
    if not e.sn:
        return g, np.zeros_like(g)
    cdot = np.float32(0.0)
    for k in range(32):                     # the kernels add the slots in fp32, in index order
        cdot = np.float32(cdot + np.float32(dot_got[k]))
    is_ = float(np.float32(sigma_got[1]))
    go = O.chain_rule(g, float(cdot), is_, e.h["u"], e.h["v_sn"])
    return go, sn_grad_bound(go, e.h["u"], e.h["v_sn"], float(cdot), is_, e.shape)


def plant(e, rng, step):
    """planted elements of a plain tensor: (g, m, v) = 0: the update is exactly 0; |g| = 1e-8 on zero moments: eps decides;
    p = 0: the update is read at full fp32 precision"""
    n = e.n
    e.planted = {}
    if n >= 1020 and not e.sn:          # a spectral-norm entry's gradient gets the u v^T term: nothing there is exactly 0 or 1e-8
        i0, i1, i2 = 5, n // 2 + 1, n - 3
        e.h["g"][i0] = e.h["m"][i0] = e.h["v"][i0] = 0.0
        e.h["g"][i1], e.h["m"][i1], e.h["v"][i1] = 1e-8, 0.0, 0.0
        e.h["p"][i2] = 0.0
        e.planted = dict(zero=i0, eps=i1, p0=i2)
    elif e.sn:
        e.h["p"][n // 3] = 0.0
    e.restore()


def check_planted(e, got, lr, wd, step):
    if not getattr(e, "planted", None):
        return
    i0, i1 = e.planted["zero"], e.planted["eps"]
    decay = np.float32(np.float32(1.0) - np.float32(np.float32(lr) * np.float32(wd)))
    assert got["p"][i0] == np.float32(e.h["p"][i0] * decay) and got["m"][i0] == 0.0 and got["v"][i0] == 0.0, "g = m = v = 0: p must become p * decay exactly"
    bc1, bc2s = coef(step)
    v1 = (1 - B2) * 1e-16
    upd = (lr / bc1) * ((1 - B1) * 1e-8) / (np.sqrt(v1) / bc2s + EPS)
    no_eps = (lr / bc1) * ((1 - B1) * 1e-8) / (np.sqrt(v1) / bc2s)
    inc = float(got["p"][i1]) - float(e.h["p"][i1])
    ref = float(e.h["p"][i1]) * (float(decay) - 1.0) - upd
    print(f"  planted |g| = 1e-8: increment {inc:.6e}, reference {ref:.6e}, without eps it would be {ref + upd - no_eps:.6e}")
    assert abs(no_eps - upd) > 0.2 * abs(upd), "eps does not decide this element"


FLAT_CASES = [(step, dtype, 0.01 if (k + dtype) % 2 == 0 else 0.0) for k, step in enumerate((1, 2, 10, 1000)) for dtype in (F32, BF16)]


@pytest.mark.parametrize("step,dtype,wd", FLAT_CASES, ids=lambda x: str(x))
def test_adamw_flat(step, dtype, wd):
    """adamw_kernel over plain tensors and (Linear-style and, for the tap arithmetic, three-tap) spectral-norm entries, with the
    clip coefficient null and 0.25; the <G,W> pass and both gradient-norm passes on the same set"""
    torch = _torch()
    rng = np.random.default_rng(100 * step + dtype)
    wd = float(np.float32(wd))
    ents = [Ent(rng, dtype, n=n, wc=(n == 8192)) for n in (4, 1020, 8192, 8196)]
    ents += [Ent(rng, dtype, taps=1, rows=9, cols=12, wc=dtype == BF16),
             Ent(rng, dtype, taps=3, rows=50, cols=60, wc=dtype == BF16),        # 9000 elements: the taps straddle two work items
             Ent(rng, dtype, taps=1, rows=37, cols=24, wc=False)]
    for e in ents:
        plant(e, rng, step)
        if e.sn:
            e.h["dot"] = np.concatenate([[np.nan], np.zeros(31)]).astype(np.float32)      # the engine's state: slot 0 from the finalize, the rest 0
    gs_dev = torch.tensor([0.25], dtype=torch.float32, device="cuda")
    with Set(dtype, ents) as st:
        for gscale in (None, 0.25):
            snaps = []
            for rep in range(2):
                st.restore()
                st.grad_dot()
                gn_pass = st.grad_norm()
                gn_upd = st.adamw(LR, wd, step, gs_dev.data_ptr() if gscale else None)
                snaps.append(st.snapshot() + [gn_pass, gn_upd])
            assert same(snaps[0][:-2], snaps[1][:-2]) and snaps[0][-2:] == snaps[1][-2:], "replay differs"
            print(f"flat AdamW step {step} dtype {dtype} wd {wd} gscale {gscale}")
            terms, extra = [], 0.0
            for i, e in enumerate(ents):
                got = {k: e.b[k].get() for k in ("p", "m", "v")}
                dot_got = e.b["dot"].get() if e.sn else None
                if e.sn:
                    check_dot(e, dot_got)
                g_ref, e_g = ref_grad(e, e.h["g"], dot_got, e.h["sigma"] if e.sn else None)
                check_update(f"entry {i} {e.shape}", e.shape, g_ref, e_g, got, e.h, LR, wd, step, gscale)
                check_planted(e, got, LR, wd, step)
                terms.append((g_ref * g_ref).ravel())
                extra += float((2 * np.abs(g_ref) * e_g + U * g_ref * g_ref).sum())
                assert np.array_equal(e.b["g"].get(), e.h["g"]), "the gradient was written"
                if e.b["wc"] is not None:
                    if dtype == BF16:
                        assert np.array_equal(e.b["wc"].get(), O.bf16_round(got["p"])), "wc is not bf16(p_new)"
                    else:
                        assert np.isnan(e.b["wc"].get()).all()
            terms = np.concatenate(terms)
            m = R.f32_sum_error(terms)[0]
            check_red(gn_upd, terms.sum(), terms.sum(), m, "gradient norm^2 from the update pass (before the clip)", extra=extra)
            check_red(gn_pass, terms.sum(), terms.sum(), m, "gradient norm^2 from the norm pass", extra=extra)
            assert abs(gn_pass - gn_upd) <= 2 * (red_tol(m) * terms.sum() + extra)


# (taps, rows, cols) of the tiled pass: 64 x 64 tiles; both edges short, exact, one vector past, and more than one tile
TILE_SHAPES = [(1, 4, 132), (2, 132, 4), (3, 60, 64), (1, 64, 60), (2, 64, 64), (1, 68, 68), (2, 132, 68), (3, 68, 132)]
TILE_CASES = [(s, dtype, (1, 10, 1000)[(i + dtype) % 3]) for i, s in enumerate(TILE_SHAPES) for dtype in (F32, BF16)]


def check_tiled(e, st, got, g_vals, lr, wd, step, dtype, gn, tag):
    g_ref, e_g = ref_grad(e, g_vals, e.h["dot"], e.h["sigma"])
    check_update(tag, e.shape, g_ref, e_g, got, e.h, lr, wd, step, None)
    pn = got["p"].reshape(e.shape)
    if e.b["wc"] is not None:
        if dtype == BF16:
            assert np.array_equal(e.b["wc"].get(), O.bf16_round(got["p"])), "wc is not bf16(p_new)"
        else:
            assert np.isnan(e.b["wc"].get()).all(), "the fp32 tiled pass has no wc to write"
    if e.b["wct"] is not None:
        want = O.wct_copy(O.bf16_round(pn) if dtype == BF16 else pn)
        assert np.array_equal(e.b["wct"].get(want.shape), want), "wct is not the flipped transpose of the compute copy of p_new"
    return (g_ref * g_ref).ravel(), float((2 * np.abs(g_ref) * e_g + U * g_ref * g_ref).sum())


@pytest.mark.parametrize("shape,dtype,step", TILE_CASES, ids=lambda x: "x".join(map(str, x)) if isinstance(x, tuple) else str(x))
def test_adamw_tiled(shape, dtype, step):
    """adamw_sn_kernel: the update, wc, wct (each null in turn), the per-tile gradient-norm partials and the W_new^T u partials
    the next power iteration reuses"""
    rng = np.random.default_rng(hash((shape, dtype, step)) % (2 ** 31))
    wd = float(np.float32(0.01 if step != 10 else 0.0))
    taps, rows, cols = shape
    for mode in ("both", "no wc", "no wct"):
        e = Ent(rng, dtype, taps=taps, rows=rows, cols=cols, tiled=True, wc=mode != "no wc", wct=mode != "no wct")
        e.h["p"][e.n // 3] = 0.0
        with Set(dtype, [e]) as st:
            snaps = []
            for rep in range(2):
                st.restore()
                gn = st.adamw(LR, wd, step)
                snaps.append(st.snapshot() + [gn])
            assert same(snaps[0][:-1], snaps[1][:-1]) and snaps[0][-1] == snaps[1][-1], "replay differs"
            print(f"tiled AdamW {shape} dtype {dtype} step {step} wd {wd} copies: {mode}")
            got = {k: e.b[k].get() for k in ("p", "m", "v")}
            terms, extra = check_tiled(e, st, got, e.h["g"], LR, wd, step, dtype, gn, "tiled")
            check_red(gn, terms.sum(), terms.sum(), R.f32_sum_error(terms)[0], "sum of the per-tile gradient-norm partials", extra=extra)
            assert np.array_equal(e.b["g"].get(), e.h["g"]), "the gradient was written"
            if mode != "both":
                continue
            # the tile pass left W_new^T u per 64-row block: a power iteration that reuses it against float64 on W_new, and
            # against a full power iteration from the same state (not bitwise: the two sum the rows in different orders)
            Wn = got["p"].reshape(e.shape)
            t, t_mag = O.wt_u(Wn, e.h["u"])
            dv = norm_bound(t, red_tol(R.f32_sum_error(O.f64(Wn) * O.f64(e.h["u"])[None, :, None], axis=1)[0]) * t_mag, red_tol(sq_err(t)))
            e.b["v_sn"].set(None)
            st.power_iteration(1, reuse=1)
            v_reuse = e.b["v_sn"].get()
            check_abs(v_reuse, O.normalize(t), dv, "v from the reused partials vs float64 W_new^T u")
            assert np.isfinite(e.b["u"].get()).all() and np.isfinite(e.b["sigma"].get()).all()
            e.b["u"].set(e.h["u"])
            e.b["v_sn"].set(None)
            st.power_iteration(1, reuse=0)
            check_abs(e.b["v_sn"].get(), v_reuse, 2 * dv, "v from a full power iteration vs the reused partials")


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("source", [1, 2])
def test_adamw_tiled_bf16_gradient_sources(dtype, source):
    """source 1: the per-entry bf16 mirror (AdamDesc::glp, one entry without a mirror falls back to fp32); source 2: the bf16 wire
    copy, entries at non-zero offsets of one arena so that g_base matters.  The fp32 gradients hold other finite values: the result
    must come from the bf16 ones, and the fp32 buffer stays untouched."""
    torch = _torch()
    rng = np.random.default_rng(31 * dtype + source)
    shapes = [(2, 68, 36), (1, 64, 64), (3, 20, 132)]
    sizes = [t * r * c for t, r, c in shapes]
    offs = [12, 12 + sizes[0] + 20, 12 + sizes[0] + 20 + sizes[1] + 4]
    total = offs[2] + sizes[2] + 8
    decoy = mags(rng, total, 3.0)
    arena = Buf(decoy)
    ents = [Ent(rng, dtype, taps=t, rows=r, cols=c, tiled=True, wc=True, wct=True, g_bf16=(source == 1 and i != 1),
                g_ext=arena.p + 4 * offs[i], bf16_grad=True) for i, (t, r, c) in enumerate(shapes)]
    wire_h = O.bf16_round(mags(rng, total, 5.0))        # a third set of values where no entry lives
    for e, o in zip(ents, offs):
        wire_h[o:o + e.n] = e.h["g"]
    wire = Buf(wire_h, bf16=True)
    step, wd = 10, float(np.float32(0.01))
    with Set(dtype, ents) as st:
        snaps = []
        for rep in range(2):
            st.restore()
            arena.set(decoy)
            for e in ents:
                if e.b["g_bf16"] is not None:
                    e.b["g_bf16"].set(e.h["g"])
            gn = st.adamw(LR, wd, step, None, source, arena.p, wire.p if source == 2 else None, total)
            snaps.append(st.snapshot() + [gn])
        assert same(snaps[0][:-1], snaps[1][:-1]) and snaps[0][-1] == snaps[1][-1], "replay differs"
        print(f"tiled AdamW gradient source {source} dtype {dtype}")
        assert np.array_equal(arena.get(), decoy), "the fp32 gradient arena was written"
        assert np.array_equal(wire.get(), wire_h), "the wire copy was written"
        terms, extra = [], 0.0
        for i, (e, o) in enumerate(zip(ents, offs)):
            used = decoy[o:o + e.n] if (source == 1 and e.b["g_bf16"] is None) else e.h["g"]
            got = {k: e.b[k].get() for k in ("p", "m", "v")}
            t, x = check_tiled(e, st, got, used, LR, wd, step, dtype, gn, f"entry {i} {e.shape}")
            terms.append(t)
            extra += x
        terms = np.concatenate(terms)
        check_red(gn, terms.sum(), terms.sum(), R.f32_sum_error(terms)[0], "gradient norm^2", extra=extra)


# ------------------------------------------------------------------------------------------------
# make_copies
# ------------------------------------------------------------------------------------------------
COPY_SHAPES = [(1, 1, 4), (2, 31, 36), (3, 32, 100), (7, 33, 4), (1, 70, 100), (2, 70, 36), (3, 1, 100)]


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("mode", ["wc", "wct", "both"])
def test_make_copies(dtype, mode):
    """32 x 32 tiles: rows and cols short of, at and past a tile, taps up to 7; one table over all shapes and a plain tensor"""
    rng = np.random.default_rng(3 + dtype)
    ents = [Ent(rng, dtype, taps=t, rows=r, cols=c, wc=mode != "wct", wct=mode != "wc") for t, r, c in COPY_SHAPES]
    if mode != "wct":
        ents.append(Ent(rng, dtype, n=100, wc=True))
    with Set(dtype, ents) as st:
        snaps = []
        for rep in range(2):
            st.restore()
            st.make_copies()
            snaps.append(st.snapshot())
        assert same(*snaps), "replay differs"
        for e in ents:
            p = e.h["p"].reshape(e.shape)
            c = O.bf16_round(p) if dtype == BF16 else p
            if e.b["wc"] is not None:
                assert np.array_equal(e.b["wc"].get(e.shape), c), f"wc {e.shape}"
            if e.b["wct"] is not None:
                assert np.array_equal(e.b["wct"].get((e.taps, e.cols, e.rows)), O.wct_copy(c)), f"wct {e.shape}"
            assert np.array_equal(e.b["p"].get(), e.h["p"])


# ------------------------------------------------------------------------------------------------
# bad arguments
# ------------------------------------------------------------------------------------------------
def test_bad_arguments_are_rejected_before_any_launch():
    lib = E.load_library()
    rng = np.random.default_rng(9)

    def rejected(e, what, dtype=F32, patch=None):
        ce = e.centry()
        if patch:
            patch(ce)
        h = C.c_void_p()
        before = e.snapshot()
        rc = lib.sgv_test_optset_create(dtype, (E.OptsetEntry * 1)(ce), 1, C.byref(h))
        msg = lib.sgv_last_error().decode()
        print(f"  {what}: {rc} '{msg}'")
        assert rc == -1 and "sgv_test_optset_create" in msg and not h.value, what
        assert same(before, e.snapshot()), "a rejected call wrote to a buffer"

    plain = Ent(rng, F32, n=16)
    sn = Ent(rng, F32, taps=1, rows=4, cols=8)
    rejected(plain, "n % 4", patch=lambda c: setattr(c, "n", 6))
    rejected(Ent(rng, F32, taps=1, rows=2, cols=6), "cols % 4 on a spectral-norm entry")
    for k in ("p", "g", "m", "v"):
        rejected(plain, f"{k} not 16-byte aligned", patch=lambda c, k=k: setattr(c, k, getattr(c, k) + 4))
    rejected(plain, "tiled without spectral norm", patch=lambda c: setattr(c, "tiled", 1))
    rejected(sn, "taps * rows * cols != n", patch=lambda c: setattr(c, "n", 36))
    rejected(sn, "unknown dtype", dtype=2)
    # a valid set: out-of-range calls on it are rejected too
    with Set(F32, [sn]) as st:
        out = C.c_double()
        assert lib.sgv_test_optset_adamw(st.h, LR, 0.0, 0, None, 0, None, None, 0, C.byref(out), None) == -1
        assert lib.sgv_test_optset_adamw(st.h, LR, 0.0, 1, None, 3, None, None, 0, C.byref(out), None) == -1
        assert lib.sgv_test_optset_adamw(st.h, LR, 0.0, 1, None, 2, None, None, 0, C.byref(out), None) == -1
        assert "sgv_test_optset_adamw" in lib.sgv_last_error().decode()
