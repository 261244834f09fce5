"""The harness of the kernel tests of the recon tails (csrc/recon_out.hip), one per pass: tests/test_{generate,summary,score,ensemble,
sobol,distribution,regression,project,temporal,gram,exceedance,cycles}_kernel_gpu.py.  A test file describes its pass as data (Pass)
and keeps its cases, its reference comparisons and its own rejection entries; everything else is here, once: the inputs and the
memo of cases with the stored field F (case), the canary-framed buffers, one checked call of sgv_test_recon_<pass> (launch), the
bitwise comparison (same), batch independence (assert_batch_independent) and the rejected calls (common_rejections, reject_all).
Groups follow the model's rule G = min(8, max(1, C // 4)).

The kernel tests import this module as `recon_kernel_common` (tests/ on sys.path), tests/surrogate_common.py as
`tests.recon_kernel_common`: two module objects.  The second takes `bits` only; the memo of cases is filled and read under the first
name alone."""
import collections
import ctypes

import numpy as np
import pytest

from simulgen_vae_amd import engine as E

ELT32 = 2e-5        # tests/test_ew_kernels_gpu.py
CANARY = 768.0
ICANARY = -777
MARGIN = 64         # elements of canary in front of and behind every buffer (keeps it 16-byte aligned)
SGV_ERR_ARG = -1
UNWRITTEN = -999    # what an int32 output holds before a launch from empty (no count, step or index is below -1); a float one holds NaN
DTYPES = pytest.mark.parametrize("dtype", [0, 1], ids=["f32", "bf16"])
SHARED = ("y", "sums", "gamma", "beta", "scale", "mn")          # the pointers every hook takes in front

# A pass as data.  name: the hook is sgv_test_recon_<name>; shapes(b, T, C, **params) -> name -> shape of every buffer behind the shared
# ones, inputs and outputs; outputs: the names among them that the pass writes; integer: those that are int32; args(a) -> the hook's
# arguments between min and B, from a: the flat dict of every argument (pointers by buffer name, None for NULL, and the params).
Pass = collections.namedtuple("Pass", "name shapes outputs args integer", defaults=[()])


def _groups(Cn):
    return min(8, max(1, Cn // 4))


def _bf16(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(torch.bfloat16).to(torch.float32).numpy()


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def same(a, b, names=None):
    """the names (all of either dict, or `names`) whose arrays are not the same bits in a and b"""
    names = sorted(set(a) | set(b)) if names is None else names
    return [k for k in names if k not in a or k not in b or not np.array_equal(bits(a[k]), bits(b[k]))]


def base_inputs(B, T, Cn, dtype, signed=True):
    """y [B, T, C], gamma, beta, scale, mn as fp32 (y not yet rounded to bf16): gamma spread enough that tanh saturates somewhere, scale of
    mixed magnitudes in [1e-3, 50], min of both signs; signed: a quarter of the scales negative (scaler_vectors admits that)"""
    rng = np.random.default_rng(1000 * Cn + 10 * T + B + dtype)
    y = (rng.standard_normal((B, T, Cn)) * 2 + 0.5).astype(np.float32)
    gamma = (1.6 + 0.4 * rng.standard_normal(Cn)).astype(np.float32)
    beta = (0.3 * rng.standard_normal(Cn)).astype(np.float32)
    scale = np.exp(rng.uniform(np.log(1e-3), np.log(50.0), Cn)).astype(np.float32)
    mn = (rng.standard_normal(Cn) * np.where(rng.random(Cn) < 0.5, 1.0, 30.0)).astype(np.float32)
    if signed:
        scale = np.where(rng.random(Cn) < 0.25, -scale, scale).astype(np.float32)
    return dict(y=y, gamma=gamma, beta=beta, scale=scale, mn=mn)


def inputs(B, T, Cn, dtype, edit=None, signed=True):
    """base_inputs, edited in place by edit(c) (copies of rows or nodes, a plateau), y rounded to bf16 where dtype == 1"""
    import torch
    c = base_inputs(B, T, Cn, dtype, signed)
    if edit is not None:
        edit(c)
    if dtype == 1:
        c["y"] = _bf16(torch, c["y"])
    return c


_CASES = {}


def case(owner, B, T, Cn, ldy, dtype, edit=None, extras=None, signed=True):
    """the case of one (owner, shape, dtype), built once per session and read-only: inputs(), the stored field F (ldy None: a file
    that tests the output pass itself has none) and what extras(c) adds to them (levels, gates, limits, references).  owner: the test
    module's name, with whatever else its extras depend on."""
    key = (owner, B, T, Cn, ldy, dtype)
    if key not in _CASES:
        c = inputs(B, T, Cn, dtype, edit, signed)
        if ldy is not None:
            c["F"] = field(c, c["y"], ldy, dtype)
        if extras is not None:
            c.update(extras(c))
        for v in c.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _CASES[key] = c
    return _CASES[key]


def canary_buffers(sizes, integer=()):
    """name -> (whole buffer with canary margins, the view of sizes[name] elements between them); int32 for the names in `integer`"""
    import torch
    bufs = {}
    for name, n in sizes.items():
        i = name in integer
        buf = torch.full((n + 2 * MARGIN,), ICANARY if i else CANARY, dtype=torch.int32 if i else torch.float32, device="cuda")
        bufs[name] = (buf, buf[MARGIN:MARGIN + n])
        assert bufs[name][1].data_ptr() % 16 == 0
    return bufs


def margins_intact(bufs):
    return all(bool((b[:MARGIN] == b[0]).all()) and bool((b[-MARGIN:] == b[0]).all()) and float(b[0]) in (CANARY, ICANARY) for b, _ in bufs.values())


def device_inputs(c, y, ldy, dtype):
    """y [b, T, C]: the samples of this launch, in a map with canary padding columns; the statistics buffer starts as NaN"""
    import torch
    b, T, Cn = y.shape
    ymap = torch.full((b * T, ldy), CANARY, dtype=torch.bfloat16 if dtype == 1 else torch.float32, device="cuda")
    ymap[:, :Cn] = torch.from_numpy(np.array(y).reshape(b * T, Cn)).cuda().to(ymap.dtype)
    f = lambda a: torch.from_numpy(np.array(a)).cuda()
    sums = torch.full((b * _groups(Cn) * 2,), float("nan"), dtype=torch.float64, device="cuda")
    return dict(y=ymap, gamma=f(c["gamma"]), beta=f(c["beta"]), scale=f(c["scale"]), mn=f(c["mn"]), sums=sums)


def padding_intact(d, Cn):
    return bool((d["y"][:, Cn:].float() == CANARY).all())


def hook_args(d, bufs, ldy, dtype, B, T, Cn, /, **params):
    """the flat dict of a hook's arguments: the shared ones from device_inputs, every buffer's pointer under its name, the params"""
    return dict({k: d[k].data_ptr() for k in SHARED}, **{k: v.data_ptr() for k, (_, v) in bufs.items()}, dtype=dtype, ldy=ldy, B=B, T=T, Cn=Cn, **params)


def sizes(ps, b, T, Cn, /, **params):
    return {k: int(np.prod(s)) for k, s in ps.shapes(b, T, Cn, **params).items()}


def outputs_of(ps, bufs, b, T, Cn, /, **params):
    """the outputs as launch() returns them, read from the front of buffers that may be larger than the shapes"""
    return {k: bufs[k][1][:int(np.prod(s))].cpu().numpy().reshape(s) for k, s in ps.shapes(b, T, Cn, **params).items() if k in ps.outputs}


def struct(cls, a, names, **fields):
    """the hook's E.*Out / E.*State argument from the pointers a[name] that are not None; NULL itself where a["no_struct"] is set"""
    return None if a.get("no_struct") else ctypes.byref(cls(**{k: a[k] for k in names if a.get(k) is not None}, **fields))


def call(ps, a):
    """sgv_test_recon_<pass> on the flat argument dict a -> its return code"""
    hook = getattr(E.load_library(), "sgv_test_recon_" + ps.name)
    return hook(a["dtype"], a["y"], a["ldy"], a["sums"], a["gamma"], a["beta"], a["scale"], a["mn"], *ps.args(a), a["B"], a["T"], a["Cn"], None)


def launch(ps, c, y, ldy, dtype, /, given=None, want=None, state=None, **params):
    """One successful call of the hook on the samples y [b, T, C] -> the outputs, all of them, as shaped numpy arrays by name.
    given: name -> array of every input buffer (None: a NULL pointer); want: the outputs asked for (default: all), the others get
    NULL; state: name -> array that an output holds before the call (a running state to continue from), else it holds NaN / UNWRITTEN.
    Checked on every call: rc, the margins of every buffer, the padding columns of y, the bits of every input, that an output asked
    for from empty is written everywhere (finite, no UNWRITTEN), and that an output not asked for is what it was."""
    import torch
    b, T, Cn = y.shape
    shapes = ps.shapes(b, T, Cn, **params)
    want = ps.outputs if want is None else want
    held = {}          # name -> what the buffer holds before the call as a flat host array; None: nothing of the caller's
    for k in shapes:
        src = (state or {}).get(k) if k in ps.outputs else (given or {})[k]
        held[k] = None if src is None else np.array(src, np.int32 if k in ps.integer else np.float32).reshape(-1)
    d = device_inputs(c, y, ldy, dtype)
    bufs = canary_buffers(sizes(ps, b, T, Cn, **params), integer=ps.integer)
    for k, (_, view) in bufs.items():
        if held[k] is not None:
            view.copy_(torch.from_numpy(held[k]).cuda())
        elif k in ps.outputs:
            view.fill_(UNWRITTEN if k in ps.integer else float("nan"))
    a = hook_args(d, bufs, ldy, dtype, b, T, Cn, **params)
    a.update({k: None for k in bufs if (k not in want if k in ps.outputs else held[k] is None)})
    rc = call(ps, a)
    assert rc == 0, E.load_library().sgv_last_error().decode()
    assert margins_intact(bufs), "a margin around a buffer was written"
    assert padding_intact(d, Cn), "the padding columns of y were written"
    res = {k: view.cpu().numpy() for k, (_, view) in bufs.items()}
    for k, got in res.items():
        if held[k] is not None:
            assert (k in ps.outputs and k in want) or np.array_equal(bits(got), bits(held[k])), f"{k} was written"
        elif k not in ps.outputs:
            assert (got == CANARY).all(), f"{k} was written although NULL was passed"
        elif k in want:
            assert (got != UNWRITTEN).all() if k in ps.integer else np.isfinite(got).all(), f"an element of {k} was not written"
        else:
            assert (got == UNWRITTEN).all() if k in ps.integer else np.isnan(got).all(), f"{k} was written although it was not asked for"
    return {k: res[k].reshape(shapes[k]) for k in ps.outputs}


FIELD = Pass("physical", lambda b, T, Cn, layout: {"out": (b, T, Cn) if layout == 0 else (b, Cn, T)}, ("out",), lambda a: (a["layout"], a["out"]))


def field(c, y, ldy, dtype):
    """F: the output pass (sgv_test_recon_physical, layout [B][T][N]) on the same inputs, [b, T, C] fp32"""
    return launch(FIELD, c, y, ldy, dtype, layout=0)["out"]


def assert_batch_independent(run, y):
    """run(y') -> dict of outputs with the batch axis in front: each sample of B = 3 launched alone, and the last two together, give
    the bits they have in the batch"""
    whole = run(y)
    for b in range(3):
        assert not same(run(y[b:b + 1]), {k: v[b:b + 1] for k, v in whole.items()}), b
    assert not same(run(y[1:]), {k: v[1:] for k, v in whole.items()})


def common_rejections(good):
    """the front of every pass's table of (override, message fragment): what all hooks refuse in the arguments they share"""
    Cn, ldy = good["Cn"], good["ldy"]
    bad = [({k: None}, "null argument") for k in SHARED]
    bad += [(dict(y=good["y"] + 4), "misaligned pointer"), (dict(B=0), "B, T >= 1"), (dict(T=0), "B, T >= 1")]
    bad += [(dict(ldy=Cn - 8), "row stride"), (dict(ldy=ldy + 4), "row stride"), (dict(dtype=2), "dtype must be")]
    return bad + [(dict(Cn=v), "C % 8 == 0 required") for v in (0, 4, Cn - 4, Cn + 4)]


def reject_all(ps, d, bufs, good, bad):
    """every (override, fragment) of `bad` on top of the good arguments is refused with SGV_ERR_ARG and the fragment; then nothing was
    launched and nothing written: every buffer, margins included, is what it was, the statistics are still NaN, the padding is
    intact; then the good call itself succeeds (its results are the caller's to check)"""
    import torch
    lib = E.load_library()
    keep = {k: b.clone() for k, (b, _) in bufs.items()}
    print(f"  {ps.name}: {len(bad)} rejected calls")
    for over, msg in bad:
        assert call(ps, dict(good, **over)) == SGV_ERR_ARG, over
        assert msg in lib.sgv_last_error().decode(), (over, lib.sgv_last_error().decode())
    torch.cuda.synchronize()
    for k, (b, _) in bufs.items():
        assert bool((b.view(torch.int32) == keep[k].view(torch.int32)).all()), f"{k} was written by a rejected call"
    assert torch.isnan(d["sums"]).all(), "a rejected call computed the statistics"
    assert padding_intact(d, good["Cn"]), "a rejected call wrote the padding columns of y"
    assert call(ps, good) == 0, lib.sgv_last_error().decode()
