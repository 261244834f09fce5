"""Surrogate exceedance durations on the GPU: Engine.exceedance (sgv_exceedance) against the numpy emulation
(tests/exceedance_reference.py) on what Engine.generate writes on the same engine, latents and injected noise; what a call leaves
behind in the engine; and Surrogate.exceedance against the emulation on Surrogate.predict, on the models of
tests/golden/predict_small.npz.

Everything is bit for bit: the statistics are integers and the excess is one fp32 chain in a fixed order.  predict and exceedance draw
the decoder's noise per call, so a comparison of the two makes one call of each on Surrogates with the same seed (the rule of
tests/test_sweep_gpu.py)."""
import os
import sys

import numpy as np
import pytest
import torch

import simulgen_vae_amd  # noqa: F401
from simulgen_vae_amd import engine as E
from simulgen_vae_amd.predict import ExceedanceResult
from tests.surrogate_common import MAXB, engine, latents, no_forward_after, signed_scaler, surrogate, training_unaffected

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import exceedance_reference as XR  # noqa: E402

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def equals_emulation(stats, excess, F, levels, side, what):
    want_stats, want_excess = XR.emulate(F, levels, side)
    for k, name in enumerate(XR.STATS):
        assert np.array_equal(stats[:, k], want_stats[:, k]), f"{what}: {name}"
    assert np.array_equal(bits(excess), bits(want_excess)), f"{what}: excess"
    ratio = XR.worst_ratio(excess, F, levels, side)
    print(f"  {what}: worst excess err / bound {ratio:.4f}")
    assert ratio <= 1.0


def result_equals_emulation(res, F, side, what):
    equals_emulation(res.stats.cpu().numpy(), res.excess.cpu().numpy(), F, res.levels.cpu().numpy(), side, what)


def same_bits(a, b):
    assert torch.equal(a.stats, b.stats) and torch.equal(a.excess.view(torch.int32), b.excess.view(torch.int32))


@pytest.mark.parametrize("side", ["above", "below"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("B", [1, 3, MAXB])
@pytest.mark.parametrize("name", ["G0", "G1"])
def test_exceedance_counts_what_generate_writes(name, B, dtype, side):
    cfg, eng = engine(name, dtype)
    T, N = cfg.num_time, cfg.num_node
    z, xs, eps = latents(cfg, B)
    scale, mn = (torch.from_numpy(a).cuda() for a in signed_scaler(N))
    eng.set_eps(eps)
    F = eng.generate(z, xs, scale, mn, fix=True).cpu().numpy()
    all4 = XR.kernel_levels(F)
    for sel in ([0], [1, 2, 3], [0, 1, 2, 3]):
        levels = all4[sel]
        eng.set_eps(eps)
        out = eng.exceedance(z, xs, scale, mn, torch.from_numpy(levels).cuda(), side=side, fix=True)
        assert sorted(out) == ["excess", "stats"]
        st, ex = out["stats"], out["excess"]
        assert st.dtype == torch.int32 and st.shape == (B, 5, len(sel), N) and st.is_contiguous()
        assert ex.dtype == torch.float32 and ex.shape == (B, len(sel), N) and ex.is_contiguous()
        equals_emulation(st.cpu().numpy(), ex.cpu().numpy(), F, levels, side, f"{name} B {B} L {len(sel)} {dtype} {side}")
    # each output alone, into the rows of larger tensors
    dev = torch.from_numpy(all4).cuda()
    big_s = torch.full((B + 2, 5, 4, N), -999, dtype=torch.int32, device="cuda")
    big_e = torch.full((B + 2, 4, N), float("nan"), device="cuda")
    eng.set_eps(eps)
    only = eng.exceedance(z, xs, scale, mn, dev, side=side, stats=big_s[1:B + 1], excess=False)
    assert sorted(only) == ["stats"] and only["stats"].data_ptr() == big_s[1:].data_ptr()
    eng.set_eps(eps)
    only = eng.exceedance(z, xs, scale, mn, dev, side=side, stats=False, excess=big_e[1:B + 1])
    assert sorted(only) == ["excess"] and only["excess"].data_ptr() == big_e[1:].data_ptr()
    assert bool((big_s[0] == -999).all()) and bool((big_s[B + 1] == -999).all()) and bool(big_e[0].isnan().all()) and bool(big_e[B + 1].isnan().all())
    assert torch.equal(big_s[1:B + 1], st) and torch.equal(big_e[1:B + 1].view(torch.int32), ex.view(torch.int32))


def test_exceedance_checks_its_arguments():
    cfg, eng = engine("G0", "f32")
    z, xs, eps = latents(cfg, 2)
    scale, mn = (torch.from_numpy(a).cuda() for a in signed_scaler(cfg.num_node))
    N, L = cfg.num_node, 3
    lv = torch.zeros((L, N), device="cuda")
    for bad in (lv[0], lv[:, :-1], lv.double(), lv.cpu(), torch.zeros((5, N), device="cuda"), torch.zeros((0, N), device="cuda"),
                torch.zeros((L, 2 * N), device="cuda")[:, ::2], lv.cpu().numpy()):
        with pytest.raises(ValueError, match="levels must be a contiguous float32 CUDA tensor of shape"):
            eng.exceedance(z, xs, scale, mn, bad)
    for bad in (torch.zeros((2, 5, L + 1, N), dtype=torch.int32, device="cuda"), torch.zeros((1, 5, L, N), dtype=torch.int32, device="cuda"),
                torch.zeros((2, 5, L, N), device="cuda"), torch.zeros((2, 5, L, N), dtype=torch.int32), None):
        with pytest.raises(ValueError, match="stats must be True, False or a contiguous torch.int32 CUDA tensor of shape"):
            eng.exceedance(z, xs, scale, mn, lv, stats=bad)
    for bad in (torch.zeros((2, L + 1, N), device="cuda"), torch.zeros((2, L, N), device="cuda").double(), torch.zeros((2, L, N)),
                torch.zeros((2, N, L), device="cuda").transpose(1, 2)):
        with pytest.raises(ValueError, match="excess must be True, False or a contiguous torch.float32 CUDA tensor of shape"):
            eng.exceedance(z, xs, scale, mn, lv, excess=bad)
    with pytest.raises(ValueError, match="nothing to compute"):
        eng.exceedance(z, xs, scale, mn, lv, stats=False, excess=False)
    with pytest.raises(ValueError, match="side must be one of"):
        eng.exceedance(z, xs, scale, mn, lv, side="over")
    with pytest.raises(ValueError, match="scale must be"):
        eng.exceedance(z, xs, scale[:-1], mn, lv)
    # the C entry point itself: SGV_ERR_ARG before anything is enqueued, so the forward of a decode stays readable
    eng.set_eps(eps)
    eng.decode(z, xs, fix=True)
    xs_t = torch.stack(xs).contiguous()
    st = torch.full((2, 5, L, N), -777, dtype=torch.int32, device="cuda")
    ex = torch.full((2, L, N), 768.0, device="cuda")
    args = [z.data_ptr(), xs_t.data_ptr(), 2, 1, scale.data_ptr(), mn.data_ptr(), lv.data_ptr(), L, 0, st.data_ptr(), ex.data_ptr()]

    def rejected(msg, **kw):
        a = list(args)
        for i, v in kw.items():
            a[int(i[1:])] = v
        assert eng.lib.sgv_exceedance(eng.h, *a) == -1
        assert msg in eng.lib.sgv_last_error().decode(), eng.lib.sgv_last_error().decode()

    for i in (0, 4, 5, 6):          # z, scale, min, levels
        rejected("null argument", **{f"a{i}": None})
    rejected("no output", a9=None, a10=None)
    rejected("needs xs", a1=None)
    rejected("batch 0 outside", a2=0)
    rejected(f"batch {MAXB + 1} outside", a2=MAXB + 1)
    rejected("n_level = 0 is outside [1, 4]", a7=0)
    rejected("n_level = 5 is outside [1, 4]", a7=5)
    rejected("unknown side 2", a8=2)
    rejected("misaligned pointer", a6=lv.data_ptr() + 2)
    rejected("misaligned pointer", a9=st.data_ptr() + 4)
    rejected("misaligned pointer", a10=ex.data_ptr() + 8)
    assert eng.lib.sgv_exceedance(None, *args) == -1
    eng.xhat()
    torch.cuda.synchronize()
    assert bool((st == -777).all()) and bool((ex == 768.0).all())


def test_no_forward_to_read_after_exceedance_and_generate_is_unchanged():
    cfg, eng = engine("G0", "bf16")

    def run(z, xs, scale, mn, before):
        F = before.cpu().numpy()
        levels = XR.kernel_levels(F)
        out = eng.exceedance(z, xs, scale, mn, torch.from_numpy(levels).cuda())
        equals_emulation(out["stats"].cpu().numpy(), out["excess"].cpu().numpy(), F, levels, "above", "after decode")
    no_forward_after(eng, cfg, run, (eng.xhat, lambda: eng.backward(1.0, 1.0)))


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_training_is_unaffected_by_exceedance(dtype):
    lv = {}

    def run(eng, z, xs, scale, mn, i):
        if "lv" not in lv:
            lv["lv"] = torch.from_numpy(np.linspace(-1.0, 1.0, 4, dtype=np.float32)[:, None].repeat(eng.cfg.num_node, 1)).cuda()
        eng.exceedance(z, xs, scale, mn, lv["lv"], side=("above", "below")[i])
    training_unaffected(dtype, run, True)


# ---- Surrogate.exceedance on the fixture's models: P = 6 conditions, T = 12, N = 520 ----
@pytest.mark.parametrize("side", ["above", "below"])
@pytest.mark.parametrize("mode", ["fix", "random"])
@pytest.mark.parametrize("kind,dtype", [("img", "f32"), ("mlp", "bf16")])
def test_surrogate_exceedance_counts_what_predict_writes(kind, dtype, mode, side):
    s, x, _ = surrogate(kind, dtype, batch=8, seed=5)          # batch >= P: one call of the decoder each
    Fd = s.predict(x, mode=mode)
    F = Fd.cpu().numpy()
    P, T, N = F.shape
    levels = XR.kernel_levels(F)
    s, x, _ = surrogate(kind, dtype, batch=8, seed=5)          # a new Surrogate re-seeds the engine: the same draws again
    res = s.exceedance(x, levels, side=side, mode=mode)
    assert isinstance(res, ExceedanceResult) and res.side == side and res.T == T
    assert res.stats.dtype == torch.int32 and res.stats.shape == (P, 5, 4, N) and res.stats.is_contiguous()
    assert res.excess.dtype == torch.float32 and res.excess.shape == (P, 4, N) and res.excess.is_contiguous()
    assert res.count.shape == (P, 4, N) and res.levels.shape == (4, N) and np.array_equal(res.levels.cpu().numpy(), levels)
    result_equals_emulation(res, F, side, f"{kind} {dtype} {mode} {side}")
    # ever() is the question sweep's peak answers, asked of predict itself
    lv = torch.from_numpy(levels).cuda()
    beyond = Fd.amax(1).unsqueeze(1) > lv if side == "above" else Fd.amin(1).unsqueeze(1) < lv
    assert torch.equal(res.ever(), beyond)
    # worst() against torch on predict
    e = (Fd.unsqueeze(2) > lv) if side == "above" else (Fd.unsqueeze(2) < lv)          # [P, T, L, N]
    cnt = e.sum(1)
    node, steps = res.worst()
    assert torch.equal(steps.long(), cnt.max(dim=2).values)
    assert np.array_equal(node.cpu().numpy(), cnt.cpu().numpy().argmax(axis=2))          # numpy: the first occurrence
    assert torch.equal(res.fraction(), cnt.float() / T) and torch.equal(res.duration(0.5), cnt.float() * 0.5)


@pytest.mark.parametrize("mode", ["fix", "random"])
def test_the_batch_size_does_not_show(mode):
    """Batch sizes 1, 3, MAXB = 4 (4 + 2: a ragged last batch) and 8 give bitwise-equal results: the kernel gives a sample the same
    bits in any batch, and condition p takes row p of the noise streams one call over all conditions would draw from, whatever the
    batch (Engine.set_draw_row), so the draw position also ends where one call leaves it."""
    s, x, _ = surrogate("mlp", "f32", batch=8, seed=7)
    F = s.predict(x, mode=mode).cpu().numpy()
    draw = s.eng.train_state()["draw"]
    levels = XR.kernel_levels(F)[:3]
    runs, draws = [], []
    for batch in (1, 3, MAXB, 8):
        s, x, _ = surrogate("mlp", "f32", batch=batch, seed=7)
        runs.append(s.exceedance(x, levels, mode=mode))
        draws.append(s.eng.train_state()["draw"])
    assert all(r.stats.shape == (6, 5, 3, 520) and r.excess.shape == (6, 3, 520) for r in runs)
    for other in runs[1:]:
        same_bits(runs[0], other)
    assert len(set(draws)) == 1 and draws[0] == draw > 0
    # and the one call is predict's: the same draws, the same field
    result_equals_emulation(runs[0], F, "above", f"batch 1 against a one-call predict, {mode}")


def test_host_and_device_levels_scalars_vectors_and_rows():
    s, x, _ = surrogate("mlp", "f32", batch=8, seed=7)          # one call of the decoder: the draws exceedance gives at any batch size
    F = s.predict(x).cpu().numpy()
    N = F.shape[2]
    levels = XR.kernel_levels(F)[:2]
    s, x, _ = surrogate("mlp", "f32", batch=MAXB, seed=7)
    host = s.exceedance(x, levels)
    result_equals_emulation(host, F, "above", "host levels")
    s, x, _ = surrogate("mlp", "f32", batch=MAXB, seed=7)
    same_bits(s.exceedance(torch.from_numpy(x).cuda(), torch.from_numpy(levels).cuda()), host)
    s, x, _ = surrogate("mlp", "f32", batch=MAXB, seed=7)
    odd = torch.zeros(2 * N + 1, device="cuda")[1:].view(2, N)          # device levels at an odd offset
    odd.copy_(torch.from_numpy(levels))
    same_bits(s.exceedance(x, odd), host)
    s, x, _ = surrogate("mlp", "f32", batch=MAXB, seed=7)
    same_bits(s.exceedance(x, levels.astype(np.float64)), host)          # float64 host rows
    # a scalar and an [L] vector are broadcast over the nodes, on the host and on the device
    q = float(np.median(F))
    vec = np.float32([q, 0.5 * q, 2.0 * q])
    s, x, _ = surrogate("mlp", "f32", batch=MAXB, seed=7)
    one = s.exceedance(x, q)
    assert one.stats.shape == (6, 5, 1, N) and one.levels.shape == (1, N)
    result_equals_emulation(one, F, "above", "a scalar level")
    assert bool(one.ever().any()) and not bool(one.ever().all())
    s, x, _ = surrogate("mlp", "f32", batch=MAXB, seed=7)
    three = s.exceedance(x, vec, side="below")
    equals_emulation(three.stats.cpu().numpy(), three.excess.cpu().numpy(), F, np.repeat(vec[:, None], N, 1), "below", "an [L] vector of levels")
    s, x, _ = surrogate("mlp", "f32", batch=MAXB, seed=7)
    same_bits(s.exceedance(x, torch.from_numpy(vec).cuda(), side="below"), three)
    s, x, _ = surrogate("mlp", "f32", batch=MAXB, seed=7)
    same_bits(s.exceedance(x, torch.tensor(q, device="cuda")), one)
    # each output alone
    s, x, _ = surrogate("mlp", "f32", batch=MAXB, seed=7)
    steps = s.exceedance(x, levels, want=("steps",))
    assert steps.excess is None and torch.equal(steps.stats, host.stats)
    s, x, _ = surrogate("mlp", "f32", batch=MAXB, seed=7)
    exc = s.exceedance(x, levels, want=("excess",))
    assert exc.stats is None and torch.equal(exc.excess.view(torch.int32), host.excess.view(torch.int32))
    with pytest.raises(ValueError, match="levels: the last dimension is 519, expected N = 520"):
        s.exceedance(x, levels[:, :-1])
    with pytest.raises(ValueError, match="mode must be"):
        s.exceedance(x, levels, mode="mean")
    with pytest.raises(ValueError, match="side must be one of"):
        s.exceedance(x, levels, side="over")
    with pytest.raises(ValueError, match="want: a tuple of 'steps' and 'excess' is required"):
        s.exceedance(x, levels, want=("runs",))
    with pytest.raises(ValueError, match="want: nothing to compute"):
        s.exceedance(x, levels, want=())


def test_the_draw_row_is_reset_after_an_exception():
    """a batch that fails leaves the engine's draw row at 0: the next call of anything draws as if exceedance had never been called"""
    s, x, _ = surrogate("mlp", "f32", batch=2, seed=7)
    rows, calls = [], []
    set_draw_row, exceedance = s.eng.set_draw_row, s.eng.exceedance

    def recording(first_row):
        rows.append(int(first_row))
        return set_draw_row(first_row)

    def failing(*a, **kw):
        calls.append(1)
        if len(calls) == 2:
            raise RuntimeError("the second batch fails")
        return exceedance(*a, **kw)
    s.eng.set_draw_row, s.eng.exceedance = recording, failing
    try:
        with pytest.raises(RuntimeError, match="the second batch fails"):
            s.exceedance(x, [0.0, 1.0], mode="random")
    finally:
        del s.eng.set_draw_row, s.eng.exceedance
    assert rows == [0, 2, 0]          # the two batches that were started, then the reset
    # and the engine is as good as new: a fresh Surrogate on it gives the bits a larger batch gives
    s, x, _ = surrogate("mlp", "f32", batch=2, seed=7)
    a = s.exceedance(x, [0.0, 1.0], mode="random")
    s, x, _ = surrogate("mlp", "f32", batch=8, seed=7)
    same_bits(a, s.exceedance(x, [0.0, 1.0], mode="random"))
    assert E.MAX_LEVELS == 4
