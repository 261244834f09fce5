"""Exact training checkpoints on the GPU: the whole-state snapshot (device permute kernels, csrc/engine_ckpt.hip) against the
per-tensor exports, its isolation from the step that follows it, restore + continue, the per-tensor optimizer state, the
torch.optim.AdamW state-dict format and the resume of modules.train.train.

Every comparison is bitwise (np.array_equal on the raw 32-bit patterns): the snapshot path only moves data, and the engine replays
a step bit for bit, so a resumed run has no tolerance to hide behind."""
import os

import numpy as np
import pytest
import torch

import simulgen_vae_amd  # noqa: F401
from simulgen_vae_amd import engine as E
from simulgen_vae_amd.init import init_state, synthetic_samples
from simulgen_vae_amd.spec import layer_list
from tests.gpu_common import G0, G1, make_cfg

pytestmark = pytest.mark.gpu

# channel widths that are multiples of 8 but not of the permute kernel's 64-wide tile, num_node = 72: every tile edge is partial
GX = dict(latent_dim=32, hierarchical_dim=8, enc=[136, 72, 40, 8], num_node=72, num_time=10)
ALPHA, BETA, LR = 1e4, 1e-3, 1e-3
B = 3


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same(a, b):
    a, b = bits(a), bits(b)
    return a.shape == b.shape and np.array_equal(a, b)


def make_engine(cfg, dtype, init_seed=7, grad_bf16=False):
    eng = E.Engine(cfg, max_batch=B, compute_dtype=dtype)
    eng.load_state(init_state(cfg, init_seed))
    if grad_bf16:
        eng.set_option("grad_bf16", 1)
    return eng


def batch(cfg, k):
    return torch.from_numpy(synthetic_samples(4242, range(k * B, (k + 1) * B), cfg.num_node, cfg.num_time)).cuda()


def step(eng, cfg, k, sync=True):
    """forward(train) + backward_step on batch k with engine-drawn noise; (scalars, gradient norm of the step)."""
    eng.set_input(batch(cfg, k))
    sc = eng.forward(train=True, sync=sync)
    eng.backward_step(ALPHA, BETA, LR)
    return sc


def export_all(eng):
    """{(key, part): array}: what sgv_export_state / sgv_export_adam return, tensor by tensor."""
    out = {(k, "value"): v for k, v in eng.state_dict().items()}
    for name, _shape, _kind, has_grad in eng.param_info():
        if has_grad:
            m, v = eng.adam_state(name)
            out[(name, "exp_avg")], out[(name, "exp_avg_sq")] = m, v
    return out


def snapshot(eng):
    buf = torch.empty(eng.snapshot_floats(), dtype=torch.float32).pin_memory()
    eng.snapshot_begin(buf)
    eng.snapshot_wait()
    return buf


def assert_buffer_equals(eng, buf, want):
    total, rows = eng.snapshot_layout()
    assert total == buf.numel() and len(rows) == len(want)
    flat = buf.numpy()
    covered = 0
    for name, part, off, cnt in rows:
        ref = want[(name, part)]
        assert cnt == ref.size, (name, part)
        assert same(flat[off:off + cnt], ref.reshape(-1)), (name, part)
        covered += cnt
    assert covered == total           # the slices tile the buffer: no gap, no overlap (offsets ascend in layout order)
    assert [r[2] for r in rows] == sorted(r[2] for r in rows)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("cfgd,small", [(G0, True), (G0, False), (G1, True), (G1, False), (GX, True)], ids=["g0s", "g0l", "g1s", "g1l", "gx"])
def test_snapshot_equals_per_tensor_export(cfgd, small, dtype):
    cfg = make_cfg(cfgd, small)
    # the state holds every case of the host permutation: Conv1d with several taps, ConvTranspose1d, both Linear kinds (head:
    # the encoder's, K = C * T; expand: the decoder's, O = C * T), their v vectors, GroupNorm
    L = layer_list(cfg)
    assert any(l.op == "conv" and l.k > 1 for l in L) and any(l.op == "convT" and l.k > 1 for l in L) and any(l.op == "gn" for l in L)
    assert any(l.op == "linear" and l.prefix.startswith("encoder.") for l in L)
    assert any(l.op == "linear" and l.prefix.startswith("decoder.") for l in L)
    assert cfg.num_time != cfg.num_filter_enc[-1]          # a transposed head permutation cannot pass by accident
    eng = make_engine(cfg, dtype)
    try:
        keys = {r[0] for r in eng.snapshot_layout()[1]}
        for l in L:
            if l.op != "gn":
                assert f"{l.prefix}.weight_orig" in keys and f"{l.prefix}.weight_v" in keys and f"{l.prefix}.weight_u" in keys
        for k in range(2):                                  # two steps: both moments are non-zero and differ from each other
            step(eng, cfg, k)
        want = export_all(eng)
        m = want[("decoder.recon.0.weight_orig", "exp_avg")]
        assert np.abs(m).max() > 0
        assert_buffer_equals(eng, snapshot(eng), want)
    finally:
        eng.close()


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_snapshot_is_isolated_from_the_next_step(dtype):
    cfg = make_cfg(G1, True)
    eng = make_engine(cfg, dtype)
    try:
        for k in range(2):
            step(eng, cfg, k)
        before = export_all(eng)
        x = batch(cfg, 2)
        buf = torch.empty(eng.snapshot_floats(), dtype=torch.float32).pin_memory()
        eng.snapshot_begin(buf)
        with pytest.raises(E.SgvError, match=r"\(-3\)"):     # a second snapshot before the first has been waited for
            eng.snapshot_begin(buf)
        eng.set_input(x)                                    # the next step is enqueued while the copy is in flight
        eng.forward(train=True, sync=False)
        eng.backward_step(ALPHA, BETA, LR)
        eng.snapshot_wait()
        after = export_all(eng)
        assert_buffer_equals(eng, buf, before)
        total, rows = eng.snapshot_layout()
        changed = [r for r in rows if not same(buf.numpy()[r[2]:r[2] + r[3]], after[(r[0], r[1])].reshape(-1))]
        assert len(changed) > len(rows) // 2                # the step did move the state the buffer no longer follows
    finally:
        eng.close()


@pytest.mark.parametrize("dtype,grad_bf16", [("f32", False), ("bf16", False), ("bf16", True)], ids=["f32", "bf16", "bf16-gradbf16"])
@pytest.mark.parametrize("cfgd,small", [(G1, True), (G0, False)], ids=["g1s", "g0l"])
def test_restore_then_continue_is_bitwise(cfgd, small, dtype, grad_bf16):
    cfg = make_cfg(cfgd, small)
    a = make_engine(cfg, dtype, init_seed=7, grad_bf16=grad_bf16)
    b = make_engine(cfg, dtype, init_seed=11, grad_bf16=grad_bf16)
    try:
        a.seed(1234)
        b.seed(99)
        for k in range(2):
            step(a, cfg, k)
        buf = snapshot(a)
        st = a.train_state()
        assert st["step"] == 2 and st["seed"] == 1234 and st["draw"] >= 2        # every noise tensor drawn advances the position
        assert not same(b.state_dict()["decoder.recon.0.weight_orig"], a.state_dict()["decoder.recon.0.weight_orig"])
        b.restore(buf.clone())                              # an unpinned copy: restore takes either
        b.set_train_state(**st)
        assert b.train_state() == st
        wa, wb = export_all(a), export_all(b)
        assert wa.keys() == wb.keys()
        for key in wa:
            assert same(wa[key], wb[key]), key
        for k in range(2, 4):
            sa, sb = step(a, cfg, k), step(b, cfg, k)
            assert sa == sb, (k, sa, sb)
            assert a.last_grad_norm() == b.last_grad_norm(), k
            wa, wb = export_all(a), export_all(b)
            bad = [key for key in wa if not same(wa[key], wb[key])]
            assert not bad, (k, bad[:8], len(bad))
        assert a.train_state() == b.train_state() == dict(step=4, seed=1234, draw=2 * st["draw"])
    finally:
        a.close()
        b.close()


def test_load_adam_round_trip_and_errors():
    cfg = make_cfg(G0, True)
    a = make_engine(cfg, "f32")
    b = make_engine(cfg, "f32", init_seed=11)
    try:
        for k in range(2):
            step(a, cfg, k)
        names = [n for n, _s, _k, hg in a.param_info() if hg]
        assert len(names) > 20
        for n in names:
            m, v = a.adam_state(n)
            b.load_adam(n, m, v)
        for n in names:
            (ma, va), (mb, vb) = a.adam_state(n), b.adam_state(n)
            assert same(ma, mb) and same(va, vb), n
        # one moment alone
        n0 = "decoder.recon.0.weight_orig"
        m, v = a.adam_state(n0)
        b.load_adam(n0, exp_avg=np.zeros_like(m))
        mb, vb = b.adam_state(n0)
        assert not mb.any() and same(vb, v)
        lib, C = b.lib, E.C
        z = np.zeros(m.size + 4, np.float32)
        p = z.ctypes.data_as(C.c_void_p)
        assert lib.sgv_load_adam(b.h, b"no.such.key", p, p, m.size) == -4                      # SGV_ERR_NAME
        assert lib.sgv_load_adam(b.h, n0.encode(), p, p, m.size + 4) == -1                      # SGV_ERR_ARG: size
        dead = next(n for n, _s, kind, hg in b.param_info() if not hg and kind == 1)
        assert lib.sgv_load_adam(b.h, dead.encode(), p, p, m.size) == -1                        # SGV_ERR_ARG: no optimizer state
        assert b"no optimizer state" in lib.sgv_last_error()
        u = next(n for n, _s, kind, _hg in b.param_info() if kind == 2)
        with pytest.raises(E.SgvError):
            b.load_adam(u, np.zeros(4, np.float32), np.zeros(4, np.float32))
        mb2, vb2 = b.adam_state(n0)                                                              # nothing was written by the refused calls
        assert same(mb2, mb) and same(vb2, vb)
        # the train state: set keeps the draw position (seed() resets it); bad reserved slot is refused
        b.set_train_state(step=5, seed=77, draw=9)
        assert b.train_state() == dict(step=5, seed=77, draw=9)
        b.seed(78)
        assert b.train_state() == dict(step=5, seed=78, draw=0)
        bad = (C.c_uint64 * 4)(1, 2, 3, 4)
        assert lib.sgv_set_train_state(b.h, bad) == -1
        # refused while an AdamW step is open
        b.set_input(batch(cfg, 0))
        b.forward(train=True)
        b.backward(ALPHA, BETA)
        nb = b.bucket_count()
        b.adamw_step_range(LR, 0, 1, True, False)
        ok = (C.c_uint64 * 4)(1, 2, 3, 0)
        assert lib.sgv_set_train_state(b.h, ok) == -3                                            # SGV_ERR_STATE
        b.adamw_step_range(LR, 1, nb, False, True)
        assert lib.sgv_set_train_state(b.h, ok) == 0
        # the binding refuses a wrong-sized or pageable snapshot buffer before any launch
        n = b.snapshot_floats()
        with pytest.raises(ValueError, match="pinned"):
            b.snapshot_begin(torch.empty(n, dtype=torch.float32))
        with pytest.raises(ValueError, match="floats"):
            b.snapshot_begin(torch.empty(n + 1, dtype=torch.float32).pin_memory())
        with pytest.raises(ValueError):
            b.restore(torch.empty(n, dtype=torch.float64))
    finally:
        a.close()
        b.close()


def test_optimizer_state_dict_is_torch_adamw_format():
    from simulgen_vae_amd.modules.VAE_network import VAE
    enc = G0["enc"]

    def model(seed):
        return VAE(G0["latent_dim"], G0["hierarchical_dim"], enc, enc[::-1], G0["num_node"], G0["num_time"], lossfun="MSE", batch_size=B,
                   small=True, compute_dtype="f32", seed=seed)

    m = model(7)
    fresh = model(11)
    try:
        cfg = m.cfg
        assert m.optimizer_state_dict()["state"] == {}                     # no step yet: torch's AdamW has no state either
        for k in range(2):
            m.training_step(batch(cfg, k), ALPHA, BETA, LR)
        osd = m.optimizer_state_dict(lr=LR)
        eng = m._eng()
        keys = [(e.name, e.shape, e.trainable) for e in eng.spec if e.kind in ("bias", "weight_orig", "gn_weight", "gn_bias")]
        assert [k for k, _ in m._param_keys()] == [k for k, _s, _t in keys]
        # torch's own validation: the dict loads into an AdamW over parameters of these shapes, in state_dict order
        params = [torch.nn.Parameter(torch.zeros(s)) for _k, s, _t in keys]
        opt = torch.optim.AdamW(params, lr=LR)
        assert set(osd["param_groups"][0]) == set(opt.state_dict()["param_groups"][0])
        opt.load_state_dict(osd)
        dead = [i for i, (_k, _s, t) in enumerate(keys) if not t]
        assert len(dead) == 22 and not any(i in osd["state"] for i in dead)
        assert sorted(osd["state"]) == [i for i, (_k, _s, t) in enumerate(keys) if t]
        for i, (name, shape, t) in enumerate(keys):
            if not t:
                assert params[i] not in opt.state
                continue
            st = opt.state[params[i]]
            mm, vv = eng.adam_state(name)
            assert float(st["step"]) == 2.0 and tuple(st["exp_avg"].shape) == tuple(shape)
            assert same(st["exp_avg"].numpy(), mm) and same(st["exp_avg_sq"].numpy(), vv), name
        fresh.load_optimizer_state_dict(osd)
        fe = fresh._eng()
        assert fe.train_state()["step"] == 2
        for name, _shape, t in keys:
            if t:
                (ma, va), (mb, vb) = eng.adam_state(name), fe.adam_state(name)
                assert same(ma, mb) and same(va, vb), name
        bad = {"state": {dead[0]: osd["state"][sorted(osd["state"])[0]]}, "param_groups": osd["param_groups"]}
        with pytest.raises(ValueError, match="never gets a gradient"):
            fresh.load_optimizer_state_dict(bad)
    finally:
        for mod in (m, fresh):
            if mod._engine is not None:
                mod._engine.close()


LOOP_ENC = [1024, 512, 256, 128]


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_train_loop_resume_is_bitwise(dtype, tmp_path, monkeypatch):
    """The arguments of tests/test_loop_gpu.py (the minimum sizes the reference's loop accepts: preset filters, N = 4096, T = 32,
    batch 4, 8 + 4 samples), 6 epochs, engine-drawn noise.  Run A checkpoints every 3 epochs; run B resumes from A's epoch-3 file
    under other seeds; run C never hears of checkpoints."""
    import random
    from simulgen_vae_amd.modules import train as T
    N, Tn, Bn, EPOCHS = 4096, 32, 4, 6
    train_batches = [torch.from_numpy(synthetic_samples(20251003, range(i * Bn, (i + 1) * Bn), N, Tn)) for i in range(2)]
    val_batches = [torch.from_numpy(synthetic_samples(20251003, range(100, 100 + Bn), N, Tn))]

    def seed(s):
        random.seed(s); np.random.seed(s); torch.manual_seed(s)

    def run(where, epochs=EPOCHS, **kw):
        os.makedirs(where, exist_ok=True)
        monkeypatch.chdir(where)
        out = T.train(epochs, Bn, train_batches, val_batches, 1e-3, LOOP_ENC, LOOP_ENC[::-1], N, 32, 8, Tn, 1e6, "MSE", True, True,
                      compute_dtype=dtype, **kw)
        sd = {k: v.numpy() for k, v in T.train.last_model.state_dict().items()}
        T.train.last_model._engine.close()
        return [np.array(a, copy=True) for a in out], sd

    written = []
    real_write = T.write_checkpoint

    def keeping_write(path, payload):
        real_write(path, payload)
        written.append(int(payload["epoch"]))
        if payload["epoch"] == 2:
            os.link(path, "resume_after_epoch3.pt")      # the replace at epoch 6 leaves this name on the old file
    monkeypatch.setattr(T, "write_checkpoint", keeping_write)

    seed(1)
    a_out, a_sd = run(tmp_path / "a", checkpoint_every=3)
    assert written == [2, 5]
    mid = str(tmp_path / "a" / "resume_after_epoch3.pt")
    assert os.path.exists(tmp_path / "a" / T.RESUME_PATH) and not os.path.exists(str(tmp_path / "a" / T.RESUME_PATH) + ".tmp")
    monkeypatch.setattr(T, "write_checkpoint", real_write)

    seed(2)
    b_out, b_sd = run(tmp_path / "b", resume_from=mid)
    for x, y in zip(a_out, b_out):
        assert x.dtype == y.dtype and np.array_equal(x.view(np.uint64), y.view(np.uint64)), (x, y)
    assert a_sd.keys() == b_sd.keys()
    bad = [k for k in a_sd if not same(a_sd[k], b_sd[k])]
    assert not bad, (bad[:8], len(bad))
    assert not os.path.exists(tmp_path / "b" / T.RESUME_PATH)

    seed(1)
    c_out, c_sd = run(tmp_path / "c")
    for x, y in zip(a_out, c_out):
        assert np.array_equal(x.view(np.uint64), y.view(np.uint64)), (x, y)
    bad = [k for k in a_sd if not same(a_sd[k], c_sd[k])]
    assert not bad, (bad[:8], len(bad))
    assert not os.path.exists(tmp_path / "c" / T.RESUME_PATH)      # no arguments, no resume file

    with pytest.raises(ValueError, match="hyper-parameter 'epochs' differs"):
        run(tmp_path / "d", epochs=8, resume_from=mid)
