"""Host side of the exact training checkpoints (no GPU): the checkpoint file's writer / reader, the atomic replace, the mismatch
messages, the data-parallel refusal and the declaration of the new entry points."""
import os
import random
import re

import numpy as np
import pytest
import torch

import simulgen_vae_amd  # noqa: F401
from simulgen_vae_amd import engine as E
from simulgen_vae_amd.modules import train as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["sgv_load_adam", "sgv_get_train_state", "sgv_set_train_state", "sgv_snapshot_floats", "sgv_snapshot_slice",
               "sgv_snapshot_begin", "sgv_snapshot_wait", "sgv_restore"]
HYPER = dict(epochs=6, batch_size=4, LR=1e-3, alpha=1e6, num_filter_enc=[32, 16, 8, 8], num_filter_dec=(8, 8, 16, 32), num_node=72,
             latent_dim=32, hierarchical_dim=8, num_time=10, lossfun="MSE", small=True, compute_dtype="bf16")
ROWS = [("a.bias", "value", 0, 8), ("a.bias", "exp_avg", 8, 8), ("a.bias", "exp_avg_sq", 16, 8), ("a.weight_u", "value", 24, 8)]


def payload(fill=1.0, epoch=2):
    arrays = {k: torch.arange(6, dtype=torch.float64) * (i + 1) for i, k in enumerate(("loss", "loss_val", "recon", "kl", "recon_val"))}
    return {"format": T.RESUME_FORMAT, "total": 32, "layout": [list(r) for r in ROWS], "buffer": torch.full((32,), fill),
            "train_state": {"step": 12, "seed": 0x5347564145, "draw": 14}, "epoch": epoch, "arrays": arrays,
            "loaders": {"train": {"epoch": 3, "indices": [4, 2, 7], "shuffle_seed": None}, "val": {"epoch": None, "indices": None, "shuffle_seed": None}},
            "rng": T.rng_state(), "hyper": T.resume_hyper(**HYPER)}


def test_checkpoint_file_round_trips(tmp_path):
    path = str(tmp_path / "resume.pt")
    random.seed(5); np.random.seed(6); torch.manual_seed(7)
    random.random(); np.random.beta(0.2, 0.2); torch.rand(3)
    p = payload()
    T.write_checkpoint(path, p)
    assert os.listdir(tmp_path) == ["resume.pt"]                # the temporary file is gone
    want = (random.random(), np.random.beta(0.2, 0.2), np.random.standard_normal(), torch.rand(3))
    random.seed(50); np.random.seed(60); torch.manual_seed(70)
    ck = T.read_checkpoint(path)                                 # the restricted unpickler: tensors and plain containers only
    assert ck["train_state"] == p["train_state"] and ck["epoch"] == 2 and ck["total"] == 32
    assert [tuple(r) for r in ck["layout"]] == ROWS
    assert torch.equal(ck["buffer"], p["buffer"]) and ck["buffer"].dtype == torch.float32
    for k, a in p["arrays"].items():
        assert torch.equal(ck["arrays"][k], a)
    assert ck["loaders"] == p["loaders"]
    assert ck["hyper"] == T.resume_hyper(**HYPER) and ck["hyper"]["num_filter_dec"] == [8, 8, 16, 32]
    T.set_rng_state(ck["rng"])                                   # all three generators continue where the payload was taken
    got = (random.random(), np.random.beta(0.2, 0.2), np.random.standard_normal(), torch.rand(3))
    assert got[:3] == want[:3] and torch.equal(got[3], want[3])
    T.check_resume_hyper(ck, T.resume_hyper(**HYPER))
    T.check_resume_layout(ck, 32, ROWS)


def test_a_failed_write_leaves_the_previous_checkpoint(tmp_path, monkeypatch):
    path = str(tmp_path / "resume.pt")
    T.write_checkpoint(path, payload(fill=1.0, epoch=2))
    real_save = torch.save

    def dying_save(obj, f, *a, **kw):
        real_save(obj, f, *a, **kw)
        with open(f, "r+b") as fh:                               # half a file on disk, then the writer dies
            fh.truncate(os.path.getsize(f) // 2)
        raise KeyboardInterrupt("killed")

    monkeypatch.setattr(T.torch, "save", dying_save)
    with pytest.raises(KeyboardInterrupt):
        T.write_checkpoint(path, payload(fill=2.0, epoch=5))
    monkeypatch.setattr(T.torch, "save", real_save)
    ck = T.read_checkpoint(path)
    assert ck["epoch"] == 2 and float(ck["buffer"][0]) == 1.0
    assert os.listdir(tmp_path) == ["resume.pt"]
    # a kill between the write and the replace: the torn temporary file does not stand in for the checkpoint
    monkeypatch.setattr(T.os, "replace", lambda a, b: (_ for _ in ()).throw(OSError("no replace")))
    with pytest.raises(OSError):
        T.write_checkpoint(path, payload(fill=3.0, epoch=8))
    assert T.read_checkpoint(path)["epoch"] == 2


def test_read_checkpoint_rejects_other_files(tmp_path):
    path = str(tmp_path / "weights.pth")
    torch.save({"w": torch.zeros(2)}, path)
    with pytest.raises(ValueError, match="not a resume checkpoint"):
        T.read_checkpoint(path)


@pytest.mark.parametrize("field,value", [("epochs", 8), ("LR", 2e-3), ("alpha", 1.0), ("batch_size", 8), ("num_filter_enc", [32, 16, 8, 16]),
                                         ("num_node", 80), ("num_time", 12), ("lossfun", "MAE"), ("small", False), ("compute_dtype", "f32"),
                                         ("latent_dim", 16), ("hierarchical_dim", 4)])
def test_hyper_parameter_mismatch_names_the_field(field, value):
    ck = payload()
    other = dict(HYPER)
    other[field] = value
    with pytest.raises(ValueError, match=rf"hyper-parameter '{field}' differs"):
        T.check_resume_hyper(ck, T.resume_hyper(**other))


def test_layout_mismatch_names_the_entry():
    ck = payload()
    rows = list(ROWS)
    rows[2] = ("a.bias", "exp_avg_sq", 16, 12)
    with pytest.raises(ValueError, match=r"layout entry 2 differs.*exp_avg_sq"):
        T.check_resume_layout(ck, 32, rows)
    with pytest.raises(ValueError, match=r"layout entry 4 differs.*b\.bias"):
        T.check_resume_layout(ck, 32, ROWS + [("b.bias", "value", 32, 4)])
    with pytest.raises(ValueError, match=r"'total' differs"):
        T.check_resume_layout(ck, 36, ROWS)


def test_loader_state_round_trip_and_mismatch():
    class Loader:
        def __init__(self, idx):
            self.indices, self.epoch, self.shuffle_seed = list(idx), 0, None

    a = Loader([4, 2, 7])
    a.epoch = 3
    st = T.loader_state(a)
    assert st == {"epoch": 3, "indices": [4, 2, 7], "shuffle_seed": None}
    b = Loader([7, 4, 2])
    T.set_loader_state(b, st, "train")
    assert b.indices == [4, 2, 7] and b.epoch == 3
    with pytest.raises(ValueError, match="train loader field 'indices' differs"):
        T.set_loader_state(Loader([1, 2]), st, "train")
    plain = [torch.zeros(1)]
    assert T.loader_state(plain) == {"epoch": None, "indices": None, "shuffle_seed": None}
    T.set_loader_state(plain, T.loader_state(plain), "val")
    with pytest.raises(ValueError, match="val loader field 'epoch' differs"):
        T.set_loader_state(plain, st, "val")


@pytest.mark.parametrize("kw", [dict(checkpoint_every=2), dict(resume_from="checkpoints/SimulGen-VAE_resume.pt")])
def test_data_parallel_resume_is_refused(kw, monkeypatch, tmp_path):
    monkeypatch.chdir(tmp_path)
    for name, value in (("is_available", True), ("is_initialized", True), ("get_rank", 0), ("get_world_size", 2)):
        monkeypatch.setattr(T.dist, name, lambda *a, _v=value, **k: _v)
    with pytest.raises(NotImplementedError, match="data-parallel resume is not built"):
        T.train(8, 4, [], [], 1e-3, [32, 16, 8, 8], [8, 8, 16, 32], 72, 32, 8, 10, 1e6, "MSE", True, True, **kw)
    assert os.listdir(tmp_path) == []                            # refused before anything is created


def test_new_arguments_are_keyword_only_and_default_off():
    import inspect
    sig = inspect.signature(T.train)
    for name, default in (("checkpoint_every", 0), ("resume_from", None)):
        p = sig.parameters[name]
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default == default
    assert list(sig.parameters)[:17] == ["epochs", "batch_size", "train_dataloader", "val_dataloader", "LR", "num_filter_enc", "num_filter_dec",
                                         "num_node", "latent_dim", "hierarchical_dim", "num_time", "alpha", "lossfun", "small", "load_all",
                                         "debug_mode", "compute_dtype"]


def test_new_symbols_are_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "sgvae.h")).read()
    declared = set(re.findall(r"\b(sgv_[a-z_0-9]+)\s*\(", hdr))
    lib = E.load_library()
    for s in NEW_SYMBOLS:
        assert s in declared and s in E.ABI_SYMBOLS, s
        assert getattr(lib, s).argtypes is not None, s
    for name in ("load_adam", "train_state", "set_train_state", "snapshot_layout", "snapshot_begin", "snapshot_wait", "restore"):
        assert callable(getattr(E.Engine, name))
    from simulgen_vae_amd.modules.VAE_network import VAE
    assert callable(VAE.optimizer_state_dict) and callable(VAE.load_optimizer_state_dict)
