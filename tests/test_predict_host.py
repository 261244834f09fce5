"""Host side of surrogate prediction (no GPU): the scaler and size checks of Surrogate.__init__ (numpy only, raised before anything
touches the device), the missing-file message of from_files, and the declaration / binding of the new entry points."""
import os
import re
import types

import numpy as np
import pytest

import simulgen_vae_amd  # noqa: F401
from simulgen_vae_amd import engine as E
from simulgen_vae_amd.predict import FILES, Surrogate
from simulgen_vae_amd.spec import VAEConfig

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["sgv_generate", "sgv_test_recon_physical", "sgv_copy_stream"]
CFG = VAEConfig(32, 8, [32, 16, 8, 8], [8, 8, 16, 32], 72, 10, "MSE", True)


class NoGpuVAE:
    """stands where the mirror VAE goes; reaching for the engine is a test failure"""
    cfg = CFG

    def _eng(self, batch=None):
        raise AssertionError("the engine was asked for before the arguments were checked")


def parts(latent_end=32, size2=3, latent=8):
    lc = types.SimpleNamespace(latent_dim_end=latent_end, size2=size2, latent_dim=latent, eval=lambda: lc)
    sc = lambda n: types.SimpleNamespace(scale_=np.linspace(0.5, 2.0, n), min_=np.linspace(-1.0, 1.0, n))
    return NoGpuVAE(), lc, sc(latent_end), sc(size2 * latent), sc(CFG.num_node)


@pytest.mark.parametrize("which,name", [(2, "latent_scaler"), (3, "xs_scaler"), (4, "data_scaler")])
@pytest.mark.parametrize("value", [0.0, float("nan"), float("inf"), 1e-60])
def test_bad_scale_names_scaler_and_index(which, name, value):
    p = list(parts())
    p[which].scale_ = p[which].scale_.copy()
    p[which].scale_[5] = value                      # 1e-60 is zero in float32, the precision the kernels divide in
    with pytest.raises(ValueError, match=rf"{name}: scale_\[5\]"):
        Surrogate(*p)


@pytest.mark.parametrize("which,name,what", [(2, "latent_scaler", "latent_dim_end = 32"), (3, "xs_scaler", r"size2 \* latent_dim = 24"),
                                             (4, "data_scaler", "num_node = 72")])
def test_length_mismatch_names_scaler_and_size(which, name, what):
    p = list(parts())
    p[which] = types.SimpleNamespace(scale_=np.ones(7), min_=np.zeros(7))
    with pytest.raises(ValueError, match=rf"{name}: .*7 / 7 entries, expected {what}"):
        Surrogate(*p)
    p = list(parts())
    p[which].min_ = p[which].min_[:-1]
    with pytest.raises(ValueError, match=name):
        Surrogate(*p)


def test_conditioner_and_vae_must_agree():
    with pytest.raises(ValueError, match="the conditioner predicts latents"):
        Surrogate(*parts(latent_end=16))
    with pytest.raises(ValueError, match="the conditioner predicts latents"):
        Surrogate(*parts(size2=2))
    with pytest.raises(ValueError, match="scale_ and min_"):
        p = list(parts())
        p[2] = object()
        Surrogate(*p)


def test_checks_pass_then_the_engine_is_asked_for():
    with pytest.raises(AssertionError, match="the engine was asked for"):
        Surrogate(*parts())


def test_from_files_names_the_missing_file(tmp_path):
    d = tmp_path / "model_save"
    d.mkdir()
    order = list(FILES.values())
    assert sorted(order) == sorted(["SimulGen-VAE", "LatentConditioner", "scaler.pkl", "latent_vectors_scaler.pkl", "xs_scaler.pkl"])
    for k, fname in enumerate(order):
        with pytest.raises(FileNotFoundError, match=re.escape(str(d / fname))):
            Surrogate.from_files(str(d))
        (d / fname).write_bytes(b"")
    with pytest.raises(FileNotFoundError, match="SimulGen-VAE"):
        Surrogate.from_files(str(tmp_path / "nowhere"))


def test_new_symbols_are_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "sgvae.h")).read()
    declared = set(re.findall(r"\b(sgv_[a-z_0-9]+)\s*\(", hdr))
    lib = E.load_library()
    for s in NEW_SYMBOLS:
        assert s in declared and s in E.ABI_SYMBOLS, s
        assert getattr(lib, s).argtypes is not None, s
    assert len(lib.sgv_generate.argtypes) == 9 and len(lib.sgv_test_recon_physical.argtypes) == 14
    for name in ("generate", "copy_stream"):
        assert callable(getattr(E.Engine, name))
    import inspect
    sig = inspect.signature(E.Engine.generate)
    assert list(sig.parameters) == ["self", "z", "xs", "scale", "min", "out", "layout", "fix"]
    assert sig.parameters["out"].default is None and sig.parameters["layout"].default == "TN" and sig.parameters["fix"].default is True
    sig = inspect.signature(Surrogate.__init__)
    assert list(sig.parameters) == ["self", "vae", "conditioner", "latent_scaler", "xs_scaler", "data_scaler", "batch", "seed"]
    assert sig.parameters["batch"].default == 16 and sig.parameters["seed"].default == 0
    for m in (Surrogate.predict, Surrogate.predict_to_host):
        assert list(inspect.signature(m).parameters) == ["self", "conditions", "out", "layout", "mode"]


def test_layout_strings_map_to_the_header_constants():
    hdr = open(os.path.join(ROOT, "include", "sgvae.h")).read()
    consts = {k: int(v) for k, v in re.findall(r"SGV_LAYOUT_([A-Z]+)\s*=\s*(\d+)", hdr)}
    assert consts == {"TN": 0, "NT": 1} and E.LAYOUTS == consts


def test_surrogate_is_not_part_of_the_reference_api():
    import sys
    simulgen_vae_amd.install_reference_api()
    assert "modules.predict" not in sys.modules
