"""CPU checks of the parametric (CSV) latent conditioner's host side: the reference module path resolves, the parameter
spec equals the reference state_dict recorded in the fixtures (keys, order, shapes), the head-width rule, the CSV reader,
and the torch restatement used by the GPU tests against the reference's recorded eval outputs."""
import os

import numpy as np
import pandas as pd
import torch

import simulgen_vae_amd
from simulgen_vae_amd.init import lc_init_state
from tests.mlp_lc_torch import TorchMLPConditioner

GOLD = os.path.join(os.path.dirname(__file__), "golden")
FIXTURES = ("mlp_lc_small", "mlp_lc_preset")


def _meta(g):
    latent_end, latent, size2, input_shape, B = (int(v) for v in g["meta"][:5])
    return [int(v) for v in g["filters"]], latent_end, input_shape, latent, size2, B


def test_reference_module_path_resolves():
    simulgen_vae_amd.install_reference_api()
    from modules.latent_conditioner_model_parametric import LatentConditioner
    from modules.latent_conditioner import read_latent_conditioner_dataset  # noqa: F401
    assert LatentConditioner.__module__.endswith("modules.latent_conditioner_model_parametric")


def test_param_spec_equals_reference_state_dict():
    from simulgen_vae_amd.modules.latent_conditioner_model_parametric import param_spec
    for name in FIXTURES:
        g = np.load(os.path.join(GOLD, name + ".npz"))
        filters, latent_end, input_shape, latent, size2, _ = _meta(g)
        spec = param_spec(filters, latent_end, input_shape, latent, size2)
        assert [n for n, _ in spec] == list(g["keys"]), name
        assert [str(tuple(s)) for _, s in spec] == list(g["shapes"]), name


def test_head_width_rule():
    from simulgen_vae_amd.modules.latent_conditioner_model_parametric import dropout_sites, head_width, param_spec
    assert head_width(32, 600, 600) == 75                   # 600 // min(8, max(2, 600 // 64)) = 600 // 8
    assert head_width(32, 1024, 16) == 512                  # ratio floors at 2
    assert head_width(32, 64, 16) == 64                     # and the width at 2 * latent_dim_end
    assert head_width(32, 1024, 4096) == 128                # and the ratio caps at 8
    shapes = dict(param_spec([48, 600, 600], 32, 600, 8, 3))
    assert shapes["latent_out.0.weight"] == (75, 600) and shapes["latent_out.4.weight"] == (37, 75)
    assert shapes["xs_out.8.weight"] == (24, 37)
    sites = dropout_sites([48, 600, 600], 32, 600, 0.3)
    assert [s for s, _, _ in sites] == ["backbone.0", "backbone.1", "backbone.2", "feature_projection",
                                        "latent_out.3", "latent_out.7", "xs_out.3", "xs_out.7"]
    np.testing.assert_allclose([p for _, _, p in sites], [0.15, 0.21, 0.3, 0.24, 0.18, 0.12, 0.18, 0.12])
    for name in FIXTURES:
        assert len(sites if name == "mlp_lc_small" else dropout_sites([32, 64, 128, 256, 512, 1024], 32, 16, 0.3)) == \
            int(np.load(os.path.join(GOLD, name + ".npz"))["n_masks"][0])


def test_csv_reader_reads_headerless_rows(tmp_path):
    from simulgen_vae_amd.modules.latent_conditioner import read_latent_conditioner_dataset
    rng = np.random.default_rng(3)
    a = rng.standard_normal((6, 7))
    path = tmp_path / "params.csv"
    np.savetxt(path, a, delimiter=",")
    got = read_latent_conditioner_dataset(str(path), ".csv")
    want = pd.read_csv(str(path), header=None).values
    assert got.shape == (6, 7)                              # the first row is data, not a header
    np.testing.assert_array_equal(got, want)


def test_torch_restatement_matches_reference_eval_outputs():
    for name in FIXTURES:
        g = np.load(os.path.join(GOLD, name + ".npz"))
        filters, latent_end, input_shape, latent, size2, _ = _meta(g)
        m = TorchMLPConditioner(filters, latent_end, input_shape, latent, size2)
        state = lc_init_state({k: tuple(v.shape) for k, v in m.state_dict().items()}, int(g["meta"][5]))
        m.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()})
        m.eval()
        with torch.no_grad():
            e1, e2 = m(torch.from_numpy(g["x"]))
        np.testing.assert_allclose(e1.numpy(), g["eval_main"], rtol=0, atol=1e-5)
        np.testing.assert_allclose(e2.numpy(), g["eval_xs"], rtol=0, atol=1e-5)
