"""Host side of surrogate scoring (no GPU): predict.truth_fields, the numpy-only validator of Surrogate.score's held-out fields,
ScoreResult, and the declaration / binding of the new entry points."""
import os
import re

import numpy as np
import pytest

import simulgen_vae_amd  # noqa: F401
from simulgen_vae_amd import engine as E
from simulgen_vae_amd.predict import ScoreResult, Surrogate, truth_fields

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["sgv_score", "sgv_test_recon_score"]
P, T, N = 3, 5, 8


def test_float32_array_and_cpu_tensor_are_accepted_as_they_are():
    import torch
    a = np.zeros((P, T, N), np.float32)
    assert truth_fields(a, P, T, N) is a
    t = torch.zeros((P, T, N), dtype=torch.float32)
    assert truth_fields(t, P, T, N) is t
    assert truth_fields(np.zeros((0, T, N), np.float32), 0, T, N).shape == (0, T, N)


@pytest.mark.parametrize("shape", [(), (N,), (T, N), (P, T, N, 1)])
def test_wrong_rank_is_rejected(shape):
    with pytest.raises(ValueError, match=r"truth: a \[P, T, N\] array is required, got shape " + re.escape(str(shape))):
        truth_fields(np.zeros(shape, np.float32), P, T, N)


@pytest.mark.parametrize("shape,name,got,want", [((P + 1, T, N), "P", P + 1, P), ((P, T - 1, N), "T", T - 1, T), ((P, T, N + 8), "N", N + 8, N),
                                                 ((P, N, T), "T", N, T)])
def test_each_wrong_dimension_is_named(shape, name, got, want):
    import torch
    for a in (np.zeros(shape, np.float32), torch.zeros(shape, dtype=torch.float32)):
        with pytest.raises(ValueError, match=rf"truth: dimension {name} is {got}, expected {name} = {want}"):
            truth_fields(a, P, T, N)


def test_other_dtypes_are_rejected():
    import torch
    for a, name in ((np.zeros((P, T, N), np.float64), "float64"), (np.zeros((P, T, N), np.float16), "float16"), (np.zeros((P, T, N), np.int32), "int32"),
                    (torch.zeros((P, T, N), dtype=torch.float64), "torch.float64"), (torch.zeros((P, T, N), dtype=torch.bfloat16), "torch.bfloat16"),
                    ([[[0.0] * N] * T] * P, "float64")):
        with pytest.raises(ValueError, match=rf"truth: dtype float32 is required, not {re.escape(name)}"):
            truth_fields(a, P, T, N)


def test_score_result_lists_the_eleven_fields():
    assert ScoreResult.FIELDS == ("node_max_abs", "node_bias", "node_mse", "t_worst", "frame_max_abs", "frame_mse", "frame_truth_ms", "n_worst",
                                  "rmse", "rel_l2", "max_abs")
    r = ScoreResult(**{k: i for i, k in enumerate(ScoreResult.FIELDS)})
    assert tuple(getattr(r, k) for k in ScoreResult.FIELDS) == tuple(range(11))
    with pytest.raises(KeyError):
        ScoreResult(node_max_abs=0)


def test_surrogate_and_engine_have_score():
    assert callable(Surrogate.score) and callable(E.Engine.score)
    assert E.SCORE_PARTS == ("node", "frame")


def test_new_entry_points_are_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "sgvae.h")).read()
    for s in NEW_SYMBOLS:
        assert re.search(rf"\bint {s}\s*\(", hdr), s
        assert s in E.ABI_SYMBOLS
    assert re.search(r"\}\s*sgv_score_out;", hdr)
    assert [f for f, _ in E.ScoreOut._fields_] == ["node_err", "node_when", "frame_err", "frame_where"]
    lib = E.load_library()
    for s in NEW_SYMBOLS:
        assert hasattr(lib, s), s
    assert len(lib.sgv_score.argtypes) == 9 and len(lib.sgv_test_recon_score.argtypes) == 14
    # without an engine the call is an argument error that says who complains
    assert lib.sgv_score(None, None, None, 1, 1, None, None, None, None) == -1 and "sgv_score" in lib.sgv_last_error().decode()
    assert lib.sgv_test_recon_score(0, None, 8, None, None, None, None, None, None, None, 1, 1, 8, None) == -1
    assert "sgv_test_recon_score: null argument" in lib.sgv_last_error().decode()
