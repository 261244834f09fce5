"""Host side of the surrogate field summaries (no GPU): predict.probe_nodes, the numpy-only validator of Surrogate.sweep's probe
list, and the declaration / binding of the new entry points."""
import os
import re

import numpy as np
import pytest

import simulgen_vae_amd  # noqa: F401
from simulgen_vae_amd import engine as E
from simulgen_vae_amd.predict import MAX_PROBES, SweepResult, probe_nodes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["sgv_set_probes", "sgv_summarize", "sgv_test_recon_summary"]
N = 72


def test_valid_list_keeps_order_and_duplicates():
    got = probe_nodes([71, 0, 5, 5, 3], N)
    assert got.dtype == np.int32 and got.tolist() == [71, 0, 5, 5, 3]
    assert probe_nodes(np.array([7], np.int64), N).tolist() == [7]
    assert probe_nodes(np.arange(MAX_PROBES, dtype=np.uint16) % N, N).shape == (MAX_PROBES,)


def test_empty_and_too_long_lists_are_rejected():
    with pytest.raises(ValueError, match=r"probes: 0 entries, between 1 and 4096"):
        probe_nodes(np.zeros(0, np.int32), N)
    with pytest.raises(ValueError, match=r"probes: 4097 entries, between 1 and 4096"):
        probe_nodes(np.zeros(MAX_PROBES + 1, np.int32), N)


@pytest.mark.parametrize("nodes,pos,value", [([3, -1, 99], 1, -1), ([3, 4, 72, -5], 2, 72), ([N], 0, N), (np.array([0, 2 ** 40], np.int64), 1, 2 ** 40)])
def test_index_out_of_range_names_the_first_bad_position(nodes, pos, value):
    with pytest.raises(ValueError, match=rf"probes\[{pos}\] = {value} is outside \[0, 72\)"):
        probe_nodes(nodes, N)


def test_non_integer_dtype_and_wrong_rank_are_rejected():
    with pytest.raises(ValueError, match="integer dtype is required, not float64"):
        probe_nodes([1.0, 2.0], N)
    with pytest.raises(ValueError, match="integer dtype is required, not bool"):
        probe_nodes([True, False], N)
    with pytest.raises(ValueError, match=r"1-D array of node indices is required, got shape \(2, 2\)"):
        probe_nodes([[1, 2], [3, 4]], N)
    with pytest.raises(ValueError, match=r"1-D array of node indices is required, got shape \(\)"):
        probe_nodes(5, N)


def test_sweep_result_holds_the_ten_fields():
    r = SweepResult(**{k: i for i, k in enumerate(SweepResult.FIELDS)})
    assert (r.node_max, r.node_min, r.node_mean, r.t_max, r.t_min, r.frame_max, r.frame_min, r.n_max, r.n_min, r.probes) == tuple(range(10))


def test_new_entry_points_are_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "sgvae.h")).read()
    for s in NEW_SYMBOLS:
        assert re.search(rf"\bint {s}\s*\(", hdr), s
        assert s in E.ABI_SYMBOLS
    assert re.search(r"\}\s*sgv_summary_out;", hdr)
    assert [f for f, _ in E.SummaryOut._fields_] == ["node_stats", "node_when", "frame_stats", "frame_where", "probes"]
    assert E.MAX_PROBES == MAX_PROBES == 4096
    lib = E.load_library()
    for s in NEW_SYMBOLS:
        assert hasattr(lib, s), s
    assert len(lib.sgv_set_probes.argtypes) == 3 and len(lib.sgv_summarize.argtypes) == 8 and len(lib.sgv_test_recon_summary.argtypes) == 15
    # without an engine both calls are argument errors that say who complains
    assert lib.sgv_set_probes(None, None, 0) == -1 and "sgv_set_probes" in lib.sgv_last_error().decode()
    assert lib.sgv_summarize(None, None, None, 1, 1, None, None, None) == -1 and "sgv_summarize" in lib.sgv_last_error().decode()
