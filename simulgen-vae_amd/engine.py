"""ctypes binding of libsgvae.so (include/sgvae.h).

PyTorch is used only as plumbing here: device memory for the tensors handed across the C ABI
and the HIP stream the engine enqueues on.  There is no fallback: if the library or a GPU is
missing, construction raises.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Dict, List, Optional

import numpy as np

from .spec import LOSS_IDS, VAEConfig, param_spec

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SGV_LIB") or os.path.join(_HERE, "csrc", "libsgvae.so")
MAX_LEVELS = 8
MAX_SCALARS = 12
DTYPES = {"f32": 0, "fp32": 0, "float32": 0, "bf16": 1, "bfloat16": 1}
LAYOUTS = {"TN": 0, "NT": 1}             # SGV_LAYOUT_*: generate() writes [B, T, N] or [B, N, T]

# every symbol include/sgvae.h declares (tests/test_abi.py checks the library exports them all)
ABI_SYMBOLS = [
    "sgv_last_error", "sgv_create", "sgv_destroy", "sgv_param_count", "sgv_param_info", "sgv_load_state",
    "sgv_export_state", "sgv_export_grad", "sgv_export_adam", "sgv_prepare", "sgv_set_input", "sgv_set_eps",
    "sgv_seed", "sgv_set_shard", "sgv_set_draw_row", "sgv_set_option", "sgv_forward", "sgv_decode", "sgv_generate", "sgv_set_probes", "sgv_summarize", "sgv_score", "sgv_ensemble", "sgv_sobol", "sgv_distribution", "sgv_regress", "sgv_project", "sgv_temporal", "sgv_gram", "sgv_exceedance", "sgv_cycles", "sgv_encode", "sgv_get_xhat", "sgv_get_activation",
    "sgv_backward", "sgv_set_bucket_callback", "sgv_grad_buffer", "sgv_scale_grads", "sgv_grad_norm",
    "sgv_adamw_step", "sgv_augment_collate", "sgv_dataset_convert", "sgv_dataset_sample_bytes",
    "sgv_adamw_step_range", "sgv_bucket_count", "sgv_bucket_dots", "sgv_wire_stream", "sgv_opt_stream", "sgv_adamw_bucket_async", "sgv_set_grad_payload", "sgv_grad_payload_buffer", "sgv_grad_payload_unpack", "sgv_memory_info", "sgv_recompute_bytes", "sgv_last_grad_norm", "sgv_scalars_accumulate", "sgv_scalars_read", "sgv_backward_step",
    "sgv_minmax_fit", "sgv_minmax_coeffs", "sgv_scale_convert",
    "sgv_rccl_unique_id", "sgv_rccl_probe", "sgv_rccl_comm_count", "sgv_rccl_allreduce", "sgv_rccl_comm_init", "sgv_rccl_comm_destroy", "sgv_allreduce_grads", "sgv_set_rccl", "sgv_comm_stream",
    "sgv_augment_stage", "sgv_augment_advance",
    "sgv_load_adam", "sgv_get_train_state", "sgv_set_train_state",
    "sgv_snapshot_floats", "sgv_snapshot_slice", "sgv_snapshot_begin", "sgv_snapshot_wait", "sgv_restore", "sgv_copy_stream",
    "sgv_kernel_time", "sgv_kernel_time_reset", "sgv_kernel_time_tag", "sgv_test_gemm_nt", "sgv_test_gemm_nt_stats", "sgv_test_gemm_nt256", "sgv_test_conv_gn_fwd", "sgv_test_conv_gn_bwd", "sgv_test_gemm_tn", "sgv_test_stream_overlap", "sgv_test_occupy", "sgv_test_fake_collective",
    "sgv_test_gn_workspace_floats", "sgv_test_gn_fwd", "sgv_test_gn_bwd", "sgv_test_recon_loss", "sgv_test_recon_physical", "sgv_test_recon_summary", "sgv_test_recon_score", "sgv_test_recon_ensemble", "sgv_test_recon_sobol", "sgv_test_recon_distribution", "sgv_test_recon_regress", "sgv_test_recon_project", "sgv_test_recon_temporal", "sgv_test_recon_gram", "sgv_test_recon_exceedance", "sgv_test_recon_cycles", "sgv_test_act", "sgv_test_latent", "sgv_test_stage", "sgv_test_linear_head", "sgv_test_linear_expand",
    "sgv_test_optset_create", "sgv_test_optset_destroy", "sgv_test_optset_power_iteration", "sgv_test_optset_grad_dot", "sgv_test_optset_grad_norm",
    "sgv_test_optset_adamw", "sgv_test_optset_make_copies",
]


class SgvConfig(C.Structure):
    _fields_ = [("latent_dim", C.c_int32), ("hierarchical_dim", C.c_int32), ("n_levels", C.c_int32),
                ("num_filter_enc", C.c_int32 * MAX_LEVELS), ("num_node", C.c_int32), ("num_time", C.c_int32),
                ("max_batch", C.c_int32), ("loss_type", C.c_int32), ("small", C.c_int32),
                ("compute_dtype", C.c_int32), ("flags", C.c_int32)]


class OptsetEntry(C.Structure):
    """sgv_optset_entry (include/sgvae.h): one tensor of the optimizer test hook, device pointers"""
    _fields_ = [("p", C.c_void_p), ("g", C.c_void_p), ("m", C.c_void_p), ("v", C.c_void_p), ("n", C.c_long),
                ("taps", C.c_int32), ("rows", C.c_int32), ("cols", C.c_int32),
                ("u", C.c_void_p), ("v_sn", C.c_void_p), ("sigma", C.c_void_p), ("dot", C.c_void_p),
                ("wc", C.c_void_p), ("wct", C.c_void_p), ("g_bf16", C.c_void_p), ("tiled", C.c_int32), ("active", C.c_int32)]


class SummaryOut(C.Structure):
    """sgv_summary_out (include/sgvae.h): the five optional outputs of sgv_summarize, device pointers"""
    _fields_ = [("node_stats", C.c_void_p), ("node_when", C.c_void_p), ("frame_stats", C.c_void_p), ("frame_where", C.c_void_p),
                ("probes", C.c_void_p)]


class ScoreOut(C.Structure):
    """sgv_score_out (include/sgvae.h): the four optional outputs of sgv_score, device pointers"""
    _fields_ = [("node_err", C.c_void_p), ("node_when", C.c_void_p), ("frame_err", C.c_void_p), ("frame_where", C.c_void_p)]


class EnsembleState(C.Structure):
    """sgv_ensemble_state (include/sgvae.h): the running state of sgv_ensemble, device pointers; a group is given whole or not at all"""
    _fields_ = [("mean", C.c_void_p), ("m2", C.c_void_p), ("max", C.c_void_p), ("min", C.c_void_p), ("arg_max", C.c_void_p),
                ("arg_min", C.c_void_p), ("limit", C.c_void_p), ("exceed", C.c_void_p)]


class SobolState(C.Structure):
    """sgv_sobol_state (include/sgvae.h): the running sums of sgv_sobol, device pointers; mean and m2 always, first_sq and / or total_sq"""
    _fields_ = [("mean", C.c_void_p), ("m2", C.c_void_p), ("first_sq", C.c_void_p), ("total_sq", C.c_void_p)]


class DistributionState(C.Structure):
    """sgv_distribution_state (include/sgvae.h): the bounds and the counts of sgv_distribution, device pointers, and the number of bins"""
    _fields_ = [("lo", C.c_void_p), ("hi", C.c_void_p), ("counts", C.c_void_p), ("bins", C.c_int)]


class RegressState(C.Structure):
    """sgv_regress_state (include/sgvae.h): the running state of sgv_regress, device pointers"""
    _fields_ = [("mean", C.c_void_p), ("m2", C.c_void_p), ("comoment", C.c_void_p)]


class CyclesOut(C.Structure):
    """sgv_cycles_out (include/sgvae.h): the outputs of sgv_cycles, device pointers; a group (reversals + ranges, rate_when + rates) whole or not at all"""
    _fields_ = [("reversals", C.c_void_p), ("ranges", C.c_void_p), ("rate_when", C.c_void_p), ("rates", C.c_void_p)]


MAX_PROBES = 4096
SUMMARY_PARTS = ("node", "frame", "probes")      # `want` of Engine.summarize
SCORE_PARTS = ("node", "frame")                  # `want` of Engine.score
ENSEMBLE_GROUPS = {"moments": ("mean", "m2"), "extrema": ("max", "min", "arg_max", "arg_min"), "exceed": ("limit", "exceed")}      # the state of Engine.ensemble
ENSEMBLE_MAX_COUNT = 1 << 24                     # members of one ensemble: beyond that float(k) is not exact
SOBOL_FIELDS = ("mean", "m2", "first_sq", "total_sq")      # the state of Engine.sobol: mean, m2 [T, N]; first_sq, total_sq [n_params, T, N]
SOBOL_MAX_PARAMS = 30                            # a block of n_params + 2 members fits the kernel's member table of 32
SOBOL_MAX_BLOCKS = 1 << 23                       # base samples of one study: 2 per block enter the moments, and float(k) is exact to 2^24
DISTRIBUTION_FIELDS = ("lo", "hi", "counts")      # the state of Engine.distribution: lo, hi [T, N] fp32 (inputs); counts [bins + 2, T, N] int32
DISTRIBUTION_MIN_BINS = 2
DISTRIBUTION_MAX_BINS = 64                       # the kernel's byte histogram of a block, (bins + 2) * 2 KiB, fits the LDS of a CU
REGRESS_FIELDS = ("mean", "m2", "comoment")       # the state of Engine.regress: mean, m2 [T, N]; comoment [n_cov, T, N], all fp32
REGRESS_MAX_COVARIATES = 32                      # the weights of a launch fit the kernel's LDS table
MAX_FUNCTIONALS = 32                             # SGV_MAX_FUNCTIONALS: the weight rows of Engine.project are the 32 columns of the kernel's MFMA tile
MAX_TEMPORAL = 32                                # SGV_MAX_TEMPORAL: the weight rows of Engine.temporal are the 32 rows of the kernel's MFMA tile
MAX_GRAM_T = 256                                 # SGV_MAX_GRAM_T: the time steps of Engine.gram are at most 8 row tiles of the kernel's accumulators
MAX_LEVELS = 4                                   # SGV_MAX_EXCEED_LEVELS: the levels of Engine.exceedance are what the kernel's per-thread state holds in registers
EXCEEDANCE_MAX_T = 65535                         # the kernel packs its step counters into 16-bit halves
EXCEEDANCE_SIDES = {"above": 0, "below": 1}      # SGV_SIDE_*
EXCEEDANCE_STATS = ("count", "first", "last", "longest", "runs")      # the planes of Engine.exceedance's stats, in this order
MAX_CYCLES_EXPONENT = 8                          # SGV_MAX_CYCLES_EXPONENT: the exponent m of the damage sum of Engine.cycles, an integer in [1, 8]
CYCLES_MAX_T = 65535                             # the kernel packs its counters and steps into 16-bit halves
CYCLES_RANGES = ("range_sum", "range_max", "damage", "open")      # the planes of Engine.cycles' ranges, in this order
CYCLES_RATES = ("rise", "fall", "path")          # the planes of Engine.cycles' rates; rate_when holds the steps of rise and fall
SNAPSHOT_PARTS = ("value", "exp_avg", "exp_avg_sq")     # `which` of sgv_snapshot_slice
BUCKET_CB = C.CFUNCTYPE(None, C.c_void_p, C.c_int, C.c_size_t, C.c_size_t)
_lib = None


class SgvError(RuntimeError):
    pass


def load_library(path: str = LIB_PATH):
    """dlopen libsgvae.so and declare the signatures.  Raises if the library has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(path):
        raise SgvError(f"{path} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                       f"(or `make -C simulgen-vae_amd/csrc`). There is no CPU fallback.")
    lib = C.CDLL(path)
    vp, i32, f32 = C.c_void_p, C.c_int, C.c_float
    lib.sgv_last_error.restype = C.c_char_p
    lib.sgv_create.argtypes = [C.POINTER(SgvConfig), vp, C.POINTER(vp)]
    lib.sgv_destroy.argtypes = [vp]
    lib.sgv_param_count.argtypes = [vp]
    lib.sgv_param_info.argtypes = [vp, i32, C.POINTER(C.c_char_p), C.POINTER(i32), C.POINTER(C.c_int64),
                                   C.POINTER(i32), C.POINTER(i32)]
    lib.sgv_load_state.argtypes = [vp, C.c_char_p, vp, C.c_size_t]
    lib.sgv_export_state.argtypes = [vp, C.c_char_p, vp, C.c_size_t]
    lib.sgv_export_grad.argtypes = [vp, C.c_char_p, vp, C.c_size_t, C.POINTER(i32)]
    lib.sgv_export_adam.argtypes = [vp, C.c_char_p, vp, vp, C.c_size_t]
    lib.sgv_load_adam.argtypes = [vp, C.c_char_p, vp, vp, C.c_size_t]
    lib.sgv_get_train_state.argtypes = [vp, C.POINTER(C.c_uint64)]
    lib.sgv_set_train_state.argtypes = [vp, C.POINTER(C.c_uint64)]
    lib.sgv_snapshot_floats.argtypes = [vp, C.POINTER(C.c_size_t)]
    lib.sgv_snapshot_slice.argtypes = [vp, i32, i32, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
    lib.sgv_snapshot_begin.argtypes = [vp, vp, C.c_size_t]
    lib.sgv_snapshot_wait.argtypes = [vp]
    lib.sgv_restore.argtypes = [vp, vp, C.c_size_t]
    lib.sgv_prepare.argtypes = [vp]
    lib.sgv_set_input.argtypes = [vp, vp, i32]
    lib.sgv_set_eps.argtypes = [vp, i32, vp, i32]
    lib.sgv_seed.argtypes = [vp, C.c_uint64]
    lib.sgv_set_shard.argtypes = [vp, i32, i32]
    lib.sgv_set_draw_row.argtypes = [vp, C.c_long]
    lib.sgv_set_option.argtypes = [vp, C.c_char_p, i32]
    lib.sgv_forward.argtypes = [vp, i32, i32, vp]
    lib.sgv_encode.argtypes = [vp, vp, vp, vp]
    lib.sgv_decode.argtypes = [vp, vp, vp, i32, i32, vp]
    lib.sgv_generate.argtypes = [vp, vp, vp, i32, i32, vp, vp, i32, vp]
    lib.sgv_set_probes.argtypes = [vp, vp, i32]
    lib.sgv_summarize.argtypes = [vp, vp, vp, i32, i32, vp, vp, C.POINTER(SummaryOut)]
    lib.sgv_score.argtypes = [vp, vp, vp, i32, i32, vp, vp, vp, C.POINTER(ScoreOut)]
    lib.sgv_ensemble.argtypes = [vp, vp, vp, i32, i32, vp, vp, C.c_long, C.POINTER(EnsembleState)]
    lib.sgv_sobol.argtypes = [vp, vp, vp, i32, i32, vp, vp, i32, C.c_long, C.POINTER(SobolState)]
    lib.sgv_distribution.argtypes = [vp, vp, vp, i32, i32, vp, vp, C.c_long, C.POINTER(DistributionState)]
    lib.sgv_regress.argtypes = [vp, vp, vp, i32, i32, vp, vp, i32, vp, C.c_long, C.POINTER(RegressState)]
    lib.sgv_project.argtypes = [vp, vp, vp, i32, i32, vp, vp, vp, i32, vp]
    lib.sgv_temporal.argtypes = [vp, vp, vp, i32, i32, vp, vp, vp, i32, vp]
    lib.sgv_gram.argtypes = [vp, vp, vp, i32, i32, vp, vp, vp, vp, vp]
    lib.sgv_exceedance.argtypes = [vp, vp, vp, i32, i32, vp, vp, vp, i32, i32, vp, vp]
    lib.sgv_cycles.argtypes = [vp, vp, vp, i32, i32, vp, vp, vp, i32, vp]
    lib.sgv_copy_stream.argtypes = [vp, C.POINTER(vp)]
    lib.sgv_get_xhat.argtypes = [vp, vp]
    lib.sgv_get_activation.argtypes = [vp, C.c_char_p, vp, C.c_size_t]
    lib.sgv_backward.argtypes = [vp, f32, f32]
    lib.sgv_set_bucket_callback.argtypes = [vp, BUCKET_CB, vp]
    lib.sgv_grad_buffer.argtypes = [vp, C.POINTER(vp), C.POINTER(C.c_size_t)]
    lib.sgv_scale_grads.argtypes = [vp, f32]
    lib.sgv_grad_norm.argtypes = [vp, C.POINTER(C.c_double)]
    lib.sgv_adamw_step.argtypes = [vp, f32]
    lib.sgv_backward_step.argtypes = [vp, f32, f32, f32]
    lib.sgv_adamw_step_range.argtypes = [vp, f32, i32, i32, i32, i32]
    lib.sgv_bucket_count.argtypes = [vp]
    lib.sgv_bucket_dots.argtypes = [vp, i32, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
    lib.sgv_opt_stream.argtypes = [vp, C.POINTER(vp)]
    lib.sgv_wire_stream.argtypes = [vp, C.POINTER(vp)]
    lib.sgv_comm_stream.argtypes = [vp, C.POINTER(vp)]
    lib.sgv_adamw_bucket_async.argtypes = [vp, f32, i32]
    lib.sgv_set_grad_payload.argtypes = [vp, C.c_int]
    lib.sgv_grad_payload_buffer.argtypes = [vp, C.POINTER(vp), C.POINTER(C.c_size_t)]
    lib.sgv_grad_payload_unpack.argtypes = [vp]
    lib.sgv_rccl_unique_id.argtypes = [vp]
    lib.sgv_rccl_comm_init.argtypes = [C.POINTER(vp), i32, vp, i32]
    lib.sgv_rccl_comm_destroy.argtypes = [vp]
    lib.sgv_rccl_probe.argtypes = []
    lib.sgv_rccl_comm_count.argtypes = [vp, C.POINTER(i32)]
    lib.sgv_rccl_allreduce.argtypes = [vp, vp, C.c_size_t, i32, vp]
    lib.sgv_test_fake_collective.argtypes = [f32, C.POINTER(C.c_long), C.POINTER(C.c_long)]
    lib.sgv_test_stream_overlap.argtypes = [vp, i32, C.POINTER(i32)]
    lib.sgv_allreduce_grads.argtypes = [vp, vp, vp]
    lib.sgv_set_rccl.argtypes = [vp, vp, vp]
    lib.sgv_last_grad_norm.argtypes = [vp, C.POINTER(C.c_double)]
    lib.sgv_memory_info.argtypes = [vp, C.POINTER(C.c_size_t)]
    lib.sgv_recompute_bytes.argtypes = [vp, C.POINTER(C.c_size_t)]
    lib.sgv_scalars_accumulate.argtypes = [vp]
    lib.sgv_scalars_read.argtypes = [vp, C.POINTER(C.c_double), i32]
    lib.sgv_augment_collate.argtypes = [vp, vp, i32, vp, vp, vp, vp, vp]
    lib.sgv_augment_stage.argtypes = [vp, vp, i32, vp, vp, vp, vp, vp]
    lib.sgv_augment_advance.argtypes = [vp]
    lib.sgv_dataset_convert.argtypes = [vp, vp, vp, i32]
    lib.sgv_dataset_sample_bytes.argtypes = [vp]
    lib.sgv_dataset_sample_bytes.restype = C.c_size_t
    lib.sgv_kernel_time.argtypes = [vp, C.c_char_p, C.POINTER(f32), C.POINTER(i32)]
    lib.sgv_kernel_time_reset.argtypes = [vp, i32]
    lib.sgv_minmax_fit.argtypes = [vp, C.c_long, i32, vp, vp, i32, vp]
    lib.sgv_minmax_coeffs.argtypes = [vp, vp, i32, f32, f32, vp, vp, vp]
    lib.sgv_scale_convert.argtypes = [i32, vp, vp, vp, vp, C.c_long, i32, vp]
    lib.sgv_kernel_time_tag.argtypes = [vp, i32, C.c_char_p, C.c_size_t, C.POINTER(f32), C.POINTER(i32)]
    lib.sgv_test_gemm_nt.argtypes = [i32, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, vp]
    lib.sgv_test_gemm_nt_stats.argtypes = [vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, vp, vp]
    lib.sgv_test_gemm_nt256.argtypes = [vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, i32, vp, vp, vp]
    lib.sgv_test_occupy.argtypes = [vp, i32, i32, i32, C.c_longlong]
    lib.sgv_test_gemm_tn.argtypes = [i32, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, vp]
    lib.sgv_test_conv_gn_fwd.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, f32, vp]
    lg, sz = C.c_long, C.c_size_t
    lib.sgv_test_gn_workspace_floats.argtypes = [i32, i32, i32]
    lib.sgv_test_gn_workspace_floats.restype = sz
    lib.sgv_test_gn_fwd.argtypes = [i32, i32, vp, lg, vp, lg, f32, vp, lg, vp, vp, vp, vp, sz, i32, i32, i32, i32, C.POINTER(i32), vp]
    lib.sgv_test_gn_bwd.argtypes = [i32, i32, vp, lg, vp, lg, f32, f32, vp, vp, vp, vp, lg, vp, vp, vp, vp, vp, vp, i32, vp, sz,
                                    i32, i32, i32, i32, C.POINTER(i32), vp]
    lib.sgv_test_recon_loss.argtypes = [i32, i32, i32, vp, lg, vp, lg, vp, lg, vp, vp, vp, vp, vp, vp, f32, vp, lg, vp, vp, vp, sz,
                                        i32, i32, i32, i32, vp]
    lib.sgv_test_recon_physical.argtypes = [i32, vp, lg, vp, vp, vp, vp, vp, i32, vp, i32, i32, i32, vp]
    lib.sgv_test_recon_summary.argtypes = [i32, vp, lg, vp, vp, vp, vp, vp, C.POINTER(SummaryOut), vp, i32, i32, i32, i32, vp]
    lib.sgv_test_recon_score.argtypes = [i32, vp, lg, vp, vp, vp, vp, vp, vp, C.POINTER(ScoreOut), i32, i32, i32, vp]
    lib.sgv_test_recon_ensemble.argtypes = [i32, vp, lg, vp, vp, vp, vp, vp, lg, C.POINTER(EnsembleState), i32, i32, i32, vp]
    lib.sgv_test_recon_sobol.argtypes = [i32, vp, lg, vp, vp, vp, vp, vp, i32, lg, C.POINTER(SobolState), i32, i32, i32, vp]
    lib.sgv_test_recon_distribution.argtypes = [i32, vp, lg, vp, vp, vp, vp, vp, lg, C.POINTER(DistributionState), i32, i32, i32, vp]
    lib.sgv_test_recon_regress.argtypes = [i32, vp, lg, vp, vp, vp, vp, vp, i32, vp, lg, C.POINTER(RegressState), i32, i32, i32, vp]
    lib.sgv_test_recon_project.argtypes = [i32, vp, lg, vp, vp, vp, vp, vp, vp, i32, vp, i32, i32, i32, vp]
    lib.sgv_test_recon_temporal.argtypes = [i32, vp, lg, vp, vp, vp, vp, vp, vp, i32, vp, i32, i32, i32, vp]
    lib.sgv_test_recon_gram.argtypes = [i32, vp, lg, vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, vp]
    lib.sgv_test_recon_exceedance.argtypes = [i32, vp, lg, vp, vp, vp, vp, vp, vp, i32, i32, vp, vp, i32, i32, i32, vp]
    lib.sgv_test_recon_cycles.argtypes = [i32, vp, lg, vp, vp, vp, vp, vp, vp, i32, vp, i32, i32, i32, vp]
    lib.sgv_test_act.argtypes = [i32, i32, vp, lg, vp, lg, f32, vp, lg, vp, vp, vp, vp, lg, vp, sz, i32, i32, i32, vp]
    lib.sgv_test_latent.argtypes = [vp, vp, vp, vp, vp, vp, f32, i32, i32, vp]
    lib.sgv_test_stage.argtypes = [i32, vp, vp, vp, vp, lg, vp, lg, vp, f32, f32, vp, vp, vp, lg, vp, vp, f32, i32, i32, vp]
    lib.sgv_test_linear_head.argtypes = [i32, vp, vp, vp, vp, vp, vp, sz, vp, vp, vp, vp, vp, i32, i32, i32, vp]
    lib.sgv_test_linear_expand.argtypes = [i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, vp]
    lib.sgv_test_conv_gn_bwd.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, vp]
    lib.sgv_test_optset_create.argtypes = [i32, C.POINTER(OptsetEntry), i32, C.POINTER(vp)]
    lib.sgv_test_optset_destroy.argtypes = [vp]
    lib.sgv_test_optset_power_iteration.argtypes = [vp, i32, i32, vp]
    lib.sgv_test_optset_grad_dot.argtypes = [vp, vp]
    lib.sgv_test_optset_grad_norm.argtypes = [vp, C.POINTER(C.c_double), vp]
    lib.sgv_test_optset_adamw.argtypes = [vp, f32, f32, i32, vp, i32, vp, vp, sz, C.POINTER(C.c_double), vp]
    lib.sgv_test_optset_make_copies.argtypes = [vp, vp]
    _lib = lib
    return lib


def is_tensor_of(v, dtype, shape=None, device="cuda"):
    """whether v is a contiguous tensor of `dtype` on `device` and, unless None, of `shape`: the form in which a tensor crosses the C ABI"""
    import torch
    return (torch.is_tensor(v) and v.device.type == device and v.dtype == dtype and v.is_contiguous()
            and (shape is None or tuple(v.shape) == tuple(shape)))


def _out_tensor(out, shape, dtype, what="out must be a contiguous float32 CUDA tensor", new=None):
    """an output of a surrogate pass: a new CUDA tensor when `out` is `new`, else `out`, checked (ValueError: `what` of shape ...)"""
    import torch
    if out is new:
        return torch.empty(shape, dtype=dtype, device="cuda")
    if not is_tensor_of(out, dtype, shape):
        raise ValueError(f"{what} of shape {shape}")
    return out


def _member_range(count_before, B) -> int:
    """count_before as an int, the members count_before .. count_before + B - 1 of a study checked against ENSEMBLE_MAX_COUNT"""
    cb = int(count_before)
    if cb < 0 or cb + B > ENSEMBLE_MAX_COUNT:
        raise ValueError(f"count_before = {cb} with a batch of {B} is outside [0, {ENSEMBLE_MAX_COUNT}]")
    return cb


def _weight_rows(w, cols, limit, name="weights", rows="R") -> int:
    """the number of rows of w, a contiguous fp32 CUDA tensor [rows, cols] with 1 <= rows <= limit"""
    import torch
    R = int(w.shape[0]) if torch.is_tensor(w) and w.dim() == 2 else 0
    if R < 1 or R > limit or not is_tensor_of(w, torch.float32, (R, cols)):
        raise ValueError(f"{name} must be a contiguous float32 CUDA tensor of shape [{rows}, {cols}] with 1 <= {rows} <= {limit}")
    return R


def _ptr(a):
    """the device pointer of a tensor as a ctypes argument, None (NULL) for None"""
    return C.c_void_p(a.data_ptr()) if a is not None else None


def _check(lib, rc: int, what: str):
    if rc != 0:
        raise SgvError(f"{what} failed ({rc}): {lib.sgv_last_error().decode()}")


class Engine:
    """One VAE engine on the current CUDA(HIP) device and torch stream."""

    def __init__(self, cfg: VAEConfig, max_batch: int, compute_dtype: str = "bf16", flags: int = 0):
        import torch
        if not torch.cuda.is_available():
            raise SgvError("no MI355X visible (torch.cuda.is_available() is False): libsgvae has no CPU fallback")
        if list(cfg.num_filter_dec) != list(cfg.num_filter_enc)[::-1]:
            raise SgvError("num_filter_dec must be num_filter_enc reversed (reference SimulGen-VAE.py:219)")
        self.torch = torch
        self.lib = load_library()
        self.cfg = cfg
        self.max_batch = int(max_batch)
        self.compute_dtype = compute_dtype
        c = SgvConfig()
        c.latent_dim, c.hierarchical_dim = cfg.latent_dim, cfg.hierarchical_dim
        c.n_levels = len(cfg.num_filter_enc)
        for i, v in enumerate(cfg.num_filter_enc):
            c.num_filter_enc[i] = v
        c.num_node, c.num_time, c.max_batch = cfg.num_node, cfg.num_time, self.max_batch
        c.loss_type = LOSS_IDS[cfg.lossfun]
        c.small = 1 if cfg.small else 0
        c.compute_dtype = DTYPES[compute_dtype]
        c.flags = flags
        self.stream = torch.cuda.current_stream().cuda_stream
        h = C.c_void_p()
        _check(self.lib, self.lib.sgv_create(C.byref(c), C.c_void_p(self.stream), C.byref(h)), "sgv_create")
        self.h = h
        self.spec = param_spec(cfg)
        self.n_kl = len(cfg.num_filter_enc) - 1
        self.batch = 0
        self._cb = None
        self.n_probes = 0

    def close(self):
        if getattr(self, "h", None):
            self.lib.sgv_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- state ----
    def param_info(self):
        out = []
        n = self.lib.sgv_param_count(self.h)
        for i in range(n):
            name, nd, kind, hg = C.c_char_p(), C.c_int(), C.c_int(), C.c_int()
            shape = (C.c_int64 * 4)()
            _check(self.lib, self.lib.sgv_param_info(self.h, i, C.byref(name), C.byref(nd), shape, C.byref(kind),
                                                     C.byref(hg)), "sgv_param_info")
            out.append((name.value.decode(), tuple(shape[j] for j in range(nd.value)), kind.value, bool(hg.value)))
        return out

    def load_state(self, state: Dict[str, np.ndarray], partial: bool = False):
        """nn.Module.load_state_dict: every key of the reference state_dict (partial=True: only the keys given,
        e.g. to restore the spectral-norm u/v vectors)."""
        for e in self.spec:
            if partial and e.name not in state:
                continue
            a = np.ascontiguousarray(state[e.name], dtype=np.float32)
            if a.shape != tuple(e.shape):
                raise SgvError(f"shape mismatch for {e.name}: {a.shape} vs {e.shape}")
            _check(self.lib, self.lib.sgv_load_state(self.h, e.name.encode(), a.ctypes.data_as(C.c_void_p), a.size),
                   f"sgv_load_state({e.name})")
        _check(self.lib, self.lib.sgv_prepare(self.h), "sgv_prepare")

    def state_dict(self) -> Dict[str, np.ndarray]:
        out = {}
        for e in self.spec:
            a = np.empty(e.shape, dtype=np.float32)
            _check(self.lib, self.lib.sgv_export_state(self.h, e.name.encode(), a.ctypes.data_as(C.c_void_p), a.size),
                   f"sgv_export_state({e.name})")
            out[e.name] = a
        return out

    def grad(self, name: str) -> Optional[np.ndarray]:
        e = next(x for x in self.spec if x.name == name)
        a = np.empty(e.shape, dtype=np.float32)
        none = C.c_int()
        _check(self.lib, self.lib.sgv_export_grad(self.h, name.encode(), a.ctypes.data_as(C.c_void_p), a.size,
                                                  C.byref(none)), f"sgv_export_grad({name})")
        return None if none.value else a

    def adam_state(self, name: str):
        e = next(x for x in self.spec if x.name == name)
        m = np.empty(e.shape, dtype=np.float32)
        v = np.empty(e.shape, dtype=np.float32)
        _check(self.lib, self.lib.sgv_export_adam(self.h, name.encode(), m.ctypes.data_as(C.c_void_p),
                                                  v.ctypes.data_as(C.c_void_p), m.size), "sgv_export_adam")
        return m, v

    def load_adam(self, name: str, exp_avg=None, exp_avg_sq=None):
        """torch.optim.AdamW state of one parameter back into the engine (reference layout; None leaves a moment alone)."""
        e = next((x for x in self.spec if x.name == name), None)
        arrs = []
        for a in (exp_avg, exp_avg_sq):
            if a is not None:
                a = np.ascontiguousarray(a, dtype=np.float32)
                if e is not None and a.shape != tuple(e.shape):
                    a = a.reshape(-1)            # the library reports the size mismatch
            arrs.append(a)
        n = next((a.size for a in arrs if a is not None), 0)
        if all(a is not None for a in arrs) and arrs[0].size != arrs[1].size:
            raise ValueError(f"load_adam({name}): exp_avg has {arrs[0].size} elements, exp_avg_sq {arrs[1].size}")
        ptr = [a.ctypes.data_as(C.c_void_p) if a is not None else None for a in arrs]
        _check(self.lib, self.lib.sgv_load_adam(self.h, name.encode(), ptr[0], ptr[1], n), f"sgv_load_adam({name})")

    def train_state(self):
        """dict(step, seed, draw): AdamW steps taken, the noise seed and the noise draws consumed (include/sgvae.h)."""
        st = (C.c_uint64 * 4)()
        _check(self.lib, self.lib.sgv_get_train_state(self.h, st), "sgv_get_train_state")
        return dict(step=int(st[0]), seed=int(st[1]), draw=int(st[2]))

    def set_train_state(self, step: int, seed: int, draw: int):
        """Put the three values of train_state() back; unlike seed() the draw position is kept."""
        st = (C.c_uint64 * 4)(int(step), int(seed), int(draw), 0)
        _check(self.lib, self.lib.sgv_set_train_state(self.h, st), "sgv_set_train_state")

    def snapshot_layout(self):
        """(total floats, [(key, which, offset, count)]) of the flat snapshot buffer: which = "value", "exp_avg" or "exp_avg_sq";
        entries without optimizer state have a "value" row only."""
        total = C.c_size_t()
        _check(self.lib, self.lib.sgv_snapshot_floats(self.h, C.byref(total)), "sgv_snapshot_floats")
        rows = []
        for i, (name, _shape, _kind, _hg) in enumerate(self.param_info()):
            for w, label in enumerate(SNAPSHOT_PARTS):
                off, cnt = C.c_size_t(), C.c_size_t()
                _check(self.lib, self.lib.sgv_snapshot_slice(self.h, i, w, C.byref(off), C.byref(cnt)), "sgv_snapshot_slice")
                if cnt.value:
                    rows.append((name, label, int(off.value), int(cnt.value)))
        return int(total.value), rows

    def snapshot_floats(self) -> int:
        total = C.c_size_t()
        _check(self.lib, self.lib.sgv_snapshot_floats(self.h, C.byref(total)), "sgv_snapshot_floats")
        return int(total.value)

    def _snapshot_buffer(self, buf, what, pinned):
        t = self.torch
        n = self.snapshot_floats()
        if not is_tensor_of(buf, t.float32, device="cpu"):
            raise ValueError(f"{what}: the buffer must be a contiguous torch.float32 CPU tensor")
        if buf.numel() != n:
            raise ValueError(f"{what}: the buffer holds {buf.numel()} floats, the engine's state has {n}")
        if pinned and not buf.is_pinned():
            raise ValueError(f"{what}: the buffer must be pinned (torch.empty(n, dtype=torch.float32, pin_memory=True))")
        return n

    def snapshot_begin(self, buf):
        """Enqueue a snapshot of the whole state (parameters, u / v, both Adam moments) into the pinned float32 CPU tensor `buf`
        (snapshot_floats() elements) and return at once; the next step may be enqueued right away.  Read `buf` only after
        snapshot_wait()."""
        n = self._snapshot_buffer(buf, "snapshot_begin", True)
        _check(self.lib, self.lib.sgv_snapshot_begin(self.h, C.c_void_p(buf.data_ptr()), n), "sgv_snapshot_begin")
        self._snap_buf = buf                       # the copy writes into it until snapshot_wait()

    def snapshot_wait(self):
        _check(self.lib, self.lib.sgv_snapshot_wait(self.h), "sgv_snapshot_wait")
        self._snap_buf = None

    def restore(self, buf):
        """The inverse of a snapshot: `buf` (float32 CPU tensor, pinned or not) replaces parameters, u / v and both moments."""
        n = self._snapshot_buffer(buf, "restore", False)
        _check(self.lib, self.lib.sgv_restore(self.h, C.c_void_p(buf.data_ptr()), n), "sgv_restore")

    # ---- step ----
    def set_option(self, key: str, value: int):
        _check(self.lib, self.lib.sgv_set_option(self.h, key.encode(), int(value)), "sgv_set_option")

    def seed(self, seed: int):
        _check(self.lib, self.lib.sgv_seed(self.h, C.c_uint64(seed)), "sgv_seed")

    def set_shard(self, rank: int, world: int):
        """Sample b of this engine's batch is sample b * world + rank of the global batch: the engine's noise draws are keyed by
        that global row (include/sgvae.h: sgv_set_shard), so the same seed on every rank gives world-size-invariant noise."""
        _check(self.lib, self.lib.sgv_set_shard(self.h, int(rank), int(world)), "sgv_set_shard")

    def set_draw_row(self, first_row: int):
        """Sample b of the following passes that draw their noise per call (generate, summarize, score, project, temporal, gram, exceedance, cycles) takes
        row first_row + b of the streams the call draws from (include/sgvae.h: sgv_set_draw_row).  With the draw position put back in
        front of every batch (set_train_state) a study cut into batches gets the noise one call over all of it would get.  Default 0."""
        _check(self.lib, self.lib.sgv_set_draw_row(self.h, int(first_row)), "sgv_set_draw_row")

    def set_input(self, x):
        """x: torch float32 CUDA tensor [B, num_node, num_time] (reference layout)."""
        t = self.torch
        assert x.is_cuda and x.dtype == t.float32 and x.is_contiguous()
        B = x.shape[0]
        assert tuple(x.shape[1:]) == (self.cfg.num_node, self.cfg.num_time), x.shape
        _check(self.lib, self.lib.sgv_set_input(self.h, C.c_void_p(x.data_ptr()), B), "sgv_set_input")
        self.batch = B

    def set_eps(self, eps_list):
        for site, e in enumerate(eps_list):
            assert e.is_cuda and e.dtype == self.torch.float32 and e.is_contiguous()
            _check(self.lib, self.lib.sgv_set_eps(self.h, site, C.c_void_p(e.data_ptr()), e.shape[0]), "sgv_set_eps")

    def forward(self, train: bool = True, fix: bool = False, sync: bool = True):
        buf = (C.c_float * MAX_SCALARS)()
        _check(self.lib, self.lib.sgv_forward(self.h, int(train), int(fix), buf if sync else None), "sgv_forward")
        if not sync:
            return None
        n = self.n_kl
        return dict(recon=buf[0], kls=[buf[1 + i] for i in range(n)], mse=buf[1 + n])

    def decode(self, z, xs, fix: bool = False):
        """Decoder.forward(z, xs, mode): z torch fp32 CUDA [B,latent]; xs list of [B,hier] in Encoder order."""
        t = self.torch
        B = z.shape[0]
        xs_t = t.stack([x.to(t.float32) for x in xs]).contiguous().cuda()
        z = z.to(t.float32).contiguous().cuda()
        buf = (C.c_float * MAX_SCALARS)()
        _check(self.lib, self.lib.sgv_decode(self.h, C.c_void_p(z.data_ptr()), C.c_void_p(xs_t.data_ptr()), B, int(fix), buf),
               "sgv_decode")
        self.batch = B
        return [buf[2 + i] for i in range(self.n_kl - 1)]

    def generate(self, z, xs, scale, min, out=None, layout="TN", fix=True):
        """Decoder.forward(z, xs, mode) delivered as a physical-unit field: (x_hat - min) / scale per node (MinMaxScaler.inverse_transform
        of data_scaler), fp32, written by the recon head's output pass straight into `out` -- [B, T, N] for layout "TN", [B, N, T] for
        "NT"; allocated when None.  z [B, latent], xs a list of [B, hier] in Encoder order (or one [n_levels - 1, B, hier] tensor),
        scale / min fp32 CUDA [num_node].  Nothing synchronises; afterwards there is no forward pass to read (xhat() raises)."""
        t = self.torch
        if layout not in LAYOUTS:
            raise ValueError(f"layout must be one of {sorted(LAYOUTS)}, not {layout!r}")
        N, T = self.cfg.num_node, self.cfg.num_time

        def tail(B):
            res = _out_tensor(out, (B, T, N) if layout == "TN" else (B, N, T), t.float32)
            return (LAYOUTS[layout], _ptr(res)), res
        return self._surrogate("sgv_generate", z, xs, scale, min, fix, tail)

    def _latents(self, z, xs):
        """the checks generate and summarize share: z [B, latent] and xs as fp32 CUDA tensors"""
        t = self.torch
        B = z.shape[0]
        z = z.to(device="cuda", dtype=t.float32).contiguous()
        xs_t = (xs if t.is_tensor(xs) else t.stack([x.to(device="cuda", dtype=t.float32) for x in xs])).to(device="cuda", dtype=t.float32).contiguous()
        if tuple(xs_t.shape) != (self.n_kl, B, self.cfg.hierarchical_dim):
            raise ValueError(f"xs of shape {tuple(xs_t.shape)}, expected {(self.n_kl, B, self.cfg.hierarchical_dim)}")
        return B, z, xs_t

    def _scaler(self, scale, min):
        t, N = self.torch, self.cfg.num_node
        for name, v in (("scale", scale), ("min", min)):
            if not (is_tensor_of(v, t.float32) and v.numel() == N):
                raise ValueError(f"{name} must be a contiguous float32 CUDA tensor of {N} elements")

    def _surrogate(self, entry, z, xs, scale, min, fix, tail):
        """the call the surrogate passes share: the checks on z, xs, scale and min, then tail(B) -> (the entry
        point's trailing arguments, what to return), which checks whatever depends on the batch, then the C call"""
        B, z, xs_t = self._latents(z, xs)
        self._scaler(scale, min)
        args, res = tail(B)
        _check(self.lib, getattr(self.lib, entry)(self.h, C.c_void_p(z.data_ptr()), C.c_void_p(xs_t.data_ptr()), B, int(fix),
                                                  C.c_void_p(scale.data_ptr()), C.c_void_p(min.data_ptr()), *args), entry)
        self.batch = B
        return res

    def _named_outputs(self, shapes, out):
        """name -> CUDA tensor for every name -> (shape, dtype) of `shapes`: out[name] where the caller gave one (checked), else a new one"""
        t = self.torch
        res = {}
        for name, (shape, dt) in shapes.items():
            res[name] = _out_tensor(None if out is None else out.get(name), shape, dt, f"out[{name!r}] must be a contiguous {dt} CUDA tensor")
        return res

    def _state(self, state, spec, what, needs):
        """the names, in the order of spec = {name: (shape, dtype)}, of the tensors the running state `state` of ensemble or sobol
        holds: a non-empty dict (ValueError(needs) otherwise) of names of `spec` with tensors as `spec` has them, or None"""
        if not isinstance(state, dict) or not state:
            raise ValueError(needs)
        for k in state:
            if k not in spec:
                raise ValueError(f"state[{k!r}] is not a tensor of the {what}")
        have = [k for k in spec if state.get(k) is not None]
        for k in have:
            shape, dt = spec[k]
            if not is_tensor_of(state[k], dt, shape):
                raise ValueError(f"state[{k!r}] must be a contiguous {dt} CUDA tensor of shape {shape}")
        return have

    def set_probes(self, nodes):
        """The probe nodes of summarize(): a 1-D integer sequence of at most MAX_PROBES node indices in [0, num_node); an empty
        one clears the list.  Duplicates are allowed and the order is kept (include/sgvae.h: sgv_set_probes)."""
        a = np.asarray(nodes)
        if a.size and not np.issubdtype(a.dtype, np.integer):
            raise ValueError(f"probe nodes must be integers, not {a.dtype}")
        if a.ndim != 1:
            raise ValueError(f"probe nodes must be 1-D, got shape {a.shape}")
        if a.size and (a.min() < -2**31 or a.max() >= 2**31):
            raise ValueError("probe nodes do not fit int32")
        a = np.ascontiguousarray(a, dtype=np.int32)
        _check(self.lib, self.lib.sgv_set_probes(self.h, a.ctypes.data_as(C.c_void_p), int(a.size)), "sgv_set_probes")
        self.n_probes = int(a.size)

    def summarize(self, z, xs, scale, min, fix=True, want=SUMMARY_PARTS, out=None):
        """Summaries of the field generate() would write, computed by the recon head's last pass itself; the field is never stored.
        Same inputs and checks as generate().  want: any of "node", "frame", "probes".  Returns a dict of CUDA tensors:
        node_stats fp32 [B, 3, N] (max, min, mean over t) and node_when int32 [B, 2, N] (t of max, of min);
        frame_stats fp32 [B, T, 2] (max, min over the nodes) and frame_where int32 [B, T, 2] (their node);
        probes fp32 [B, T, K] at the nodes of set_probes().  Ties go to the smallest index.  out: a dict of such tensors to
        write into (those present are reused).  Nothing synchronises; afterwards xhat() raises, as after generate()."""
        t = self.torch
        want = tuple(want)
        if not want or any(w not in SUMMARY_PARTS for w in want):
            raise ValueError(f"want must name at least one of {SUMMARY_PARTS}, not {want!r}")
        if "probes" in want and self.n_probes < 1:
            raise ValueError("want includes 'probes', but no probe nodes are set (set_probes)")
        N, T = self.cfg.num_node, self.cfg.num_time

        def tail(B):
            shapes = {}
            if "node" in want:
                shapes.update(node_stats=((B, 3, N), t.float32), node_when=((B, 2, N), t.int32))
            if "frame" in want:
                shapes.update(frame_stats=((B, T, 2), t.float32), frame_where=((B, T, 2), t.int32))
            if "probes" in want:
                shapes.update(probes=((B, T, self.n_probes), t.float32))
            res = self._named_outputs(shapes, out)
            return (C.byref(SummaryOut(**{name: v.data_ptr() for name, v in res.items()})),), res
        return self._surrogate("sgv_summarize", z, xs, scale, min, fix, tail)

    def score(self, z, xs, scale, min, truth, fix=True, want=SCORE_PARTS, out=None):
        """The error of the field generate() would write against `truth` (contiguous fp32 CUDA [B, T, N], physical units), reduced by
        the recon head's last pass itself: e = field - truth, one fp32 subtraction; neither is stored.  Same inputs and checks as
        summarize().  want: any of "node", "frame".  Returns a dict of CUDA tensors:
        node_err fp32 [B, 3, N] (max_t |e|, mean_t e, mean_t e^2) and node_when int32 [B, N] (t of the largest |e|);
        frame_err fp32 [B, T, 3] (max_n |e|, mean_n e^2, mean_n truth^2) and frame_where int32 [B, T] (its node).  Ties go to the
        smallest index.  truth must be finite (not checked).  out: a dict of such tensors to write into (those present are reused).
        Nothing synchronises; afterwards xhat() raises, as after generate()."""
        t = self.torch
        want = tuple(want)
        if not want or any(w not in SCORE_PARTS for w in want):
            raise ValueError(f"want must name at least one of {SCORE_PARTS}, not {want!r}")
        N, T = self.cfg.num_node, self.cfg.num_time

        def tail(B):
            if not is_tensor_of(truth, t.float32, (B, T, N)):
                raise ValueError(f"truth must be a contiguous float32 CUDA tensor of shape {(B, T, N)}")
            shapes = {}
            if "node" in want:
                shapes.update(node_err=((B, 3, N), t.float32), node_when=((B, N), t.int32))
            if "frame" in want:
                shapes.update(frame_err=((B, T, 3), t.float32), frame_where=((B, T), t.int32))
            res = self._named_outputs(shapes, out)
            return (C.c_void_p(truth.data_ptr()), C.byref(ScoreOut(**{name: v.data_ptr() for name, v in res.items()}))), res
        return self._surrogate("sgv_score", z, xs, scale, min, fix, tail)

    def ensemble(self, z, xs, scale, min, state, count_before, fix=True):
        """Merges the fields generate() would write for this batch into the running statistics `state`, per (time step, node), by
        the recon head's last pass itself; the fields are never stored.  Same inputs and checks as summarize().  state: a dict of
        contiguous CUDA tensors [T, N], whole groups only (ENSEMBLE_GROUPS): "mean", "m2" fp32 (Welford: variance = m2 / count);
        "max", "min" fp32 with "arg_max", "arg_min" int32 (the index of the member that produced the extremum, the earliest on a
        tie); "limit" fp32 [N] (input) with "exceed" int32 (members with field > limit, strict).  Sample b of the batch is member
        count_before + b; with count_before == 0 the state is not read.  The tensors are updated in place and `state` is returned.
        Any cut of the same members into calls gives the same bits, the decoder's noise included: unless set with set_eps() it
        follows the member's index (the rows count_before + b of the streams the first call after seed() draws from) and the
        draw position does not move.  Nothing synchronises; afterwards xhat() raises, as after generate()."""
        t = self.torch
        N, T = self.cfg.num_node, self.cfg.num_time
        spec = {k: ((N,) if k == "limit" else (T, N), t.int32 if k in ("arg_max", "arg_min", "exceed") else t.float32)
                for names in ENSEMBLE_GROUPS.values() for k in names}
        held = self._state(state, spec, f"ensemble state ({sorted(spec)})",
                           f"state must be a dict with the tensors of at least one of the groups {ENSEMBLE_GROUPS}")
        for g, names in ENSEMBLE_GROUPS.items():
            have = [k for k in names if k in held]
            if have and len(have) != len(names):
                raise ValueError(f"state: group {g!r} needs all of {names}, got only {have}")

        def tail(B):
            return (_member_range(count_before, B), C.byref(EnsembleState(**{k: v.data_ptr() for k, v in state.items() if v is not None}))), state
        return self._surrogate("sgv_ensemble", z, xs, scale, min, fix, tail)

    def sobol(self, z, xs, scale, min, state, n_params, blocks_before, fix=True):
        """Merges this batch into the running sums `state` of a Sobol sensitivity study, per (time step, node), by the recon head's
        last pass itself; the fields are never stored.  Same inputs and checks as summarize().  The batch holds whole blocks of
        n_params + 2 members in this order: A_j, B_j, AB_1_j .. AB_d_j (AB_i_j: base sample A_j with the inputs of parameter i
        taken from B_j); block j of the call is base sample blocks_before + j.  state: a dict of contiguous fp32 CUDA tensors,
        "mean" and "m2" [T, N] (Welford over the A and B members: variance = m2 / (2 n)), and "first_sq" and / or "total_sq"
        [n_params, T, N] (sums of (xB - xAB_i)^2 and of (xA - xAB_i)^2: Jansen's estimators).  With blocks_before == 0 the state is
        not read.  The tensors are updated in place and `state` is returned.  Any cut of the same blocks into calls gives the same
        bits, the decoder's noise included: unless set with set_eps() it follows the member's index
        blocks_before * (n_params + 2) + b, as in ensemble(), and the draw position does not move.  Nothing synchronises;
        afterwards xhat() raises, as after generate()."""
        t = self.torch
        N, T = self.cfg.num_node, self.cfg.num_time
        d = int(n_params)
        if d < 1 or d > SOBOL_MAX_PARAMS:
            raise ValueError(f"n_params = {d} is outside [1, {SOBOL_MAX_PARAMS}]")
        spec = {k: ((T, N) if k in ("mean", "m2") else (d, T, N), t.float32) for k in SOBOL_FIELDS}
        have = self._state(state, spec, f"Sobol state ({SOBOL_FIELDS})",
                           "state must be a dict with the tensors 'mean', 'm2' and at least one of 'first_sq', 'total_sq'")
        if "mean" not in have or "m2" not in have or len(have) < 3:
            raise ValueError(f"state needs 'mean', 'm2' and at least one of 'first_sq', 'total_sq', got only {have}")

        def tail(B):
            bb = int(blocks_before)
            if B % (d + 2):
                raise ValueError(f"a batch of {B} members is not whole blocks of n_params + 2 = {d + 2}")
            if bb < 0 or bb + B // (d + 2) > SOBOL_MAX_BLOCKS:
                raise ValueError(f"blocks_before = {bb} with {B // (d + 2)} blocks is outside [0, {SOBOL_MAX_BLOCKS}]")
            return (d, bb, C.byref(SobolState(**{k: state[k].data_ptr() for k in have}))), state
        return self._surrogate("sgv_sobol", z, xs, scale, min, fix, tail)

    def distribution(self, z, xs, scale, min, state, count_before, fix=True):
        """Counts the fields generate() would write for this batch into the histogram `state`, per (time step, node), by the recon
        head's last pass itself; the fields are never stored.  Same inputs and checks as summarize().  state: a dict of contiguous
        CUDA tensors, all three required: "lo", "hi" fp32 [T, N] (inputs: the bounds, hi >= lo, e.g. "min" and "max" of an
        ensemble() over the same members) and "counts" int32 [bins + 2, T, N] with DISTRIBUTION_MIN_BINS <= bins <=
        DISTRIBUTION_MAX_BINS: row 0 the members below lo, rows 1 .. bins the uniform bins between lo and hi (a value equal to hi
        is in the last), row bins + 1 the members above hi (the rule: include/sgvae.h, sgv_distribution).  The pass only adds to
        counts: a new state is torch.zeros, a continuation adds to what is there, and any cut of the same members into calls gives
        the same bits.  Sample b of the batch is member count_before + b: that places it in the noise streams exactly as
        ensemble() does and leaves the draw position alone; it does not decide whether the state is read.  counts is updated in
        place and `state` is returned.  Nothing synchronises; afterwards xhat() raises, as after generate()."""
        t = self.torch
        N, T = self.cfg.num_node, self.cfg.num_time
        needs = "state must be a dict with the tensors 'lo', 'hi' [T, N] and 'counts' [bins + 2, T, N]"
        counts = state.get("counts") if isinstance(state, dict) else None
        rows = int(counts.shape[0]) if t.is_tensor(counts) and counts.dim() == 3 else DISTRIBUTION_MIN_BINS + 2
        bins = rows - 2
        if bins < DISTRIBUTION_MIN_BINS or bins > DISTRIBUTION_MAX_BINS:
            raise ValueError(f"state['counts'] has {rows} rows: bins = rows - 2 = {bins} is outside [{DISTRIBUTION_MIN_BINS}, {DISTRIBUTION_MAX_BINS}]")
        spec = {"lo": ((T, N), t.float32), "hi": ((T, N), t.float32), "counts": ((rows, T, N), t.int32)}
        have = self._state(state, spec, f"distribution state ({DISTRIBUTION_FIELDS})", needs)
        if len(have) != 3:
            raise ValueError(f"state needs all of {DISTRIBUTION_FIELDS}, got only {have}")

        def tail(B):
            cb = _member_range(count_before, B)
            st = DistributionState(lo=state["lo"].data_ptr(), hi=state["hi"].data_ptr(), counts=state["counts"].data_ptr(), bins=bins)
            return (cb, C.byref(st)), state
        return self._surrogate("sgv_distribution", z, xs, scale, min, fix, tail)

    def regress(self, z, xs, scale, min, state, weights, count_before, fix=True):
        """Merges the fields generate() would write for this batch into the running state `state` of a linear response surface on
        the covariates, per (time step, node), by the recon head's last pass itself; the fields are never stored.  Same inputs and
        checks as summarize().  state: a dict of contiguous fp32 CUDA tensors, all three required: "mean", "m2" [T, N] (Welford,
        bit for bit the moments of ensemble()) and "comoment" [n_cov, T, N], 1 <= n_cov <= REGRESS_MAX_COVARIATES: the sum over the
        members of (field - its mean)(covariate i - its mean).  weights: contiguous fp32 CUDA [B, n_cov], the centred covariates of
        this batch's members as predict.regression_weights forms them (y_m - ybar, ybar the running mean including member m).
        Sample b of the batch is member count_before + b; with count_before == 0 the state is not read.  The tensors are updated in
        place and `state` is returned.  Any cut of the same members into calls gives the same bits, the decoder's noise included:
        it follows the member's index as in ensemble() and the draw position does not move.  Nothing synchronises; afterwards xhat()
        raises, as after generate()."""
        t = self.torch
        N, T = self.cfg.num_node, self.cfg.num_time
        needs = "state must be a dict with the tensors 'mean', 'm2' [T, N] and 'comoment' [n_cov, T, N]"
        co = state.get("comoment") if isinstance(state, dict) else None
        K = int(co.shape[0]) if t.is_tensor(co) and co.dim() == 3 else 1
        if K < 1 or K > REGRESS_MAX_COVARIATES:
            raise ValueError(f"state['comoment'] has {K} rows: n_cov is outside [1, {REGRESS_MAX_COVARIATES}]")
        spec = {"mean": ((T, N), t.float32), "m2": ((T, N), t.float32), "comoment": ((K, T, N), t.float32)}
        have = self._state(state, spec, f"regression state ({REGRESS_FIELDS})", needs)
        if len(have) != 3:
            raise ValueError(f"state needs all of {REGRESS_FIELDS}, got only {have}")

        def tail(B):
            cb = int(count_before)
            if not is_tensor_of(weights, t.float32, (B, K)):
                raise ValueError(f"weights must be a contiguous float32 CUDA tensor of shape {(B, K)}")
            _member_range(cb, B)
            st = RegressState(mean=state["mean"].data_ptr(), m2=state["m2"].data_ptr(), comoment=state["comoment"].data_ptr())
            return (K, C.c_void_p(weights.data_ptr()), cb, C.byref(st)), state
        return self._surrogate("sgv_regress", z, xs, scale, min, fix, tail)

    def project(self, z, xs, scale, min, weights, fix=True, out=None):
        """Linear functionals of the field generate() would write, by the recon head's last pass itself; the field is never stored.
        Same inputs and checks as summarize().  weights: contiguous fp32 CUDA [R, N], 1 <= R <= MAX_FUNCTIONALS (predict.functional_weights
        validates and uploads a host array).  Returns fp32 CUDA [B, T, R], values[b, t, r] = sum over n of weights[r, n] * field[b, t, n]:
        fp32 fused multiply-adds in a fixed order inside fixed shares of the mesh, the shares added in float64 and rounded once.  A
        value depends on its sample, its row and its weight row alone, so any cut of the conditions into batches gives the same
        bits.  out: a contiguous fp32 CUDA tensor [B, T, R] to write into (a slice along the first axis of a larger one will do).
        Nothing synchronises; afterwards xhat() raises, as after generate()."""
        t = self.torch
        N, T = self.cfg.num_node, self.cfg.num_time
        R = _weight_rows(weights, N, MAX_FUNCTIONALS)

        def tail(B):
            res = _out_tensor(out, (B, T, R), t.float32)
            return (_ptr(weights), R, _ptr(res)), res
        return self._surrogate("sgv_project", z, xs, scale, min, fix, tail)

    def temporal(self, z, xs, scale, min, weights, fix=True, out=None):
        """Linear functionals over time of the field generate() would write, by the recon head's last pass itself; the field is never
        stored.  Same inputs and checks as summarize().  weights: contiguous fp32 CUDA [R, T], 1 <= R <= MAX_TEMPORAL
        (predict.temporal_weights validates and uploads a host array).  Returns fp32 CUDA [B, R, N], values[b, r, n] = sum over t of
        weights[r, t] * field[b, t, n]: one fp32 fused multiply-add chain per value over t ascending.  A value depends on its sample,
        its weight row and its node alone, so any cut of the conditions into batches gives the same bits.  out: a contiguous fp32
        CUDA tensor [B, R, N] to write into (a slice along the first axis of a larger one will do).  Nothing synchronises;
        afterwards xhat() raises, as after generate()."""
        t = self.torch
        N, T = self.cfg.num_node, self.cfg.num_time
        R = _weight_rows(weights, T, MAX_TEMPORAL)

        def tail(B):
            res = _out_tensor(out, (B, R, N), t.float32)
            return (_ptr(weights), R, _ptr(res)), res
        return self._surrogate("sgv_temporal", z, xs, scale, min, fix, tail)

    def gram(self, z, xs, scale, min, node_weights=None, offset=None, fix=True, out=None):
        """The temporal Gram matrix of the field generate() would write, by the recon head's last pass itself; the field is never
        stored.  Same inputs and checks as summarize(); num_time <= MAX_GRAM_T.  node_weights (w) and offset (m): contiguous fp32
        CUDA [N] or None for w = 1 / m = 0 (predict.gram_weights and gram_offset validate and upload host arrays).  Returns fp32
        CUDA [B, T, T], values[b, t, t'] = sum over n of w[n] * (field[b, t, n] - m[n]) * (field[b, t', n] - m[n]) on the matrix
        cores in fp32: bitwise symmetric, the diagonal >= 0 for w >= 0.  A matrix depends on its sample alone, so any cut of the
        conditions into batches gives the same bits.  out: a contiguous fp32 CUDA tensor [B, T, T] to write into (a slice along the
        first axis of a larger one will do).  Nothing synchronises; afterwards xhat() raises, as after generate()."""
        t = self.torch
        N, T = self.cfg.num_node, self.cfg.num_time
        if T > MAX_GRAM_T:
            raise ValueError(f"num_time = {T} is beyond the limit of {MAX_GRAM_T} time steps of the Gram pass")
        for name, a in (("node_weights", node_weights), ("offset", offset)):
            if a is not None and not is_tensor_of(a, t.float32, (N,)):
                raise ValueError(f"{name} must be None or a contiguous float32 CUDA tensor of shape [{N}]")

        def tail(B):
            res = _out_tensor(out, (B, T, T), t.float32)
            return (_ptr(node_weights), _ptr(offset), _ptr(res)), res
        return self._surrogate("sgv_gram", z, xs, scale, min, fix, tail)

    def exceedance(self, z, xs, scale, min, levels, side="above", fix=True, stats=True, excess=True):
        """The level-crossing statistics over time of the field generate() would write, by the recon head's last pass itself; the
        field is never stored.  Same inputs and checks as summarize(); num_time <= EXCEEDANCE_MAX_T.  levels: contiguous fp32 CUDA
        [L, N], 1 <= L <= MAX_LEVELS (predict.exceedance_levels validates and shapes a host array); side "above" or "below": a
        time step exceeds its level when the value is strictly above / below it.  stats, excess: True for a new tensor, False to
        leave that output out (not both), or a contiguous CUDA tensor to write into, int32 [B, 5, L, N] / fp32 [B, L, N] (a slice
        along the first axis of a larger one will do).  Returns {"stats": ..., "excess": ...} with the outputs asked for:
        stats[b, k] for k in EXCEEDANCE_STATS order is count (steps that exceed), first and last (their smallest and largest time
        step, -1 if none), longest (the longest run of consecutive exceeding steps) and runs (the number of maximal runs);
        excess[b, l, n] is the fp32 sum over the exceeding steps, t ascending, of fl(value - level) (fl(level - value) below),
        exactly +0.0 where nothing exceeds.  Every output depends on its sample, level and node alone, so any cut of the conditions
        into batches gives the same bits.  Nothing synchronises; afterwards xhat() raises, as after generate()."""
        t = self.torch
        N, T = self.cfg.num_node, self.cfg.num_time
        if T > EXCEEDANCE_MAX_T:
            raise ValueError(f"num_time = {T} is beyond the limit of {EXCEEDANCE_MAX_T} time steps of the exceedance pass")
        if side not in EXCEEDANCE_SIDES:
            raise ValueError(f"side must be one of {sorted(EXCEEDANCE_SIDES)}, not {side!r}")
        L = _weight_rows(levels, N, MAX_LEVELS, "levels", "L")
        if stats is False and excess is False:
            raise ValueError("nothing to compute: stats and excess are both False")

        def tail(B):
            res = {}
            for name, v, dt, shape in (("stats", stats, t.int32, (B, 5, L, N)), ("excess", excess, t.float32, (B, L, N))):
                if v is not False:
                    res[name] = _out_tensor(v, shape, dt, f"{name} must be True, False or a contiguous {dt} CUDA tensor", new=True)
            return (_ptr(levels), L, EXCEEDANCE_SIDES[side], _ptr(res.get("stats")), _ptr(res.get("excess"))), res
        return self._surrogate("sgv_exceedance", z, xs, scale, min, fix, tail)

    def cycles(self, z, xs, scale, min, gate, exponent=3, fix=True, turns=True, rates=True):
        """The load cycles and the rates of every node's time history in the field generate() would write, by the recon head's last
        pass itself; the field is never stored.  Same inputs and checks as summarize(); num_time <= CYCLES_MAX_T.  gate: contiguous
        fp32 CUDA [N], >= 0 (predict.cycles_gate validates a host array); exponent: the integer m of the damage sum, 1 <= m <=
        MAX_CYCLES_EXPONENT.  turns, rates: True for new tensors, False to leave the group out (not both), or a pair of contiguous
        CUDA tensors to write into, (reversals int32 [B, N], ranges fp32 [B, 4, N]) / (rate_when int32 [B, 2, N], rates fp32
        [B, 3, N]) (slices along the first axis of larger ones will do).  Returns a dict with the tensors of the groups asked for.
        The turns are ASTM E1049 simple-range counting behind the hysteresis gate: reversals is the number of confirmed turning
        points, ranges[b, k] for k in CYCLES_RANGES order the sum and the largest of the ranges between successive turning points,
        the damage sum of range^m and the open excursion at the end; rates[b, k] for k in CYCLES_RATES order is the largest and the
        smallest first difference and the path length, rate_when[b] the steps of the first two (-1 at num_time = 1); the contract,
        to the rounding, is in include/sgvae.h (sgv_cycles_out).  Every output depends on its sample and node alone, so any cut of
        the conditions into batches gives the same bits.  Nothing synchronises; afterwards xhat() raises, as after generate()."""
        t = self.torch
        N, T = self.cfg.num_node, self.cfg.num_time
        if T > CYCLES_MAX_T:
            raise ValueError(f"num_time = {T} is beyond the limit of {CYCLES_MAX_T} time steps of the cycles pass")
        if not is_tensor_of(gate, t.float32, (N,)):
            raise ValueError(f"gate must be a contiguous float32 CUDA tensor of shape [{N}]")
        m = int(exponent)
        if m != exponent or m < 1 or m > MAX_CYCLES_EXPONENT:
            raise ValueError(f"exponent = {exponent!r} is not an integer in [1, {MAX_CYCLES_EXPONENT}]")
        if turns is False and rates is False:
            raise ValueError("nothing to compute: turns and rates are both False")

        def tail(B):
            res = {}
            groups = (("turns", turns, (("reversals", t.int32, (B, N)), ("ranges", t.float32, (B, 4, N)))),
                      ("rates", rates, (("rate_when", t.int32, (B, 2, N)), ("rates", t.float32, (B, 3, N)))))
            for group, v, parts in groups:
                if v is False:
                    continue
                if v is not True and not (isinstance(v, (tuple, list)) and len(v) == len(parts)):
                    raise ValueError(f"{group} must be True, False or a pair of CUDA tensors ({parts[0][0]}, {parts[1][0]})")
                for k, (name, dt, shape) in enumerate(parts):
                    res[name] = _out_tensor(True if v is True else v[k], shape, dt, f"{name} must be a contiguous {dt} CUDA tensor", new=True)
            return (_ptr(gate), m, C.byref(CyclesOut(**{name: v.data_ptr() for name, v in res.items()}))), res
        return self._surrogate("sgv_cycles", z, xs, scale, min, fix, tail)

    def copy_stream(self) -> int:
        """Raw HIP stream of the engine's device-to-host copies (include/sgvae.h: sgv_copy_stream); wrap with torch.cuda.ExternalStream."""
        p = C.c_void_p()
        _check(self.lib, self.lib.sgv_copy_stream(self.h, C.byref(p)), "sgv_copy_stream")
        return p.value

    def encode(self):
        B, Z, Hd = self.batch, self.cfg.latent_dim, self.cfg.hierarchical_dim
        mu = np.empty((B, Z), np.float32)
        lv = np.empty((B, Z), np.float32)
        xs = np.empty((self.n_kl, B, Hd), np.float32)
        _check(self.lib, self.lib.sgv_encode(self.h, mu.ctypes.data_as(C.c_void_p), lv.ctypes.data_as(C.c_void_p),
                                             xs.ctypes.data_as(C.c_void_p)), "sgv_encode")
        return mu, lv, [xs[i] for i in range(self.n_kl)]

    def xhat(self):
        t = self.torch
        out = t.empty((self.batch, self.cfg.num_node, self.cfg.num_time), dtype=t.float32, device="cuda")
        _check(self.lib, self.lib.sgv_get_xhat(self.h, C.c_void_p(out.data_ptr())), "sgv_get_xhat")
        return out

    def activation(self, name: str, shape) -> np.ndarray:
        a = np.empty(shape, dtype=np.float32)
        _check(self.lib, self.lib.sgv_get_activation(self.h, name.encode(), a.ctypes.data_as(C.c_void_p), a.size),
               f"sgv_get_activation({name})")
        return a

    def backward(self, alpha: float, beta: float):
        _check(self.lib, self.lib.sgv_backward(self.h, float(alpha), float(beta)), "sgv_backward")

    def backward_step(self, alpha: float, beta: float, lr: float):
        """backward + AdamW with the optimizer of finished buckets overlapped under the rest of backward."""
        _check(self.lib, self.lib.sgv_backward_step(self.h, float(alpha), float(beta), float(lr)), "sgv_backward_step")

    def grad_norm(self) -> float:
        d = C.c_double()
        _check(self.lib, self.lib.sgv_grad_norm(self.h, C.byref(d)), "sgv_grad_norm")
        return d.value

    def adamw_step(self, lr: float):
        _check(self.lib, self.lib.sgv_adamw_step(self.h, float(lr)), "sgv_adamw_step")

    def adamw_step_range(self, lr: float, bucket_lo: int, bucket_hi: int, first: bool, last: bool):
        _check(self.lib, self.lib.sgv_adamw_step_range(self.h, float(lr), int(bucket_lo), int(bucket_hi), int(first), int(last)),
               "sgv_adamw_step_range")

    def bucket_count(self) -> int:
        return int(self.lib.sgv_bucket_count(self.h))

    def bucket_dots(self, bucket: int):
        """(offset, count) in the fp32 gradient arena of the <G,W> scalars of weight bucket `bucket`'s conv layers."""
        off, cnt = C.c_size_t(), C.c_size_t()
        _check(self.lib, self.lib.sgv_bucket_dots(self.h, int(bucket), C.byref(off), C.byref(cnt)), "sgv_bucket_dots")
        return off.value, cnt.value

    def comm_stream(self) -> int:
        """Raw HIP stream for set_rccl that the engine placed on a hardware queue of its own (include/sgvae.h: sgv_comm_stream)."""
        p = C.c_void_p()
        _check(self.lib, self.lib.sgv_comm_stream(self.h, C.byref(p)), "sgv_comm_stream")
        return p.value

    def wire_stream(self) -> int:
        """Raw HIP stream released buckets are complete (and packed) on once option "wire_stream" is set."""
        p = C.c_void_p()
        _check(self.lib, self.lib.sgv_wire_stream(self.h, C.byref(p)), "sgv_wire_stream")
        return p.value

    def opt_stream(self) -> int:
        """Raw HIP stream the ahead-of-step bucket updates run on (wrap with torch.cuda.ExternalStream)."""
        p = C.c_void_p()
        _check(self.lib, self.lib.sgv_opt_stream(self.h, C.byref(p)), "sgv_opt_stream")
        return p.value

    def adamw_bucket_async(self, lr: float, bucket: int):
        """AdamW of one weight bucket's conv weights on the optimizer stream (include/sgvae.h: the caller has made that stream
        wait for the bucket's and its <G,W> scalars' all-reduce); the closing adamw_step_range calls skip it."""
        _check(self.lib, self.lib.sgv_adamw_bucket_async(self.h, float(lr), int(bucket)), "sgv_adamw_bucket_async")

    def last_grad_norm(self) -> float:
        d = C.c_double()
        _check(self.lib, self.lib.sgv_last_grad_norm(self.h, C.byref(d)), "sgv_last_grad_norm")
        return d.value

    def memory_info(self):
        """dict of device bytes: params, grads, adam, copies, activations, workspaces."""
        buf = (C.c_size_t * 6)()
        _check(self.lib, self.lib.sgv_memory_info(self.h, buf), "sgv_memory_info")
        return dict(zip(("params", "grads", "adam", "copies", "activations", "workspaces"), [int(v) for v in buf]))

    def recompute_bytes(self) -> int:
        """Bytes of the activation maps the last backward regenerated under option "recompute_activations" (include/sgvae.h)."""
        n = C.c_size_t()
        _check(self.lib, self.lib.sgv_recompute_bytes(self.h, C.byref(n)), "sgv_recompute_bytes")
        return int(n.value)

    def accumulate_scalars(self):
        """Add the scalars of the step just enqueued to the device-side epoch accumulator (no host sync)."""
        _check(self.lib, self.lib.sgv_scalars_accumulate(self.h), "sgv_scalars_accumulate")

    def read_accumulated(self, reset: bool = True):
        """dict(recon, kls, mse, grad_norm, steps): sums over the accumulated steps (one host sync)."""
        buf = (C.c_double * 16)()
        _check(self.lib, self.lib.sgv_scalars_read(self.h, buf, int(reset)), "sgv_scalars_read")
        return dict(recon=buf[0], kls=[buf[1 + i] for i in range(self.n_kl)], mse=buf[8], grad_norm=buf[9], steps=int(buf[10]))

    def grad_buffer(self):
        """(device pointer, element count) of the flat fp32 gradient arena."""
        p, n = C.c_void_p(), C.c_size_t()
        _check(self.lib, self.lib.sgv_grad_buffer(self.h, C.byref(p), C.byref(n)), "sgv_grad_buffer")
        return p.value, n.value

    def set_grad_payload(self, dtype: str):
        """Wire format of the data-parallel weight buckets: "f32" (the arena itself) or "bf16" (include/sgvae.h: sgv_set_grad_payload)."""
        _check(self.lib, self.lib.sgv_set_grad_payload(self.h, DTYPES[dtype]), "sgv_set_grad_payload")

    def grad_payload_buffer(self):
        """(device pointer, element count) of the bf16 payload buffer (same element offsets as the fp32 arena)."""
        p, n = C.c_void_p(), C.c_size_t()
        _check(self.lib, self.lib.sgv_grad_payload_buffer(self.h, C.byref(p), C.byref(n)), "sgv_grad_payload_buffer")
        return p.value, n.value

    def grad_payload_unpack(self):
        _check(self.lib, self.lib.sgv_grad_payload_unpack(self.h), "sgv_grad_payload_unpack")

    def scale_grads(self, f: float):
        _check(self.lib, self.lib.sgv_scale_grads(self.h, float(f)), "sgv_scale_grads")

    def set_bucket_callback(self, fn):
        """fn(bucket, offset_elems, count_elems) is called from inside backward()."""
        if fn is None:
            self._cb = BUCKET_CB(0)
        else:
            self._cb = BUCKET_CB(lambda user, b, off, cnt: fn(b, off, cnt))
        _check(self.lib, self.lib.sgv_set_bucket_callback(self.h, self._cb, None), "sgv_set_bucket_callback")

    def set_rccl(self, comm, comm_stream):
        """Register an RCCL communicator (sgv_rccl_comm_init) + communication stream: backward() then issues the bucket
        all-reduces itself and adamw_step() / backward_step() wait for them bucket by bucket.  comm=None unregisters."""
        _check(self.lib, self.lib.sgv_set_rccl(self.h, C.c_void_p(comm), C.c_void_p(comm_stream) if comm else None), "sgv_set_rccl")

    def stream_overlaps(self):
        """Probe results for the engine's auxiliary streams (second lane, weight-gradient side stream, optimizer stream,
        communication stream): 1 = its kernels run beside the main stream's, 0 = it shares the main stream's hardware queue (the
        overlap it exists for is lost), -1 = the stream does not exist.  Creates the optimizer / communication streams."""
        out = {}
        for which, name in enumerate(("lane", "side", "opt", "comm")):
            v = C.c_int(-2)
            _check(self.lib, self.lib.sgv_test_stream_overlap(self.h, which, C.byref(v)), "sgv_test_stream_overlap")
            out[name] = v.value
        return out

    def stream_overlaps_existing(self):
        """stream_overlaps() for the streams a single-GPU engine has (lane, side) -- creates nothing."""
        out = {}
        for which, name in enumerate(("lane", "side")):
            v = C.c_int(-2)
            _check(self.lib, self.lib.sgv_test_stream_overlap(self.h, which, C.byref(v)), "sgv_test_stream_overlap")
            out[name] = v.value
        return out

    def allreduce_grads(self, comm, comm_stream=None):
        """Mean all-reduce of the whole gradient arena (stream-ordered, not overlapped)."""
        _check(self.lib, self.lib.sgv_allreduce_grads(self.h, C.c_void_p(comm), C.c_void_p(comm_stream) if comm_stream else None),
               "sgv_allreduce_grads")

    # ---- data ----
    def sample_bytes(self) -> int:
        return self.lib.sgv_dataset_sample_bytes(self.h)

    def dataset_convert(self, src, dst, count: int):
        _check(self.lib, self.lib.sgv_dataset_convert(self.h, C.c_void_p(src.data_ptr()), C.c_void_p(dst.data_ptr()),
                                                      count), "sgv_dataset_convert")

    def augment_collate(self, dataset, idx, noise_seed, scale, mix_idx, lam):
        idx = np.ascontiguousarray(idx, np.int32)
        ns = np.ascontiguousarray(noise_seed, np.uint64)
        sc = np.ascontiguousarray(scale, np.float32)
        mi = np.ascontiguousarray(mix_idx, np.int32)
        lm = np.ascontiguousarray(lam, np.float32)
        B = len(idx)
        _check(self.lib, self.lib.sgv_augment_collate(self.h, C.c_void_p(dataset.data_ptr()), B,
                                                      idx.ctypes.data_as(C.c_void_p), ns.ctypes.data_as(C.c_void_p),
                                                      sc.ctypes.data_as(C.c_void_p), mi.ctypes.data_as(C.c_void_p),
                                                      lm.ctypes.data_as(C.c_void_p)), "sgv_augment_collate")
        self.batch = B

    def augment_stage(self, dataset, idx, noise_seed, scale, mix_idx, lam):
        """Prefetch: enqueue the NEXT batch's augmentation into the spare input buffer (runs beside the current step)."""
        idx = np.ascontiguousarray(idx, np.int32)
        ns = np.ascontiguousarray(noise_seed, np.uint64)
        sc = np.ascontiguousarray(scale, np.float32)
        mi = np.ascontiguousarray(mix_idx, np.int32)
        lm = np.ascontiguousarray(lam, np.float32)
        _check(self.lib, self.lib.sgv_augment_stage(self.h, C.c_void_p(dataset.data_ptr()), len(idx),
                                                    idx.ctypes.data_as(C.c_void_p), ns.ctypes.data_as(C.c_void_p),
                                                    sc.ctypes.data_as(C.c_void_p), mi.ctypes.data_as(C.c_void_p),
                                                    lm.ctypes.data_as(C.c_void_p)), "sgv_augment_stage")
        self._staged_batch = len(idx)

    def augment_advance(self):
        """The staged batch becomes the current input."""
        _check(self.lib, self.lib.sgv_augment_advance(self.h), "sgv_augment_advance")
        self.batch = self._staged_batch

    # ---- profiling ----
    def kernel_time_reset(self, enable: bool):
        _check(self.lib, self.lib.sgv_kernel_time_reset(self.h, int(enable)), "sgv_kernel_time_reset")

    def kernel_time_tags(self):
        """[(tag, total_ms, launches)] for every timer tag (per layer and shape after kernel_time_reset(2))."""
        out, i = [], 0
        buf = C.create_string_buffer(256)
        while True:
            ms, n = C.c_float(), C.c_int()
            if self.lib.sgv_kernel_time_tag(self.h, i, buf, 256, C.byref(ms), C.byref(n)) != 0:
                return out
            if n.value:
                out.append((buf.value.decode(), ms.value, n.value))
            i += 1

    def kernel_time(self, which: str):
        ms, n = C.c_float(), C.c_int()
        _check(self.lib, self.lib.sgv_kernel_time(self.h, which.encode(), C.byref(ms), C.byref(n)), "sgv_kernel_time")
        return ms.value, n.value
