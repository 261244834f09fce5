"""Surrogate prediction: a trained VAE plus a trained latent conditioner as a simulator -- conditions in, `[T, N]` fields in
physical units out.  Not a mirror of anything in the reference, which has no such entry point; it is not
registered by install_reference_api().

Per batch: conditioner forward (eval mode) -> MinMaxScaler.inverse_transform of both latent heads (`ops.cols_sub_div`) -> the VAE
decoder (`Engine.generate`), whose last kernel applies tanh, the recon head's GroupNorm and the inverse of `data_scaler` in fp32 and
writes the field straight into the caller's buffer.  The three scalers are anything with `scale_` and `min_` arrays (sklearn's
MinMaxScaler, GpuMinMaxScaler, a namespace); sklearn itself is only needed to unpickle the files `from_files` reads.

Host waits: none between batches.  One in front of the first batch, and only with the image conditioner and conditions that are
already on the device: whether they are in [-1, 1] (the model then maps them to [0, 1]) is read back once, a full pass over
`[P, H*W]` on the caller's stream, instead of once per batch inside the model's forward; host conditions are ranged with numpy and
the parametric conditioner has no such test.  `predict_to_host` adds its one wait at the end.

    s = Surrogate.from_files("model_save", batch=16)
    fields = s.predict(conditions)                 # [P, T, N] fp32 on the device, physical units
    fields = s.predict_to_host(conditions)         # the same in pinned host memory, for P too large for the device
"""
from __future__ import annotations

import inspect
import os
import pickle

import numpy as np

from .engine import LAYOUTS

FILES = {"vae": "SimulGen-VAE", "conditioner": "LatentConditioner", "data_scaler": "scaler.pkl",
         "latent_scaler": "latent_vectors_scaler.pkl", "xs_scaler": "xs_scaler.pkl"}      # names the mirrors write under model_save/


def scaler_vectors(scaler, name, length, what):
    """(scale_, min_) of a fitted min-max scaler as float32 numpy vectors of `length` (= `what`) entries; ValueError naming the
    scaler and the first offending index otherwise.  numpy only."""
    try:
        scale, mn = np.asarray(scaler.scale_, np.float64).reshape(-1), np.asarray(scaler.min_, np.float64).reshape(-1)
    except AttributeError:
        raise ValueError(f"{name}: a fitted scaler with scale_ and min_ arrays is required") from None
    if scale.size != length or mn.size != length:
        raise ValueError(f"{name}: scale_ / min_ hold {scale.size} / {mn.size} entries, expected {what} = {length}")
    s32 = scale.astype(np.float32)
    bad = np.flatnonzero(~np.isfinite(s32) | (s32 == 0.0))
    if bad.size:
        raise ValueError(f"{name}: scale_[{int(bad[0])}] = {scale[bad[0]]!r} is zero or not finite (the inverse transform divides by it)")
    bad = np.flatnonzero(~np.isfinite(mn.astype(np.float32)))
    if bad.size:
        raise ValueError(f"{name}: min_[{int(bad[0])}] = {mn[bad[0]]!r} is not finite")
    return s32, mn.astype(np.float32)


class Surrogate:
    def __init__(self, vae, conditioner, latent_scaler, xs_scaler, data_scaler, batch=16, seed=0):
        """vae: the mirror VAE; conditioner: LatentConditionerImg or the parametric LatentConditioner (put in eval mode);
        scalers: duck-typed (scale_, min_).  The engine runs at max_batch = batch and is seeded with `seed`.
        The engine is the VAE object's own, shared with everything else that uses that object: constructing a Surrogate re-seeds
        it (sgv_seed: the noise position goes back to 0), which changes the noise of any later training or sampling on the same
        VAE.  If the VAE rebuilds its engine later (a call with a larger batch), the next predict picks the new engine up and
        seeds it again with `seed`."""
        cfg = vae.cfg
        self.batch = int(batch)
        if self.batch < 1:
            raise ValueError(f"batch must be >= 1, not {batch}")
        self.size2, self.hier = int(conditioner.size2), int(conditioner.latent_dim)
        self.latent_end = int(conditioner.latent_dim_end)
        vecs = [scaler_vectors(latent_scaler, "latent_scaler", self.latent_end, "latent_dim_end"),
                scaler_vectors(xs_scaler, "xs_scaler", self.size2 * self.hier, "size2 * latent_dim"),
                scaler_vectors(data_scaler, "data_scaler", cfg.num_node, "num_node")]
        n_kl = len(cfg.num_filter_enc) - 1
        if self.latent_end != cfg.latent_dim or self.hier != cfg.hierarchical_dim or self.size2 != n_kl:
            raise ValueError(f"the conditioner predicts latents of ({self.latent_end}, {self.size2} x {self.hier}), the VAE decodes "
                             f"({cfg.latent_dim}, {n_kl} x {cfg.hierarchical_dim})")
        import torch
        self.torch = torch
        self.vae, self.conditioner = vae, conditioner.eval()
        self.N, self.T = cfg.num_node, cfg.num_time
        self.seed = int(seed)
        # whether the conditioner's forward can be told the input range instead of reading the batch's minimum back (image model)
        try:
            self._takes_remap = "remap" in inspect.signature(getattr(conditioner, "forward", conditioner)).parameters
        except (TypeError, ValueError):
            self._takes_remap = False
        self.eng = None
        self._engine()
        # the six vectors, uploaded once
        (self.lat_scale, self.lat_min), (self.xs_scale, self.xs_min), (self.data_scale, self.data_min) = (
            tuple(torch.from_numpy(a).cuda() for a in pair) for pair in vecs)

    def _engine(self):
        """the VAE's engine at max_batch >= batch; a new engine object (first use, or rebuilt by the VAE) is seeded and its streams wrapped"""
        eng = self.vae._eng(self.batch)
        if eng is not self.eng:
            t = self.torch
            self.eng = eng
            eng.seed(self.seed)
            self._stream = t.cuda.ExternalStream(eng.stream) if eng.stream else t.cuda.default_stream()
            self._copy_stream = None
        return eng

    @classmethod
    def from_files(cls, model_dir="model_save", **kw):
        """The files a training run of the mirrors leaves in `model_dir`; FileNotFoundError names the first one missing."""
        paths = {k: os.path.join(model_dir, v) for k, v in FILES.items()}
        for p in paths.values():
            if not os.path.exists(p):
                raise FileNotFoundError(f"Surrogate.from_files: {p} not found")
        import torch
        vae = torch.load(paths["vae"], map_location="cpu", weights_only=False)
        loaded = {}
        for k in ("conditioner", "latent_scaler", "xs_scaler", "data_scaler"):
            with open(paths[k], "rb") as f:
                loaded[k] = pickle.load(f)
        return cls(vae, loaded["conditioner"], loaded["latent_scaler"], loaded["xs_scaler"], loaded["data_scaler"], **kw)

    # ---- one batch: conditions [b, F] -> the field, written into `dst` ([b, T, N] or [b, N, T]) on the engine stream ----
    def _generate(self, cond, dst, layout, fix, remap):
        from . import ops
        y = self.conditioner(cond, remap=remap) if self._takes_remap else self.conditioner(cond)
        y1, y2 = (y["latent_main"], y["xs"]) if isinstance(y, dict) else y          # a conditioner built with return_dict=True
        b = y1.shape[0]
        lat = ops.cols_sub_div(y1.contiguous(), self.lat_min, self.lat_scale)
        xs = ops.cols_sub_div(y2.reshape(b, -1).contiguous(), self.xs_min, self.xs_scale)
        # list order of ReconstructionEvaluator._reconstruct_from_latents: xs_list[k] = columns k*d .. (k+1)*d
        xs = xs.view(b, self.size2, self.hier).transpose(0, 1).contiguous()
        self.eng.generate(lat, xs, self.data_scale, self.data_min, out=dst, layout=layout, fix=fix)

    def _args(self, conditions, layout, mode):
        t = self.torch
        if layout not in LAYOUTS:
            raise ValueError(f"layout must be one of {sorted(LAYOUTS)}, not {layout!r}")
        if mode not in ("fix", "random"):
            raise ValueError(f"mode must be 'fix' or 'random', not {mode!r}")
        if not t.is_tensor(conditions):
            conditions = t.from_numpy(np.ascontiguousarray(conditions, dtype=np.float32))
        if conditions.dim() != 2:
            raise ValueError(f"conditions must be [P, F], got {tuple(conditions.shape)}")
        P = conditions.shape[0]
        shape = (P, self.T, self.N) if layout == "TN" else (P, self.N, self.T)
        # the image model maps inputs in [-1, 1] to [0, 1] when a batch's minimum is below -0.1, which it reads back per call;
        # decided here once for all of `conditions` instead (host data: no device involved; device data: one read, before
        # anything is enqueued), so that no batch makes the host wait for the stream
        remap = bool(P > 0 and float(conditions.min()) < -0.1) if self._takes_remap else None
        self._engine()
        return conditions, P, shape, remap

    def _batch(self, conditions, lo, hi):
        return conditions[lo:hi].to(device="cuda", dtype=self.torch.float32, non_blocking=True)

    def predict(self, conditions, out=None, layout="TN", mode="fix"):
        """conditions [P, F] (host array or CUDA tensor, preprocessed as the conditioner's training set holds them) -> fp32 device
        tensor [P, T, N] (layout "TN") or [P, N, T] ("NT") in physical units.  mode "fix": the mean (the reference's "fix": the
        latents' noise times 1e-10, so bitwise-equal results need the same seed and call sequence); "random": sampled.
        Nothing makes the host wait between batches; with the image conditioner the input range is decided once for all of
        `conditions` in front of the first batch (see _args: for a CUDA tensor that is one device-to-host read), not per batch as
        the model's own forward does.  Host conditions in pageable memory are uploaded
        batch by batch with blocking copies; pass a pinned or a CUDA tensor to keep the host ahead."""
        t = self.torch
        conditions, P, shape, remap = self._args(conditions, layout, mode)
        if out is None:
            out = t.empty(shape, dtype=t.float32, device="cuda")
        elif not (t.is_tensor(out) and out.is_cuda and out.dtype == t.float32 and out.is_contiguous() and tuple(out.shape) == shape):
            raise ValueError(f"out must be a contiguous float32 CUDA tensor of shape {shape}")
        self._stream.wait_stream(t.cuda.current_stream())             # conditions / out may come from the caller's stream
        with t.cuda.stream(self._stream):
            for lo in range(0, P, self.batch):
                hi = min(P, lo + self.batch)
                self._generate(self._batch(conditions, lo, hi), out[lo:hi], layout, mode == "fix", remap)
        if t.cuda.current_stream() != self._stream:
            t.cuda.current_stream().wait_stream(self._stream)
        return out

    def predict_to_host(self, conditions, out=None, layout="TN", mode="fix"):
        """The same result in pinned host memory: two device batch buffers alternate, each batch's device-to-host copy runs on the
        engine's copy stream behind the batch's last kernel, and the host waits once, at the end."""
        t = self.torch
        conditions, P, shape, remap = self._args(conditions, layout, mode)
        if out is None:
            out = t.empty(shape, dtype=t.float32, pin_memory=True)
        elif not (t.is_tensor(out) and out.device.type == "cpu" and out.is_pinned() and out.dtype == t.float32 and out.is_contiguous()
                  and tuple(out.shape) == shape):
            raise ValueError(f"out must be a contiguous pinned float32 CPU tensor of shape {shape}")
        if self._copy_stream is None:
            self._copy_stream = t.cuda.ExternalStream(self.eng.copy_stream())
        cs = self._copy_stream
        self._stream.wait_stream(t.cuda.current_stream())
        with t.cuda.stream(self._stream):
            bufs = [t.empty((self.batch,) + shape[1:], dtype=t.float32, device="cuda") for _ in range(min(2, (P + self.batch - 1) // self.batch))]
        copied = [None, None]
        for i, lo in enumerate(range(0, P, self.batch)):
            hi = min(P, lo + self.batch)
            buf = bufs[i % 2][:hi - lo]
            with t.cuda.stream(self._stream):
                if copied[i % 2] is not None:
                    self._stream.wait_event(copied[i % 2])          # the buffer's previous copy has left it
                self._generate(self._batch(conditions, lo, hi), buf, layout, mode == "fix", remap)
                done = t.cuda.Event()
                done.record(self._stream)
            cs.wait_event(done)
            with t.cuda.stream(cs):
                out[lo:hi].copy_(buf, non_blocking=True)
                copied[i % 2] = t.cuda.Event()
                copied[i % 2].record(cs)
        cs.synchronize()                                             # the one host wait; the buffers are free again after it
        return out
