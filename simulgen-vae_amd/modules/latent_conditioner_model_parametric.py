"""`LatentConditioner` (the MLP over tabular simulation parameters) with the constructor / state_dict of the reference's
modules.latent_conditioner_model_parametric.LatentConditioner (latent_conditioner_model_parametric.py:25-213), on the MI355X.

  m = LatentConditioner(latent_conditioner_filter, latent_dim_end, input_shape, latent_dim, size2, dropout_rate=0.3)
  latent_main, xs = m(x)                       # x: [B, input_shape] -> [B, latent_dim_end], [B, size2, latent_dim]
  m.loss_backward(x, y1, y2)                   # forward, 10*MSE(y1) + MSE(y2), backward -> gradients in m.grads

The layer graph and its hand-derived backward live here; every tensor operation is a HIP kernel of csrc/mlp.hip
(include/sgvae_ops.h, sgv_op_mlp_*), two launches per dense layer in each direction:
  forward   sgv_op_mlp_gemm_fwd (Linear; linear2 + skip Linear of a ResidualBlock, and the same layer of both heads, share a
            launch) then sgv_op_mlp_rows_fwd (LayerNorm [+ LayerNorm'd skip | + identity] -> GELU -> dropout; the
            feature_projection LayerNorm + dropout folded into the last block's tail);
  backward  sgv_op_mlp_rows_bwd (dropout, [LayerNorm c], GELU', LayerNorm backward, per-row dgamma / dbeta partials) then
            sgv_op_mlp_gemm_bwd (dX summed over main and skip paths, dW, db, the batch sums of the partials).
Parameters and gradients live in two flat arenas with every slot padded to a multiple of 4 floats (zeros), so the fused
clip + AdamW pass (ops.ParamSet) takes every CSV width; gradients are written straight into their slots.  The dropout
masks of a training step are one torch.rand draw over all sites (keep where u >= p); tests inject 0/1 masks instead."""
from __future__ import annotations

import math

import numpy as np
import torch

from .. import ops
from ..engine import SgvError


def head_width(latent_dim_end, final_feature_size, input_shape):
    """hidden_size of the two heads (reference :150-151)."""
    complexity_ratio = min(8, max(2, int(input_shape) // 64))
    return max(int(latent_dim_end) * 2, int(final_feature_size) // complexity_ratio)


def param_spec(latent_conditioner_filter, latent_dim_end, input_shape, latent_dim, size2):
    """[(name, shape)] of every parameter in the reference's state_dict order (the model has no buffers).  Host only."""
    filters = [int(v) for v in latent_conditioner_filter]
    out = []

    def lin(prefix, o, k):
        out.extend([(prefix + ".weight", (o, k)), (prefix + ".bias", (o,))])

    def ln(prefix, c):
        out.extend([(prefix + ".weight", (c,)), (prefix + ".bias", (c,))])
    ln("input_norm", int(input_shape))
    cur = int(input_shape)
    for i, f in enumerate(filters):
        p = f"backbone.{i}"
        if i == 0:
            lin(p + ".0", f, cur)
            ln(p + ".1", f)
        else:
            lin(p + ".linear1", f, cur)
            ln(p + ".ln1", f)
            lin(p + ".linear2", f, f)
            ln(p + ".ln2", f)
            if cur != f:
                lin(p + ".skip_connection.0", f, cur)
                ln(p + ".skip_connection.1", f)
        cur = f
    ln("feature_projection.0", cur)
    h = head_width(latent_dim_end, cur, input_shape)
    for head, odim in (("latent_out", int(latent_dim_end)), ("xs_out", int(latent_dim) * int(size2))):
        lin(head + ".0", h, cur)
        ln(head + ".1", h)
        lin(head + ".4", h // 2, h)
        ln(head + ".5", h // 2)
        lin(head + ".8", odim, h // 2)
    return out


def dropout_sites(latent_conditioner_filter, latent_dim_end, input_shape, dropout_rate):
    """[(site, width, p)] of the Dropout layers in the order the reference's forward calls them."""
    filters = [int(v) for v in latent_conditioner_filter]
    r = float(dropout_rate)
    sched = [r * 0.5, r * 0.7, r * 1.0, r * 1.2]
    sites = [(f"backbone.{i}", f, sched[min(i, 3)]) for i, f in enumerate(filters)]
    sites.append(("feature_projection", filters[-1], r * 0.8))
    h = head_width(latent_dim_end, filters[-1], input_shape)
    for head in ("latent_out", "xs_out"):
        sites += [(head + ".3", h, r * 0.6), (head + ".7", h // 2, r * 0.4)]
    return sites


class LatentConditioner:
    def __init__(self, latent_conditioner_filter, latent_dim_end, input_shape, latent_dim, size2, dropout_rate=0.3, seed=0):
        self.latent_conditioner_filter = [int(v) for v in latent_conditioner_filter]
        if not self.latent_conditioner_filter:
            raise SgvError("latent_conditioner_filter needs at least one width")
        self.latent_dim, self.size2, self.latent_dim_end = int(latent_dim), int(size2), int(latent_dim_end)
        self.input_shape, self.dropout_rate = int(input_shape), float(dropout_rate)
        self.num_latent_conditioner_filter = len(self.latent_conditioner_filter)
        self.hidden_size = head_width(self.latent_dim_end, self.latent_conditioner_filter[-1], self.input_shape)
        self.training = True
        self.pset = None
        self.grads = {}
        self._ctx = None
        self._alloc()
        self._init_state(seed)

    # ---- parameters -------------------------------------------------------------------------------------------------
    def _spec(self):
        return param_spec(self.latent_conditioner_filter, self.latent_dim_end, self.input_shape, self.latent_dim, self.size2)

    def _alloc(self):
        """Parameter and gradient arenas: slot k starts at a multiple of 4 floats (16 bytes), padding stays zero."""
        spec = self._spec()
        self._slots, off = [], 0
        for name, shape in spec:
            numel = int(np.prod(shape))
            self._slots.append((name, shape, off, (numel + 3) // 4 * 4))
            off += (numel + 3) // 4 * 4
        self._parena = torch.zeros(off, dtype=torch.float32, device="cuda")
        self._garena = torch.zeros(off, dtype=torch.float32, device="cuda")
        self.P, self.G = {}, {}
        for name, shape, o, _ in self._slots:
            numel = int(np.prod(shape))
            self.P[name] = self._parena[o:o + numel].view(shape)
            self.G[name] = self._garena[o:o + numel].view(shape)
        self.pset = None

    def _init_state(self, seed):
        """The reference constructor's `_init_weights`: xavier_uniform Linear weights, zero biases, LayerNorm ones / zeros
        (values from numpy Philox: same distributions, different stream)."""
        rng = np.random.Generator(np.random.Philox(seed))
        for name, shape in self._spec():
            if len(shape) == 2:
                bound = math.sqrt(6.0 / (shape[0] + shape[1]))
                a = rng.uniform(-bound, bound, shape)
            elif name.endswith(".bias"):
                a = np.zeros(shape)
            else:
                a = np.ones(shape)
            self.P[name].copy_(torch.from_numpy(a.astype(np.float32)))

    def state_dict(self):
        return {name: self.P[name].detach().cpu().clone() for name, _ in self._spec()}

    def load_state_dict(self, sd, strict=True):
        names = [n for n, _ in self._spec()]
        missing = [n for n in names if n not in sd]
        extra = [k for k in sd if k not in names]
        if strict and (missing or extra):
            raise RuntimeError(f"Error(s) in loading state_dict: missing {missing[:4]}, unexpected {extra[:4]}")
        for name, shape in self._spec():
            if name in sd:
                v = sd[name]
                a = torch.as_tensor(np.asarray(v.detach().cpu() if torch.is_tensor(v) else v), dtype=torch.float32)
                if tuple(a.shape) != tuple(shape):
                    raise RuntimeError(f"size mismatch for {name}: {tuple(a.shape)} vs {tuple(shape)}")
                self.P[name].copy_(a.to("cuda"))          # in place: the arena slots (and the ParamSet tables) stay valid
        return self

    def __getstate__(self):
        d = {k: v for k, v in self.__dict__.items() if k not in ("P", "G", "_parena", "_garena", "pset", "grads", "_ctx")}
        d["P"] = {k: v.detach().cpu().numpy() for k, v in self.P.items()}
        return d

    def __setstate__(self, d):
        P = d.pop("P")
        self.__dict__.update(d)
        self.grads, self._ctx = {}, None
        self._alloc()
        for k, v in P.items():
            self.P[k].copy_(torch.from_numpy(np.ascontiguousarray(v)))

    def named_parameters(self):
        return [(n, self.P[n]) for n, _ in self._spec()]

    def parameters(self):
        return [t for _, t in self.named_parameters()]

    def train(self, mode=True):
        self.training = bool(mode)
        return self

    def eval(self):
        return self.train(False)

    def to(self, device=None, *a, **k):
        if device is not None and str(device).startswith("cpu"):
            raise SgvError("this model only runs on an MI355X: there is no CPU path")
        return self

    def apply(self, fn):
        """latent_conditioner.apply(safe_initialize_weights_He) (latent_conditioner.py:169-177,223): every Linear weight
        kaiming_uniform(relu) (bound sqrt(6 / fan_in)), every Linear bias zero, LayerNorms untouched.  Values from numpy's
        generator (same distribution, different stream)."""
        rng = np.random.default_rng(int(torch.randint(0, 2 ** 31 - 1, (1,)).item()))
        for n, sh in self._spec():
            if len(sh) != 2:
                continue
            bound = math.sqrt(6.0 / sh[1])
            self.P[n].copy_(torch.from_numpy(rng.uniform(-bound, bound, sh).astype(np.float32)))
            self.P[n[:-len("weight")] + "bias"].zero_()
        return self

    def _fused(self):
        """The multi-tensor clip + AdamW pass over the padded arena slots (every slot qualifies by construction)."""
        if self.pset is None:
            entries = [dict(p=self._parena[o:o + n], g=self._garena[o:o + n]) for _, _, o, n in self._slots]
            self.pset = ops.ParamSet(entries)
        return True

    # ---- forward ----------------------------------------------------------------------------------------------------
    def _masks(self, B, dropout_masks):
        """site -> dict(mask, mask_thr, mask_scale) for the active Dropout layers of a training forward."""
        if not self.training:
            return {}
        sites = [(s, w, p) for s, w, p in dropout_sites(self.latent_conditioner_filter, self.latent_dim_end, self.input_shape,
                                                         self.dropout_rate) if p > 0.0]
        out = {}
        if dropout_masks is not None:
            masks = list(dropout_masks)
            if len(masks) != len(sites):
                raise ValueError(f"{len(masks)} dropout masks for {len(sites)} dropout layers")
            for (s, w, p), m in zip(sites, masks):
                m = torch.as_tensor(m).to(device="cuda", dtype=torch.float32).contiguous()
                if tuple(m.shape) != (B, w):
                    raise ValueError(f"dropout mask of shape {tuple(m.shape)} for {s} of shape {(B, w)}")
                out[s] = dict(mask=m, mask_thr=0.5, mask_scale=1.0 / (1.0 - p))
            return out
        u = torch.rand(B * sum(w for _, w, _ in sites), device="cuda")          # one launch for every site of the step
        off = 0
        for s, w, p in sites:
            out[s] = dict(mask=u[off:off + B * w].view(B, w), mask_thr=p, mask_scale=1.0 / (1.0 - p))
            off += B * w
        return out

    def forward(self, x, dropout_masks=None):
        """x: [B, input_shape] (anything reshapeable to it) -> (latent_main [B, latent_dim_end], xs [B, size2, latent_dim])."""
        if not torch.is_tensor(x):
            x = torch.as_tensor(np.asarray(x))
        x = x.to(device="cuda", dtype=torch.float32)
        B = x.shape[0]
        x = x.reshape(B, -1).contiguous()
        if x.shape[1] != self.input_shape:
            raise ValueError(f"input of {x.shape[1]} features for a model built for {self.input_shape}")
        P, F = self.P, self.latent_conditioner_filter
        masks = self._masks(B, dropout_masks)
        n = len(F)
        row_in = dict(za=x, ga=P["input_norm.weight"], ba=P["input_norm.bias"])
        (h, row_in["stats"]), = ops.mlp_rows_fwd([row_in], B)
        xn = h
        blocks = []
        for i in range(n):
            pre = f"backbone.{i}"
            fold_fp = i == n - 1 and i > 0          # feature_projection rides on the tail of the last ResidualBlock
            if i == 0:
                z, = ops.mlp_gemm_fwd([dict(x=h, W=P[pre + ".0.weight"], bias=P[pre + ".0.bias"])], B)
                row = dict(za=z, ga=P[pre + ".1.weight"], ba=P[pre + ".1.bias"], gelu=True, **masks.get(pre, {}))
                (out, row["stats"]), = ops.mlp_rows_fwd([row], B)
                blocks.append(dict(x=h, row=row))
            else:
                skip = (pre + ".skip_connection.0.weight") in P
                z1, = ops.mlp_gemm_fwd([dict(x=h, W=P[pre + ".linear1.weight"], bias=P[pre + ".linear1.bias"])], B)
                row1 = dict(za=z1, ga=P[pre + ".ln1.weight"], ba=P[pre + ".ln1.bias"], gelu=True, **masks.get(pre, {}))
                (a1, row1["stats"]), = ops.mlp_rows_fwd([row1], B)
                probs = [dict(x=a1, W=P[pre + ".linear2.weight"], bias=P[pre + ".linear2.bias"])]
                if skip:
                    probs.append(dict(x=h, W=P[pre + ".skip_connection.0.weight"], bias=P[pre + ".skip_connection.0.bias"]))
                zs = ops.mlp_gemm_fwd(probs, B)
                row2 = dict(za=zs[0], ga=P[pre + ".ln2.weight"], ba=P[pre + ".ln2.bias"], gelu=True)
                if skip:
                    row2.update(zb=zs[1], gb=P[pre + ".skip_connection.1.weight"], bb=P[pre + ".skip_connection.1.bias"])
                else:
                    row2["r"] = h
                if fold_fp:
                    row2.update(gc=P["feature_projection.0.weight"], bc=P["feature_projection.0.bias"], **masks.get("feature_projection", {}))
                (out, row2["stats"]), = ops.mlp_rows_fwd([row2], B)
                blocks.append(dict(x=h, a1=a1, row1=row1, row2=row2, skip=skip, fold_fp=fold_fp))
            h = out
        fp_row = None
        if n == 1:                                  # no ResidualBlock to fold into: feature_projection on its own
            fp_row = dict(za=h, ga=P["feature_projection.0.weight"], ba=P["feature_projection.0.bias"], **masks.get("feature_projection", {}))
            (h, fp_row["stats"]), = ops.mlp_rows_fwd([fp_row], B)
        features = h
        heads = ("latent_out", "xs_out")
        z0 = ops.mlp_gemm_fwd([dict(x=features, W=P[hd + ".0.weight"], bias=P[hd + ".0.bias"]) for hd in heads], B)
        rows_h1 = [dict(za=z0[k], ga=P[hd + ".1.weight"], ba=P[hd + ".1.bias"], gelu=True, **masks.get(hd + ".3", {})) for k, hd in enumerate(heads)]
        a_h1 = ops.mlp_rows_fwd(rows_h1, B)
        for r, (_, st) in zip(rows_h1, a_h1):
            r["stats"] = st
        z1 = ops.mlp_gemm_fwd([dict(x=a_h1[k][0], W=P[hd + ".4.weight"], bias=P[hd + ".4.bias"]) for k, hd in enumerate(heads)], B)
        rows_h2 = [dict(za=z1[k], ga=P[hd + ".5.weight"], ba=P[hd + ".5.bias"], gelu=True, **masks.get(hd + ".7", {})) for k, hd in enumerate(heads)]
        a_h2 = ops.mlp_rows_fwd(rows_h2, B)
        for r, (_, st) in zip(rows_h2, a_h2):
            r["stats"] = st
        y = ops.mlp_gemm_fwd([dict(x=a_h2[k][0], W=P[hd + ".8.weight"], bias=P[hd + ".8.bias"]) for k, hd in enumerate(heads)], B, tanh_out=True)
        self._ctx = dict(B=B, xn=xn, row_in=row_in, blocks=blocks, fp_row=fp_row, features=features, rows_h1=rows_h1, a_h1=[a for a, _ in a_h1],
                         rows_h2=rows_h2, a_h2=[a for a, _ in a_h2], y=y)
        return y[0], y[1].view(B, self.size2, self.latent_dim)

    __call__ = forward

    # ---- backward ---------------------------------------------------------------------------------------------------
    def backward(self, d_main, d_xs):
        """Gradients of the last training forward for output gradients d_main [B, latent_dim_end], d_xs [B, size2*latent_dim]
        (or [B, size2, latent_dim]), written into the gradient arena; returns self.grads."""
        c = self._ctx
        if c is None:
            raise SgvError("backward() needs a preceding forward()")
        self._ctx = None
        B, P, G = c["B"], self.P, self.G
        heads = ("latent_out", "xs_out")
        d_out = [d_main.reshape(B, -1).contiguous(), d_xs.reshape(B, -1).contiguous()]

        def lin_grads(prefix, dz, x, dx=None, y_tanh=None, W=True):
            return dict(dz=dz, y_tanh=y_tanh, x=x, W=P[prefix + ".weight"], dx=dx, dW=G[prefix + ".weight"] if W else None,
                        db=G[prefix + ".bias"] if W else None)

        def ln_sums(prefix, part, gplane=0, bplane=1):
            return [(part[gplane], G[prefix + ".weight"]), (part[bplane], G[prefix + ".bias"])]

        # heads: Tanh output layer (its derivative folded into the GEMM's operand loads), then two Linear -> LN -> GELU -> Dropout
        da2 = [torch.empty_like(a) for a in c["a_h2"]]
        ops.mlp_gemm_bwd([lin_grads(hd + ".8", d_out[k], c["a_h2"][k], da2[k], y_tanh=c["y"][k]) for k, hd in enumerate(heads)], B)
        rb2 = ops.mlp_rows_bwd([dict(r, dout=da2[k]) for k, r in enumerate(c["rows_h2"])], B)
        da1 = [torch.empty_like(a) for a in c["a_h1"]]
        ops.mlp_gemm_bwd([lin_grads(hd + ".4", rb2[k]["dza"], c["a_h1"][k], da1[k]) for k, hd in enumerate(heads)], B,
                         colsums=ln_sums("latent_out.5", rb2[0]["part"]) + ln_sums("xs_out.5", rb2[1]["part"]))
        rb1 = ops.mlp_rows_bwd([dict(r, dout=da1[k]) for k, r in enumerate(c["rows_h1"])], B)
        dfeat = torch.empty_like(c["features"])
        ops.mlp_gemm_bwd([lin_grads(hd + ".0", rb1[k]["dza"], c["features"], dfeat if k == 0 else None) for k, hd in enumerate(heads)], B, dx_sum=True,
                         colsums=ln_sums("latent_out.1", rb1[0]["part"]) + ln_sums("xs_out.1", rb1[1]["part"]))
        dh = dfeat
        pending = []                 # LayerNorm partials whose batch sums ride on the next backward GEMM launch
        if c["fp_row"] is not None:
            rf, = ops.mlp_rows_bwd([dict(c["fp_row"], dout=dh)], B)
            dh = rf["dza"]
            pending += ln_sums("feature_projection.0", rf["part"])
        for i in range(len(c["blocks"]) - 1, 0, -1):
            blk, pre = c["blocks"][i], f"backbone.{i}"
            r2, = ops.mlp_rows_bwd([dict(blk["row2"], dout=dh, need_dr=not blk["skip"])], B)
            part = r2["part"]
            sums = ln_sums(pre + ".ln2", part)
            probs = [lin_grads(pre + ".linear2", r2["dza"], blk["a1"], torch.empty_like(blk["a1"]))]
            if blk["skip"]:
                sums += ln_sums(pre + ".skip_connection.1", part, 2, 1)
                probs.append(lin_grads(pre + ".skip_connection.0", r2["dzb"], blk["x"]))
            if blk["fold_fp"]:
                sums += ln_sums("feature_projection.0", part, 3, 4)
            ops.mlp_gemm_bwd(probs, B, colsums=sums + pending)
            pending = []
            da1 = probs[0]["dx"]
            r1, = ops.mlp_rows_bwd([dict(blk["row1"], dout=da1)], B)
            dx = torch.empty_like(blk["x"])
            probs = [lin_grads(pre + ".linear1", r1["dza"], blk["x"], dx)]
            if blk["skip"]:                 # + the skip Linear's input gradient, summed in the same tiles
                probs.append(dict(dz=r2["dzb"], W=P[pre + ".skip_connection.0.weight"]))
            ops.mlp_gemm_bwd(probs, B, dx_sum=True, dx_addend=None if blk["skip"] else r2["dr"], colsums=ln_sums(pre + ".ln1", r1["part"]))
            dh = dx
        blk = c["blocks"][0]
        r0, = ops.mlp_rows_bwd([dict(blk["row"], dout=dh)], B)
        dxn = torch.empty_like(c["xn"])
        ops.mlp_gemm_bwd([lin_grads("backbone.0.0", r0["dza"], blk["x"], dxn)], B, colsums=ln_sums("backbone.0.1", r0["part"]) + pending)
        rin, = ops.mlp_rows_bwd([dict(c["row_in"], dout=dxn, need_dza=False)], B)
        ops.mlp_gemm_bwd([], B, colsums=ln_sums("input_norm", rin["part"]))
        self.grads = dict(self.G)
        return self.grads

    def loss_backward(self, x, y1, y2, dropout_masks=None, w1=10.0, w2=1.0, preds=None, sync=True):
        """latent_conditioner.py:285-301: forward, A = MSE(y_pred1, y1), B = MSE(y_pred2, y2), loss = w1*A + w2*B, backward.
        Returns (loss, A, B) as floats (sync=False: A and B as device tensors, no host synchronisation)."""
        p1, p2 = preds if preds is not None else self.forward(x, dropout_masks)
        y1 = torch.as_tensor(y1).to(device="cuda", dtype=torch.float32).contiguous()
        y2 = torch.as_tensor(y2).to(device="cuda", dtype=torch.float32).contiguous()
        la, d1 = ops.mse(p1, y1, gscale=float(w1))
        lb, d2 = ops.mse(p2.reshape(p2.shape[0], -1), y2.reshape(y2.shape[0], -1), gscale=float(w2))
        self.backward(d1, d2)
        if not sync:
            return None, la, lb
        A, Bv = float(la), float(lb)
        return float(w1) * A + float(w2) * Bv, A, Bv
