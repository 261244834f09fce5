"""An independent PyTorch restatement of the parametric (CSV) latent conditioner, written from its description (input
LayerNorm; Linear -> LayerNorm -> GELU -> Dropout; ResidualBlocks linear1 -> ln1 -> GELU -> dropout -> linear2 -> ln2 plus a
Linear + LayerNorm skip when the width changes, summed, GELU; feature_projection LayerNorm + Dropout; two heads
Linear -> LN -> GELU -> Dropout twice, then Linear -> Tanh).  Parameter names match the model's state_dict, so a state
loads into both.  Used as the float64 CPU comparator of the dense-layer operator tests and as the PyTorch-eager baseline
of tests/micro/mlp_lc_bench.py; it is not the model under test."""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F


def sample_positions(name, numel, n=256):
    """Positions at which the fixtures record the entries of a large tensor (name-seeded, the same on every box)."""
    seed = int.from_bytes(name.encode()[-8:].rjust(8, b"\0"), "little") % (2 ** 31)
    rng = np.random.Generator(np.random.Philox(key=[978, seed]))
    return rng.integers(0, numel, size=min(n, numel))


def head_width(latent_dim_end, f_last, input_shape):
    return max(2 * latent_dim_end, f_last // min(8, max(2, input_shape // 64)))


class Block(nn.Module):
    def __init__(self, cin, cout, p):
        super().__init__()
        self.linear1, self.ln1 = nn.Linear(cin, cout), nn.LayerNorm(cout)
        self.linear2, self.ln2 = nn.Linear(cout, cout), nn.LayerNorm(cout)
        self.dropout = nn.Dropout(p)
        self.skip_connection = nn.Sequential(nn.Linear(cin, cout), nn.LayerNorm(cout)) if cin != cout else None

    def forward(self, x):
        h = self.ln2(self.linear2(self.dropout(F.gelu(self.ln1(self.linear1(x))))))
        return F.gelu(h + (self.skip_connection(x) if self.skip_connection is not None else x))


def _head(f, h, out, p):
    return nn.Sequential(nn.Linear(f, h), nn.LayerNorm(h), nn.GELU(), nn.Dropout(p * 0.6),
                         nn.Linear(h, h // 2), nn.LayerNorm(h // 2), nn.GELU(), nn.Dropout(p * 0.4),
                         nn.Linear(h // 2, out), nn.Tanh())


class TorchMLPConditioner(nn.Module):
    def __init__(self, filters, latent_dim_end, input_shape, latent_dim, size2, dropout_rate=0.3):
        super().__init__()
        self.size2, self.latent_dim = size2, latent_dim
        p = dropout_rate
        sched = [p * 0.5, p * 0.7, p, p * 1.2]
        self.input_norm = nn.LayerNorm(input_shape)
        self.backbone = nn.ModuleList()
        cur = input_shape
        for i, f in enumerate(filters):
            if i == 0:
                self.backbone.append(nn.Sequential(nn.Linear(cur, f), nn.LayerNorm(f), nn.GELU(), nn.Dropout(sched[0])))
            else:
                self.backbone.append(Block(cur, f, sched[min(i, 3)]))
            cur = f
        h = head_width(latent_dim_end, cur, input_shape)
        self.feature_projection = nn.Sequential(nn.LayerNorm(cur), nn.Dropout(p * 0.8))
        self.latent_out = _head(cur, h, latent_dim_end, p)
        self.xs_out = _head(cur, h, latent_dim * size2, p)

    def forward(self, x):
        x = self.input_norm(x)
        for layer in self.backbone:
            x = layer(x)
        f = self.feature_projection(x)
        return self.latent_out(f), self.xs_out(f).view(x.shape[0], self.size2, self.latent_dim)


def dense_reference(x, W, b, g, beta, mask=None, p=0.0, tanh=False, gelu=True, skip=None, resid=None, post=None):
    """One fused dense layer on the CPU (any dtype): z = x W^T + b; y = LN(z) * g + beta [+ LN(x Ws^T + bs) * gs + betas
    | + resid], GELU, [LN(y) * gc + bc], then mask / (1 - p); with tanh: tanh(z) (the head's last layer)."""
    z = x @ W.t() + b
    if tanh:
        return torch.tanh(z)
    y = F.layer_norm(z, (z.shape[1],), g, beta, 1e-5)
    if skip is not None:
        xs, Ws, bs, gs, betas = skip
        y = y + F.layer_norm(xs @ Ws.t() + bs, (Ws.shape[0],), gs, betas, 1e-5)
    if resid is not None:
        y = y + resid
    if gelu:
        y = F.gelu(y)
    if post is not None:
        y = F.layer_norm(y, (y.shape[1],), post[0], post[1], 1e-5)
    if mask is not None:
        y = y * mask / (1.0 - p)
    return y
