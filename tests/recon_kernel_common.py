"""What the kernel tests of the recon tails (csrc/recon_out.hip) share: tests/test_generate_kernel_gpu.py, test_summary_kernel_gpu.py,
test_score_kernel_gpu.py and test_ensemble_kernel_gpu.py build their inputs, their canary-framed buffers and the stored field F, the
reference of the three reducing passes, with the helpers below.  Groups follow the model's rule G = min(8, max(1, C // 4))."""
import numpy as np

from simulgen_vae_amd import engine as E

ELT32 = 2e-5        # tests/test_ew_kernels_gpu.py
CANARY = 768.0
ICANARY = -777
MARGIN = 64         # elements of canary in front of and behind every buffer (keeps it 16-byte aligned)


def _groups(Cn):
    return min(8, max(1, Cn // 4))


def _bf16(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(torch.bfloat16).to(torch.float32).numpy()


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def base_inputs(B, T, Cn, dtype, signed=True):
    """y [B, T, C], gamma, beta, scale, mn as fp32 (y not yet rounded to bf16): gamma spread enough that tanh saturates somewhere, scale of
    mixed magnitudes in [1e-3, 50], min of both signs; signed: a quarter of the scales negative (scaler_vectors admits that)"""
    rng = np.random.default_rng(1000 * Cn + 10 * T + B + dtype)
    y = (rng.standard_normal((B, T, Cn)) * 2 + 0.5).astype(np.float32)
    gamma = (1.6 + 0.4 * rng.standard_normal(Cn)).astype(np.float32)
    beta = (0.3 * rng.standard_normal(Cn)).astype(np.float32)
    scale = np.exp(rng.uniform(np.log(1e-3), np.log(50.0), Cn)).astype(np.float32)
    mn = (rng.standard_normal(Cn) * np.where(rng.random(Cn) < 0.5, 1.0, 30.0)).astype(np.float32)
    if signed:
        scale = np.where(rng.random(Cn) < 0.25, -scale, scale).astype(np.float32)
    return dict(y=y, gamma=gamma, beta=beta, scale=scale, mn=mn)


def canary_buffers(sizes, integer=()):
    """name -> (whole buffer with canary margins, the view of sizes[name] elements between them); int32 for the names in `integer`"""
    import torch
    bufs = {}
    for name, n in sizes.items():
        i = name in integer
        buf = torch.full((n + 2 * MARGIN,), ICANARY if i else CANARY, dtype=torch.int32 if i else torch.float32, device="cuda")
        bufs[name] = (buf, buf[MARGIN:MARGIN + n])
        assert bufs[name][1].data_ptr() % 16 == 0
    return bufs


def margins_intact(bufs):
    return all(bool((b[:MARGIN] == b[0]).all()) and bool((b[-MARGIN:] == b[0]).all()) and float(b[0]) in (CANARY, ICANARY) for b, _ in bufs.values())


def device_inputs(c, y, ldy, dtype):
    """y [b, T, C]: the samples of this launch, in a map with canary padding columns; the statistics buffer starts as NaN"""
    import torch
    b, T, Cn = y.shape
    ymap = torch.full((b * T, ldy), CANARY, dtype=torch.bfloat16 if dtype == 1 else torch.float32, device="cuda")
    ymap[:, :Cn] = torch.from_numpy(np.array(y).reshape(b * T, Cn)).cuda().to(ymap.dtype)
    f = lambda a: torch.from_numpy(np.array(a)).cuda()
    sums = torch.full((b * _groups(Cn) * 2,), float("nan"), dtype=torch.float64, device="cuda")
    return dict(y=ymap, gamma=f(c["gamma"]), beta=f(c["beta"]), scale=f(c["scale"]), mn=f(c["mn"]), sums=sums)


def hook_inputs(d, ldy):
    """the leading arguments of every sgv_test_recon_* hook after dtype"""
    return (d["y"].data_ptr(), ldy, d["sums"].data_ptr(), d["gamma"].data_ptr(), d["beta"].data_ptr(), d["scale"].data_ptr(), d["mn"].data_ptr())


def padding_intact(d, Cn):
    return bool((d["y"][:, Cn:].float() == CANARY).all())


def field(c, y, ldy, dtype):
    """F: the output pass (sgv_test_recon_physical, layout [B][T][N]) on the same inputs, [b, T, C] fp32"""
    import torch
    lib = E.load_library()
    b, T, Cn = y.shape
    d = device_inputs(c, y, ldy, dtype)
    out = torch.full((b * T * Cn,), float("nan"), dtype=torch.float32, device="cuda")
    rc = lib.sgv_test_recon_physical(dtype, *hook_inputs(d, ldy), 0, out.data_ptr(), b, T, Cn, None)
    assert rc == 0, lib.sgv_last_error().decode()
    return out.cpu().numpy().reshape(b, T, Cn)
