"""The float64 formulas the decoder-block ops are tested against (inputs are upcast first)."""
import torch


def add_rms_norm(z, res, w, eps):
    v = z.double() if res is None else res.double() + z.double()
    return v / torch.sqrt((v * v).mean(-1, keepdim=True) + eps) * w.double(), v


def swiglu(x):
    g, u = x.double().chunk(2, -1)
    return g / (1 + torch.exp(-g)) * u


def rotary(qkv, kv_heads, cos, sin, pos=None):
    b, s, heads, _ = qkv.shape
    pos = torch.arange(s, device=qkv.device).expand(b, s) if pos is None else pos.long()
    out = qkv.double().clone()
    c, sn = cos.double()[pos][:, :, None], sin.double()[pos][:, :, None]
    x = qkv.double()[:, :, :heads - kv_heads]
    out[:, :, :heads - kv_heads, :64] = x[..., :64] * c - x[..., 64:] * sn
    out[:, :, :heads - kv_heads, 64:] = x[..., 64:] * c + x[..., :64] * sn
    return out
