"""The plain float64 formula of one-token attention against a KV cache (ops.attention, "Decoding").
A helper module, not a test file: tests/test_attn_decode_gpu.py and tests/test_llama_decode_cpu.py
import it."""
import math

import torch


def reference(q, kv_cache, kv_heads, lens):
    """q [b, hq, d], kv_cache [b, S_max, 2 kv_heads, d], lens [b] -> (out [b, hq, d], lse [b, hq]
    in the log2 domain of the scaled scores), float64 on the CPU.  lens == 0: out = 0, lse = -inf."""
    q, kv_cache = q.detach().double().cpu(), kv_cache.detach().double().cpu()
    b, hq, d = q.shape
    G = hq // kv_heads
    out = torch.zeros(b, hq, d, dtype=torch.float64)
    lse = torch.full((b, hq), -math.inf, dtype=torch.float64)
    for i, n in enumerate(int(x) for x in lens):
        if n == 0:
            continue
        k, v = kv_cache[i, :n].split(kv_heads, dim=1)                    # [n, kv_heads, d]
        s = torch.einsum("hd,nhd->hn", q[i], k.repeat_interleave(G, 1)) / math.sqrt(d)
        lse[i] = torch.logsumexp(s, -1) / math.log(2.0)
        out[i] = torch.einsum("hn,nhd->hd", torch.softmax(s, -1), v.repeat_interleave(G, 1))
    return out, lse
