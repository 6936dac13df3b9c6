"""Decode attention: one workgroup per head against the split-context kernel and against the split-context kernel on the e4m3 KV cache
(lhrs_decode_attn_kv8), us per launch at the contexts the bench walks.
   python tools/decode_attn_ab.py [BATCH [CTX,CTX,...]]        e.g.  python tools/decode_attn_ab.py 8 127,255,511,1023"""
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from lhrs_bot_amd import kernels as hk
from oracle.lhrs_oracle import rope_tables

dev = "cuda"
B = int(sys.argv[1]) if len(sys.argv) > 1 else 1
ctxs = tuple(int(c) for c in sys.argv[2].split(",")) if len(sys.argv) > 2 else (203, 330, 459, 587, 714)
H, D, max_ctx = 32, 128, max(715, max(ctxs) + 1)
d = H * D
cos, sin = (t.to(dev) for t in rope_tables(max_ctx, D))
caches = [(torch.randn(B * max_ctx, d, device=dev).bfloat16(), torch.randn(B * max_ctx, d, device=dev).bfloat16()) for _ in range(32)]   # 32 layers: no L2 reuse between launches
caches8 = []
for kc, vc in caches:   # the same rows in the kv8 format
    c8 = tuple(torch.empty((B * max_ctx, n), device=dev, dtype=torch.uint8) for n in (d, d, H, H))
    hk.kv8_quant_rows(kc, c8[0], c8[2], 0, H)
    hk.kv8_quant_rows(vc, c8[1], c8[3], 0, H)
    caches8.append(c8)
qkv = torch.randn(B, 3 * d, device=dev).bfloat16()
o = torch.empty(B, d, device=dev, dtype=torch.bfloat16)


def timeit(fn, n=5):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / (n * 32)


print(f"batch {B}, {H} heads, us per launch (mean over 32 layers' caches x 5); kv8 = the e4m3 cache at the same split")
for ctx in ctxs:
    pos = torch.full((B,), ctx, dtype=torch.int32, device=dev)
    row = [f"ctx {ctx:4d}: one WG/head {timeit(lambda: [hk.decode_attn(qkv, kc, vc, cos, sin, pos, o, B, H, D, max_ctx, 1 / math.sqrt(D)) for kc, vc in caches]):6.2f} us"]
    for ns in (3, 6, 8, 12):
        part = torch.zeros(B, H, ns, 132, device=dev)
        tk = torch.zeros(B, H, device=dev, dtype=torch.int32)
        t = timeit(lambda: [hk.decode_attn_split(qkv, kc, vc, cos, sin, pos, o, B, H, D, max_ctx, 1 / math.sqrt(D), ns, part, tk) for kc, vc in caches])
        t8 = timeit(lambda: [hk.decode_attn_kv8(qkv, *c8, cos, sin, pos, o, B, H, D, max_ctx, 1 / math.sqrt(D), ns, part, tk) for c8 in caches8])
        row.append(f"split {ns:2d}: {t:6.2f} kv8 {t8:6.2f}")
    print(" | ".join(row))
