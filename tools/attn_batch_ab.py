"""Same-process A/B of the batched e4m3 attention entry points (include/fairygen_hip_batch8.h) at B = 2, the batch of a merged CFG call.

    python tools/attn_batch_ab.py [--n 8190 27280 --heads 24 --ctx 512 --rounds 12 --iters 2]

Per token count N, ONE process, random data, HIP events on the launch stream, the legs of a chain timed round-robin (leg A, leg B, leg C,
leg A, ..) after a warm-up, so that drift of the clocks hits all legs alike; medians, standard deviations and extremes of
rounds * iters runs per leg.

The self-attention chain, from the (2, N, 3 C) q | k | v buffer to the (2, N, C) attention output:
  bf16         RMSNorm+RoPE of k and q per element (the row kernel's table is indexed by the row: 4 launches), fg_attn_fwd_bf16 with B = 2;
  e4m3 x 2     the fused producers, fg_attn_quant_vt_bf16 and fg_attn_fwd_pv8_bf16, called once per element (what a merged CFG call runs
               today with enable_qk8_attention(fused_producer=True, pv8=True));
  e4m3 batched the same chain through the _b entry points, one launch sequence.
The cross-attention chain over --ctx keys, from the q Linear's (2, N, C) output to the attention output, the context operands ready (they
are made once per denoise loop): bf16 (RMSNorm of q on 2 N rows, fg_attn_fwd_bf16 with B = 2), e4m3 x 2 (fg_rmsnorm_rope_q8_bf16 and
fg_attn_fwd_cross8_bf16 per element), e4m3 batched.  The context quantisation is timed beside it, 2 x single against batched.
Before anything is timed the batched outputs are compared with the per-element ones (torch.equal).
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fairygen_amd import hip  # noqa: E402

BF16, EPS, B = torch.bfloat16, 1e-6, 2


def time_legs(title, legs, rounds, iters):
    names = list(legs)
    for n in names:      # warm-up: allocations of the binding's scratch, hipFuncSetAttribute, clocks
        for _ in range(iters + 1):
            legs[n]()
    torch.cuda.synchronize()
    times = {n: [] for n in names}
    for _ in range(rounds):
        for n in names:
            for _ in range(iters):
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record()
                legs[n]()
                e.record()
                e.synchronize()
                times[n].append(s.elapsed_time(e))
    base = None
    for n in names:
        ts = sorted(times[n])
        med, mean = ts[len(ts) // 2], sum(ts) / len(ts)
        sd = (sum((t - mean) ** 2 for t in ts) / (len(ts) - 1)) ** 0.5
        base = med if base is None else base
        print(f"{title} | {n:13s}: median {med:8.4f} ms, sd {sd:.4f}, min {ts[0]:.4f}, max {ts[-1]:.4f} ({len(ts)} runs; "
              f"{100.0 * (med / base - 1.0):+6.1f} % against {names[0]})", flush=True)


def self_chain(n, heads, rounds, iters):
    dev, c = "cuda", heads * 128
    g = torch.Generator(dev).manual_seed(n)
    qkv = torch.randn((B, n, 3 * c), generator=g, device=dev).to(BF16)
    qkv[1] *= 1.5      # the CFG branches are not the same tensor
    w = torch.ones(c, dtype=BF16, device=dev)
    ang = torch.rand((n, 64), generator=g, device=dev, dtype=torch.float64) * 6.283185307179586
    tab = torch.stack([ang.cos(), ang.sin()], -1).float().contiguous()
    qs, ks, vs = qkv[..., :c], qkv[..., c:2 * c], qkv[..., 2 * c:]
    scale = 128.0 ** -0.5
    qn, kn = torch.empty((B, n, c), dtype=BF16, device=dev), torch.empty((B, n, c), dtype=BF16, device=dev)
    out_a, out_b, out_c = (torch.empty((B, n, c), dtype=BF16, device=dev) for _ in range(3))
    one = [(hip.attention_qk8_fused_scratch(n, heads, 128, dev), hip.attention_pv8_scratch(n, heads, 128, dev)) for _ in range(B)]
    both = (hip.attention_qk8_fused_scratch(n, heads, 128, dev, B), hip.attention_pv8_scratch(n, heads, 128, dev, B))
    ws_bf16, ws_one, ws_both = [], [], []

    def bf16():
        for e in range(B):
            hip.rmsnorm_rope(ks[e:e + 1], w, heads, EPS, tab, None, out=kn[e:e + 1])
            hip.rmsnorm_rope(qs[e:e + 1], w, heads, EPS, tab, None, out=qn[e:e + 1])
        hip.attention(qn, kn, vs, heads, out=out_a, scale=scale, workspace=ws_bf16)

    def chain8(x, bufs, pvb, out, ws):
        q8, k8, sq, sk, kbar, parts = bufs
        k, _ = hip.rmsnorm_rope_kstats(x[..., c:2 * c], w, heads, EPS, tab, None, partials=parts)
        hip.rmsnorm_rope_q8(x[..., :c], w, heads, EPS, tab, None, q8=q8, sq=sq)
        hip.attn_quant_k(k, parts, heads, k8, sk, kbar)
        hip.attention_qk8_pre(q8, k8, sq, sk, x[..., 2 * c:], heads, out=out, scale=scale, workspace=ws, pv8=True, pv8_bufs=pvb)

    def e4m3_x2():
        for e in range(B):
            chain8(qkv[e:e + 1], one[e][0], one[e][1], out_b[e:e + 1], ws_one)

    def e4m3_batched():
        chain8(qkv, both[0], both[1], out_c, ws_both)

    e4m3_x2()
    e4m3_batched()
    torch.cuda.synchronize()
    assert torch.equal(out_b, out_c), "the batched chain must reproduce the per-element bytes"
    time_legs(f"self  N={n} H={heads} B={B}", {"bf16": bf16, "e4m3 x 2": e4m3_x2, "e4m3 batched": e4m3_batched}, rounds, iters)


def cross_chain(n, heads, ctx, rounds, iters):
    dev, c = "cuda", heads * 128
    g = torch.Generator(dev).manual_seed(n + 1)
    qc = torch.randn((B, n, c), generator=g, device=dev).to(BF16)
    kvc = torch.randn((B, ctx, 2 * c), generator=g, device=dev).to(BF16)
    kvc[1] *= 1.5
    w = torch.ones(c, dtype=BF16, device=dev)
    qn = torch.empty((B, n, c), dtype=BF16, device=dev)
    out_a, out_b, out_c = (torch.empty((B, n, c), dtype=BF16, device=dev) for _ in range(3))

    def context(x):
        k, parts = hip.rmsnorm_rope_kstats(x[..., :c], w, heads, EPS)
        k8, sk, _ = hip.attn_quant_k(k, parts, heads)
        v8t, sv, _ = hip.attn_quant_vt(x[..., c:], heads)
        return k8, sk, v8t, sv

    kn = hip.rmsnorm_rope(kvc[..., :c].contiguous(), w, heads, EPS)
    vc = kvc[..., c:]
    ops1 = [context(kvc[e:e + 1]) for e in range(B)]
    opsb = context(kvc)
    q8s = [(torch.empty((n, c), dtype=torch.float8_e4m3fn, device=dev), torch.empty((n, heads), dtype=torch.float32, device=dev)) for _ in range(B)]
    q8b = (torch.empty((B, n, c), dtype=torch.float8_e4m3fn, device=dev), torch.empty((B, n, heads), dtype=torch.float32, device=dev))
    ws = []

    def bf16():
        hip.rmsnorm_rope(qc, w, heads, EPS, out=qn)
        hip.attention(qn, kn, vc, heads, out=out_a, workspace=ws)

    def e4m3_x2():
        for e in range(B):
            q8, sq = hip.rmsnorm_rope_q8(qc[e:e + 1], w, heads, EPS, q8=q8s[e][0], sq=q8s[e][1])
            k8, sk, v8t, sv = ops1[e]
            hip.attention_cross8_pre(q8, k8, sq, sk, v8t, sv, heads, out=out_b[e:e + 1])

    def e4m3_batched():
        q8, sq = hip.rmsnorm_rope_q8(qc, w, heads, EPS, q8=q8b[0], sq=q8b[1])
        hip.attention_cross8_pre(q8, opsb[0], sq, opsb[1], opsb[2], opsb[3], heads, out=out_c)

    e4m3_x2()
    e4m3_batched()
    torch.cuda.synchronize()
    assert torch.equal(out_b, out_c), "the batched chain must reproduce the per-element bytes"
    time_legs(f"cross Nq={n} Nkv={ctx} H={heads} B={B}", {"bf16": bf16, "e4m3 x 2": e4m3_x2, "e4m3 batched": e4m3_batched}, rounds, iters)
    time_legs(f"context quantisation Nkv={ctx} H={heads} B={B}",
              {"e4m3 x 2": lambda: [context(kvc[e:e + 1]) for e in range(B)], "e4m3 batched": lambda: context(kvc)}, rounds, iters)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, nargs="+", default=[8190, 27280])
    ap.add_argument("--heads", type=int, default=24)
    ap.add_argument("--ctx", type=int, default=512)
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--iters", type=int, default=2)
    a = ap.parse_args()
    props = torch.cuda.get_device_properties(0)
    print(f"device: {props.name}, {props.multi_processor_count} CUs; torch {torch.__version__}; B = {B}, {a.rounds} rounds x {a.iters} "
          f"runs per leg, legs interleaved", flush=True)
    for n in a.n:
        self_chain(n, a.heads, a.rounds, a.iters)
        cross_chain(n, a.heads, a.ctx, a.rounds, a.iters)


if __name__ == "__main__":
    main()
