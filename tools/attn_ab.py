"""A/B of fg_attn_fwd_bf16 builds in ONE process (interleaved rounds, random data, HIP events on the launch stream).

    python tools/attn_ab.py --libs base=fairygen_amd/libfairygen_hip.so,new=fairygen_amd/csrc/build/ab/libfg_new.so \
        [--nq 27280 --nkv 27280 --heads 24 --rounds 8 --check-rows 192]

Every library is checked first against an fp32 reference (sampled query rows x all keys, every head) with the criterion of
tests/test_hip_kernels.py (max|out - ref_f32| against the bf16 rounding of the reference), then timed round-robin.
"""
import argparse
import ctypes
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fairygen_amd import hip  # noqa: E402

_i64, _i32, _f32, _vp = ctypes.c_int64, ctypes.c_int, ctypes.c_float, ctypes.c_void_p


def load(path):
    lib = ctypes.CDLL(os.path.abspath(path))
    lib.fg_attn_fwd_bf16.restype = ctypes.c_int
    lib.fg_attn_fwd_bf16.argtypes = hip._SIGNATURES["fg_attn_fwd_bf16"]
    lib.fg_attn_workspace_bytes.restype = _i64
    lib.fg_attn_workspace_bytes.argtypes = [_i32, _i64, _i64, _i32]
    lib.fg_last_error.restype = ctypes.c_char_p
    return lib


def runner(lib, q, k, v, heads, out):
    b, nq, hd = q.shape
    nkv = k.shape[1]
    need = lib.fg_attn_workspace_bytes(b, nq, nkv, heads)
    ws = torch.empty(max(need, 16), dtype=torch.uint8, device=q.device)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def fn():
        rc = lib.fg_attn_fwd_bf16(q.data_ptr(), q.stride(1), k.data_ptr(), k.stride(1), v.data_ptr(), v.stride(1), out.data_ptr(),
                                  b, nq, nkv, heads, hd // heads, float(hd // heads) ** -0.5, ws.data_ptr() if need else None, need, stream)
        if rc:
            raise RuntimeError(lib.fg_last_error().decode())
    return fn


def shard8(a):
    """--shard8: one rank's attention chain of the K / V all-gather layout, from its rows of the q | k | v buffer to its attention output, at
    nq = ceil(nkv / world) local rows against nkv keys: 'chain-bf16' (RMSNorm+RoPE x 2, gather of k and v, fg_attn_fwd_bf16), 'chain-qk8-sharded'
    and 'chain-pv8-sharded' (enable_qk8_attention(sharded=True): key statistics, record, e4m3 q, quantise, gather of the e4m3 bytes, the
    transpose pass, the e4m3 attention) and 'chain-pv8s-sharded' (sharded="all" with smooth_v: the 32 C byte record, v8 of v - mu, the
    attention that adds mu back).  ONE process, ONE GPU: local copies of the same size stand in for the collectives, so nothing here
    says anything about xGMI.  Then the HBM-bound passes alone with their achieved GB/s, beside fg_attn_quant_vt_bf16 on the same rows."""
    dev, heads, n = "cuda", a.heads, a.nkv
    c, nl = heads * 128, -(-a.nkv // a.world)
    g = torch.Generator(dev).manual_seed(0)
    qkv = torch.randn((1, nl, 3 * c), generator=g, device=dev).to(torch.bfloat16)
    w = torch.ones(c, dtype=torch.bfloat16, device=dev)
    ang = torch.rand((nl, 64), generator=g, device=dev, dtype=torch.float64) * 6.283
    tab = torch.stack([ang.cos(), ang.sin()], -1).float().contiguous()
    qs, ks, vs = qkv[..., :c], qkv[..., c:2 * c], qkv[..., 2 * c:]
    out = torch.empty((1, nl, c), dtype=torch.bfloat16, device=dev)

    def gather(local):      # every "peer" contributes a copy of the local rows
        return local.reshape(1, nl, -1).expand(a.world, nl, -1).reshape(a.world * nl, -1)[:n]

    def chain_bf16():
        k = hip.rmsnorm_rope(ks, w, heads, 1e-6, tab)
        q = hip.rmsnorm_rope(qs, w, heads, 1e-6, tab)
        hip.attention(q, gather(k[0]).unsqueeze(0), gather(vs[0]).unsqueeze(0), heads, out=out)

    def chain_8(pv8):
        v = vs if pv8 else None
        k, parts = hip.rmsnorm_rope_kstats(ks, w, heads, 1e-6, tab)
        rec = hip.attn_shard8_stats(parts, nl, heads, v)
        q8, sq = hip.rmsnorm_rope_q8(qs, w, heads, 1e-6, tab)
        k8, v8, sk, _, sv = hip.attn_shard8_quant(rec.view(1, -1).repeat(a.world, 1), n, k, heads, v)
        k8f = gather(k8.view(torch.uint8)).view(torch.float8_e4m3fn)
        if pv8:
            hip.attention_pv8_pre(q8, k8f, sq, sk, hip.attn_shard8_vt(gather(v8.view(torch.uint8)), heads), sv, heads, out=out)
        else:
            hip.attention_qk8_pre(q8, k8f, sq, sk, gather(vs[0]).unsqueeze(0), heads, out=out)

    def chain_8s():
        k, parts = hip.rmsnorm_rope_kstats(ks, w, heads, 1e-6, tab)
        rec = hip.attn_shard8s_stats(parts, nl, heads, vs)
        q8, sq = hip.rmsnorm_rope_q8(qs, w, heads, 1e-6, tab)
        k8, v8, sk, _, sv, mu = hip.attn_shard8s_quant(rec.view(1, -1).repeat(a.world, 1), n, k, heads, vs)
        k8f = gather(k8.view(torch.uint8)).view(torch.float8_e4m3fn)
        hip.attention_pv8_pre(q8, k8f, sq, sk, hip.attn_shard8_vt(gather(v8.view(torch.uint8)), heads), sv, heads, out=out, mu=mu)

    k, parts = hip.rmsnorm_rope_kstats(ks, w, heads, 1e-6, tab)
    rec = hip.attn_shard8_stats(parts, nl, heads, vs).view(1, -1).repeat(a.world, 1)
    rec_s = hip.attn_shard8s_stats(parts, nl, heads, vs).view(1, -1).repeat(a.world, 1)
    v8_full = torch.empty((n, c), dtype=torch.uint8, device=dev).random_(0, 120)
    vt_bufs = hip.attention_pv8_scratch(nl, heads, 128, dev)
    mb = nl * c / 1e6
    fns = [("chain-bf16", chain_bf16, None), ("chain-qk8-sharded", lambda: chain_8(False), None), ("chain-pv8-sharded", lambda: chain_8(True), None),
           ("chain-pv8s-sharded", chain_8s, None),
           ("shard8-stats (v)", lambda: hip.attn_shard8_stats(parts, nl, heads, vs), 2 * mb),
           ("shard8s-stats (v)", lambda: hip.attn_shard8s_stats(parts, nl, heads, vs), 2 * mb),
           ("shard8-quant (k, v)", lambda: hip.attn_shard8_quant(rec, n, k, heads, vs), 6 * mb),
           ("shard8s-quant (k, v)", lambda: hip.attn_shard8s_quant(rec_s, n, k, heads, vs), 6 * mb),
           ("shard8-vt", lambda: hip.attn_shard8_vt(v8_full, heads), 2 * n * c / 1e6),
           ("quant-vt (same rows)", lambda: hip.attn_quant_vt(vs, heads, vt_bufs), 5 * mb)]
    times = {name: [] for name, _, _ in fns}
    for _ in range(a.rounds):
        for name, fn, _ in fns:
            for _ in range(a.iters):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                torch.cuda.synchronize()
                times[name].append(e0.elapsed_time(e1))
    print(f"one rank of {a.world}: nq = {nl}, nkv = {n}, {heads} heads; medians of {a.rounds * a.iters} launches after {a.iters} warm-up; "
          "local copies stand in for the collectives (no xGMI figure)")
    for name, _, mbytes in fns:
        t = sorted(times[name][a.iters:])
        med, sd = t[len(t) // 2], torch.tensor(t).std().item()
        print(f"{name:24s} {med:8.3f} ms  (sd {sd:.3f})" + (f"   {mbytes / med:7.0f} GB/s ({mbytes:.1f} MB read + written)" if mbytes else ""), flush=True)


def padded_context_v(l_text, l=512, heads=24, seed=180, device="cuda"):
    """V of a text context as the pipeline leaves it (the context rows behind the prompt are zeroed and the v Linear acts row by row):
    l_text rows ~ N(0, 1), the other l - l_text rows ONE common row ~ 4 N(0, 1) per channel.  (l, heads * 128) bf16; the generator of
    tests/test_attention_cross8s.py."""
    c = heads * 128
    rows = torch.randn((l_text, c), generator=torch.Generator("cpu").manual_seed(seed), dtype=torch.float32).to(torch.bfloat16)
    pad = (4.0 * torch.randn((1, c), generator=torch.Generator("cpu").manual_seed(seed + 1), dtype=torch.float32)).to(torch.bfloat16)
    return torch.cat([rows, pad.expand(l - l_text, c)], dim=0).contiguous().to(device)


def cross8(a):
    """--cross8: cross-attention from the q Linear's output to the attention output, 24 heads over a context of --nkv rows (512), in ONE
    process with alternating launches, at every --cross8-nq: (a) 'chain-bf16' = rmsnorm_rope + fg_attn_fwd_bf16, (b) 'chain-pv8' = the q8
    producer (fg_rmsnorm_rope_q8_bf16 without a table) + fg_attn_fwd_pv8_bf16, (c) 'chain-cross8' = the q8 producer + fg_attn_fwd_cross8_bf16
    (K8 and V8^T resident in LDS); the three attention launches alone ('attn-*'); and 'quant-context' = the quantisation of a block's
    context (key norm with statistics, fg_attn_quant_k_bf16, fg_attn_quant_vt_bf16), paid once per denoise loop and timed on its own.
    (b) and (c) are first checked to be the same bytes.
    --smooth-v-cross adds a third e4m3 leg on a context whose V is padded_context_v(--l-text, nkv): (d) 'chain-cross8s' = the q8 producer +
    fg_attn_fwd_cross8s_bf16 on the operands of the smoothing V producer (include/fairygen_hip_cross8s.h), 'attn-cross8s' and
    'quant-context-s' (fg_attn_quant_vt_smooth_bf16 in place of fg_attn_quant_vt_bf16); (d) is checked against fg_attn_fwd_pv8s_bf16."""
    dev, heads, nkv = "cuda", a.heads, a.nkv
    c = heads * 128
    g = torch.Generator(dev).manual_seed(0)
    rnd = lambda *s: torch.randn(s, generator=g, device=dev, dtype=torch.float32).to(torch.bfloat16)  # noqa: E731
    wq, wk = (1 + 0.1 * rnd(c).float()).to(torch.bfloat16), (1 + 0.1 * rnd(c).float()).to(torch.bfloat16)
    kvc = rnd(1, nkv, 2 * c)
    if a.smooth_v_cross:
        kvc[0, :, c:] = padded_context_v(min(a.l_text, nkv), nkv, heads, device=dev)

    def quant_context_s():
        k, parts = hip.rmsnorm_rope_kstats(kvc[..., :c], wk, heads, 1e-6)
        k8, sk, _ = hip.attn_quant_k(k, parts, heads)
        v8t, sv, _, mu = hip.attn_quant_vt(kvc[..., c:], heads, smooth=True)
        return k8, sk, v8t, sv, mu

    def quant_context():
        k, parts = hip.rmsnorm_rope_kstats(kvc[..., :c], wk, heads, 1e-6)
        k8, sk, _ = hip.attn_quant_k(k, parts, heads)
        v8t, sv, _ = hip.attn_quant_vt(kvc[..., c:], heads)
        return k8, sk, v8t, sv
    k8, sk, v8t, sv = quant_context()
    k16, v16 = hip.rmsnorm_rope(kvc[..., :c], wk, heads, 1e-6), kvc[..., c:]
    ops_s = quant_context_s() if a.smooth_v_cross else None
    for nq in (int(x) for x in a.cross8_nq.split(",")):
        x = rnd(1, nq, c)
        q16, o16, o8, oc = (torch.empty((1, nq, c), dtype=torch.bfloat16, device=dev) for _ in range(4))
        q8, sq = torch.empty((nq, c), dtype=torch.float8_e4m3fn, device=dev), torch.empty((nq, heads), dtype=torch.float32, device=dev)
        ws16, ws8 = [], []

        def prod16():
            hip.rmsnorm_rope(x, wq, heads, 1e-6, out=q16)

        def prod8():
            hip.rmsnorm_rope_q8(x, wq, heads, 1e-6, q8=q8, sq=sq)

        def attn16():
            hip.attention(q16, k16, v16, heads, out=o16, workspace=ws16)

        def attn8():
            hip.attention_pv8_pre(q8, k8, sq, sk, v8t, sv, heads, out=o8, workspace=ws8)

        def attnc():
            hip.attention_cross8_pre(q8, k8, sq, sk, v8t, sv, heads, out=oc)
        fns = [("chain-bf16", lambda: (prod16(), attn16())), ("chain-pv8", lambda: (prod8(), attn8())), ("chain-cross8", lambda: (prod8(), attnc())),
               ("attn-bf16", attn16), ("attn-pv8", attn8), ("attn-cross8", attnc), ("quant-context", quant_context)]
        if a.smooth_v_cross:
            os_ = torch.empty_like(oc)

            def attns():
                hip.attention_cross8_pre(q8, ops_s[0], sq, ops_s[1], ops_s[2], ops_s[3], heads, out=os_, mu=ops_s[4])
            fns += [("chain-cross8s", lambda: (prod8(), attns())), ("attn-cross8s", attns), ("quant-context-s", quant_context_s)]
        for _, fn in fns:
            for _ in range(2):
                fn()
        torch.cuda.synchronize()
        if a.smooth_v_cross:
            same = torch.equal(os_, hip.attention_pv8_pre(q8, ops_s[0], sq, ops_s[1], ops_s[2], ops_s[3], heads, workspace=None, mu=ops_s[4]))
            e_s, e_c = (os_.float() - o16.float()).abs().mean().item(), (oc.float() - o16.float()).abs().mean().item()
            print(f"check nq={nq}: fg_attn_fwd_cross8s_bf16 and fg_attn_fwd_pv8s_bf16 {'are the same bytes  OK' if same else 'DIFFER  FAIL'}; padded "
                  f"context (L_text {min(a.l_text, nkv)} of {nkv}): mean |out - bf16 chain| cross8 {e_c:.6f}, cross8s {e_s:.6f}", flush=True)
        err = (oc.float() - o16.float()).abs()
        print(f"check nq={nq}: fg_attn_fwd_cross8_bf16 and fg_attn_fwd_pv8_bf16 {'are the same bytes  OK' if torch.equal(oc, o8) else 'DIFFER  FAIL'}; "
              f"against the bf16 chain max {err.max().item():.5f}, mean {err.mean().item():.6f}", flush=True)
        times = {n: [] for n, _ in fns}
        for _ in range(a.rounds):
            for n, fn in fns:
                evs = []
                for _ in range(a.iters):
                    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    s.record(); fn(); e.record()
                    evs.append((s, e))
                torch.cuda.synchronize()
                times[n] += [s.elapsed_time(e) for s, e in evs]
        fl = 4.0 * nq * nkv * c
        for n, ts in times.items():
            ts = sorted(ts)
            mean = sum(ts) / len(ts)
            sd = (sum((t - mean) ** 2 for t in ts) / max(len(ts) - 1, 1)) ** 0.5
            rate = f" = {fl / ts[len(ts) // 2] / 1e9:.0f} TFLOP/s" if n.startswith("attn-") else ""
            print(f"{n}: nq={nq} nkv={nkv} H={heads}: median {ts[len(ts) // 2]:.4f} ms{rate}, mean {mean:.4f}, sd {sd:.4f}, min {ts[0]:.4f}, max {ts[-1]:.4f} "
                  f"({len(ts)} runs)", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cross8", action="store_true", help="time cross-attention over --nkv context rows (use --nkv 512) from the q Linear's output "
                    "to the attention output: bf16, the e4m3 kernel of self-attention, and the kernel that keeps K8 / V8^T in LDS; nothing else runs")
    ap.add_argument("--cross8-nq", default="27280,8190")
    ap.add_argument("--smooth-v-cross", action="store_true", help="with --cross8: V of the context is padded_context_v(--l-text, nkv), and a third "
                    "e4m3 leg runs in the same rounds: 'chain-cross8s' / 'attn-cross8s' = fg_attn_fwd_cross8s_bf16 on mean-smoothed V "
                    "(include/fairygen_hip_cross8s.h), 'quant-context-s' = the context quantisation with the smoothing V producer")
    ap.add_argument("--l-text", type=int, default=40, help="with --smooth-v-cross: the context rows that are text; the others are one common row")
    ap.add_argument("--shard8", action="store_true", help="time one rank's attention chain of the K / V all-gather layout (--world ranks, nkv keys "
                    "in all) for bf16, qk8-sharded and pv8-sharded, and the new passes alone; nothing else runs")
    ap.add_argument("--world", type=int, default=8)
    ap.add_argument("--libs", default="base=" + hip.library_path())
    ap.add_argument("--nq", type=int, default=27280)
    ap.add_argument("--nkv", type=int, default=27280)
    ap.add_argument("--heads", type=int, default=24)
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--iters", type=int, default=3, help="launches per library per round")
    ap.add_argument("--check-rows", type=int, default=192)
    ap.add_argument("--stamp", default="", help="comma list of libraries built with gen_attn_w4.py --stamp: decode their cycle stamps")
    ap.add_argument("--spike", action="store_true", help="also check an input that forces the deferred-rescale branch")
    ap.add_argument("--qk8", action="store_true", help="also time the e4m3 Q K^T form of the package's own library in the same rounds: "
                    "'qk8' = fg_attn_quant_qk_bf16 + fg_attn_fwd_qk8_bf16, 'qk8-attn' = the attention launch alone (nq == nkv)")
    ap.add_argument("--pv8", action="store_true", help="implies --qk8; also time, in the same rounds, the form with the P V product in e4m3 too: "
                    "'pv8' = fg_attn_quant_qk_bf16 + fg_attn_quant_vt_bf16 + fg_attn_fwd_pv8_bf16, 'pv8-attn' = the attention launch alone, "
                    "and the quantise passes alone: 'quant-qk', 'quant-vt' (nq == nkv)")
    ap.add_argument("--smooth-v", action="store_true", help="with --pv8: also time, in the same rounds, the form with V mean-smoothed "
                    "(include/fairygen_hip_smoothv.h): 'pv8s' = fg_attn_quant_qk_bf16 + fg_attn_quant_vt_smooth_bf16 + fg_attn_fwd_pv8s_bf16, "
                    "'pv8s-attn' = the attention launch alone, 'quant-vts' = its V producer alone; every leg is then reported with its standard "
                    "deviation")
    ap.add_argument("--qk8-fused", action="store_true", help="time the whole chain from the q | k | v buffer of the qkv GEMM to the attention "
                    "output (nq == nkv), in three forms: 'chain-bf16' = RMSNorm+RoPE of q and k + fg_attn_fwd_bf16 (the default path, its "
                    "pre-multiplied form), 'chain-qk8' = the same two norms + fg_attn_quant_qk_bf16 + fg_attn_fwd_qk8_bf16, 'chain-qk8-fused' = "
                    "the fused producers (fg_rmsnorm_rope_kstats_bf16, fg_rmsnorm_rope_q8_bf16, fg_attn_quant_k_bf16) + fg_attn_fwd_qk8_bf16; "
                    "and the producers of each form alone ('prod-*').  The two e4m3 chains are first checked to be the same bytes")
    a = ap.parse_args()
    if a.shard8:
        return shard8(a)
    if a.cross8 or a.smooth_v_cross:
        return cross8(a)
    a.pv8 = a.pv8 or a.smooth_v
    a.qk8 = a.qk8 or a.pv8
    dev = "cuda"
    g = torch.Generator(dev).manual_seed(0)
    c = a.heads * 128
    rnd = lambda *s: torch.randn(s, generator=g, device=dev, dtype=torch.float32).to(torch.bfloat16)  # noqa: E731
    q, k, v = rnd(1, a.nq, c), rnd(1, a.nkv, c), rnd(1, a.nkv, c)
    libs = [(n, load(p)) for n, p in (item.split("=", 1) for item in a.libs.split(","))]
    rows = torch.randperm(a.nq, generator=g, device=dev)[: a.check_rows].sort().values
    rows = torch.cat([rows, torch.tensor([0, a.nq - 1], device=dev)]).unique()

    def reference(q, k, v):
        qs = q[0, rows].view(-1, a.heads, 128).float().transpose(0, 1)             # (H, R, 128)
        kk = k[0].view(-1, a.heads, 128).float().permute(1, 2, 0)                  # (H, 128, N)
        p = torch.softmax(torch.bmm(qs, kk) * 128 ** -0.5, dim=-1)
        return torch.bmm(p, v[0].view(-1, a.heads, 128).float().transpose(0, 1)).transpose(0, 1).reshape(-1, c)

    cases = [("random", q, k, v)]
    if a.spike:      # one key row aligned with a few query rows at growing magnitude: the running max jumps past the defer threshold
        k2 = k.clone()
        for i, pos in enumerate((a.nkv // 3, a.nkv // 2, a.nkv - 5)):
            k2[0, pos] = (q[0, rows[i % len(rows)]].float() * (1.5 + i)).to(torch.bfloat16)
        cases.append(("spiked", q, k2, v))
    for cname, cq, ck, cv in cases:
        ref = reference(cq, ck, cv)
        ref_bf = ref.to(torch.bfloat16).float()
        err_ref = (ref_bf - ref).abs().max().item()
        for name, lib in libs:
            out = torch.zeros((1, a.nq, c), dtype=torch.bfloat16, device=dev)
            runner(lib, cq, ck, cv, a.heads, out)()
            torch.cuda.synchronize()
            got = out[0, rows].float()
            err = (got - ref).abs().max().item()
            mean = (got - ref).abs().mean().item()
            ok = err <= 2 * err_ref + 2e-2 and bool(torch.isfinite(out.float()).all())
            print(f"check[{cname}] {name}: max|out - ref_f32| = {err:.5f} (bf16 rounding of ref: {err_ref:.5f}), mean {mean:.6f}  "
                  f"{'OK' if ok else 'FAIL'}", flush=True)
    for name, lib in libs:
        if name not in a.stamp.split(","):
            continue
        out = torch.zeros((1, a.nq, c), dtype=torch.bfloat16, device=dev)
        fn = runner(lib, q, k, v, a.heads, out)
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        raw = out[0, 0::256, :].contiguous().view(torch.int32).view(-1, a.heads, 64)[:, :, :4].reshape(-1, 4).cpu()
        raw = raw[raw[:, 2] > 0]
        cyc, ticks, steps = raw[:, 0].double(), raw[:, 1].double(), raw[:, 2].double()
        per_step = (cyc / steps).median().item()
        clock = (cyc / ticks * 100).median().item()
        outside = (raw[:, 3].double() - cyc).median().item()
        print(f"stamp {name}: {len(raw)} workgroups, median {per_step:.0f} shader cycles per step (64 MFMAs = 2048), "
              f"in-kernel clock {clock:.0f} MHz, steps {int(steps.median().item())}, prologue+epilogue {outside:.0f} cycles "
              f"(loop total {cyc.median().item():.0f})", flush=True)
    out = torch.empty((1, a.nq, c), dtype=torch.bfloat16, device=dev)
    fns = [(n, runner(lib, q, k, v, a.heads, out)) for n, lib in libs]
    if a.qk8:
        bufs, ws = hip.attention_qk8_scratch(a.nq, a.heads, 128, q.device), []
        need = hip.load().fg_attn_workspace_bytes(1, a.nq, a.nq, a.heads)
        wsb = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)

        def attn_only():
            hip._call("fg_attn_fwd_qk8_bf16", *[hip._ptr(t) for t in bufs[:4]], hip._ptr(v), v.stride(1), hip._ptr(out), a.nq, a.nq, a.heads, 128,
                      128 ** -0.5, hip._ptr(wsb) if need else None, need, hip._stream(out))
        fns += [("qk8", lambda: hip.attention_qk8(q, k, v, a.heads, out=out, workspace=ws, bufs=bufs)), ("qk8-attn", attn_only)]
    if a.pv8:
        pv_bufs, ws_pv = hip.attention_pv8_scratch(a.nq, a.heads, 128, q.device), []

        def pv8_attn_only():
            hip._call("fg_attn_fwd_pv8_bf16", *[hip._ptr(t) for t in bufs[:4]], hip._ptr(pv_bufs[0]), hip._ptr(pv_bufs[1]), hip._ptr(out), a.nq, a.nq,
                      a.heads, 128, 128 ** -0.5, hip._ptr(wsb) if need else None, need, hip._stream(out))

        def pv8_chain():
            hip.attention_qk8(q, k, v, a.heads, out=out, workspace=ws_pv, bufs=bufs, pv8=True, pv8_bufs=pv_bufs)
        ref = reference(q, k, v)
        for name, fn in (("qk8", fns[-2][1]), ("pv8", pv8_chain)):
            out.zero_()
            fn()
            torch.cuda.synchronize()
            err = (out[0, rows].float() - ref).abs()
            print(f"check[random] {name}: max|out - ref_f32| = {err.max().item():.5f}, mean {err.mean().item():.6f}", flush=True)
        fns += [("pv8", pv8_chain), ("pv8-attn", pv8_attn_only), ("quant-qk", lambda: hip.attn_quant_qk(q, k, a.heads, bufs)),
                ("quant-vt", lambda: hip.attn_quant_vt(v, a.heads, pv_bufs))]
    if a.smooth_v:
        pvs_bufs, ws_pvs = hip.attention_pv8_scratch(a.nq, a.heads, 128, q.device, smooth=True), []

        def pv8s_attn_only():
            hip._call("fg_attn_fwd_pv8s_bf16", *[hip._ptr(t) for t in bufs[:4]], hip._ptr(pvs_bufs[0]), hip._ptr(pvs_bufs[1]), hip._ptr(pvs_bufs[3]),
                      hip._ptr(out), a.nq, a.nq, a.heads, 128, 128 ** -0.5, hip._ptr(wsb) if need else None, need, hip._stream(out))

        def pv8s_chain():
            hip.attention_qk8(q, k, v, a.heads, out=out, workspace=ws_pvs, bufs=bufs, pv8=True, pv8_bufs=pvs_bufs, smooth=True)
        out.zero_()
        pv8s_chain()
        torch.cuda.synchronize()
        err = (out[0, rows].float() - reference(q, k, v)).abs()
        print(f"check[random] pv8s: max|out - ref_f32| = {err.max().item():.5f}, mean {err.mean().item():.6f}", flush=True)
        fns += [("pv8s", pv8s_chain), ("pv8s-attn", pv8s_attn_only), ("quant-vts", lambda: hip.attn_quant_vt(v, a.heads, pvs_bufs, smooth=True))]
    if a.qk8_fused:
        n, nh = a.nq, a.heads
        qkv = rnd(1, n, 3 * c)
        wq, wk = (1 + 0.1 * rnd(c).float()).to(torch.bfloat16), (1 + 0.1 * rnd(c).float()).to(torch.bfloat16)
        ang = torch.rand((n, 64), generator=g, device=dev, dtype=torch.float64) * 6.283185307179586
        tab = torch.stack([ang.cos(), ang.sin()], -1).float().contiguous()
        xq, xk, xv = qkv[..., :c], qkv[..., c:2 * c], qkv[..., 2 * c:]
        q16, k16 = torch.empty((1, n, c), dtype=torch.bfloat16, device=dev), torch.empty((1, n, c), dtype=torch.bfloat16, device=dev)
        b2, bf = hip.attention_qk8_scratch(n, nh, 128, dev), hip.attention_qk8_fused_scratch(n, nh, 128, dev)
        ws16, ws2, wsf = [], [], []
        scale16 = hip.pow2_softmax_scale(128)[0]
        o16, o2, of = (torch.empty((1, n, c), dtype=torch.bfloat16, device=dev) for _ in range(3))

        def norms():
            hip.rmsnorm_rope(xk, wk, nh, 1e-6, tab, None, out=k16)
            hip.rmsnorm_rope(xq, wq, nh, 1e-6, tab, None, out=q16)

        def prod_two():
            norms()
            hip.attn_quant_qk(q16, k16, nh, b2)

        def prod_fused():
            hip.rmsnorm_rope_kstats(xk, wk, nh, 1e-6, tab, None, out=k16, partials=bf[5])
            hip.rmsnorm_rope_q8(xq, wq, nh, 1e-6, tab, None, q8=bf[0], sq=bf[2])
            hip.attn_quant_k(k16, bf[5], nh, bf[1], bf[3], bf[4])

        def chain_bf16():
            norms()
            hip.attention(q16, k16, xv, nh, out=o16, scale=scale16, workspace=ws16)

        def chain_two():
            prod_two()
            hip.attention_qk8_pre(*b2[:4], xv, nh, out=o2, workspace=ws2)

        def chain_fused():
            prod_fused()
            hip.attention_qk8_pre(*bf[:4], xv, nh, out=of, workspace=wsf)
        chain_two(), chain_fused()
        torch.cuda.synchronize()
        same = all(torch.equal(x.view(torch.uint8) if x.dtype == torch.float8_e4m3fn else x, y.view(torch.uint8) if y.dtype == torch.float8_e4m3fn else y)
                   for x, y in zip(b2, bf[:5])) and torch.equal(o2, of)
        print(f"check[chain] the fused producers and the two-step path: q8, k8, sq, sk, key mean and the attention output "
              f"{'are the same bytes  OK' if same else 'DIFFER  FAIL'}", flush=True)
        fns += [("chain-bf16", chain_bf16), ("chain-qk8", chain_two), ("chain-qk8-fused", chain_fused), ("prod-bf16", norms), ("prod-qk8", prod_two),
                ("prod-qk8-fused", prod_fused)]
    for _, fn in fns:
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    times = {n: [] for n, _ in fns}
    for _ in range(a.rounds):
        for n, fn in fns:
            evs = []
            for _ in range(a.iters):
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record(); fn(); e.record()
                evs.append((s, e))
            torch.cuda.synchronize()
            times[n] += [s.elapsed_time(e) for s, e in evs]
    fl = 4.0 * a.nq * a.nkv * c
    for n, ts in times.items():
        ts = sorted(ts)
        med, mn = ts[len(ts) // 2], ts[0]
        if n.startswith(("chain-", "prod-", "quant-")):      # several launches: the mean and the spread of the repeated runs, no FLOP rate
            mean = sum(ts) / len(ts)
            sd = (sum((t - mean) ** 2 for t in ts) / max(len(ts) - 1, 1)) ** 0.5
            print(f"{n}: N={a.nq} H={a.heads}: mean {mean:.4f} ms, sd {sd:.4f}, median {med:.4f}, min {mn:.4f}, max {ts[-1]:.4f} ({len(ts)} runs)", flush=True)
            continue
        spread = ""
        if a.smooth_v:
            mean = sum(ts) / len(ts)
            spread = f", mean {mean:.3f}, sd {(sum((t - mean) ** 2 for t in ts) / max(len(ts) - 1, 1)) ** 0.5:.4f} ({len(ts)} runs)"
        print(f"{n}: nq={a.nq} nkv={a.nkv} H={a.heads}: median {med:.3f} ms = {fl / med / 1e9:.1f} TFLOP/s, min {mn:.3f} ms = {fl / mn / 1e9:.1f}"
              f"{spread}", flush=True)


if __name__ == "__main__":
    main()
