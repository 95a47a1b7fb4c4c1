"""The gated residual store of a stacked CFG pair two ways, per GEMM: A = two fg_gemm_*_s launches of N rows (one per element, what the
stacked forward does without the opt-in), B = one fg_gemm_*_sp launch on 2 N rows with rows_per_element = N
(enable_stacked_cfg(periodic_gate=True)).  In the style of tools/gemm_ab.py: legs interleaved in one process, device events around every
sample, median and standard deviation.

    python tools/gemm_periodic_ab.py                          # self_attn.o (3072 x 3072) and ffn.2 (3072 x 14336) at N = 8 190 and 27 280
    python tools/gemm_periodic_ab.py --dtype fp8 --rows 8190

A sample is `--inner` back-to-back repetitions of a leg (the residual stream is updated in place; its values do not matter to the time)
between two events; `--rounds` rounds alternate A and B.  Before timing, both legs run once from the same residual stream and their
results are compared: "differ" counts the elements whose bits differ (0 where the two plans give every element the same summation — the
rule itself never differs: tests/test_gemm_periodic_gate.py) and the largest difference."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fairygen_amd import hip  # noqa: E402

SHAPES = {"self_attn.o": (3072, 3072), "ffn.2": (3072, 14336)}      # (out features, in features)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="8190,27280", help="rows of ONE element")
    ap.add_argument("--dtype", default="bf16,fp8")
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--inner", type=int, default=4)
    ap.add_argument("--first-rows", type=int, default=0, help="default: one latent frame of a 13-frame clip, rows / 13")
    a = ap.parse_args()
    hip.load()
    dev = "cuda"
    g = torch.Generator("cpu").manual_seed(7)
    rnd = lambda *s, scale=1.0: (torch.randn(s, generator=g) * scale).to(torch.bfloat16).to(dev)      # noqa: E731
    out = []
    for rows in (int(r) for r in a.rows.split(",")):
        first = a.first_rows or rows // 13
        for name, (n, k) in SHAPES.items():
            x, w, bias = rnd(2, rows, k, scale=0.5), rnd(n, k, scale=0.02), rnd(n, scale=0.2)
            mod = hip.ModTable(rnd(2, 6, n), first)
            res = rnd(2, rows, n)
            for dtype in a.dtype.split(","):
                if dtype == "fp8":
                    xq, sc = hip.fp8_quant_rows(x)
                    w8 = w.to(torch.float8_e4m3fn)

                    def leg_a(c):
                        for e in range(2):
                            hip.gemm_fp8(xq[e * rows:(e + 1) * rows], sc[e * rows:(e + 1) * rows], w8, bias, out=c[e:e + 1], residual=True, mod=mod, gate_idx=2)

                    def leg_b(c):
                        hip.gemm_fp8(xq, sc, w8, bias, out=c, residual=True, mod=mod, gate_idx=2, rows_per_element=rows)
                else:
                    def leg_a(c):
                        for e in range(2):
                            hip.gemm_epilogue(x[e:e + 1], w, bias, out=c[e:e + 1], residual=True, mod=mod, gate_idx=2)

                    def leg_b(c):
                        hip.gemm_epilogue(x, w, bias, out=c, residual=True, mod=mod, gate_idx=2, rows_per_element=rows)
                ca, cb = res.clone(), res.clone()
                leg_a(ca), leg_b(cb)
                torch.cuda.synchronize()
                differ, max_diff = int((ca != cb).sum().item()), (ca.float() - cb.float()).abs().max().item()
                c = res.clone()
                samples = {"A": [], "B": []}
                for _ in range(a.rounds):
                    for tag, fn in (("A", leg_a), ("B", leg_b)):
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        for _ in range(a.inner):
                            fn(c)
                        e1.record()
                        e1.synchronize()
                        samples[tag].append(e0.elapsed_time(e1) * 1000.0 / a.inner)
                        c.copy_(res)
                med = {t: statistics.median(v) for t, v in samples.items()}
                sd = {t: statistics.pstdev(v) for t, v in samples.items()}
                flop = 2.0 * 2 * rows * n * k
                row = {"linear": name, "rows": rows, "dtype": dtype, "first_rows": first, "A_two_s_us": round(med["A"], 1), "A_sd_us": round(sd["A"], 1),
                       "B_one_sp_us": round(med["B"], 1), "B_sd_us": round(sd["B"], 1), "B_over_A": round(med["B"] / med["A"], 4),
                       "A_tflops": round(flop / med["A"] / 1e6, 1), "B_tflops": round(flop / med["B"] / 1e6, 1), "differ": differ,
                       "max_diff": max_diff, "samples": a.rounds}
                out.append(row)
                print(f"{name:12s} {dtype:4s} rows 2 x {rows:6d}: A (two _s) {row['A_two_s_us']:9.1f} us sd {row['A_sd_us']:6.1f} | B (one _sp) "
                      f"{row['B_one_sp_us']:9.1f} us sd {row['B_sd_us']:6.1f} | B / A {row['B_over_A']:.4f} | {row['A_tflops']} -> {row['B_tflops']} TFLOP/s | "
                      f"differ {differ} max {max_diff:.4g}", flush=True)
            del x, w, bias, res
            torch.cuda.empty_cache()
    print(json.dumps({"tool": "gemm_periodic_ab", "rounds": a.rounds, "inner": a.inner, "device": torch.cuda.get_device_name(0), "rows": out}))


if __name__ == "__main__":
    main()
