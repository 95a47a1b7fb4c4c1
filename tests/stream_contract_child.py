"""Child process of tests/test_stream_contract.py::test_first_launch_of_a_process_inside_a_capture.

The first thing this process asks of libfairygen_hip.so is, per case of CHILD_CASES, one call inside a stream capture on a fresh side
stream: the function-local statics of the launchers (hipFuncSetAttribute for the kernels with more than 64 KiB of LDS, the device / CU-count
caches, the getenv switches) and the runtime's loading of the kernels all happen there.  Operands are made on the CPU and copied by torch;
the GEMM scheduler block is zeroed by torch and its scratch is sized and allocated inside the capture, so the device query behind
fg_gemm_workspace_bytes runs there too.  Each graph is then replayed once into sentinel-filled outputs and compared, byte for byte, with the eager call on the default
stream.  Exits non-zero at the first error and starts nothing after it."""
import sys
import traceback

import torch

import test_stream_contract as sc
from fairygen_amd import hip


def main():
    assert torch.cuda.is_available(), "needs the GPU"
    lib = hip.load()
    done = []
    for name in sc.CHILD_CASES:
        case = sc.CASES[name]
        t = {k: v.cuda() for k, v in sc.cpu_set(name, sc.SEEDS[0]).items()}
        for k in case.outs:
            sc.fill_sentinel(t[k])
        kept = {k: v.clone() for k, v in t.items()}
        sched = torch.zeros(lib.fg_gemm_sched_bytes(), dtype=torch.uint8, device="cuda") if case.scratch == "gemm" else None
        torch.cuda.synchronize()
        side, graph = torch.cuda.Stream(), torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            state = None
            if sched is not None:
                state = (sched, torch.empty(lib.fg_gemm_workspace_bytes(256, 256, 256), dtype=torch.uint8, device="cuda"))
            if case.derive is not None:
                case.derive(hip, t)
            outs = case.run(hip, t, state=state)
        torch.cuda.synchronize()
        for o in outs:
            sc.fill_sentinel(o)
        for k in case.inputs:
            if k in kept:
                t[k].copy_(kept[k])
        graph.replay()
        torch.cuda.synchronize()
        got = [o.clone() for o in outs]
        done.append((name, case, kept, got, graph))
        print(f"captured and replayed {name}", flush=True)
    for name, case, kept, got, _ in done:
        if case.derive is not None:
            case.derive(hip, kept)
        want = sc.eager(hip, case, kept)
        torch.cuda.synchronize()
        sc.assert_outputs(got, want, f"{name}, captured as the first launch of the process")
        print(f"{name}: equal to eager", flush=True)
    print(f"{len(done)} captures equal eager")


if __name__ == "__main__":
    try:
        main()
    except BaseException:
        traceback.print_exc()
        sys.stdout.flush()
        sys.exit(1)
