"""fp32 MatMul time per compute type ("default" exact, "bf16", "bf16x3", "bf16x6") on the headline 4096^3 and the Llama projection
2048 x 4096 x 4096, timed like tools/gemm_shapes.py (20 ms of launches first, 5 warm-up calls per column, HIP events around `--iters`
calls). The split modes' time includes their input pass (split.hip). TF = 2 m n k / time: the rate of the fp32 problem, not of the
bf16 products behind it.  python tools/gemm_compute_types.py [--iters 50]"""
import argparse
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import torch

from infinitensor_amd import RocmRuntime, ops
from infinitensor_amd.runtime import Event

SHAPES = [("headline", 4096, 4096, 4096), ("llama qkv/o", 2048, 4096, 4096)]
TYPES = ["default", "bf16", "bf16x3", "bf16x6"]

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=50)
args = ap.parse_args()
rt = RocmRuntime(0)
try:
    for name, m, n, k in SHAPES:
        a = torch.randn(m, k, device="cuda")
        b = torch.randn(k, n, device="cuda") * 0.05
        c = torch.empty(m, n, device="cuda")
        torch.cuda.synchronize()
        ops.set_matmul_compute_type(rt, "default")
        t_end = time.perf_counter() + 0.02
        while time.perf_counter() < t_end:
            for _ in range(2):
                ops.matmul(rt, a, b, out=c)
            rt.sync()
        ref = None
        line = f"{name:12s} {m:5d}x{n:5d}x{k:5d} {2.0 * m * n * k / 1e9:8.1f} GF |"
        for ct in TYPES:
            ops.set_matmul_compute_type(rt, ct)
            for _ in range(5):
                ops.matmul(rt, a, b, out=c)
            e0, e1 = Event(), Event()
            rt.record(e0)
            for _ in range(args.iters):
                ops.matmul(rt, a, b, out=c)
            rt.record(e1)
            us = rt.elapsed_ms(e0, e1) / args.iters * 1e3
            rt.sync()
            if ref is None:
                ref = c.double()
            err = float((c.double() - ref).abs().max())
            line += f" {ct:>7s} [{ops.matmul_last_variant(rt)}]: {us:8.1f} us {2.0 * m * n * k / us / 1e6:7.1f} TF, max |c - default| {err:.1e} |"
        print(line, flush=True)
finally:
    ops.set_matmul_compute_type(rt, "default")
