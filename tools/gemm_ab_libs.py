"""Interleaved A/B of two BUILDS of libinfini_rocm.so in one process (tools/build_variant.py makes them; a copy of an older build's
library serves as the parent): bf16 NN GEMMs through the plain C ABI of each library, `--rounds` rounds of `--reps` launches per
library and shape, alternating, on N(0,1) operands (--variant wave128 forces the four-wave kernel on shapes the planner routes elsewhere). Prints min / median / max microseconds per launch and library.
  python tools/gemm_ab_libs.py NAME=path/to/a.so NAME=path/to/b.so [...] [--rounds 8] [--reps 30] [--shapes 4096x4096x4096,8192x4096x4096]
Give the same library under two names for the noise floor. (Each library is loaded with RTLD_LOCAL | RTLD_DEEPBIND, so its calls bind
to its own code, and has its own runtime and stream; a round of one library is synchronised before the other's starts.)"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import torch

BF16 = 16


class Lib:
    def __init__(self, name, path):
        self.name = name
        self.L = C.CDLL(path, mode=os.RTLD_LOCAL | os.RTLD_DEEPBIND)
        vp, i32, i64 = C.c_void_p, C.c_int, C.c_int64
        self.L.infini_rocm_last_error.restype = C.c_char_p
        self.L.infini_rocm_runtime_create.argtypes = [i32, C.POINTER(vp)]
        self.L.infini_rocm_runtime_sync.argtypes = [vp]
        self.L.infini_rocm_event_create.argtypes = [C.POINTER(vp)]
        self.L.infini_rocm_event_record.argtypes = [vp, vp]
        self.L.infini_rocm_event_elapsed_ms.argtypes = [vp, vp, C.POINTER(C.c_float)]
        self.L.infini_rocm_matmul.argtypes = [vp, i32, vp, vp, vp, vp, i64, i64, i64, i64, i32, i32, i64, i64, i64, i64, i64, i32]
        self.L.infini_rocm_matmul_last_variant.argtypes = [vp, C.POINTER(C.c_int)]
        self.L.infini_rocm_matmul_set_variant.argtypes = [vp, i32]
        self.L.infini_rocm_matmul_num_variants.restype = i32
        self.L.infini_rocm_matmul_variant_name.argtypes = [i32]
        self.L.infini_rocm_matmul_variant_name.restype = C.c_char_p
        self.rt = vp()
        self.ok(self.L.infini_rocm_runtime_create(0, C.byref(self.rt)))
        self.e0, self.e1 = vp(), vp()
        self.ok(self.L.infini_rocm_event_create(C.byref(self.e0)))
        self.ok(self.L.infini_rocm_event_create(C.byref(self.e1)))

    def ok(self, st):
        if st != 0:
            sys.exit(f"{self.name}: status {st}: {self.L.infini_rocm_last_error().decode(errors='replace')}")

    def matmul(self, a, b, c, m, n, k):
        self.ok(self.L.infini_rocm_matmul(self.rt, BF16, a.data_ptr(), b.data_ptr(), None, c.data_ptr(), 1, m, n, k, 0, 0, 0, 0, 0, 0, 0, 0))

    def round_us(self, a, b, c, m, n, k, reps):
        for _ in range(3):
            self.matmul(a, b, c, m, n, k)
        self.ok(self.L.infini_rocm_event_record(self.rt, self.e0))
        for _ in range(reps):
            self.matmul(a, b, c, m, n, k)
        self.ok(self.L.infini_rocm_event_record(self.rt, self.e1))
        self.ok(self.L.infini_rocm_runtime_sync(self.rt))
        ms = C.c_float()
        self.ok(self.L.infini_rocm_event_elapsed_ms(self.e0, self.e1, C.byref(ms)))
        return ms.value * 1000.0 / reps

    def force(self, name):
        names = [self.L.infini_rocm_matmul_variant_name(i).decode() for i in range(self.L.infini_rocm_matmul_num_variants())]
        self.ok(self.L.infini_rocm_matmul_set_variant(self.rt, names.index(name) if name else -1))

    def variant(self):
        v = C.c_int(-1)
        self.ok(self.L.infini_rocm_matmul_last_variant(self.rt, C.byref(v)))
        return self.L.infini_rocm_matmul_variant_name(v.value).decode()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("libs", nargs="+", help="NAME=path")
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warm", type=int, default=300, help="launches per library before the first round of a shape")
    ap.add_argument("--shapes", default="4096x4096x4096")
    ap.add_argument("--variant", default="", help="force this kernel variant (e.g. wave128) instead of the route planner's choice")
    args = ap.parse_args()
    libs = [Lib(*s.split("=", 1)) for s in args.libs]
    for lb in libs:
        lb.force(args.variant)
    for shape in args.shapes.split(","):
        m, n, k = (int(v) for v in shape.split("x"))
        a = torch.randn(m, k, device="cuda").to(torch.bfloat16)
        b = torch.randn(k, n, device="cuda").to(torch.bfloat16)
        outs = [torch.empty(m, n, device="cuda", dtype=torch.bfloat16) for _ in libs]
        torch.cuda.synchronize()
        for lb, c in zip(libs, outs):
            for _ in range(args.warm):
                lb.matmul(a, b, c, m, n, k)
            lb.ok(lb.L.infini_rocm_runtime_sync(lb.rt))
        res = {lb.name: [] for lb in libs}
        for _ in range(args.rounds):
            for lb, c in zip(libs, outs):
                res[lb.name].append(lb.round_us(a, b, c, m, n, k, args.reps))
        same = all(torch.equal(outs[0].view(torch.int16), c.view(torch.int16)) for c in outs[1:])
        row = {"shape": [m, n, k], "dtype": "bf16", "layout": "NN", "rounds": args.rounds, "reps": args.reps, "variant": libs[0].variant(),
               "results_bit_equal": same}
        for name, v in res.items():
            row[name] = {"min_us": round(min(v), 2), "median_us": round(statistics.median(v), 2), "max_us": round(max(v), 2)}
        print(json.dumps(row), flush=True)
