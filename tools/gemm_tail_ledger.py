"""Where a launch of the four-wave GEMM (csrc/gemm128w.hip) spends its time outside the K loop: per-workgroup clock stamps at kernel
entry, first MFMA, last MFMA, last store issued and after the final wait, taken by wave 0 of every workgroup in the DIAGNOSTIC build
(IROCM_W128_DBG=16: tools/diag_build.py; the shipped library holds no stamp) and written to the runtime workspace, never into C.
  python tools/gemm_tail_ledger.py [--m 4096 --n 4096 --k 4096] [--seconds 2.0] [--label parent] [--lib path/to/another/diagnostic/build.so]
bf16 NN on N(0,1) operands; the launch that is read is the last one of `--seconds` of back-to-back launches (warm clocks). Medians over
workgroups, in microseconds of the 100 MHz reference (core cycles in brackets); launch span = latest end - earliest entry."""
import argparse
import os
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
if "--lib" in sys.argv:  # (before the package is imported: it binds the library named by INFINI_ROCM_LIB)
    os.environ["INFINI_ROCM_LIB"] = sys.argv[sys.argv.index("--lib") + 1]
else:
    from tools.diag_build import use_diag_build

    use_diag_build()
os.environ["IROCM_W128_DBG"] = "16"
import numpy as np  # noqa: E402
import torch  # noqa: E402

from infinitensor_amd import RocmRuntime, ops  # noqa: E402

STAMPS = 8  # u64 per workgroup: core clock at entry, first MFMA, last MFMA, last store, end; 100 MHz clock at entry, last MFMA, end

if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=4096)
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--k", type=int, default=4096)
    ap.add_argument("--seconds", type=float, default=2.0)
    ap.add_argument("--label", default="")
    ap.add_argument("--lib", default=None, help="a diagnostic build other than infinitensor_amd/lib/ab/diag.so")
    a = ap.parse_args()
    rt = RocmRuntime(0)
    dt = torch.bfloat16
    x = torch.randn(a.m, a.k, device="cuda").to(dt)
    y = torch.randn(a.k, a.n, device="cuda").to(dt)
    out = torch.empty(a.m, a.n, device="cuda", dtype=dt)
    grid = min((a.m // 256) * (a.n // 256), rt.device_info()["compute_units"])
    nbytes = grid * STAMPS * 8
    rt.workspace(nbytes)
    ops.set_matmul_variant(rt, ops.matmul_variants().index("wave128"))
    try:
        t0 = time.time()
        launches = 0
        while time.time() - t0 < a.seconds:
            for _ in range(200):
                ops.matmul(rt, x, y, out=out)
            launches += 200
            rt.sync()
        assert ops.matmul_last_variant(rt) == "wave128"
    finally:
        ops.set_matmul_variant(rt, -1)
    rt.sync()
    host = np.zeros(grid * STAMPS, dtype=np.uint64)
    rt.copy_to_cpu(host.ctypes.data, rt.workspace(nbytes), nbytes)
    s = host.reshape(grid, STAMPS).astype(np.int64)
    assert (s[:, 4] > s[:, 0]).all(), "no stamps: is this the diagnostic build?"
    mhz = statistics.median(((s[:, 4] - s[:, 0]) / np.maximum(s[:, 7] - s[:, 5], 1) * 100).tolist())

    def row(name, cyc):
        med = statistics.median(cyc.tolist())
        print(f"  {name:<34} {med / mhz:8.2f} us  [{int(med):>7} cycles]  min {cyc.min() / mhz:7.2f}  max {cyc.max() / mhz:7.2f}")

    print(f"{a.label or 'ledger'}: bf16 NN {a.m} x {a.n} x {a.k}, {grid} workgroups, launch {launches} of {a.seconds:.1f} s back to back, core clock {mhz:.0f} MHz")
    row("entry -> first MFMA", s[:, 1] - s[:, 0])
    row("first MFMA -> last MFMA", s[:, 2] - s[:, 1])
    row("last MFMA -> last store issued", s[:, 3] - s[:, 2])
    row("last store issued -> final wait", s[:, 4] - s[:, 3])
    row("last MFMA -> workgroup end", s[:, 4] - s[:, 2])
    row("entry -> workgroup end", s[:, 4] - s[:, 0])
    span = (s[:, 7].max() - s[:, 5].min()) / 100.0
    print(f"  launch span (100 MHz clock): first entry -> last end {span:.2f} us; entries spread over {(s[:, 5].max() - s[:, 5].min()) / 100.0:.2f} us; "
          f"median last MFMA -> last end of the launch {(s[:, 7].max() - statistics.median(s[:, 6].tolist())) / 100.0:.2f} us")
