"""Row-op routing without a GPU: infini_rocm_rowop_plan_route (csrc/rowops_route.h: rowop_plan) against the Python mirror that the
selector tests derive their bounds from (rowop_cases.route), over exactly the grid of rowop_cases.scan_routes, so that a threshold
edited on one side alone fails here. tests/test_gpu_rowop_selectors.py holds the planner to what a launch reports
(ops.rowop_last_route after every launch)."""
import ctypes

import pytest
import torch

import rowop_cases as C
from infinitensor_amd import ops
from infinitensor_amd._lib import check, lib

TD = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
OPS = [(op, dt, pre) for op in ops.ROWOPS for dt in C.DTS for pre in ((False, True) if op == "add_norm" else (False,))]


def plan(op, dt, outer, n, inner=1, aligned=True, has_pre=False, **kw):
    return ops.rowop_plan_route(op, TD[dt], outer, n, inner, has_pre, ptr_lo=0 if aligned else 8, **kw)


@pytest.mark.parametrize("op,dt,has_pre", OPS, ids=lambda v: str(v))
def test_planner_and_mirror_agree_on_the_whole_scan(op, dt, has_pre):
    v, seen = C.VEC[dt], set()
    ns = sorted({m + d for m in range(0, 2048 * v + 3 * v, v) for d in (-1, 0, 1) if m + d >= 1})  # scan_routes' grid
    for n in ns:
        for al in (True, False):
            for outer in (5, 4096):
                got = plan(op, dt, outer, n, 1, al, has_pre)
                assert got == C.route(op, dt, outer, n, 1, al, int(op == "add_norm"), has_pre), (n, al, outer)
                seen.add(got)
    if op == "softmax":
        got = plan(op, dt, 5, 7, 3)
        assert got == C.route(op, dt, 5, 7, 3) == "softmax_strided"
        seen.add(got)
    assert seen == C.scan_routes(op, dt, has_pre)


TENSORS = {"softmax": ("x", "y"), "layer_norm": ("x", "y", "scale", "bias"), "rms_norm": ("x", "y", "scale"),
           "add_norm": ("a", "b", "pre", "y", "scale", "bias")}
EVERY_NAME = ("x", "y", "a", "b", "pre", "scale", "bias")


@pytest.mark.parametrize("op,dt,has_pre", OPS, ids=lambda v: str(v))
def test_one_pointer_eight_bytes_off(op, dt, has_pre):
    """Each tensor the op is given, alone 8 bytes off a 16-byte boundary, takes the unaligned route; one it is not given changes nothing."""
    n = 64 * C.VEC[dt]
    base = 0x7F0000001000
    add = int(op == "add_norm")
    aligned, unaligned = C.route(op, dt, 5, n, 1, True, add, has_pre), C.route(op, dt, 5, n, 1, False, add, has_pre)
    assert aligned != unaligned
    given = [t for t in TENSORS[op] if t != "pre" or has_pre]
    for name in EVERY_NAME:
        lo = ops.rowop_ptr_lo(op, has_pre, **{t: base + (8 if t == name else 0) for t in EVERY_NAME})
        assert lo == (8 if name in given else 0), name
        assert ops.rowop_plan_route(op, TD[dt], 5, n, 1, has_pre, ptr_lo=lo) == (unaligned if name in given else aligned), name
    for lo in range(1, 16):  # any low bit, not only 8
        assert ops.rowop_plan_route(op, TD[dt], 5, n, 1, has_pre, ptr_lo=lo) == unaligned
    assert ops.rowop_plan_route(op, TD[dt], 5, n, 1, has_pre, ptr_lo=16) == aligned  # the low four bits only


@pytest.mark.parametrize("dt", C.DTS)
def test_row_groups_start_at_4096_rows(dt):
    for row_bytes, r in ((1024, 4), (2048, 2)):
        n = row_bytes // C.SIZE[dt]
        c = C.ceil_div(n, 64 * C.VEC[dt])
        assert plan("softmax", dt, 4095, n) == f"softmax_wave/C{c}/aligned/R1"
        assert plan("softmax", dt, 4096, n) == f"softmax_wave/C{c}/aligned/R{r}"
        assert plan("softmax", dt, 4096, n, aligned=False) == f"softmax_wave/C{c}/unaligned/R1"
    # R = 2 is the planner's choice up to 3072 bytes, but rows above 2048 bytes are three chunks and take the four-chunk kernel, which is
    # built for R = 1 only: nothing flips there (as in the dispatch this planner replaced)
    n = 3072 // C.SIZE[dt]
    assert plan("softmax", dt, 4095, n) == plan("softmax", dt, 4096, n) == "softmax_wave/C4/aligned/R1"


def test_zero_extents_and_bad_arguments():
    f16 = torch.float16
    for op in ops.ROWOPS:
        assert ops.rowop_plan_route(op, f16, 0, 64) == "none"
        assert ops.rowop_plan_route(op, f16, 5, 0) == "none"
    assert ops.rowop_plan_route("softmax", f16, 5, 64, inner=0) == "none"
    for bad in (dict(dtype=torch.int32), dict(num_cu=0), dict(num_cu=-1), dict(outer=-1), dict(n=-1), dict(n=1 << 31), dict(inner=-1)):
        kw = dict(op="softmax", dtype=f16, outer=5, n=64, inner=1)
        kw.update(bad)
        with pytest.raises(RuntimeError):
            ops.rowop_plan_route(**kw)
    with pytest.raises(RuntimeError):
        ops.rowop_plan_route("layer_norm", f16, 5, 64, inner=2)  # only softmax has an inner extent
    with pytest.raises(ValueError):
        ops.rowop_plan_route("batch_norm", f16, 5, 64)
    with pytest.raises(RuntimeError):
        buf = ctypes.create_string_buffer(64)
        check(lib().infini_rocm_rowop_plan_route(len(ops.ROWOPS), int(ops._TORCH2DT[f16]), 5, 64, 1, 0, 0, 256, buf, len(buf)))  # a bad op
