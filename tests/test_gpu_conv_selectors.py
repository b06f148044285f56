"""Conv2d on a real MI355X against the exact selector inputs and the per-element bound of tests/conv_cases.py (proved on the oracle
alone in tests/test_conv_selectors_cpu.py): every route of csrc/conv_route.h and every kernel form of csrc/conv_s1.hip, the tile
widths and split-K factors behind the IROCM_CONV_* switches, the fused stem + pool and ConvTranspose.

Selector tests compare with `==`: one-hot filters (every tap x the channels at the ends of every K tile) and delta images (corners,
edges, the 16-byte run boundary, the element where the tensor ends). x, w, bias and residual sit in the middle of buffers filled with
1000 (a tap that reaches outside its tensor must contribute exactly 0; a leak shows as +-1000 w), the output is pre-filled with 7
(an unwritten element is a wrong element) inside a block whose guard regions must keep their fill, a residual must come back
untouched, and the launch must report the declared route: a silent fall-back is a failure.

test_conv_random_inputs_per_element repeats the random inputs of the allclose tests in tests/test_gpu_nn.py and checks them against
bound = u |want| + 2^-17 S instead (the residual cases of the pixel-slot GEMM, which rounds conv + bias before it adds the residual,
with the derived term u |conv + bias| on top: conv_cases.ROUNDS_BEFORE_RESIDUAL; against the shared bound alone they reach 13.9 in
f16 and 57.8 in bf16). Worst err / bound per (route, dtype), from the lines it prints (pytest -s), measured on an MI355X:

    route            dtype worst  launches  where
    depthwise        f16   0.491      9     (1, 3, 15, 7) of dw-2x32x30x30x1x3x1x1
    depthwise        bf16  0.497      9     (1, 18, 2, 16) of dw-2x12x17x23x2x3x1x1
    generic          f16   0.477      3     (0, 11, 0, 7) of oracle-3x32x9x11x48x8x3x2x2x0x2x1x1x2
    generic          bf16  0.494      3     (2, 38, 5, 0) of oracle-3x32x9x11x48x8x3x2x2x0x2x1x1x2
    pixel_gemm       f16   0.477      8     (3, 270, 2, 5) of pw_gemm-5x128x14x14x512
    pixel_gemm       bf16  0.495      8     (1, 111, 3, 2) of pw_gemm-2x64x5x3x256
    resident         f16   0.473      1     (0, 1, 40, 48) of s1-1x64x56x56x64x3x3
    resident         bf16  0.493      1     (0, 22, 44, 51) of s1-1x64x56x56x64x3x3
    tap_gemm         f16   0.476      5     (1, 273, 0, 0) of tap-2x64x30x18x300x2
    tap_gemm         bf16  0.495      5     (1, 160, 0, 7) of tap-2x64x30x18x300x2
    tap_gemm_splitk  f16   0.477     12     (1, 182, 5, 6) of tap-2x128x14x14x512x2
    tap_gemm_splitk  bf16  0.493     12     (0, 195, 5, 3) of tap-2x128x7x7x512x1
    tap_shifted      f16   0.487     36     (0, 62, 44, 0) of oracle-2x64x56x56x64x64x1x1x0x0x1x1x1x1
    tap_shifted      bf16  0.496     36     (1, 195, 10, 6) of oracle-2x128x14x14x256x128x1x1x0x0x1x1x1x1

Every figure is the final rounding's half ulp against the bound's whole one: no route accumulates below fp32 or rounds twice, the
pixel-slot GEMM's residual epilogue apart. The whole file (834 tests) ran in 8 seconds; no selector case failed on any route.
"""
import numpy as np
import pytest
import torch

import conv_cases as C
from infinitensor_amd import ops
from test_gpu_nn import TD, dev_slack2

pytestmark = pytest.mark.gpu
GUARD = 512  # elements of fill in front of and behind the output


def slack(a, dt):
    return None if a is None else dev_slack2(np.asarray(a, dtype=np.float32), TD[dt], fill=C.SLACK_FILL)


def out_block(shape, dt):
    numel = int(np.prod(shape))
    block = torch.full((numel + 2 * GUARD,), C.OUT_FILL, device="cuda", dtype=TD[dt])
    return block, block[GUARD:GUARD + numel].view(shape)


def host(t):
    return t.float().cpu().numpy().astype(np.float64)


def guards_hold(block):
    return bool(torch.all(block[:GUARD] == C.OUT_FILL).item() and torch.all(block[-GUARD:] == C.OUT_FILL).item())


def set_env(monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))


def launch(rt, g, dt, xd, wd, bd, rd, act):
    """One conv2d into a pre-filled block -> (block, output on the host, reported route)."""
    block, out = out_block((g.n, g.f, g.oh, g.ow), dt)
    ops.conv2d(rt, xd, wd, g.ph, g.pw, g.sh, g.sw, g.dh, g.dw, bias=bd, act=act, out=out, residual=rd)
    return block, host(out), ops.conv_last_route(rt)


@pytest.mark.parametrize("name,dt,mode", C.case_params(True), ids=lambda v: str(v))
def test_tap_selectors(rt, name, dt, mode, monkeypatch):
    g = C.CASES[name]
    set_env(monkeypatch, g.env)
    inp = C.tap_inputs(name, dt, mode)
    xd, bd, rd = slack(inp.x, dt), slack(inp.bias, dt), slack(inp.res, dt)
    keep = None if rd is None else rd.clone()
    try:
        ops.set_conv_variant(rt, g.variant)
        for j, sel in enumerate(C.tap_rounds(g)):
            wd = slack(sel.w, dt)
            want = C.epilogue(C.selected(g, inp.x, sel), inp.bias, inp.res, inp.act)
            for run in range(g.runs):
                block, got, route = launch(rt, g, dt, xd, wd, bd, rd, inp.act)
                what = f"{name} {dt} {mode} round {j} run {run} ({route})"
                assert route == g.gpu_route, what
                C.assert_exact(got, want, what, C.describe_tap(g, inp.x, sel))
                assert guards_hold(block), f"{what}: wrote outside the output"
    finally:
        ops.set_conv_variant(rt, -1)
    assert rd is None or torch.equal(rd, keep), "the residual was written"


@pytest.mark.parametrize("name,dt", C.case_params(False), ids=lambda v: str(v))
def test_pixel_selectors(rt, name, dt, monkeypatch):
    g = C.CASES[name]
    set_env(monkeypatch, g.env)
    w = C.pixel_weights(name, dt)
    wd = slack(w, dt)
    try:
        ops.set_conv_variant(rt, g.variant)
        for j, deltas in enumerate(C.pixel_rounds(g)):
            x = C.delta_image(g, deltas)
            xd = slack(x, dt)
            want = C.conv_sparse(g, x, w)
            for run in range(g.runs):
                block, got, route = launch(rt, g, dt, xd, wd, None, None, 0)
                what = f"{name} {dt} pixel round {j} run {run} ({route})"
                assert route == g.gpu_route, what
                C.assert_exact(got, want, what, C.describe_pixel(g, deltas, w))
                assert guards_hold(block), f"{what}: wrote outside the output"
    finally:
        ops.set_conv_variant(rt, -1)


@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("mode", C.STEM_MODES)
@pytest.mark.parametrize("name", list(C.STEM_POOL))
def test_stem_pool_selectors(rt, name, mode, dt):
    """ops.conv2d_pool (7 x 7 / 2 + bias + ReLU + MaxPool 3 x 3 / 2): the max-pool of the exact selected values."""
    g = C.STEM_POOL[name]
    inp = C.tap_inputs(name, dt, mode, "stem")
    xd, bd = slack(inp.x, dt), slack(inp.bias, dt)
    for j, sel in enumerate(C.tap_rounds(g)):
        want = C.stem_pool_selected(g, inp.x, sel, inp.bias)
        block, out = out_block(want.shape, dt)
        ops.conv2d_pool(rt, xd, slack(sel.w, dt), bd, 3, 3, 2, 2, 3, 2, 1, out=out)
        what = f"{name} {dt} {mode} round {j}"
        assert ops.conv_last_route(rt) == "stem_pool", what
        C.assert_exact(host(out), want, what,
                       lambda idx: f"filter {idx[1]} selects (c, r, s) = ({sel.c[idx[1]]}, {sel.r[idx[1]]}, {sel.s[idx[1]]}) x {sel.v[idx[1]]}")
        assert guards_hold(block), f"{what}: wrote outside the output"


@pytest.mark.parametrize("dt", ["f32", "f16", "bf16"])
@pytest.mark.parametrize("name", list(C.CONVT))
def test_conv_transpose_selectors(rt, name, dt):
    """conv_transpose_direct, the only ConvTranspose kernel (no route to report; ops.conv_transpose2d allocates its own output, so
    no guard regions either): one non-zero weight per output channel, random x and — with bias + ReLU — the grid."""
    cfg = C.CONVT[name]
    n, f, h, w, cg, r, s, ph, pw, sh, sw, dh, dw, oph, opw, groups = cfg
    rng = np.random.default_rng(C.seed_of(name, dt, 3))
    for grid in (False, True):
        x = C.grid_x(rng, (n, f, h, w)) if grid else C.storage_normal(rng, (n, f, h, w), dt)
        bias = C.grid_bias(cg * groups) if grid else None
        xd, bd = slack(x, dt), slack(bias, dt)
        for j, sel in enumerate(C.convt_rounds(cfg)):
            y = ops.conv_transpose2d(rt, xd, slack(sel.w, dt), ph, pw, sh, sw, dh, dw, oph, opw, groups, bias=bd, act=1 if grid else 0)
            want = C.epilogue(C.convt_selected(cfg, x, sel), bias, None, 1 if grid else 0)
            C.assert_exact(host(y), want, f"{name} {dt} {'grid bias relu' if grid else 'plain'} round {j}",
                           lambda idx: f"output channel {idx[1]} selects (f, r, s) = ({sel.f[idx[1]]}, {sel.r[idx[1]]}, {sel.s[idx[1]]}) x {sel.v[idx[1]]}")


_RANDOM = C.random_params()


@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("family,cfg", _RANDOM, ids=[C.random_geom(f, c).name for f, c in _RANDOM])
def test_conv_random_inputs_per_element(rt, family, cfg, dt, monkeypatch):
    """The generators and seeds of test_conv_vs_oracle, test_conv_s1_vs_oracle_and_generic_kernel, test_conv_pointwise_gemm_mode,
    test_conv3x3_tap_gemm_mode, test_conv3x3_tap_gemm_split_k (on sampled outputs: those layers are too large for a dense fp64
    reference in seconds) and test_conv_depthwise_kernel, against the per-element bound instead of an allclose."""
    ref = C.random_reference(family, cfg, dt)
    g = ref.g
    _, variant, _, has_res, act = C.RANDOM_FAMILIES[family]
    set_env(monkeypatch, g.env)
    planned = ops.conv_plan_route(TD[dt], g.n, g.c, g.h, g.w, g.f, g.r, g.s, g.ph, g.pw, g.sh, g.sw, g.dh, g.dw, g.groups, act, has_res,
                                  variant, rt.device_info()["compute_units"])[0]
    if planned == "tap_shifted" and g.n * g.c * g.h * g.w * 2 < 64:
        planned = "generic"  # the launcher declines inputs of less than 64 bytes (csrc/conv_s1.hip, fill_args)
    xd, wd, bd, rd = slack(ref.x, dt), slack(ref.w, dt), slack(ref.bias, dt), slack(ref.res, dt)
    keep = None if rd is None else rd.clone()
    try:
        ops.set_conv_variant(rt, variant)
        for run in range(2 if family == "tap_split" else 1):
            block, got, route = launch(rt, g, dt, xd, wd, bd, rd, act)
            assert route == planned, (g.name, dt, route, planned)
            if ref.coords is not None:
                got = got[tuple(ref.coords.T)]
            # (the one derived exception: a route that rounds conv + bias before it adds the residual — conv_cases.py)
            bound = ref.bound_rounded_pre if has_res and route in C.ROUNDS_BEFORE_RESIDUAL else ref.bound
            worst, idx = C.worst_ratio(got, ref.want, bound)
            at = idx if ref.coords is None else tuple(int(v) for v in ref.coords[idx[0]])
            print(f"\nworst conv {route} {dt} {worst:.3f} at {at} ({g.name})", end="")
            C.assert_within(got, ref.want, bound, f"{g.name} {dt} ({route})")
            assert guards_hold(block)
    finally:
        ops.set_conv_variant(rt, -1)
    assert rd is None or torch.equal(rd, keep)
