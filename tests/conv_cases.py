"""Selector inputs and a per-element bound for the Conv2d kernels (csrc/conv*.hip, csrc/gemm256p_conv*.hip, csrc/gemm32.hip).

With random normal x and w / sqrt(K) one product is about 1 / sqrt(K), the size of the tolerance of an allclose: a term that is
dropped, counted twice or read from a neighbour is seen by luck or not at all. A convolution is linear in w and in x, so the inputs
built here make ONE product carry a whole output element and the result exact in f16, bf16 and f32, whatever the order of the
sum, the split-K factor or the roundings of the epilogue. numpy and oracle/ref_ops.py only: imports without a GPU.

Tap selectors (one-hot filters)
  w[f] is zero except w[f, c_f, r_f, s_f] = v_f, v_f from {1, -1, 2, -1/2}: y[n, f, oh, ow] = v_f x[n, c_f, oh sh - ph + r_f dh,
  ow sw - pw + s_f dw] exactly, and exactly 0 where that index is padding (every other product is 0 * finite, fp32 sums of zeros
  are exact, a product with a power of two does not round). Targets: every tap x the target channels (0, C - 1 and both sides of
  every 8-, 32- and 64-channel boundary, inside the filter's own group); round j gives filter f the target T[(j F + f) mod |T|].
  Above MAX_TAP_ROUNDS rounds the 8- and 32-boundaries are thinned; taps, channel 0, channel C - 1 and the 64-boundaries never.
  x: random normal rounded to storage with magnitudes below 2^-6 pushed up to 2^-6 (nothing rests on how the matrix instruction
  treats f16 subnormals), or — in the modes with a real bias / residual — the grid: x in multiples of 1/4 up to 4, bias and
  residual in multiples of 1/8 up to 4, so that every value and partial sum of v x + bias + residual is a multiple of 1/8 of
  magnitude at most 16: at most 8 significant bits, which bf16 holds, however often the kernel rounds.
Pixel selectors (delta images)
  x[n] is zero except for a few deltas of value 1, -2 or 1/2 whose output footprints are disjoint (asserted); w dense random normal
  rounded to storage and pushed up to 2^-6 likewise. Every output is exactly one weight times the delta, or exactly 0. Target pixels:
  corners, edge middles, centre, pixels 7 and 8 of the plane (the 16-byte run boundary), the last pixel; the last image of every
  round carries the last pixel of its plane in channel C - 1: the element where the tensor ends.
Both are compared with `==` element by element (-0 equals +0, NaN equals nothing); `assert_exact` names the first wrong element and
the (c, r, s) it should have selected.

Per-element bound for random inputs: the constants and the reasoning of tests/test_gpu_matmul.py::test_matmul_16bit_variants,
      bound = u |want| + 2^-17 S,   S = conv(|x|, |w|) + |bias| + |residual| of THAT element,   u = 2^-7 (bf16), 2^-10 (f16)
  one storage ulp of the result for its final rounding plus the fp32 accumulation error, 2^-17 S being ~2^7 fp32 ulps of S; `want`
  is the fp64 result of the rounded operands. Nothing here comes from what a kernel returned.

MUTATIONS: numpy convolutions with one named defect each, for tests/test_conv_selectors_cpu.py to prove that the selectors see
them (and that the allclose form does not).
"""
from __future__ import annotations

import functools
from types import SimpleNamespace

import numpy as np

from attention_cases import assert_within, worst_ratio  # noqa: F401  (the checker of the attention selectors, shared)
from oracle import ref_ops as R

U = {"f16": 2.0 ** -10, "bf16": 2.0 ** -7}
SLACK_FILL = 1000.0   # around x, w, bias and the residual: a tap that reaches outside its tensor shows as +-1000 w
OUT_FILL = 7.0        # the output and its guard regions before the launch
FLOOR = 2.0 ** -6
W_VALUES = (1.0, -1.0, 2.0, -0.5)
DELTA_VALUES = (1.0, -2.0, 0.5)
MAX_TAP_ROUNDS = 6
MAX_PIXEL_ROUNDS = 8
DELTAS_PER_IMAGE = 4


# ------------------------------------------------------------------------------------------------------------------------
# geometry and the case table
# ------------------------------------------------------------------------------------------------------------------------
def geom(n, c, h, w, f, cpg, r, s, ph, pw, sh=1, sw=1, dh=1, dw=1, **extra):
    """One Conv2d problem; oh / ow by the reference's shape rule (src/operators/conv.cc:98-101, as oracle/ref_ops.py::conv2d)."""
    assert c % cpg == 0 and f % (c // cpg) == 0
    g = SimpleNamespace(n=n, c=c, h=h, w=w, f=f, cpg=cpg, r=r, s=s, ph=ph, pw=pw, sh=sh, sw=sw, dh=dh, dw=dw, groups=c // cpg,
                        fpg=f // (c // cpg), oh=(h - (r - sh) * dh + 2 * ph) // sh, ow=(w - (s - sw) * dw + 2 * pw) // sw, **extra)
    g.k = cpg * r * s
    g.macs = n * f * g.oh * g.ow * g.k
    g.args = (ph, pw, sh, sw, dh, dw)
    return g


# epilogue modes: name -> (grid inputs, bias: None / "zero" / "grid", residual, act)
MODES = {
    "plain": (False, None, False, 0),
    "relu": (False, None, False, 1),  # (the fused stem + pool only: its ReLU is part of the kernel)
    "zero_bias_relu": (False, "zero", False, 1),
    "bias": (True, "grid", False, 0),
    "bias_relu": (True, "grid", False, 1),
    "res": (True, None, True, 0),
    "res_relu": (True, None, True, 1),
    "bias_res": (True, "grid", True, 0),
    "bias_res_relu": (True, "grid", True, 1),
}

CASES: dict = {}


def _case(name, n, c, h, w, f, r, s, route, form="", *, cpg=None, pad=None, stride=(1, 1), dil=(1, 1), variant=-1, env=None,
          gpu_route=None, dts=("f16", "bf16"), residual=True, runs=1):
    """pad None: the "same" padding of tests/test_gpu_nn.py::S1_CONVS, (R - 1) dh / 2. `route`, `form`: what the planner reports for
    256 CUs; `gpu_route`: what the launch reports where the launcher refines it (the fp32 split-K). `residual`: whether the route
    takes one (a route that does not would silently hand the call to another kernel: those modes are left out, not skipped)."""
    ph, pw = ((r - 1) * dil[0] // 2, (s - 1) * dil[1] // 2) if pad is None else pad
    modes = tuple(m for m, (_, _, res, _) in MODES.items() if m != "relu" and (residual or not res))
    assert name not in CASES
    CASES[name] = geom(n, c, h, w, f, c if cpg is None else cpg, r, s, ph, pw, stride[0], stride[1], dil[0], dil[1], name=name,
                       variant=variant, env=dict(env or {}), route=route, form=form, gpu_route=gpu_route or route, dts=dts,
                       modes=modes, runs=runs)


# generic implicit GEMM (variant 1)
_case("generic-grouped-asym", 3, 32, 9, 11, 48, 3, 2, "generic", cpg=8, pad=(2, 0), stride=(2, 1), dil=(1, 2), variant=1)
_case("generic-c512-f130", 1, 512, 7, 7, 130, 3, 3, "generic", variant=1)  # ragged filter tile, K = 4608
# conv_s1.hip forms
_case("s1_1_4_32-49px", 5, 64, 7, 7, 64, 3, 3, "tap_shifted", "s1<1,4,32>", variant=4)  # 49-pixel planes, tiles span images
_case("s1_2_2_32-5x5", 2, 96, 12, 10, 72, 5, 5, "tap_shifted", "s1<2,2,32>", variant=4)  # C % 64 != 0
_case("s1_2_2_64", 2, 64, 16, 16, 128, 3, 3, "tap_shifted", "s1<2,2,64>", variant=4)
_case("pw-64px", 3, 64, 8, 8, 256, 1, 1, "tap_shifted", "pw", variant=2)  # 1.5 column tiles, two filter tiles
_case("pw-196px-f200", 2, 128, 14, 14, 200, 1, 1, "tap_shifted", "pw", variant=2)  # two K-steps, ragged filters, pad slots
_case("rowtap-stem", 2, 3, 32, 32, 64, 7, 7, "tap_shifted", "rowtap", stride=(2, 2), variant=2)  # K = 147 padded to 160
_case("rowtap-c5-f70", 2, 5, 11, 7, 70, 3, 5, "tap_shifted", "rowtap", stride=(2, 1), variant=2)  # K = 75, two filter tiles
_case("rowtap-k1", 3, 1, 6, 6, 8, 1, 1, "tap_shifted", "rowtap", variant=2)  # K = 1
_case("patch-49px-f136", 9, 256, 7, 7, 136, 3, 3, "tap_shifted", "patch", variant=2)  # tiles span 2-3 images, tensor ends mid-run
_case("patch-3x1", 3, 160, 9, 11, 100, 3, 1, "tap_shifted", "patch", variant=2)  # five channel blocks, 99-pixel planes
_case("patch_wide", 3, 64, 14, 14, 256, 3, 3, "tap_shifted", "patch_wide", variant=6)
_case("resident-one-tile", 2, 64, 8, 8, 64, 3, 3, "resident", "resident", residual=False)
_case("resident-c32-f48", 3, 32, 16, 16, 48, 3, 3, "resident", "resident", residual=False)
_case("phase-3x3s2", 3, 64, 14, 14, 96, 3, 3, "tap_shifted", "s1<2,2,64>", stride=(2, 2), variant=2)  # all four phases
_case("phase-odd", 2, 32, 7, 9, 40, 3, 3, "tap_shifted", "s1<1,4,32>", stride=(2, 2), variant=2)  # last phase row / column is padding
_case("phase-5x3s3x2", 2, 32, 9, 10, 24, 5, 3, "tap_shifted", "s1<1,4,32>", stride=(3, 2), variant=2)
_case("dilation2", 2, 64, 11, 11, 70, 3, 3, "tap_shifted", "s1<2,2,64>", dil=(2, 2), variant=2)
# the persistent 256-row GEMM in conv mode: pixel slots (variant 5), taps (variant 7), every tile width
for _nt in (2, 3, 4):
    _case(f"pixel_gemm-49px-f320-nt{_nt}", 9, 192, 7, 7, 320, 1, 1, "pixel_gemm", variant=5, env={"IROCM_CONV_PW_NT": _nt})
    _case(f"pixel_gemm-15px-nt{_nt}", 2, 64, 5, 3, 256, 1, 1, "pixel_gemm", variant=5, env={"IROCM_CONV_PW_NT": _nt})  # 7-pixel tail
    _case(f"tap_gemm-f320-nt{_nt}", 5, 192, 9, 11, 320, 3, 3, "tap_gemm", variant=7, env={"IROCM_CONV_TAP_NT": _nt}, residual=False)
    _case(f"tap_gemm-s2-odd-nt{_nt}", 2, 64, 15, 13, 256, 3, 3, "tap_gemm", stride=(2, 2), pad=(1, 1), variant=7,
          env={"IROCM_CONV_TAP_NT": _nt}, residual=False)
_case("pixel_gemm-strided", 8, 128, 15, 13, 256, 1, 1, "pixel_gemm", stride=(2, 2), variant=5)  # through the phase split
# (run twice: the hand-off flags must be zero again after the first launch)
_case("tap_splitk-x2", 16, 128, 14, 14, 256, 3, 3, "tap_gemm_splitk", variant=7, env={"IROCM_CONV_TAP_SPLIT": 2}, residual=False, runs=2)
_case("tap_splitk-x4", 16, 256, 14, 14, 256, 3, 3, "tap_gemm_splitk", variant=7, env={"IROCM_CONV_TAP_SPLIT": 4}, residual=False, runs=2)
_case("tap_splitk-s2-x2", 10, 256, 28, 28, 256, 3, 3, "tap_gemm_splitk", stride=(2, 2), pad=(1, 1), variant=7,
      env={"IROCM_CONV_TAP_SPLIT": 2}, residual=False, runs=2)
_case("batched_gemm", 2, 128, 16, 16, 256, 1, 1, "batched_gemm", variant=3, residual=False)
# depthwise (conv_dw.hip): n, c, h, w, multiplier, k, stride, pad of tests/test_gpu_nn.py::DW_CFGS
_case("dw-5x5s2", 3, 24, 19, 19, 24, 5, 5, "depthwise", cpg=1, stride=(2, 2), pad=(2, 2), residual=False)
_case("dw-mult2", 2, 12, 17, 23, 24, 3, 3, "depthwise", cpg=1, pad=(1, 1), residual=False)
_case("dw-tiny-planes", 4, 20, 7, 7, 20, 3, 3, "depthwise", cpg=1, pad=(1, 1), residual=False)
_case("dw-valid", 1, 6, 12, 12, 6, 3, 3, "depthwise", cpg=1, pad=(0, 0), residual=False)
# fp32: the implicit GEMM on the fp32 matrix instruction, its split-K and 128^2 forms, one GEMM per image, one output per thread
_F32 = dict(dts=("f32",))
_case("igemm32-49px-f160", 3, 64, 7, 7, 160, 3, 3, "igemm32", **_F32)
_case("igemm32-stem", 5, 3, 38, 38, 72, 7, 7, "igemm32", stride=(2, 2), **_F32)  # K = 147 -> rows of 148 floats
_case("igemm32-k45", 2, 5, 11, 13, 9, 3, 3, "igemm32", **_F32)
_case("igemm32-asym", 1, 8, 33, 17, 24, 5, 3, "igemm32", pad=(2, 0), stride=(1, 2), dil=(1, 2), **_F32)
_case("igemm32-splitk3", 3, 64, 7, 7, 160, 3, 3, "igemm32", gpu_route="igemm32_splitk", env={"IROCM_CONV32_SPLIT": 3}, **_F32)
_case("igemm32-splitk4", 3, 64, 7, 7, 160, 3, 3, "igemm32", gpu_route="igemm32_splitk", env={"IROCM_CONV32_SPLIT": 4}, **_F32)
_case("igemm32-tile128", 3, 64, 7, 7, 160, 3, 3, "igemm32", env={"IROCM_CONV32_TILE": 2}, **_F32)
_case("batched_gemm32", 3, 64, 14, 14, 96, 1, 1, "batched_gemm32", env={"IROCM_CONV32_PW_BATCHED": 1}, residual=False, **_F32)
_case("direct32", 1, 8, 33, 17, 24, 5, 3, "direct32", pad=(2, 0), stride=(1, 2), dil=(1, 2), variant=1, **_F32)
_case("direct32-grouped", 3, 32, 9, 11, 48, 3, 2, "direct32", cpg=8, pad=(2, 0), stride=(2, 1), dil=(1, 2), variant=1, **_F32)

# the fused stem + pool (ops.conv2d_pool: 7 x 7 / 2 / 3 + bias + ReLU + MaxPool 3 x 3 / 2 / 1): n, h, w
STEM_POOL = {"stem-32x32": geom(2, 3, 32, 32, 64, 3, 7, 7, 3, 3, 2, 2, name="stem-32x32"),
             "stem-9x8": geom(2, 3, 9, 8, 64, 3, 7, 7, 3, 3, 2, 2, name="stem-9x8")}
STEM_MODES = ("relu", "zero_bias_relu", "bias_relu")
# ConvTranspose (conv_transpose_direct), from tests/test_gpu_nn.py::CONVT: n, f, h, w, cg, r, s, ph, pw, sh, sw, dh, dw, oph, opw, groups
CONVT = {"convt-up2": (2, 8, 5, 6, 4, 3, 3, 1, 1, 2, 2, 1, 1, 1, 1, 1),
         "convt-grouped-strided": (2, 6, 7, 5, 2, 3, 2, 0, 1, 1, 3, 2, 1, 0, 2, 3)}


def case_params(with_modes: bool):
    """(case name, dt[, mode]) for every case of the table."""
    out = []
    for name, cs in CASES.items():
        for dt in cs.dts:
            out += [(name, dt, m) for m in cs.modes] if with_modes else [(name, dt)]
    return out


# ------------------------------------------------------------------------------------------------------------------------
# values
# ------------------------------------------------------------------------------------------------------------------------
def storage_normal(rng, shape, dt):
    """Random normal rounded to the storage type, magnitudes below 2^-6 pushed up to 2^-6 (the sign kept)."""
    a = R.round_to(rng.standard_normal(shape), dt)
    return np.where(np.abs(a) < FLOOR, np.where(a < 0, -FLOOR, FLOOR), a)


def grid_x(rng, shape):
    return rng.integers(-16, 17, shape) / 4.0


def grid_bias(f):
    """Multiples of 1/8 up to 4; neighbouring filters never share a value (a bias taken from filter f - 1 is a wrong value)."""
    return ((5 * np.arange(f) + 3) % 65 - 32) / 8.0


def grid_residual(rng, shape):
    return rng.integers(-32, 33, shape) / 8.0


def epilogue(y, bias, res, act):
    if bias is not None:
        y = y + np.asarray(bias, dtype=np.float64).reshape(1, -1, 1, 1)
    if res is not None:
        y = y + res
    return np.maximum(y, 0) if act else y


# ------------------------------------------------------------------------------------------------------------------------
# three exact evaluators of the same convolution: one-hot filters (a gather), sparse images (a scatter), dense (tap loops)
# ------------------------------------------------------------------------------------------------------------------------
def padded(g, x, leak: bool = False):
    """x with its zero padding (and whatever the last tap reaches beyond it). leak: the defect "pad_row_leak"."""
    hp = max(g.h + 2 * g.ph, (g.oh - 1) * g.sh + (g.r - 1) * g.dh + 1)
    wp = max(g.w + 2 * g.pw, (g.ow - 1) * g.sw + (g.s - 1) * g.dw + 1)
    xp = np.zeros((g.n, g.c, hp, wp))
    xp[:, :, g.ph:g.ph + g.h, g.pw:g.pw + g.w] = x
    if leak:  # the row below a plane is the first row of the plane that follows it in memory
        planes = np.asarray(x, dtype=np.float64).reshape(g.n * g.c, g.h, g.w)
        xp.reshape(g.n * g.c, hp, wp)[:-1, g.ph + g.h, g.pw:g.pw + g.w] = planes[1:, 0, :]
    return xp


def _gather(g, xp, cl, rr, ss, val):
    ch = (np.arange(g.f) // g.fpg) * g.cpg + cl
    iy = np.arange(g.oh)[None, :] * g.sh + (rr * g.dh)[:, None]
    ix = np.arange(g.ow)[None, :] * g.sw + (ss * g.dw)[:, None]
    return val[None, :, None, None] * xp[:, ch[:, None, None], iy[:, :, None], ix[:, None, :]]


def selected(g, x, sel):
    """The expected output of a tap-selector round: filter f reads one input element per output element, times v_f."""
    return _gather(g, padded(g, x), sel.c, sel.r, sel.s, sel.v)


def conv_onehot(g, xp, w):
    flat = w.reshape(g.f, -1)
    assert ((flat != 0).sum(axis=1) <= 1).all()
    k = np.abs(flat).argmax(axis=1)
    cl, rr, ss = np.unravel_index(k, w.shape[1:])
    return _gather(g, xp, cl, rr, ss, flat[np.arange(g.f), k])


def conv_sparse(g, x, w, leak: bool = False):
    y = np.zeros((g.n, g.f, g.oh, g.ow))
    for n, c0, h0, w0 in np.argwhere(x != 0):
        hits = [(n, c0, h0)]
        if leak and h0 == 0 and n * g.c + c0 > 0:  # row 0 also stands below the plane in front of this one
            hits.append(((n * g.c + c0 - 1) // g.c, (n * g.c + c0 - 1) % g.c, g.h))
        for n1, c1, h1 in hits:
            fs = slice(c1 // g.cpg * g.fpg, (c1 // g.cpg + 1) * g.fpg)
            for rr in range(g.r):
                oy, rem = divmod(h1 + g.ph - rr * g.dh, g.sh)
                if rem or not 0 <= oy < g.oh:
                    continue
                for ss in range(g.s):
                    ox, rem = divmod(w0 + g.pw - ss * g.dw, g.sw)
                    if rem == 0 and 0 <= ox < g.ow:
                        y[n1, fs, oy, ox] += x[n, c0, h0, w0] * w[fs, c1 % g.cpg, rr, ss]
    return y


def conv_dense(g, xp, w):
    y = np.zeros((g.n, g.f, g.oh, g.ow))
    for gi in range(g.groups):
        xs, ws = xp[:, gi * g.cpg:(gi + 1) * g.cpg], w[gi * g.fpg:(gi + 1) * g.fpg]
        for rr in range(g.r):
            for ss in range(g.s):
                patch = xs[:, :, rr * g.dh: rr * g.dh + (g.oh - 1) * g.sh + 1: g.sh, ss * g.dw: ss * g.dw + (g.ow - 1) * g.sw + 1: g.sw]
                y[:, gi * g.fpg:(gi + 1) * g.fpg] += np.einsum("nchw,fc->nfhw", patch, ws[:, :, rr, ss], optimize=True)
    return y


def conv_any(g, x, w, leak: bool = False):
    x, w = np.asarray(x, dtype=np.float64), np.asarray(w, dtype=np.float64)
    if ((w.reshape(g.f, -1) != 0).sum(axis=1) <= 1).all():
        return conv_onehot(g, padded(g, x, leak), w)
    if np.count_nonzero(x) <= 64:
        return conv_sparse(g, x, w, leak)
    return conv_dense(g, padded(g, x, leak), w)


# ------------------------------------------------------------------------------------------------------------------------
# tap selectors
# ------------------------------------------------------------------------------------------------------------------------
def _sides(cpg, b):
    return {c for k in range(b, cpg, b) for c in (k - 1, k)}


def required_channels(cpg):
    return sorted({0, cpg - 1} | _sides(cpg, 64))


def boundary_channels(cpg):
    """0, C - 1 and both sides of every 8-, 32- and 64-channel boundary that exists."""
    return sorted({0, cpg - 1} | _sides(cpg, 8) | _sides(cpg, 32) | _sides(cpg, 64))


def target_channels(cpg, f, taps, max_rounds=MAX_TAP_ROUNDS):
    """0, C - 1 and both sides of every 8-, 32- and 64-channel boundary of a group; where that makes more than `max_rounds`
    rounds of f filters, as many of the 32- and then the 8-boundaries (evenly spaced) as fit."""
    req = set(required_channels(cpg))
    full = set(boundary_channels(cpg))
    if -(-len(full) * taps // f) <= max_rounds:
        return sorted(full)
    budget = max(0, max_rounds * f // taps - len(req))
    opt32 = sorted(_sides(cpg, 32) - req)[:budget]
    opt8 = sorted(full - req - set(opt32))
    room = budget - len(opt32)
    pick = [opt8[i] for i in sorted({int(i) for i in np.linspace(0, len(opt8) - 1, room)})] if room > 0 and opt8 else []
    return sorted(req | set(opt32) | set(pick))


def tap_targets(g):
    """[(c, r, s)]: every tap crossed with the target channels, tap-major."""
    chans = target_channels(g.cpg, g.f, g.r * g.s)
    return [(c, rr, ss) for rr in range(g.r) for ss in range(g.s) for c in chans]


def tap_rounds(g):
    """The one-hot weight tensors of a case: [SimpleNamespace(w [F, C/g, R, S], c, r, s, v per filter)]."""
    T = tap_targets(g)
    nrounds = -(-len(T) // g.f)
    assert 1 <= nrounds <= MAX_TAP_ROUNDS, (g.name, nrounds)
    out = []
    for j in range(nrounds):
        t = np.array([T[(j * g.f + f) % len(T)] for f in range(g.f)])
        v = np.array([W_VALUES[(f + j) % 4] for f in range(g.f)])
        w = np.zeros((g.f, g.cpg, g.r, g.s))
        w[np.arange(g.f), t[:, 0], t[:, 1], t[:, 2]] = v
        out.append(SimpleNamespace(w=w, c=t[:, 0], r=t[:, 1], s=t[:, 2], v=v))
    return out


def seed_of(name, dt, salt):
    return [salt, sorted(("f16", "bf16", "f32")).index(dt)] + [ord(ch) for ch in name]


@functools.lru_cache(maxsize=4)
def tap_inputs(name: str, dt: str, mode: str, table: str = "conv"):
    """x, bias, residual and act of one (case, dtype, mode), shared by the rounds (and not to be modified)."""
    g = {"conv": CASES, "stem": STEM_POOL}[table][name]
    grid, bias_kind, has_res, act = MODES[mode]
    rng = np.random.default_rng(seed_of(name, dt, 1))
    x = grid_x(rng, (g.n, g.c, g.h, g.w)) if grid else storage_normal(rng, (g.n, g.c, g.h, g.w), dt)
    bias = {None: None, "zero": np.zeros(g.f), "grid": grid_bias(g.f)}[bias_kind]
    res = grid_residual(rng, (g.n, g.f, g.oh, g.ow)) if has_res else None
    for a in (x, bias, res):
        if a is not None:
            assert np.array_equal(R.round_to(a, dt), a)
            a.setflags(write=False)
    return SimpleNamespace(x=x, bias=bias, res=res, act=act, grid=grid)


def describe_tap(g, x, sel):
    """idx (n, f, oh, ow) -> what that element should have selected, for the failure message."""
    def say(idx):
        n, f, oy, ox = idx
        c = f // g.fpg * g.cpg + sel.c[f]
        iy, ix = oy * g.sh - g.ph + sel.r[f] * g.dh, ox * g.sw - g.pw + sel.s[f] * g.dw
        inside = 0 <= iy < g.h and 0 <= ix < g.w
        src = f"x[{n}, {c}, {iy}, {ix}] = {x[n, c, iy, ix]!r}" if inside else f"padding at ({iy}, {ix})"
        return f"filter {f} selects (c, r, s) = ({c}, {sel.r[f]}, {sel.s[f]}) with weight {sel.v[f]}: {src}"
    return say


def assert_exact(got, want, what: str = "", describe=None):
    """got == want element by element (-0 equals +0, NaN equals nothing); names the first wrong element."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = ~(got == want)
    if bad.any():
        idx = tuple(int(i) for i in np.unravel_index(int(np.argmax(bad)), bad.shape))
        more = f"; {describe(idx)}" if describe is not None else ""
        raise AssertionError(f"{what}: {int(bad.sum())} wrong elements, the first at (n, f, oh, ow) = {idx}: got {got[idx]!r}, "
                             f"want {want[idx]!r}{more}")


# ------------------------------------------------------------------------------------------------------------------------
# pixel selectors
# ------------------------------------------------------------------------------------------------------------------------
def target_pixels(h, w):
    """Corners, edge middles, centre, pixels 7 and 8 of the plane, the last pixel; each once."""
    px = [(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1), (0, w // 2), (h // 2, 0), (h // 2, w - 1), (h - 1, w // 2), (h // 2, w // 2)]
    px += [divmod(p, w) for p in (7, 8) if p < h * w]
    return list(dict.fromkeys(px + [(h - 1, w - 1)]))


def pixel_channels(g):
    local = target_channels(g.cpg, g.f, g.r * g.s)
    return [gi * g.cpg + c for gi in range(g.groups) for c in local]


def footprint(g, h0, w0):
    """[OH, OW] bool: the output pixels that read input pixel (h0, w0)."""
    rows, cols = np.zeros(g.oh, dtype=bool), np.zeros(g.ow, dtype=bool)
    for rr in range(g.r):
        oy, rem = divmod(h0 + g.ph - rr * g.dh, g.sh)
        if rem == 0 and 0 <= oy < g.oh:
            rows[oy] = True
    for ss in range(g.s):
        ox, rem = divmod(w0 + g.pw - ss * g.dw, g.sw)
        if rem == 0 and 0 <= ox < g.ow:
            cols[ox] = True
    return rows[:, None] & cols[None, :]


def pixel_rounds(g):
    """[[(n, c, h, w, value)]]: the deltas of every round. Pixels and channels are paired cyclically over images and rounds; an
    image takes up to DELTAS_PER_IMAGE deltas whose footprints are disjoint; the last image always starts with the tensor's
    last element. Every target pixel is covered (asserted); channels as far as MAX_PIXEL_ROUNDS rounds reach."""
    P, Ch = target_pixels(g.h, g.w), pixel_channels(g)
    pending = [(P[i % len(P)], Ch[i % len(Ch)]) for i in range(max(len(P), len(Ch)))]
    last = (g.h - 1, g.w - 1)
    rounds, count = [], 0
    while (pending or not rounds) and len(rounds) < MAX_PIXEL_ROUNDS:
        rnd = []
        for n in range(g.n):
            occ = np.zeros((g.oh, g.ow), dtype=bool)
            taken = 0
            if n == g.n - 1:
                occ |= footprint(g, *last)
                rnd.append((n, g.c - 1, last[0], last[1], DELTA_VALUES[count % 3]))
                count, taken = count + 1, 1
                for i, (p, _) in enumerate(pending):
                    if p == last:
                        pending.pop(i)
                        break
            i = 0
            while i < len(pending) and taken < DELTAS_PER_IMAGE:
                (py, px), ch = pending[i]
                fp = footprint(g, py, px)
                if (occ & fp).any():
                    i += 1
                    continue
                occ |= fp
                rnd.append((n, ch, py, px, DELTA_VALUES[count % 3]))
                count, taken = count + 1, taken + 1
                pending.pop(i)
        rounds.append(rnd)
    covered = {(d[2], d[3]) for rnd in rounds for d in rnd}
    assert set(P) <= covered, (g.name, sorted(set(P) - covered))
    for rnd in rounds:
        assert (g.n - 1, g.c - 1, g.h - 1, g.w - 1) in {d[:4] for d in rnd}
        for n in range(g.n):
            fps = [footprint(g, d[2], d[3]) for d in rnd if d[0] == n]
            assert not fps or np.sum(fps, axis=0).max() <= 1, "footprints of one image must be disjoint"
    return rounds


def delta_image(g, deltas):
    x = np.zeros((g.n, g.c, g.h, g.w))
    for n, c, h0, w0, v in deltas:
        x[n, c, h0, w0] = v
    return x


@functools.lru_cache(maxsize=4)
def pixel_weights(name: str, dt: str):
    g = CASES[name]
    w = storage_normal(np.random.default_rng(seed_of(name, dt, 2)), (g.f, g.cpg, g.r, g.s), dt)
    w.setflags(write=False)
    return w


def describe_pixel(g, deltas, w):
    def say(idx):
        n, f, oy, ox = idx
        for n0, c0, h0, w0, v in deltas:
            if n0 == n and c0 // g.cpg == f // g.fpg and footprint(g, h0, w0)[oy, ox]:
                rr, ss = (h0 + g.ph - oy * g.sh) // g.dh, (w0 + g.pw - ox * g.sw) // g.dw
                return (f"the delta {v} at x[{n0}, {c0}, {h0}, {w0}] selects (c, r, s) = ({c0}, {rr}, {ss}): "
                        f"w[{f}, {c0 % g.cpg}, {rr}, {ss}] = {w[f, c0 % g.cpg, rr, ss]!r}")
        return f"no delta of image {n} reaches it: 0 (deltas {[d for d in deltas if d[0] == n]})"
    return say


def stem_pool_selected(g, x, sel, bias):
    """The fused stem: MaxPool 3 x 3 / 2 / 1 of ReLU(selected value + bias), every value exact."""
    return R.pool2d(epilogue(selected(g, x, sel), bias, None, 1), "max", 3, 3, 1, 1, 1, 1, 2, 2, 0)


# ------------------------------------------------------------------------------------------------------------------------
# ConvTranspose: one-hot per OUTPUT channel
# ------------------------------------------------------------------------------------------------------------------------
def convt_rounds(cfg):
    """Output channel co (group gi, local cl) gets one non-zero w[f, cl, r, s] = v with f in its group: y[n, co, oy, ox] =
    v x[n, f, (oy + ph - r dh) / sh, (ox + pw - s dw) / sw] where both divide and are in range, else 0.
    -> out shape helper, [SimpleNamespace(w, f, r, s, v per output channel)]."""
    n, f, h, w, cg, r, s, ph, pw, sh, sw, dh, dw, oph, opw, groups = cfg
    fg, cout = f // groups, cg * groups
    T = [(c, rr, ss) for rr in range(r) for ss in range(s) for c in target_channels(fg, cout, r * s)]
    nrounds = -(-len(T) // cout)
    assert nrounds <= MAX_TAP_ROUNDS
    out = []
    for j in range(nrounds):
        t = np.array([T[(j * cout + co) % len(T)] for co in range(cout)])
        v = np.array([W_VALUES[(co + j) % 4] for co in range(cout)])
        wt = np.zeros((f, cg, r, s))
        co = np.arange(cout)
        fsel = co // cg * fg + t[:, 0]
        wt[fsel, co % cg, t[:, 1], t[:, 2]] = v
        out.append(SimpleNamespace(w=wt, f=fsel, r=t[:, 1], s=t[:, 2], v=v))
    return out


def convt_selected(cfg, x, sel):
    n, f, h, w, cg, r, s, ph, pw, sh, sw, dh, dw, oph, opw, groups = cfg
    oh = (h - 1) * sh - 2 * ph + dh * (r - 1) + oph + 1
    ow = (w - 1) * sw - 2 * pw + dw * (s - 1) + opw + 1
    y = np.zeros((n, cg * groups, oh, ow))
    for co in range(cg * groups):
        ny, nx = np.arange(oh) + ph - sel.r[co] * dh, np.arange(ow) + pw - sel.s[co] * dw
        oky, okx = (ny % sh == 0) & (ny // sh >= 0) & (ny // sh < h), (nx % sw == 0) & (nx // sw >= 0) & (nx // sw < w)
        src = x[:, sel.f[co]][:, np.clip(ny // sh, 0, h - 1)][:, :, np.clip(nx // sw, 0, w - 1)]
        y[:, co] = np.where(oky[:, None] & okx[None, :], sel.v[co] * src, 0.0)
    return y


# ------------------------------------------------------------------------------------------------------------------------
# random inputs of the allclose tests in tests/test_gpu_nn.py, for the per-element bound
# ------------------------------------------------------------------------------------------------------------------------
MAX_RANDOM_MACS = 2.5e8  # larger layers take the fp64 reference more than a few seconds (two dense convolutions per dtype)

# family -> (test in tests/test_gpu_nn.py whose generator and seed it repeats, conv variant, bias, residual, act)
RANDOM_FAMILIES = {
    "oracle": ("test_conv_vs_oracle", -1, False, False, 0),
    "s1": ("test_conv_s1_vs_oracle_and_generic_kernel", 2, True, False, 1),
    "pw_gemm": ("test_conv_pointwise_gemm_mode[bias_res_relu]", 5, True, True, 1),
    "tap": ("test_conv3x3_tap_gemm_mode[bias_relu]", 7, True, False, 1),
    "tap_split": ("test_conv3x3_tap_gemm_split_k", 7, True, False, 1),
    "dw": ("test_conv_depthwise_kernel[bias_relu]", -1, True, False, 1),
}


def random_geom(family: str, cfg):
    """The problem of one entry of that test's shape list, and the environment it sets."""
    env = {}
    if family == "oracle":
        g = geom(*cfg)
    elif family == "s1":
        n, c, h, w, f, r, s, sh, sw, dh, dw = cfg + (1, 1, 1, 1) if len(cfg) == 7 else cfg
        g = geom(n, c, h, w, f, c, r, s, (r - 1) * dh // 2, (s - 1) * dw // 2, sh, sw, dh, dw)
    elif family == "pw_gemm":
        n, c, h, w, f = cfg
        g = geom(n, c, h, w, f, c, 1, 1, 0, 0)
    elif family in ("tap", "tap_split"):
        n, c, h, w, f, st = cfg[:6]
        g = geom(n, c, h, w, f, c, 3, 3, 1, 1, st, st)
        if family == "tap_split":
            env = {"IROCM_CONV_TAP_SPLIT": cfg[6]}
    elif family == "dw":
        n, c, h, w, mult, k, st, pad = cfg
        g = geom(n, c, h, w, c * mult, 1, k, k, pad, pad, st, st)
    else:
        raise ValueError(family)
    g.env = env
    g.name = f"{family}-" + "x".join(str(v) for v in cfg)
    return g


def random_lists() -> dict:
    """{family: the shape list of its test}, imported from tests/test_gpu_nn.py (which imports torch: only on demand)."""
    import test_gpu_nn as N

    split = next(m for m in N.test_conv3x3_tap_gemm_split_k.pytestmark if m.name == "parametrize" and m.args[0] == "cfg").args[1]
    return {"oracle": N.CONVS, "s1": N.S1_CONVS, "pw_gemm": N.PW_GEMM, "tap": N.TAP_CFGS, "tap_split": split, "dw": N.DW_CFGS}


def random_params(lists: dict | None = None):
    """[(family, cfg)] over the imported shape lists {family: list}, without the layers above MAX_RANDOM_MACS — except the
    split-K shapes, which are all above it and are checked on SAMPLED outputs instead (random_reference)."""
    lists = random_lists() if lists is None else lists
    return [(fam, tuple(cfg)) for fam in RANDOM_FAMILIES for cfg in lists[fam]
            if fam == "tap_split" or random_geom(fam, tuple(cfg)).macs <= MAX_RANDOM_MACS]


def sample_coords(g, count=4096):
    """Random output positions plus the corners of the first and the last image at the first and the last filter."""
    rng = np.random.default_rng(12345)
    co = np.stack([rng.integers(0, m, count) for m in (g.n, g.f, g.oh, g.ow)], axis=1)
    edge = [(n, f, oy, ox) for n in (0, g.n - 1) for f in (0, g.f - 1) for oy in (0, g.oh - 1) for ox in (0, g.ow - 1)]
    return np.concatenate([co, np.array(edge)], axis=0)


@functools.lru_cache(maxsize=2)
def random_inputs(family: str, cfg: tuple):
    """x, w, bias, residual (float32, unrounded) drawn as the named test draws them: same seed, same order, same scaling."""
    g = random_geom(family, cfg)
    _, _, has_bias, has_res, act = RANDOM_FAMILIES[family]
    rng = np.random.default_rng(abs(hash(cfg)) % 2 ** 32)
    x = rng.standard_normal((g.n, g.c, g.h, g.w)).astype(np.float32)
    scale = g.r if family == "dw" else np.sqrt(g.cpg * g.r * g.s)
    w = (rng.standard_normal((g.f, g.cpg, g.r, g.s)) / scale).astype(np.float32)
    b = rng.standard_normal((g.f,)).astype(np.float32) if has_bias else None
    res = rng.standard_normal((g.n, g.f, g.oh, g.ow)).astype(np.float32) if has_res else None
    return SimpleNamespace(g=g, x=x, w=w, bias=b, res=res, act=act)


# Routes that round conv + bias to the storage type BEFORE the residual is added — a stated decision of the kernel
# (csrc/gemm256p_kernel.h, epilogue_conv: "y = act(round(conv + bias) + residual) — the arithmetic of the reference's separate Conv
# and Add kernels"). With a residual their result carries one more rounding, of the intermediate p = conv + bias, by at most one
# storage ulp of p: u |p|. The shared bound stays as it is for everything else; this term is added for these routes' residual cases
# only (derived from that one extra rounding, not fitted).
ROUNDS_BEFORE_RESIDUAL = ("pixel_gemm",)


def bound_for(dt, want, absum, pre=None):
    """pre: conv + bias in fp64, for the residual cases of ROUNDS_BEFORE_RESIDUAL only."""
    return U[dt] * np.abs(want) + 2.0 ** -17 * absum + (0.0 if pre is None else U[dt] * np.abs(pre))


@functools.lru_cache(maxsize=2)
def random_reference(family: str, cfg: tuple, dt: str):
    """Rounded operands, want (fp64 of the rounded operands) and the per-element bound. Layers above MAX_RANDOM_MACS: at
    `coords` [k, 4] only (one fp64 dot product each, R.conv2d_at), want / absum / bound then [k]; else coords is None."""
    inp = random_inputs(family, cfg)
    g = inp.g
    rd = lambda a: None if a is None else R.round_to(a, dt)  # noqa: E731
    x, w, b, res = rd(inp.x), rd(inp.w), rd(inp.bias), rd(inp.res)
    if g.macs <= MAX_RANDOM_MACS:
        coords = None
        pre = epilogue(R.conv2d(x, w, *g.args), b, None, 0)
        want = epilogue(pre, None, res, inp.act)
        absum = epilogue(R.conv2d(np.abs(x), np.abs(w), *g.args), None if b is None else np.abs(b), None if res is None else np.abs(res), 0)
    else:
        coords = sample_coords(g)
        at = lambda a: 0.0 if a is None else a[tuple(coords.T)]  # noqa: E731
        bf = lambda a: 0.0 if a is None else a[coords[:, 1]]  # noqa: E731
        pre = R.conv2d_at(x, w, coords, *g.args) + bf(b)
        want = np.maximum(pre + at(res), 0) if inp.act else pre + at(res)
        absum = R.conv2d_at(np.abs(x), np.abs(w), coords, *g.args) + np.abs(bf(b)) + np.abs(at(res))
    return SimpleNamespace(g=g, x=x, w=w, bias=b, res=res, act=inp.act, coords=coords, want=want, absum=absum, pre=pre,
                           bound=bound_for(dt, want, absum),
                           bound_rounded_pre=bound_for(dt, want, absum, pre) if res is not None else None)


# ------------------------------------------------------------------------------------------------------------------------
# mutations: the same convolution with one defect
# ------------------------------------------------------------------------------------------------------------------------
FILTER_TILE = 64
INDEX_MUTATIONS = ("drop_corner", "neighbour_last_slot", "pad_row_leak", "swap_channels", "drop_k_tail", "double_k_tile",
                   "bias_of_previous_filter", "skip_residual_last_pixel")
NUMERICS_MUTATION = "round_partials_64"


def _corner_tap(g):
    """The first tap that is inside the image at the output corner (OH - 1, OW - 1), or None."""
    for rr in range(g.r):
        for ss in range(g.s):
            iy, ix = (g.oh - 1) * g.sh - g.ph + rr * g.dh, (g.ow - 1) * g.sw - g.pw + ss * g.dw
            if 0 <= iy < g.h and 0 <= ix < g.w:
                return rr, ss, iy, ix
    return None


def _k_order(g):
    """Flat K index of w[:, c, r, s] in the tap-major order of the ROWTAP form: k = (r S + s) C + c."""
    c, rr, ss = np.meshgrid(np.arange(g.cpg), np.arange(g.r), np.arange(g.s), indexing="ij")
    return (rr * g.s + ss) * g.cpg + c


def inside_k(g):
    """The terms of the centre output that are not padding: what a sum there really adds up (K, unless the plane is smaller than
    the window — a 3 x 3 window on a 1 x 1 plane has K = 9 C and C terms)."""
    oy, ox = g.oh // 2, g.ow // 2
    rows = sum(0 <= oy * g.sh - g.ph + rr * g.dh < g.h for rr in range(g.r))
    cols = sum(0 <= ox * g.sw - g.pw + ss * g.dw < g.w for ss in range(g.s))
    return g.cpg * rows * cols


def mutation_applies(g, mut: str, has_bias: bool = False, has_res: bool = False) -> bool:
    return {
        "drop_corner": _corner_tap(g) is not None,
        "neighbour_last_slot": g.oh * g.ow >= 9,
        "pad_row_leak": g.n * g.c > 1 and (g.oh - 1) * g.sh + (g.r - 1) * g.dh >= g.ph + g.h,
        "swap_channels": g.cpg >= 2,
        "drop_k_tail": g.k % 32 != 0,
        "double_k_tile": True,
        "bias_of_previous_filter": has_bias and g.f >= 2,
        "skip_residual_last_pixel": has_res,
        NUMERICS_MUTATION: inside_k(g) > 64,
    }[mut]


def forward(g, x, w, bias=None, res=None, act=0, mut=None):
    """fp64 conv + epilogue; `mut` names the defect (None: the correct result)."""
    x, w = np.asarray(x, dtype=np.float64), np.asarray(w, dtype=np.float64)
    wm = w
    if mut == "swap_channels":  # the first and the last channel of the last 32-block change places
        a, b = (g.cpg - 1) // 32 * 32, g.cpg - 1
        wm = w.copy()
        wm[:, [a, b]] = w[:, [b, a]]
    elif mut == "drop_k_tail":  # the last K mod 32 terms
        wm = np.where(_k_order(g)[None] >= g.k - g.k % 32, 0.0, w)
    elif mut == "double_k_tile":  # the first 32 terms are counted twice
        wm = np.where(_k_order(g)[None] < 32, 2.0 * w, w)
    y = conv_any(g, x, wm, leak=mut == "pad_row_leak")
    if mut == "drop_corner":  # one (c, tap) at one output corner only
        rr, ss, iy, ix = _corner_tap(g)
        ch = (np.arange(g.f) // g.fpg) * g.cpg + g.cpg - 1
        y[:, :, g.oh - 1, g.ow - 1] -= w[None, :, g.cpg - 1, rr, ss] * x[:, ch, iy, ix]
    elif mut == "neighbour_last_slot":  # the last slot of every 8-pixel run holds its neighbour's value
        flat = y.reshape(g.n, g.f, -1).copy()
        p = np.arange(7, flat.shape[-1], 8)
        flat[..., p] = flat[..., np.where(p + 1 < flat.shape[-1], p + 1, p - 1)]
        y = flat.reshape(y.shape)
    if mut == "bias_of_previous_filter" and bias is not None:  # in the last filter tile
        bias = np.array(bias, dtype=np.float64)
        f0 = max(1, (g.f - 1) // FILTER_TILE * FILTER_TILE)
        bias[f0:] = np.asarray(bias)[f0 - 1:-1].copy()
    out = epilogue(y, bias, res, 0)
    if mut == "skip_residual_last_pixel" and res is not None:
        out[:, :, -1, -1] -= res[:, :, -1, -1]
    return np.maximum(out, 0) if act else out


def forward_rounded_partials(g, x, w, dt, bias=None, res=None, act=0, every=64):
    """The numerics mutation: the running sum is rounded to the storage type every `every` terms (K in (c, r, s) order)."""
    xp = padded(g, np.asarray(x, dtype=np.float64))
    y = np.zeros((g.n, g.f, g.oh, g.ow))
    for gi in range(g.groups):
        cols = np.stack([xp[:, gi * g.cpg + c, rr * g.dh: rr * g.dh + (g.oh - 1) * g.sh + 1: g.sh,
                            ss * g.dw: ss * g.dw + (g.ow - 1) * g.sw + 1: g.sw]
                         for c in range(g.cpg) for rr in range(g.r) for ss in range(g.s)], axis=1)  # [n, K, oh, ow]
        wk = np.asarray(w, dtype=np.float64)[gi * g.fpg:(gi + 1) * g.fpg].reshape(g.fpg, g.k)
        acc = np.zeros((g.n, g.fpg, g.oh, g.ow))
        for k0 in range(0, g.k, every):
            acc = R.round_to(acc + np.einsum("nkhw,fk->nfhw", cols[:, k0:k0 + every], wk[:, k0:k0 + every], optimize=True), dt)
        y[:, gi * g.fpg:(gi + 1) * g.fpg] = acc
    return epilogue(y, bias, res, act)
