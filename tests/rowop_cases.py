"""Selector inputs, a derived per-element bound and a Python mirror of the dispatch for the row operators of csrc/rowops.hip:
Softmax, LayerNorm, RMSNorm and the fused add_norm / bias_add_norm. numpy and oracle/ref_ops.py only: imports without a GPU.

route(op, dt, outer, n, inner, aligned, add, has_pre) restates softmax_dispatch, norm_dispatch, launch_norm_rows and
add_norm_dispatch: VEC = 4 (f32) / 8 (16-bit), chunks of 64 VEC elements, the 4096-byte limit of norm_rows_kernel with its chunk-width
rule (8-byte chunks where c8 = ceil(bytes / 512) is 1 or 3 and leaves fewer idle lanes), 256 VEC {2, 4, 8} for the block-resident
kernels and the row groups (R = 4 up to 1024 bytes, R = 2 up to 3072, from 4096 aligned rows on). A case DECLARES the route it was
built for (from the ranges written in _softmax_ranges and _norm_ranges); tests/test_rowop_selectors_cpu.py holds the mirror against the
declarations and the table against everything the mirror can return, tests/test_rowop_route_cpu.py holds the mirror against the planner
of csrc/rowops_route.h (ops.rowop_plan_route), and the GPU file asserts after every launch that ops.rowop_last_route names the declared route.

Template values the kernels accept that no route names, so they are not built:
  norm_wave_kernel<.., ALIGNED = true> aligned rows up to 4096 bytes all go to norm_rows_kernel
  norm_wave_kernel<.., ROWS = 2>       likewise never named
(softmax_wave_kernel's ROWS = 8 and norm_rows_kernel's ROWS = 2 lost their launch sites with the hooks that chose them:
docs/history/rowops_dropped_hooks.md.)

Inputs. Every launch is made of PATTERN rows: a family holds P rows [P, n] with their expectation and bound, and row r of a launch
is pattern (base + r) mod P (consecutive rows always differ). A case with few rows walks the patterns in rounds (base = round *
outer); a case with thousands of rows holds every pattern many times and costs one small fp64 pass.
  softmax pair rows   v at p and q = (p + n / 2) mod n, a decoy elsewhere (-inf on even patterns, FINITE_DECOY on odd ones): 0.5 at p
                      and q, 0 elsewhere, written directly. v = 0: exact in every dtype. v = 1000: within the bound.
  softmax single rows v = 0 at p alone: 1 at p, exact. (Two equal maxima hide a maximum that misses one of them; one does not.)
  softmax mask rows   -inf over the first element, the first 256, one thread's share, one wave's share; random finite elsewhere.
  norm pair rows      c everywhere, + a at p, - a at q (c in {0, 3}, a in {1, 2, 4}): sum, mean and centred values exact in fp32 in
                      any order; the expectation is the fp64 closed form. eps = 0 and n = 2 4^k: rstd = 2^k / a, the f32 result exact.
  add-norm rows       the same rows split as a + b and (a + pre) + b with integer parts (every sum exact), and rows whose two
                      roundings matter (ROUNDING): the oracle is the norm of round_to(round_to(a + pre) + b).
  random rows         the inputs of test_softmax_vs_oracle, test_layernorm_vs_oracle and test_rmsnorm_vs_oracle of
                      tests/test_gpu_rowops.py with their seeds, the three smallest shapes per route.
p walks targets(): 0 and n - 1, both sides of every chunk boundary k 64 VEC, the last VEC elements, both sides of the thread-stride
boundaries of the block kernels in the first and the last trip (never thinned), and both sides of every lane boundary of the first
and the last chunk (thinned evenly where the patterns would exceed ROWS * MAX_ROUNDS).

The bound: |got - want| <= u_out |want| + E_f32 (1 + u_out) (+ u 2^-14 for f16), u_out one rounding to the output type. E_f32 is
derived in softmax_bound / norm_bound from the operations the kernels perform; replay_* repeat each kernel's order of operations in
numpy float32 (serial per-thread partials, the DPP wave tree, the 4-wave combine, two-pass norms) and the CPU file holds the fp32
value of every replay at or below half of 2^-24 |want| + E_f32, the bound of an f32 launch (replay_bound), and the value rounded to
storage within the whole bound. Nothing here comes from what a kernel returned.

MUTATIONS: numpy forwards with one named defect each, for the CPU file to prove that the inputs see them.
"""
from __future__ import annotations

import functools
from types import SimpleNamespace

import numpy as np

from attention_cases import assert_within, worst_ratio  # noqa: F401  (the checker of the attention selectors, shared)
from matmul_cases import assert_exact  # noqa: F401
from oracle import ref_ops as R

DTS = ("f32", "f16", "bf16")
VEC = {"f32": 4, "f16": 8, "bf16": 8}
SIZE = {"f32": 4, "f16": 2, "bf16": 2}
U_OUT = {"f32": 2.0 ** -24, "f16": 2.0 ** -11, "bf16": 2.0 ** -8}
U32 = 2.0 ** -24
SLACK = 512           # elements of fill on both sides of every operand and of the output
SLACK_FILL = 1000.0   # around the inputs: a read outside a row changes a max or a mean visibly
OUT_FILL = 7.0
FINITE_DECOY = {"f32": -1e30, "bf16": -1e30, "f16": -30000.0}
NUM_CU = 256          # the persistent grids are sized for it; fewer CUs only make the second trips longer
ROWS = 5              # rows of a selector launch: a partial group of 4 waves
MAX_ROUNDS = 8        # as matmul_cases.MAX_ROUNDS: above it the lane boundaries are thinned, the required targets never
MAX_REQUIRED_ROUNDS = 40
EPS = 1e-5
LOG2E32 = np.float32(1.4426950408889634)


def ceil_div(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------------------------------------------------
# the mirror of the dispatch
# ------------------------------------------------------------------------------------------------------------------------
def _rows_route(dt, n, add):
    rb = n * SIZE[dt]
    c16, c8 = ceil_div(rb, 1024), ceil_div(rb, 512)
    use8 = c8 in (1, 3) and (c8 * 512 - rb) < (c16 * 1024 - rb)
    return f"norm_rows/B8/C{c8}/ADD{add}" if use8 else f"norm_rows/B16/C{min(c16, 4)}/ADD{add}"


def route(op, dt, outer, n, inner=1, aligned=True, add=0, has_pre=False):
    """The kernel a launch takes. op: "softmax", "layer_norm", "rms_norm" (one dispatch, RMS a template flag) or "add_norm" (add is
    then 1, has_pre says whether a row `pre` is added first). aligned: every pointer on a 16-byte boundary."""
    v, rb = VEC[dt], n * SIZE[dt]
    al = aligned and n % v == 0
    how = "aligned" if al else "unaligned"
    chunks, bch = ceil_div(n, 64 * v), ceil_div(n, 256 * v)
    if op == "softmax":
        if inner != 1:
            return "softmax_strided"
        rpw = 1 if (not al or outer < 4096) else (4 if rb <= 1024 else (2 if rb <= 3072 else 1))
        if chunks <= 1:
            return f"softmax_wave/C1/{how}/R{rpw if al else 1}"
        if chunks <= 2:
            return f"softmax_wave/C2/{how}/R{rpw if al else 1}"
        if chunks <= 8:
            return f"softmax_wave/C{4 if chunks <= 4 else 8}/{how}/R1"
        if al and bch <= 8:
            return f"softmax_blockreg/C{4 if bch <= 4 else 8}"
        return f"softmax_block/{how}"
    if op in ("layer_norm", "rms_norm"):
        assert not add
        if al and rb <= 4096:
            return _rows_route(dt, n, 0)
        if chunks <= 4:
            return f"norm_wave/C{1 if chunks <= 1 else (2 if chunks <= 2 else 4)}/unaligned/R1"
        if al and bch <= 8:
            return f"norm_blockreg/C{2 if bch <= 2 else (4 if bch <= 4 else 8)}/ADD0"
        return f"norm_block/{how}"
    assert op == "add_norm" and add
    a = 2 if has_pre else 1
    if al and rb <= 4096:
        return _rows_route(dt, n, a)
    if al and bch <= 8:
        return f"norm_blockreg/C{2 if bch <= 2 else (4 if bch <= 4 else 8)}/ADD{a}"
    return "chain"


def scan_routes(op, dt, has_pre=False):
    """Every route the mirror can return for (op, dt): n on every multiple of VEC up to past the last threshold and next to it,
    pointers aligned and not, few rows and many, both inner."""
    v, out = VEC[dt], set()
    ns = sorted({m + d for m in range(0, 2048 * v + 3 * v, v) for d in (-1, 0, 1) if m + d >= 1})
    for n in ns:
        for al in (True, False):
            for outer in (5, 4096):
                out.add(route(op, dt, outer, n, 1, al, int(op == "add_norm"), has_pre))
    if op == "softmax":
        out.add(route(op, dt, 5, 7, 3))
    return out


# ------------------------------------------------------------------------------------------------------------------------
# the case table: (route, [n lo .. n hi]) written from the kernels' limits, cases generated from the ranges
# ------------------------------------------------------------------------------------------------------------------------
def _softmax_ranges(dt):
    """route stem -> (lo, hi) of n, hi None: unbounded."""
    v = VEC[dt]
    ch = 64 * v
    out = {}
    for c, prev in ((1, 0), (2, 1), (4, 2), (8, 4)):
        out[f"softmax_wave/C{c}"] = (prev * ch + 1, c * ch)
    out["softmax_blockreg/C4"] = (8 * ch + 1, 1024 * v)
    out["softmax_blockreg/C8"] = (1024 * v + 1, 2048 * v)
    out["softmax_block/aligned"] = (2048 * v + 1, None)
    out["softmax_block/unaligned"] = (8 * ch + 1, None)
    return out


def _norm_ranges(dt):
    v, s = VEC[dt], SIZE[dt]
    out = {"norm_rows/B8/C1": (1, 512 // s), "norm_rows/B16/C1": (512 // s + 1, 1024 // s), "norm_rows/B8/C3": (1024 // s + 1, 1536 // s),
           "norm_rows/B16/C2": (1536 // s + 1, 2048 // s), "norm_rows/B16/C3": (2048 // s + 1, 3072 // s),
           "norm_rows/B16/C4": (3072 // s + 1, 4096 // s)}
    ch = 64 * v
    for c, prev in ((1, 0), (2, 1), (4, 2)):
        out[f"norm_wave/C{c}"] = (prev * ch + 1, c * ch)
    for c, prev in ((2, 1), (4, 2), (8, 4)):
        out[f"norm_blockreg/C{c}"] = (prev * 256 * v + 1, c * 256 * v)
    out["norm_block/aligned"] = (2048 * v + 1, None)
    out["norm_block/unaligned"] = (4 * ch + 1, None)
    return out


CASES: dict = {}
_FIRST: set = set()


def _case(op, dt, route_, n, outer, form="aligned", inner=1, add=0, kinds=("pair",), rms=False, eps=EPS):
    """form: "aligned", "odd_n" (n % VEC != 0) or "offset" (an aligned n in views one element into an aligned buffer)."""
    name = f"{op}{'-rms' if rms else ''}{'-add%d' % add if add else ''}-{dt}-n{n}-o{outer}" + (f"-i{inner}" if inner != 1 else "") + \
           ("" if form == "aligned" else f"-{form}") + ("" if eps == EPS else "-eps0") + "".join(f"-{k}" for k in kinds if k != "pair")
    assert name not in CASES, name
    assert n * outer * inner * SIZE[dt] <= 128 << 20, name
    first = outer == ROWS and eps == EPS and (op, rms, add, dt, route_) not in _FIRST  # the scale / bias forms: once per route
    if first:
        _FIRST.add((op, rms, add, dt, route_))
    CASES[name] = SimpleNamespace(name=name, op=op, dt=dt, route=route_, n=n, outer=outer, form=form, inner=inner, add=add,
                                  kinds=tuple(kinds), rms=rms, eps=eps, aligned=form != "offset", all_forms=first and not rms)
    return CASES[name]


def _up(x, v):
    return ceil_div(x, v) * v


def _ns_aligned(lo, hi, dt, stride):
    """smallest, largest, and one whose last chunk (of `stride` elements) holds 5 lanes only."""
    v = VEC[dt]
    lo = _up(lo, v)
    if hi is None:
        return [lo, lo + 3 * stride + 5 * v]
    mid = (hi - 1) // stride * stride + 5 * v
    return sorted({lo, hi, mid if lo < mid < hi else lo})


def _ns_odd(lo, hi, dt, stride):
    """the same with n % VEC != 0: the last chunk partial for one lane, whole for some, absent for the others."""
    v = VEC[dt]
    if hi is None:
        return [lo, _up(lo, v) + 3 * stride + 5 * v + 3]
    hi = hi - 1 if hi % v == 0 else hi
    mid = (hi - 1) // stride * stride + 5 * v + 3
    return sorted({lo if lo % v else lo + 1, hi, mid if lo < mid < hi else hi}) if hi >= lo and hi % v else []


def _build_table():
    for dt in DTS:
        v = VEC[dt]
        ch = 64 * v
        # ---- softmax
        for stem, (lo, hi) in _softmax_ranges(dt).items():
            kern = stem.split("/")[0]
            stride = ch if kern == "softmax_wave" else 256 * v
            kinds = ("pair", "single", "pair1000", "mask")
            if kern == "softmax_wave":
                c = int(stem[-1])
                for n in _ns_aligned(lo, hi, dt, stride):
                    _case("softmax", dt, f"{stem}/aligned/R1", n, ROWS, kinds=kinds)
                _case("softmax", dt, f"{stem}/aligned/R1", _up(lo, v), 1)
                if c <= 2:  # the row groups: 4096 + 3 rows, and a second trip of their persistent loop
                    r = 4 if c == 1 else 2
                    _case("softmax", dt, f"{stem}/aligned/R{r}", _up(lo, v), 4096 + 3)
                    _case("softmax", dt, f"{stem}/aligned/R{r}", hi, 4096 + 3, kinds=("pair", "single", "mask"))
                    _case("softmax", dt, f"{stem}/aligned/R{r}", _up(lo, v), 8 * 4 * r * NUM_CU + 3)
                if c == 4:
                    _case("softmax", dt, f"{stem}/aligned/R1", _up(lo, v), 8 * 4 * NUM_CU + 3)
                for n in _ns_odd(lo, hi, dt, stride):
                    _case("softmax", dt, f"{stem}/unaligned/R1", n, ROWS, "odd_n", kinds=kinds)
                for n in (_up(lo, v), hi):
                    _case("softmax", dt, f"{stem}/unaligned/R1", n, ROWS, "offset", kinds=kinds)
                _case("softmax", dt, f"{stem}/unaligned/R1", lo if lo % v else lo + 1, 1, "odd_n")
                if c == 1:
                    _case("softmax", dt, f"{stem}/unaligned/R1", 1, 8 * 4 * NUM_CU + 3, "odd_n")
                    _case("softmax", dt, f"{stem}/unaligned/R1", v, 4096 + 3, "offset")  # many rows and still R = 1
            elif stem.endswith("unaligned"):
                for n in _ns_odd(lo, hi, dt, stride):
                    _case("softmax", dt, stem, n, ROWS, "odd_n", kinds=kinds)
                _case("softmax", dt, stem, _up(lo, v), ROWS, "offset", kinds=kinds)
                _case("softmax", dt, stem, lo if lo % v else lo + 1, 1, "odd_n")
                _case("softmax", dt, stem, lo if lo % v else lo + 1, 8192 + 3, "odd_n")
            else:
                for n in _ns_aligned(lo, hi, dt, stride):
                    _case("softmax", dt, stem, n, ROWS, kinds=kinds)
                _case("softmax", dt, stem, _up(lo, v), 1)
                if stem == "softmax_blockreg/C4":  # one second trip per grid-stride loop, at the smallest n of the kernel (the scalar
                    # block kernel takes its second trip on unaligned rows: aligned ones start at 2048 VEC, 256 MiB for 8195 rows)
                    _case("softmax", dt, stem, _up(lo, v), 8192 + 3)
        for inner, outer, dim in ((2, 3, 5), (3, 2, 33), (64, 2, 7), (65, 3, 16)):
            _case("softmax", dt, "softmax_strided", dim, outer, inner=inner, kinds=("pair", "single", "pair1000", "mask"))
        _case("softmax", dt, "softmax_strided", 3, 16384 * 256 // 65 + 7, inner=65)  # the grid-stride loop: more than 16384 blocks
        # ---- LayerNorm / RMSNorm
        for rms in (False, True):
            op = "rms_norm" if rms else "layer_norm"
            for stem, (lo, hi) in _norm_ranges(dt).items():
                kern = stem.split("/")[0]
                if kern == "norm_rows":
                    b = int(stem.split("/")[1][1:])
                    stride = 64 * b // SIZE[dt]
                    for n in _ns_aligned(lo, hi, dt, stride):
                        _case(op, dt, f"{stem}/ADD0", n, ROWS, rms=rms)
                    _case(op, dt, f"{stem}/ADD0", _up(lo, v), 1, rms=rms)
                    if stem == "norm_rows/B8/C1":
                        _case(op, dt, f"{stem}/ADD0", v, 4 * 4 * NUM_CU + 3, rms=rms)
                elif kern == "norm_wave":
                    for n in _ns_odd(lo, hi, dt, ch):
                        _case(op, dt, f"{stem}/unaligned/R1", n, ROWS, "odd_n", rms=rms)
                    for n in (_up(lo, v), hi):
                        _case(op, dt, f"{stem}/unaligned/R1", n, ROWS, "offset", rms=rms)
                    _case(op, dt, f"{stem}/unaligned/R1", lo if lo % v else lo + 1, 1, "odd_n", rms=rms)
                    if stem == "norm_wave/C1":
                        _case(op, dt, f"{stem}/unaligned/R1", 1, 8 * 4 * NUM_CU + 3, "odd_n", rms=rms)
                elif kern == "norm_blockreg":
                    for n in _ns_aligned(lo, hi, dt, 256 * v):
                        _case(op, dt, f"{stem}/ADD0", n, ROWS, rms=rms)
                    _case(op, dt, f"{stem}/ADD0", _up(lo, v), 1, rms=rms)
                    if stem == "norm_blockreg/C2":
                        _case(op, dt, f"{stem}/ADD0", _up(lo, v), 8192 + 3, rms=rms)
                elif stem.endswith("unaligned"):
                    for n in _ns_odd(lo, hi, dt, 256 * v):
                        _case(op, dt, stem, n, ROWS, "odd_n", rms=rms)
                    _case(op, dt, stem, _up(lo, v), ROWS, "offset", rms=rms)
                    _case(op, dt, stem, lo if lo % v else lo + 1, 1, "odd_n", rms=rms)
                    _case(op, dt, stem, lo if lo % v else lo + 1, 8192 + 3, "odd_n", rms=rms)
                else:
                    for n in _ns_aligned(lo, hi, dt, 256 * v):
                        _case(op, dt, stem, n, ROWS, rms=rms)
                    _case(op, dt, stem, _up(lo, v), 1, rms=rms)
            # eps = 0, n = 2 4^k: rstd a power of two
            for k in range(1, 7):
                n = 2 * 4 ** k
                _case(op, dt, route(op, dt, ROWS, n), n, ROWS, rms=rms, eps=0.0)
        # ---- add_norm / bias_add_norm
        for rms in (False, True):
            for add in (1, 2):
                kinds = ("pair", "rounding")
                for stem, (lo, hi) in _norm_ranges(dt).items():
                    kern = stem.split("/")[0]
                    if kern == "norm_rows":
                        b = int(stem.split("/")[1][1:])
                        for n in _ns_aligned(lo, hi, dt, 64 * b // SIZE[dt])[:1 if rms else 3]:  # (RMS: a template flag of the same code)
                            _case("add_norm", dt, f"{stem}/ADD{add}", n, ROWS, add=add, rms=rms, kinds=kinds)
                        if stem == "norm_rows/B8/C1":
                            _case("add_norm", dt, f"{stem}/ADD{add}", _up(lo, v), 1, add=add, rms=rms)
                            _case("add_norm", dt, f"{stem}/ADD{add}", v, 4 * 4 * NUM_CU + 3, add=add, rms=rms)
                    elif kern == "norm_blockreg":
                        lo_ = max(lo, 4096 // SIZE[dt] + 1)
                        for n in _ns_aligned(lo_, hi, dt, 256 * v)[:1 if rms else 3]:
                            _case("add_norm", dt, f"{stem}/ADD{add}", n, ROWS, add=add, rms=rms, kinds=kinds)
                        if stem == "norm_blockreg/C2":
                            _case("add_norm", dt, f"{stem}/ADD{add}", _up(lo_, v), 1, add=add, rms=rms)
                            if not rms:
                                _case("add_norm", dt, f"{stem}/ADD{add}", _up(lo_, v), 8192 + 3, add=add, rms=rms)
                # the chain: unaligned n (a wave kernel and the block kernel behind the Add), an offset view, rows above 256 VEC 8
                for n, form in ((33, "odd_n"), (256 * v + 3, "odd_n"), (2 * ch, "offset"), (2048 * v + v, "aligned")):
                    _case("add_norm", dt, "chain", n, ROWS, form, add=add, rms=rms, kinds=kinds)


_build_table()


def cases_of(op=None, dt=None):
    return [c for c in CASES.values() if (op is None or c.op == op) and (dt is None or c.dt == dt)]


def norm_route_of(cs):
    """The kernel that does the arithmetic (for the depth of its sums): behind the chain it is the in-place norm."""
    if cs.route != "chain":
        return cs.route
    return route("rms_norm" if cs.rms else "layer_norm", cs.dt, cs.outer, cs.n, 1, cs.aligned)


# ------------------------------------------------------------------------------------------------------------------------
# targets
# ------------------------------------------------------------------------------------------------------------------------
def _sides(n, step, first_last_only=False):
    ts = list(range(step, n, step))
    if first_last_only and ts:
        ts = [ts[0], ts[-1]]
    return {x for t in ts for x in (t - 1, t)}


def targets(route_, dt, n):
    """-> (required, optional) positions of p, sorted."""
    v = VEC[dt]
    ch = 64 * v
    req = {0, n - 1} | _sides(n, ch) | set(range(max(0, n - v), n))
    kern = route_.split("/")[0]
    if kern in ("softmax_block", "norm_block"):
        req |= _sides(n, 256, True)
    if kern in ("softmax_blockreg", "norm_blockreg"):
        req |= _sides(n, 256 * v, True)
    if kern == "softmax_strided":
        return sorted(range(n)), []
    last = (n - 1) // ch * ch
    opt = ({x for x in _sides(min(n, ch), v)} | {last + x for x in _sides(n - last, v)}) - req
    return sorted(req), sorted(opt)


def pattern_targets(route_, dt, n):
    req, opt = targets(route_, dt, n)
    room = ROWS * MAX_ROUNDS - len(req)
    if room <= 0:
        opt = []
    elif len(opt) > room:
        opt = [opt[i] for i in sorted({int(i) for i in np.linspace(0, len(opt) - 1, room)})]
    t = sorted(set(req) | set(opt))
    assert set(req) <= set(t) and ceil_div(len(t), ROWS) <= MAX_REQUIRED_ROUNDS, (route_, dt, n, len(t))
    return np.array(t)


# ------------------------------------------------------------------------------------------------------------------------
# depth of the sums, from the route
# ------------------------------------------------------------------------------------------------------------------------
def depth(route_, dt, n):
    """(serial additions of one thread, further additions of the wave tree and the 4-wave combine, online trips or 0)."""
    parts = route_.split("/")
    kern, v = parts[0], VEC[dt]
    if kern in ("softmax_wave", "norm_wave"):
        return int(parts[1][1:]) * v, 6, 0
    if kern == "norm_rows":
        return int(parts[2][1:]) * int(parts[1][1:]) // SIZE[dt] + 1, 6, 0
    if kern in ("softmax_blockreg", "norm_blockreg"):
        return int(parts[1][1:]) * v, 9, 0
    if kern == "norm_block":
        return ceil_div(n, 256), 9, 0
    if kern == "softmax_block":
        return ceil_div(n, 256), 9, ceil_div(n, 256) + 2
    assert kern == "softmax_strided", route_
    return n, 0, n


# ------------------------------------------------------------------------------------------------------------------------
# the bound
# ------------------------------------------------------------------------------------------------------------------------
K_ARG = 3.0   # roundings of the exponent's argument, each at most 2^-24 |x - m|: the subtraction (or the fma), the product with
#               log2(e), the constant itself (float(log2 e) is off by 0.2 * 2^-24). In the 16-bit wave path the rounding of m log2(e)
#               is the SAME factor on every element of a row and cancels between the numerator and the sum.
K_EXP = 2.0   # expf / v_exp_f32: 1 ulp = 2 * 2^-24


def out_rounding(dt, want, e32):
    b = U_OUT[dt] * np.abs(want) + e32 * (1 + U_OUT[dt])
    return b + (U_OUT[dt] * 2.0 ** -14 if dt == "f16" else 0.0)


def softmax_bound(dt, x, want, route_, n):
    """x, want [P, n] (the softmax axis last), fp64. got = fl(e_i * fl(1 / s)), s the fp32 sum of the e_j, e_j = exp(x_j - m) with
      relative error eps_j <= 2^-24 (K_ARG |x_j - m| + k),  k = K_EXP for the two-pass kernels. The online kernels reach e_j as a
      product of exponentials whose arguments add up to x_j - m exactly (the running maximum only grows), one factor, one multiply
      and one add per trip and per combine step: k = (K_EXP + 2) (trips).
    The sum of positive terms has relative error <= sum_j p_j eps_j + D 2^-24 (p = want, D additions on an element's way); the
    reciprocal is 1 ulp (2 * 2^-24) and the last product one rounding. A weight below 2^-126 may flush to 0: 2^-125 absolute."""
    s, tree, trips = depth(route_, dt, n)
    k = (K_EXP + 2) * trips if trips else K_EXP
    m = x.max(axis=-1, keepdims=True)
    with np.errstate(invalid="ignore"):
        ad = np.where(np.isinf(x), 0.0, np.abs(x - m))  # a -inf element has weight exactly 0
    wsum = (want * ad).sum(axis=-1, keepdims=True)
    rel = U32 * (K_ARG * (ad + wsum) + 2 * k + (s + tree) + 3)
    e32 = want * rel + np.where(np.isinf(x), 0.0, 2.0 ** -125)
    return out_rounding(dt, want, e32), e32


def norm_bound(dt, x, g, b, eps, rms, route_, n):
    """-> want, bound [P, n]. x: the row as the kernel normalises it (for add-norm the stored sum), g, b broadcastable ([n] or [1]).
      mu^ = mu + delta, |delta| <= (D + 1) 2^-24 mean|x|   (D additions on an element's way, the divide by n; 0 for RMSNorm)
      d^ = (x - mu^)(1 + e1);  var^: D additions, the two e1 of a square, the divide by n (or fl(1 / n) and the fma), the add of
      eps and eps itself as a float (1e-5 is off by 0.44 * 2^-24): relative (D + 6) 2^-24 + delta^2 / (var + eps)  (sum (d - delta)^2 = n var + n delta^2: the cross term is sum d = 0)
      rstd^: half of that, + 1 ulp (2 * 2^-24) for inv_sqrt / 1 / sqrtf            =: rho
      y^ = fma(fl(d^ rstd^), g, b): one multiply, one fma
    |y^ - y| <= |d rstd g| (rho + 3 2^-24) + |b| 2^-24 + |delta| rstd |g| (1 + rho)."""
    s, tree, _ = depth(route_, dt, n)
    dd = s + tree
    mu = 0.0 if rms else x.mean(axis=-1, keepdims=True)
    d = x - mu
    var = (d * d).mean(axis=-1, keepdims=True)
    rstd = 1.0 / np.sqrt(var + eps)
    want = d * rstd * g + (0.0 if b is None else b)
    delta = 0.0 if rms else (dd + 1) * U32 * np.abs(x).mean(axis=-1, keepdims=True)
    rho = 0.5 * ((dd + 6) * U32 + delta ** 2 / (var + eps)) + 2 * U32
    e32 = np.abs(d * rstd * g) * (rho + 3 * U32) + (0.0 if b is None else np.abs(b) * U32) + delta * rstd * np.abs(g) * (1 + rho)
    return want, out_rounding(dt, want, e32), e32 * np.ones_like(want)


# ------------------------------------------------------------------------------------------------------------------------
# families of pattern rows
# ------------------------------------------------------------------------------------------------------------------------
def seed_of(*key):
    return [ord(ch) for ch in "|".join(map(str, key))]


def grid_scale(n):
    return 1.0 + (np.arange(n) % 7) / 8.0


def grid_bias(n):
    return (np.arange(n) % 5) - 2.0


SB_FORMS = ("grid", "one", "nobias")


def scale_bias(form, n, rms):
    """g, b as the tensors the launch gets (float64 values, exact in every dtype); b None: no bias (always for RMSNorm, whose weight
    has n elements by its interface)."""
    if rms:
        return grid_scale(n), None
    if form == "grid":
        return grid_scale(n), grid_bias(n)
    if form == "one":
        return np.array([1.25]), np.array([-1.5])
    return grid_scale(n), None


@functools.lru_cache(maxsize=8)
def softmax_pair(route_, dt, n, v, single=False):
    """v at p and q, decoys elsewhere -> x [P, n], want, bound, p, q; exact for v = 0. single: q = p, the row has ONE element above
    the decoys and the expectation is 1 there — with two equal maxima a maximum that misses p is still right, with one it is the
    decoy and the row inf or NaN."""
    t = pattern_targets(route_, dt, n)
    p = t
    q = p if single else (p + n // 2) % n
    P = len(t)
    x = np.where((np.arange(P) % 2 == 0)[:, None], -np.inf, R.round_to(np.array([FINITE_DECOY[dt]]), dt)[0]) * np.ones((P, n))
    x[np.arange(P), p] = v
    x[np.arange(P), q] = v
    want = np.zeros((P, n))
    want[np.arange(P), p] = 0.5
    want[np.arange(P), q] = np.where(p == q, 1.0, 0.5)
    bound, e32 = softmax_bound(dt, x, want, route_, n)
    return SimpleNamespace(kind=("single" if single else "pair") if v == 0 else "pair1000", x=x, want=want, bound=bound, e32=e32, p=p, q=q, exact=v == 0)


def thread_of(route_, dt, n):
    """element -> the thread (0 .. 255) of a block kernel that holds it; for a wave kernel the lane."""
    kern, v = route_.split("/")[0], VEC[dt]
    e = np.arange(n)
    if kern in ("softmax_blockreg", "norm_blockreg"):
        return (e // v) % 256
    if kern in ("softmax_block", "norm_block"):
        return e % 256
    return (e // v) % 64


@functools.lru_cache(maxsize=8)
def softmax_mask(route_, dt, n):
    """-inf over: the first element; the first 256; the elements t, t + 256, ...; the share of thread 1 and of thread 255 as THIS
    kernel deals the row out; the share of its second wave (threads 64 .. 127; of a wave kernel: lanes 16 .. 31); everything but the
    last element. Masks that would cover a whole row are left out (the oracle gives NaN for such a row as well)."""
    rng = np.random.default_rng(seed_of("mask", route_, dt, n))
    th = thread_of(route_, dt, n)
    e = np.arange(n)
    wave_kernel = route_.split("/")[0] in ("softmax_wave", "softmax_strided")
    masks = [e < 1, e < 256, e % 256 == 3, th == 1, th == 255 if not wave_kernel else th == 63,
             (th >= 16) & (th < 32) if wave_kernel else (th >= 64) & (th < 128), e < n - 1, e > 0]
    masks = [m for m in masks if m.any() and not m.all()]
    if not masks:
        return None
    x = R.round_to(rng.standard_normal((len(masks), n)) * 3, dt)
    x[np.array(masks)] = -np.inf
    with np.errstate(invalid="ignore"):
        want = R.softmax(x, -1)
    bound, e32 = softmax_bound(dt, x, want, route_, n)
    return SimpleNamespace(kind="mask", x=x, want=want, bound=bound, e32=e32, p=None, q=None, exact=False)


def pair_rows(route_, dt, n):
    t = pattern_targets(route_, dt, n)
    P = len(t)
    p, q = t, (t + n // 2) % n
    c = np.where(np.arange(P) % 2 == 0, 0.0, 3.0)
    a = np.take((1.0, 2.0, 4.0), np.arange(P) % 3)
    x = c[:, None] * np.ones((P, n))
    x[np.arange(P), p] += a
    x[np.arange(P), q] -= a  # n = 1: p = q, the row is c
    return x, p, q, c, a


@functools.lru_cache(maxsize=8)
def norm_pair(route_, dt, n, rms, eps, form):
    """c + a at p, c - a at q. want: the closed form (mean c, variance 2 a^2 / n; RMS: mean square c^2 + 2 a^2 / n)."""
    x, p, q, c, a = pair_rows(route_, dt, n)
    g, b = scale_bias(form, n, rms)
    want, bound, e32 = norm_bound(dt, x, g, b, eps, rms, route_, n)
    if n > 1:  # the closed form, against the dense pass above
        ms = (c * c if rms else 0.0) + 2 * a * a / n
        closed = (x - (0.0 if rms else c[:, None])) / np.sqrt(ms + eps)[:, None] * g + (0.0 if b is None else b)
        assert np.allclose(closed, want, rtol=1e-12, atol=1e-12)
        want = closed
    exact = eps == 0.0 and dt == "f32" and not rms  # (RMSNorm: c = 3 makes the mean square no power of four)
    return SimpleNamespace(kind="pair", x=x, g=g, b=b, want=want, bound=bound, e32=e32, p=p, q=q, exact=exact, eps=eps, rms=rms, form=form)


ROUNDING = {"bf16": 2.0 ** -8, "f16": 2.0 ** -11, "f32": 2.0 ** -24}  # half an ulp of 1: round(round(1 + h) + h) = 1, unrounded 1 + 2 h


@functools.lru_cache(maxsize=8)
def add_rows(route_, dt, n, rms, add, kind, form):
    """The operands of (a + pre) + b (add = 2) or a + b (add = 1).
    "pair": the pair rows split into integer parts: every sum exact, the expectation that of norm_pair.
    "rounding": at every third position a = 1 (add = 2: pre = h, b = h, on every other of them b = 2 h, where the ORDER of the two
      sums shows; add = 1: a = 1 + 2 h, b = h, a tie that rounds to even, up), h = ROUNDING: a kernel that keeps the unrounded sum
      normalises 1 + 2 h (1 + 3 h) there. Elsewhere the pair rows."""
    x, p, q, c, a_ = pair_rows(route_, dt, n)
    j = np.arange(n)
    b2 = ((j % 3) - 1.0) * np.ones_like(x)
    pre = (j % 2).astype(np.float64) if add == 2 else None
    a = x - b2 - (pre if pre is not None else 0.0)
    if kind == "rounding":
        h = ROUNDING[dt]
        hot = (j % 3 == 1) & (j != p[:, None]) & (j != q[:, None])
        b2 = np.where(hot, h, b2)
        if add == 2:
            hotcol = j % 3 == 1
            b2 = np.where(hot & (j % 6 == 4), 2 * h, b2)  # round(round(1 + h) + 2 h) = 1 + 2 h, but round(round(1 + 2 h) + h) = 1 + 4 h
            a = np.where(hot, 1.0, x - b2 - (j % 2))  # (p and q on a hot column: integers + h, rounded by the oracle like the rest)
            pre = np.where(hotcol, h, pre)
        else:
            a = np.where(hot, 1.0 + 2 * h, a)
    for o in (a, b2, pre):
        assert o is None or np.array_equal(R.round_to(o, dt), o)
    mid = R.round_to(a + pre, dt) if pre is not None else a
    s = R.round_to(mid + b2, dt)
    if kind == "pair":
        assert np.array_equal(s, x)
    g, b = scale_bias(form, n, rms)
    want, bound, e32 = norm_bound(dt, s, g, b, EPS, rms, route_, n)
    return SimpleNamespace(kind=kind, a=a, pre=pre, b2=b2, x=s, g=g, b=b, want=want, bound=bound, e32=e32, p=p, q=q, exact=False, eps=EPS, rms=rms,
                           form=form)


def families(cs):
    """The families of a case, in the order of its kinds. The first 5-row case of every norm route (its smallest n) runs its pair rows
    with every scale / bias form — a grid of distinct values, one-element tensors, no bias —, the others with the grid."""
    nr = norm_route_of(cs)
    out = []
    for kind in cs.kinds:
        if cs.op == "softmax":
            fam = {"pair": lambda: softmax_pair(cs.route, cs.dt, cs.n, 0.0), "single": lambda: softmax_pair(cs.route, cs.dt, cs.n, 0.0, True),
                   "pair1000": lambda: softmax_pair(cs.route, cs.dt, cs.n, 1000.0),
                   "mask": lambda: softmax_mask(cs.route, cs.dt, cs.n)}[kind]()
            if fam is not None:
                out.append(fam)
        elif cs.op == "add_norm":
            for form in (SB_FORMS if kind == "pair" and cs.all_forms else SB_FORMS[:1]):
                out.append(add_rows(nr, cs.dt, cs.n, cs.rms, cs.add, kind, form))
        else:
            for form in (SB_FORMS if cs.all_forms else SB_FORMS[:1]):
                out.append(norm_pair(nr, cs.dt, cs.n, cs.rms, cs.eps, form))
    return out


def launches(cs, fam):
    """The pattern index of every row of every launch of (case, family): [rounds][rows] (for the strided softmax rows = outer *
    inner columns). Few rows: as many rounds as the patterns need; many rows: one launch that holds them all."""
    P = fam.x.shape[0]
    rows = cs.outer * cs.inner
    if cs.outer == 1 and cs.inner == 1:
        return [np.array([0])]
    nr = ceil_div(P, rows)
    return [(r * rows + np.arange(rows)) % P for r in range(nr)]


def covered(cs, fam):
    return set(int(fam.p[i]) for idx in launches(cs, fam) for i in idx) if fam.p is not None else set()


def replay_bound(fam):
    """What the fp32 value a kernel hands to its store is held to, whatever the storage type: the f32 form of the bound, 2^-24 |want|
    + E_f32. (E_f32 counts every fp32 rounding once and a single rounding reaches its half ulp, so E_f32 alone is met with equality
    by the last fma of a LayerNorm; the f32 bound counts that rounding a second time as the rounding to the output type.)"""
    return np.zeros_like(fam.want) if fam.exact else U32 * np.abs(fam.want) + fam.e32


# ------------------------------------------------------------------------------------------------------------------------
# random inputs of tests/test_gpu_rowops.py
# ------------------------------------------------------------------------------------------------------------------------
SOFTMAX_SHAPES = [((4, 12, 64, 512), 3), ((7, 1000), 1), ((3, 5, 17), 2), ((6, 33, 40), 1), ((5, 64, 3), 0), ((2, 2048), 1),
                  ((3, 5000), 1), ((2, 20000), 1), ((16, 1), 1), ((1, 7), 0), ((4, 513), 1), ((3, 8192), 1), ((2, 16384), 1),
                  ((3, 4104), 1), ((300, 6144), 1)]
LN_SHAPES = [((4, 512, 768), -1), ((5, 7, 33), -1), ((4, 3, 8, 16), 2), ((9, 1024), 1), ((3, 4096), 1), ((2, 10000), 1), ((6, 1), 1),
             ((4, 257), 1), ((5, 8192), 1), ((3, 16384), 1), ((2, 12288), 1), ((300, 5120), 1)]
RMS_SHAPE = (2, 37, 4096)
PER_ROUTE = 3


def _split(shape, axis):
    axis %= len(shape)
    return int(np.prod(shape[:axis])), shape[axis], int(np.prod(shape[axis + 1:]))


def random_params():
    """[(op, dt, shape, axis, with_bias, route)]: per (op, dt, route) the PER_ROUTE smallest shapes of the old lists."""
    out = []
    for dt in DTS:
        by = {}
        for shape, axis in SOFTMAX_SHAPES:
            o, n, i = _split(shape, axis)
            by.setdefault(route("softmax", dt, o, n, i), []).append((shape, axis))
        for r, lst in by.items():
            out += [("softmax", dt, s, a, False, r) for s, a in sorted(lst, key=lambda sa: int(np.prod(sa[0])))[:PER_ROUTE]]
        by = {}
        for shape, axis in LN_SHAPES:
            o = int(np.prod(shape[:axis % len(shape)]))
            n = int(np.prod(shape[axis % len(shape):]))
            by.setdefault(route("layer_norm", dt, o, n), []).append((shape, axis))
        for r, lst in by.items():
            for s, a in sorted(lst, key=lambda sa: int(np.prod(sa[0])))[:PER_ROUTE]:
                out += [("layer_norm", dt, s, a, wb, r) for wb in (True, False)]
        out.append(("rms_norm", dt, RMS_SHAPE, -1, False, route("rms_norm", dt, 74, 4096)))
    return out


@functools.lru_cache(maxsize=2)
def random_reference(op, dt, shape, axis, with_bias, route_):
    """Storage-rounded inputs (float64), want, bound — the generator, seed and scaling of the named test."""
    if op == "softmax":
        x = R.round_to((np.random.default_rng(5).standard_normal(shape) * 3).astype(np.float32), dt)
        o, n, i = _split(shape, axis)
        xm = np.moveaxis(x, axis, -1)
        want = R.softmax(xm, -1)
        bound, e32 = softmax_bound(dt, xm, want, route_, n)
        return SimpleNamespace(x=x, g=None, b=None, want=np.ascontiguousarray(np.moveaxis(want, -1, axis)),
                               bound=np.ascontiguousarray(np.moveaxis(bound, -1, axis)),
                               e32=np.ascontiguousarray(np.moveaxis(e32, -1, axis)), axis=axis)
    if op == "layer_norm":
        rng = np.random.default_rng(9)
        x = (rng.standard_normal(shape) * 2 + 0.5).astype(np.float32)
        nshape = shape[axis:]
        g = rng.standard_normal(nshape).astype(np.float32)
        b = rng.standard_normal(nshape).astype(np.float32) if with_bias else None
    else:
        rng = np.random.default_rng(3)
        x = rng.standard_normal(shape).astype(np.float32)
        g, b = rng.standard_normal(shape[-1:]).astype(np.float32), None
    x, g, b = R.round_to(x, dt), R.round_to(g, dt), None if b is None else R.round_to(b, dt)
    n = int(np.prod(shape[axis % len(shape):]))
    x2 = x.reshape(-1, n)
    want, bound, e32 = norm_bound(dt, x2, g.ravel(), None if b is None else b.ravel(), EPS, op == "rms_norm", route_, n)
    ref = R.rms_norm(x, g, EPS) if op == "rms_norm" else R.layer_norm(x, g, b, EPS, axis)
    assert np.allclose(want.reshape(shape), ref, rtol=1e-11, atol=1e-11)
    return SimpleNamespace(x=x, g=g, b=b, want=ref, bound=bound.reshape(shape), e32=e32.reshape(shape), axis=axis)


def release():
    for cached in (softmax_pair, softmax_mask, norm_pair, add_rows, random_reference):
        cached.cache_clear()


# ------------------------------------------------------------------------------------------------------------------------
# float32 replays of the kernels' order of operations
# ------------------------------------------------------------------------------------------------------------------------
F = np.float32
_L = np.arange(64)
_PERMS = (_L ^ 1, _L ^ 2, (_L & ~7) | (7 - (_L & 7)), (_L & ~15) | (15 - (_L & 15)))


def _wave_reduce(v, op):
    """wave_sum / wave_max over the last axis [.., 64]: quad swaps, row_half_mirror, row_mirror, row_bcast15 into rows 1 and 3,
    row_bcast31 into rows 2 and 3, lane 63."""
    v = np.asarray(v, dtype=F)
    for perm in _PERMS:
        v = op(v, v[..., perm])
    r = v.reshape(v.shape[:-1] + (4, 16)).copy()
    l15 = r[..., :, 15].copy()
    r[..., 1, :] = op(r[..., 1, :], l15[..., 0, None])
    r[..., 3, :] = op(r[..., 3, :], l15[..., 2, None])
    l31 = r[..., 1, 15].copy()
    r[..., 2, :] = op(r[..., 2, :], l31[..., None])
    r[..., 3, :] = op(r[..., 3, :], l31[..., None])
    return r[..., 3, 15]


def _reduce(part, op, threads):
    """part [P, threads]: the wave tree, then for 256 threads ((w0 + w1) + w2) + w3."""
    if threads == 64:
        return _wave_reduce(part, op)
    w = _wave_reduce(part.reshape(part.shape[0], 4, 64), op)
    return op(op(op(w[:, 0], w[:, 1]), w[:, 2]), w[:, 3])


def _deal(x, route_, dt, fill):
    """x [P, n] -> [P, threads, S]: what each thread holds, in the order it walks it; slots past the row hold `fill`."""
    parts = route_.split("/")
    kern, v, (P, n) = parts[0], VEC[dt], x.shape
    if kern in ("softmax_wave", "norm_wave", "norm_rows"):
        c = int(parts[1][1:]) if kern != "norm_rows" else int(parts[2][1:])
        w = v if kern != "norm_rows" else int(parts[1][1:]) // SIZE[dt]
        pad = np.full((P, c * 64 * w), fill)
        pad[:, :n] = x
        return pad.reshape(P, c, 64, w).transpose(0, 2, 1, 3).reshape(P, 64, c * w), 64
    if kern in ("softmax_blockreg", "norm_blockreg"):
        c = int(parts[1][1:])
        pad = np.full((P, c * 256 * v), fill)
        pad[:, :n] = x
        return pad.reshape(P, c, 256, v).transpose(0, 2, 1, 3).reshape(P, 256, c * v), 256
    t = ceil_div(n, 256)
    pad = np.full((P, t * 256), fill)
    pad[:, :n] = x
    return pad.reshape(P, t, 256).transpose(0, 2, 1), 256


def _undeal(y, route_, dt, n):
    parts = route_.split("/")
    kern, v, P = parts[0], VEC[dt], y.shape[0]
    if kern in ("softmax_wave", "norm_wave", "norm_rows"):
        c = int(parts[1][1:]) if kern != "norm_rows" else int(parts[2][1:])
        w = v if kern != "norm_rows" else int(parts[1][1:]) // SIZE[dt]
        return y.reshape(P, 64, c, w).transpose(0, 2, 1, 3).reshape(P, -1)[:, :n]
    if kern in ("softmax_blockreg", "norm_blockreg"):
        c = int(parts[1][1:])
        return y.reshape(P, 256, c, v).transpose(0, 2, 1, 3).reshape(P, -1)[:, :n]
    return y.transpose(0, 2, 1).reshape(P, -1)[:, :n]


def _fma(a, b, c):
    return (np.asarray(a, dtype=np.float64) * np.asarray(b, dtype=np.float64) + np.asarray(c, dtype=np.float64)).astype(F)


def _fast_exp(d):
    """__expf: v_exp_f32 of the fp32 product with log2(e)."""
    with np.errstate(invalid="ignore", over="ignore"):
        return np.exp2((np.asarray(d, dtype=F) * LOG2E32).astype(F)).astype(F)


def _serial_sum(a):
    return np.cumsum(np.asarray(a, dtype=F), axis=-1, dtype=F)[..., -1]


def _online(vals):
    """The online recurrence over the last axis of vals [.., T] (with the -inf guard: no rescale where the maximum stays)."""
    m = np.full(vals.shape[:-1], -np.inf, dtype=F)
    s = np.zeros(vals.shape[:-1], dtype=F)
    with np.errstate(invalid="ignore"):
        for k in range(vals.shape[-1]):
            v = vals[..., k]
            nm = np.maximum(m, v)
            s = (s * np.where(m == nm, F(1), _fast_exp(m - nm))).astype(F) + np.where(v == nm, F(1) * ~np.isinf(v), _fast_exp(v - nm))
            s = s.astype(F)
            m = nm
    return m, s


def _rescale(s, m, gm):
    with np.errstate(invalid="ignore"):
        return (s * np.where(m == gm, F(1), _fast_exp(m - gm))).astype(F)


def replay_softmax(x, route_, dt, rounded=True):
    """x [P, n] (storage values) -> what the kernel of `route_` stores, float64 of the storage type; rounded = False: the fp32 value
    it rounds (what E_f32 bounds)."""
    rd = (lambda y, _: np.asarray(y, dtype=np.float64)) if not rounded else R.round_to
    x = np.asarray(x, dtype=F)
    kern, n = route_.split("/")[0], x.shape[1]
    with np.errstate(invalid="ignore", over="ignore"):
        if kern == "softmax_strided":
            m, s = _online(x)
            y = _fast_exp(x - m[:, None]) * (F(1) / s)[:, None]
            return rd(y.astype(F), dt)
        d, threads = _deal(x, route_, dt, -np.inf)
        d = d.astype(F)
        if kern == "softmax_block":
            m, s = _online(d)
            mw = m.reshape(-1, 4, 64)
            gm = _wave_reduce(mw, np.maximum)
            sw = _wave_reduce(_rescale(s.reshape(-1, 4, 64), mw, gm[..., None]), np.add)
            bm = gm.max(axis=1)
            sw = _rescale(sw, gm, bm[:, None])
            bs = ((sw[:, 0] + sw[:, 1]) + sw[:, 2]) + sw[:, 3]
            y = _fast_exp(x - bm[:, None]) * (F(1) / bs)[:, None]
            return rd(y.astype(F), dt)
        m = _reduce(d.max(axis=-1), np.maximum, threads)[:, None, None]
        if kern == "softmax_blockreg":
            e = _fast_exp(d - m)
        elif dt == "f32":
            e = np.exp((d - m).astype(F)).astype(F)
        else:
            e = np.exp2(_fma(d, LOG2E32, -(m * LOG2E32).astype(F))).astype(F)
        s = _reduce(_serial_sum(e), np.add, threads)
        y = (e * (F(1) / s)[:, None, None]).astype(F)
    return rd(_undeal(y, route_, dt, n), dt)


def replay_norm(x, g, b, eps, rms, route_, dt, rounded=True):
    """x [P, n], g / b [n] or [1] (b None) -> the stored result of the kernel of `route_` (two passes, the row in registers)."""
    x = np.asarray(x, dtype=F)
    P, n = x.shape
    kern = route_.split("/")[0]
    d, threads = _deal(x, route_, dt, 0.0)
    d = d.astype(F)
    live, _ = _deal(np.ones((P, n)), route_, dt, 0.0)
    fn = F(n)
    mu = np.zeros(P, dtype=F)
    rows = kern == "norm_rows"
    if not rms:
        if rows:  # float2 pairs: the two halves summed apart, then x + y
            pr = d.reshape(P, 64, -1, 2)
            part = (_serial_sum(pr[..., 0].copy()) + _serial_sum(pr[..., 1].copy())).astype(F)
        else:
            part = _serial_sum(d)
        mu = (_reduce(part, np.add, threads) / fn).astype(F)
    cen = np.where(live > 0, (d - mu[:, None, None]).astype(F), F(0))

    def sq(a):  # q = fma(d, d, q) along the last axis
        q = np.zeros(a.shape[:-1], dtype=F)
        for k in range(a.shape[-1]):
            q = _fma(a[..., k], a[..., k], q)
        return q
    if rows:
        pl = int(route_.split("/")[1][1:]) // SIZE[dt]  # elements of one chunk per lane
        pr = cen.reshape(P, 64, -1, 2)
        head, last = pr[:, :, : (pr.shape[2] - pl // 2)], pr[:, :, (pr.shape[2] - pl // 2):]
        q2 = (sq(head[..., 0]) + sq(head[..., 1])).astype(F) if head.shape[2] else np.zeros((P, 64), dtype=F)
        ql = (sq(last[..., 0]) + sq(last[..., 1])).astype(F)
        tot = _reduce((q2 + ql).astype(F), np.add, threads)
        var = _fma(tot, F(1) / fn, F(eps))
        rstd = (1.0 / np.sqrt(var.astype(np.float64))).astype(F)  # inv_sqrt: under 1 ulp
    else:
        tot = _reduce(sq(cen), np.add, threads)
        var = ((tot / fn).astype(F) + F(eps)).astype(F)
        rstd = (F(1) / np.sqrt(var).astype(F)).astype(F)
    gd, _ = _deal(np.broadcast_to(np.asarray(g, dtype=np.float64), (P, n)), route_, dt, 0.0)
    bd, _ = _deal(np.broadcast_to(np.zeros(1) if b is None else np.asarray(b, dtype=np.float64), (P, n)), route_, dt, 0.0)
    y = _fma((cen * rstd[:, None, None]).astype(F), gd.astype(F), bd.astype(F))
    return R.round_to(_undeal(y, route_, dt, n), dt) if rounded else _undeal(y, route_, dt, n).astype(np.float64)


# ------------------------------------------------------------------------------------------------------------------------
# mutations: the same operators in fp64 with one defect each
# ------------------------------------------------------------------------------------------------------------------------
SOFTMAX_MUTATIONS = ("drop_from_sum", "drop_from_max", "tail_zero_filled", "tail_unstored", "group_row_from_first", "online_no_guard")
NORM_MUTATIONS = ("drop_from_mean", "drop_from_var", "padding_adds_mu2", "scale_off_by_a_chunk", "scale1_read_as_vector",
                  "bias1_ignored", "eps_dropped")
ADD_MUTATIONS = ("sum_not_rounded", "b_before_pre", "fallback_reads_overwritten_b")


def padded(route_, dt, n):
    """Slots of the register image of a wave kernel past the row end."""
    parts = route_.split("/")
    if parts[0] in ("softmax_wave", "norm_wave"):
        return int(parts[1][1:]) * 64 * VEC[dt] - n
    if parts[0] == "norm_rows":
        return int(parts[2][1:]) * 64 * int(parts[1][1:]) // SIZE[dt] - n
    return 0


def dropped_index(route_, dt, n):
    """The element a "drop" defect loses: the first element of the last chunk (a loop that ends one chunk early for lane 0)."""
    return (n - 1) // (64 * VEC[dt]) * (64 * VEC[dt])


def mutation_applies(mut, cs, fam):
    v = VEC[cs.dt]
    kern = norm_route_of(cs).split("/")[0]
    return {
        "drop_from_sum": cs.n > 1, "drop_from_max": cs.n > 1,
        "tail_zero_filled": padded(cs.route, cs.dt, cs.n) > 0,
        "tail_unstored": cs.n % v != 0 and cs.n > v,
        "group_row_from_first": cs.route.endswith(("R2", "R4")),
        "online_no_guard": kern in ("softmax_block", "softmax_strided"),
        "drop_from_mean": not cs.rms and cs.n > 1, "drop_from_var": cs.n > 1,
        "padding_adds_mu2": not cs.rms and padded(norm_route_of(cs), cs.dt, cs.n) > 0,
        "scale_off_by_a_chunk": cs.n > 64 * v and np.size(getattr(fam, "g", 0)) > 1,
        "scale1_read_as_vector": np.size(getattr(fam, "g", 0)) == 1 and cs.n > 1,
        "bias1_ignored": getattr(fam, "b", None) is not None and np.size(fam.b) == 1,
        "eps_dropped": cs.n > 1 and cs.eps != 0.0,
        "sum_not_rounded": fam.kind == "rounding", "b_before_pre": fam.kind == "rounding" and cs.add == 2,
        "fallback_reads_overwritten_b": cs.route == "chain" and cs.add == 2,
    }[mut]


def softmax_forward(x, route_, dt, mut=None, rows_per_group=1):
    """x [rows, n] -> fp64 softmax over the last axis as a kernel with the defect `mut` would return it."""
    x = np.asarray(x, dtype=np.float64)
    n = x.shape[1]
    k = dropped_index(route_, dt, n)
    if mut == "group_row_from_first":
        x = x[np.arange(x.shape[0]) // rows_per_group * rows_per_group]
    keep = np.ones(n, dtype=bool)
    keep[k] = False
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        if mut == "online_no_guard":  # per thread, as written: exp(m - nm) with m = nm = -inf is NaN
            d = x[:, None, :] if route_ == "softmax_strided" else _deal(x, route_, dt, np.nan)[0]
            m = np.full(d.shape[:2], -np.inf)
            s = np.zeros(d.shape[:2])
            for t in range(d.shape[2]):
                v = d[..., t]
                ok = ~np.isnan(v)  # slots past the row are not visited
                nm = np.where(ok, np.maximum(m, np.where(ok, v, m)), m)
                s = np.where(ok, s * np.exp(m - nm) + np.exp(v - nm), s)
                m = nm
            gm = m.max(axis=1, keepdims=True)
            tot = (s * np.exp(m - gm)).sum(axis=1, keepdims=True)
            return np.exp(x - gm) / tot
        m = x.max(axis=1, keepdims=True)
        if mut == "drop_from_max":
            m = x[:, keep].max(axis=1, keepdims=True)
        pads = padded(route_, dt, n) if mut == "tail_zero_filled" else 0
        if pads:
            m = np.maximum(m, 0.0)
        e = np.exp(x - m)
        s = e.sum(axis=1, keepdims=True) + pads * np.exp(0.0 - m)
        if mut == "drop_from_sum":
            s = e[:, keep].sum(axis=1, keepdims=True)
        y = e / s
    if mut == "tail_unstored":
        y[:, n - n % VEC[dt]:] = OUT_FILL
    return y


def norm_forward(x, g, b, eps, rms, route_, dt, mut=None):
    """x [rows, n], g / b as the tensors handed over -> fp64 LayerNorm / RMSNorm with the defect `mut`."""
    x = np.asarray(x, dtype=np.float64)
    n = x.shape[1]
    k = dropped_index(route_, dt, n)
    keep = np.ones(n, dtype=bool)
    keep[k] = False
    mu = 0.0 if rms else x.mean(axis=1, keepdims=True)
    if mut == "drop_from_mean":
        mu = x[:, keep].sum(axis=1, keepdims=True) / n
    d = x - mu
    q = (d * d).sum(axis=1, keepdims=True)
    if mut == "drop_from_var":
        q = (d[:, keep] ** 2).sum(axis=1, keepdims=True)
    if mut == "padding_adds_mu2":
        q = q + padded(route_, dt, n) * mu * mu
    with np.errstate(divide="ignore", invalid="ignore"):  # (a constant row without eps: inf, NaN — a miss like any other)
        rstd = 1.0 / np.sqrt(q / n + (0.0 if mut == "eps_dropped" else eps))
    gv = np.broadcast_to(np.asarray(g, dtype=np.float64), (n,))
    if mut == "scale_off_by_a_chunk":
        gv = np.concatenate([gv, np.full(64 * VEC[dt], SLACK_FILL)])[64 * VEC[dt]:][:n]
    if mut == "scale1_read_as_vector":  # what follows a one-element tensor is its slack
        gv = np.concatenate([gv[:1], np.full(n - 1, SLACK_FILL)])
    bv = np.zeros(n) if b is None or (mut == "bias1_ignored" and np.size(b) == 1) else np.broadcast_to(np.asarray(b, dtype=np.float64), (n,))
    with np.errstate(invalid="ignore"):
        return d * rstd * gv + bv


def add_forward(fam, route_, dt, mut=None, alias=None):
    """The rows an add-norm normalises, with the defect, then the correct norm of them."""
    a, b2, pre = fam.a, fam.b2, fam.pre
    if mut == "sum_not_rounded":
        s = a + b2 + (pre if pre is not None else 0.0)
    elif mut == "b_before_pre":
        s = R.round_to(R.round_to(a + b2, dt) + pre, dt)
    elif mut == "fallback_reads_overwritten_b":  # out aliases b: y = a + pre is stored over b, then y + "b" adds y to itself
        mid = R.round_to(a + pre, dt)
        s = R.round_to(mid + mid, dt) if alias == "b" else R.round_to(mid + b2, dt)
    else:
        s = R.round_to((R.round_to(a + pre, dt) if pre is not None else a) + b2, dt)
    return norm_forward(s, fam.g, fam.b, fam.eps, fam.rms, route_, dt)


def bound_of(fam):
    """The bound a family's rows are held to: 0 where the expectation is exact."""
    return np.zeros_like(fam.want) if fam.exact or fam.bound is None else fam.bound
