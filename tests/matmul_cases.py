"""Selector inputs and a per-element bound for the MatMul kernels (csrc/gemm.hip, gemm256.hip, gemm256p_*.hip, gemm128w.hip, gemm32.hip;
the nine variants of csrc/gemm_route.h, the head-split store, the grouped launch and the cast path of an fp32 MatMul).

With random N(0, 1) operands one product is O(1) and the sum of K of them O(sqrt(K)): the size of every tolerance the random tests can
afford. A product that is dropped, counted twice or read from a neighbour is seen by luck. A GEMM is linear in each operand, so the
inputs built here make ONE product carry a whole output element and the result exact in f16, bf16 and f32, whatever the order of the
sum, the split-K factor or the tile walk. numpy and oracle/ref_ops.py only: imports without a GPU.

Column selectors
  B is zero except b[k_j, j] = v_j, v_j from {1, -1, 2, -1/2}: C[i, j] = v_j a[i, k_j] exactly (every other product is 0 * finite, fp32
  sums of zeros are exact, a product with a power of two does not round). A: random normal rounded to storage, magnitudes below 2^-6
  pushed up to 2^-6 (nothing rests on how a matrix instruction treats f16 subnormals); fp32 keeps its full mantissa.
Row selectors
  the roles swapped: a[i, k_i] = v_i, B dense: C[i, j] = v_i b[k_i, j]. They exercise B's addressing as column selectors do A's.
Grid mode (every mode with a real bias)
  the dense operand holds multiples of 1/4 up to 4, the bias multiples of 1/8 up to 4: v a + bias is a multiple of 1/8 of magnitude at
  most 12 — 8 significant bits, exact in bf16 however the kernel rounds.
K targets (required_k / k_targets), from the kernels' own constants: 0 and K - 1; both sides of every multiple of 8, 32, 64 and 128;
  the first and the last element of a K tail (K % 64 for the 16-bit tile kernels, K % 32 for fast32 and the generic kernel); both sides
  of every split-K slice boundary, computed as launch256_splitk does (per = ceil(nk / splits), the last slice possibly shorter); for
  wave128 both sides of every k-step (32) — which holds the cache-line pairs (64), the blocks of four k-steps (128) and the last three
  k-steps of K, the final block. Round r gives column (row) j of batch b the target T[(r cnt + j + 5 b) mod |T|]. Above MAX_ROUNDS
  rounds the 8- and then the 32-boundaries are thinned (wave128: the 8-boundaries only); 0, K - 1, the 64- and 128-boundaries, the tail
  and the slice boundaries never — where those alone need more rounds (m = 3 rows and K = 1000) the rounds are as many as they need.
Diagonal cases: one per kernel at its smallest one-tile shape, k_j = (j + r) mod K for r in 0 .. KT - 1 (KT: the kernel's K-tile, 32
  for the generic kernel, fast32 and wave128's k-step, 64 otherwise): every k of a K-tile meets every column position mod KT.

Everything is compared with `==` (-0 equals +0, NaN equals nothing); `assert_exact` names the first wrong element and the k it should
have selected.

Per-element bound for random inputs: exactly tests/test_gpu_matmul.py::test_matmul_16bit_variants',
      bound = u |want| + 2^-17 S,   S = |A| |B| + |bias| of THAT element,   u = 2^-7 (bf16), 2^-10 (f16)
`want` is the fp64 product of the rounded operands. random_reference rebuilds the inputs of test_persistent_gemm_walks_several_tiles,
test_matmul_splitk_heuristic_shapes and test_matmul_headline_shape_sampled_rows with their own seeds; products too large for a dense
fp64 reference in seconds are referenced on sampled ROWS (whole rows: every column tile, the edges of the row tiles included).

MUTATIONS: numpy GEMMs with one named defect each, for tests/test_matmul_selectors_cpu.py to prove that the selectors see them.
Nothing here comes from what a kernel returned.
"""
from __future__ import annotations

import functools
from types import SimpleNamespace

import numpy as np

from attention_cases import assert_within, worst_ratio  # noqa: F401  (the checker of the attention selectors, shared)
from oracle import ref_ops as R

U = {"f16": 2.0 ** -10, "bf16": 2.0 ** -7}
SLACK = 512           # elements of fill on both sides of every operand and of the output
SLACK_FILL = 1000.0   # around A, B and the bias: a read outside an operand shows as +-1000 v
OUT_FILL = 7.0        # the output block and its guard regions before the launch
FLOOR = 2.0 ** -6
VALUES = (1.0, -1.0, 2.0, -0.5)
MAX_ROUNDS = 6        # as conv_cases.MAX_TAP_ROUNDS
MAX_REQUIRED_ROUNDS = 16  # where the targets that are never thinned need more than MAX_ROUNDS by themselves
VARIANTS = ("generic64", "fast128_glds", "tile256", "tile256_splitk", "persist256", "persist192", "persist128", "fast32", "wave128")
LAYOUTS = {"nn": (False, False), "nt": (False, True), "tn": (True, False), "tt": (True, True)}
ALL, K_MAJOR_A = ("nn", "nt", "tn", "tt"), ("nn", "nt")
# the K-tile whose tail a kernel zero-fills, and the period of the diagonal cases
K_TILE = {"generic64": 32, "fast32": 32, "wave128": 32, "fast128_glds": 64, "tile256": 64, "tile256_splitk": 64, "persist256": 64,
          "persist192": 64, "persist128": 64}

# epilogue modes: name -> (grid inputs, bias form: None / "zero" / "n" / "mn" / "1" / "bmn" / "m1", act)
MODES = {
    "plain": (False, None, 0),
    "zero_bias_relu": (False, "zero", 1),
    "bias": (True, "n", 0),
    "bias_relu": (True, "n", 1),
    # the bias forms of test_matmul_bias_broadcast_forms (matmul.cc:86-118), on the kernels that take them
    "bias_mn": (True, "mn", 0),
    "bias_1": (True, "1", 1),
    "bias_bmn": (True, "bmn", 0),
    "bias_m1": (True, "m1", 1),
}
BASIC = ("plain", "zero_bias_relu", "bias", "bias_relu")
FORMS = ("bias_mn", "bias_1", "bias_bmn", "bias_m1")
F16S, F32 = ("f16", "bf16"), ("f32",)


def bias_shape(form, b, m, n):
    return {"zero": (n,), "n": (n,), "mn": (m, n), "1": (1,), "bmn": (b, m, n), "m1": (m, 1)}[form]


def bias_strides(form, m, n):
    """(batch, m, n) strides in elements, as infini_rocm_matmul_plan broadcasts the form into C."""
    return {"zero": (0, 0, 1), "n": (0, 0, 1), "mn": (0, n, 1), "1": (0, 0, 0), "bmn": (m * n, n, 1), "m1": (0, 1, 0)}[form]


# ------------------------------------------------------------------------------------------------------------------------
# the case table
# ------------------------------------------------------------------------------------------------------------------------
CASES: dict = {}


def _case(name, shape, variant, report, layouts=ALL, dts=F16S, modes=BASIC, *, splits=None, env=None, runs=1, shared_b=False,
          shared_a=False, a_lo=0, ct=None, head=None, grouped=False, diag=False, only=None):
    """shape (b, m, n, k); `variant`: what set_matmul_variant is given; `report`: what the launch must report (and the planner answers
    for 256 CUs); `splits`: the planner's split-K factor where the report is tile256_splitk; `ct`: the compute type of an fp32 MatMul
    ("bf16" / "fp16": dts then names the type the VALUES are exact in, storage is fp32); `a_lo`: A starts that many bytes off a
    16-byte boundary. A (layout, mode) whose contract fails would silently run another kernel: it is left out here, never skipped.
    `only`: the (dtype, layout, mode) groups that are LAUNCHED where that is not the whole product (the multi-tile shapes: 17 M outputs a
    launch); the CPU file proves the whole product all the same."""
    b, m, n, k = shape
    assert name not in CASES and report in VARIANTS
    CASES[name] = SimpleNamespace(name=name, b=b, m=m, n=n, k=k, variant=variant, report=report, layouts=tuple(layouts), dts=tuple(dts),
                                  modes=tuple(modes), splits=splits, env=dict(env or {}), runs=runs, shared_b=shared_b,
                                  shared_a=shared_a or grouped, a_lo=a_lo, ct=ct, head=head, grouped=grouped, diag=diag,
                                  kt=K_TILE[report], macs=b * m * n * k,
                                  groups=tuple(only) if only is not None else tuple((d, l, mo) for d in dts for l in layouts for mo in modes))
    assert all(d in dts and l in layouts and mo in modes for d, l, mo in CASES[name].groups)


# generic64: any shape, stride and alignment; 16-bit and fp32
_case("generic-77x53x41", (1, 77, 53, 41), 0, "generic64", modes=BASIC + FORMS)  # nothing aligned
_case("generic-3x130x72x64", (3, 130, 72, 64), 0, "generic64", modes=BASIC + FORMS)
_case("generic32-77x53x41", (1, 77, 53, 41), 0, "generic64", dts=F32, modes=BASIC + FORMS)
_case("generic32-3x7x1000", (1, 3, 7, 1000), 0, "generic64", dts=F32)
_case("generic-misaligned-a", (1, 128, 128, 64), 1, "generic64", a_lo=8)  # forced fast128: A 8 bytes off sends it to the generic kernel
_case("generic-diag", (1, 64, 64, 32), 0, "generic64", layouts=("nn", "tt"), modes=("plain",), diag=True)
# fast128: 128 x 128 x 64 LDS-DMA tiles, K tail zero-filled
_case("fast128-one-tile", (1, 128, 128, 64), 1, "fast128_glds")
_case("fast128-ragged-3kt", (1, 200, 136, 192), 1, "fast128_glds")  # three K-tiles through the double buffer
_case("fast128-k72", (1, 128, 128, 72), 1, "fast128_glds")
_case("fast128-k8", (1, 64, 72, 8), 1, "fast128_glds")
_case("fast128-ktail32", (2, 136, 200, 160), 1, "fast128_glds")  # K % 64 = 32
_case("fast128-diag", (1, 128, 128, 64), 1, "fast128_glds", layouts=("nn", "tt"), modes=("plain",), diag=True)
# tile256: one 256^2 tile per workgroup, every epilogue (an M-major A needs m % 8 == 0)
_case("tile256-one-tile", (1, 256, 256, 64), 2, "tile256", modes=BASIC + FORMS)
_case("tile256-ragged", (1, 300, 264, 192), 2, "tile256", layouts=K_MAJOR_A, modes=BASIC + FORMS)
_case("tile256-batch3", (3, 130, 72, 64), 2, "tile256", layouts=K_MAJOR_A, modes=BASIC + FORMS)
_case("tile256-diag", (1, 256, 256, 64), 2, "tile256", layouts=("nn", "tt"), modes=("plain",), diag=True)
# tile256_splitk, run twice (the second launch meets the workspace the first one left)
_case("splitk-one-ktile", (1, 256, 256, 64), 3, "tile256_splitk", splits=2, runs=2, modes=BASIC + FORMS)  # two slices asked, one left
_case("splitk-2+1", (1, 300, 264, 192), 3, "tile256_splitk", layouts=K_MAJOR_A, splits=2, runs=2, modes=BASIC + FORMS)
_case("splitk-k1024", (1, 256, 256, 1024), 3, "tile256_splitk", splits=2, runs=2)
_case("splitk-heuristic-k2048", (1, 300, 264, 2048), -1, "tile256_splitk", layouts=K_MAJOR_A, splits=4, runs=2)
_case("splitk-diag", (1, 256, 256, 64), 3, "tile256_splitk", layouts=("nn", "tt"), splits=2, modes=("plain",), diag=True)
# the persistent kernels: one workgroup per CU walks its tiles through one flat K-tile pipeline
for _v, _w in ((4, 256), (5, 192), (6, 128)):
    _p = f"persist{_w}"
    _case(f"{_p}-one-tile", (1, 256, 256, 64), _v, _p)
    _case(f"{_p}-ragged", (1, 300, 200, 192), _v, _p, layouts=K_MAJOR_A)
    # 33 ragged row tiles x 8 / 11 / 16 column tiles: more than 256 tiles, a workgroup walks at least two. K = 64: the B cursor runs
    # two tiles ahead; an odd K-tile count flips the LDS parity
    # (every layout, both dtypes and both modes are launched, spread over the two K; the walk itself depends on none of them)
    _case(f"{_p}-walk-k64", (1, 8200, 2040, 64), _v, _p, layouts=("nn", "nt", "tn"), modes=("plain", "bias_relu"),
          only=[("bf16", "nn", "bias_relu"), ("f16", "nt", "bias_relu"), ("bf16", "tn", "plain")])
    _case(f"{_p}-walk-k192", (1, 8200, 2040, 192), _v, _p, layouts=("nn", "nt", "tn"), modes=("plain", "bias_relu"),
          only=[("f16", "nn", "plain"), ("bf16", "nt", "bias_relu"), ("f16", "tn", "bias_relu")])
    _case(f"{_p}-walk-shared-b", (2, 8200, 2040, 64), _v, _p, layouts=("nn",), dts=("bf16",), modes=("bias_relu",), shared_b=True)
    for _t in (0, 1, 2):  # the tile table shortened: in-place decode, and the hand-over between the two
        _case(f"{_p}-walk-tab{_t}", (1, 8200, 2040, 64), _v, _p, layouts=("nn",), dts=("bf16",), modes=("bias_relu",),
              env={"IROCM_GEMM_TAB_N": _t})
    _case(f"{_p}-diag", (1, 256, 256, 64), _v, _p, layouts=("nn", "tt"), modes=("plain",), diag=True)
# wave128: plain GEMMs on whole 256^2 tiles, K % 128 == 0
_case("wave128-final-block-alone", (1, 256, 256, 128), 8, "wave128", modes=("plain",))
_case("wave128-k256", (1, 256, 256, 256), 8, "wave128", modes=("plain",))
_case("wave128-6tiles-k384", (1, 512, 768, 384), 8, "wave128", modes=("plain",))
_case("wave128-batch3", (3, 512, 256, 384), 8, "wave128", modes=("plain",))
# 17 x 16 = 272 tiles: some workgroups walk two, the first a non-final tile; the last tile-row group is ragged
_case("wave128-272tiles", (1, 4352, 4096, 128), 8, "wave128", modes=("plain",),
      only=[("bf16", "nn", "plain"), ("bf16", "tt", "plain"), ("f16", "nt", "plain"), ("f16", "tn", "plain")])
_case("wave128-diag", (1, 256, 256, 128), 8, "wave128", layouts=("nn", "tt"), modes=("plain",), diag=True)
# fast32: fp32 LDS-DMA tiles, A K-major, K % 4 == 0 with a zero-filled tail in the last 32
_case("fast32-one-tile", (1, 128, 128, 32), 7, "fast32", layouts=K_MAJOR_A, dts=F32, modes=BASIC + FORMS)
_case("fast32-batch3-k100", (3, 130, 132, 100), 7, "fast32", layouts=K_MAJOR_A, dts=F32, modes=BASIC + FORMS)
_case("fast32-k36", (1, 257, 516, 36), 7, "fast32", layouts=K_MAJOR_A, dts=F32)
_case("fast32-k4", (2, 64, 8, 4), 7, "fast32", layouts=K_MAJOR_A, dts=F32)
_case("fast32-tile128", (1, 2048, 1536, 36), 7, "fast32", layouts=K_MAJOR_A, dts=F32, modes=("plain", "bias_relu"))  # the 128^2 form at 256 CUs
_case("fast32-diag", (1, 128, 128, 32), 7, "fast32", layouts=K_MAJOR_A, dts=F32, modes=("plain",), diag=True)
# fp32 operands with compute type "bf16" / "fp16": 16-bit copies, the split-K kernel, fp32 output
for _ct, _dt in (("bf16", "bf16"), ("fp16", "f16")):
    _case(f"cast-{_ct}-one-tile", (1, 256, 256, 64), -1, "tile256_splitk", dts=(_dt,), modes=("plain",), splits=1, ct=_ct)
    _case(f"cast-{_ct}-shared-b", (3, 256, 264, 128), -1, "tile256_splitk", dts=(_dt,), modes=("plain",), splits=1, ct=_ct, shared_b=True)
    _case(f"cast-{_ct}-k1024", (1, 300, 520, 1024), -1, "tile256_splitk", layouts=K_MAJOR_A, dts=(_dt,), modes=("bias_relu",), splits=2,
          ct=_ct)
# head-split store: [m, n] kept as [m / S, n / D, S, D]; forced variants -1 .. 6 and fp32
_HS = {  # variant -> what it resolves to on the two problems (the second has K % 64 != 0: no 256-row kernel)
    "a": ((2, 256, 256, 64), (128, 64), ("fast128_glds", "generic64", "fast128_glds", "tile256", "tile256_splitk", "persist256",
                                         "persist192", "persist128")),
    "b": ((1, 384, 200, 136), (96, 40), ("fast128_glds", "generic64") + ("fast128_glds",) * 6),
}
for _k, (_shape, _sd, _reports) in _HS.items():
    for _v, _r in zip(range(-1, 7), _reports):
        _case(f"headsplit-{_k}-v{_v}", _shape, _v, _r, layouts=("nn",), modes=("plain", "bias_relu"), head=_sd,
              splits=2 if _r == "tile256_splitk" else None)
    _case(f"headsplit-{_k}-f32", _shape, -1, "fast32", layouts=("nn",), dts=F32, modes=("plain", "bias_relu"), head=_sd)
# grouped: three MatMuls of one activation, weights / biases / outputs carved out of slabs with gaps (batch index = member)
GROUPED_GAPS = {"w": 64, "bias": 8, "out": 128}  # as test_matmul_grouped_members_at_a_stride
for _v, _r in ((-1, "fast128_glds"), (2, "tile256"), (4, "persist256"), (5, "persist192"), (6, "persist128")):
    _case(f"grouped-v{_v}", (3, 640, 384, 256), _v, _r, layouts=("nn",), modes=("bias_relu",), grouped=True)


def case_params(diag: bool):
    """(case, dtype) of the table (the diagonal cases apart, or alone); groups_of gives the (layout, mode) each of them launches."""
    return [(name, dt) for name, cs in CASES.items() if cs.diag == diag for dt in cs.dts if groups_of(cs, dt)]


def groups_of(cs, dt):
    return [(lay, mode) for d, lay, mode in cs.groups if d == dt]


def storage_of(cs, dt):
    """The type the tensors are stored in: fp32 for the cast path, whose VALUES are exact in dt."""
    return "f32" if cs.ct is not None else dt


def bias_of(cs, mode):
    return MODES[mode][1]


def plan_args(cs, layout, mode):
    """The keyword arguments of ops.matmul_plan_route for one launch of the case, with the alignment bits the GPU file produces:
    512 elements of slack keep every operand on a 16-byte boundary, the misaligned case has a_lo = 8."""
    ta, tb = LAYOUTS[layout]
    _, form, act = MODES[mode]
    kw = dict(trans_a=ta, trans_b=tb, stride_a=0 if cs.shared_a or cs.b == 1 else cs.m * cs.k,
              stride_b=0 if cs.shared_b or cs.b == 1 else cs.n * cs.k, act=act, variant=cs.variant, a_lo=cs.a_lo)
    if cs.grouped:  # the members' distances in their slabs
        kw.update(stride_b=cs.n * cs.k + GROUPED_GAPS["w"], stride_c=cs.m * cs.n + GROUPED_GAPS["out"])
    if form is not None:
        _, sm, sn = bias_strides(form, cs.m, cs.n)
        kw.update(bias=True, bias_stride_m=sm, bias_stride_n=sn)
    if cs.head is not None:
        kw.update(head_dim=cs.head[1])
    if cs.ct is not None:
        kw.update(compute_type=cs.ct)
    return kw


# ------------------------------------------------------------------------------------------------------------------------
# K targets
# ------------------------------------------------------------------------------------------------------------------------
def _sides(k, step):
    return {x for t in range(step, k, step) for x in (t - 1, t)}


def slice_boundaries(k, splits):
    """The first K index of every split-K slice but the first, as launch256_splitk cuts them: per = ceil(nk / splits) K-tiles of 64 per
    slice, empty slices dropped, the last one possibly shorter."""
    nk = k // 64
    per = -(-nk // splits)
    return [s * 64 for s in range(per, nk, per)]


def required_k(cs):
    """The targets that are never thinned."""
    k = cs.k
    req = {0, k - 1} | _sides(k, 64) | _sides(k, 128)
    if k % cs.kt:
        req |= {k - k % cs.kt, k - 1}
    if cs.splits is not None and cs.splits > 1:
        req |= {x for s in slice_boundaries(k, cs.splits) for x in (s - 1, s)}
    if cs.report == "wave128":  # every k-step; the last three are the final block
        req |= _sides(k, 32)
        assert {k - 96, k - 65, k - 64, k - 33, k - 32, k - 1} <= req
    return sorted(req)


def boundary_k(cs):
    return sorted(set(required_k(cs)) | _sides(cs.k, 8) | _sides(cs.k, 32))


def k_targets(cs, cnt, max_rounds=MAX_ROUNDS):
    req, full = set(required_k(cs)), set(boundary_k(cs))
    if -(-len(full) // cnt) <= max_rounds:
        return sorted(full)
    budget = max_rounds * cnt - len(req)
    if budget <= 0:
        return sorted(req)
    opt32 = sorted(_sides(cs.k, 32) - req)[:budget]
    opt8 = sorted(full - req - set(opt32))
    room = budget - len(opt32)
    pick = [opt8[i] for i in sorted({int(i) for i in np.linspace(0, len(opt8) - 1, room)})] if room > 0 and opt8 else []
    return sorted(req | set(opt32) | set(pick))


def rounds(cs, kind):
    """The selectors of a case: [SimpleNamespace(kind "col" / "row", k [nb, cnt], v [nb, cnt])], nb = 1 for a shared operand. "col":
    column j of B holds v at row k; "row": row i of A holds v at column k."""
    cnt = cs.n if kind == "col" else cs.m
    nb = 1 if (cs.shared_b if kind == "col" else cs.shared_a) else cs.b
    j, bi = np.arange(cnt)[None, :], np.arange(nb)[:, None]
    out = []
    if cs.diag:
        for r in range(cs.kt):
            out.append(SimpleNamespace(kind=kind, k=(j + r + 0 * bi) % cs.k, v=np.take(VALUES, (j + r + bi) % 4)))
        return out
    T = np.array(k_targets(cs, cnt))
    nr = -(-len(T) // cnt)
    assert 1 <= nr <= (MAX_ROUNDS if len(T) > len(required_k(cs)) else MAX_REQUIRED_ROUNDS), (cs.name, kind, nr)
    for r in range(nr):
        out.append(SimpleNamespace(kind=kind, k=T[(r * cnt + j + 5 * bi) % len(T)], v=np.take(VALUES, (j + r + bi) % 4)))
    return out


def onehot(cs, sel):
    """The selector operand, logical: B [nb, k, n] ("col") or A [nb, m, k] ("row"), float32."""
    nb, cnt = sel.k.shape
    x = np.zeros((nb, cnt, cs.k), dtype=np.float32)
    x[np.arange(nb)[:, None], np.arange(cnt)[None, :], sel.k] = sel.v
    return np.ascontiguousarray(x.swapaxes(1, 2)) if sel.kind == "col" else x


# ------------------------------------------------------------------------------------------------------------------------
# values
# ------------------------------------------------------------------------------------------------------------------------
def storage_normal(rng, shape, dt):
    """Random normal rounded to dt, magnitudes below 2^-6 pushed up to 2^-6 (the sign kept); float32 holds every such value."""
    a = R.round_to(rng.standard_normal(shape, dtype=np.float32), dt)
    return np.where(np.abs(a) < FLOOR, np.where(a < 0, -FLOOR, FLOOR), a).astype(np.float32)


def grid_values(rng, shape):
    return (rng.integers(-16, 17, shape) / 4.0).astype(np.float32)


def grid_bias(shape):
    """Multiples of 1/8 up to 4; neighbours along either axis never share a value (a bias read with the wrong stride is a wrong value)."""
    shape = tuple(shape)
    idx = np.arange(int(np.prod(shape))).reshape(shape)
    if len(shape) >= 2:
        idx = idx + 7 * (idx // shape[-1])
    return (((5 * idx + 3) % 65 - 32) / 8.0).astype(np.float32)


def seed_of(name, dt, salt):
    return [salt, sorted(("f16", "bf16", "f32")).index(dt)] + [ord(ch) for ch in name]


@functools.lru_cache(maxsize=4)
def inputs(name: str, dt: str, mode: str, kind: str):
    """The dense operand (logical A [ba, m, k] for "col", B [bb, k, n] for "row"), the bias and act of one (case, dtype, mode),
    shared by the rounds and the layouts (and not to be modified)."""
    cs = CASES[name]
    grid, form, act = MODES[mode]
    rng = np.random.default_rng(seed_of(name, dt, 1 if kind == "col" else 2))
    nb = 1 if (cs.shared_a if kind == "col" else cs.shared_b) else cs.b
    shape = (nb, cs.m, cs.k) if kind == "col" else (nb, cs.k, cs.n)
    dense = grid_values(rng, shape) if grid else storage_normal(rng, shape, dt)
    if form is None:
        bias = None
    elif cs.grouped:  # one row bias per member
        bias = grid_bias((cs.b, cs.n))[:, None, :]
    else:
        bias = np.zeros(cs.n, dtype=np.float32) if form == "zero" else grid_bias(bias_shape(form, cs.b, cs.m, cs.n))
    for a in (dense, bias):
        if a is not None:
            assert a.dtype == np.float32 and np.array_equal(R.round_to(a, dt), a)
            a.setflags(write=False)
    return SimpleNamespace(dense=dense, bias=bias, act=act, grid=grid, kind=kind)


def epilogue(y, bias, act, out=None):
    """out: y itself where the caller owns it (the 17 M-element expectations are built in place)."""
    if bias is not None:
        y = np.add(y, bias, out=out)
    return np.maximum(y, 0, out=out) if act else y


def head_split(y, head):
    """[b, m, n] as [b, m / S, n / D, S, D]: MatMul -> Reshape -> Transpose(0, 2, 1, 3)."""
    if head is None:
        return y
    s, d = head
    b, m, n = y.shape
    return np.ascontiguousarray(y.reshape(b, m // s, s, n // d, d).transpose(0, 1, 3, 2, 4))


def selected(cs, dense, sel):
    """The product of a selector round as a gather: no GEMM. [b, m, n], in the dtype of `dense` (float32 holds every value)."""
    out = np.empty((cs.b, cs.m, cs.n), dtype=dense.dtype)
    for bi in range(cs.b):
        d = dense[bi if dense.shape[0] > 1 else 0]
        k, v = (a[bi if sel.k.shape[0] > 1 else 0] for a in (sel.k, sel.v))
        np.take(d, k, axis=1 if sel.kind == "col" else 0, out=out[bi])
        out[bi] *= v[None, :].astype(dense.dtype) if sel.kind == "col" else v[:, None].astype(dense.dtype)
    return out


def expected(cs, inp, sel):
    """What a launch of the round must return, in the layout of the output tensor."""
    y = selected(cs, inp.dense, sel)
    return head_split(epilogue(y, inp.bias, inp.act, out=y), cs.head)


def operands(cs, inp, sel):
    """Logical A [ba, m, k] and B [bb, k, n] of a round."""
    hot = onehot(cs, sel)
    return (inp.dense, hot) if sel.kind == "col" else (hot, inp.dense)


def stored(x, transposed):
    """A logical [nb, rows, cols] operand as it lies in memory."""
    return np.ascontiguousarray(x.swapaxes(1, 2)) if transposed else x


def describe(cs, inp, sel):
    """idx of the output -> what that element should have selected, for the failure message."""
    def say(idx):
        if cs.head is not None:
            s, d = cs.head
            bi, i, j = idx[0], idx[1] * s + idx[3], idx[2] * d + idx[4]
        else:
            bi, i, j = idx
        p = j if sel.kind == "col" else i
        sb = bi if sel.k.shape[0] > 1 else 0
        k, v = int(sel.k[sb, p]), float(sel.v[sb, p])
        db = bi if inp.dense.shape[0] > 1 else 0
        src = f"a[{db}, {i}, {k}] = {inp.dense[db, i, k]!r}" if sel.kind == "col" else f"b[{db}, {k}, {j}] = {inp.dense[db, k, j]!r}"
        bias = "" if inp.bias is None else f" + bias {np.broadcast_to(inp.bias, (cs.b, cs.m, cs.n))[bi, i, j]!r}"
        tiles = f"row tile {i // 256} (row {i % 256}), column {j} (64-column block {j // 64}), K-tile {k // 64} (k % 64 = {k % 64})"
        return (f"C[{bi}, {i}, {j}] selects k = {k} of K = {cs.k} with {'b' if sel.kind == 'col' else 'a'} = {v}: {src}{bias}"
                f"{', relu' if inp.act else ''}; {tiles}")
    return say


def assert_exact(got, want, what: str = "", describe=None):
    """got == want element by element (-0 equals +0, NaN equals nothing); names the first wrong element."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = ~(got == want)
    if bad.any():
        idx = tuple(int(i) for i in np.unravel_index(int(np.argmax(bad)), bad.shape))
        more = f"; {describe(idx)}" if describe is not None else ""
        raise AssertionError(f"{what}: {int(bad.sum())} wrong elements, the first at {idx}: got {got[idx]!r}, want {want[idx]!r}{more}")


# ------------------------------------------------------------------------------------------------------------------------
# random inputs of three tests of tests/test_gpu_matmul.py, for the per-element bound
# ------------------------------------------------------------------------------------------------------------------------
MAX_RANDOM_MACS = 2.5e8  # above: whole sampled rows instead of the dense fp64 product
SAMPLED_ROWS = 64

WALK_SHAPES = [(1, 16384, 1536, 192), (1, 8192, 4096, 64), (1, 4104, 3080, 128), (3, 2048, 2560, 256), (1, 16384, 768, 768)]
WALK_LAYOUTS = ("nn", "nt", "tn")
SPLITK_SHAPES = [(2048, 4096, 4096), (2048, 512, 4096), (2048, 1024, 11008)]
HEADLINE = 4096

# family -> (the test whose generator and seed it repeats, the variants it forces, row bias)
RANDOM_FAMILIES = {
    "walk": ("test_persistent_gemm_walks_several_tiles", (4, 5, 6), True),
    "splitk": ("test_matmul_splitk_heuristic_shapes", (-1,), False),
    "headline": ("test_matmul_headline_shape_sampled_rows", (1, 2, 3, 4, 5, 6, 8), False),
}


def random_params():
    """[(family, cfg)]: cfg = (shape, layout) / (index into SPLITK_SHAPES,) / (layout,). The headline product is referenced once, NN:
    its NT launch multiplies by the transposed copy of the same B, so the reference is the same."""
    return ([("walk", (s, lay)) for s in WALK_SHAPES for lay in WALK_LAYOUTS] + [("splitk", (i,)) for i in range(len(SPLITK_SHAPES))]
            + [("headline", ("nn",))])


def random_dts(family, cfg):
    """bf16, the type of the three tests; f16 as well on one ragged walk shape (the bound's other u)."""
    return ("f16", "bf16") if family == "walk" and cfg == (WALK_SHAPES[2], "nn") else ("bf16",)


def random_name(family, cfg):
    return f"{family}-" + "-".join("x".join(map(str, c)) if isinstance(c, tuple) else str(c) for c in cfg)


def _edge_rows(m):
    return [r for r in (0, 255, 256, m - 257, m - 256, m - 1) if 0 <= r < m]


@functools.lru_cache(maxsize=1)
def _splitk_draws():
    """The draws of test_matmul_splitk_heuristic_shapes in its order: one generator for the three shapes, rows included."""
    rng = np.random.default_rng(17)
    out = []
    for m, n, k in SPLITK_SHAPES:
        a = rng.standard_normal((m, k)).astype(np.float32)
        w = rng.standard_normal((k, n)).astype(np.float32)
        out.append((a, w, rng.choice(m, 16, replace=False)))
    return out


@functools.lru_cache(maxsize=1)
def random_inputs(family: str, cfg: tuple):
    """a, b as STORED (float32, unrounded), bias, the layout and the rows the named test samples — same seed, order and scaling."""
    if family == "walk":
        shape, lay = cfg
        ta, tb = LAYOUTS[lay]
        b, m, n, k = shape
        rng = np.random.default_rng(hash((shape, ta, tb)) % 2 ** 32)
        a = rng.standard_normal((b, k, m) if ta else (b, m, k)).astype(np.float32)
        bm = rng.standard_normal((n, k) if tb else (k, n)).astype(np.float32)
        bias = rng.standard_normal((n,)).astype(np.float32)
        rows = np.unique(np.concatenate([rng.choice(m, 24, replace=False), [0, 255, 256, m - 1]]))
    elif family == "splitk":
        a, bm, rows = _splitk_draws()[cfg[0]]
        lay, bias = "nn", None
        a = a[None]
    else:
        lay = cfg[0]
        rng = np.random.default_rng(0)
        a = rng.standard_normal((HEADLINE, HEADLINE)).astype(np.float32)[None]
        bm = rng.standard_normal((HEADLINE, HEADLINE)).astype(np.float32)
        rows, bias = rng.choice(HEADLINE, 48, replace=False), None
        if lay == "nt":  # (the test multiplies by b.t().contiguous() with trans_b: the same product)
            bm = np.ascontiguousarray(bm.T)
    ta, tb = LAYOUTS[lay]
    b, (m, k) = a.shape[0], (a.shape[2], a.shape[1]) if ta else a.shape[1:]
    n = bm.shape[0] if tb else bm.shape[1]
    return SimpleNamespace(a=a, b=bm, bias=bias, layout=lay, shape=(b, m, n, k), test_rows=np.asarray(rows))


def release():
    """Drop every cached input and reference (about 1 GB of host memory after the random cases): the test files call it when their
    module is done, so that nothing of theirs stays behind for the rest of the session."""
    for cached in (inputs, random_inputs, random_reference, _splitk_draws):
        cached.cache_clear()


def bound_for(dt, want, absum):
    return U[dt] * np.abs(want) + 2.0 ** -17 * absum


@functools.lru_cache(maxsize=2)
def random_reference(family: str, cfg: tuple, dt: str):
    """Rounded operands as stored (float32), want (fp64 of the rounded operands) and the per-element bound. Products above
    MAX_RANDOM_MACS: on the rows `rows` only (the rows the test itself samples, the edges of the row tiles and random ones up to
    SAMPLED_ROWS), want / absum / bound then [b, len(rows), n]; else rows is None."""
    inp = random_inputs(family, cfg)
    ta, tb = LAYOUTS[inp.layout]
    b, m, n, k = inp.shape
    rd = lambda x: None if x is None else R.round_to(x, dt).astype(np.float32)  # noqa: E731
    a, bm, bias = rd(inp.a), rd(inp.b), rd(inp.bias)
    rows = None
    al = a.swapaxes(1, 2) if ta else a  # logical [b, m, k]
    if b * m * n * k > MAX_RANDOM_MACS:
        extra = np.random.default_rng(12345).choice(m, SAMPLED_ROWS, replace=False)
        rows = np.unique(np.concatenate([inp.test_rows, _edge_rows(m), extra]))
        al = al[:, rows, :]
    al = np.asarray(al, dtype=np.float64)
    bl = np.asarray(bm.T if tb else bm, dtype=np.float64)
    want = R.matmul(al, bl, bias)
    absum = R.matmul(np.abs(al), np.abs(bl), None if bias is None else np.abs(bias))
    return SimpleNamespace(a=a, b=bm, bias=bias, layout=inp.layout, shape=inp.shape, rows=rows, test_rows=inp.test_rows, want=want,
                           absum=absum, bound=bound_for(dt, want, absum), al=al, bl=bl)


# ------------------------------------------------------------------------------------------------------------------------
# mutations: the same GEMM with one defect
# ------------------------------------------------------------------------------------------------------------------------
INDEX_MUTATIONS = ("drop_last_k_last_column_tile", "k_tail_not_zero_filled", "double_k64", "skip_last_ktile_of_uneven_slice",
                   "swap_a_chunks", "batch_reads_a0", "bias_strides_swapped", "head_split_s_d_swapped", "column_past_n_over_last")
NUMERICS_MUTATION = "round_partials_64"
COLUMN_TILE = 64  # the narrowest column block any tile kernel stores (NT units of 64 columns)


def mutation_applies(cs, mut: str, dt: str, form=None) -> bool:
    chunk = 4 if storage_of(cs, dt) == "f32" else 8
    return {
        "drop_last_k_last_column_tile": True,
        "k_tail_not_zero_filled": cs.k % cs.kt != 0,
        "double_k64": cs.k > 64,
        "skip_last_ktile_of_uneven_slice": bool(cs.splits and cs.splits > 1 and (cs.k // 64) % -(-(cs.k // 64) // cs.splits) != 0),
        "swap_a_chunks": cs.m > 10 and cs.k >= 2 * chunk,
        "batch_reads_a0": cs.b > 1 and not cs.shared_a,
        "bias_strides_swapped": form in ("n", "mn", "bmn", "m1") and not cs.grouped,
        "head_split_s_d_swapped": cs.head is not None and cs.head[0] != cs.head[1],
        "column_past_n_over_last": cs.n % COLUMN_TILE != 0,
        NUMERICS_MUTATION: cs.k > 64,
    }[mut]


def _memory(x, kmajor, rows_ext, k_ext):
    """A logical operand [nb, rows, k] read as [nb, rows_ext, k_ext] with the SAME strides: an index past a row or past the matrix reads
    what follows it in memory — the next row, the next batch, and behind the tensor the slack (SLACK_FILL, however far)."""
    nb, rows, k = x.shape
    flat = np.concatenate([(x if kmajor else x.swapaxes(1, 2)).ravel().astype(np.float64), [SLACK_FILL]])
    bi, i, kk = np.ogrid[:nb, :rows_ext, :k_ext]
    off = bi * rows * k + (i * k + kk if kmajor else kk * rows + i)
    return flat[np.minimum(off, flat.size - 1)]


def forward(cs, layout, a, b, bias=None, act=0, mut=None, dt="bf16"):
    """fp64 GEMM + epilogue (+ head-split store) of logical a [ba, m, k], b [bb, k, n]; `mut` names the defect (None: the correct
    result). `layout` says how the operands lie in memory, which is what the out-of-bounds defects read."""
    ta, tb = LAYOUTS[layout]
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    m, n, k = cs.m, cs.n, cs.k
    if mut == "batch_reads_a0":
        a = a[:1]
    elif mut == "swap_a_chunks":  # 16-byte chunks c and c ^ 1 change places for rows with (r >> 1) & 7 == 5
        chunk = 4 if storage_of(cs, dt) == "f32" else 8
        kk = np.arange(k)
        src = np.where(((kk // chunk) ^ 1) * chunk + chunk <= k, ((kk // chunk) ^ 1) * chunk + kk % chunk, kk)
        hit = (np.arange(m) >> 1) & 7 == 5
        a = np.where(hit[None, :, None], a[:, :, src], a)
    elif mut == "double_k64":
        a = a.copy()
        a[:, :, 64] *= 2
    elif mut == "skip_last_ktile_of_uneven_slice":
        a = a.copy()
        a[:, :, k - 64:] = 0
    elif mut == "k_tail_not_zero_filled":  # the last K-tile is read whole
        kp = -(-k // cs.kt) * cs.kt
        a = _memory(a, not ta, m, kp)
        b = _memory(b.swapaxes(1, 2), tb, n, kp).swapaxes(1, 2)
    y = np.matmul(a, b)
    y = np.broadcast_to(y, (cs.b, m, n)).copy()
    if mut == "drop_last_k_last_column_tile":
        c0 = (n - 1) // COLUMN_TILE * COLUMN_TILE
        y[:, :, c0:] -= a[:, :, k - 1:k] * b[:, k - 1:k, c0:]
    elif mut == "column_past_n_over_last":
        bx = _memory(b.swapaxes(1, 2), tb, n + 1, k).swapaxes(1, 2)
        y[:, :, n - 1] = np.matmul(a, bx[:, :, n:])[..., 0]
    if bias is not None and mut == "bias_strides_swapped":
        form = next(f for f in ("n", "mn", "bmn", "m1") if bias.shape == bias_shape(f, cs.b, m, n))
        sb, sm, sn = bias_strides(form, m, n)
        flat = np.concatenate([np.asarray(bias, dtype=np.float64).ravel(), [SLACK_FILL]])
        bi, i, j = np.ogrid[:cs.b, :m, :n]
        y = y + flat[np.minimum(bi * sb + i * sn + j * sm, flat.size - 1)]
        bias = None
    y = epilogue(y, None if bias is None else np.asarray(bias, dtype=np.float64), act)
    if cs.head is None:
        return y
    if mut != "head_split_s_d_swapped":
        return head_split(y, cs.head)
    s, d = cs.head  # the row stride inside a head is S instead of D; what lands behind the tensor is lost in the guard
    out = np.full(cs.b * m * n + s * s, OUT_FILL)
    bi, i, j = np.ogrid[:cs.b, :m, :n]
    out[bi * m * n + ((i // s) * (n // d) + j // d) * s * d + (i % s) * s + j % d] = y
    return out[: cs.b * m * n].reshape(cs.b, m // s, n // d, s, d)


def forward_rounded_partials(a, b, dt, bias=None, every=64):
    """The numerics mutation: the running sum is rounded to the storage type every `every` terms."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    acc = np.zeros(np.broadcast_shapes(a.shape[:-2], b.shape[:-2]) + (a.shape[-2], b.shape[-1]))
    for k0 in range(0, a.shape[-1], every):
        acc = R.round_to(acc + np.matmul(a[..., k0:k0 + every], b[..., k0:k0 + every, :]), dt)
    return acc if bias is None else acc + bias
