"""MatMul on a real MI355X against the exact selector inputs and the per-element bound of tests/matmul_cases.py (proved on the oracle
alone in tests/test_matmul_selectors_cpu.py): the nine kernels of csrc/gemm_route.h in every layout and epilogue each of them takes,
split-K by force and by the heuristic, the persistent kernels over more tiles than CUs (tile table and in-place decode), the cast
path of an fp32 MatMul, the head-split store and the grouped launch.

Every launch: A, B and the bias sit in the middle of blocks filled with 1000 (512 elements on each side: a read outside an operand
shows as +-1000 v), the output — given through out= — inside a block pre-filled with 7 with 512-element guards (an unwritten element
is a wrong element), the gaps of the grouped slabs filled likewise. Asserted in this order: the launch reports the declared variant
(a silent fall-back is a failure); got == want element by element on the whole output; the guards and gaps keep their fill; the
operand blocks, slack included, are bit-identical to before the launch.

test_matmul_random_inputs_per_element repeats the random inputs of test_persistent_gemm_walks_several_tiles,
test_matmul_splitk_heuristic_shapes and test_matmul_headline_shape_sampled_rows (tests/test_gpu_matmul.py) in bf16, the type of those
tests (and one walk shape in f16), and checks whole sampled rows against bound = u |want| + 2^-17 S instead. Worst err / bound per
(variant, dtype), from the lines it prints (pytest -s), measured on an MI355X:

    variant         dtype worst  launches  where
    fast128_glds    bf16  0.488      2     (0, 651, 3013) of headline, NN and NT
    tile256         bf16  0.488      2     (0, 651, 3013) of headline, NN and NT
    tile256_splitk  bf16  0.488      4     (0, 651, 3013) of headline, NN and NT
    persist256      f16   0.484      1     (0, 2916, 358) of walk-1x4104x3080x128-nn
    persist256      bf16  0.497     17     (0, 2178, 160) of walk-1x8192x4096x64-nn
    persist192      f16   0.484      1     (0, 2916, 358) of walk-1x4104x3080x128-nn
    persist192      bf16  0.497     17     (0, 2178, 160) of walk-1x8192x4096x64-nn
    persist128      f16   0.484      1     (0, 2916, 358) of walk-1x4104x3080x128-nn
    persist128      bf16  0.497     18     (0, 2178, 160) of walk-1x8192x4096x64-nn
    wave128         bf16  0.488      2     (0, 651, 3013) of headline, NN and NT

Every figure is the final rounding's half ulp against the bound's whole one — the figures of the fp64 reference rounded once
(tests/test_matmul_selectors_cpu.py, item 5, which covers f16 on every case): no kernel accumulates below fp32 or rounds twice, and
the kernels of one shape agree to the element. No selector case failed on any kernel.

Cost: 171 tests, one per (case, dtype) with its layouts and modes inside; 9 seconds inside the whole GPU suite on the MI355X, the
slowest test 0.9. What keeps it there: the multi-tile cases (17 M outputs a launch) launch a spread of (dtype, layout, mode) instead
of the whole product, expectations are built in place and compared on the device, and the cached references are dropped when the
file is done (leave_nothing_behind).

That the file can fail was checked by hand against a library with two defects (a scratch build, not kept): stage_kmajor of
csrc/gemm32.hip zero-filling the K tail from kend + 4 instead of kend failed every NT case of fast32-k36 and fast32-batch3-k100 (NN
stayed exact: its B tail goes through stage_nmajor and is still zero), and slice 0 of a split-K tile skipping its last K-tile
(csrc/gemm256.hip) failed every case of splitk-2+1 and splitk-k1024, e.g. "splitk-2+1 f16 nn plain col round 0 run 0: 26400 wrong
elements, the first at (0, 0, 16): got 0.0, want -0.812; C[0, 0, 16] selects k = 64 of K = 192 ... K-tile 1 (k % 64 = 0)".
"""
import numpy as np
import pytest
import torch

import matmul_cases as C
from infinitensor_amd import ops
from test_gpu_nn import TD, dev_slack2

pytestmark = pytest.mark.gpu
GUARD = C.SLACK  # elements of fill in front of and behind the output


@pytest.fixture(scope="module", autouse=True)
def leave_nothing_behind():
    """After the last test of this file: the cached references go, and the device blocks torch still holds for them."""
    yield
    C.release()
    torch.cuda.empty_cache()


def slack(a, st, off_bytes=0):
    """`a` in the middle of a block of SLACK_FILL; off_bytes: that many bytes off a 16-byte boundary."""
    if a is None:
        return None
    t = dev_slack2(np.asarray(a, dtype=np.float32), TD[st], fill=C.SLACK_FILL, spare=C.SLACK + off_bytes // TD[st].itemsize)
    assert t.data_ptr() & 15 == off_bytes
    return t


def bits(t):
    return t.view(torch.int32 if t.element_size() == 4 else torch.int16)


class Kept:
    """The blocks of the operands (slack included) as they were before the launches."""

    def __init__(self, *tensors):
        self.blocks = [t._base if t._base is not None else t for t in tensors if t is not None]
        self.before = [b.clone() for b in self.blocks]

    def unchanged(self):
        return all(torch.equal(bits(b), bits(k)) for b, k in zip(self.blocks, self.before))


def out_block(shapes, st, gap=0):
    """One block of OUT_FILL holding len(shapes) outputs `gap` elements apart, guards in front and behind -> block, views, the
    (start, end) of everything that is NOT an output."""
    numels = [int(np.prod(s)) for s in shapes]
    block = torch.full((2 * GUARD + sum(numels) + gap * len(shapes),), C.OUT_FILL, device="cuda", dtype=TD[st])
    views, outside, at = [], [(0, GUARD)], GUARD
    for s, ne in zip(shapes, numels):
        views.append(block[at:at + ne].view(s))
        outside.append((at + ne, at + ne + gap))
        at += ne + gap
    outside.append((at, block.numel()))
    assert at + GUARD == block.numel()
    return block, views, outside


def guards_hold(block, outside):
    return bool(torch.all(torch.cat([block[lo:hi] for lo, hi in outside]) == C.OUT_FILL).item())


def check(out, want, st, what, say):
    """got == want on the device, in fp32 (which holds every value of the storage type; `want` is exact in it: the CPU file); the host
    only to name a wrong element."""
    assert want.dtype == np.float32
    if not bool((out.float() == torch.from_numpy(np.ascontiguousarray(want)).cuda()).all().item()):
        C.assert_exact(out.float().cpu().numpy(), want, what, say)


def set_env(monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))


def batch_view(t, shared):
    return t[0] if shared else t


def run_rounds(rt, cs, dt, lay, mode, kind, reported, first_only=False):
    """Every round of one (case, dtype, layout, mode, selector kind); the caller holds the variant, the compute type and the env."""
    st = C.storage_of(cs, dt)
    ta, tb = C.LAYOUTS[lay]
    inp = C.inputs(cs.name, dt, mode, kind)
    dense_is_a = kind == "col"
    dense_d = slack(C.stored(inp.dense, ta if dense_is_a else tb), st, cs.a_lo if dense_is_a else 0)
    bias_d = slack(inp.bias, st)
    kept_dense = Kept(dense_d, bias_d)
    shape = (cs.b, cs.m, cs.n) if cs.head is None else (cs.b, cs.m // cs.head[0], cs.n // cs.head[1]) + cs.head
    for r, sel in enumerate(C.rounds(cs, kind)):
        hot_d = slack(C.stored(C.onehot(cs, sel), tb if dense_is_a else ta), st, 0 if dense_is_a else cs.a_lo)
        kept_hot = Kept(hot_d)
        a_d, b_d = (dense_d, hot_d) if dense_is_a else (hot_d, dense_d)
        want = C.expected(cs, inp, sel)
        for run in range(cs.runs):
            block, (out,), outside = out_block([shape], st)
            ops.matmul(rt, a_d, batch_view(b_d, cs.shared_b), bias_d, ta, tb, act=inp.act, out=out, head_split=cs.head)
            got = ops.matmul_last_variant(rt)
            what = f"{cs.name} {dt} {lay} {mode} {kind} round {r} run {run} ({got})"
            assert got == cs.report, what
            reported.add(got)
            check(out, want, st, what, C.describe(cs, inp, sel))
            assert guards_hold(block, outside), f"{what}: wrote outside the output"
            assert kept_dense.unchanged() and kept_hot.unchanged(), f"{what}: an operand block was written"
        if first_only:
            break


def run_grouped(rt, cs, dt, mode, kind, reported):
    """infini_rocm_matmul_grouped: weights, biases and outputs carved out of slabs with gaps (slab and gaps filled like the slack)."""
    g, m, n, k = cs.b, cs.m, cs.n, cs.k
    inp = C.inputs(cs.name, dt, mode, kind)
    gw, gb, go = (C.GROUPED_GAPS[x] for x in ("w", "bias", "out"))

    def slab(x, gap):  # x [g, ...] -> the members as views of one block, `gap` elements of fill behind each
        per = int(np.prod(x.shape[1:]))
        rows = np.full((g, per + gap), C.SLACK_FILL, dtype=np.float32)
        rows[:, :per] = x.reshape(g, per)
        flat = slack(rows, dt)
        return [flat[j, :per].view(x.shape[1:]) for j in range(g)]

    biases = slab(np.ascontiguousarray(inp.bias[:, 0, :]), gb)
    for r, sel in enumerate(C.rounds(cs, kind)):
        a_l, b_l = C.operands(cs, inp, sel)
        a_d = slack(a_l[0], dt)
        ws = slab(b_l, gw)
        kept = Kept(a_d, ws[0], biases[0])
        block, outs, outside = out_block([(m, n)] * g, dt, gap=go)
        ops.matmul_grouped(rt, a_d, ws, outs, biases, act=inp.act)
        got = ops.matmul_last_variant(rt)
        what = f"{cs.name} {dt} {mode} {kind} round {r} ({got})"
        assert got == cs.report, what
        reported.add(got)
        want = C.expected(cs, inp, sel)
        check(torch.stack(outs), want, dt, what, C.describe(cs, inp, sel))
        assert guards_hold(block, outside), f"{what}: wrote into a gap or a guard"
        assert kept.unchanged(), f"{what}: an operand block was written"


def run_case(rt, monkeypatch, name, dt, reported, first_only=False):
    """Every (layout, mode) the case launches in one dtype, column and row selectors each."""
    cs = C.CASES[name]
    set_env(monkeypatch, cs.env)
    try:
        ops.set_matmul_variant(rt, cs.variant)
        if cs.ct is not None:
            ops.set_matmul_compute_type(rt, cs.ct)
        for lay, mode in C.groups_of(cs, dt)[:1 if first_only else None]:
            for kind in ("col", "row"):
                if cs.grouped:
                    run_grouped(rt, cs, dt, mode, kind, reported)
                else:
                    run_rounds(rt, cs, dt, lay, mode, kind, reported, first_only)
        rt.sync()
    finally:
        ops.set_matmul_variant(rt, -1)
        ops.set_matmul_compute_type(rt, "default")
        for key in cs.env:
            monkeypatch.delenv(key, raising=False)


@pytest.mark.parametrize("name,dt", C.case_params(False), ids=lambda v: str(v))
def test_selectors(rt, name, dt, monkeypatch):
    """Column and row selectors of every case of the table at the targets of required_k / k_targets, in every layout and mode the
    case launches (a failure names them)."""
    run_case(rt, monkeypatch, name, dt, set())


@pytest.mark.parametrize("name,dt", C.case_params(True), ids=lambda v: str(v))
def test_diagonal_selectors(rt, name, dt, monkeypatch):
    """One tile of every kernel, KT launches: every k of a K-tile against every column (row) position mod KT."""
    run_case(rt, monkeypatch, name, dt, set())


def test_every_variant_is_reported_by_a_selector_launch(rt, monkeypatch):
    """The first round of the first case of every kernel: together they report all of ops.matmul_variants(); and the fp32 tile kernel
    takes the form gemm_plan's rule gives for this device's CU count."""
    reported = set()
    first = {cs.report: name for name, cs in reversed(C.CASES.items())}
    assert len(first) == len(C.VARIANTS)
    for name in first.values():
        cs = C.CASES[name]
        run_case(rt, monkeypatch, name, cs.dts[-1], reported, first_only=True)
    assert reported == set(ops.matmul_variants())
    cus = rt.device_info()["compute_units"]
    for name in ("fast32-tile128", "fast32-k36"):
        cs = C.CASES[name]
        small = -(-cs.m // 128) * -(-cs.n // 128) * cs.b * 2 < cus
        print(f"\n{name} on {cus} CUs: the {'64^2' if small else '128^2'} form", end="")


_RANDOM = C.random_params()


@pytest.mark.parametrize("family,cfg,dt", [(f, c, dt) for f, c in _RANDOM for dt in C.random_dts(f, c)],
                         ids=[f"{C.random_name(f, c)}-{dt}" for f, c in _RANDOM for dt in C.random_dts(f, c)])
def test_matmul_random_inputs_per_element(rt, family, cfg, dt):
    """The generators and seeds of three tests of tests/test_gpu_matmul.py, every variant each of them forces, against the per-element
    bound on whole rows (the rows the test samples, the edges of the row tiles and random ones) instead of their sqrt(k) / 0.5 forms."""
    ref = C.random_reference(family, cfg, dt)
    b, m, n, k = ref.shape
    ta, tb = C.LAYOUTS[ref.layout]
    a_d, b_d, bias_d = slack(ref.a, dt), slack(ref.b, dt), slack(ref.bias, dt)
    launches = [(variant, b_d, tb, ref.layout) for variant in C.RANDOM_FAMILIES[family][1]]
    if family == "headline":  # as the test does: the same product again through the transposed copy of B
        bt_d = slack(np.ascontiguousarray(ref.b.T), dt)
        launches += [(variant, bt_d, True, "nt") for variant in C.RANDOM_FAMILIES[family][1]]
    kept = Kept(a_d, b_d, bias_d)
    rows = None if ref.rows is None else torch.from_numpy(ref.rows).cuda()
    try:
        for variant, b_d, tb, lay in launches:
            ops.set_matmul_variant(rt, variant)
            block, (out,), outside = out_block([(b, m, n)], dt)
            ops.matmul(rt, a_d, b_d, bias_d, ta, tb, out=out)
            name = ops.matmul_last_variant(rt) + ("" if lay == ref.layout else " " + lay)
            got = (out if rows is None else out[:, rows]).float().cpu().numpy().astype(np.float64)
            worst, idx = C.worst_ratio(got, ref.want, ref.bound)
            at = idx if ref.rows is None else (idx[0], int(ref.rows[idx[1]]), idx[2])
            print(f"\nworst matmul {name} {dt} {worst:.3f} at {at} ({C.random_name(family, cfg)})", end="")
            C.assert_within(got, ref.want, ref.bound, f"{C.random_name(family, cfg)} {dt} ({name})")
            assert guards_hold(block, outside) and kept.unchanged()
    finally:
        ops.set_matmul_variant(rt, -1)
