"""The selector inputs, the checker and the mutations of tests/matmul_cases.py, proved on the oracle alone (no GPU): the proof that the
expectations of tests/test_gpu_matmul_selectors.py do not come from a kernel.

1. Expected values: the gathered expectation of every round equals oracle/ref_ops.py::matmul (+ the epilogue in fp64, + the head-split
   reshape / transpose) on the same operands EXACTLY and is unchanged by a rounding to its storage type. R.matmul is run on the cases
   of at most DENSE_MACS multiply-adds; the rounds of the larger ones (the *-walk-* cases of the persistent kernels and
   wave128-272tiles, named by test_the_cases_left_to_the_rounding_check) are checked for the rounding only (R.round_to on every
   eighth row, the bit pattern of the storage type on every element) — the same gather, the same K targets as their small siblings.
2. Coverage: every required K target of every case is selected in some round, by a column and by a row; the diagonal cases cover every
   (k mod KT, position mod KT) pair; the round caps hold.
3. Every index mutation that applies to a case changes an element of one of its selector rounds (the out-of-bounds ones with the
   1000-filled slack modelled).
4. What the current forms miss. On the real inputs of the three existing tests, ONE product a[i, K - 1] b[K - 1, j] dropped from an
   output and the result rounded to bf16: share of the referenced outputs (whole sampled rows) that still PASS the test's own assertion
   / the per-element bound of test_matmul_16bit_variants:
       test_persistent_gemm_walks_several_tiles  (1, 16384, 768, 768) nn   u |c| + u sqrt(k)   52.5 %   /   28.1 %
       test_matmul_splitk_heuristic_shapes       (2048, 512, 4096)         u |c| + u sqrt(k)   82.5 %   /   55.9 %
       test_matmul_headline_shape_sampled_rows   4096^3 nn                 2^-7 |c| + 0.5      76.5 %   /   47.9 %
   (bf16, on the rows the test itself samples). The same defect at one output corner alone passes each of the three assertions, while
   a selector round fails on every element of the last column tile of every row that selects K - 1. No bound on a random sum can
   close that gap: a product of two N(0, 1) values is smaller than half a bf16 ulp of a sum of sqrt(K) of them about half the time.
5. The per-element bound: the fp64 reference rounded once to storage stays within it on every random case the GPU file runs (worst
   err / bound 0.497 in bf16, 0.489 in f16: half a storage ulp against a whole one); the numerics mutation (the running sum rounded
   to storage every 64 terms) exceeds it on every case with K >= 576, 6.7 - 10-fold in f16 and 32 - 67-fold in bf16.
6. Every case's declared variant, and split factor where declared, is what ops.matmul_plan_route answers for 256 CUs in every layout
   and mode the case runs, with the alignment bits the GPU file produces.
Each test prints what it measured (pytest -s)."""
import numpy as np
import pytest
import torch

import matmul_cases as C
from infinitensor_amd import ops
from oracle import ref_ops as R

TD = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
DENSE_MACS = 3e8
K_NUMERICS = 576
KINDS = ("col", "row")


@pytest.fixture(scope="module", autouse=True)
def leave_nothing_behind():
    yield
    C.release()


def _representable(x, dt):
    """Every float32 of x is a value of dt, by its bits: the low 16 bits of a bf16 are zero, an f16 survives the conversion."""
    assert x.dtype == np.float32
    if dt == "bf16":
        return not (np.ascontiguousarray(x).view(np.uint32) & 0xFFFF).any()
    return dt == "f32" or np.array_equal(x.astype(np.float16).astype(np.float32), x)


def _rounds_to_check(cs, kind):
    """Every round; of a diagonal case every eighth (they differ by a rotation only) — coverage is asserted on all of them below."""
    rs = C.rounds(cs, kind)
    return rs[::8] if cs.diag else rs


@pytest.mark.parametrize("name", list(C.CASES))
def test_expected_values_are_the_oracles_exactly(name):
    cs = C.CASES[name]
    dense = cs.macs <= DENSE_MACS
    checked = 0
    for dt in cs.dts:
        st = C.storage_of(cs, dt)
        for mode in cs.modes:
            for kind in KINDS:
                inp = C.inputs(name, dt, mode, kind)
                for sel in _rounds_to_check(cs, kind):
                    want = C.expected(cs, inp, sel)
                    assert want.dtype == np.float32
                    assert want.shape == ((cs.b, cs.m, cs.n) if cs.head is None else (cs.b, cs.m // cs.head[0], cs.n // cs.head[1]) + cs.head)
                    assert _representable(want, dt)
                    # (R.round_to itself: on everything, or on every eighth row of the 17 M elements of a multi-tile case)
                    some = want if dense else want[:, ::8]
                    assert np.array_equal(R.round_to(some, dt), some) and (st == dt or np.array_equal(R.round_to(some, st), some))
                    if inp.grid:
                        assert np.abs(want).max() <= 12 and np.array_equal(want * 8, np.round(want * 8))
                    if dense:
                        a, b = C.operands(cs, inp, sel)
                        assert np.array_equal(R.round_to(a, dt), a) and np.array_equal(R.round_to(b, dt), b)
                        ref = C.head_split(np.broadcast_to(C.epilogue(R.matmul(a, b), inp.bias, inp.act), (cs.b, cs.m, cs.n)), cs.head)
                        assert np.array_equal(want, ref)
                        # (the same through the layouts as they are stored)
                        ta, tb = C.LAYOUTS[cs.layouts[-1]]
                        assert np.array_equal(R.matmul(C.stored(a, ta), C.stored(b, tb), None, ta, tb), R.matmul(a, b))
                    checked += 1
    print(f"\n{name}: {cs.macs:.3g} multiply-adds, {checked} rounds {'checked against R.matmul' if dense else 'rounding only'}")


def test_the_cases_left_to_the_rounding_check():
    skipped = [n for n, cs in C.CASES.items() if cs.macs > DENSE_MACS]
    print("\nnot run through R.matmul:", ", ".join(skipped))
    assert all("-walk-" in n or n == "wave128-272tiles" for n in skipped)
    kept = {cs.report for cs in C.CASES.values() if cs.macs <= DENSE_MACS}
    assert kept == set(C.VARIANTS)  # every kernel still has cases that are


@pytest.mark.parametrize("name", list(C.CASES))
def test_coverage(name):
    cs = C.CASES[name]
    req = set(C.required_k(cs))
    assert {0, cs.k - 1} <= req
    for step in (64, 128):
        assert {x for t in range(step, cs.k, step) for x in (t - 1, t)} <= req
    if cs.k % cs.kt:
        assert {cs.k - cs.k % cs.kt, cs.k - 1} <= req
    if cs.splits and cs.splits > 1:  # the slices as launch256_splitk cuts them
        nk = cs.k // 64
        per = (nk + cs.splits - 1) // cs.splits
        left = (nk + per - 1) // per
        starts = [s * per * 64 for s in range(1, left)]
        assert C.slice_boundaries(cs.k, cs.splits) == starts
        assert {x for s in starts for x in (s - 1, s)} <= req
    if cs.report == "wave128":
        assert {x for t in range(32, cs.k, 32) for x in (t - 1, t)} <= req
    line = []
    for kind in KINDS:
        cnt = cs.n if kind == "col" else cs.m
        rs = C.rounds(cs, kind)
        got = {int(k) for sel in rs for k in sel.k[0]}
        for sel in rs:
            assert sel.k.shape == sel.v.shape and sel.k.min() >= 0 and sel.k.max() < cs.k
            assert set(np.unique(sel.v)) <= set(C.VALUES)
            hot = C.onehot(cs, sel)
            assert (np.count_nonzero(hot, axis=1 if kind == "col" else 2) == 1).all()  # one target per column (row)
        if cs.diag:
            assert len(rs) == cs.kt
            pairs = {(int(k) % cs.kt, j % cs.kt) for sel in rs for j, k in enumerate(sel.k[0])}
            assert len(pairs) == cs.kt * cs.kt, "every k of a K-tile meets every position mod KT"
            assert got == set(range(cs.k))
        else:
            T = C.k_targets(cs, cnt)
            assert req <= set(T) <= set(C.boundary_k(cs))
            assert req <= got and got == set(T)
            full = C.boundary_k(cs)
            if -(-len(full) // cnt) <= C.MAX_ROUNDS:
                assert T == full  # nothing to thin
            assert len(rs) <= C.MAX_ROUNDS or (set(T) == req and len(rs) <= C.MAX_REQUIRED_ROUNDS)
        if cnt >= 4:
            assert {float(v) for sel in rs for v in sel.v[0]} == set(C.VALUES)
        line.append(f"{kind}: {len(rs)} rounds, {len(got)} targets")
    print(f"\n{name}: K = {cs.k}, {len(req)} required; " + "; ".join(line))


@pytest.mark.parametrize("name", [n for n, cs in C.CASES.items() if cs.macs <= DENSE_MACS and not cs.diag])
def test_index_mutations_change_a_selector_round(name):
    cs = C.CASES[name]
    dt = cs.dts[0]
    seen = []
    for mut in C.INDEX_MUTATIONS:
        modes = [m for m in cs.modes if C.MODES[m][1] in ("n", "mn", "bmn", "m1")] if mut == "bias_strides_swapped" else [cs.modes[0]]
        for mode in modes:
            if not C.mutation_applies(cs, mut, dt, C.MODES[mode][1]):
                continue
            for lay in cs.layouts:
                hit = None
                for kind in KINDS:
                    inp = C.inputs(name, dt, mode, kind)
                    for r, sel in enumerate(C.rounds(cs, kind)):
                        a, b = C.operands(cs, inp, sel)
                        if not np.array_equal(C.forward(cs, lay, a, b, inp.bias, inp.act, mut, dt), C.expected(cs, inp, sel)):
                            hit = f"{kind} round {r} {lay}"
                            break
                    if hit:
                        break
                assert hit is not None and hit.endswith(lay), (name, mut, mode, lay)  # in EVERY layout the case runs
            seen.append(f"{mut}{'/' + mode if len(modes) > 1 else ''} ({hit})")
    print(f"\n{name}: " + ", ".join(seen))
    assert len(seen) >= 2


def test_mutations_are_defects_and_the_unmutated_forward_is_the_oracle():
    """On dense random inputs: forward(None) is R.matmul, every mutation that applies differs from it; over the table every mutation
    applies somewhere."""
    rng = np.random.default_rng(0)
    applied = set()
    for name in ("generic-3x130x72x64", "fast128-ktail32", "splitk-2+1", "tile256-batch3", "headsplit-b-v1", "generic-77x53x41"):
        cs = C.CASES[name]
        a, b = rng.standard_normal((cs.b, cs.m, cs.k)), rng.standard_normal((cs.b, cs.k, cs.n))
        bias = C.grid_bias((cs.m, cs.n)).astype(np.float64)
        want = C.head_split(R.matmul(a, b, bias), cs.head)
        for lay in cs.layouts:
            assert np.allclose(C.forward(cs, lay, a, b, bias), want, rtol=0, atol=1e-11)
            for mut in C.INDEX_MUTATIONS:
                if C.mutation_applies(cs, mut, cs.dts[0], "mn"):
                    assert np.abs(C.forward(cs, lay, a, b, bias, 0, mut, cs.dts[0]) - want).max() > 1e-3, (name, lay, mut)
                    applied.add(mut)
        assert np.allclose(C.forward_rounded_partials(a, b, "f32", bias, every=10 ** 6), R.matmul(a, b, bias), rtol=1e-6, atol=1e-5)
    assert applied == set(C.INDEX_MUTATIONS)
    for mut in C.INDEX_MUTATIONS:
        assert any(C.mutation_applies(cs, mut, cs.dts[0], C.MODES[m][1]) for cs in C.CASES.values() for m in cs.modes), mut


def _existing_bound(family, want, k):
    return 2.0 ** -7 * np.abs(want) + (0.5 if family == "headline" else 2.0 ** -7 * np.sqrt(k))


@pytest.mark.parametrize("family,cfg,selector", [("walk", ((1, 16384, 768, 768), "nn"), "persist256-ragged"), ("splitk", (1,), "splitk-k1024"),
                                                 ("headline", ("nn",), "wave128-k256")])
def test_what_the_current_forms_miss(family, cfg, selector):
    ref = C.random_reference(family, cfg, "bf16")
    b, m, n, k = ref.shape
    assert ref.rows is not None
    # the rows the test itself looks at: inside what is referenced here
    mine = np.searchsorted(ref.rows, ref.test_rows)
    assert np.array_equal(ref.rows[mine], ref.test_rows)
    dropped = R.round_to(ref.want - ref.al[:, :, k - 1:k] * ref.bl[k - 1:k, :], "bf16")
    err = np.abs(dropped - ref.want)
    old_pass = err[:, mine] <= _existing_bound(family, ref.want[:, mine], k)
    new_pass = (err <= ref.bound)[:, mine]
    print(f"\n{C.random_name(family, cfg)} bf16: one product dropped per output: {100 * old_pass.mean():.1f} % pass the existing assertion "
          f"({old_pass.size} outputs), {100 * new_pass.mean():.1f} % the per-element bound ({new_pass.size} outputs)")
    assert old_pass.mean() > max(0.25, new_pass.mean()), "the existing form passes more of the outputs with a product missing"
    # ... at one output corner alone (the last column of the last row the test samples): the test's assertion passes
    row = int(mine[np.argmax(ref.test_rows)])
    corner = R.round_to(ref.want, "bf16")
    cols = [j for j in range(n - 1, n - 65, -1) if old_pass[0, list(mine).index(row), j]]
    assert cols, "no passing corner in the last column tile"
    corner[0, row, cols[0]] = dropped[0, row, cols[0]]
    assert (np.abs(corner - ref.want)[:, mine] <= _existing_bound(family, ref.want[:, mine], k)).all()
    # ... and the same defect fails a selector round of the same kernel family, on the row that selects K - 1
    cs = C.CASES[selector]
    inp = C.inputs(selector, "bf16", "plain", "row")
    hits = 0
    for sel in C.rounds(cs, "row"):
        a, bb = C.operands(cs, inp, sel)
        bad = C.forward(cs, "nn", a, bb, None, 0, "drop_last_k_last_column_tile") != C.expected(cs, inp, sel)
        hits += int(bad.sum())
        assert bad.sum() == ((sel.k == cs.k - 1).sum() * (cs.n - (cs.n - 1) // C.COLUMN_TILE * C.COLUMN_TILE))
    print(f"  {selector}: {hits} wrong elements over its row-selector rounds")
    assert hits > 0


_RANDOM = C.random_params()


@pytest.mark.parametrize("family,cfg", _RANDOM, ids=[C.random_name(f, c) for f, c in _RANDOM])
def test_per_element_bound_admits_the_rounded_reference_and_not_16_bit_partial_sums(family, cfg):
    for dt in ("f16", "bf16"):
        ref = C.random_reference(family, cfg, dt)
        k = ref.shape[3]
        worst = C.assert_within(R.round_to(ref.want, dt), ref.want, ref.bound, f"{C.random_name(family, cfg)} {dt} rounded reference")
        line = f"\n{C.random_name(family, cfg)} {dt}: K = {k}{'' if ref.rows is None else f' ({len(ref.rows)} rows)'}, rounded reference worst err/bound {worst:.3f}"
        assert worst <= 0.5 + 1e-9  # half a storage ulp against a whole one
        if k >= K_NUMERICS:
            sub = slice(0, 8)  # eight referenced rows are enough to exceed it
            y = R.round_to(C.forward_rounded_partials(ref.al[:, sub], ref.bl, dt, ref.bias), dt)
            factor, idx = C.worst_ratio(y, ref.want[:, sub], ref.bound[:, sub])
            line += f", partial sums in {dt}: {factor:.3g} at {idx}"
            assert factor > 1.0, (family, cfg, dt, factor)
        print(line, end="")


def test_the_random_cases_are_the_existing_tests_inputs():
    """The shape lists and seeds repeated in matmul_cases.py are those of tests/test_gpu_matmul.py (read from its source: importing it
    needs no GPU, but its parametrize marks are the record)."""
    import test_gpu_matmul as M

    marks = {m.args[0]: m.args[1] for m in M.test_persistent_gemm_walks_several_tiles.pytestmark if m.name == "parametrize"}
    assert list(marks["shape"]) == C.WALK_SHAPES
    assert [C.LAYOUTS[lay] for lay in C.WALK_LAYOUTS] == list(marks["ta,tb"])
    assert tuple(marks["variant"]) == C.RANDOM_FAMILIES["walk"][1]
    import inspect

    src = inspect.getsource(M.test_matmul_splitk_heuristic_shapes)
    assert "default_rng(17)" in src and str(tuple(C.SPLITK_SHAPES)).replace(",)", ")") in src.replace("\n", "")
    src = inspect.getsource(M.test_matmul_headline_shape_sampled_rows)
    assert "default_rng(0)" in src and "M = N = K = 4096" in src and "rng.choice(M, 48, replace=False)" in src
    assert {f for f, _ in _RANDOM} == set(C.RANDOM_FAMILIES) and max(k for _, _, k in C.SPLITK_SHAPES) >= 4096


@pytest.mark.parametrize("name", list(C.CASES))
def test_declared_variants_are_the_planners(name):
    cs = C.CASES[name]
    for dt in cs.dts:
        for lay in cs.layouts:
            for mode in cs.modes:
                got = ops.matmul_plan_route(TD[C.storage_of(cs, dt)], cs.b, cs.m, cs.n, cs.k, num_cu=256, **C.plan_args(cs, lay, mode))
                assert got[0] == cs.report, (name, dt, lay, mode, got)
                if cs.splits is not None:
                    assert got[1] == cs.splits, (name, dt, lay, mode, got)
                else:
                    assert got[1] == 1
    if cs.a_lo:  # the planner agrees that it is the alignment alone
        kw = dict(C.plan_args(cs, cs.layouts[0], cs.modes[0]), a_lo=0)
        assert ops.matmul_plan_route(TD[cs.dts[0]], cs.b, cs.m, cs.n, cs.k, num_cu=256, **kw)[0] == "fast128_glds"
    print(f"\n{name}: variant {cs.variant} -> {cs.report}{'' if cs.splits is None else f' x {cs.splits}'} in {', '.join(cs.layouts)}; {', '.join(cs.modes)}")


def test_the_table_reaches_every_variant_and_form():
    assert {cs.report for cs in C.CASES.values()} == set(ops.matmul_variants()) == set(C.VARIANTS)
    assert list(C.VARIANTS) == ops.matmul_variants()
    assert {cs.report for cs in C.CASES.values() if cs.diag} == set(C.VARIANTS)  # one diagonal case per kernel
    assert {cs.env.get("IROCM_GEMM_TAB_N") for cs in C.CASES.values() if cs.env} == {0, 1, 2}
    for forms_on in ("generic64", "tile256", "tile256_splitk", "fast32"):
        assert any(set(C.FORMS) <= set(cs.modes) for cs in C.CASES.values() if cs.report == forms_on), forms_on
    big = C.CASES["fast32-tile128"]
    small = C.CASES["fast32-k36"]
    form = lambda cs: "64^2" if -(-cs.m // 128) * -(-cs.n // 128) * cs.b * 2 < 256 else "128^2"  # noqa: E731  gemm_plan's rule
    print(f"\nfast32 at 256 CUs: {big.name} {form(big)}, {small.name} {form(small)}")
    assert form(big) == "128^2" and all(form(cs) == "64^2" for cs in C.CASES.values() if cs.report == "fast32" and cs is not big and cs.head is None)
