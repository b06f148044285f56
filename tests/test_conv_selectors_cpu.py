"""The selector inputs, the checker and the mutations of tests/conv_cases.py, proved on the oracle alone (no GPU).

1. Expected values: the gathered / scattered expectation of every round equals oracle/ref_ops.py::conv2d (+ the epilogue in fp64) on
   the same inputs EXACTLY and is unchanged by a rounding to the storage type. R.conv2d is run on the cases of at most
   DENSE_MACS multiply-adds (the rounds of the larger ones are checked for the rounding only); skipped for R.conv2d: the three tap_splitk-* cases
   (0.9 - 1.2 G multiply-adds each; the unsplit tap GEMM cases run the same kernel's addressing through R.conv2d).
2. Coverage: every tap x every required channel, a target on every filter in every round, every target pixel, the tensor's last
   element in every pixel round, the round caps.
3. Every index mutation that applies to a case changes an element of one of its selector rounds.
4. What the allclose form misses: on the random inputs of test_conv_vs_oracle at bf16, (1, 512, 7, 7, 130, 3 x 3), seed as there, the
   "one corner" mutation (one product dropped at one output corner of every filter) PASSES np.allclose(rtol = atol = 1.6e-2) —
   largest error 0.0069 — while the per-element bound rejects it 14.7-fold. The "last slot of a run" mutation as built here (the
   whole output element of every eighth slot comes from its neighbour) is an O(1) error and is caught by either form, on this
   and on every other shape of that test; the allclose form lets through "drop_corner" alone.
5. The per-element bound: the fp64 reference rounded once to storage stays within it on every random case the GPU file runs, worst
   err / bound 0.497 (half a storage ulp against a whole one); the numerics mutation (the running sum rounded to storage every 64 terms) exceeds it on every case
   whose sums have K >= 576 terms inside the image, by a factor of 10.4 - 22.9 in f16 and 53.9 - 137 in bf16 (19 layers). K counts the
   terms that are not padding: test_conv_s1's 3 x 3 window on a 1 x 1 plane has K = 576 and 64 real terms per output, and is not
   asked to fail. The split-K layers are referenced on sampled outputs and take no part in the mutation.
   The one route-specific term: the pixel-slot GEMM rounds conv + bias before it adds the residual (a stated decision of
   csrc/gemm256p_kernel.h); replayed in numpy that arithmetic misses the shared bound 13.9-fold (f16) / 57.8-fold (bf16) — the very figures the
   kernel gave on an MI355X — and stays within bound + u |conv + bias| (worst 0.48).
6. Every case's declared (route, form) is what ops.conv_plan_route answers for 256 CUs, in every epilogue mode the case runs.
Each test prints what it measured (pytest -s)."""
import numpy as np
import pytest
import torch

import conv_cases as C
from infinitensor_amd import ops
from oracle import ref_ops as R

TD = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
DENSE_MACS = 3e8
K_NUMERICS = 576


def _modes_to_check(g):
    return ("plain", "zero_bias_relu", "bias_res_relu" if "bias_res_relu" in g.modes else "bias_relu")


@pytest.mark.parametrize("name", list(C.CASES))
def test_expected_values_are_the_oracles_exactly(name):
    g = C.CASES[name]
    dense = g.macs <= DENSE_MACS
    for dt in g.dts:
        for mode in _modes_to_check(g):
            inp = C.tap_inputs(name, dt, mode)
            for sel in C.tap_rounds(g):
                want = C.epilogue(C.selected(g, inp.x, sel), inp.bias, inp.res, inp.act)
                assert want.shape == (g.n, g.f, g.oh, g.ow)
                assert np.array_equal(R.round_to(want, dt), want)
                assert np.array_equal(R.round_to(sel.w, dt), sel.w)
                if inp.grid:
                    assert np.abs(want).max() <= 16 and np.array_equal(want * 8, np.round(want * 8))
                if dense:
                    assert np.array_equal(want, C.epilogue(R.conv2d(inp.x, sel.w, *g.args), inp.bias, inp.res, inp.act))
        w = C.pixel_weights(name, dt)
        for deltas in C.pixel_rounds(g):
            x = C.delta_image(g, deltas)
            want = C.conv_sparse(g, x, w)
            assert np.array_equal(R.round_to(want, dt), want)
            if dense:
                assert np.array_equal(want, R.conv2d(x, w, *g.args))
    print(f"\n{name}: {g.macs:.3g} multiply-adds, {'checked against R.conv2d' if dense else 'rounding only'}")


def test_the_cases_left_to_the_rounding_check_are_the_larger_half():
    skipped = [n for n, g in C.CASES.items() if g.macs > DENSE_MACS]
    print("\nnot run through R.conv2d:", ", ".join(skipped))
    assert len(skipped) <= len(C.CASES) // 2
    # every route and form still has a case that is
    kept = {(g.route, g.form, g.gpu_route) for g in C.CASES.values() if g.macs <= DENSE_MACS}
    assert {(g.route, g.form, g.gpu_route) for g in C.CASES.values()} - kept <= {("tap_gemm_splitk", "", "tap_gemm_splitk")}


@pytest.mark.parametrize("name", list(C.STEM_POOL))
def test_stem_pool_expected_values(name):
    g = C.STEM_POOL[name]
    for dt in ("f16", "bf16"):
        for mode in C.STEM_MODES:
            inp = C.tap_inputs(name, dt, mode, "stem")
            for sel in C.tap_rounds(g):
                want = C.stem_pool_selected(g, inp.x, sel, inp.bias)
                ref = R.pool2d(np.maximum(C.epilogue(R.conv2d(inp.x, sel.w, *g.args), inp.bias, None, 0), 0), "max", 3, 3, 1, 1, 1, 1, 2, 2, 0)
                assert np.array_equal(want, ref) and np.array_equal(R.round_to(want, dt), want)
    assert {(c, r, s) for sel in C.tap_rounds(g) for c, r, s in zip(sel.c, sel.r, sel.s)} == {(c, r, s) for c in (0, 2) for r in range(7)
                                                                                            for s in range(7)}


@pytest.mark.parametrize("name", list(C.CONVT))
def test_conv_transpose_expected_values(name):
    cfg = C.CONVT[name]
    n, f, h, w, cg, r, s, ph, pw, sh, sw, dh, dw, oph, opw, groups = cfg
    rounds = C.convt_rounds(cfg)
    for dt in ("f32", "f16", "bf16"):
        x = C.storage_normal(np.random.default_rng(5), (n, f, h, w), dt)
        for sel in rounds:
            want = C.convt_selected(cfg, x, sel)
            assert np.array_equal(want, R.conv_transpose2d(x, sel.w, ph, pw, sh, sw, dh, dw, oph, opw, groups))
            assert np.array_equal(R.round_to(want, dt), want)
            assert ((sel.w != 0).sum(axis=(0, 2, 3)) == groups).all()  # one non-zero per output channel (cg columns x groups)
    fg = f // groups
    assert {(c, rr, ss) for sel in rounds for c, rr, ss in zip(sel.f % fg, sel.r, sel.s)} == {(c, rr, ss) for c in (0, fg - 1)
                                                                                             for rr in range(r) for ss in range(s)}


@pytest.mark.parametrize("name", list(C.CASES))
def test_coverage(name):
    g = C.CASES[name]
    rounds = C.tap_rounds(g)
    assert len(rounds) <= C.MAX_TAP_ROUNDS
    got = {(c, r, s) for sel in rounds for c, r, s in zip(sel.c, sel.r, sel.s)}
    chans = C.target_channels(g.cpg, g.f, g.r * g.s)
    assert set(C.required_channels(g.cpg)) <= set(chans)
    every = C.boundary_channels(g.cpg)
    assert {c for b in (8, 32, 64) for k in range(b, g.cpg, b) for c in (k - 1, k)} | {0, g.cpg - 1} == set(every)
    if -(-len(every) * g.r * g.s // g.f) <= C.MAX_TAP_ROUNDS:  # nothing to thin: both sides of every 8- and 32-boundary too
        assert chans == every
    assert got == {(c, r, s) for c in chans for r in range(g.r) for s in range(g.s)}
    for sel in rounds:  # every filter carries exactly one target, with a value of the cycle
        assert ((sel.w != 0).reshape(g.f, -1).sum(axis=1) == 1).all()
        assert set(np.unique(sel.v)) <= set(C.W_VALUES)
    if g.f >= 4:
        assert {v for sel in rounds for v in sel.v} == set(C.W_VALUES)
    pr = C.pixel_rounds(g)
    assert 1 <= len(pr) <= C.MAX_PIXEL_ROUNDS
    assert set(C.target_pixels(g.h, g.w)) <= {(d[2], d[3]) for rnd in pr for d in rnd}
    for rnd in pr:
        assert (g.n - 1, g.c - 1, g.h - 1, g.w - 1) in {d[:4] for d in rnd}, "the element where the tensor ends"
        assert {d[4] for d in rnd} <= set(C.DELTA_VALUES)
    pixel_chans = {d[1] for rnd in pr for d in rnd}
    assert {0, g.c - 1} <= pixel_chans


@pytest.mark.parametrize("name", list(C.CASES))
def test_index_mutations_change_a_selector_round(name):
    g = C.CASES[name]
    dt = g.dts[0]
    seen = []
    for mut in C.INDEX_MUTATIONS:
        mode = {"bias_of_previous_filter": "bias", "skip_residual_last_pixel": "res"}.get(mut, "plain")
        if mode not in g.modes:
            continue
        inp = C.tap_inputs(name, dt, mode)
        if not C.mutation_applies(g, mut, inp.bias is not None, inp.res is not None):
            continue
        hit = None
        for j, sel in enumerate(C.tap_rounds(g)):
            if not np.array_equal(C.forward(g, inp.x, sel.w, inp.bias, inp.res, inp.act, mut),
                                  C.epilogue(C.selected(g, inp.x, sel), inp.bias, inp.res, inp.act)):
                hit = f"tap round {j}"
                break
        if hit is None and mode == "plain":
            w = C.pixel_weights(name, dt)
            for j, deltas in enumerate(C.pixel_rounds(g)):
                x = C.delta_image(g, deltas)
                if not np.array_equal(C.forward(g, x, w, mut=mut), C.conv_sparse(g, x, w)):
                    hit = f"pixel round {j}"
                    break
        assert hit is not None, (name, mut)
        seen.append(f"{mut} ({hit})")
    print(f"\n{name}: " + ", ".join(seen))
    assert len(seen) >= 3


def test_mutations_are_defects_and_the_unmutated_forward_is_the_oracle():
    """On dense random inputs: forward(None) is R.conv2d, every mutation differs from it, the three evaluators agree."""
    g = C.CASES["generic-grouped-asym"]
    rng = np.random.default_rng(0)
    x, w = rng.standard_normal((g.n, g.c, g.h, g.w)), rng.standard_normal((g.f, g.cpg, g.r, g.s))
    b, res = C.grid_bias(g.f), C.grid_residual(rng, (g.n, g.f, g.oh, g.ow))
    want = C.epilogue(R.conv2d(x, w, *g.args), b, res, 0)
    assert np.allclose(C.forward(g, x, w, b, res), want, rtol=0, atol=1e-12)
    for mut in C.INDEX_MUTATIONS:
        assert C.mutation_applies(g, mut, True, True) and np.abs(C.forward(g, x, w, b, res, 0, mut) - want).max() > 1e-3, mut
    xs = C.delta_image(g, C.pixel_rounds(g)[0])
    for leak in (False, True):
        assert np.allclose(C.conv_sparse(g, xs, w, leak), C.conv_dense(g, C.padded(g, xs, leak), w), rtol=0, atol=1e-12)
    sel = C.tap_rounds(g)[0]
    for leak in (False, True):
        assert np.array_equal(C.conv_onehot(g, C.padded(g, x, leak), sel.w), C.conv_dense(g, C.padded(g, x, leak), sel.w))
    assert np.allclose(C.forward_rounded_partials(g, x, w, "f32", b, res, every=10 ** 6), want, rtol=1e-6, atol=1e-6)


def test_what_the_allclose_form_misses():
    import test_gpu_nn as N

    cfg = (1, 512, 7, 7, 130, 512, 3, 3, 1, 1, 1, 1, 1, 1)
    assert cfg in N.CONVS
    ref = C.random_reference("oracle", cfg, "bf16")
    passes = {}
    for mut in ("drop_corner", "neighbour_last_slot"):
        y = C.forward(ref.g, ref.x, ref.w, mut=mut)
        passes[mut] = bool(np.allclose(y, ref.want, rtol=1.6e-2, atol=1.6e-2))
        worst, idx = C.worst_ratio(y, ref.want, ref.bound)
        print(f"\n{mut}: allclose {'passes' if passes[mut] else 'fails'}, max err {np.abs(y - ref.want).max():.4f}, worst err/bound {worst:.3g} at {idx}")
        assert worst > 8.0, "the per-element bound sees it"
    assert passes == {"drop_corner": True, "neighbour_last_slot": False}


_RANDOM = C.random_params()


@pytest.mark.parametrize("family,cfg", _RANDOM, ids=[C.random_geom(f, c).name for f, c in _RANDOM])
def test_per_element_bound_admits_the_rounded_reference_and_not_16_bit_partial_sums(family, cfg):
    for dt in ("f16", "bf16"):
        ref = C.random_reference(family, cfg, dt)
        g = ref.g
        worst = C.assert_within(R.round_to(ref.want, dt), ref.want, ref.bound, f"{g.name} {dt} rounded reference")
        line = f"\n{g.name} {dt}: K = {g.k}{'' if ref.coords is None else ' (sampled)'}, rounded reference worst err/bound {worst:.3f}"
        assert worst <= 0.5 + 1e-9  # half a storage ulp against a whole one
        if C.inside_k(g) >= K_NUMERICS and ref.coords is None:
            y = R.round_to(C.forward_rounded_partials(g, ref.x, ref.w, dt, ref.bias, ref.res, ref.act), dt)
            factor, idx = C.worst_ratio(y, ref.want, ref.bound)
            line += f", partial sums in {dt}: {factor:.3g} at {idx}"
            assert factor > 1.0, (g.name, dt, factor)
        print(line, end="")


def test_rounding_before_the_residual_needs_its_own_term_and_fits_it():
    """The pixel-slot GEMM computes act(round(conv + bias) + residual) (csrc/gemm256p_kernel.h): replayed in numpy on the inputs of
    test_conv_pointwise_gemm_mode[bias_res_relu], that arithmetic misses the shared bound (near-zero sums of O(1) terms keep the
    rounding error of the O(1) intermediate) and stays within the bound with the derived term u |conv + bias|."""
    assert C.ROUNDS_BEFORE_RESIDUAL == ("pixel_gemm",)
    for dt in ("f16", "bf16"):
        ref = C.random_reference("pw_gemm", (3, 64, 8, 8, 256), dt)
        y = R.round_to(np.maximum(R.round_to(ref.pre, dt) + ref.res, 0), dt)
        shared, _ = C.worst_ratio(y, ref.want, ref.bound)
        own = C.assert_within(y, ref.want, ref.bound_rounded_pre, f"two roundings {dt}")
        print(f"\nround(conv + bias) + residual in {dt}: worst err/bound {shared:.3g} against the shared bound, {own:.3f} with u |conv + bias|")
        assert shared > 1.0 and own <= 1.0


def test_the_random_cases_cover_every_family_and_a_long_k():
    fams = {f for f, _ in _RANDOM}
    assert fams == set(C.RANDOM_FAMILIES)
    assert max(C.random_geom(f, c).k for f, c in _RANDOM) >= 4608
    dropped = [C.random_geom(f, tuple(c)).name for f in C.RANDOM_FAMILIES for c in C.random_lists()[f] if (f, tuple(c)) not in _RANDOM]
    print("\nleft out (above MAX_RANDOM_MACS):", ", ".join(dropped))


@pytest.mark.parametrize("name", list(C.CASES))
def test_declared_routes_are_the_planners(name, monkeypatch):
    g = C.CASES[name]
    for k, v in g.env.items():
        monkeypatch.setenv(k, str(v))
    for dt in g.dts:
        for mode in g.modes:
            _, _, has_res, act = C.MODES[mode]
            got = ops.conv_plan_route(TD[dt], g.n, g.c, g.h, g.w, g.f, g.r, g.s, g.ph, g.pw, g.sh, g.sw, g.dh, g.dw, g.groups, act, has_res,
                                      g.variant, 256)
            assert got == (g.route, g.form), (name, dt, mode, got)
    assert g.gpu_route == g.route or (g.route, g.gpu_route) == ("igemm32", "igemm32_splitk")  # (the launcher's refinement: conv.hip)


def test_the_table_reaches_every_route_and_form():
    routes = {g.gpu_route for g in C.CASES.values()}
    assert routes == {"igemm32", "igemm32_splitk", "batched_gemm32", "direct32", "depthwise", "pixel_gemm", "tap_gemm", "tap_gemm_splitk",
                      "tap_shifted", "resident", "batched_gemm", "generic"}  # (+ "stem_pool": STEM_POOL)
    assert {g.form for g in C.CASES.values()} == {"", "pw", "rowtap", "patch_wide", "patch", "resident", "s1<1,4,32>", "s1<2,2,32>", "s1<2,2,64>"}
    for key, values in (("IROCM_CONV_PW_NT", {2, 3, 4}), ("IROCM_CONV_TAP_NT", {2, 3, 4}), ("IROCM_CONV_TAP_SPLIT", {2, 4}),
                        ("IROCM_CONV32_SPLIT", {3, 4}), ("IROCM_CONV32_TILE", {2})):
        assert {g.env[key] for g in C.CASES.values() if key in g.env} == values
