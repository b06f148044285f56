"""The instruments of tests/test_gpu_rowop_selectors.py, proved on the oracle alone (no GPU): tests/rowop_cases.py.

1. the mirror of the dispatch answers every case with the route the case declares, and the table reaches every route the mirror
   can return, for f32, f16 and bf16 (Softmax, LayerNorm, RMSNorm, add_norm with and without `pre`);
2. every required target is the p of some row that is launched;
3. every selector expectation equals the oracle exactly where it is declared exact and lies within the bound elsewhere;
4. a numpy float32 replay of every kernel's order of operations stays at or below HALF the bound on every family of the table and
   on the random inputs: the fp32 value the kernel rounds to storage against 2^-24 |want| + E_f32, the bound of an f32 launch
   (C.replay_bound says why not E_f32 alone), and the value rounded to storage within the whole bound;
5. every mutation misses the bound on at least one selector family, by the factors printed (pytest -s);
6. the share of random-input elements a mutated operator still gets through the TOL of tests/test_gpu_rowops.py.

Largest replay err / bound per (op, dtype), item 4, as printed by test_expectations_equal_the_oracle_and_replays_stay_below_half_the_bound:

                  f32     f16     bf16
    softmax       0.338   0.260   0.240    mask rows (the random inputs reach 0.32)
    layer_norm    0.143   0.130   0.130    pair rows (random inputs: 0.46 in f32, the last fma's half ulp counted twice)
    rms_norm      0.174   0.145   0.145
    add_norm      0.205   0.171   0.173    the rows whose two roundings matter

Item 5, the largest finite err / bound per mutation (inf: the mutated row holds inf, NaN or the output fill):
    softmax     drop_from_sum, drop_from_max, tail_zero_filled, tail_unstored, group_row_from_first, online_no_guard: inf each.
                drop_from_max is seen by the SINGLE rows only: with two equal maxima the other one still gives the right maximum.
    norms       drop_from_mean 8.4e5, drop_from_var 5.2e5, padding_adds_mu2 5.4e5 (c = 3 only), scale_off_by_a_chunk 1.1e9,
                scale1_read_as_vector 9.1e8, bias1_ignored 8.4e6, eps_dropped 4.9e3 (rows of 512 elements and more)
    add-norm    sum_not_rounded 986 and b_before_pre 3.2e3 (16-bit types: an fp32 sum is its own storage rounding),
                fallback_reads_overwritten_b 7.2e7
Item 6, examples (16-bit, one element dropped): softmax (7, 1000) drop_from_sum passes TOL on 100 % of the elements and the bound on
99.97 %; LayerNorm (3, 4096) drop_from_mean passes TOL on 100 %, the bound on 61 - 77 % (f16) — random inputs see such a defect
through the bound only in part, the selector rows see it whole.
"""
import numpy as np
import pytest

import rowop_cases as C
from oracle import ref_ops as R

TOL = {"f32": (1e-4, 1e-6), "f16": (2e-3, 1e-3), "bf16": (1.6e-2, 8e-3)}  # of tests/test_gpu_rowops.py


def mirror(cs):
    return C.route(cs.op, cs.dt, cs.outer, cs.n, cs.inner, cs.aligned, int(cs.add > 0), cs.add == 2)


def unique_families(op=None):
    """(case, family) once per distinct family of the table (the cases of one row length share theirs)."""
    seen, built = set(), set()
    for cs in sorted(C.cases_of(op), key=lambda c: (-len(c.kinds), not c.all_forms)):  # the cases with the most families first
        whole = (cs.op, C.norm_route_of(cs), cs.dt, cs.n, cs.rms, cs.eps, cs.add)
        if (whole, cs.kinds, cs.all_forms) in built or (whole, ("pair",)) in built and cs.kinds == ("pair",) and not cs.all_forms:
            continue  # the same families as a case before it (they differ in the rows launched, not in the patterns)
        built.update({(whole, cs.kinds, cs.all_forms), (whole, ("pair",))} if "pair" in cs.kinds else {(whole, cs.kinds, cs.all_forms)})
        for fam in C.families(cs):
            key = (cs.op, C.norm_route_of(cs), cs.dt, cs.n, fam.kind, getattr(fam, "form", None), cs.rms, cs.eps, cs.add)
            if key not in seen:
                seen.add(key)
                yield cs, sampled(fam)


MAX_DENSE = 150000  # elements of a family the dense fp64 oracle and the replay go through; above: every k-th pattern row


def sampled(fam):
    P, n = fam.x.shape
    step = -(-P * n // MAX_DENSE)
    if step <= 1:
        return fam
    rows = np.arange(0, P, step)
    return C.SimpleNamespace(**{k: (v[rows] if isinstance(v, np.ndarray) and v.shape[:1] == (P,) and k not in ("g", "b", "pre") else v)
                                for k, v in vars(fam).items()})


def test_every_case_takes_the_route_it_declares():
    wrong = [(cs.name, cs.route, mirror(cs)) for cs in C.CASES.values() if mirror(cs) != cs.route]
    assert not wrong, wrong[:5]
    for cs in C.CASES.values():
        assert (cs.n % C.VEC[cs.dt] != 0) == (cs.form == "odd_n") or cs.inner != 1, cs.name
        assert cs.n * cs.outer * cs.inner * C.SIZE[cs.dt] <= 128 << 20


@pytest.mark.parametrize("dt", C.DTS)
def test_the_table_reaches_every_route(dt):
    for op, pre in (("softmax", False), ("layer_norm", False), ("rms_norm", False), ("add_norm", False), ("add_norm", True)):
        have = {cs.route for cs in C.cases_of(op, dt) if op != "add_norm" or (cs.add == 2) == pre}
        want = C.scan_routes(op, dt, pre)
        assert have == want, (op, pre, sorted(want - have), sorted(have - want))
        # every ALIGNED = false route in both forms, every route with 1 row and with 5
        for r in want:
            cases = [cs for cs in C.cases_of(op, dt) if cs.route == r and (op != "add_norm" or (cs.add == 2) == pre)]
            if "unaligned" in r:
                assert {"odd_n", "offset"} <= {cs.form for cs in cases}, r
            if op != "add_norm" and r != "softmax_strided" and not r.endswith(("R2", "R4")):
                assert {1, C.ROWS} <= {cs.outer for cs in cases}, r
    # the second trips of the persistent loops and the row groups
    outers = {(cs.route.split("/")[0], cs.route.split("/")[-1], cs.outer) for cs in C.cases_of(dt=dt)}
    assert {("softmax_wave", "R4", 4099), ("softmax_wave", "R2", 4099), ("softmax_wave", "R4", 32771), ("softmax_wave", "R2", 16387),
            ("softmax_wave", "R1", 8195), ("softmax_blockreg", "C4", 8195), ("softmax_block", "unaligned", 8195),
            ("norm_rows", "ADD0", 4099), ("norm_rows", "ADD1", 4099), ("norm_rows", "ADD2", 4099), ("norm_wave", "R1", 8195),
            ("norm_blockreg", "ADD0", 8195), ("norm_blockreg", "ADD1", 8195), ("norm_block", "unaligned", 8195)} <= outers


def test_every_required_target_is_selected():
    checked = 0
    for cs in C.CASES.values():
        if cs.outer * cs.inner < C.ROWS:
            continue
        r = C.norm_route_of(cs)
        p = C.pattern_targets(r, cs.dt, cs.n)  # the p of every family with selectors (softmax_pair, pair_rows)
        fam = C.SimpleNamespace(p=p, x=p[:, None])
        req, _ = C.targets(r, cs.dt, cs.n)
        assert set(req) <= C.covered(cs, fam), (cs.name, sorted(set(req) - C.covered(cs, fam))[:5])
        v, n = C.VEC[cs.dt], cs.n
        assert {0, n - 1} <= set(req) and all(x in req for k in range(64 * v, n, 64 * v) for x in (k - 1, k))
        checked += 1
    assert checked > 500


def oracle_of(cs, fam):
    if cs.op == "softmax":
        with np.errstate(invalid="ignore"):
            return R.softmax(fam.x, -1)
    x = fam.x if cs.op != "add_norm" else R.round_to((R.round_to(fam.a + fam.pre, cs.dt) if fam.pre is not None else fam.a) + fam.b2, cs.dt)
    return R.rms_norm(x, fam.g, fam.eps) if cs.rms else R.layer_norm(x, fam.g, fam.b, fam.eps, -1)


def expectation_equals_the_oracle(cs, fam):
    ref = oracle_of(cs, fam)
    if fam.exact:
        C.assert_exact(fam.want, ref, f"{cs.name} {fam.kind}")
        assert np.array_equal(R.round_to(fam.want, cs.dt), fam.want), cs.name  # representable: the GPU file compares with ==
    else:
        C.assert_within(fam.want, ref, fam.bound * 1e-3, f"{cs.name} {fam.kind}")  # (the closed forms: fp64 noise only)
    return fam.exact


def replayed(cs, fam):
    nr = C.norm_route_of(cs)
    if cs.op == "softmax":
        return C.replay_softmax(fam.x, cs.route, cs.dt, rounded=False)
    return C.replay_norm(fam.x, fam.g, fam.b, fam.eps, cs.rms, nr, cs.dt, rounded=False)



@pytest.mark.parametrize("op", ["softmax", "layer_norm", "rms_norm", "add_norm"])
def test_expectations_equal_the_oracle_and_replays_stay_below_half_the_bound(op):
    """Items 3 and 4, in one walk over the families."""
    worst, exact = {}, 0
    for cs, fam in unique_families(op):
        exact += expectation_equals_the_oracle(cs, fam)
        if op == "add_norm" and fam.kind == "pair":
            continue  # the rows, the depth of the sums and so the bound of the norm families of this n, replayed there
        got = replayed(cs, fam)
        ratio, idx = C.worst_ratio(got, fam.want, C.replay_bound(fam))
        assert C.worst_ratio(R.round_to(got, cs.dt), fam.want, C.bound_of(fam))[0] <= 1.0, (cs.name, fam.kind)
        assert ratio <= 0.5, (cs.name, fam.kind, getattr(fam, "form", None), ratio, idx, got[idx], fam.want[idx])
        key = (op, cs.dt)
        if ratio > worst.get(key, (0, ""))[0]:
            worst[key] = (ratio, f"{cs.name} {fam.kind} {idx}")
    assert exact >= (3 if op == "layer_norm" else 0) + (30 if op == "softmax" else 0)
    for key, (ratio, where) in sorted(worst.items()):
        print(f"replay worst err/bound {key[0]:>10} {key[1]:>4}: {ratio:.3f}  {where}")
    for params in C.random_params():
        if params[0] != op:
            continue
        ref = C.random_reference(*params)
        o, dt, shape, axis, wb, r = params
        n = shape[axis % len(shape)] if op == "softmax" else int(np.prod(shape[axis % len(shape):]))
        if op == "softmax":
            x2 = np.moveaxis(ref.x, axis, -1).reshape(-1, n)
            got = np.moveaxis(C.replay_softmax(x2, r, dt, rounded=False).reshape(np.moveaxis(ref.x, axis, -1).shape), -1, axis)
        else:
            got = C.replay_norm(ref.x.reshape(-1, n), ref.g.ravel(), None if ref.b is None else ref.b.ravel(), C.EPS, op == "rms_norm", r,
                                dt, rounded=False).reshape(shape)
        ratio, idx = C.worst_ratio(got, ref.want, C.replay_bound(C.SimpleNamespace(exact=False, want=ref.want, e32=ref.e32)))
        assert C.worst_ratio(R.round_to(got, dt), ref.want, ref.bound)[0] <= 1.0, params
        print(f"replay random {op} {dt} {shape} {r}: {ratio:.3f}")
        assert ratio <= 0.5, (params, ratio, idx)
    C.release()


def mutated(cs, fam, mut, idx):
    """The rows of one launch (pattern indices idx) through the operator with the defect -> got, want, bound of those rows."""
    nr = C.norm_route_of(cs)
    if cs.op == "softmax":
        got = C.softmax_forward(fam.x[idx], cs.route, cs.dt, mut, rows_per_group=int(cs.route[-1]) if cs.route[-1] in "24" else 1)
    elif cs.op == "add_norm":
        sub = C.SimpleNamespace(**{**vars(fam), "a": fam.a[idx], "b2": fam.b2[idx]})
        got = C.add_forward(sub, nr, cs.dt, mut, alias="b") if mut in C.ADD_MUTATIONS else C.norm_forward(fam.x[idx], fam.g, fam.b, fam.eps, cs.rms, nr, cs.dt, mut)
    else:
        got = C.norm_forward(fam.x[idx], fam.g, fam.b, fam.eps, cs.rms, nr, cs.dt, mut)
    return R.round_to(got, cs.dt), fam.want[idx], C.bound_of(fam)[idx]


@pytest.mark.parametrize("mut", C.SOFTMAX_MUTATIONS + C.NORM_MUTATIONS + C.ADD_MUTATIONS)
def test_every_mutation_misses_the_bound(mut):
    ops = ("softmax",) if mut in C.SOFTMAX_MUTATIONS else (("add_norm",) if mut in C.ADD_MUTATIONS else ("layer_norm", "rms_norm", "add_norm"))
    caught, missed, best = 0, [], (0.0, "")
    for dt in C.DTS:
        per_dt = 0
        for cs in C.CASES.values():
            if cs.op not in ops or cs.dt != dt or cs.outer > 5000 or cs.n > 2200 or (cs.outer != C.ROWS and not cs.route.endswith(("R2", "R4"))
                                                                      and cs.route != "softmax_strided"):
                continue
            hit = False
            for fam in C.families(cs):
                if not C.mutation_applies(mut, cs, fam):
                    continue
                for idx in C.launches(cs, fam)[:C.MAX_REQUIRED_ROUNDS]:
                    idx = idx[:64]
                    got, want, bound = mutated(cs, fam, mut, idx)
                    ratio, _ = C.worst_ratio(got, want, bound)
                    if ratio > 1.0:
                        hit = True
                        per_dt += 1
                        if best[0] < ratio < np.inf or best[0] == 0.0:
                            best = (ratio, f"{cs.name} {fam.kind}")
                        break
                if hit:
                    break
            else:
                if any(C.mutation_applies(mut, cs, f) for f in C.families(cs)):
                    missed.append(cs.name)
            caught += hit
        # (an fp32 sum IS its storage rounding, and with h = 2^-24 both orders of the two sums round to 1)
        assert per_dt > 0 or (mut in ("sum_not_rounded", "b_before_pre") and dt == "f32"), (mut, dt)
    print(f"mutation {mut}: caught on {caught} cases, largest finite err/bound {best[0]:.3g} ({best[1]}); not seen on {len(missed)}: {missed[:4]}")
    assert caught > 0
    C.release()


def test_what_the_old_tolerances_let_through():
    """Evidence of the gap: the share of elements of the random inputs of tests/test_gpu_rowops.py that a mutated operator still gets
    through np.allclose at TOL, next to the share the per-element bound lets through."""
    for params in C.random_params():
        op, dt, shape, axis, wb, r = params
        if dt == "f32" or int(np.prod(shape)) > 200000:
            continue
        ref = C.random_reference(*params)
        rtol, atol = TOL[dt]
        n = shape[axis % len(shape)] if op == "softmax" else int(np.prod(shape[axis % len(shape):]))
        for mut in (("drop_from_sum", "tail_zero_filled") if op == "softmax" else ("drop_from_mean", "drop_from_var", "eps_dropped")):
            if op == "softmax":
                if _is_strided(shape, axis) or (mut == "tail_zero_filled" and not C.padded(r, dt, n)):
                    continue
                x2 = np.moveaxis(ref.x, axis, -1).reshape(-1, n)
                got = np.moveaxis(C.softmax_forward(x2, r, dt, mut).reshape(np.moveaxis(ref.x, axis, -1).shape), -1, axis)
                at = atol
            else:
                if op == "rms_norm" and mut == "drop_from_mean":
                    continue
                got = C.norm_forward(ref.x.reshape(-1, n), ref.g.ravel(), None if ref.b is None else ref.b.ravel(), C.EPS, op == "rms_norm", r,
                                     dt, mut).reshape(shape)
                at = max(atol, rtol)
            got = R.round_to(got, dt)
            old = np.mean(np.abs(got - ref.want) <= at + rtol * np.abs(ref.want))
            new = np.mean(np.abs(got - ref.want) <= ref.bound)
            print(f"{op} {dt} {shape} {r} {mut}: passes TOL {old:.4f}, passes the bound {new:.4f}")
            assert new <= old
    C.release()


def _is_strided(shape, axis):
    return int(np.prod(shape[axis % len(shape) + 1:])) != 1
