"""The selector inputs and the checker of tests/attention_cases.py, proved on the oracle alone (no GPU): the fp64 reference
rounded once to the storage type passes assert_within on every case tests/test_gpu_attention_selectors.py runs, and every
subtly wrong attention below misses the bound by a factor of at least 8 wherever it applies. Each test prints the worst
err / bound of the unmutated reference and of every mutation (pytest -s)."""
import numpy as np
import pytest
import torch

import attention_cases as C
from infinitensor_amd import ops
from oracle import ref_ops as R

TD = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
MIN_RATIO = 8.0


def fails(name, got, c, rows=None):
    """The mutated result must miss the bound by MIN_RATIO somewhere (within `rows` [BH, Sq] when given)."""
    got, want, bound = got, c.want, c.bound
    if rows is not None:
        assert rows.any(), name
        got, want, bound = got[rows], want[rows], bound[rows]
    worst, idx = C.worst_ratio(got, want, bound)
    print(f"    {name}: worst err/bound {worst:.3g}")
    assert worst >= MIN_RATIO, (name, worst, idx)


def online_without_rescale(q, k, v, scale, add):
    """Online softmax over 64-key tiles whose running sums are never rescaled when the maximum moves (alpha = 1)."""
    s = np.matmul(q, np.swapaxes(k, -1, -2)) * scale + add
    m = np.full(s.shape[:-1] + (1,), -np.inf)
    l = np.zeros_like(m)
    o = np.zeros(s.shape[:-1] + (v.shape[-1],))
    for k0 in range(0, s.shape[-1], C.KT):
        st = s[..., k0:k0 + C.KT]
        m = np.maximum(m, st.max(-1, keepdims=True))
        with np.errstate(invalid="ignore"):
            e = np.where(np.isfinite(m), np.exp(st - np.where(np.isfinite(m), m, 0.0)), 0.0)
        l = l + e.sum(-1, keepdims=True)
        o = o + np.matmul(e, v[..., k0:k0 + C.KT, :])
    return o / np.where(l > 0, l, 1.0)


@pytest.mark.parametrize("p", C.prefill_params(), ids=C.prefill_id)
def test_prefill_selectors_reference_passes_and_mutations_fail(p):
    c = C.prefill_case(*p)
    bh, sq, sk, group, G = c.bh, c.sq, c.sk, c.group, c.G
    add = C.additive(c.mask3, group, bh, sq, sk, c.causal)
    worst = C.assert_within(R.round_to(c.want, c.dt), c.want, c.bound, "rounded reference")
    print(f"\n{C.prefill_id(p)}: g = {c.g}, rounded reference worst err/bound {worst:.3g}")
    assert worst <= 1.0
    # what the rows promise: a single winner has (nearly) all the weight, a tie is an exact half and half, dead rows are 0
    hh = np.arange(bh)[:, None]
    vmax = np.abs(c.v).max()
    single = c.kind == "target"
    assert (np.take_along_axis(c.p, np.maximum(c.winner, 0)[..., None], -1)[..., 0][single] >= C.P_STAR).all()
    assert np.abs(c.want - c.v[hh, np.maximum(c.winner, 0)])[single].max() <= 2.0 ** -11 * vmax
    for h, i, a, b in c.ties:
        assert c.p[h, i, a] == c.p[h, i, b] and c.p[h, i, a] > 0.49
    assert (c.want[c.dead] == 0).all() and (c.bound[c.dead] == 0).all()
    assert c.dead.any() == (c.mask_form == 2 or (c.causal and (sk < sq or (sk == sq and c.mask_form == 1))))

    # (a) one target key dropped — each special key in turn, in every head where a live row wins with it
    for x in c.specials:
        rows = (c.winner == x) & ~c.dead
        a2 = add.copy()
        a2[:, :, x] = -np.inf
        fails(f"(a) key {x} dropped", C.attend(c.q, c.k, c.v, c.scale, a2), c, rows)
    if c.causal:
        # (b) the causal limit off by one, either way
        up = C.additive(c.mask3, group, bh, sq, sk, True, shift=1)
        fails("(b) key lim + 1 admitted", C.attend(c.q, c.k, c.v, c.scale, up), c, c.kind == "cdecoy")
        down = C.additive(c.mask3, group, bh, sq, sk, True, shift=-1)
        rows = (c.winner == c.lim[None, :]) & ~c.dead
        fails("(b) key lim dropped", C.attend(c.q, c.k, c.v, c.scale, down), c, rows)
    # (c) keys >= Sk admitted as copies of row Sk - 1 (the clamped loads of the ragged tile, unmasked)
    pad = (-sk) % C.KT
    tie_last = np.zeros((bh, sq), dtype=bool)
    for h, i, a, b in c.ties:
        tie_last[h, i] |= a == sk - 1
    if pad:
        rep = lambda t: np.concatenate([t, np.repeat(t[:, -1:], pad, axis=1)], axis=1)  # noqa: E731
        a2 = np.concatenate([add, np.repeat(add[:, :, -1:], pad, axis=2)], axis=2)
        fails("(c) keys past Sk admitted", C.attend(c.q, rep(c.k), rep(c.v), c.scale, a2), c, tie_last)
    if c.mask_form == 1:
        # (d) the per-key mask shifted by one key
        m = np.broadcast_to(np.roll(c.mask, 1, axis=1)[:, None, :], (G, sq, sk))
        fails("(d) per-key mask shifted by a key", C.attend(c.q, c.k, c.v, c.scale, C.additive(m, group, bh, sq, sk, c.causal)),
              c, np.isin(c.kind, ("mdecoy", "bias")))
    if c.mask_form == 2:
        # (d) the full mask shifted by one query row
        m = np.roll(c.mask, 1, axis=1)
        fails("(d) full mask shifted by a row", C.attend(c.q, c.k, c.v, c.scale, C.additive(m, group, bh, sq, sk, c.causal)),
              c, np.isin(c.kind, ("mdecoy", "bias")))
    if c.mask_form and group > 1:
        # (e) head h takes mask row h (wrapped into the G rows there are) instead of h // group
        a2 = C.additive(c.mask3[np.arange(bh) % G], 1, bh, sq, sk, c.causal)
        fails("(e) mask row by head, not by group", C.attend(c.q, c.k, c.v, c.scale, a2), c)
    # (i) running sums not rescaled when the maximum moves: every row whose winner lies past the first tile, ties included
    if sk > C.KT:
        got = online_without_rescale(c.q, c.k, c.v, c.scale, add)
        fails("(i) no rescale, all rows", got, c)
        late = np.zeros((bh, sq), dtype=bool)
        for h, i, a, b in c.ties:
            late[h, i] |= min(a, b) >= C.KT
        if late.any():
            fails("(i) no rescale, ties past tile 0", got, c, late)


def test_prefill_params_cover_every_kernel_build():
    ps = C.prefill_params()
    assert len(set(ps)) == len(ps)
    builds = {(dt, d, causal, mf) for dt, d, _, _, causal, mf, _, _ in ps}
    assert builds == {(dt, d, ca, mf) for dt in ("f16", "bf16") for d in (64, 128) for ca in (False, True) for mf in (0, 1, 2)}
    assert {sc for *_, sc in ps} == {"imm", "div", "neg"}
    assert any(mf == 1 and h // 2 > 1 for _, _, _, _, _, mf, h, _ in ps)  # one per-key mask row serves several heads
    assert any(sk % 4 == 0 for _, _, _, sk, _, mf, _, _ in ps if mf) and any(sk % 4 for _, _, _, sk, _, mf, _, _ in ps if mf)


def test_builder_refuses_inputs_without_a_dominant_target(monkeypatch):
    monkeypatch.setattr(C, "P_STAR", 1.0 + 2.0 ** -30)  # a weight no softmax row can reach, whatever g
    with pytest.raises(ValueError, match="no g <= 64"):
        C.prefill_case.__wrapped__("f16", 64, 200, 200, False, 0, 2)


def test_checker_reports_the_worst_element():
    want = np.array([[1.0, 2.0], [0.0, 4.0]])
    bound = np.array([[0.1, 0.1], [0.0, 0.1]])
    got = want.copy()
    assert C.assert_within(got, want, bound) == 0.0
    got[0, 1] += 0.05
    assert abs(C.assert_within(got, want, bound) - 0.5) < 1e-12
    got[1, 1] -= 0.3
    with pytest.raises(AssertionError, match=r"worst err/bound 3 at \(1, 1\)"):
        C.assert_within(got, want, bound, "x")
    got = want.copy()
    got[1, 0] = 1e-30  # a zero bound admits the exact value only
    assert C.worst_ratio(got, want, bound) == (np.inf, (1, 0))
    got[1, 0] = np.nan
    assert C.worst_ratio(got, want, bound) == (np.inf, (1, 0))


def decode_builds(dt, d):
    K = ops.kvcache_keys_per_iteration(TD[dt], d)
    seen = []
    for pos, ms in C.DECODE_POSITIONS:
        for split in C.DECODE_SPLITS:
            key = (dt, d, pos, ms, C.decode_chunk_len(pos + 1, split, K))
            if key not in seen:
                seen.append(key)
    return seen


@pytest.mark.parametrize("dt", ["f32", "f16", "bf16"])
@pytest.mark.parametrize("d", ops.KVCACHE_HEAD_DIMS)
def test_decode_selectors_reference_passes_and_mutations_fail(dt, d):
    for key in decode_builds(dt, d):
        rounds = C.decode_case(*key)
        _, _, pos, ms, chunk_len = key
        print(f"\n{dt} d{d} pos {pos} of {ms}, chunk {chunk_len}: {len(rounds)} call(s), g = {[r.g for r in rounds]}")
        checked_h = 0
        for r in rounds:
            hh = np.arange(C.DECODE_HEADS)
            worst = C.assert_within(R.round_to(r.want, dt), r.want, r.bound, "rounded reference")
            print(f"    rounded reference: worst err/bound {worst:.3g}")
            assert (r.p[hh, 0, r.t] >= C.P_STAR).all()
            assert (r.kc[:, pos:] == 2 * np.where((r.t == pos)[:, None], r.kn[:, 0], r.kc[hh, np.minimum(r.t, pos - 1)])[:, None]).all()
            assert (r.vc[:, pos:] == C.DECOY_V).all()
            q = r.q.astype(np.float64)
            sc = 1.0 / np.sqrt(d)
            if pos + 1 < ms:
                # (f) one stale row past pos is read
                k2 = np.concatenate([r.valid_k, r.kc[:, pos + 1:pos + 2]], axis=1)
                v2 = np.concatenate([r.valid_v, r.vc[:, pos + 1:pos + 2]], axis=1)
                fails("(f) a stale row past pos read", C.attend(q, k2, v2, sc, 0.0), r)
            # (g) the stale cache row at pos instead of the new k / v
            k2, v2 = r.valid_k.copy(), r.valid_v.copy()
            k2[:, pos], v2[:, pos] = r.kc[:, pos], r.vc[:, pos]
            fails("(g) stale row at pos instead of k / v", C.attend(q, k2, v2, sc, 0.0), r)
            # (h) the last key of a chunk dropped: in the heads that ask for one
            lasts = np.array([c1 - 1 for _, c1 in r.chunks])
            add = np.zeros((C.DECODE_HEADS, 1, pos + 1))
            add[:, :, lasts] = -np.inf
            rows = np.isin(r.t, lasts)[:, None]
            if pos > 0 and rows.any():  # (a later call of a long target list may hold first keys only)
                checked_h += 1
                fails("(h) last key of every chunk dropped", C.attend(q, r.valid_k, r.valid_v, sc, add), r, rows)
        assert checked_h >= (pos > 0)


def test_decode_targets_cover_the_chunk_edges():
    assert C.decode_chunk_len(701, 5, 64) == 192 and C.decode_chunk_len(701, 16, 64) == 64 and C.decode_chunk_len(701, 1, 64) is None
    assert C.decode_chunks(701, 192) == [(0, 192), (192, 384), (384, 576), (576, 701)]
    assert C.decode_targets(700, 192) == [0, 700, 699, 191, 192, 383, 384, 575, 576]
    assert C.decode_targets(0, None) == [0]
    rounds = C.decode_case("f16", 64, 700, 1024, 64)  # 11 chunks: 22 edges + key 699 -> two calls
    assert len(rounds) == 2 and {0, 63, 64, 639, 640, 699, 700} <= set(int(x) for r in rounds for x in r.t)
