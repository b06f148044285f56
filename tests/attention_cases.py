"""Selector inputs and a per-element bound for the attention kernels (csrc/attention.hip, csrc/attention_kvcache.hip).

With standard-normal Q / K / V every softmax weight is about 1 / Sk: a key that is dropped, counted twice or wrongly admitted
moves an output by less than the tolerance of an allclose. The inputs built here make ONE key (or an exact 50/50 pair) carry
the whole weight of a query row, so that any such mistake is an O(1) error, and `assert_within` checks every element against
a bound made of the roundings the kernels are entitled to. numpy and oracle/ref_ops.py only: imports without a GPU.

Inputs
  K rows: distinct random +-1 vectors (exact in f16 and bf16), V: standard normal rounded to the storage type.
  Query row i = g * k[t(i)], g a power of two: with scale = 1 / sqrt(D) key t scores g * sqrt(D), every other key strictly
  less. The builders take the smallest g <= 64 for which the fp64 reference gives every single-target row the weight
  p* >= 1 - 2^-12 and raise if there is none (a condition on the inputs, checked on the CPU).
  Row kinds of a prefill case (mixed within the case):
    target  q = g k_t                      -> v_t
    tie     q = g (k_a + k_b), k_a.k_b = 0, a and b in different 64-key tiles: two equal integer scores -> (v_a + v_b) / 2;
            some ties use a = Sk - 1 (were the clamped rows past Sk not masked, key Sk - 1 would be counted many times)
    decoy   q = g (k_t + 2 k_x), x a key that must not count and would win if admitted: x = lim(i) + 1 under causal
            (lim(i) = i + Sk - Sq, t = lim(i)), or x hidden by the per-key / full mask with -inf or -10000
    bias    q = g (k_t + k_y): t and y tie for any pair of +-1 rows (both score g (D + k_t.k_y) / sqrt(D)); the mask holds
            the finite bias +16 at y, which moves the winner to y (weight of t: e^-16). A mask applied at the wrong key, the
            wrong row or in the wrong units leaves the tie or flips it.
    dead    no admissible key (causal with Sk < Sq, or every visible key at -inf): the output is exactly 0 (header of
            attention.hip); the oracle's NaN rows are replaced by 0 there and only there.

Bound (u = 2^-11 for f16, 2^-8 for bf16, 2^-24 for f32; A = sum_j p_j |v_j| from the fp64 reference)
      bound = u |want| + (2 u + 2^-16) A            f32 decode: u |want| + 2^-17 A
  - one rounding of the output to the storage type:                                         u |want|
    (f16 results below 2^-14 are subnormal, spaced 2^-24 apart whatever their size: there the rounding is u 2^-14, i.e.
    u max(|want|, 2^-14) — without it the fp64 reference rounded once to f16 misses the bound, which
    tests/test_attention_selectors_cpu.py found at outputs of about 7e-6)
  - P is rounded to 16 bits before the P V product (prefill), each weight by at most u:     u A
    (f16 prefill: a weight below 2^-14 of its row's largest is an f16 subnormal and is rounded by up to 2^-25 instead:
    + min(2^-25 sum_{such j} |v_j|, 2 u A), so that the P terms never exceed 4 u A. Found by replaying attention.hip's
    roundings in numpy on these inputs — P to f16, fp32 sums, one output rounding: outputs of 1e-5 .. 5e-5 beside a
    sharp target missed the plain bound by up to 1.17)
  - the normaliser is summed over the rounded (MFMA row sum) or the unrounded (VALU sum) weights, either within u of
    the sum the numerator uses:                                                             u A
  - fp32 accumulation: the project's convention of 2^-17 of the absolute sum (tests/test_gpu_matmul.py), once for the
    numerator and once for the normaliser:                                                  2^-16 A
  Decode keeps P in fp32, so the f32 bound has the accumulation term alone; the 16-bit decode types are checked with the
  prefill form (their only 16-bit rounding is the output's). The bound is derived, not fitted: no term comes from what a
  kernel returned.
"""
from __future__ import annotations

import functools
from types import SimpleNamespace

import numpy as np

from oracle import ref_ops as R

U = {"f16": 2.0 ** -11, "bf16": 2.0 ** -8, "f32": 2.0 ** -24}
KT = 64            # keys per tile of the prefill kernel
WG_ROWS = 128      # query rows per workgroup of the prefill kernel
P_STAR = 1.0 - 2.0 ** -12
BIAS = 16.0        # the finite additive bias of the bias rows (exact in every type)
DECOY_V = 1000.0   # V of the decode cache rows that must never be read (exact in every type)
NEG = (-np.inf, -10000.0)
F16_MIN_NORMAL = 2.0 ** -14


# ------------------------------------------------------------------------------------------------------------------------
# checker
# ------------------------------------------------------------------------------------------------------------------------
def f16_subnormal_weights(p: np.ndarray, absv: np.ndarray) -> np.ndarray:
    """2^-25 sum_j |v_j| over the keys whose weight is below 2^-14 of the row's largest: the kernel keeps P relative to the
    row maximum, and such a weight is an f16 subnormal, rounded by up to 2^-25 whatever its size."""
    top = p.max(axis=-1, keepdims=True)
    sub = (p < F16_MIN_NORMAL * top) & (p > 0)
    return 2.0 ** -25 * np.matmul(sub.astype(np.float64), absv)


def bound_for(dt: str, want: np.ndarray, absum: np.ndarray, decode: bool = False, p_sub=None) -> np.ndarray:
    u = U[dt]
    if dt == "f32":
        assert decode, "prefill has no f32 build"
        return u * np.abs(want) + 2.0 ** -17 * absum
    out = np.abs(want)
    if dt == "f16":  # (where A == 0 — a fully masked row — the result is exactly 0 and stays so)
        out = np.where(absum > 0, np.maximum(out, F16_MIN_NORMAL), out)
    extra = 0.0
    if dt == "f16" and p_sub is not None and not decode:
        extra = np.minimum(p_sub, 2 * u * absum)  # the P terms together never exceed 4 u A
    return u * out + (2 * u + 2.0 ** -16) * absum + extra


def worst_ratio(got, want, bound):
    """-> (worst err / bound, index of it). A zero bound admits only the exact value; NaN in `got` is an infinite error."""
    got, want, bound = (np.asarray(a, dtype=np.float64) for a in (got, want, bound))
    assert got.shape == want.shape == bound.shape, (got.shape, want.shape, bound.shape)
    err = np.abs(got - want)
    err = np.where(np.isnan(err), np.inf, err)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err == 0, 0.0, np.where(bound > 0, err / bound, np.inf))
    idx = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    return float(ratio[idx]), tuple(int(i) for i in idx)


def assert_within(got, want, bound, what: str = "") -> float:
    """Every |got - want| <= bound; the message names the worst err / bound and where it is. Returns the worst ratio."""
    worst, idx = worst_ratio(got, want, bound)
    assert worst <= 1.0, (f"{what}: worst err/bound {worst:.3g} at {idx}: got {np.asarray(got)[idx]!r}, "
                          f"want {np.asarray(want)[idx]!r}, bound {np.asarray(bound)[idx]:.3e}")
    return worst


# ------------------------------------------------------------------------------------------------------------------------
# fp64 reference pieces
# ------------------------------------------------------------------------------------------------------------------------
def weights(q, k, scale, add):
    """softmax(scale q k^T + add) in fp64 over [BH, Sq, Sk]; rows without an admissible key (all -inf) get weight 0
    everywhere. -> p, dead [BH, Sq]."""
    s = np.matmul(q, np.swapaxes(k, -1, -2)) * scale + add
    m = s.max(axis=-1, keepdims=True)
    dead = ~np.isfinite(m[..., 0])
    with np.errstate(invalid="ignore"):
        e = np.where(dead[..., None], 0.0, np.exp(s - np.where(dead[..., None], 0.0, m)))
    l = e.sum(axis=-1, keepdims=True)
    return e / np.where(l > 0, l, 1.0), dead


def attend(q, k, v, scale, add):
    p, _ = weights(q, k, scale, add)
    return np.matmul(p, v)


def additive(mask3, group: int, bh: int, sq: int, sk: int, causal: bool, shift: int = 0) -> np.ndarray:
    """The whole additive term [BH, Sq, Sk]: mask row h // group (mask3 [G, Sq, Sk] or None) plus the bottom-right aligned
    causal limit key <= i + Sk - Sq + shift as -inf."""
    add = np.zeros((bh, sq, sk))
    if mask3 is not None:
        add = add + mask3[np.arange(bh) // group]
    if causal:
        add = np.where(np.tril(np.ones((sq, sk), dtype=bool), k=sk - sq + shift), add, -np.inf)
    return add


def oracle_prefill(q, k, v, scale, mask, group, causal):
    """oracle/ref_ops.py::attention on [1, BH, ...] with the mask expanded per head; NaN rows stay NaN."""
    bh = q.shape[0]
    m4 = None
    if mask is not None:
        m = mask[:, None, :] if mask.ndim == 2 else mask
        m4 = m[np.arange(bh) // group][None]
    with np.errstate(invalid="ignore"):
        return R.attention(q[None], k[None], v[None], scale, m4, causal)[0]


# ------------------------------------------------------------------------------------------------------------------------
# prefill builder
# ------------------------------------------------------------------------------------------------------------------------
def _pm1(rng, shape):
    return rng.integers(0, 2, shape).astype(np.float64) * 2.0 - 1.0


def _orthogonalise(ka, kb, rng):
    """Flip entries of the +-1 row kb (in place) until ka . kb == 0."""
    d = ka.size
    agree = np.flatnonzero(ka == kb)
    differ = np.flatnonzero(ka != kb)
    excess = agree.size - d // 2
    flip = rng.choice(agree, excess, replace=False) if excess > 0 else rng.choice(differ, -excess, replace=False)
    kb[flip] *= -1.0
    assert ka @ kb == 0


def special_keys(sk: int) -> list[int]:
    """0, 63, 64, Sk - 1 and the first and last key of the last (ragged) tile, those that exist."""
    first_of_last = (sk - 1) // KT * KT
    return sorted({x for x in (0, KT - 1, KT, first_of_last, sk - 1) if 0 <= x < sk})


@functools.lru_cache(maxsize=8)
def prefill_case(dt: str, d: int, sq: int, sk: int, causal: bool, mask_form: int, heads: int, scale_kind: str = "imm",
                 seed: int = 0):
    """One selector case for ops.attention. mask_form: 0 none, 1 per key [G, Sk], 2 full [G, Sq, Sk] (G = 2 rows for
    `heads` heads). scale_kind: "imm" (a float), "div" (sqrt(D) in device memory, used as a divisor), "neg" (a negative
    scale, Q negated so that the targets keep winning). The result is shared and must not be modified."""
    rng = np.random.default_rng([seed, d, sq, sk, int(causal), mask_form, heads])
    bh, G = heads, (2 if mask_form else 1)
    assert bh % G == 0
    group = bh // G
    off = sk - sq
    lim = np.minimum(np.arange(sq) + off, sk - 1) if causal else np.full(sq, sk - 1)
    ntiles = (sk + KT - 1) // KT
    specials = special_keys(sk)
    k = _pm1(rng, (bh, sk, d))
    gi_of = lambda h: h // group  # noqa: E731

    kind = np.full((bh, sq), "", dtype=object)
    t_of = np.full((bh, sq), -1)
    x_of = np.full((bh, sq), -1)
    m3 = np.zeros((G, sq, sk)) if mask_form else None
    m2 = np.zeros((G, sk)) if mask_form == 1 else None
    taken_g = [set() for _ in range(G)]  # mask_form 2: rows of a mask row group whose mask row is spoken for
    count = [0]

    def next_neg():  # -inf and -10000 in turn
        count[0] += 1
        return NEG[count[0] % 2]

    def find_row(h, need, start):
        for j in range(sq):
            i = (start + j) % sq
            if lim[i] >= need and kind[h, i] == "" and (mask_form != 2 or i not in taken_g[gi_of(h)]):
                return i
        return None

    # ---- per-key mask: hidden keys and the biased key of every mask row (before the ties, which must avoid them) ----
    hidden = [dict() for _ in range(G)]
    ykey = [-1] * G
    if mask_form == 1:
        for n_, x in enumerate(specials):
            hidden[n_ % G][x] = -np.inf if x == 0 else next_neg()  # (key 0 at -inf: causal row 0 is then fully masked)
        plain = [x for x in range(sk) if x not in specials]
        extra = rng.choice(plain, min(len(plain), 3 * G), replace=False)
        for gi in range(G):
            for x in extra[2 * gi:2 * gi + 2]:
                hidden[gi][int(x)] = next_neg()
            ykey[gi] = int(extra[2 * G + gi]) if len(extra) >= 3 * G else -1
            for x, val in hidden[gi].items():
                m2[gi, x] = val
            if ykey[gi] >= 0:
                m2[gi, ykey[gi]] = BIAS
        m3[:] = m2[:, None, :]
    reserved = set().union(*[set(hd) for hd in hidden]) | set(ykey)

    # ---- ties: pairs (a, b) in different tiles with k_a . k_b == 0; pair 0 of the even heads uses a = Sk - 1 ----
    ties = []
    for h in range(bh):
        gi = gi_of(h)
        free = [x for x in range(sk - 1) if x not in reserved and x not in specials]
        rng.shuffle(free)
        pairs, used = [], set()

        def pick(tile_not, beyond_first=False):
            for x in free:
                if x not in used and (ntiles == 1 or x // KT != tile_not) and not (beyond_first and x < KT):
                    used.add(x)
                    return x
            return None

        if h % 2 == 0 and (sk - 1) not in hidden[gi]:
            b = pick((sk - 1) // KT)
            if b is not None:
                pairs.append((sk - 1, b, sq - 1))
        for n_ in range(2):
            a = pick(-1, beyond_first=(n_ == 0 and ntiles >= 3))
            b = None if a is None else pick(a // KT, beyond_first=(n_ == 0 and ntiles >= 3))
            if a is not None and b is not None:
                pairs.append((a, b, None))
        for a, b, row in pairs:
            i = row if row is not None else find_row(h, max(a, b), (41 * (h + 1) + 67 * len(ties)) % sq)
            if i is None or kind[h, i] != "" or lim[i] < max(a, b):
                continue
            _orthogonalise(k[h, a], k[h, b], rng)
            kind[h, i], t_of[h, i], x_of[h, i] = "tie", a, b
            ties.append((h, i, a, b))
            if mask_form == 2:
                taken_g[gi].add(i)
    for h in range(bh):
        assert len({r.tobytes() for r in k[h]}) == sk, "K rows must be distinct"

    # ---- masked decoys, bias rows, fully masked rows ----
    if mask_form == 1:
        for gi in range(G):
            hs = [h for h in range(bh) if gi_of(h) == gi]
            for n_, (x, _) in enumerate(sorted(hidden[gi].items())):
                for rep in range(2):
                    h = hs[(n_ + rep) % len(hs)]
                    i = find_row(h, max(x, 1), (29 * n_ + 53 * rep + 11 * h) % sq)
                    if i is not None:
                        kind[h, i], x_of[h, i] = "mdecoy", x
            for h in hs:
                for rep in range(3):
                    i = find_row(h, max(ykey[gi], 1), (17 + 61 * rep + 7 * h) % sq) if ykey[gi] >= 0 else None
                    if i is not None:
                        kind[h, i], x_of[h, i] = "bias", ykey[gi]
    elif mask_form == 2:
        def claim(gi, i, k_):
            taken_g[gi].add(i)
            for h in range(bh):
                if gi_of(h) == gi:
                    kind[h, i] = k_

        for i in (5, sq - 3):  # every key at -inf: one early row, one in the partial last workgroup
            if 0 <= i < sq and i not in taken_g[0]:
                m3[0, i, :] = -np.inf
                claim(0, i, "dead")
        h_of_g = [gi * group for gi in range(G)]
        todo = [(x, n_ % G) for n_, x in enumerate(specials)] + [(x, (n_ + 1) % G) for n_, x in enumerate(specials)]
        for n_, (x, gi) in enumerate(todo):
            i = find_row(h_of_g[gi], max(x, 1), (37 * n_ + 3) % sq)
            if i is not None:
                m3[gi, i, x] = next_neg()
                claim(gi, i, "mdecoy")
                x_of[[h for h in range(bh) if gi_of(h) == gi], i] = x
        for gi in range(G):
            for i in range(sq):
                if i in taken_g[gi] or lim[i] < 1 or kind[h_of_g[gi], i] != "":
                    continue
                if causal and lim[i] + 1 in specials:
                    continue  # (kept for the causal decoy of that special key)
                if i % 4 == 1 or i % 9 == 4:
                    x = int(rng.integers(0, lim[i] + 1))
                    m3[gi, i, x] = next_neg() if i % 4 == 1 else BIAS
                    claim(gi, i, "mdecoy" if i % 4 == 1 else "bias")
                    x_of[[h for h in range(bh) if gi_of(h) == gi], i] = x

    # ---- causal decoys: t = lim, x = lim + 1 (hidden by the causal limit alone) ----
    if causal:
        for h in range(bh):
            for i in range(sq):
                x = lim[i] + 1
                if kind[h, i] != "" or lim[i] < 0 or x >= sk or not (x in specials or (i + h) % 5 == 0):
                    continue
                if mask_form and (m3[gi_of(h), i, lim[i]] != 0 or m3[gi_of(h), i, x] != 0):
                    continue
                kind[h, i], t_of[h, i], x_of[h, i] = "cdecoy", lim[i], x

    # ---- targets: the scarcest rows first, each takes the largest key nobody has won yet ----
    def visible(h, i):
        ok = np.zeros(sk, dtype=bool)
        ok[:max(lim[i] + 1, 0)] = True
        if mask_form:
            ok &= m3[gi_of(h), i] == 0
        if x_of[h, i] >= 0:
            ok[x_of[h, i]] = False
        return ok

    won = set(int(t) for t in t_of[kind == "cdecoy"])
    won |= set(int(x) for x in x_of[kind == "bias"])
    order = sorted(((lim[i], h, i) for h in range(bh) for i in range(sq) if kind[h, i] in ("", "mdecoy", "bias")))
    for _, h, i in order:
        ok = visible(h, i)
        cand = np.flatnonzero(ok)
        if cand.size == 0:
            live = lim[i] >= 0 and kind[h, i] == "bias"
            kind[h, i], t_of[h, i] = ("target", x_of[h, i]) if live else ("dead", 0)
            if kind[h, i] == "dead" and x_of[h, i] >= 0:
                t_of[h, i] = x_of[h, i]  # (the query of a dead row asks for a key it may not have)
            x_of[h, i] = -1 if live else x_of[h, i]
            continue
        fresh = [c for c in cand[::-1] if int(c) not in won]
        t = int(fresh[0]) if fresh else int(rng.choice(cand))
        t_of[h, i] = t
        if kind[h, i] == "":
            kind[h, i] = "target"
        if kind[h, i] != "bias":
            won.add(t)
    for h, i in zip(*np.nonzero(kind == "dead")):
        t_of[h, i] = max(t_of[h, i], 0)

    # ---- queries ----
    hh = np.arange(bh)[:, None]
    kt = k[hh, np.maximum(t_of, 0)]
    kx = k[hh, np.maximum(x_of, 0)]
    coef = np.select([kind == "tie", kind == "bias", (kind == "mdecoy") | (kind == "cdecoy")], [1.0, 1.0, 2.0], 0.0)
    coef = np.where((kind == "dead"), 0.0, coef)
    q_unit = kt + coef[..., None] * kx
    rt_d = float(R.round_to(np.array([np.sqrt(d)]), dt)[0])
    scale = {"imm": 1.0 / np.sqrt(d), "div": 1.0 / rt_d, "neg": -1.0 / np.sqrt(d)}[scale_kind]
    if scale_kind == "neg":
        q_unit = -q_unit
    mask = None if not mask_form else R.round_to(m2 if mask_form == 1 else m3, dt)
    mask3 = None if mask is None else (np.broadcast_to(mask[:, None, :], (G, sq, sk)) if mask_form == 1 else mask)
    add = additive(mask3, group, bh, sq, sk, causal)
    winner = np.where(np.isin(kind, ("target", "mdecoy", "cdecoy")), t_of, np.where(kind == "bias", x_of, -1))
    single = kind == "target"
    for g in (1, 2, 4, 8, 16, 32, 64):
        p, dead = weights(g * q_unit, k, scale, add)
        pw = np.take_along_axis(p, np.maximum(winner, 0)[..., None], -1)[..., 0]
        if (pw[single] >= P_STAR).all():
            break
    else:
        raise ValueError(f"no g <= 64 gives every target row the weight 1 - 2^-12 (worst {pw[single].min()})")
    q = g * q_unit
    assert np.array_equal(R.round_to(q, dt), q) and np.abs(q).max() <= 3 * 64
    assert np.array_equal(dead, kind == "dead"), "the plan's fully masked rows are the reference's"
    v = R.round_to(rng.standard_normal((bh, sk, d)), dt)
    want = oracle_prefill(q, k, v, scale, mask, group, causal)
    assert np.array_equal(np.isnan(want).any(-1), dead) and np.array_equal(np.isnan(want).all(-1), dead)
    want = np.where(dead[..., None], 0.0, want)  # attention.hip: fully masked rows produce 0
    absum = np.matmul(p, np.abs(v))
    assert np.abs(want - np.matmul(p, v)).max() <= 1e-9

    # ---- what the case promises ----
    live_winner = set(int(w) for w in winner[winner >= 0])
    assert live_winner == set(range(sk)), f"keys never the single winner of a row: {sorted(set(range(sk)) - live_winner)}"
    decoy_x = set(int(x) for x in x_of[np.isin(kind, ("mdecoy", "cdecoy")) & ~dead])
    allowed = set()
    if mask_form:
        allowed |= set(specials)
    if causal:
        allowed |= {x for x in specials if x >= 1 and 0 <= x - 1 - off < sq}
    assert allowed <= decoy_x, f"special keys never a forbidden decoy: {sorted(allowed - decoy_x)}"
    assert set(np.arange(sq) % WG_ROWS) == set(range(min(sq, WG_ROWS))), "every row position of a workgroup"
    assert sq % WG_ROWS != 0, "a partial last workgroup"
    if ntiles > 1:
        assert all(a // KT != b // KT for _, _, a, b in ties)
    assert all(k[h, a] @ k[h, b] == 0 for h, _, a, b in ties)
    return SimpleNamespace(dt=dt, d=d, sq=sq, sk=sk, causal=causal, mask_form=mask_form, bh=bh, group=group, G=G, g=g,
                           scale=scale, scale_kind=scale_kind, scale_div=rt_d, q=q, k=k, v=v, mask=mask, mask3=mask3,
                           want=want, absum=absum,
                           bound=bound_for(dt, want, absum, p_sub=f16_subnormal_weights(p, np.abs(v))), dead=dead, kind=kind, t=t_of,
                           x=x_of, winner=winner, ties=ties, lim=lim, p=p, specials=specials)


# (Sq, Sk, causal): two workgroups + a ragged tile of 8 keys with Sk % 4 == 0 (vector mask loads); both ends ragged with
# Sk % 4 != 0 (element mask loads); causal with Sk > Sq (tile skipping); causal with Sk < Sq: rows 0..63 fully masked and key 0
# the diagonal of row 64; the whole first workgroup fully masked.
PREFILL_SHAPES = [(200, 200, False), (150, 77, False), (200, 200, True), (150, 77, True), (40, 200, True), (200, 136, True),
                  (200, 40, True)]


def prefill_heads(sq: int, sk: int, mask_form: int) -> int:
    """B = 1; two heads, four where two mask rows must each serve two heads, and as many as it takes for every key to be
    the winner of some row where the queries are few."""
    return (8 if sq < sk else 4) if mask_form else (6 if sq < sk else 2)


def prefill_params():
    """(dt, D, Sq, Sk, causal, mask_form, heads, scale_kind): every one of the 24 kernel builds at every shape of its causal
    setting, plus a device-memory divisor scale and a negative scale."""
    out = []
    for d in (64, 128):
        for dt in ("f16", "bf16"):
            for mask_form in (0, 1, 2):
                for sq, sk, causal in PREFILL_SHAPES:
                    out.append((dt, d, sq, sk, causal, mask_form, prefill_heads(sq, sk, mask_form), "imm"))
    out.append(("f16", 128, 200, 200, False, 1, 4, "div"))
    out.append(("bf16", 128, 150, 77, True, 2, 4, "div"))
    out.append(("bf16", 64, 200, 200, True, 1, 4, "neg"))
    out.append(("f16", 64, 150, 77, False, 2, 4, "neg"))
    return out


def prefill_id(p) -> str:
    dt, d, sq, sk, causal, mask_form, heads, sc = p
    return f"{dt}-d{d}-{sq}x{sk}-{'causal' if causal else 'full'}-mask{mask_form}-h{heads}-{sc}"


def random_reference(dt, q, k, v, scale, mask4, causal):
    """want, bound for arbitrary rounded inputs [B, H, S, D] (mask4 broadcastable to [B, H, Sq, Sk] or None): the oracle
    for the value, the fp64 weights for A."""
    want = R.attention(q, k, v, scale, mask4, causal)
    b, h, sq, _ = q.shape
    sk = k.shape[2]
    add = np.zeros((b, h, sq, sk)) if mask4 is None else np.broadcast_to(np.asarray(mask4, dtype=np.float64), (b, h, sq, sk))
    if causal:
        add = np.where(np.tril(np.ones((sq, sk), dtype=bool), k=sk - sq), add, -np.inf)
    p, dead = weights(q, k, scale, add)
    assert not dead.any()
    return want, bound_for(dt, want, np.matmul(p, np.abs(v)), p_sub=f16_subnormal_weights(p, np.abs(v)))


# ------------------------------------------------------------------------------------------------------------------------
# decode builder
# ------------------------------------------------------------------------------------------------------------------------
DECODE_HEADS = 16
DECODE_POSITIONS = [(0, 64), (63, 64), (64, 80), (700, 1024), (1022, 1024)]
DECODE_SPLITS = [0, 1, 2, 5, 16]


def decode_chunk_len(n: int, split: int, keys_per_iteration: int):
    """Chunk length of the split decode kernel for n keys cut G ways (csrc/attention_kvcache.hip: rounded up to the keys a
    workgroup takes per iteration); None for the one-workgroup kernels (split 0 and 1: one chunk)."""
    if split <= 1:
        return None
    return ((n + split - 1) // split + keys_per_iteration - 1) // keys_per_iteration * keys_per_iteration


def decode_chunks(n: int, chunk_len) -> list[tuple[int, int]]:
    if chunk_len is None or chunk_len >= n:
        return [(0, n)]
    return [(c0, min(n, c0 + chunk_len)) for c0 in range(0, n, chunk_len)]


def decode_targets(pos: int, chunk_len) -> list[int]:
    """Key 0, the new key, the one before it, the first and last key of every chunk; each once."""
    out = [0, pos, pos - 1]
    for c0, c1 in decode_chunks(pos + 1, chunk_len):
        out += [c0, c1 - 1]
    return list(dict.fromkeys(x for x in out if 0 <= x <= pos))


@functools.lru_cache(maxsize=2)
def _decode_base(dt: str, d: int, pos: int, max_seq: int):
    rng = np.random.default_rng([7, d, pos, max_seq, sorted(U).index(dt)])
    kc = _pm1(rng, (DECODE_HEADS, max_seq, d)).astype(np.float32)
    kn = _pm1(rng, (DECODE_HEADS, 1, d)).astype(np.float32)
    vc = R.round_to(rng.standard_normal((DECODE_HEADS, max_seq, d)), dt).astype(np.float32)
    vn = R.round_to(rng.standard_normal((DECODE_HEADS, 1, d)), dt).astype(np.float32)
    for h in range(DECODE_HEADS):
        rows = {r.tobytes() for r in kc[h, :pos]} | {kn[h, 0].tobytes()}
        assert len(rows) == pos + 1, "K rows must be distinct"
    for a in (kc, kn, vc, vn):
        a.setflags(write=False)
    return kc, kn, vc, vn


@functools.lru_cache(maxsize=4)
def decode_case(dt: str, d: int, pos: int, max_seq: int, chunk_len=None):
    """Selector calls for one decode step: a list of rounds, each one call of ops.attention_kvcache with B x H = 16 heads and
    16 targets of decode_targets(pos, chunk_len) (the last round is filled up with other keys). Head h asks for its target
    t(h): q = g k_t. The cache rows the step must not read — the stale row at `pos`, which the append overwrites, and every
    row in (pos, max_seq) — hold 2 k_t (twice the target's score if read) with V = 1000. Shared; not to be modified."""
    kc0, kn, vc0, vn = _decode_base(dt, d, pos, max_seq)
    n = pos + 1
    targets = decode_targets(pos, chunk_len)
    rng = np.random.default_rng([11, d, pos, max_seq])
    rounds = []
    for r0 in range(0, len(targets), DECODE_HEADS):
        ts = targets[r0:r0 + DECODE_HEADS]
        ts = ts + [int(x) for x in rng.integers(0, n, DECODE_HEADS - len(ts))]
        t = np.array(ts)
        hh = np.arange(DECODE_HEADS)
        k_t = np.where((t == pos)[:, None], kn[:, 0], kc0[hh, np.minimum(t, max_seq - 1)]).astype(np.float64)
        kc, vc = kc0.copy(), vc0.copy()
        kc[:, pos:] = 2.0 * k_t[:, None, :]
        vc[:, pos:] = DECOY_V
        valid_k = np.concatenate([kc[:, :pos].astype(np.float64), kn.astype(np.float64)], axis=1)  # [16, n, d]
        valid_v = np.concatenate([vc[:, :pos].astype(np.float64), vn.astype(np.float64)], axis=1)
        for g in (1, 2, 4, 8, 16, 32, 64):
            q = g * k_t[:, None, :]
            p, _ = weights(q, valid_k, 1.0 / np.sqrt(d), 0.0)
            if (p[hh, 0, t] >= P_STAR).all():
                break
        else:
            raise ValueError(f"no g <= 64 gives every decode target the weight 1 - 2^-12 (worst {p[hh, 0, t].min()})")
        want = R.attention_kvcache(kc[None], vc[None], q[None], kn[None], vn[None], pos)[0][0]
        absum = np.matmul(p, np.abs(valid_v))
        assert np.abs(want - np.matmul(p, valid_v)).max() <= 1e-9
        rounds.append(SimpleNamespace(dt=dt, d=d, pos=pos, max_seq=max_seq, g=g, t=t, q=q.astype(np.float32), kc=kc, vc=vc,
                                      kn=kn, vn=vn, valid_k=valid_k, valid_v=valid_v, want=want, absum=absum, p=p,
                                      bound=bound_for(dt, want, absum, decode=True), chunks=decode_chunks(n, chunk_len)))
    covered = set(int(x) for r in rounds for x in r.t)
    assert set(targets) <= covered and {0, pos} <= covered
    for c0, c1 in decode_chunks(n, chunk_len):
        assert c0 in covered and c1 - 1 in covered, "first and last key of every chunk"
    return rounds
