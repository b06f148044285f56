"""The "bf16x3" / "bf16x6" compute types of an fp32 MatMul on a real MI355X: the split kernel alone (bit-exact against an emulation in
integer arithmetic), the GEMM on selector inputs whose result is exact (a wrong plane offset or a broken pairing of the two plane
tables shows at any K position), random data against the emulated split product and the bounds include/infini_rocm.h promises, and
both modes through the reference's MatMul operator."""
import itertools

import numpy as np
import pytest
import torch

from infinitensor_amd import ops

pytestmark = pytest.mark.gpu

# plane tables of csrc/gemm_route.h (kSplitPieceA / kSplitPieceB): term t multiplies piece A[t] of A with piece B[t] of B
TABLES = {"bf16x3": ((1, 0, 0), (0, 1, 0)), "bf16x6": ((1, 2, 0, 1, 0, 0), (1, 0, 2, 0, 1, 0))}


@pytest.fixture(scope="module")
def B(plugin_backend):
    return plugin_backend


@pytest.fixture(scope="module")
def rocm(B):
    return B.RocmRuntime(0)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.float().cpu().numpy().astype(np.float64)


# ---- the split in numpy ----------------------------------------------------------------------------------------------------------
def rne_bf16(x):
    """fp32 -> the nearest bf16 (ties to even), returned as fp32. NaN stays NaN (quiet bit set)."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) & 0xFFFF
    r = np.where(np.isnan(x), (u >> 16) | 0x40, r)
    return (r.astype(np.uint32) << 16).view(np.float32).reshape(np.shape(x))


def pieces(x):
    """p0 = rne(x), p1 = rne(x - p0), p2 = rne((x - p0) - p1) in fp32 arithmetic; a p0 that is not finite zeroes the lower pieces"""
    x = np.asarray(x, dtype=np.float32)
    p0 = rne_bf16(x)
    with np.errstate(invalid="ignore", over="ignore"):
        r1 = np.where(np.isfinite(p0), x - p0, np.float32(0)).astype(np.float32)
    p1 = rne_bf16(r1)
    r2 = (r1 - p1).astype(np.float32)
    return p0, p1, rne_bf16(r2)


def split_product(a, b, mode):
    """sum over the mode's terms of A_piece B_piece, in fp64"""
    pa, pb = [p.astype(np.float64) for p in pieces(a)], [p.astype(np.float64) for p in pieces(b)]
    ta, tb = TABLES[mode]
    return sum(pa[i] @ pb[j] for i, j in zip(ta, tb))


def test_the_emulation_and_the_tables():
    """(no kernel) the tables pair up to every product with i + j <= 1 (x3, minus lo * lo) / i + j <= 2 (x6), once each; the three
    pieces of a normal fp32 value add up to it exactly."""
    assert sorted(zip(*TABLES["bf16x3"])) == [(0, 0), (0, 1), (1, 0)]
    assert sorted(zip(*TABLES["bf16x6"])) == sorted((i, j) for i in range(3) for j in range(3) if i + j <= 2)
    x = np.random.default_rng(0).standard_normal(4096).astype(np.float32)
    p0, p1, p2 = (p.astype(np.float64) for p in pieces(x))
    assert np.array_equal(p0 + p1 + p2, x.astype(np.float64))
    assert np.all(np.abs(x - p0) <= 2.0 ** -8 * np.abs(x)) and np.all(np.abs(x - p0 - p1) <= 2.0 ** -16 * np.abs(x))
    assert rne_bf16(np.float32(1 + 2.0 ** -8)) == 1.0 and rne_bf16(np.float32(1 + 3 * 2.0 ** -8)) == np.float32(1 + 2.0 ** -6)  # ties to even


# ---- 1. the split kernel alone ---------------------------------------------------------------------------------------------------
SPECIALS = [0.0, -0.0, np.inf, -np.inf, np.nan, np.finfo(np.float32).max, -np.finfo(np.float32).max, 1 + 2.0 ** -9, 1 + 2.0 ** -17,
            -(1 + 2.0 ** -9), 1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 3.4e38, 1e-30, 65535.0, 1 - 2.0 ** -24]


def bits(t):
    return t.contiguous().view(torch.int16)


@pytest.mark.parametrize("lead", [(), (2,)], ids=["one_block", "two_blocks"])
@pytest.mark.parametrize("k_is_cols", [1, 0])
@pytest.mark.parametrize("side", [0, 1], ids=["A_tables", "B_tables"])
def test_split_kernel_is_bit_exact(rt, lead, k_is_cols, side):
    rng = np.random.default_rng(11 + k_is_cols)
    x = (rng.standard_normal(lead + (72, 128)) * np.exp2(rng.integers(-20, 20, lead + (72, 128)))).astype(np.float32)
    x[..., 5, : len(SPECIALS)] = np.array(SPECIALS, dtype=np.float32)
    x[..., 71, 128 - len(SPECIALS):] = np.array(SPECIALS, dtype=np.float32)
    p = pieces(x)
    # Inf -> (Inf, 0, 0), also for a finite value that rounds up to bf16's Inf (the largest fp32, 3.4e38)
    for col in (2, 3, 5, 6, 12):
        assert np.isinf(p[0][..., 5, col]).all() and (p[1][..., 5, col] == 0).all() and (p[2][..., 5, col] == 0).all()
    dx = dev(x)
    for mode in ("bf16x3", "bf16x6"):
        table = TABLES[mode][side]
        got = ops.split_bf16(rt, dx, bool(k_is_cols), table)
        rt.sync()
        want = torch.from_numpy(np.concatenate([p[i] for i in table], axis=-1 if k_is_cols else -2)).to(torch.bfloat16)  # exact: bf16 values
        assert got.dtype == torch.bfloat16 and got.shape == want.shape
        got = got.cpu()
        nan = torch.isnan(want)
        assert torch.equal(torch.isnan(got), nan)
        assert int(nan.sum()) == 2 * table.count(0) * (2 if lead else 1)  # two NaNs per block: NaN in the p0 planes, 0 in the others
        assert torch.equal(bits(torch.where(nan, torch.zeros_like(got), got)), bits(torch.where(nan, torch.zeros_like(want), want)))


def test_split_kernel_rejects_what_it_cannot_do(rt):
    x = torch.zeros(16, 64, device="cuda")
    for bad in ([0, 1, 3], [0] * 7, [-1]):
        with pytest.raises(RuntimeError):
            ops.split_bf16(rt, x, True, bad)
    with pytest.raises(RuntimeError):
        ops.split_bf16(rt, torch.zeros(16, 60, device="cuda"), True, [0, 1])  # cols % 8
    with pytest.raises(RuntimeError):
        ops.split_bf16(rt, torch.zeros(16 * 64 + 4, device="cuda")[1:1 + 16 * 64].view(16, 64), True, [0, 1])  # 4 bytes off
    assert ops.split_bf16(rt, x[:0], True, [0, 1]).shape == (0, 128)


# ---- 2. selector inputs: an exact GEMM -------------------------------------------------------------------------------------------
def mm(rt, a, b, ta, tb):
    """C = A B for logical A [m, k], B [k, n], stored transposed where asked"""
    da = dev(a.T if ta else a)
    db = dev(b.T if tb else b)
    return ops.matmul(rt, da, db, None, ta, tb)


def with_compute_type(rt, ct, fn):
    try:
        ops.set_matmul_compute_type(rt, ct)
        out = fn()
        rt.sync()
        return out
    finally:
        ops.set_matmul_compute_type(rt, "default")


LAYOUTS = list(itertools.product([False, True], repeat=2))


@pytest.mark.parametrize("ta,tb", LAYOUTS, ids=["nn", "nt", "tn", "tt"])
def test_integer_selectors_are_exact_under_the_split(rt, ta, tb):
    """16-bit integers need exactly hi + lo, {-1, 0, 1} is one piece: lo * lo is identically 0 and every partial sum is an integer
    below 128 * 65535 < 2^23, so the result IS the integer product under x3 (and x6) in any order of summation — and visibly not
    under plain "bf16". (a) the integers in A, (b) in B: the two cross terms."""
    m, n, k = 64, 72, 128
    rng = np.random.default_rng(23)
    ints_a = rng.integers(0, 65536, (m, k)).astype(np.float32)
    ints_b = rng.integers(0, 65536, (k, n)).astype(np.float32)
    sel_b = rng.integers(-1, 2, (k, n)).astype(np.float32)
    sel_a = rng.integers(-1, 2, (m, k)).astype(np.float32)
    for ints in (ints_a, ints_b):  # the premise, checked: hi + lo is the integer, and lo is needed
        p0, p1, p2 = pieces(ints)
        assert np.array_equal(p0.astype(np.float64) + p1, ints.astype(np.float64))
        assert (p2 == 0).all() and (p1 != 0).mean() > 0.9
    for a, b in ((ints_a, sel_b), (sel_a, ints_b)):
        want = a.astype(np.int64) @ b.astype(np.int64)
        assert (np.abs(a.astype(np.int64)) @ np.abs(b.astype(np.int64))).max() < 2 ** 23
        for ct in ("bf16x3", "bf16x6"):
            got = with_compute_type(rt, ct, lambda: mm(rt, a, b, ta, tb))
            assert ops.matmul_last_variant(rt) == "tile256_splitk"
            assert np.array_equal(host(got), want.astype(np.float64)), (ct, np.abs(host(got) - want).max())
        rough = with_compute_type(rt, "bf16", lambda: mm(rt, a, b, ta, tb))
        assert np.abs(host(rough) - want).max() > 100  # one rounding of a 16-bit integer is off by up to 128


def exact_in_any_order(x):
    """True where the three pieces of x add up to x in fp32 in every order (what a different plane order, K-tile order or split-K
    slicing could do to the sum of the three products of one selected element)"""
    p = pieces(x)
    ok = np.ones(x.shape, dtype=bool)
    for i, j, l in itertools.permutations(range(3)):
        s = ((p[i] + p[j]).astype(np.float32) + p[l]).astype(np.float32)
        ok &= s.view(np.uint32) == x.view(np.uint32)
    return ok


def full_mantissa_values(rng, shape):
    x = (rng.standard_normal(shape) * np.exp2(rng.integers(-8, 8, shape))).astype(np.float32)
    for _ in range(64):
        bad = ~exact_in_any_order(x)
        if not bad.any():
            break
        x[bad] = rng.standard_normal(int(bad.sum())).astype(np.float32)
    assert exact_in_any_order(x).all()
    assert (pieces(x)[2] != 0).mean() > 0.9  # the third piece is needed
    return x


@pytest.mark.parametrize("k", [128, 1024], ids=["k128_one_slice", "k1024_twelve_slices"])
@pytest.mark.parametrize("ta,tb", LAYOUTS, ids=["nn", "nt", "tn", "tt"])
def test_one_hot_selectors_return_fp32_values_bit_for_bit_under_x6(rt, ta, tb, k):
    """(c) B has one +-1 per column at a chosen k: under x6 every output is the selected element of A, all 24 bits of it (the three
    products p2, p1, p0 of that element sit at K' = k + K, k + 3 K, k + 5 K); then the roles swapped. K = 1024 is cut into twelve
    K slices of 512, so the chosen k fall into different slices as well. Under x3 the same outputs carry 16 bits."""
    m, n = 64, 72
    rng = np.random.default_rng(31 + k)
    edges = [0, 63, 64, k - 1, 31, 32, k // 2 - 1, k // 2] + ([511, 512, 513, 1000] if k > 512 else [])
    for roles in ("select_from_a", "select_from_b"):
        cnt = n if roles == "select_from_a" else m
        ks = np.array(edges + list(rng.integers(0, k, cnt - len(edges))))
        sign = np.where(rng.integers(0, 2, cnt) == 1, 1.0, -1.0).astype(np.float32)
        if roles == "select_from_a":
            a = full_mantissa_values(rng, (m, k))
            b = np.zeros((k, n), dtype=np.float32)
            b[ks, np.arange(n)] = sign
            want = a[:, ks] * sign[None, :]
        else:
            b = full_mantissa_values(rng, (k, n))
            a = np.zeros((m, k), dtype=np.float32)
            a[np.arange(m), ks] = sign
            want = b[ks, :] * sign[:, None]
        got = with_compute_type(rt, "bf16x6", lambda: mm(rt, a, b, ta, tb))
        assert ops.matmul_last_variant(rt) == "tile256_splitk"
        assert np.array_equal(got.cpu().numpy().view(np.uint32), want.astype(np.float32).view(np.uint32)), roles
        got3 = with_compute_type(rt, "bf16x3", lambda: mm(rt, a, b, ta, tb))
        err3 = np.abs(host(got3) - want)
        assert (err3 <= 2.0 ** -16 * np.abs(want)).all() and err3.max() > 0, roles


# ---- 3. random data against the emulation ----------------------------------------------------------------------------------------
RANDOM = [(1, 512, 768, 256, False, False), (1, 300, 520, 1024, True, True), (3, 256, 512, 512, False, False)]


@pytest.mark.parametrize("shape", RANDOM, ids=["512x768x256", "300x520x1024_bias_relu", "3x256x512x512_shared_b"])
def test_random_data_against_the_emulated_split(rt, shape):
    """x3 against the emulated three-term product in fp64, x6 against the exact fp64 product, both within what the exact fp32 kernel
    is allowed against its oracle (rtol 1e-4, atol 2e-5: only fp32 summation separates them); x3 additionally inside the header's
    bound 3 * 2^-16 (|A| |B|) per element and at least 32 x closer than "bf16" (the emulation gives ~500 x)."""
    bt, m, n, k, use_bias, relu = shape
    rng = np.random.default_rng(m + n + k)
    a = rng.standard_normal((bt, m, k) if bt > 1 else (m, k)).astype(np.float32)
    b = (rng.standard_normal((k, n)) / np.sqrt(k)).astype(np.float32)
    bias = rng.standard_normal((n,)).astype(np.float32) if use_bias else None
    da, db, dbias = dev(a), dev(b), (dev(bias) if use_bias else None)
    act = 1 if relu else 0

    def fin(v):
        v = v + bias.astype(np.float64) if use_bias else v
        return np.maximum(v, 0) if relu else v

    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    exact = fin(a64 @ b64)
    bound = 3 * 2.0 ** -16 * (np.abs(a64) @ np.abs(b64))
    allow = 1e-4 * np.abs(exact) + 2e-5

    got = {}
    for ct in ("bf16x3", "bf16x6", "bf16"):
        got[ct] = host(with_compute_type(rt, ct, lambda: ops.matmul(rt, da, db, dbias, act=act)))
        assert ops.matmul_last_variant(rt) == "tile256_splitk", ct
    want3 = fin(split_product(a, b, "bf16x3"))
    err = {ct: np.abs(v - exact) for ct, v in got.items()}
    print({ct: float(e.max()) for ct, e in err.items()}, "x3 vs emulation", float(np.abs(got["bf16x3"] - want3).max()),
          "x3 error / bound", float((err["bf16x3"] / bound).max()))
    assert np.allclose(got["bf16x3"], want3, rtol=1e-4, atol=2e-5), np.abs(got["bf16x3"] - want3).max()
    assert np.allclose(got["bf16x6"], exact, rtol=1e-4, atol=2e-5), err["bf16x6"].max()
    assert (err["bf16x3"] <= bound + allow).all()
    assert err["bf16x3"].max() * 32 <= err["bf16"].max(), (err["bf16x3"].max(), err["bf16"].max())

    # K - 8 is no multiple of 64: the exact kernel, under both modes
    a_odd, b_odd = np.ascontiguousarray(a[..., : k - 8]), np.ascontiguousarray(b[: k - 8])
    for ct in ("bf16x3", "bf16x6"):
        y_odd = host(with_compute_type(rt, ct, lambda: ops.matmul(rt, dev(a_odd), dev(b_odd), dbias, act=act)))
        assert ops.matmul_last_variant(rt) == "fast32", ct
        assert np.allclose(y_odd, fin(a_odd.astype(np.float64) @ b_odd.astype(np.float64)), rtol=1e-4, atol=2e-5)
    # and "default" is the exact kernel again
    y = host(ops.matmul(rt, da, db, dbias, act=act))
    assert ops.matmul_last_variant(rt) == "fast32"
    assert np.allclose(y, exact, rtol=1e-4, atol=2e-5)


# ---- 4. through the reference operator -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ct", ["bf16x3", "bf16x6"])
def test_split_compute_types_through_the_reference_operator(B, rocm, ct):
    """MatmulObj::computeType is a free string from OnnxStub(matmul_compute_type=...) down to the kernel: the plugin maps the two new
    ones (shapes and data of test_gpu_plugin.py::test_matmul_compute_type_through_the_reference_operator)."""
    rng = np.random.default_rng(71)
    a = rng.standard_normal((256, 512)).astype(np.float32)
    w = (rng.standard_normal((512, 384)) / 22).astype(np.float32)
    h = B.GraphHandler(rocm)
    ta, tw = h.tensor([256, 512], 1), h.tensor([512, 384], 1)
    ta.set_input()
    tw.set_weight()
    out = h.matmul(ta, tw, None, False, False, None, B.ActType.Linear, ct)
    h.data_malloc()
    ta.copyin_numpy(a)
    tw.copyin_numpy(w)
    h.run()
    got = out.copyout_numpy().astype(np.float64).reshape(256, 384)
    exact = a.astype(np.float64) @ w.astype(np.float64)
    rough = rne_bf16(a).astype(np.float64) @ rne_bf16(w).astype(np.float64)
    want = split_product(a, w, ct) if ct == "bf16x3" else exact
    assert np.allclose(got, want, rtol=1e-4, atol=2e-5), np.abs(got - want).max()
    assert np.abs(got - exact).max() * 32 <= np.abs(rough - exact).max()  # not the "bf16" product
    if ct == "bf16x3":
        assert (np.abs(got - exact) <= 3 * 2.0 ** -16 * (np.abs(a).astype(np.float64) @ np.abs(w).astype(np.float64)) + 1e-4 * np.abs(exact) + 2e-5).all()
