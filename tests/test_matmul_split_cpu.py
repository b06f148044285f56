"""Routing of the "bf16x3" / "bf16x6" compute types of an fp32 MatMul without a GPU (csrc/gemm_route.h through
infini_rocm_matmul_plan_route, 256 CUs): the split problem is the bf16 one with K' = terms * K (terms = 3 / 6), so the split-K factor is
gemm_f32out_splits on K' — min(CUs / 256^2 tiles, K' / 512), at least 1, at most 16 — and everything the 16-bit compute types send to the
exact kernels goes there too, plus the limits that K' reaches earlier than K. Expected values are worked out by hand below."""
import pytest
import torch

from infinitensor_amd import ops

NUM_CU = 256
F32 = torch.float32
TERMS = {"bf16x3": 3, "bf16x6": 6}


def route(dtype, shape, **kw):
    return ops.matmul_plan_route(dtype, *shape, num_cu=NUM_CU, **kw)


# (batch, m, n, k), extras, splits under x3, splits under x6:   tiles = ceil(m / 256) ceil(n / 256) batch
SPLITS = [
    ((1, 256, 512, 512), {}, 3, 6),                    # 2 tiles -> 128 by tiles; K' = 1536 / 3072 -> 3 / 6 by K
    ((3, 256, 512, 512), dict(stride_b=0), 3, 6),      # 6 tiles -> 42; the same K'
    ((1, 512, 768, 256), {}, 1, 3),                    # K' = 768 -> 1 (one slice: the kernel writes C itself); 1536 -> 3
    ((1, 300, 520, 1024), {}, 6, 12),                  # 2 x 3 ragged tiles -> 42; K' = 3072 / 6144
    ((1, 256, 256, 4096), {}, 16, 16),                 # K' / 512 = 24 / 48: the cap
    ((1, 2048, 4096, 4096), {}, 2, 2),                 # the Llama projection: 128 tiles -> 2
    ((1, 4096, 4096, 4096), {}, 1, 1),                 # 256 tiles fill the device
    ((1, 64, 72, 128), {}, 1, 1),                      # K' = 384 / 768
    ((1, 64, 72, 1024), {}, 6, 12),
]


@pytest.mark.parametrize("shape,extras,s3,s6", SPLITS, ids=["x".join(map(str, r[0])) for r in SPLITS])
def test_split_modes_run_the_split_k_kernel_on_k_prime(shape, extras, s3, s6):
    for ta in (False, True):
        for tb in (False, True):
            if ta and shape[1] % 8:
                continue  # an M-major A needs m % 8 == 0 (below)
            assert route(F32, shape, trans_a=ta, trans_b=tb, compute_type="bf16x3", **extras) == ("tile256_splitk", s3)
            assert route(F32, shape, trans_a=ta, trans_b=tb, compute_type="bf16x6", **extras) == ("tile256_splitk", s6)


@pytest.mark.parametrize("ct", ["bf16x3", "bf16x6"])
def test_what_the_split_cannot_serve_keeps_the_exact_kernels(ct):
    base = (3, 256, 512, 512)
    assert route(F32, base, stride_b=0, compute_type=ct)[0] == "tile256_splitk"
    assert route(F32, (3, 256, 512, 504), stride_b=0, compute_type=ct) == ("fast32", 1)            # K % 64 != 0
    assert route(F32, base, stride_b=2 * 512 * 512, compute_type=ct) == ("fast32", 1)              # a batch stride of two blocks
    assert route(F32, base, stride_b=0, stride_c=256 * 512, compute_type=ct) == ("fast32", 1)      # grouped output
    assert route(F32, base, stride_b=0, c_lo=8, compute_type=ct) == ("fast32", 1)                  # misaligned C
    assert route(F32, (1, 256, 512, 512), head_dim=64, compute_type=ct) == ("fast32", 1)           # head-split output
    # the split kernel loads 16 bytes at a time: a misaligned A or B is exact too (and, 8 bytes off, the generic fp32 kernel's)
    assert route(F32, base, stride_b=0, a_lo=8, compute_type=ct) == ("generic64", 1)
    assert route(F32, base, stride_b=0, b_lo=8, compute_type=ct) == ("generic64", 1)
    # an M-major A (N-major B) is read in 16-byte runs along m (n)
    assert route(F32, (1, 300, 512, 512), trans_a=True, compute_type=ct) == ("generic64", 1)
    assert route(F32, (1, 256, 516, 512), compute_type=ct) == ("fast32", 1)
    # the exact types, and 16-bit operands under any type
    assert route(F32, base, stride_b=0) == ("fast32", 1)
    assert route(F32, base, stride_b=0, compute_type="tf32") == ("fast32", 1)
    for dt in (torch.bfloat16, torch.float16):
        assert route(dt, base, stride_b=0, compute_type=ct) == route(dt, base, stride_b=0)
        assert route(dt, (1, 512, 512, 4096), compute_type=ct) == ("tile256_splitk", 8)


def test_an_over_long_k_prime_keeps_the_exact_kernels():
    """gemm256_supported's 32-bit lane offsets, on the split copies: m * K' and n * K' stay below 2^31."""
    # n K = 2^30: fine for "bf16", 3 * 2^30 for x3
    assert route(F32, (1, 64, 1 << 16, 1 << 14), compute_type="bf16") == ("tile256_splitk", 1)
    assert route(F32, (1, 64, 1 << 16, 1 << 14), compute_type="bf16x3") == ("fast32", 1)
    assert route(F32, (1, 64, 1 << 16, 1 << 14), compute_type="bf16x6") == ("fast32", 1)
    # half that K: 3 * 2^29 < 2^31 for x3, 6 * 2^29 for x6
    assert route(F32, (1, 64, 1 << 16, 1 << 13), compute_type="bf16x3") == ("tile256_splitk", 1)
    assert route(F32, (1, 64, 1 << 16, 1 << 13), compute_type="bf16x6") == ("fast32", 1)
    # the same limit on m K' (A K-major)
    assert route(F32, (1, 1 << 16, 64, 1 << 14), compute_type="bf16x3") == ("fast32", 1)
    assert route(F32, (1, 1 << 16, 64, 1 << 13), compute_type="bf16x3") == ("tile256_splitk", 1)
    # right at the edge: K' = 3 * 10880 = 32640; 65792 * 32640 = 2^31 - 32768, 65800 * 32640 = 2^31 + 228352
    assert 65792 * 32640 < 2 ** 31 <= 65800 * 32640
    assert route(F32, (1, 64, 65792, 10880), compute_type="bf16x3") == ("tile256_splitk", 1)
    assert route(F32, (1, 64, 65800, 10880), compute_type="bf16x3") == ("fast32", 1)


def test_compute_type_numbers():
    """0 to 4 are compute types (3 = "bf16x3", 4 = "bf16x6"); 5 is not."""
    shape = (1, 256, 512, 512)
    assert route(F32, shape, compute_type=3) == route(F32, shape, compute_type="bf16x3") == ("tile256_splitk", 3)
    assert route(F32, shape, compute_type=4) == route(F32, shape, compute_type="bf16x6") == ("tile256_splitk", 6)
    assert route(F32, shape, compute_type=1) == route(F32, shape, compute_type="bf16") == ("tile256_splitk", 1)
    for bad in (5, -1):
        with pytest.raises(RuntimeError):
            route(F32, shape, compute_type=bad)
    with pytest.raises(KeyError):
        route(F32, shape, compute_type="bf16x9")
