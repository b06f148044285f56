"""MatMul routing without a GPU: infini_rocm_matmul_plan_route (csrc/gemm_route.h: gemm_plan) answers for a 256-CU device which of the
nine GEMM kernels a problem launches and with how many K slices — the routes bench.py's shapes depend on, what every forced variant
resolves to (the fall-backs included), and the alignment edges. tests/test_gpu_matmul.py::test_plan_route_agrees_with_the_launch
holds the planner to what a launch reports."""
import pytest
import torch

from infinitensor_amd import ops

NUM_CU = 256
ROW_BIAS = dict(bias=True, bias_stride_m=0, bias_stride_n=1)
NT, TN = dict(trans_b=True), dict(trans_a=True)

# (batch, m, n, k), extras, variant name, split-K factor (None: not split-K). Worked out by hand from the dispatcher as it stood before
# the planner existed and confirmed there on an MI355X (ops.matmul, then ops.matmul_last_variant) for bf16 and f16.
HEURISTIC = [
    ((1, 4096, 4096, 4096), {}, "wave128", None),
    ((1, 4096, 4096, 4096), TN, "wave128", None),
    ((1, 4096, 4096, 4096), NT, "persist256", None),  # both operands K-major: the four-wave kernel measured behind
    ((1, 4096, 4096, 4096), ROW_BIAS, "persist256", None),
    ((1, 4096, 4096, 2048), {}, "wave128", None),
    ((1, 4096, 4096, 1024), {}, "persist256", None),  # K < 2048
    ((1, 8192, 8192, 8192), {}, "persist256", None),  # more than two rounds of tiles
    ((1, 4096, 4100, 4096), {}, "generic64", None),   # n % 8 != 0 with an N-major B
    ((1, 16384, 3072, 768), dict(ROW_BIAS, act=5), "persist256", None),  # BERT FFN1 (+ Gelu)
    ((1, 16384, 768, 3072), ROW_BIAS, "persist192", None),               # BERT FFN2
    ((1, 16384, 2304, 768), ROW_BIAS, "persist192", None),               # BERT fused QKV
    ((2, 2048, 11008, 4096), {}, "persist256", None),                    # Llama gate / up
    ((1, 2048, 4096, 11008), {}, "tile256_splitk", 2),                   # Llama down projection
    ((1, 128, 1000, 2048), ROW_BIAS, "tile256_splitk", 4),               # a classifier head
    ((1, 2048, 2048, 2048), {}, "persist128", None),
    ((1, 1024, 1024, 1024), {}, "tile256_splitk", 2),
    ((1, 512, 512, 4096), {}, "tile256_splitk", 8),
    ((32, 512, 512, 64), {}, "persist128", None),
    ((1, 4104, 3080, 128), {}, "persist256", None),
    ((1, 300, 256, 256), {}, "fast128_glds", None),
    ((1, 33, 48, 64), {}, "fast128_glds", None),
]


def route(dtype, shape, **kw):
    return ops.matmul_plan_route(dtype, *shape, num_cu=NUM_CU, **kw)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
@pytest.mark.parametrize("shape,extras,name,splits", HEURISTIC, ids=[f"{i:02d}_{'x'.join(map(str, r[0]))}" for i, r in enumerate(HEURISTIC)])
def test_heuristic_routes_on_256_cus(dtype, shape, extras, name, splits):
    got, got_splits = route(dtype, shape, **extras)
    assert got == name
    assert got_splits == (splits if splits is not None else 1)


def test_fp32_routes():
    """The cases of test_matmul_fp32_heuristic_picks_the_tile_kernel_for_large_problems, and the reduced-precision compute types:
    16-bit products run the split-K kernel with fp32 output wherever the 256-row family serves the problem, the exact kernels otherwise."""
    f32 = torch.float32
    assert route(f32, (1, 2048, 2048, 512)) == ("fast32", 1)
    assert route(f32, (1, 64, 2048, 512)) == ("fast32", 1)
    assert route(f32, (1, 32, 64, 32)) == ("generic64", 1)
    assert route(f32, (1, 2048, 2048, 512), trans_a=True) == ("generic64", 1)
    for ct in ("bf16", "fp16"):
        assert route(f32, (3, 256, 512, 512), stride_b=0, compute_type=ct) == ("tile256_splitk", 1)
        assert route(f32, (3, 256, 512, 504), stride_b=0, compute_type=ct) == ("fast32", 1)  # K % 64 != 0: an exact kernel
        assert route(f32, (3, 256, 512, 2048), stride_b=0, compute_type=ct) == ("tile256_splitk", 4)
        # a batch stride that is neither 0 nor one dense block, a head-split or grouped output: exact
        assert route(f32, (3, 256, 512, 512), stride_b=2 * 512 * 512, compute_type=ct) == ("fast32", 1)
        assert route(f32, (3, 256, 512, 512), stride_b=0, stride_c=256 * 512, compute_type=ct) == ("fast32", 1)
    assert route(f32, (3, 256, 512, 512), stride_b=0) == ("fast32", 1)
    assert route(torch.bfloat16, (3, 256, 512, 512), stride_b=0, compute_type="bf16")[0] != "tile256_splitk"  # 16-bit operands ignore it


SMALL = (1, 300, 256, 256)   # too few tiles for any 256-row kernel by the heuristic, outside the four-wave kernel's contract (m % 256)
TILES = (1, 1024, 1024, 1024)  # 16 whole 256^2 tiles, K % 128 == 0: every 16-bit kernel can serve it
FORCED = [
    # variant, shape, extras, dtype, name, splits
    (-1, SMALL, {}, torch.bfloat16, "fast128_glds", 1),
    (0, SMALL, {}, torch.bfloat16, "generic64", 1),
    (1, SMALL, {}, torch.bfloat16, "fast128_glds", 1),
    (2, SMALL, {}, torch.bfloat16, "tile256", 1),
    (3, SMALL, {}, torch.bfloat16, "tile256_splitk", 2),  # K / 512 = 0 slices by the factor: forced split-K runs two
    (4, SMALL, {}, torch.bfloat16, "persist256", 1),
    (5, SMALL, {}, torch.bfloat16, "persist192", 1),
    (6, SMALL, {}, torch.bfloat16, "persist128", 1),
    (7, SMALL, {}, torch.bfloat16, "fast128_glds", 1),    # fast32 on 16-bit operands: back to the heuristic
    (8, SMALL, {}, torch.bfloat16, "fast128_glds", 1),    # wave128 outside its contract: back to the heuristic
    (-1, TILES, {}, torch.float16, "tile256_splitk", 2),
    (0, TILES, {}, torch.float16, "generic64", 1),
    (1, TILES, {}, torch.float16, "fast128_glds", 1),
    (2, TILES, {}, torch.float16, "tile256", 1),
    (3, TILES, {}, torch.float16, "tile256_splitk", 2),
    (4, TILES, {}, torch.float16, "persist256", 1),
    (5, TILES, {}, torch.float16, "persist192", 1),
    (6, TILES, {}, torch.float16, "persist128", 1),
    (7, TILES, {}, torch.float16, "tile256_splitk", 2),
    (8, TILES, {}, torch.float16, "wave128", 1),
    (7, TILES, {}, torch.float32, "fast32", 1),
    (7, (1, 32, 64, 32), {}, torch.float32, "fast32", 1),  # forced below the heuristic's 16 tiles
    (3, TILES, {}, torch.float32, "generic64", 1),         # a 16-bit kernel forced on fp32 operands
    # the persistent kernels' epilogues: relu / Gelu and a row bias; everything else is the one-shot kernel's
    (4, TILES, dict(act=2), torch.bfloat16, "tile256", 1),
    (5, TILES, dict(act=2), torch.bfloat16, "tile256", 1),
    (6, TILES, dict(act=2), torch.bfloat16, "tile256", 1),
    (4, TILES, dict(bias=True, bias_stride_m=1, bias_stride_n=0), torch.bfloat16, "tile256", 1),
    (4, TILES, dict(ROW_BIAS, act=5), torch.bfloat16, "persist256", 1),
    (8, TILES, ROW_BIAS, torch.bfloat16, "tile256_splitk", 2),  # the four-wave kernel has no epilogue: the heuristic's answer
    (2, (1, 128, 128, 72), {}, torch.bfloat16, "fast128_glds", 1),  # K % 64 != 0: 128^2 tiles
    (4, (1, 128, 128, 72), {}, torch.bfloat16, "fast128_glds", 1),
    (1, (1, 128, 128, 7), {}, torch.bfloat16, "generic64", 1),      # K % 8 != 0
    (2, (1, 128, 128, 7), {}, torch.bfloat16, "generic64", 1),
]


@pytest.mark.parametrize("variant,shape,extras,dtype,name,splits", FORCED,
                         ids=[f"{i:02d}_v{r[0]}_{'x'.join(map(str, r[1]))}" for i, r in enumerate(FORCED)])
def test_every_forced_variant_resolves_as_stated(variant, shape, extras, dtype, name, splits):
    assert route(dtype, shape, variant=variant, **extras) == (name, splits)


def test_every_variant_value_is_forced_on_both_problems_and_bad_arguments_are_errors():
    for shape in (SMALL, TILES):
        assert {r[0] for r in FORCED if r[1] is shape and not r[2] and r[3] != torch.float32} == set(range(-1, 9))
    for bad in (dict(variant=9), dict(variant=-2), dict(act=6), dict(num_cu=0), dict(head_dim=12)):
        with pytest.raises(RuntimeError):
            ops.matmul_plan_route(torch.bfloat16, *TILES, **bad)
    with pytest.raises(RuntimeError):
        ops.matmul_plan_route(torch.int32, *TILES)
    with pytest.raises(RuntimeError):
        ops.matmul_plan_route(torch.bfloat16, 3, 256, 256, 64, stride_c=100)  # overlapping output blocks
    assert ops.matmul_plan_route(torch.bfloat16, 1, 0, 256, 64) == ("none", 0)


def test_operand_alignment():
    """The LDS-DMA kernels read A and B in 16-byte runs: an operand 8 bytes off sends the problem to the generic kernel. C 8 bytes off
    keeps the 256-row family (its epilogue falls back to 8-byte stores by itself) but not the four-wave kernel or the 128^2 tiles."""
    big = (1, 4096, 4096, 4096)
    for dtype in (torch.bfloat16, torch.float16):
        assert route(dtype, big, a_lo=8) == ("generic64", 1)
        assert route(dtype, big, b_lo=8) == ("generic64", 1)
        assert route(dtype, big, c_lo=8) == ("persist256", 1)
        assert route(dtype, big, c_lo=4) == ("generic64", 1)
        assert route(dtype, SMALL, c_lo=8) == ("generic64", 1)
        assert route(dtype, (1, 300, 254, 256), trans_b=True, c_lo=8) == ("fast128_glds", 1)  # n % 4 != 0: scalar stores anyway
    assert route(torch.float32, (1, 2048, 2048, 512), a_lo=8) == ("generic64", 1)
    assert route(torch.float32, (3, 256, 512, 512), stride_b=0, compute_type="bf16", c_lo=8) == ("fast32", 1)
    assert route(torch.float32, (3, 256, 512, 512), stride_b=0, compute_type="bf16", a_lo=8) == ("tile256_splitk", 1)  # A and B are copied


def test_the_tables_reach_every_variant():
    names = {r[2] for r in HEURISTIC} | {r[4] for r in FORCED}
    assert names == set(ops.matmul_variants())
    assert len(names) == 9
