"""Conv2d routing without a GPU: infini_rocm_conv2d_plan_route (csrc/conv_route.h) answers for a 256-CU device what
tests/test_gpu_bench_routes.py observes on one — the route of every ResNet-50 layer at batch 128 — plus the kernel form of
csrc/conv_s1.hip behind "tap_shifted" / "resident" that the routing comments state, and what each conv variant forces."""
import pytest
import torch

from infinitensor_amd import ops
from test_gpu_bench_routes import BATCH, LAYERS

NUM_CU = 256

# (C, H, F, R, stride) -> kernel form, from the measurements quoted in csrc/conv_route.h
FORMS = {
    (64, 56, 64, 3, 1): "resident",
    (128, 28, 128, 3, 1): "patch_wide",
    (256, 14, 256, 3, 1): "patch_wide",
    (3, 224, 64, 7, 2): "rowtap",
    (64, 56, 64, 1, 1): "s1<1,4,32>",
}


@pytest.mark.parametrize("layer", LAYERS, ids=lambda l: f"C{l[0]}_{l[1]}x{l[1]}_F{l[2]}_{l[3]}x{l[3]}s{l[4]}")
def test_resnet50_layer_routes_at_batch_128(layer):
    c, h, f, r, st, pad, route, epilogues = layer
    for ep in epilogues:
        got, form = ops.conv_plan_route(torch.float16, BATCH, c, h, h, f, r, r, pad, pad, st, st, act=0 if ep == "b" else 1,
                                        residual=ep == "brr", num_cu=NUM_CU)
        assert got == route, (ep, got, form)
        if (c, h, f, r, st) in FORMS:
            assert form == FORMS[(c, h, f, r, st)], (ep, got, form)
        elif got not in ("tap_shifted", "resident"):
            assert form == ""


def test_every_form_in_the_table_is_a_layer_of_the_bench():
    assert set(FORMS) <= {(l[0], l[1], l[2], l[3], l[4]) for l in LAYERS}


# No one shape is eligible for every variant (the pixel-slot GEMM wants a 1 x 1 window, the tap GEMM a 3 x 3 one), so two small
# layers share the table: a pointwise C128 -> F256 and a 3 x 3 / pad 1 C64 -> F128, both on 16 x 16 planes at batch 2 — too few
# tiles for the heuristic to pick a persistent-kernel route on its own, so every forced route below is the variant's doing.
POINTWISE = dict(n=2, c=128, h=16, w=16, f=256, r=1, s=1, ph=0, pw=0)
THREE = dict(n=2, c=64, h=16, w=16, f=128, r=3, s=3, ph=1, pw=1)
VARIANTS = [
    (-1, POINTWISE, "tap_shifted", "pw"),
    (-1, THREE, "tap_shifted", "patch"),
    (0, POINTWISE, "tap_shifted", "pw"),
    (0, THREE, "tap_shifted", "patch"),
    (1, POINTWISE, "generic", ""),
    (1, THREE, "generic", ""),
    (2, POINTWISE, "tap_shifted", "pw"),
    (2, THREE, "tap_shifted", "patch"),
    (3, POINTWISE, "batched_gemm", ""),
    (4, THREE, "tap_shifted", "s1<2,2,64>"),
    (5, POINTWISE, "pixel_gemm", ""),
    (6, THREE, "tap_shifted", "patch_wide"),
    (7, THREE, "tap_gemm", ""),
]


@pytest.mark.parametrize("variant,shape,route,form", VARIANTS, ids=[f"v{v[0]}_{'1x1' if v[1] is POINTWISE else '3x3'}" for v in VARIANTS])
def test_every_conv_variant_forces_the_route_its_name_says(variant, shape, route, form):
    assert ops.conv_plan_route(torch.float16, **shape, act=1, variant=variant, num_cu=NUM_CU) == (route, form)


def test_every_variant_value_is_covered_and_bad_ones_are_errors():
    assert {v[0] for v in VARIANTS} == set(range(-1, 8))
    with pytest.raises(RuntimeError):
        ops.conv_plan_route(torch.float16, **POINTWISE, variant=8)
    with pytest.raises(RuntimeError):
        ops.conv_plan_route(torch.float16, **POINTWISE, groups=3)


def test_fp32_and_depthwise_routes():
    assert ops.conv_plan_route(torch.float32, **THREE) == ("igemm32", "")
    assert ops.conv_plan_route(torch.float32, **THREE, variant=1) == ("direct32", "")
    assert ops.conv_plan_route(torch.float16, 2, 32, 16, 16, 32, 3, 3, 1, 1, groups=32) == ("depthwise", "")
