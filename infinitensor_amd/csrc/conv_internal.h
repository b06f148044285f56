// Launchers the Conv2d dispatcher (conv.hip) and the conv_s1.hip family share. Each returns -1 when the operands do not qualify
// (alignment, 32-bit offset limits, unprovable slack around a tensor): the caller takes its next candidate. Any other value is a status.
#pragma once
#include "conv_route.h"

namespace irocm {

// conv_s1.hip: pixel-slot GEMM of a strided pointwise layer, tap GEMM, or the planned tap-shifted / patch / resident kernel form
int launch_conv_s1(infiniRocmRuntime_t rt, int dtype, const void *x, const void *w, const void *bias, const void *res, void *y,
                   const ConvProblem &q, const ConvS1Plan &plan, const ConvHooks &hk);

// conv_dw.hip
int launch_conv_depthwise(infiniRocmRuntime_t rt, int dtype, const void *x, const void *w, const void *bias, void *y, int64_t n, int64_t c,
                          int64_t h, int64_t wd, int64_t f, int r, int s, int ph, int pw, int sh, int sw, int oh, int ow, int act);

// gemm32.hip: fp32 implicit GEMM (groups == 1)
int launch_conv_igemm32(infiniRocmRuntime_t rt, const void *x, const void *w, const void *bias, const void *res, void *y, int64_t n,
                        int64_t c, int64_t h, int64_t wd, int64_t f, int r, int s, int ph, int pw, int sh, int sw, int dh, int dw, int oh,
                        int ow, int act, const ConvHooks &hk);

// gemm256p_conv.hip: a pointwise layer over a dense [n][c][hw] activation as one GEMM over pixel slots
int launch_conv_pw_gemm(infiniRocmRuntime_t rt, int dtype, const void *x, const void *w, const void *bias, const void *res, void *y,
                        int64_t n, int64_t c, int64_t hw, int64_t f, int act, const ConvHooks &hk);

// gemm256p_conv3.hip: a 3 x 3 / pad 1 layer as one GEMM with K = 9 C (split, slab: conv_tap_split)
int launch_conv_tap_gemm(infiniRocmRuntime_t rt, int dtype, const void *x, const void *wp, const void *bias, void *y, int64_t n,
                         int64_t c, int oh, int ow, int in_h, int in_w, int stride, int64_t plane_elems, int64_t f, int act,
                         int split, void *slab, size_t slab_bytes, const ConvHooks &hk);

} // namespace irocm
