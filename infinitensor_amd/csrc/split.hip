// bf16 split of an fp32 operand: the input pass of the "bf16x3" / "bf16x6" compute types of an fp32 MatMul (gemm_route.h, gemm.hip).
//
// Every value x becomes up to three bf16 pieces, rne = round-to-nearest-even to bf16:
//     p0 = rne(x)      p1 = rne(x - p0)      p2 = rne((x - p0) - p1)
// Both subtractions are exact in fp32, so p0 + p1 carries 16 and p0 + p1 + p2 all 24 significant bits of x. A p0 that is not
// finite (x is Inf or NaN, or rounds up to Inf) zeroes the lower pieces: Inf stays (Inf, 0, 0) instead of turning into NaN by Inf - Inf.
//
// The destination is the operand AS THE GEMM READS IT with K' = terms * K: plane t holds piece plane_piece[t] of every element.
//     K-major source [rows][K]:   plane t = columns t * K .. of a row of pitch terms * K
//     source stored  [K][cols]:   plane t = rows    t * K .. (a dense block behind plane t - 1)
// One pass over the input, 8 elements per thread: two 16-byte loads, one 16-byte store per plane. HBM-bound — 4 bytes read and
// 2 * terms bytes written per element.
#include "gemm_common.h"

namespace irocm {

// table: plane_piece[t] in bits 2 t, 2 t + 1. `span`: the elements after which the source moves on to the next `terms` planes, which is
// also the distance between two planes — one source row (K) of a K-major operand, one whole block (K * cols) otherwise. span % 8 == 0,
// so the 8 elements of a thread never straddle two spans.
__global__ __launch_bounds__(256) void split_bf16_kernel(const float *__restrict__ x, unsigned short *__restrict__ y, long groups,
                                                         long span, int terms, unsigned table) {
    for (long g = (long)blockIdx.x * 256 + threadIdx.x; g < groups; g += (long)gridDim.x * 256) {
        const long e = g * 8;
        const f32x4 lo = *(const f32x4 *)(x + e), hi = *(const f32x4 *)(x + e + 4);
        const float v[8] = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
        float r1[8], r2[8];
        u32x4_t piece[3];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const unsigned p0 = Bf16Traits::pack2(v[2 * j], v[2 * j + 1]);
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const float f0 = Bf16Traits::to_f32((unsigned short)(p0 >> (16 * h)));
                r1[2 * j + h] = __builtin_isfinite(f0) ? v[2 * j + h] - f0 : 0.f;
            }
            const unsigned p1 = Bf16Traits::pack2(r1[2 * j], r1[2 * j + 1]);
#pragma unroll
            for (int h = 0; h < 2; ++h)
                r2[2 * j + h] = r1[2 * j + h] - Bf16Traits::to_f32((unsigned short)(p1 >> (16 * h)));
            piece[0][j] = p0;
            piece[1][j] = p1;
            piece[2][j] = Bf16Traits::pack2(r2[2 * j], r2[2 * j + 1]);
        }
        const long outer = e / span, inner = e - outer * span;
        unsigned short *dst = y + outer * terms * span + inner;
        for (int t = 0; t < terms; ++t) {
            const unsigned pp = (table >> (2 * t)) & 3u;
            *(u32x4_t *)(dst + (long)t * span) = pp == 0 ? piece[0] : pp == 1 ? piece[1] : piece[2];
        }
    }
}

} // namespace irocm

using namespace irocm;

extern "C" {

int infini_rocm_split_bf16(infiniRocmRuntime_t rt, const void *x, void *y, int64_t blocks, int64_t rows, int64_t cols, int k_is_cols,
                           int terms, const int *plane_piece) {
    IROCM_CHECK_ARG(rt && plane_piece, "split_bf16: NULL argument");
    IROCM_CHECK_ARG(terms >= 1 && terms <= kSplitMaxTerms, "split_bf16: %d planes (1 to %d)", terms, kSplitMaxTerms);
    unsigned table = 0;
    for (int t = 0; t < terms; ++t) {
        IROCM_CHECK_ARG(plane_piece[t] >= 0 && plane_piece[t] <= 2, "split_bf16: plane %d holds piece %d (0, 1 or 2)", t, plane_piece[t]);
        table |= (unsigned)plane_piece[t] << (2 * t);
    }
    IROCM_CHECK_ARG(blocks >= 0 && rows >= 0 && cols >= 0, "split_bf16: negative extent");
    IROCM_CHECK_ARG(cols % 8 == 0, "split_bf16: %lld columns (16-byte runs: a multiple of 8)", (long long)cols);
    IROCM_CHECK_ARG(blocks < (1ll << 31) && rows < (1ll << 31) && cols < (1ll << 31) &&
                        (blocks == 0 || rows * cols < (1ll << 59) / kSplitMaxTerms / blocks),
                    "split_bf16: extent too large");
    if (blocks == 0 || rows == 0 || cols == 0)
        return INFINI_ROCM_OK;
    IROCM_CHECK_ARG(x && y, "split_bf16: NULL tensor");
    IROCM_CHECK_ARG((((uintptr_t)x | (uintptr_t)y) & 15) == 0, "split_bf16: x and y must be 16-byte aligned");
    const long groups = (long)(blocks * rows * cols / 8);
    long grid = ceil_div(groups, 256);
    if (grid > (long)rt->num_cu * 16)
        grid = (long)rt->num_cu * 16;
    hipLaunchKernelGGL(split_bf16_kernel, dim3((unsigned)grid), dim3(256), 0, rt->stream, (const float *)x, (unsigned short *)y, groups,
                       (long)(k_is_cols ? cols : rows * cols), terms, table);
    IROCM_LAUNCH_CHECK("split_bf16");
    return INFINI_ROCM_OK;
}

} // extern "C"
