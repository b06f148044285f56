// MatMul for gfx950: hand-written MFMA GEMM kernels behind infini_rocm_matmul.
//
// Replaces matmulCublas::do_compute (reference: src/kernels/cuda/matmul.cc:67-174), which
// forwards to cublasGemmEx / cublasGemmStridedBatchedEx. Semantics (batch broadcast by zero
// stride, transA/transB, bias broadcast into C) follow that file and the op definition
// src/operators/matmul.cc:26-49.
//
// Kernels
//   gemm_generic16 / gemm_generic32 : any shape / stride / alignment; 64x64 tile, LDS staged
//       through registers with bounds checks, v_mfma_f32_16x16x32_{bf16,f16} or the exact-f32
//       v_mfma_f32_16x16x4_f32. Correctness anchor and fallback for ragged shapes.
//   gemm_fast128<A_KMAJOR,B_KMAJOR> : 16-bit, 128x128x64 tile, 4 waves (2x2, 64x64 each),
//       global->LDS by LDS-DMA (global_load_lds_dwordx4) into a double buffer, one barrier per
//       K-tile. K-major operands ([rows][k], k contiguous) are read with ds_read_b128 from an
//       XOR-swizzled image (swizzle applied on the global SOURCE address because the DMA
//       destination is lane-linear); M/N-major operands ([k][cols], the ONNX MatMul "NN" B and
//       the transA A) are read with the gfx950 transpose read ds_read_b64_tr_b16, so no
//       transposition pass is ever materialised.
//   gemm_256 (gemm256.hip)         : 256x256x64 tile, 8 waves, staggered LOAD | COMPUTE schedule; one tile per
//       workgroup, and the split-K form for few-tile / long-K shapes.
//   gemm256p (gemm256p_kernel.h)   : the same inner loop as ONE persistent workgroup per CU walking its tiles through a
//       flat K-tile pipeline (no cold prologue after the first tile, epilogues overlapped); tile widths 256 / 192 / 128.
#include "gemm_common.h"

namespace irocm {



// ------------------------------------------------------------------------------------------------
// Generic 16-bit kernel
// ------------------------------------------------------------------------------------------------
template <typename Tr> __global__ __launch_bounds__(256) void gemm_generic16(GemmArgs p) {
    constexpr int BM = 64, BN = 64, BK = 32, PITCH = BK + 8;
    __shared__ __attribute__((aligned(16))) unsigned short As[BM][PITCH];
    __shared__ __attribute__((aligned(16))) unsigned short Bs[BN][PITCH];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int wm = w >> 1, wn = w & 1;
    const int ib = blockIdx.z;
    const int m0 = (blockIdx.x / p.tiles_n) * BM, n0 = (blockIdx.x % p.tiles_n) * BN;
    const unsigned short *A = (const unsigned short *)p.a + (long)ib * p.a_bs;
    const unsigned short *B = (const unsigned short *)p.b + (long)ib * p.b_bs;

    f32x4 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
            acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    const bool a_kc = (p.a_cs == 1), b_kc = (p.b_rs == 1);
    for (int k0 = 0; k0 < p.k; k0 += BK) {
#pragma unroll
        for (int j = 0; j < (BM * BK) / 256; ++j) {
            const int idx = t + j * 256;
            int i, kk;
            if (a_kc) { kk = idx % BK; i = idx / BK; } else { i = idx % BM; kk = idx / BM; }
            const int gi = m0 + i, gk = k0 + kk;
            unsigned short v = 0;
            if (gi < p.m && gk < p.k)
                v = A[(long)gi * p.a_rs + (long)gk * p.a_cs];
            As[i][kk] = v;
        }
#pragma unroll
        for (int j = 0; j < (BN * BK) / 256; ++j) {
            const int idx = t + j * 256;
            int jn, kk;
            if (b_kc) { kk = idx % BK; jn = idx / BK; } else { jn = idx % BN; kk = idx / BN; }
            const int gj = n0 + jn, gk = k0 + kk;
            unsigned short v = 0;
            if (gj < p.n && gk < p.k)
                v = B[(long)gk * p.b_rs + (long)gj * p.b_cs];
            Bs[jn][kk] = v;
        }
        __syncthreads();
        s16x8_t af[2], bf[2];
#pragma unroll
        for (int i = 0; i < 2; ++i)
            af[i] = *(const s16x8_t *)&As[wm * 32 + i * 16 + (lane & 15)][(lane >> 4) * 8];
#pragma unroll
        for (int j = 0; j < 2; ++j)
            bf[j] = *(const s16x8_t *)&Bs[wn * 32 + j * 16 + (lane & 15)][(lane >> 4) * 8];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
                acc[i][j] = Tr::mfma(af[i], bf[j], acc[i][j]);
        __syncthreads();
    }
    // one copy of the epilogue per activation class (0 none, 1 relu, 5 A-S Gelu, -1 = p.act at run time): see gemm256p_kernel.h
    auto epilogue = [&](auto actc) __attribute__((always_inline)) {
        constexpr int ACT = decltype(actc)::value;
        auto act1 = [&](float v) {
            if constexpr (ACT == 1) return v > 0.f ? v : 0.f;
            else if constexpr (ACT == 5) return gelu_poly(v);
            else if constexpr (ACT < 0) return apply_act(v, p.act);
            else return v;
        };
        // C/D layout of 16x16 MFMA: col = lane & 15, row = (lane >> 4) * 4 + reg
        unsigned short *C = (unsigned short *)p.c + (long)ib * p.c_bs;
        const unsigned short *bias = (const unsigned short *)p.bias;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = m0 + wm * 32 + i * 16 + (lane >> 4) * 4 + r;
                    const int col = n0 + wn * 32 + j * 16 + (lane & 15);
                    if (row < p.m && col < p.n) {
                        float v = acc[i][j][r];
                        if (bias)
                            v += Tr::to_f32(bias[(long)ib * p.bias_b + (long)row * p.bias_m + (long)col * p.bias_n]);
                        v = act1(v);
                        C[c_off(p, row, col)] = Tr::from_f32(v);
                    }
                }
    };
    if (p.act == 0) epilogue(std::integral_constant<int, 0>{});
    else if (p.act == 1) epilogue(std::integral_constant<int, 1>{});
    else if (p.act == 5) epilogue(std::integral_constant<int, 5>{});
    else epilogue(std::integral_constant<int, -1>{});
}

// ------------------------------------------------------------------------------------------------
// Generic fp32 kernel: v_mfma_f32_16x16x4_f32 == an fmaf chain in k order (exact f32).
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gemm_generic32(GemmArgs p) {
    constexpr int BM = 64, BN = 64, BK = 16, PITCH = BK + 1;
    __shared__ float As[BM][PITCH];
    __shared__ float Bs[BN][PITCH];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int wm = w >> 1, wn = w & 1;
    const int ib = blockIdx.z;
    const int m0 = (blockIdx.x / p.tiles_n) * BM, n0 = (blockIdx.x % p.tiles_n) * BN;
    const float *A = (const float *)p.a + (long)ib * p.a_bs;
    const float *B = (const float *)p.b + (long)ib * p.b_bs;

    f32x4 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
            acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    const bool a_kc = (p.a_cs == 1), b_kc = (p.b_rs == 1);
    for (int k0 = 0; k0 < p.k; k0 += BK) {
#pragma unroll
        for (int j = 0; j < (BM * BK) / 256; ++j) {
            const int idx = t + j * 256;
            int i, kk;
            if (a_kc) { kk = idx % BK; i = idx / BK; } else { i = idx % BM; kk = idx / BM; }
            const int gi = m0 + i, gk = k0 + kk;
            float v = 0.f;
            if (gi < p.m && gk < p.k)
                v = A[(long)gi * p.a_rs + (long)gk * p.a_cs];
            As[i][kk] = v;
        }
#pragma unroll
        for (int j = 0; j < (BN * BK) / 256; ++j) {
            const int idx = t + j * 256;
            int jn, kk;
            if (b_kc) { kk = idx % BK; jn = idx / BK; } else { jn = idx % BN; kk = idx / BN; }
            const int gj = n0 + jn, gk = k0 + kk;
            float v = 0.f;
            if (gj < p.n && gk < p.k)
                v = B[(long)gk * p.b_rs + (long)gj * p.b_cs];
            Bs[jn][kk] = v;
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < BK / 4; ++kk) {
            float af[2], bf[2];
#pragma unroll
            for (int i = 0; i < 2; ++i)
                af[i] = As[wm * 32 + i * 16 + (lane & 15)][kk * 4 + (lane >> 4)];
#pragma unroll
            for (int j = 0; j < 2; ++j)
                bf[j] = Bs[wn * 32 + j * 16 + (lane & 15)][kk * 4 + (lane >> 4)];
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[i], bf[j], acc[i][j], 0, 0, 0);
        }
        __syncthreads();
    }
    float *C = (float *)p.c + (long)ib * p.c_bs;
    const float *bias = (const float *)p.bias;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = m0 + wm * 32 + i * 16 + (lane >> 4) * 4 + r;
                const int col = n0 + wn * 32 + j * 16 + (lane & 15);
                if (row < p.m && col < p.n) {
                    float v = acc[i][j][r];
                    if (bias)
                        v += bias[(long)ib * p.bias_b + (long)row * p.bias_m + (long)col * p.bias_n];
                    C[c_off(p, row, col)] = apply_act(v, p.act);
                }
            }
}

// ------------------------------------------------------------------------------------------------
// Fast 16-bit kernel, 128x128x64, LDS-DMA double buffer.
// ------------------------------------------------------------------------------------------------

template <typename Tr, bool A_KMAJOR, bool B_KMAJOR>
__global__ __launch_bounds__(256) void gemm_fast128(GemmArgs p) {
    using namespace f128;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    auto a_tile = [&](int buf) -> char * { return smem + buf * TILE_BYTES; };
    auto b_tile = [&](int buf) -> char * { return smem + (2 + buf) * TILE_BYTES; };

    const int t = threadIdx.x, lane = t & 63;
    const int w = __builtin_amdgcn_readfirstlane(t >> 6);
    const int wm = w >> 1, wn = w & 1;

    // workgroup -> (batch, tile_m, tile_n): XCD-aware remap, then grouped raster (8 tile-rows).
    const unsigned per_batch = (unsigned)p.tiles_m * p.tiles_n;
    unsigned wg = xcd_remap(blockIdx.x, gridDim.x);
    const int ib = wg / per_batch;
    wg -= ib * per_batch;
    constexpr int GROUP_M = 8;
    const unsigned per_group = GROUP_M * p.tiles_n;
    const unsigned group = wg / per_group;
    const int first_m = group * GROUP_M;
    const int gsz = min(p.tiles_m - first_m, GROUP_M);
    const int tm = first_m + (wg % per_group) % gsz;
    const int tn = (wg % per_group) / gsz;
    const int m0 = tm * BM, n0 = tn * BN;

    const unsigned short *A = (const unsigned short *)p.a + (long)ib * p.a_bs;
    const unsigned short *B = (const unsigned short *)p.b + (long)ib * p.b_bs;
    const long lda = A_KMAJOR ? p.a_rs : p.a_cs; // leading dimension of the stored matrix
    const long ldb = B_KMAJOR ? p.b_cs : p.b_rs;

    // chunks of the last K-tile that start at k >= p.k come from a block of zeros (k % 8 == 0 but k % 64 != 0)
    const unsigned short *Z = (const unsigned short *)p.zeros;
    auto stage = [&](int buf, int k0) {
        if constexpr (A_KMAJOR)
            stage_kmajor(A, lda, m0, p.m, k0, a_tile(buf), w, lane, p.k, Z);
        else
            stage_mnmajor(A, lda, m0, p.m, k0, a_tile(buf), w, lane, p.k, Z);
        if constexpr (B_KMAJOR)
            stage_kmajor(B, ldb, n0, p.n, k0, b_tile(buf), w, lane, p.k, Z);
        else
            stage_mnmajor(B, ldb, n0, p.n, k0, b_tile(buf), w, lane, p.k, Z);
    };

    f32x4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
            acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int nk = (p.k + BK - 1) / BK;
    // One K-tile step with a COMPILE-TIME buffer index: hipcc only keeps the LDS-DMA of the next
    // tile in flight across the ds_reads of the current one when it can prove the two LDS ranges
    // distinct; a runtime (kt & 1) index makes it drain vmcnt(0) before the first ds_read.
    auto step = [&](auto bufc, int kt) {
        constexpr int buf = decltype(bufc)::value;
        // tile kt has landed (own DMA waited for, then barrier => everybody's), and every wave has
        // finished reading the other buffer (its compute of tile kt-1 precedes this barrier).
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (kt + 1 < nk)
            stage(buf ^ 1, (kt + 1) * BK);
        const char *at = a_tile(buf), *bt = b_tile(buf);
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            s16x8_t af[4], bf[4];
#pragma unroll
            for (int i = 0; i < 4; ++i)
                af[i] = A_KMAJOR ? frag_kmajor(at, wm * 64 + i * 16, ks, lane)
                                 : frag_mnmajor(at, wm * 64 + i * 16, ks, lane);
#pragma unroll
            for (int j = 0; j < 4; ++j)
                bf[j] = B_KMAJOR ? frag_kmajor(bt, wn * 64 + j * 16, ks, lane)
                                 : frag_mnmajor(bt, wn * 64 + j * 16, ks, lane);
            // swapped operands: D[i][j] = sum_k Bop[k][i] Aop[j][k] = C[m = j][n = i], so a lane
            // ends up with 4 consecutive n of one m row (vector stores in the epilogue).
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    acc[i][j] = Tr::mfma(bf[j], af[i], acc[i][j]);
        }
    };
    stage(0, 0);
    for (int kt = 0; kt < nk; kt += 2) {
        step(std::integral_constant<int, 0>{}, kt);
        if (kt + 1 < nk)
            step(std::integral_constant<int, 1>{}, kt + 1);
    }

    // one copy of the epilogue per activation class (0 none, 1 relu, 5 A-S Gelu, -1 = p.act at run time): see gemm256p_kernel.h
    auto epilogue = [&](auto actc) __attribute__((always_inline)) {
        constexpr int ACT = decltype(actc)::value;
        auto act1 = [&](float v) {
            if constexpr (ACT == 1) return v > 0.f ? v : 0.f;
            else if constexpr (ACT == 5) return gelu_poly(v);
            else if constexpr (ACT < 0) return apply_act(v, p.act);
            else return v;
        };
        unsigned short *C = (unsigned short *)p.c + (long)ib * p.c_bs;
        const unsigned short *bias = (const unsigned short *)p.bias;
        const bool interior = (m0 + BM <= p.m) && (n0 + BN <= p.n) && (p.n % 4 == 0);
        if (interior && (p.n % 8 == 0) && ((((uintptr_t)p.c) & 15) == 0)) {
            // 16-byte stores by swapping half tiles between lane groups g4 / g4^1 (same exchange as gemm256.hip)
            const int l15 = lane & 15, g4 = lane >> 4;
            const bool odd = g4 & 1;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int row = m0 + wm * 64 + i * 16 + l15;
#pragma unroll
                for (int jp = 0; jp < 2; ++jp) {
                    unsigned pk[2][2];
#pragma unroll
                    for (int t2 = 0; t2 < 2; ++t2) {
                        const int col = n0 + wn * 64 + (jp * 2 + t2) * 16 + g4 * 4;
                        float v[4];
#pragma unroll
                        for (int r = 0; r < 4; ++r)
                            v[r] = acc[i][jp * 2 + t2][r];
                        if (bias) {
                            const unsigned short *bp = bias + (long)ib * p.bias_b + (long)row * p.bias_m + (long)col * p.bias_n;
#pragma unroll
                            for (int r = 0; r < 4; ++r)
                                v[r] += Tr::to_f32(bp[(long)r * p.bias_n]);
                        }
#pragma unroll
                        for (int r = 0; r < 4; ++r)
                            v[r] = act1(v[r]);
                        pk[t2][0] = (unsigned)Tr::from_f32(v[0]) | ((unsigned)Tr::from_f32(v[1]) << 16);
                        pk[t2][1] = (unsigned)Tr::from_f32(v[2]) | ((unsigned)Tr::from_f32(v[3]) << 16);
                    }
                    const unsigned s0 = odd ? pk[0][0] : pk[1][0], s1 = odd ? pk[0][1] : pk[1][1];
                    const unsigned r0 = (unsigned)__shfl_xor((int)s0, 16), r1 = (unsigned)__shfl_xor((int)s1, 16);
                    u32x4_t o;
                    if (odd) { o[0] = r0; o[1] = r1; o[2] = pk[1][0]; o[3] = pk[1][1]; }
                    else { o[0] = pk[0][0]; o[1] = pk[0][1]; o[2] = r0; o[3] = r1; }
                    const int col = n0 + wn * 64 + (jp * 2 + (odd ? 1 : 0)) * 16 + (g4 & ~1) * 4;
                    *(u32x4_t *)(C + c_off(p, row, col)) = o;
                }
            }
        } else if (interior) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int row = m0 + wm * 64 + i * 16 + (lane & 15);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int col = n0 + wn * 64 + j * 16 + (lane >> 4) * 4;
                    float v[4];
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        v[r] = acc[i][j][r];
                    if (bias) {
                        const unsigned short *bp = bias + (long)ib * p.bias_b + (long)row * p.bias_m + (long)col * p.bias_n;
#pragma unroll
                        for (int r = 0; r < 4; ++r)
                            v[r] += Tr::to_f32(bp[(long)r * p.bias_n]);
                    }
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        v[r] = act1(v[r]);
                    u32x2_t pk;
                    pk[0] = (unsigned)Tr::from_f32(v[0]) | ((unsigned)Tr::from_f32(v[1]) << 16);
                    pk[1] = (unsigned)Tr::from_f32(v[2]) | ((unsigned)Tr::from_f32(v[3]) << 16);
                    *(u32x2_t *)(C + c_off(p, row, col)) = pk;
                }
            }
        } else {
            for (int i = 0; i < 4; ++i) {
                const int row = m0 + wm * 64 + i * 16 + (lane & 15);
                for (int j = 0; j < 4; ++j) {
                    const int col = n0 + wn * 64 + j * 16 + (lane >> 4) * 4;
                    for (int r = 0; r < 4; ++r) {
                        // select the register with a static index (runtime-indexed vectors go to scratch)
                        float v = 0.f;
#pragma unroll
                        for (int ii = 0; ii < 4; ++ii)
#pragma unroll
                            for (int jj = 0; jj < 4; ++jj)
#pragma unroll
                                for (int rr = 0; rr < 4; ++rr)
                                    if (ii == i && jj == j && rr == r)
                                        v = acc[ii][jj][rr];
                        if (row < p.m && col + r < p.n) {
                            if (bias)
                                v += Tr::to_f32(bias[(long)ib * p.bias_b + (long)row * p.bias_m + (long)(col + r) * p.bias_n]);
                            C[c_off(p, row, col + r)] = Tr::from_f32(act1(v));
                        }
                    }
                }
            }
        }
    };
    if (p.act == 0) epilogue(std::integral_constant<int, 0>{});
    else if (p.act == 1) epilogue(std::integral_constant<int, 1>{});
    else if (p.act == 5) epilogue(std::integral_constant<int, 5>{});
    else epilogue(std::integral_constant<int, -1>{});
}

// implemented in gemm256.hip
int launch_gemm256(infiniRocmRuntime_t rt, int dtype, const GemmArgs &p, bool a_kmajor, bool b_kmajor);
namespace g256p { // persistent multi-tile kernels, tile 256 x 64 NT (gemm256p_kernel.h)
int launch_gemm256p_nt4(infiniRocmRuntime_t rt, int dtype, const GemmArgs &p, bool akm, bool bkm);
int launch_gemm256p_nt3(infiniRocmRuntime_t rt, int dtype, const GemmArgs &p, bool akm, bool bkm);
int launch_gemm256p_nt2(infiniRocmRuntime_t rt, int dtype, const GemmArgs &p, bool akm, bool bkm);
int launch_gemm256p_trace(infiniRocmRuntime_t rt, int dtype, const GemmArgs &p, int nt, unsigned long long *trace);
} // namespace g256p
int launch_gemm256_splitk(infiniRocmRuntime_t rt, int dtype, const GemmArgs &p, bool a_kmajor, bool b_kmajor, int splits);
int launch_gemm256_f32out(infiniRocmRuntime_t rt, int dtype16, const GemmArgs &p, bool a_kmajor, bool b_kmajor, int splits, float *planes);
namespace g128w { // four waves x 128 x 128 wave tiles, four-stage ring (gemm128w.hip): plain GEMMs on whole 256^2 tiles, K % 128 == 0
int launch_gemm128w(infiniRocmRuntime_t rt, int dtype, const GemmArgs &p, bool akm, bool bkm);
} // namespace g128w
// implemented in gemm32.hip: the fp32 128^2 LDS-DMA tile kernel (v_mfma_f32_32x32x2_f32)
int launch_fast32(infiniRocmRuntime_t rt, GemmArgs p, bool b_kmajor, int small_tiles);

template <typename Tr> static int launch_fast128(infiniRocmRuntime_t rt, GemmArgs p, bool akm, bool bkm) {
    p.tiles_m = (int)ceil_div(p.m, f128::BM);
    p.tiles_n = (int)ceil_div(p.n, f128::BN);
    const unsigned grid = (unsigned)p.tiles_m * p.tiles_n * p.batch;
    const size_t lds = 4 * f128::TILE_BYTES;
    return with_layout(akm, bkm, [&](auto ak, auto bk) -> int {
        auto kern = gemm_fast128<Tr, decltype(ak)::value, decltype(bk)::value>;
        IROCM_LDS_ATTR(kern, (int)lds, rt);
        hipLaunchKernelGGL(kern, dim3(grid), dim3(256), lds, rt->stream, p);
        IROCM_LAUNCH_CHECK("gemm_fast128");
        return INFINI_ROCM_OK;
    });
}

static int launch_generic64(infiniRocmRuntime_t rt, int dtype, GemmArgs p) {
    p.tiles_m = (int)ceil_div(p.m, 64);
    p.tiles_n = (int)ceil_div(p.n, 64);
    IROCM_CHECK_ARG((int64_t)p.tiles_m * p.tiles_n < (1ll << 31), "matmul: too many tiles");
    dim3 grid((unsigned)(p.tiles_m * p.tiles_n), 1, (unsigned)p.batch);
    if (dtype == INFINI_DT_F32)
        hipLaunchKernelGGL(gemm_generic32, grid, dim3(256), 0, rt->stream, p);
    else if (dtype == INFINI_DT_BF16)
        hipLaunchKernelGGL(gemm_generic16<Bf16Traits>, grid, dim3(256), 0, rt->stream, p);
    else
        hipLaunchKernelGGL(gemm_generic16<F16Traits>, grid, dim3(256), 0, rt->stream, p);
    IROCM_LAUNCH_CHECK("gemm_generic");
    return INFINI_ROCM_OK;
}

// The reduced-precision compute types of an fp32 MatMul (gemm_reduced_precision_ok): A and B are converted once into the workspace —
// (stride ? batch : 1) dense blocks each — and the split-K kernel writes fp32. The plan was made on shape and alignment alone, so
// the workspace is grown only for a problem that takes this path. "bf16" / "fp16" cast; "bf16x3" / "bf16x6" write `terms` bf16 planes
// per operand (split.hip) and the same kernel runs on K' = terms * K.
static int launch_f32_reduced(infiniRocmRuntime_t rt, int compute_type, GemmArgs p, bool akm, bool bkm, int splits) {
    const int dt16 = compute_type == 2 ? INFINI_DT_F16 : INFINI_DT_BF16;
    const int terms = gemm_split_terms(compute_type);
    const int64_t k = p.k, kp = (int64_t)terms * k;
    const int64_t mk = (int64_t)p.m * kp, nk = (int64_t)p.n * kp, mn = (int64_t)p.m * p.n;
    const bool a_shared = p.a_bs == 0 || p.batch == 1, b_shared = p.b_bs == 0 || p.batch == 1;
    const int64_t a_blocks = a_shared ? 1 : p.batch, b_blocks = b_shared ? 1 : p.batch;
    const int64_t na = a_blocks * mk, nb = b_blocks * nk;
    const size_t a_bytes = ((size_t)na * 2 + 255) & ~(size_t)255, b_bytes = ((size_t)nb * 2 + 255) & ~(size_t)255;
    char *ws = nullptr;
    int st = infini_rocm_workspace(rt, a_bytes + b_bytes + (size_t)splits * p.batch * mn * sizeof(float), (void **)&ws);
    if (st != INFINI_ROCM_OK)
        return st;
    if (terms == 1) {
        st = infini_rocm_cast(rt, INFINI_DT_F32, dt16, p.a, ws, na);
        if (st == INFINI_ROCM_OK)
            st = infini_rocm_cast(rt, INFINI_DT_F32, dt16, p.b, ws + a_bytes, nb);
    } else {
        // A is stored [m][k] (K-major) or [k][m]; B [n][k] (K-major) or [k][n]
        const int table = compute_type - 3;
        st = infini_rocm_split_bf16(rt, p.a, ws, a_blocks, akm ? p.m : k, akm ? k : p.m, akm ? 1 : 0, terms, kSplitPieceA[table]);
        if (st == INFINI_ROCM_OK)
            st = infini_rocm_split_bf16(rt, p.b, ws + a_bytes, b_blocks, bkm ? p.n : k, bkm ? k : p.n, bkm ? 1 : 0, terms, kSplitPieceB[table]);
        p.k = (int)kp;
        if (akm)
            p.a_rs = kp;
        if (bkm)
            p.b_cs = kp;
    }
    if (st != INFINI_ROCM_OK)
        return st;
    p.a = ws;
    p.b = ws + a_bytes;
    p.a_bs = a_shared ? 0 : mk;
    p.b_bs = b_shared ? 0 : nk;
    return launch_gemm256_f32out(rt, dt16, p, akm, bkm, splits, (float *)(ws + a_bytes + b_bytes));
}

} // namespace irocm

using namespace irocm;

extern "C" {

int infini_rocm_matmul_num_variants(void) { return kNumVariants; }

const char *infini_rocm_matmul_variant_name(int v) { return matmul_variant_name(v); }

int infini_rocm_matmul_last_variant(infiniRocmRuntime_t rt, int *variant) {
    IROCM_CHECK_ARG(rt && variant, "NULL argument");
    *variant = rt->last_matmul_variant;
    return INFINI_ROCM_OK;
}

// MatmulObj::getComputeType() (reference: matmul.cc:51-64 — "tf32" / "fp16" / "bf16" select cuBLAS compute types whose PRODUCTS
// take reduced-precision inputs while sums and outputs stay fp32). 0 "default" / "tf32": exact fp32 products (gfx950 has no
// xf32 MFMA; more accurate than asked). 1 "bf16", 2 "fp16": an fp32 MatMul converts A and B once into the workspace and runs the
// 16-bit MFMA kernel with fp32 accumulation and fp32 output — the reference's opt-in ~10x over exact fp32. 3 "bf16x3", 4 "bf16x6":
// the same kernel on two / three bf16 pieces per value, the cross products side by side along K (gemm_route.h; include/infini_rocm.h
// has the accuracy statement). Sticky per runtime (the plugin sets it around the one launch); ignored for 16-bit operands.
int infini_rocm_matmul_set_compute_type(infiniRocmRuntime_t rt, int compute_type) {
    IROCM_CHECK_ARG(rt, "NULL runtime");
    IROCM_CHECK_ARG(compute_type >= 0 && compute_type < kComputeTypes, "compute type %d: 0 default / tf32, 1 bf16, 2 fp16, 3 bf16x3, 4 bf16x6",
                    compute_type);
    rt->matmul_compute_type = compute_type;
    return INFINI_ROCM_OK;
}

int infini_rocm_matmul_set_variant(infiniRocmRuntime_t rt, int variant) {
    IROCM_CHECK_ARG(rt, "NULL runtime");
    IROCM_CHECK_ARG(variant >= -1 && variant < kNumVariants, "variant %d out of range", variant);
    rt->matmul_variant = variant;
    return INFINI_ROCM_OK;
}

// Split-K's fp32 partial planes take the runtime workspace. (So do the 16-bit copies of the reduced-precision compute types, which
// this answer does not know about: kept as it is — callers rely on today's answer, and changing it is a change of behaviour.)
int infini_rocm_matmul_may_use_workspace(infiniRocmRuntime_t rt, int64_t batch, int64_t m, int64_t n, int *may) {
    IROCM_CHECK_ARG(rt && may, "NULL argument");
    *may = (rt->matmul_variant == kGemmTile256SplitK || gemm_splitk_tiles_fit(batch, m, n, rt->num_cu)) ? 1 : 0;
    return INFINI_ROCM_OK;
}

int infini_rocm_matmul(infiniRocmRuntime_t rt, int dtype, const void *a, const void *b,
                       const void *bias, void *c, int64_t batch, int64_t m, int64_t n, int64_t k,
                       int trans_a, int trans_b, int64_t stride_a, int64_t stride_b,
                       int64_t bias_stride_b, int64_t bias_stride_m, int64_t bias_stride_n,
                       int act) {
    return infini_rocm_matmul_headsplit(rt, dtype, a, b, bias, c, batch, m, n, k, trans_a, trans_b, stride_a, stride_b,
                                        bias_stride_b, bias_stride_m, bias_stride_n, act, 0, 0);
}

int infini_rocm_matmul_headsplit(infiniRocmRuntime_t rt, int dtype, const void *a, const void *b,
                                 const void *bias, void *c, int64_t batch, int64_t m, int64_t n, int64_t k,
                                 int trans_a, int trans_b, int64_t stride_a, int64_t stride_b,
                                 int64_t bias_stride_b, int64_t bias_stride_m, int64_t bias_stride_n,
                                 int act, int64_t seq, int64_t head_dim) {
    return infini_rocm_matmul_grouped(rt, dtype, a, b, bias, c, batch, m, n, k, trans_a, trans_b, stride_a, stride_b, 0,
                                      bias_stride_b, bias_stride_m, bias_stride_n, act, seq, head_dim);
}

// argument checks shared by the launch entry and infini_rocm_matmul_plan_route
static int matmul_check_args(int dtype, int64_t batch, int64_t m, int64_t n, int64_t k, int64_t stride_c, int act, int64_t seq, int64_t head_dim) {
    IROCM_CHECK_ARG(stride_c == 0 || stride_c >= m * n || stride_c <= -(m * n) || batch <= 1,
                    "matmul: output blocks of %lld elements overlap at a batch stride of %lld", (long long)(m * n), (long long)stride_c);
    IROCM_CHECK_ARG(stride_c % 8 == 0, "matmul: the output batch stride must be a multiple of 8 elements (16-byte stores)");
    IROCM_CHECK_ARG((seq == 0) == (head_dim == 0), "matmul: seq and head_dim go together");
    if (head_dim) {
        IROCM_CHECK_ARG(seq > 0 && head_dim > 0 && head_dim % 8 == 0 && m % seq == 0 && n % head_dim == 0 &&
                            seq < (1ll << 31) && head_dim < (1ll << 31),
                        "matmul: head split [m/%lld][n/%lld][%lld][%lld] does not tile m = %lld, n = %lld (head_dim %% 8 == 0)",
                        (long long)seq, (long long)head_dim, (long long)seq, (long long)head_dim, (long long)m, (long long)n);
    }
    IROCM_CHECK_ARG(dtype == INFINI_DT_F32 || dtype == INFINI_DT_F16 || dtype == INFINI_DT_BF16,
                    "matmul: unsupported dtype %s", dtype_name(dtype));
    IROCM_CHECK_ARG(batch >= 0 && m >= 0 && n >= 0 && k >= 0, "matmul: negative dimension");
    IROCM_CHECK_ARG(batch < 65536 && m < (1ll << 31) && n < (1ll << 31) && k < (1ll << 31),
                    "matmul: dimension too large");
    IROCM_CHECK_ARG(act >= 0 && act <= 5, "matmul: bad act %d", act);
    return INFINI_ROCM_OK;
}

// everything of GemmArgs but the pointers
static GemmArgs matmul_args(int64_t batch, int64_t m, int64_t n, int64_t k, int trans_a, int trans_b, int64_t stride_a, int64_t stride_b,
                            int64_t stride_c, int64_t bias_stride_b, int64_t bias_stride_m, int64_t bias_stride_n, int act, int64_t seq,
                            int64_t head_dim) {
    GemmArgs p;
    p.a = p.b = p.bias = p.zeros = nullptr; p.c = nullptr;
    p.m = (int)m; p.n = (int)n; p.k = (int)k; p.batch = (int)batch;
    p.a_rs = trans_a ? 1 : k; p.a_cs = trans_a ? m : 1; p.a_bs = stride_a;
    p.b_rs = trans_b ? 1 : n; p.b_cs = trans_b ? k : 1; p.b_bs = stride_b;
    p.bias_b = bias_stride_b; p.bias_m = bias_stride_m; p.bias_n = bias_stride_n;
    p.c_bs = stride_c ? stride_c : m * n;
    p.act = act;
    p.tiles_m = p.tiles_n = 0;
    p.splitk = 1;
    p.partial = nullptr;
    p.epi16 = 1; // 16-byte epilogue stores
    p.hs_s = (int)seq;
    p.hs_d = (int)head_dim;
    return p;
}

int infini_rocm_matmul_grouped(infiniRocmRuntime_t rt, int dtype, const void *a, const void *b,
                               const void *bias, void *c, int64_t batch, int64_t m, int64_t n, int64_t k,
                               int trans_a, int trans_b, int64_t stride_a, int64_t stride_b, int64_t stride_c,
                               int64_t bias_stride_b, int64_t bias_stride_m, int64_t bias_stride_n,
                               int act, int64_t seq, int64_t head_dim) {
    IROCM_CHECK_ARG(rt, "NULL runtime");
    if (const int st = matmul_check_args(dtype, batch, m, n, k, stride_c, act, seq, head_dim); st != INFINI_ROCM_OK)
        return st;
    if (batch == 0 || m == 0 || n == 0)
        return INFINI_ROCM_OK;
    IROCM_CHECK_ARG(a && b && c, "matmul: NULL operand");

    GemmArgs p = matmul_args(batch, m, n, k, trans_a, trans_b, stride_a, stride_b, stride_c, bias_stride_b, bias_stride_m, bias_stride_n,
                             act, seq, head_dim);
    p.a = a; p.b = b; p.bias = bias; p.c = c;
    p.zeros = rt->zeros;
    const bool akm = !trans_a, bkm = trans_b != 0;

    const GemmPlan plan = gemm_plan(gemm_problem(p, dtype, akm, bkm, stride_c != 0), rt->matmul_variant, rt->matmul_compute_type, rt->num_cu);
    rt->last_matmul_variant = plan.variant;
    switch (plan.variant) {
    case kGemmFast32:
        return launch_fast32(rt, p, bkm, plan.fast32_small ? 1 : 0);
    case kGemmWave128:
        return g128w::launch_gemm128w(rt, dtype, p, akm, bkm);
    case kGemmPersist256:
        return g256p::launch_gemm256p_nt4(rt, dtype, p, akm, bkm);
    case kGemmPersist192:
        return g256p::launch_gemm256p_nt3(rt, dtype, p, akm, bkm);
    case kGemmPersist128:
        return g256p::launch_gemm256p_nt2(rt, dtype, p, akm, bkm);
    case kGemmTile256SplitK:
        return plan.reduced_precision ? launch_f32_reduced(rt, rt->matmul_compute_type, p, akm, bkm, plan.splits)
                                      : launch_gemm256_splitk(rt, dtype, p, akm, bkm, plan.splits);
    case kGemmTile256:
        return launch_gemm256(rt, dtype, p, akm, bkm);
    case kGemmFast128:
        return dtype == INFINI_DT_BF16 ? launch_fast128<Bf16Traits>(rt, p, akm, bkm) : launch_fast128<F16Traits>(rt, p, akm, bkm);
    default:
        return launch_generic64(rt, dtype, p);
    }
}

// What infini_rocm_matmul_grouped would launch for this problem on `num_cu` CUs under `variant` (-1: the heuristic) and `compute_type`,
// given the low four address bits of the operands: gemm_plan without a runtime or a GPU. *splits is 1 unless the answer is split-K.
int infini_rocm_matmul_plan_route(int dtype, int64_t batch, int64_t m, int64_t n, int64_t k, int trans_a, int trans_b, int64_t stride_a,
                                  int64_t stride_b, int64_t stride_c, int has_bias, int64_t bias_stride_m, int64_t bias_stride_n, int act,
                                  int64_t head_dim, int compute_type, int variant, int num_cu, int a_lo, int b_lo, int c_lo,
                                  const char **name, int *splits) {
    IROCM_CHECK_ARG(name && splits, "NULL argument");
    IROCM_CHECK_ARG(variant >= -1 && variant < kNumVariants && compute_type >= 0 && compute_type < kComputeTypes && num_cu > 0,
                    "matmul: bad variant %d / compute type %d / CU count %d", variant, compute_type, num_cu);
    const int64_t seq = head_dim ? (m > 0 ? m : 1) : 0; // one head-split block: routing reads head_dim only
    if (const int st = matmul_check_args(dtype, batch, m, n, k, stride_c, act, seq, head_dim); st != INFINI_ROCM_OK)
        return st;
    *name = "none";
    *splits = 0;
    if (batch == 0 || m == 0 || n == 0)
        return INFINI_ROCM_OK;
    GemmProblem q = gemm_problem(matmul_args(batch, m, n, k, trans_a, trans_b, stride_a, stride_b, stride_c, 0, bias_stride_m, bias_stride_n,
                                             act, seq, head_dim),
                                 dtype, !trans_a, trans_b != 0, stride_c != 0);
    q.bias = has_bias != 0;
    q.a_lo = a_lo & 15; q.b_lo = b_lo & 15; q.c_lo = c_lo & 15;
    const GemmPlan plan = gemm_plan(q, variant, compute_type, num_cu);
    *name = matmul_variant_name(plan.variant);
    *splits = plan.splits;
    return INFINI_ROCM_OK;
}

// Diagnostics: one launch of the persistent GEMM (bf16, NN, no bias) with every wave stamping s_memtime at its phase
// boundaries; trace receives [min(tiles, CUs)][8][128] stamps (0 = unused slot): slot 0 kernel entry, then per K-tile
// {L1 start, L2 start}, per tile {epilogue start, epilogue end}, last = after the final store drain.
int infini_rocm_probe_gemm_timeline(infiniRocmRuntime_t rt, const void *a, const void *b, void *c, int64_t m, int64_t n,
                                    int64_t k, int tile_cols, void *trace) {
    IROCM_CHECK_ARG(rt && a && b && c && trace, "probe: NULL argument");
    IROCM_CHECK_ARG(tile_cols == 256 || tile_cols == 192, "probe: tile_cols must be 256 or 192");
    GemmArgs p;
    memset(&p, 0, sizeof(p));
    p.a = a; p.b = b; p.c = c;
    p.m = (int)m; p.n = (int)n; p.k = (int)k; p.batch = 1;
    p.a_rs = k; p.a_cs = 1; p.b_rs = n; p.b_cs = 1;
    p.splitk = 1; p.epi16 = 1; p.zeros = rt->zeros;
    IROCM_CHECK_ARG(gemm256_supported(gemm_problem(p, INFINI_DT_BF16, true, false)), "probe: shape not served by the 256-row kernels");
    return g256p::launch_gemm256p_trace(rt, INFINI_DT_BF16, p, tile_cols / 64, (unsigned long long *)trace);
}

} // extern "C"
