// MatMul routing: which of the nine GEMM kernels serves a problem, with how many K slices. Host code only, plain C++17: no HIP call, no
// runtime object — gemm_plan is a pure function of the problem, the forced variant, the compute type and the CU count, so
// infini_rocm_matmul_plan_route (and the CPU tests) can ask it without a GPU. gemm.hip validates, fills GemmArgs, asks gemm_plan and
// launches what it says. Unlike the conv planner this one sees everything the kernels' contracts depend on (the low address bits
// included), so no launcher declines: each kernel's contract is ONE predicate here, and the launchers that re-check defensively call it.
#pragma once
#include "infini_rocm.h"
#include <cstdint>

namespace irocm {

// infini_rocm_matmul_set_variant's argument and what infini_rocm_matmul_last_variant reports (include/infini_rocm.h).
// 1-6 and 8 serve f16 / bf16, 7 serves f32, 0 everything.
enum MatmulVariant : int {
    kGemmHeuristic = -1,    // the cost model below
    kGemmGeneric64 = 0,     // gemm_generic16 / gemm_generic32 (gemm.hip): any shape, stride, alignment
    kGemmFast128 = 1,       // gemm_fast128 (gemm.hip): 128 x 128 x 64 LDS-DMA tiles
    kGemmTile256 = 2,       // gemm256_kernel (gemm256.hip): one 256^2 tile per workgroup, every epilogue
    kGemmTile256SplitK = 3, // ... with `splits` workgroups per tile and a reduce pass over fp32 planes in the workspace
    kGemmPersist256 = 4,    // gemm256p_kernel (gemm256p_kernel.h): one persistent workgroup per CU, 256-column tiles
    kGemmPersist192 = 5,    //   192-column tiles
    kGemmPersist128 = 6,    //   128-column tiles
    kGemmFast32 = 7,        // gemm_fast32 (gemm32.hip): fp32 LDS-DMA tiles, 128^2 or 64^2
    kGemmWave128 = 8,       // gemm128w_kernel (gemm128w.hip): four waves x 128 x 128 wave tiles on whole 256^2 tiles
};
constexpr int kNumVariants = 9;
inline const char *matmul_variant_name(int v) {
    static const char *const names[kNumVariants] = {"generic64",  "fast128_glds", "tile256", "tile256_splitk", "persist256",
                                                    "persist192", "persist128",   "fast32",  "wave128"};
    return (v >= 0 && v < kNumVariants) ? names[v] : "invalid";
}

// ---- the problem and the kernels' contracts ----------------------------------------------------------------------------------------
// Everything routing reads. A is [m][k] (akm: k contiguous) or [k][m]; B is [n][k] (bkm) or [k][n]; lda / ldb are the leading
// dimensions of the stored matrices in elements.
struct GemmProblem {
    int dtype;
    int64_t batch, m, n, k;
    bool akm, bkm;
    int64_t lda, ldb;
    int64_t a_bs, b_bs, c_bs; // batch strides in elements (0: shared operand); c_bs is m * n unless the caller groups separate outputs
    bool c_grouped;           // the caller gave c_bs itself (infini_rocm_matmul_grouped's stride_c != 0)
    bool bias;
    int64_t bias_m, bias_n;
    int act;
    int64_t hs_d;               // head-split store (GemmArgs::hs_d), 0 = off
    unsigned a_lo, b_lo, c_lo;  // the low four address bits of a, b, c
};
inline int64_t gemm_cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }
inline bool aligned16(uintptr_t addr) { return (addr & 15) == 0; }

// the 256-row family (gemm256.hip, gemm256p_kernel.h): whole 64-wide K-tiles, 16-byte DMA runs
inline bool gemm256_supported(const GemmProblem &q) {
    if (q.k % 64 != 0 || q.k < 64)
        return false;
    if (!aligned16(q.a_lo) || !aligned16(q.b_lo) || (q.a_bs % 8) || (q.b_bs % 8))
        return false;
    if (!q.akm && (q.m % 8 != 0 || q.m < 8))
        return false;
    if (!q.bkm && (q.n % 8 != 0 || q.n < 8))
        return false;
    if ((q.c_lo & 7) != 0)
        return false;
    // per-lane DMA offsets are 32-bit byte offsets inside one operand matrix
    if (q.m * q.k >= (1ll << 31) || q.n * q.k >= (1ll << 31))
        return false;
    return true;
}

inline bool fast128_supported(const GemmProblem &q) {
    if (q.k % 8 != 0 || q.k < 8) // 16-byte K runs; a K tail inside the last 64-wide tile is zero-filled
        return false;
    if (!aligned16(q.a_lo) || !aligned16(q.b_lo) || (q.a_bs % 8) || (q.b_bs % 8))
        return false;
    if (!q.akm && (q.m % 8 != 0 || q.m < 8))
        return false;
    if (!q.bkm && (q.n % 8 != 0 || q.n < 8))
        return false;
    if (!aligned16(q.c_lo) && (q.n % 4 == 0))
        return false;
    return true;
}

// A K-major with 16-byte rows; B K-major or N-major with 16-byte rows; K a multiple of 4 (a K tail inside the last
// 32-wide tile is zero-filled); the generic kernel serves the rest
inline bool fast32_supported(const GemmProblem &q) {
    if (!q.akm || q.k % 4 != 0 || q.k < 4 || q.m < 1 || q.n < 4)
        return false;
    if (!aligned16(q.a_lo) || !aligned16(q.b_lo) || (q.a_bs % 4) || (q.b_bs % 4) || (q.lda % 4))
        return false;
    if (q.ldb % 4 != 0 || (!q.bkm && q.n % 4 != 0))
        return false;
    return true;
}

// the four-wave kernel (gemm128w.hip): plain GEMMs on whole 256^2 tiles, K % 128 == 0
inline bool wave128_supported(const GemmProblem &q) {
    if (q.m <= 0 || q.n <= 0 || q.k < 128 || q.m % 256 || q.n % 256 || q.k % 128)
        return false;
    if (q.bias || q.act != 0 || q.hs_d != 0)
        return false;
    if (!aligned16(q.a_lo | q.b_lo | q.c_lo))
        return false;
    if ((q.a_bs % 8) || (q.b_bs % 8) || (q.c_bs % 8))
        return false;
    // per-lane piece offsets are 32-bit: 256 rows of the major index must stay below 4 GiB
    if (q.lda * 512 >= (1ll << 32) || q.ldb * 512 >= (1ll << 32) || q.n * 32 >= (1ll << 32))
        return false;
    if ((q.m / 256) * (q.n / 256) * q.batch >= (1ll << 31))
        return false;
    // the kernel keeps a lane's byte offset from the tile corner — the rows of its pieces PLUS the whole k advance of a tile — in 32 bits
    const int64_t a_max = q.akm ? (255 * q.lda + q.k + 64) * 2 : ((q.k + 32) * q.lda + 256) * 2;
    const int64_t b_max = q.bkm ? (255 * q.ldb + q.k + 64) * 2 : ((q.k + 32) * q.ldb + 256) * 2;
    return a_max < (1ll << 32) && b_max < (1ll << 32);
}

// sigmoid / tanh / erff-Gelu epilogues and biases other than one row vector live in the one-shot kernel, not the persistent ones
inline bool persist_epilogue_ok(const GemmProblem &q) {
    return (q.act == 0 || q.act == 1 || q.act == 5) && (!q.bias || (q.bias_m == 0 && q.bias_n == 1));
}

// ---- cost model -------------------------------------------------------------------------------------------------------------------
// Cost model behind the heuristic (microseconds; fitted to tools/gemm_shapes.py on MI355X, bf16 / f16, N(0,1) data).
// A workgroup of the persistent kernel walks its tiles: a K-tile of a 256 x 64 NT tile costs kKt[NT]; every tile pays its
// tile boundary (both wave rows' epilogues side by side + the pipeline restart; gemm256p_kernel.h); launch + first prologue
// ~3 us once. Re-fitted after the epilogues were de-serialised (round 2: ~12.4 k cycles per boundary) and again after their
// stores went quad-contiguous (round 3: ~7.9 k cycles; profiles/r03_gemm_shapes_bf16.txt).
constexpr double kKt[5] = {0, 0, 0.91, 1.10, 1.40};
constexpr double kStoreTail[5] = {0, 0, 4.2, 5.2, 5.5};
inline double persist_cost(long m, long n, long k, long batch, int nt, int cus) {
    const long tiles = gemm_cdiv(m, 256) * gemm_cdiv(n, 64 * nt) * batch;
    const long full = tiles / cus;
    const double frac = (double)(tiles - full * cus) / cus;
    // a partial last round still costs most of a tile time (every workgroup's tile takes what it takes; only the shared
    // L2 / HBM / power budget is lighter): 0.55 + 0.5 frac of a full round fits the sweep from frac = 0.25 to 0.8
    const double waves = (double)full + (frac > 0 ? (0.55 + 0.5 * frac < 1.0 ? 0.55 + 0.5 * frac : 1.0) : 0.0);
    return waves * ((double)(k / 64) * kKt[nt] + kStoreTail[nt]) + 3.0;
}
// split-K: `splits` workgroups per 256^2 tile write fp32 partial planes, one reduce pass adds them
inline double splitk_cost(long m, long n, long k, long batch, int splits) {
    return 3.0 + (double)(k / 64) / splits * kKt[4] + 12.0 + (double)batch * m * n * (4.0 * splits + 2.0) / 5.0e6;
}

// tile width (NT = 4 / 3 / 2 -> 256 / 192 / 128 columns) the cost model prefers for an m x n x k problem on the persistent
// kernels; max_nt caps it (the conv mode's residual copy exists up to NT = 3)
inline int persist_pick_nt(long m, long n, long k, int cus, int max_nt) {
    int best_nt = max_nt < 4 ? max_nt : 4;
    double best = 1e30;
    for (int nt = best_nt; nt >= 2; --nt) {
        const double c = persist_cost(m, n, k, 1, nt, cus);
        if (c < best * 0.97) {
            best = c;
            best_nt = nt;
        }
    }
    return best_nt;
}

// ---- split-K ----------------------------------------------------------------------------------------------------------------------
// split-K (the fp32 partial planes take the runtime workspace) needs few enough 256^2 tiles
inline bool gemm_splitk_tiles_fit(int64_t batch, int64_t m, int64_t n, int num_cu) {
    return gemm_cdiv(m, 256) * gemm_cdiv(n, 256) * batch * 2 <= num_cu + num_cu / 4;
}
// split-K factor for the 256^2 kernel: fill the CUs when the tiles alone cannot and K is long enough that every
// slice still runs >= 8 K-tiles (the fp32 partial planes cost 8 bytes per output element and slice). Below 2: no split.
inline int gemm_splitk_factor(const GemmProblem &q, int num_cu) {
    if (!gemm256_supported(q) || !gemm_splitk_tiles_fit(q.batch, q.m, q.n, num_cu))
        return 1;
    const int64_t by_tiles = num_cu / (gemm_cdiv(q.m, 256) * gemm_cdiv(q.n, 256) * q.batch), by_k = q.k / (8 * 64);
    const int64_t splits = by_tiles < by_k ? by_tiles : by_k;
    return (int)(splits < 16 ? splits : 16);
}
// The reduced-precision compute types of an fp32 MatMul always run the split-K form (its slices write raw fp32 sums), so their
// bounds are DIFFERENT on purpose: any tile count (one slice when the tiles fill the CUs), one slice per 512 of K, at least one.
inline int gemm_f32out_splits(const GemmProblem &q, int num_cu) {
    const int64_t by_tiles = num_cu / (gemm_cdiv(q.m, 256) * gemm_cdiv(q.n, 256) * q.batch), by_k = q.k / 512;
    const int64_t splits = by_tiles < by_k ? by_tiles : by_k;
    return (int)(splits < 1 ? 1 : splits < 16 ? splits : 16);
}

// ---- the plan ---------------------------------------------------------------------------------------------------------------------
struct GemmPlan {
    MatmulVariant variant;  // what runs, and what infini_rocm_matmul_last_variant reports
    int splits;             // kGemmTile256SplitK: workgroups per tile (before empty slices are dropped), 1 otherwise
    bool fast32_small;      // kGemmFast32: 64^2 tiles instead of 128^2
    bool reduced_precision; // fp32 operands cast (or split into bf16 pieces) in the workspace, the split-K kernel with fp32 output
};

// MatmulObj::getComputeType() 1 "bf16" / 2 "fp16" on an fp32 MatMul: 16-bit copies of A and B in the workspace, the 256^2 split-K
// kernel (raw fp32 slice sums), fp32 output. Shapes it cannot serve (K % 64, alignment, a head-split or grouped output) keep the exact
// kernels: never LESS accurate than asked.
// (batch strides: the casts copy (stride ? batch : 1) CONTIGUOUS blocks of m * k (n * k) elements, so the path is taken only
// for operands that ARE such blocks — stride 0 (shared) or exactly one block; any other stride keeps the exact kernels.
// Round-4 advisor: with another stride the cast read the wrong rows and the kernel indexed the 16-bit copy past its end.)
//
// 3 "bf16x3" / 4 "bf16x6": every fp32 value is written as a sum of two / three bf16 pieces (split.hip) and the cross products that
// matter are laid SIDE BY SIDE ALONG K — A' = [A_p | ...], B' = [B_q | ...], one plane per term, K' = terms * K — so one launch of the
// same bf16 kernel sums them all (and its split-K gets terms x more K to cut). Term t multiplies piece kSplitPieceA[t] of A with piece
// kSplitPieceB[t] of B (piece 0 = the bf16 rounding, 1 and 2 the roundings of what is left): x3 drops only lo * lo, x6 has every pair
// with i + j <= 2; the small products come first. The two tables are a PAIR: the same t must name one product on both sides.
constexpr int kComputeTypes = 5; // 0 default / tf32, 1 bf16, 2 fp16, 3 bf16x3, 4 bf16x6
constexpr int kSplitMaxTerms = 6;
constexpr int kSplitPieceA[2][kSplitMaxTerms] = {{1, 0, 0, 0, 0, 0}, {1, 2, 0, 1, 0, 0}};
constexpr int kSplitPieceB[2][kSplitMaxTerms] = {{0, 1, 0, 0, 0, 0}, {1, 0, 2, 0, 1, 0}};
inline int gemm_split_terms(int compute_type) { return compute_type == 3 ? 3 : compute_type == 4 ? 6 : 1; }

// The 16-bit problem the reduced-precision path hands to the 256^2 kernel: copies 256-byte aligned in the workspace, dense blocks,
// K' = terms * K with the leading dimension of a K-major operand growing with it.
inline GemmProblem gemm_reduced_problem(const GemmProblem &q, int compute_type) {
    const int64_t terms = gemm_split_terms(compute_type);
    GemmProblem q16 = q;
    q16.k = terms * q.k;
    q16.lda = q.akm ? q16.k : q.m;
    q16.ldb = q.bkm ? q16.k : q.n;
    q16.a_lo = q16.b_lo = 0;
    q16.a_bs = (q.a_bs == 0 || q.batch == 1) ? 0 : q.m * q16.k;
    q16.b_bs = (q.b_bs == 0 || q.batch == 1) ? 0 : q.n * q16.k;
    return q16;
}
inline bool gemm_reduced_precision_ok(const GemmProblem &q, int compute_type) {
    if (q.dtype != INFINI_DT_F32 || compute_type == 0 || q.hs_d != 0 || q.c_grouped)
        return false;
    if (q.batch != 1 && !((q.a_bs == 0 || q.a_bs == q.m * q.k) && (q.b_bs == 0 || q.b_bs == q.n * q.k)))
        return false;
    // the split kernel reads its fp32 source in 16-byte runs (the casts of 1 / 2 take any address)
    if (compute_type >= 3 && !(aligned16(q.a_lo) && aligned16(q.b_lo)))
        return false;
    // whole K-tiles of the ORIGINAL K too: K' % 64 == 0 alone would let a plane boundary fall inside a K-tile — harmless for the sums,
    // but the contract stays the one of the 16-bit types
    if (q.k % 64 != 0)
        return false;
    return gemm256_supported(gemm_reduced_problem(q, compute_type)) && aligned16(q.c_lo);
}

// `forced`: the runtime's variant (kGemmHeuristic or a kernel). A forced kernel that cannot serve the problem falls back the way the
// heuristic's last step does (fast128, then generic); wave128 outside its contract and fast32 on 16-bit operands go back to the heuristic.
inline GemmPlan gemm_plan(const GemmProblem &q, int forced, int compute_type, int num_cu) {
    GemmPlan pl = {kGemmGeneric64, 1, false, false};
    if (gemm_reduced_precision_ok(q, compute_type)) {
        pl.variant = kGemmTile256SplitK;
        pl.splits = gemm_f32out_splits(gemm_reduced_problem(q, compute_type), num_cu);
        pl.reduced_precision = true;
        return pl;
    }
    if (q.dtype == INFINI_DT_F32) {
        // fp32: the LDS-DMA tile kernel (gemm32.hip; 128^2 or 64^2 tiles) when it can serve the operands and the problem has
        // at least 16 tiles of 64^2 (or it is forced); the generic register-staged 64^2 kernel otherwise
        const bool want = forced == kGemmFast32 || (forced < 0 && gemm_cdiv(q.m, 64) * gemm_cdiv(q.n, 64) * q.batch >= 16 && q.k >= 64);
        if (want && fast32_supported(q)) {
            pl.variant = kGemmFast32;
            // 128^2 tiles when they give at least ~half a tile per CU, 64^2 tiles otherwise (512^3: 64 tiles)
            pl.fast32_small = gemm_cdiv(q.m, 128) * gemm_cdiv(q.n, 128) * q.batch * 2 < num_cu;
        }
        return pl;
    }
    int variant = forced;
    if (variant == kGemmFast32 || (variant == kGemmWave128 && !wave128_supported(q)))
        variant = kGemmHeuristic;
    const bool ok256 = gemm256_supported(q), ok128 = fast128_supported(q);
    const int splits = gemm_splitk_factor(q, num_cu);
    if (variant < 0) {
        // heuristic: the cheapest of {persistent 256 / 192 / 128-wide tiles, split-K} by the cost model when the 256-row
        // kernels can serve the problem and it has at least ~half a tile per CU; otherwise 128^2 tiles; otherwise generic
        double best = 1e30;
        if (ok256) {
            for (int nt = 4; nt >= 2; --nt) {
                if (gemm_cdiv(q.m, 256) * gemm_cdiv(q.n, 64 * nt) * q.batch * 2 < num_cu)
                    continue;
                const double c = persist_cost(q.m, q.n, q.k, q.batch, nt, num_cu);
                if (c < best * 0.97) { // prefer the wider tile unless a narrower one is clearly cheaper
                    best = c;
                    variant = kGemmPersist256 + (4 - nt);
                }
            }
            if (splits >= 2 && splitk_cost(q.m, q.n, q.k, q.batch, splits) < best * 0.97)
                variant = kGemmTile256SplitK;
        }
        // the four-wave kernel (gemm128w.hip) where it measured ahead of persist256 (profiles/r06_gemm_wave128_ab.txt: + 2-8 %): plain
        // single-batch GEMMs of one or two rounds of whole 256^2 tiles with a long K, any layout but NT (both operands K-major: - 3.5 %)
        const int64_t tiles256 = gemm_cdiv(q.m, 256) * gemm_cdiv(q.n, 256) * q.batch;
        if (variant == kGemmPersist256 && q.batch == 1 && q.k >= 2048 && !(q.akm && q.bkm) && tiles256 >= num_cu && tiles256 <= 2l * num_cu &&
            wave128_supported(q))
            variant = kGemmWave128;
        if (variant < 0)
            variant = ok128 ? kGemmFast128 : kGemmGeneric64;
    } else if (variant >= kGemmTile256 && !ok256) {
        variant = ok128 ? kGemmFast128 : kGemmGeneric64;
    } else if (variant == kGemmFast128 && !ok128) {
        variant = kGemmGeneric64;
    }
    if (variant >= kGemmPersist256 && variant <= kGemmPersist128 && !persist_epilogue_ok(q))
        variant = kGemmTile256;
    pl.variant = (MatmulVariant)variant;
    if (variant == kGemmTile256SplitK)
        pl.splits = splits < 2 ? 2 : splits; // forced on a problem the factor would not split: two slices
    return pl;
}

} // namespace irocm
