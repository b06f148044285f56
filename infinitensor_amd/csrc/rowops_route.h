// Row-operator routing: which kernel of rowops.hip serves a Softmax, LayerNorm, RMSNorm or (bias_)add_norm call, with which template
// choices and on what grid. Host code only, plain C++17: no HIP call, no runtime object — rowop_plan is a pure function of the problem,
// the two grid hooks and the CU count, so infini_rocm_rowop_plan_route (and the CPU tests) can ask it without a GPU. rowops.hip
// validates, fills RowopProblem, asks rowop_plan and launches what it says; every threshold of the dispatch is written here, once.
#pragma once
#include "infini_rocm.h"
#include <cstdint>
#include <cstdio>
#include <cstdlib>

namespace irocm {

enum RowopOp : int { kRowopSoftmax = 0, kRowopLayerNorm = 1, kRowopRmsNorm = 2, kRowopAddNorm = 3 }; // infini_rocm_rowop_plan_route's `op`
constexpr int kNumRowopOps = 4;

// Everything routing reads. The tensor is [outer][n][inner]; only Softmax has inner != 1.
struct RowopProblem {
    RowopOp op;
    int dtype; // INFINI_DT_F32 / F16 / BF16 (the caller has checked)
    int64_t outer, n, inner;
    bool has_pre; // add_norm: a row `pre` is added first (bias_add_norm)
    unsigned lo;  // the OR of the low four address bits of every non-null pointer the op touches
};

// ---- environment switches, read once per process --------------------------------------------------------
struct RowopHooks {
    int norm_blocks_per_cu;   // IROCM_NORM_BLOCKS_PER_CU    4  norm_rows_kernel: 16 persistent waves per CU, rows pipelined
    int rowops_blocks_per_cu; // IROCM_ROWOPS_BLOCKS_PER_CU  0  > 0: the wave kernels take this many workgroups per CU, not the resident count
};
inline RowopHooks rowop_hooks() {
    static const RowopHooks once = [] {
        const char *norm = getenv("IROCM_NORM_BLOCKS_PER_CU"), *rows = getenv("IROCM_ROWOPS_BLOCKS_PER_CU");
        return RowopHooks{norm ? atoi(norm) : 4, rows ? atoi(rows) : 0};
    }();
    return once;
}

// ---- the plan -----------------------------------------------------------------------------------------------------------------------
enum RowopKernel : int {
    kRowopNone,            // a zero extent: nothing runs
    kRowopSoftmaxWave,     // softmax_wave_kernel<T, C, aligned, R>: a row in the registers of one wave, R rows per wave
    kRowopSoftmaxBlockreg, // softmax_blockreg_kernel<T, C>: a row in the registers of one 256-thread block
    kRowopSoftmaxBlock,    // softmax_block_kernel<T>: any length and alignment, three passes
    kRowopSoftmaxStrided,  // softmax_strided_kernel<T>: inner != 1
    kRowopNormRows,        // norm_rows_kernel<T, B, C, RMS, 1, ADD>: aligned rows up to 4 KiB
    kRowopNormWave,        // norm_wave_kernel<T, C, false, RMS, 1>
    kRowopNormBlockreg,    // norm_blockreg_kernel<T, C, RMS, ADD>
    kRowopNormBlock,       // norm_block_kernel<T, RMS>
    kRowopChain,           // add_norm outside the fused kernels' reach: the caller runs Add, then the norm
};
// The persistent grid is min(work, cap) workgroups of 256 threads, cap by one of four policies:
enum RowopGrid : int {
    kGridResident, // CUs x the workgroups of THIS kernel resident on a CU, asked from the HIP runtime at the launch (cap = 0 here)
    kGridPerCu,    // CUs x a hook's count
    kGrid8192,     // one row per workgroup and trip
    kGrid16384,    // 256 (outer, inner) pairs per workgroup and trip
};
struct RowopPlan {
    RowopKernel kernel;
    int B, C;     // chunk bytes per lane (norm_rows only: 8 or 16) and chunks per lane (per thread for the block-resident kernels)
    bool aligned; // THE alignment predicate: every pointer on 16 bytes and whole 16-byte vectors in a row
    int R;        // rows per wave
    int add;      // ADD: 0 none, 1 a + b, 2 (a + pre) + b
    int64_t work; // workgroups the rows need
    RowopGrid grid;
    int64_t cap;
};
inline int64_t rowop_cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }
inline unsigned rowop_grid(const RowopPlan &pl, int64_t cap) { return (unsigned)(pl.work < cap ? pl.work : cap); }

inline RowopPlan rowop_plan(const RowopProblem &q, const RowopHooks &hk, int num_cu) {
    RowopPlan pl = {kRowopNone, 16, 1, false, 1, 0, 0, kGrid8192, 8192};
    if (q.outer == 0 || q.n == 0 || q.inner == 0)
        return pl;
    const int64_t esize = q.dtype == INFINI_DT_F32 ? 4 : 2, vec = 16 / esize, row_bytes = q.n * esize;
    const bool al = pl.aligned = (q.lo & 15) == 0 && q.n % vec == 0;
    const int64_t chunks = rowop_cdiv(q.n, 64 * vec); // 16-byte chunks per lane of a wave-resident row
    const int64_t bch = rowop_cdiv(q.n, 256 * vec);   // ... per thread of a block-resident row
    const auto ladder = [](int64_t c, int lowest) { return c <= lowest ? lowest : c <= 2 ? 2 : c <= 4 ? 4 : 8; };
    const auto wave = [&](RowopKernel k, int c, int rows) { // four waves of `rows` rows per workgroup
        pl.kernel = k, pl.C = c, pl.R = rows, pl.work = rowop_cdiv(q.outer, 4 * rows);
        pl.grid = hk.rowops_blocks_per_cu > 0 ? kGridPerCu : kGridResident;
        pl.cap = hk.rowops_blocks_per_cu > 0 ? (int64_t)num_cu * hk.rowops_blocks_per_cu : 0;
    };
    const auto block = [&](RowopKernel k, int c) { pl.kernel = k, pl.C = c, pl.work = q.outer; };

    if (q.op == kRowopSoftmax) {
        if (q.inner != 1) {
            pl.kernel = kRowopSoftmaxStrided, pl.aligned = false, pl.work = rowop_cdiv(q.outer * q.inner, 256);
            pl.grid = kGrid16384, pl.cap = 16384;
        } else if (chunks <= 8) {
            // rows per wave: ~4 KiB of loads in flight per wave, once there are rows enough; built for one and two chunks
            const int c = ladder(chunks, 1);
            wave(kRowopSoftmaxWave, c, (al && q.outer >= 4096 && c <= 2) ? (row_bytes <= 1024 ? 4 : row_bytes <= 3072 ? 2 : 1) : 1);
        } else if (al && bch <= 8) {
            block(kRowopSoftmaxBlockreg, ladder(bch, 4));
        } else {
            block(kRowopSoftmaxBlock, 1);
        }
        return pl;
    }
    pl.add = q.op == kRowopAddNorm ? (q.has_pre ? 2 : 1) : 0;
    if (al && row_bytes <= 4096) {
        // chunk width: the one that leaves the fewest idle lanes (768 f16 = 3 x 8 B, not 2 x 16 B with half a chunk idle)
        const int64_t c16 = rowop_cdiv(row_bytes, 1024), c8 = rowop_cdiv(row_bytes, 512);
        const bool use8 = (c8 == 1 || c8 == 3) && (c8 * 512 - row_bytes) < (c16 * 1024 - row_bytes);
        pl.kernel = kRowopNormRows, pl.B = use8 ? 8 : 16, pl.C = (int)(use8 ? c8 : c16), pl.work = rowop_cdiv(q.outer, 4);
        pl.grid = kGridPerCu, pl.cap = (int64_t)num_cu * hk.norm_blocks_per_cu;
    } else if (!pl.add && chunks <= 4) {
        wave(kRowopNormWave, ladder(chunks, 1), 1); // (unaligned by now: aligned rows this short are norm_rows')
    } else if (al && bch <= 8) {
        block(kRowopNormBlockreg, ladder(bch, 2)); // up to 256 threads x 8 chunks x 16 B = 32 KiB
    } else if (!pl.add) {
        block(kRowopNormBlock, 1);
    } else {
        pl.kernel = kRowopChain;
    }
    return pl;
}

// What infini_rocm_rowop_last_route / _plan_route report, in the grammar of tests/rowop_cases.py's route().
constexpr size_t kRowopRouteCap = 40;
inline void rowop_route_name(const RowopPlan &pl, char *buf, size_t cap) {
    const char *how = pl.aligned ? "aligned" : "unaligned";
    switch (pl.kernel) {
    case kRowopSoftmaxWave: snprintf(buf, cap, "softmax_wave/C%d/%s/R%d", pl.C, how, pl.R); break;
    case kRowopSoftmaxBlockreg: snprintf(buf, cap, "softmax_blockreg/C%d", pl.C); break;
    case kRowopSoftmaxBlock: snprintf(buf, cap, "softmax_block/%s", how); break;
    case kRowopSoftmaxStrided: snprintf(buf, cap, "softmax_strided"); break;
    case kRowopNormRows: snprintf(buf, cap, "norm_rows/B%d/C%d/ADD%d", pl.B, pl.C, pl.add); break;
    case kRowopNormWave: snprintf(buf, cap, "norm_wave/C%d/%s/R%d", pl.C, how, pl.R); break;
    case kRowopNormBlockreg: snprintf(buf, cap, "norm_blockreg/C%d/ADD%d", pl.C, pl.add); break;
    case kRowopNormBlock: snprintf(buf, cap, "norm_block/%s", how); break;
    case kRowopChain: snprintf(buf, cap, "chain"); break;
    default: snprintf(buf, cap, "none"); break;
    }
}

} // namespace irocm
