// Conv2d routing: which kernel serves which layer. Host code only, plain C++17: no HIP call, no runtime object — the planner is a pure
// function of the problem, the variant, the CU count and the environment switches, so infini_rocm_conv2d_plan_route (and the CPU tests)
// can ask it without a GPU. conv.hip walks conv_plan's candidates; conv_s1.hip launches the ConvS1Plan. The planner assumes that the
// pointers it cannot see qualify: alignment, 32-bit offset limits and hipMemGetAddressRange stay in the launchers, which return -1
// ("declined") — the dispatcher then takes the next candidate.
#pragma once
#include "diag.h"
#include "infini_rocm.h"
#include <cstddef>
#include <cstdint>
#include <cstdlib>

namespace irocm {

// infini_rocm_conv2d_set_variant's argument (include/infini_rocm.h)
enum ConvVariant : int {
    kConvHeuristic = -1,    // the measured rules below
    kConvNoPersistent = 0,  // the heuristic without the persistent-kernel routes (pixel-slot GEMM, tap GEMM): the round-2 routing
    kConvGeneric = 1,       // conv_igemm16 (f16 / bf16) / conv_direct32 (f32) only
    kConvS1 = 2,            // the conv_s1.hip kernels for every shape they serve
    kConvBatchedGemm = 3,   // the batched-GEMM route for every eligible pointwise shape
    kConvTapShifted = 4,    // = 2 with the patch and resident kernels off
    kConvPixelGemm = 5,     // pointwise layers as one GEMM over pixel slots wherever they qualify
    kConvPatchWide = 6,     // = 2 with the 8-wave 128 x 256 patch kernel wherever it serves
    kConvTapGemm = 7,       // 3 x 3 / pad 1 layers as one GEMM with K = 9 C wherever they qualify
};

// what infini_rocm_conv2d_last_route reports
enum ConvRoute : int {
    kRouteNone, kRouteIgemm32, kRouteIgemm32SplitK, kRouteBatchedGemm32, kRouteDirect32, kRouteDepthwise, kRoutePixelGemm, kRouteTapGemm,
    kRouteTapGemmSplitK, kRouteTapShifted, kRouteResident, kRouteBatchedGemm, kRouteGeneric, kRouteStemPool,
};
inline const char *conv_route_name(ConvRoute r) {
    static const char *const names[] = {"none", "igemm32", "igemm32_splitk", "batched_gemm32", "direct32", "depthwise", "pixel_gemm", "tap_gemm",
                                        "tap_gemm_splitk", "tap_shifted", "resident", "batched_gemm", "generic", "stem_pool"};
    return names[r];
}

// the kernel of conv_s1.hip behind "tap_shifted" / "resident"
enum ConvForm : int { kFormNone, kFormPw, kFormRowtap, kFormPatchWide, kFormPatch, kFormResident, kFormS1_1_4_32, kFormS1_2_2_32, kFormS1_2_2_64 };
inline const char *conv_form_name(ConvForm f) {
    static const char *const names[] = {"", "pw", "rowtap", "patch_wide", "patch", "resident", "s1<1,4,32>", "s1<2,2,32>", "s1<2,2,64>"};
    return names[f];
}

// ---- environment switches -----------------------------------------------------------------------------
inline int env_int(const char *name, int dflt) {
    const char *e = getenv(name);
    return e ? atoi(e) : dflt;
}
struct ConvHooks {
    // read once per process (A/B and tuning hooks of tools/conv_bench.py: one setting per run)
    int pw;         // IROCM_CONV_PW          1    conv_pw_kernel: 0 off, 1 up to 128 channels, 2 up to 256 and ahead of the one-K-step rule
    int wide;       // IROCM_CONV_WIDE        2    LDS-staged epilogue: 0 off, 1 even planes only, 2 all (9: device-side ablation)
    int epi_probe;  // IROCM_CONV_EPI_PROBE   0    device-side ablation of the epilogue: diagnostic build only, 0 in the shipped library
    int tap;        // IROCM_CONV_TAP         1    0: the heuristic never takes the tap GEMM
    int patch;      // IROCM_CONV_PATCH       1    0: no patch / resident kernels
    int patch_wide; // IROCM_CONV_PATCH_WIDE  -1   0 / 1 force the 4-wave / 8-wave patch kernel
    int resident;   // IROCM_CONV_RESIDENT    1    0: no resident kernel
    int cfg;        // IROCM_CONV_CFG         0    1: s1<2,2,32> where s1<2,2,64> would run
    int res_nt4;    // IROCM_CONV_RES_NT4     1    0: the pixel-slot GEMM with a residual stays on <= 192-column tiles
    // read per call (tests set them with monkeypatch)
    int pw_nt;              // IROCM_CONV_PW_NT         0  2 / 3 / 4 force the pixel-slot GEMM's tile width
    int tap_split;          // IROCM_CONV_TAP_SPLIT     0  1 = never split, 2 / 4 = only that factor
    int tap_nt;             // IROCM_CONV_TAP_NT        0  2 / 3 / 4 force the tap GEMM's tile width (unsplit)
    int conv32_tile;        // IROCM_CONV32_TILE        0  1 = 64^2 tiles, 2 = 128^2
    int conv32_split;       // IROCM_CONV32_SPLIT       0  1 = never, 2 / 4 = that factor wherever a slice keeps >= 2 K-tiles
    bool conv32_pw_batched; // IROCM_CONV32_PW_BATCHED  set (to anything): fp32 unit-stride pointwise layers as one GEMM per image
};
inline ConvHooks conv_hooks() {
    static const char *const probe = diag_getenv("IROCM_CONV_EPI_PROBE"); // (diagnostic build only: diag.h; 2 = no global stores)
    static const ConvHooks once = {env_int("IROCM_CONV_PW", 1),    env_int("IROCM_CONV_WIDE", 2),        probe ? atoi(probe) : 0,
                                   env_int("IROCM_CONV_TAP", 1),   env_int("IROCM_CONV_PATCH", 1),       env_int("IROCM_CONV_PATCH_WIDE", -1),
                                   env_int("IROCM_CONV_RESIDENT", 1), env_int("IROCM_CONV_CFG", 0),      env_int("IROCM_CONV_RES_NT4", 1),
                                   0, 0, 0, 0, 0, false};
    ConvHooks h = once;
    h.pw_nt = env_int("IROCM_CONV_PW_NT", 0);
    h.tap_split = env_int("IROCM_CONV_TAP_SPLIT", 0);
    h.tap_nt = env_int("IROCM_CONV_TAP_NT", 0);
    h.conv32_tile = env_int("IROCM_CONV32_TILE", 0);
    h.conv32_split = env_int("IROCM_CONV32_SPLIT", 0);
    h.conv32_pw_batched = getenv("IROCM_CONV32_PW_BATCHED") != nullptr;
    return h;
}

// ---- the problem and its shape predicates -----------------------------------------------------------------------------------------
struct ConvProblem {
    int64_t n, c, h, w, f;
    int r, s, ph, pw, sh, sw, dh, dw;
    int64_t groups;
    int oh, ow; // reference output size: src/operators/conv.cc:98-101
    int act;
    bool residual;
    int64_t npix() const { return (int64_t)oh * ow; }
    int64_t npix8() const { return (npix() + 7) / 8 * 8; } // a plane in pixel slots: rounded up to a 16-byte run
};
inline int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

inline bool conv_1x1(const ConvProblem &q) { return q.r == 1 && q.s == 1 && q.ph == 0 && q.pw == 0; }
inline bool conv_unit_stride(const ConvProblem &q) { return q.sh == 1 && q.sw == 1; }
// unit stride, no dilation, one group, output plane == input plane
inline bool conv_same_s1(const ConvProblem &q) {
    return conv_unit_stride(q) && q.dh == 1 && q.dw == 1 && q.groups == 1 && q.oh == q.h && q.ow == q.w;
}

// depthwise (conv_dw.hip): groups == C, one input channel per filter; 3 x 3 / 5 x 5, stride 1 / 2, any channel multiplier
inline bool conv_dw_window(int r, int s, int sh, int sw, int64_t f, int64_t c) {
    return ((r == 3 && s == 3) || (r == 5 && s == 5)) && (sh == 1 || sh == 2) && sh == sw && f % c == 0;
}
inline bool conv_depthwise_shape(const ConvProblem &q) {
    return q.groups == q.c && q.groups > 1 && q.dh == 1 && q.dw == 1 && !q.residual && conv_dw_window(q.r, q.s, q.sh, q.sw, q.f, q.c);
}

// Pixel-slot GEMM (gemm256p_conv.hip): a pointwise layer is ONE GEMM  Y[f][slot] = W[f][c] X[c][slot]  over pixel slots (image, pixel) on
// the persistent 256-row kernels in conv mode (gemm256p_kernel.h, CONV): LDS-DMA staging of both operands, tiles that span images
// (14 x 14 and 7 x 7 planes do not waste tiles), per-filter bias, residual and activation in the epilogue, NCHW stores. As plain GEMMs
// these layers run 1.2-1.8 x faster on that machinery than on the register-staged tap-shifted kernel (tools/probes/conv_as_gemm.py,
// profiles/r03_conv_as_gemm.txt). The layer is either unit-stride (the dispatcher's candidate) or a strided 1 x 1 whose single phase
// plane conv_s1.hip has just written as a dense [n][c][oh][ow] activation (ResNet's down-sampling branches).
inline bool conv_pixel_gemm_shape(const ConvProblem &q) {
    return conv_1x1(q) && q.groups == 1 && q.dh == 1 && q.dw == 1 && q.c % 64 == 0 && (q.act == 0 || q.act == 1);
}
// Fill rule: >= 128 filters (C256->F128 @56x56 78 vs 100 us, C512->F128 @28x28 33 vs 40; with 64 the 256-row tile is 3/4 empty: 69 vs 60
// us). The grid may be thin — C1024->F256 @14x14 is 100 tiles of 256^2 and still 22.6 vs 31.1 us, C2048->F512 @7x7 50 tiles and 38.8 vs
// 45.1 — but below ~3/16 of the CUs the 128 x 128 tiles of the tap-shifted kernel spread better.
inline bool conv_pixel_gemm_fills(const ConvProblem &q, int num_cu) {
    return q.f >= 128 && cdiv(q.f, 256) * cdiv(q.n * q.npix8(), 256) * 16 >= (int64_t)num_cu * 3;
}
inline bool conv_pixel_gemm_wanted(const ConvProblem &q, int variant, int num_cu) {
    return conv_pixel_gemm_shape(q) && (variant == kConvPixelGemm || (variant < 0 && conv_pixel_gemm_fills(q, num_cu)));
}

// Tap GEMM (gemm256p_conv3.hip): 3 x 3 / pad 1 layers of stride 1 or 2 as ONE GEMM with K = 9 C on the persistent 256-row kernels
// (gemm256p_kernel.h, CONV = 3: TAP mode).
inline bool conv_tap_shape(const ConvProblem &q) {
    return q.r == 3 && q.s == 3 && q.ph == 1 && q.pw == 1 && q.dh == 1 && q.dw == 1 && ((q.sh == 1 && q.sw == 1) || (q.sh == 2 && q.sw == 2)) &&
           q.c % 64 == 0 && !q.residual && (q.act == 0 || q.act == 1) && q.npix() >= 8;
}
// Split-K of the tap GEMM: how many workgroups share one 256 x 256 tile (1 = no split) and the bytes of the fp32 exchange slab the
// caller has to provide. The split form runs ONE unit per workgroup (grid <= CUs: every slice of every tile resident at once), so
// it is taken only when the 256 x 256 tiles number less than half the CUs — ResNet-50 at batch 128: 100 tiles (14 x 14 planes, F 256)
// -> 2 slices of 18 K-tiles, 56 tiles (7 x 7, F 512) -> 4 slices of 18. `flag_words`: capacity of the runtime's hand-off flag array;
// `forced`: IROCM_CONV_TAP_SPLIT.
inline int conv_tap_split(int64_t n, int64_t hw, int64_t c, int64_t f, int num_cu, int64_t flag_words, int forced, size_t *slab_bytes = nullptr) {
    const int64_t hwp = (hw + 7) & ~(int64_t)7;
    const int64_t tiles = cdiv(f, 256) * cdiv(n * hwp, 256);
    const int64_t nk = 9 * (c / 64);
    const int cus = num_cu >= 8 ? (num_cu / 8) * 8 : num_cu;
    int split = 1;
    for (int s : {4, 2}) {
        // every slice keeps >= 9 K-tiles (one channel block's taps); the flag words of all (tile, source, destination, wave) fit
        if (nk % s == 0 && nk / s >= 9 && cdiv(tiles, 8) * 8 * s <= cus && tiles * s * s * 8 <= flag_words && (forced == 0 || forced == s)) {
            split = s;
            break;
        }
    }
    if (forced == 1)
        split = 1;
    if (slab_bytes)
        *slab_bytes = split > 1 ? (size_t)tiles * split * 8 * 8 * 4 * 1024 : 0;
    return split;
}
// Conv variant 7 forces the tap GEMM for every eligible shape (tests, tune(), tools/conv_bench.py). Default routing by measurement
// (batch 128, f16, us; tools/conv_bench.py on three boxes):
//   strided layers (the tap-shifted kernel on phase planes was their only kernel): C256 28 x 28 / 2 -> 74-77 vs 87-92,
//     C512 14 x 14 / 2 -> 78-82 vs 115-120 (split-K x 4): taken from 128 filters on — half of the 256-row tile is empty there, and the
//     tap GEMM still wins (C128 -> 128 @56^2 / 2: 98.2 vs 104.7 us) — when there is enough work for the persistent kernels at all;
//   unit-stride layers need 256 filters and compete with the patch kernels: C512 7 x 7 (56 tiles, split-K x 4) 58-61 vs 69-73: taken;
//     C256 14 x 14 (100 tiles, split-K x 2) 51-57 vs 49.5: not taken — i.e. only where the tiles are so few that the split is by four.
inline bool conv_tap_wanted(const ConvProblem &q, int variant, int num_cu, const ConvHooks &hk, int64_t flag_words) {
    if (!conv_tap_shape(q))
        return false;
    if (variant == kConvTapGemm)
        return true;
    if (variant >= 0 || !hk.tap || !(q.f >= 256 || (q.sh == 2 && q.f >= 128)))
        return false;
    if (q.sh == 2)
        return cdiv(q.f, 256) * cdiv(q.n * q.npix8(), 256) * 4 >= num_cu / 2;
    return conv_tap_split(q.n, q.npix(), q.c, q.f, num_cu, flag_words, hk.tap_split) >= 4;
}

// conv_pw_kernel (conv_s1.hip), measured with tools/conv_bench.py: with <= 128 input channels it wins everywhere (C64->F256 @56x56 64 vs
// 89 us generic, C128->F512 @28x28 44 vs 59 us conv_s1); at C = 256 its 100 KiB of LDS leaves one workgroup per CU and it loses
// (IROCM_CONV_PW=2 sends those there too)
inline bool conv_pw_kernel_shape(const ConvProblem &q, const ConvHooks &hk) {
    return hk.pw >= 1 && conv_1x1(q) && q.groups == 1 && q.c % 64 == 0 && q.c <= (hk.pw == 2 ? 256 : 128) && q.f > 64 && q.npix() % 2 == 0;
}
// a single K-step leaves nothing to pipeline: the small generic tile (more workgroups per CU) hides the latency better
inline bool conv_one_kstep(const ConvProblem &q) { return q.c * q.r * q.s <= 64 && q.f >= 128; }

// pointwise convolution == batched GEMM  Y[n] = W[F x C] . X[n][C x HW]  (A broadcast over batch) on the LDS-DMA kernels
inline bool conv_batched_gemm_shape(const ConvProblem &q) { return conv_1x1(q) && conv_same_s1(q) && q.npix() % 8 == 0 && q.c % 64 == 0; }
// ... by default only for long-K layers on big planes without a residual: with K <= 512 its 256^2 tiles run 8 K-tiles each and the
// per-tile prologue + epilogue dominates (C512->F256 @28x28: 88 us vs 66 us on conv_s1)
inline bool conv_batched_gemm_first(const ConvProblem &q, int variant) {
    if (!conv_batched_gemm_shape(q))
        return false;
    if (variant == kConvBatchedGemm)
        return true;
    return !(variant == kConvS1 || variant == kConvTapShifted || variant == kConvPatchWide || variant == kConvTapGemm) && !q.residual &&
           q.f >= 256 && q.c >= 1024 && q.npix() >= 2048;
}

// ---- the conv_s1.hip family -------------------------------------------------------------------------------------------------------
// what launch_conv_s1 serves at all: windows up to 7 x 7, an output extent of ceil(input / stride) (phase planes), at most 16 phases,
// a per-k LDS table of 2048 entries for channel counts that are not a multiple of 32 (ROWTAP)
inline bool conv_s1_shape(const ConvProblem &q) {
    if (q.groups != 1 || q.r > 7 || q.s > 7 || q.sh * q.sw > 16 || q.oh != (q.h + q.sh - 1) / q.sh || q.ow != (q.w + q.sw - 1) / q.sw)
        return false;
    if (q.c % 32 != 0 && ((q.c * q.r * q.s + 31) & ~(int64_t)31) > 2048)
        return false;
    return q.n * q.npix8() < (1ll << 31);
}
struct ConvS1Plan {
    bool pixel_gemm; // strided pointwise layer: continue on the pixel-slot GEMM after the phase split
    bool tap;        // the tap GEMM (on the input, or on the four phase planes of a stride-2 layer)
    int tap_split;   // its split-K factor
    size_t tap_slab_bytes;
    ConvForm form;   // the conv_s1.hip kernel that runs when neither is taken (or both decline)
    int halo8;       // patch / resident forms: elements a tap reaches in front of a slot run, rounded up to 8
};
inline ConvS1Plan conv_s1_plan(const ConvProblem &q, int variant, int num_cu, const ConvHooks &hk, int64_t flag_words) {
    ConvS1Plan pl = {false, false, 1, 0, kFormNone, 0};
    const bool split = q.sh * q.sw > 1;
    pl.pixel_gemm = split && conv_pixel_gemm_wanted(q, variant, num_cu);
    pl.tap = conv_tap_wanted(q, variant, num_cu, hk, flag_words);
    if (pl.tap)
        pl.tap_split = conv_tap_split(q.n, q.npix(), q.c, q.f, num_cu, flag_words, hk.tap_split, &pl.tap_slab_bytes);
    if (conv_pw_kernel_shape(q, hk)) {
        pl.form = kFormPw;
    } else if (q.c % 32 != 0) {
        pl.form = kFormRowtap;
    } else if (hk.patch && q.r * q.s > 1 && q.r * q.s <= 32 && !split && q.dh == 1 && q.dw == 1 && q.oh == q.h && q.ow == q.w && 2 * q.ph == q.r - 1 &&
               2 * q.pw == q.s - 1 && variant != kConvTapShifted) {
        // unit-stride "same" R x S (the 3x3 layers): input patch resident in LDS, every tap an aligned row offset
        pl.halo8 = (int)((q.ph * q.w + q.pw + 7) & ~(int64_t)7);
        if (q.f > 64 && 2 * pl.halo8 <= 128) {
            // 128 f x 128 slots. (The 64 f x 256 slots form of the same kernel, <1, 4>, was measured on ResNet's C64 -> F64 56x56 layers —
            // two channel blocks, 18 taps per workgroup: 119 us against 96 us for the tap-shifted kernel, whose 64 x 256 x 32 tile has
            // no patch / transpose prologue to amortise — and is not instantiated.)
            // 128 f x 256 slots on 8 waves (one workgroup per CU, three weight stages) when that still fills most of the chip: every
            // weight tile streamed from L2 then serves twice the slots. C128 28x28 60.6 -> 58.3 us, C256 14x14 55.1 -> 51.6; C512 7x7
            // (100 workgroups) 73.8 -> 83.2: stays on the 4-wave form.
            const bool wide_fills = cdiv(q.f, 128) * cdiv(q.n * q.npix8(), 256) * 10 >= (int64_t)num_cu * 7;
            pl.form = (hk.patch_wide == 1 || variant == kConvPatchWide || (hk.patch_wide < 0 && wide_fills)) ? kFormPatchWide : kFormPatch;
        } else if (hk.resident && q.f <= 64 && q.npix() % 8 == 0 && 2 * pl.halo8 <= 128 && !q.residual && q.r == 3 && q.s == 3 && q.ph == 1 &&
                   q.pw == 1 && (q.c == 32 || q.c == 64) && hk.wide == 2) {
            // F <= 64, C <= 64: the whole weight tensor resident in LDS, persistent workgroups over 256-slot tiles (needs a 16-byte
            // aligned x: else s1<1,4,32>)
            pl.form = kFormResident;
        }
    }
    if (pl.form == kFormNone)
        pl.form = q.f <= 64 ? kFormS1_1_4_32 : ((q.c % 64 != 0 || hk.cfg == 1) ? kFormS1_2_2_32 : kFormS1_2_2_64);
    return pl;
}

// ---- the plan ---------------------------------------------------------------------------------------------------------------------
// The routes the dispatcher tries, in order; the generic kernel (conv_igemm16 / conv_direct32) serves everything and runs when the list
// is exhausted. kRouteTapShifted stands for the whole conv_s1.hip family, whose own order is in `s1`: pixel-slot GEMM, tap GEMM, form.
struct ConvPlan {
    int count;
    ConvRoute cand[4];
    ConvS1Plan s1;
};
inline ConvPlan conv_plan(const ConvProblem &q, int dtype, int variant, int num_cu, const ConvHooks &hk, int64_t flag_words) {
    ConvPlan pl = {0, {}, {false, false, 1, 0, kFormNone, 0}};
    if (dtype == INFINI_DT_F32) {
        // fp32 on the fp32 matrix instruction (v_mfma_f32_32x32x2_f32: exact products and sums at 157 TF/s): every groups == 1 layer is
        // the implicit GEMM of gemm32.hip (columns run across images; K rows that are not a multiple of 4 floats — the 3-channel stem —
        // are copied into padded rows). Unit-stride pointwise layers were first routed to the fp32 tile GEMM as one GEMM per image (zero
        // copy, "batched_gemm32"): measured at batch 32 the implicit GEMM with 64 x 64 tiles is faster on every ResNet-50 layer but one
        // (C64 -> 64 @ 56^2: 25.5 vs 69 us; C1024 -> 256 @ 14^2: 52.9 vs 101; C512 -> 256 @ 28^2: 82.6 vs 79.8) — per-image GEMMs leave
        // 23 % of a 14^2 / 7^2 plane's tiles empty and launch few workgroups; IROCM_CONV32_PW_BATCHED keeps that route for A/B. Grouped
        // layers, unaligned operands and variant 1 (A/B, tests) take the one-output-per-thread kernel.
        if (q.groups == 1 && variant != kConvGeneric) {
            if (hk.conv32_pw_batched && conv_1x1(q) && conv_unit_stride(q) && q.dh == 1 && q.dw == 1 && !q.residual && q.npix() % 4 == 0 &&
                q.c % 4 == 0 && q.n * q.f * q.npix() < (1ll << 31))
                pl.cand[pl.count++] = kRouteBatchedGemm32;
            pl.cand[pl.count++] = kRouteIgemm32;
        }
        return pl;
    }
    if (variant == kConvGeneric)
        return pl;
    if (conv_depthwise_shape(q))
        pl.cand[pl.count++] = kRouteDepthwise;
    if (conv_same_s1(q) && conv_pixel_gemm_wanted(q, variant, num_cu))
        pl.cand[pl.count++] = kRoutePixelGemm;
    // (an earlier rule also sent 56x56 pointwise layers with >= 128 filters and <= 256 channels to the small generic tile; since the
    // LDS-staged epilogue conv_s1 wins there too: C256->F128 @56x56 93 vs 112 us)
    if (variant < 0 && conv_one_kstep(q) && !(conv_unit_stride(q) && conv_pw_kernel_shape(q, hk)))
        return pl;
    if (conv_s1_shape(q) && !conv_batched_gemm_first(q, variant)) {
        pl.cand[pl.count++] = kRouteTapShifted;
        pl.s1 = conv_s1_plan(q, variant, num_cu, hk, flag_words);
    }
    if (conv_batched_gemm_shape(q) && !q.residual)
        pl.cand[pl.count++] = kRouteBatchedGemm;
    return pl;
}
// the route and conv_s1.hip form that run when no launcher declines
inline ConvRoute conv_plan_first(const ConvPlan &pl, int dtype, const ConvHooks &hk, ConvForm *form) {
    *form = kFormNone;
    if (pl.count == 0)
        return dtype == INFINI_DT_F32 ? kRouteDirect32 : kRouteGeneric;
    if (pl.cand[0] != kRouteTapShifted)
        return pl.cand[0];
    if (pl.s1.pixel_gemm)
        return kRoutePixelGemm;
    if (pl.s1.tap)
        return pl.s1.tap_split > 1 && !(hk.tap_nt >= 2 && hk.tap_nt <= 4) ? kRouteTapGemmSplitK : kRouteTapGemm;
    *form = pl.s1.form;
    return pl.s1.form == kFormResident ? kRouteResident : kRouteTapShifted;
}

} // namespace irocm
