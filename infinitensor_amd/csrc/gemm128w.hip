// 16-bit GEMM, FOUR waves per workgroup x 128 x 128 wave tiles (round 6). Reference contract: src/kernels/cuda/matmul.cc:67-174
// (C = op(A) op(B), fp32 accumulation, 16-bit output); this kernel serves the plain case — no bias, no activation, M and N multiples
// of 256, K a multiple of 128 — everything else stays on gemm256p_kernel.h.
//
// Why a second K loop. The 8-wave kernel (2 waves per SIMD, 128 x 64 wave tiles, LOAD | COMPUTE phases) holds 0.57-0.60 of the nominal
// MFMA peak, and round 6's probes (probe.hip, profiles/r06_mfma_ceiling.json) showed what a wave that shares nothing could do: with ONE
// wave per SIMD a wave owns one issue slot in four and an MFMA (16 cycles) needs one slot in four, so every other instruction rides in
// a free slot IF it stands alone between two MFMAs — a clump of eight of them behind a group of MFMAs drains the matrix pipe (probe:
// 1 450 TF/s clumped, 1 715-1 742 spread, 2 050 MFMA-only on the same box). A 128 x 128 wave tile also reads half the fragment bytes
// per MFMA of a 128 x 64 one. This kernel is that schedule made real:
//   * a ring of FOUR 32 KB stages in LDS, one k-step of 32 each: [A 256 rows x 32 k | B 32 k x 256 columns];
//   * per k-step and wave: 64 MFMAs (8 x 8 tiles of v_mfma_f32_16x16x32), the fragment reads of the NEXT k-step (stage s + 1 into the
//     other register set), 8 LDS-DMA pieces of the k-step THREE ahead (stage s + 3: the stage whose reads ended at the last barrier),
//     s_waitcnt vmcnt(8) — the pieces issued one step ago — and one barrier;
//   * inside a group of eight MFMAs (accumulator row i) every gap between two MFMAs holds at most ONE other instruction, assigned by
//     the gap map below (gap_busy / adv_map): a fragment read behind MFMA 0 .. 3 (packed into the earliest rows where a K-major
//     operand leaves read gaps over), s_add m0 / the piece behind MFMA 4 / 5 and 6 / 7, and the k advance of a lane offset as one
//     v_add_u32 in an otherwise empty gap behind the offset's last piece of the step — inline asm throughout, accumulators pinned to
//     AGPRs ("+a"), fragments to VGPRs; between a step's first MFMA and its barrier the compiler places nothing but its s_nop 0
//     in front of an s_add m0 and the K loop's counter (read the disassembly of all eight builds after a change to the loop);
//   * persistent over tiles (XCD-chunked, 4-row groups), the k-step stream runs THROUGH tile boundaries: the last three steps of a tile
//     request the next tile's first three, the epilogue (permlane16 swap -> 16-byte stores) runs under them;
//   * a workgroup's LAST tile ends differently (final_block below): its last three k-steps request nothing and run ROW-major, so
//     that accumulator row I is final after 24 (I + 1) MFMAs and its reads, converts, swaps and stores ride in the gaps of row
//     I + 1's MFMAs. Why: the stamps of the diagnostic build (tools/gemm_tail_ledger.py, profiles/gemm128w_tail_ledger.txt; bf16 NN
//     4096^3, one tile per CU, median workgroup) put 5.5 us between the last MFMA and the end of the workgroup — 5.0 of them ISSUING
//     the 32 stores of a wave, i.e. waiting for the store path: 32 MiB leave 256 CUs at once, at what memory takes — and no byte of C
//     moved before them. With the final block the same stretch is 1.0 us; the K phase grows by 3.1 us (the stores now stall issue
//     between MFMAs), the workgroup ends 1.5 us earlier. The C stores are write-through (sc0 sc1): a row's bytes start for memory
//     when they are stored, not at the end-of-kernel write-back — alone worth 2.0 us of 91 (profiles/gemm128w_final_block_ab.txt).
// LDS images. K-major operand (k contiguous in memory): 16-row blocks of sixteen 64-byte SLOTS; row l15 of a block sits in slot
// s = b0 | b3 << 1 | (b2 b1) << 2 of its bits and physical 16-byte chunk c' of slot s holds logical chunk c' ^ (s >> 2). The bit
// permutation is what makes ds_read_b128 conflict-free: the counters (SQ_LDS_BANK_CONFLICT) showed that a b128 read is served in four
// passes of the lanes with EQUAL (l15 >> 1) & 3 — rows l15 = {2p, 2p + 1, 2p + 8, 2p + 9} of all four lane groups — and with rows in
// plain order those four rows cover only two of the four 64-byte bank quarters (a 2-way conflict on every read: + 4 cycles). M/N-major
// operand: gemm256_common.h's image [32 k][512 B] with the mn_f XOR, read by ds_read_b64_tr_b16 pairs.
#include "gemm256_common.h"
#include "diag.h"

namespace irocm {
namespace g128w {

using g256::mn_f;
using g256::sfor;

constexpr int kStage = 32768, kOper = 16384;
constexpr int kLds = 4 * kStage; // 128 KiB
constexpr int kGroupM = 4;       // tile rows per group: 32 consecutive tile indices (one XCD's CUs) form a 4 x 8 block

struct WArgs {
    GemmArgs g;
    int total_tiles;
    int dbg; // IROCM_W128_DBG (bring-up / diagnosis): 1 = no stores (but those the final block issues under its MFMAs), 2 = every piece reads the tile corner, 8 = K-loop clocks into C[0..15], 16 = clock stamps into `stamps`
    unsigned long long *stamps; // dbg & 16 (diagnostic build only): kStamps values per workgroup in the runtime workspace, never in C
};
#ifdef IROCM_DIAG
constexpr bool kDiag = true;
#else
constexpr bool kDiag = false; // the shipped kernels hold no clock read
#endif
constexpr int kStamps = 8; // core clock at entry, first MFMA, last MFMA, last store issued, after the final wait; 100 MHz clock at entry,
                           // last MFMA, after the final wait (tools/gemm_tail_ledger.py)

// Fragment sets: two register sets x 8 fragments of one operand (a third, and DST = a register other than the fragment's own, only in
// the final block of a workgroup's last tile: registers are assigned by liveness, a set nobody holds costs none).
template <bool KMAJOR> struct Frags;
template <> struct Frags<true> {
    s16x8_t v[3][8];
    unsigned base[2]; // lane address in stage 0 / stage 2 (stages 1 / 3 by the immediate offset)
    __device__ __forceinline__ void init(unsigned lds_oper, int half, int l15, int g4) {
        const int slot = (l15 & 1) | (((l15 >> 3) & 1) << 1) | (((l15 >> 1) & 3) << 2); // row l15 of a 16-row block -> its 64-byte slot
        base[0] = lds_oper + (unsigned)(half * 8192 + slot * 64 + ((g4 ^ (slot >> 2)) & 3) * 16);
        base[1] = base[0] + 2u * kStage;
    }
    template <int SET, int F, int STAGE, int DST = F> __device__ __forceinline__ void read0() {
        asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(v[SET][DST]) : "v"(base[STAGE >> 1]), "i"(F * 1024 + (STAGE & 1) * kStage));
    }
    template <int SET, int F, int STAGE, int DST = F> __device__ __forceinline__ void read1() {}
    template <int SET, int F> __device__ __forceinline__ s16x8_t get() const { return v[SET][F]; }
};
template <> struct Frags<false> {
    s16x4_t lo[3][8], hi[3][8];
    unsigned addr[8]; // lane address of fragment f in stage 0 (stage 1 by the immediate offset, stages 2 / 3 by one VALU add at the read:
                      // sixteen more address registers per operand spilled the both-operands-M/N-major build)
    __device__ __forceinline__ void init(unsigned lds_oper, int half, int l15, int g4) {
        const int mnf = ((l15 >> 2) & 3) | ((g4 & 1) << 2);
        const unsigned mn_lane = (unsigned)((g4 * 8 + (l15 >> 2)) * 512 + (l15 & 1) * 8);
#pragma unroll
        for (int f = 0; f < 8; ++f) {
            const int c16 = ((l15 >> 1) & 1) | (((half * 8 + f) ^ mnf) << 1);
            addr[f] = lds_oper + mn_lane + (unsigned)c16 * 16u;
        }
    }
    template <int SET, int F, int STAGE, int DST = F> __device__ __forceinline__ void read0() {
        const unsigned a = STAGE >= 2 ? addr[F] + 2u * kStage : addr[F];
        asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(lo[SET][DST]) : "v"(a), "i"((STAGE & 1) * kStage));
    }
    template <int SET, int F, int STAGE, int DST = F> __device__ __forceinline__ void read1() {
        const unsigned a = STAGE >= 2 ? addr[F] + 2u * kStage : addr[F];
        asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(hi[SET][DST]) : "v"(a), "i"((STAGE & 1) * kStage + 2048));
    }
    template <int SET, int F> __device__ __forceinline__ s16x8_t get() const {
        return s16x8_t{lo[SET][F][0], lo[SET][F][1], lo[SET][F][2], lo[SET][F][3], hi[SET][F][0], hi[SET][F][1], hi[SET][F][2], hi[SET][F][3]};
    }
};

// per-lane byte offsets of a wave's four pieces of one operand's stage, relative to the tile's (row0 / col0, k0) corner
template <bool KMAJOR> __device__ __forceinline__ void piece_offs(unsigned (&off)[4], long ld, int w, int lane) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int piece = w * 4 + i;
        if constexpr (KMAJOR) {
            const int slot = lane >> 2; // the lane's 64-byte slot of the piece's 1 KB; it holds row (bit permutation below) of the block
            const int r = piece * 16 + ((slot & 1) | (((slot >> 2) & 3) << 1) | (((slot >> 1) & 1) << 3));
            const int c_log = (lane & 3) ^ ((slot >> 2) & 3);
            off[i] = (unsigned)(((long)r * ld + c_log * 8) * 2);
        } else {
            const int kr = piece * 2 + (lane >> 5);
            const int c_log = (lane & 31) ^ (mn_f(kr) << 1);
            off[i] = (unsigned)(((long)kr * ld + c_log * 8) * 2);
        }
    }
}

// Which pieces a wave requests in the k-step at position S of a block of four (the pieces of k-step g + 3, stage (S + 3) & 3).
// An M/N-major operand takes four every step. A K-MAJOR operand's 64-byte row segment is HALF a 128-byte cache line whose other half
// is the next k-step's: requested a step apart, every line would travel L2 -> L1 twice (measured: each K-major operand cost 5-10 %).
// So a K-major operand requests on ODD steps only, the four pieces of k-step g + 3 each followed by its sibling of k-step g + 4 (same
// lane offset + 64 bytes, into stage S & 3 — the stage the MFMAs of this step took their fragments from a step ago, free since the
// last barrier): the sibling finds its line in flight or in L1.
struct PieceSel {
    int oper, idx, stage, imm;
};
template <bool AKM, bool BKM> constexpr int step_pieces(int S) { return (AKM ? ((S & 1) ? 8 : 0) : 4) + (BKM ? ((S & 1) ? 8 : 0) : 4); }
template <bool AKM, bool BKM> constexpr PieceSel piece_sel(int S, int q) {
    const int na = AKM ? ((S & 1) ? 8 : 0) : 4;
    const int oper = q < na ? 0 : 1, r = q < na ? q : q - na;
    const bool km = oper == 0 ? AKM : BKM;
    if (!km)
        return {oper, r, (S + 3) & 3, 0};
    return {oper, r >> 1, (r & 1) ? (S & 3) : ((S + 3) & 3), (r & 1) * 64};
}
// entry of the list that goes behind MFMA 4 / 5 (slot 0) or 6 / 7 (slot 1) of MFMA group I; -1: none
constexpr int slot_piece(int n, int I, int slot) {
    if (n == 0)
        return -1;
    if (n <= 8) {
        const int stride = 8 / n;
        return (slot == 0 && I % stride == 0) ? I / stride : -1;
    }
    return slot == 0 ? I : (8 + I < n ? 8 + I : -1);
}

// The GAP MAP of a k-step. Gap g = 8 I + J is the issue slot behind MFMA J of accumulator row I; a gap holds at most ONE instruction.
//   * fragment reads of the next k-step: gaps J = 0 .. 3, one read per gap in the EARLIEST rows, in the order of use (per fragment f:
//     A's read(s), then B's): 32 reads with two M/N-major operands (fragment I in row I), 24 with one (rows 0 .. 5), 16 with none
//     (rows 0 .. 3) — the boundary's lgkmcnt(0) then waits for reads issued at least 32 MFMAs earlier;
//   * pieces: s_add m0 / the LDS-DMA load in gaps J = 4 / 5 (slot 0) and 6 / 7 (slot 1) of the rows slot_piece names;
//   * the k advance of a lane offset (four per operand; due in every step that requests from it): ONE v_add_u32 in the first gap
//     behind the step's last piece that reads the offset which holds nothing else. Where a step leaves no such gap (both operands
//     K-major, odd steps: sixteen pieces, the last in row 7, J = 7) the add goes into the first empty gap of the FOLLOWING step, ahead
//     of that step's first piece off the same offset (there: none, a K-major operand requests nothing on even steps).
// Left to the compiler, the advances become induction variables and land as clumps of three to eight VALU adds in front of the barriers
// and behind them — on the one stretch of a step where no MFMA covers them.
struct ReadSel {
    int oper, f, half;
};
template <bool AKM, bool BKM> constexpr int step_reads() { return 32 - (AKM ? 8 : 0) - (BKM ? 8 : 0); }
template <bool AKM, bool BKM> constexpr ReadSel read_sel(int r) {
    const int na = AKM ? 1 : 2, per = na + (BKM ? 1 : 2), f = r / per, w = r % per;
    return w < na ? ReadSel{0, f, w} : ReadSel{1, f, w - na};
}
template <bool AKM, bool BKM> constexpr bool gap_busy(int S, int g) {
    const int I = g >> 3, J = g & 7;
    return J < 4 ? I * 4 + J < step_reads<AKM, BKM>() : slot_piece(step_pieces<AKM, BKM>(S), I, (J - 4) >> 1) >= 0;
}
// gap of the first (last = false) / last load in step S that reads lane offset k = 4 oper + idx; -1: the step requests nothing off it
template <bool AKM, bool BKM> constexpr int offset_use(int S, int k, bool last) {
    const int np = step_pieces<AKM, BKM>(S);
    int found = -1;
    for (int g = 0; g < 64; ++g) {
        const int I = g >> 3, J = g & 7;
        if (J != 5 && J != 7)
            continue;
        const int q = slot_piece(np, I, (J - 4) >> 1);
        if (q < 0)
            continue;
        const PieceSel ps = piece_sel<AKM, BKM>(S, q);
        if (ps.oper * 4 + ps.idx != k)
            continue;
        if (!last)
            return g;
        found = g;
    }
    return found;
}
struct AdvMap {
    int own[8]; // gap of the add due in this step; -1: none due, or no gap left behind the last use (then it is in `in` of the next step)
    int in[8];  // gap of the add the previous step could not place; -1: none
};
template <bool AKM, bool BKM> constexpr AdvMap adv_own(int S) {
    AdvMap m{};
    bool taken[64] = {};
    for (int g = 0; g < 64; ++g) taken[g] = gap_busy<AKM, BKM>(S, g);
    for (int k = 0; k < 8; ++k) {
        m.own[k] = m.in[k] = -1;
        const int lu = offset_use<AKM, BKM>(S, k, true);
        if (lu < 0)
            continue;
        for (int g = lu + 1; g < 64; ++g)
            if (!taken[g]) {
                taken[g] = true;
                m.own[k] = g;
                break;
            }
    }
    return m;
}
template <bool AKM, bool BKM> constexpr bool adv_deferred(int S, int k) {
    return offset_use<AKM, BKM>(S, k, true) >= 0 && adv_own<AKM, BKM>(S).own[k] < 0;
}
template <bool AKM, bool BKM> constexpr AdvMap adv_map(int S) {
    AdvMap m = adv_own<AKM, BKM>(S);
    bool taken[64] = {};
    for (int g = 0; g < 64; ++g) taken[g] = gap_busy<AKM, BKM>(S, g);
    for (int k = 0; k < 8; ++k)
        if (m.own[k] >= 0)
            taken[m.own[k]] = true;
    for (int k = 0; k < 8; ++k) {
        if (!adv_deferred<AKM, BKM>((S + 3) & 3, k))
            continue;
        for (int g = 0; g < 64; ++g)
            if (!taken[g]) {
                taken[g] = true;
                m.in[k] = g;
                break;
            }
    }
    return m;
}
// lane offset advanced in gap g of step S; -1: none
template <bool AKM, bool BKM> constexpr int adv_at(int S, int g) {
    const AdvMap m = adv_map<AKM, BKM>(S);
    for (int k = 0; k < 8; ++k)
        if (m.own[k] == g || m.in[k] == g)
            return k;
    return -1;
}
// every add has its gap, and an add that moved into the following step stands ahead of that step's first piece off its offset
template <bool AKM, bool BKM> constexpr bool adv_map_ok() {
    for (int S = 0; S < 4; ++S) {
        const AdvMap m = adv_map<AKM, BKM>(S);
        for (int k = 0; k < 8; ++k) {
            const int fu = offset_use<AKM, BKM>(S, k, false);
            if (adv_deferred<AKM, BKM>((S + 3) & 3, k) && (m.in[k] < 0 || (fu >= 0 && m.in[k] > fu)))
                return false;
        }
    }
    return true;
}

// The final block's epilogue of one accumulator row as 60 single instructions, in the order they are issued one to three per MFMA gap
// of the NEXT row: P(jp) = the 8 accumulator reads and 4 packed converts of column-tile pair jp (read, read, convert; 12), W(jp) = its
// two lane-group swaps, T(jp) = its 16-byte store. Order P0 P1 W0 P2 T0 W1 P3 T1 W2 T2 W3 T3: at least four instructions lie between a
// convert and the swap that reads it (the hazard asks for two wait states), and a store's registers are rewritten by the next row only.
// (the instruction Tr::pack2 compiles to, as a statement that stays where it is written)
template <typename Tr> __device__ __forceinline__ unsigned cvt_pk_a(float lo, float hi) {
    unsigned r;
    if constexpr (Tr::kDType == INFINI_DT_BF16) asm volatile("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(r) : "v"(lo), "v"(hi));
    else asm volatile("v_cvt_pk_f16_f32 %0, %1, %2" : "=v"(r) : "v"(lo), "v"(hi));
    return r;
}
// C stores write through (tools/build_variant.py ... -DIROCM_W128_C_WB builds the write-back variant the A/B was taken against)
#ifdef IROCM_W128_C_WB
#define W128_ST_MOD ""
#else
#define W128_ST_MOD " sc0 sc1"
#endif
struct EpiUnit {
    int kind, jp, t; // kind 0 = P (t = 0 .. 11), 1 = W (t = 0, 1), 2 = T
};
constexpr int kEpiUnits = 60;
constexpr EpiUnit epi_unit(int e) {
    const int kind[12] = {0, 0, 1, 0, 2, 1, 0, 2, 1, 2, 1, 2};
    const int jp[12] = {0, 1, 0, 2, 0, 1, 3, 1, 2, 2, 3, 3};
    const int size[12] = {12, 12, 2, 12, 1, 2, 12, 1, 2, 1, 2, 1};
    int s = 0;
    for (int i = 0; i < 12; ++i) {
        if (e < s + size[i])
            return {kind[i], jp[i], e - s};
        s += size[i];
    }
    return {-1, 0, 0};
}

template <typename Tr, bool FIRST> __device__ __forceinline__ void mfma_a(f32x4 &acc, s16x8_t x, s16x8_t y) {
    if constexpr (Tr::kDType == INFINI_DT_BF16) {
        if constexpr (FIRST) asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, 0" : "=a"(acc) : "v"(x), "v"(y));
        else asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, %0" : "+a"(acc) : "v"(x), "v"(y));
    } else {
        if constexpr (FIRST) asm volatile("v_mfma_f32_16x16x32_f16 %0, %1, %2, 0" : "=a"(acc) : "v"(x), "v"(y));
        else asm volatile("v_mfma_f32_16x16x32_f16 %0, %1, %2, %0" : "+a"(acc) : "v"(x), "v"(y));
    }
}

template <typename Tr, bool AKM, bool BKM>
__global__ __launch_bounds__(256, 1) void gemm128w_kernel(WArgs pw) {
    extern __shared__ __attribute__((aligned(1024))) char smem[];
    const GemmArgs &p = pw.g;
    unsigned long long tc0 = 0, tr0 = 0; // kernel entry
    if constexpr (kDiag) {
        tc0 = __builtin_amdgcn_s_memtime();
        tr0 = __builtin_amdgcn_s_memrealtime();
    }
    const int t = threadIdx.x, lane = t & 63, l15 = lane & 15, g4 = lane >> 4;
    int w;
    asm volatile("v_readfirstlane_b32 %0, %1" : "=s"(w) : "v"(t >> 6));
    const int wr = w >> 1, wc = w & 1;
    const unsigned lds0 = (unsigned)(unsigned long)IROCM_LDS_PTR(smem);
    unsigned lds0s;
    asm volatile("v_readfirstlane_b32 %0, %1" : "=s"(lds0s) : "v"(lds0));

    // ---- operand geometry (bytes) -----------------------------------------------------------------
    const long lda = AKM ? p.a_rs : p.a_cs, ldb = BKM ? p.b_cs : p.b_rs; // elements between rows of the image's major index
    unsigned a_kstep = (unsigned)(AKM ? 64 : 64 * lda), b_kstep = (unsigned)(BKM ? 64 : 64 * ldb); // 32 k
    const long a_tile = AKM ? 512 * lda : 512, b_tile = BKM ? 512 * ldb : 512; // 256 rows / columns
    // The k advance lives in the LANE offsets (eight VALU adds per step), the 64-bit corner in an SGPR pair that changes once per tile:
    // a VMEM instruction in inline asm must not read an SGPR within five wait states of the instruction that wrote it, and a pointer the
    // compiler advances by SALU every step ends up written wherever its scheduler likes.
    unsigned a_off[4], b_off[4];
    piece_offs<AKM>(a_off, lda, w, lane);
    piece_offs<BKM>(b_off, ldb, w, lane);
    if (pw.dbg & 2) {
        a_kstep = b_kstep = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) a_off[i] = b_off[i] = (unsigned)lane * 16u;
    }
    const int ksteps = p.k >> 5, nkb = ksteps >> 2;
    const unsigned a_span = a_kstep * (unsigned)ksteps, b_span = b_kstep * (unsigned)ksteps; // a tile's whole k advance

    // ---- tiles: workgroup ids consecutive per XCD, tile index -> (batch, tile row, tile column) in groups of kGroupM rows -------
    const unsigned grid = gridDim.x, wg = xcd_remap(blockIdx.x, grid);
    const unsigned per_batch = (unsigned)(p.tiles_m * p.tiles_n);
    auto decode = [&](unsigned tile, const char *&ab, const char *&bb, long &c_elem) {
        const unsigned ib = tile / per_batch, r = tile - ib * per_batch;
        const unsigned gspan = (unsigned)(kGroupM * p.tiles_n), grp = r / gspan, i = r - grp * gspan;
        const unsigned first_m = grp * kGroupM;
        const unsigned gsz = (unsigned)p.tiles_m - first_m < (unsigned)kGroupM ? (unsigned)p.tiles_m - first_m : (unsigned)kGroupM;
        const unsigned tn = i / gsz, tm = first_m + (i - tn * gsz);
        ab = (const char *)p.a + ((long)ib * p.a_bs) * 2 + (long)tm * a_tile;
        bb = (const char *)p.b + ((long)ib * p.b_bs) * 2 + (long)tn * b_tile;
        c_elem = (long)ib * p.c_bs + (long)tm * 256 * p.n + (long)tn * 256;
    };
    auto uniform = [](const char *q) {
        const unsigned long v = (unsigned long)q;
        const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v), hi = __builtin_amdgcn_readfirstlane((unsigned)(v >> 32));
        return (const char *)(((unsigned long)hi << 32) | lo);
    };

    unsigned tile = wg;
    const char *pa, *pb; // tile corner the pieces of the NEXT issuing step read from (a_off / b_off carry the k advance)
    long c_elem;
    decode(tile, pa, pb, c_elem);
    pa = uniform(pa);
    pb = uniform(pb);

    // ---- LDS-DMA ------------------------------------------------------------------------------------
    unsigned m0w = lds0s + (unsigned)w * 4096u; // this wave's first piece slot of operand A in stage 0
    auto load_piece = [&](auto operc, auto idxc, auto immc) __attribute__((always_inline)) {
        constexpr int OP = decltype(operc)::value, IDX = decltype(idxc)::value, IMM = decltype(immc)::value;
        const unsigned off = OP == 0 ? a_off[IDX] : b_off[IDX]; // (copies: clang does not capture a variable a generic lambda names
        const char *base = OP == 0 ? pa : pb;                   //  only in an asm operand)
        // (default cache policy for both kinds of piece: `nt` on the M/N-major ones cost 13 %, `sc0` nothing either way —
        // profiles/gemm128w_kstep_ab.txt)
        asm volatile("global_load_lds_dwordx4 %0, %1 offset:%2" ::"v"(off), "s"(base), "i"(IMM) : "memory");
    };
    // the k advance of one lane offset as ONE instruction that stays where it is written (the gap map above)
    auto bump = [&](auto operc, auto idxc) __attribute__((always_inline)) {
        constexpr int OP = decltype(operc)::value, IDX = decltype(idxc)::value;
        unsigned &off = OP == 0 ? a_off[IDX] : b_off[IDX];
        if constexpr (OP == 0 ? AKM : BKM) {
            asm volatile("v_add_u32 %0, 0x80, %0" : "+v"(off));
        } else {
            const unsigned by = OP == 0 ? a_kstep : b_kstep;
            asm volatile("v_add_u32 %0, %1, %0" : "+v"(off) : "s"(by));
        }
    };
    // (the instruction offset of an LDS-DMA load moves BOTH addresses, memory and LDS: IMM is taken back out of M0)
    auto set_m0 = [&m0w](auto stc, auto operc, auto idxc, auto immc) __attribute__((always_inline)) {
        constexpr int ST = decltype(stc)::value, OP = decltype(operc)::value, IDX = decltype(idxc)::value, IMM = decltype(immc)::value;
        const unsigned m0base = m0w;
        // (s_add writes SCC: undeclared, the compiler parks an add-with-carry or a compare across this statement)
        asm volatile("s_add_u32 m0, %0, %1" ::"s"(m0base), "i"(ST * kStage + OP * kOper + IDX * 1024 - IMM) : "memory", "scc");
    };
    // A VMEM instruction must not read an SGPR within five wait states of the SALU / VALU instruction that wrote it, and the compiler
    // keeps that rule only for instructions it knows: the tile corners are therefore pinned into their registers where they are
    // computed (an empty asm the pointer passes through), at least one MFMA group away from the inline-asm pieces that read them.
    auto pin = [&]() __attribute__((always_inline)) { asm volatile("" : "+s"(pa), "+s"(pb)); };
    // prologue: one operand's four pieces of k-step ST (M/N-major) or of the k-step pair ST, ST + 1 (K-major), back to back
    auto request = [&](auto stc, auto operc) __attribute__((always_inline)) {
        constexpr int ST = decltype(stc)::value, OP = decltype(operc)::value;
        constexpr bool KM = OP == 0 ? AKM : BKM;
        sfor<4>([&](auto idxc) {
            set_m0(stc, operc, idxc, std::integral_constant<int, 0>{});
            asm volatile("s_nop 0" ::: "memory");
            load_piece(operc, idxc, std::integral_constant<int, 0>{});
            if constexpr (KM) {
                set_m0(std::integral_constant<int, ST + 1>{}, operc, idxc, std::integral_constant<int, 64>{});
                asm volatile("s_nop 0" ::: "memory");
                load_piece(operc, idxc, std::integral_constant<int, 64>{});
            }
        });
    };
    auto advance = [&](auto operc, unsigned by) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if constexpr (decltype(operc)::value == 0) a_off[i] += by;
            else b_off[i] += by;
        }
    };
    // the prologue's last advance stands for step 3's: an offset whose add step 3 hands on to step 0 (gap map) is left to step 0 here too
    auto advance_entry = [&](auto operc, unsigned by) __attribute__((always_inline)) {
        constexpr int OP = decltype(operc)::value;
        sfor<4>([&](auto idxc) {
            constexpr int IDX = decltype(idxc)::value;
            if constexpr (!adv_deferred<AKM, BKM>(3, OP * 4 + IDX)) {
                if constexpr (OP == 0) a_off[IDX] += by;
                else b_off[IDX] += by;
            }
        });
    };
    static_assert(adv_map_ok<AKM, BKM>(), "gap map: an offset's add has no gap");
    constexpr std::integral_constant<int, 0> kA{};
    constexpr std::integral_constant<int, 1> kB{};

    // ---- fragments -----------------------------------------------------------------------------------
    Frags<AKM> fa;
    Frags<BKM> fb;
    fa.init(lds0, wr, l15, g4);
    fb.init(lds0 + kOper, wc, l15, g4);
    f32x4 acc[8][8];

    // ---- prologue: k-steps 0 .. 2 of the first tile requested (a K-major operand: pairs 0 and 1 = k-steps 0 .. 3), step 0's fragments
    // read. Issue order = order of need, so that the counted waits below leave exactly the later groups in flight.
    constexpr int nKM = (AKM ? 1 : 0) + (BKM ? 1 : 0), nMN = 2 - nKM;
    pin();
    asm volatile("s_nop 4" ::: "memory");
    if constexpr (AKM) request(std::integral_constant<int, 0>{}, kA); // group 0: everything k-step 0 needs (K-major: the pair 0, 1)
    if constexpr (BKM) request(std::integral_constant<int, 0>{}, kB);
    if constexpr (!AKM) request(std::integral_constant<int, 0>{}, kA);
    if constexpr (!BKM) request(std::integral_constant<int, 0>{}, kB);
    if constexpr (AKM) advance(kA, 128);
    else advance(kA, a_kstep);
    if constexpr (BKM) advance(kB, 128);
    else advance(kB, b_kstep);
    if constexpr (!AKM) request(std::integral_constant<int, 1>{}, kA); // group 1: the M/N-major operands' k-step 1
    if constexpr (!BKM) request(std::integral_constant<int, 1>{}, kB);
    if constexpr (!AKM) advance(kA, a_kstep);
    if constexpr (!BKM) advance(kB, b_kstep);
    if constexpr (AKM) request(std::integral_constant<int, 2>{}, kA); // group 2: k-step 2 (K-major: the pair 2, 3)
    if constexpr (BKM) request(std::integral_constant<int, 2>{}, kB);
    if constexpr (!AKM) request(std::integral_constant<int, 2>{}, kA);
    if constexpr (!BKM) request(std::integral_constant<int, 2>{}, kB);
    if constexpr (AKM) advance_entry(kA, 128);
    else advance_entry(kA, a_kstep);
    if constexpr (BKM) advance_entry(kB, 128);
    else advance_entry(kB, b_kstep);
    constexpr int kG1 = 4 * nMN, kG2 = 8 * nKM + 4 * nMN;
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(kG1 + kG2) : "memory");
    __builtin_amdgcn_s_barrier();
    sfor<8>([&](auto fc) {
        constexpr int F = decltype(fc)::value;
        fa.template read0<0, F, 0>();
        fa.template read1<0, F, 0>();
        fb.template read0<0, F, 0>();
        fb.template read1<0, F, 0>();
    });
    asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(kG2) : "memory");
    __builtin_amdgcn_s_barrier();

    // one k-step: S = position in the block of four (register set S & 1; reads stage S + 1; its pieces go to stage S + 3)
    const char *na = pa, *nb = pb; // the next tile's corner
    auto step = [&](auto sc, auto firstc, bool last_block) __attribute__((always_inline)) {
        constexpr int S = decltype(sc)::value;
        constexpr bool FIRST = decltype(firstc)::value;
        constexpr int CUR = S & 1, NXT = CUR ^ 1, RS = (S + 1) & 3, NP = step_pieces<AKM, BKM>(S);
        sfor<8>([&](auto ic) {
            constexpr int I = decltype(ic)::value;
            sfor<8>([&](auto jc) {
                constexpr int J = decltype(jc)::value;
                mfma_a<Tr, FIRST>(acc[I][J], fb.template get<CUR, J>(), fa.template get<CUR, I>());
                if constexpr (J < 4 && I * 4 + J < step_reads<AKM, BKM>()) {
                    constexpr ReadSel rs = read_sel<AKM, BKM>(I * 4 + J);
                    if constexpr (rs.oper == 0 && rs.half == 0) fa.template read0<NXT, rs.f, RS>();
                    if constexpr (rs.oper == 0 && rs.half == 1) fa.template read1<NXT, rs.f, RS>();
                    if constexpr (rs.oper == 1 && rs.half == 0) fb.template read0<NXT, rs.f, RS>();
                    if constexpr (rs.oper == 1 && rs.half == 1) fb.template read1<NXT, rs.f, RS>();
                }
                constexpr int ADV = adv_at<AKM, BKM>(S, I * 8 + J);
                if constexpr (ADV >= 0) bump(std::integral_constant<int, (ADV >> 2)>{}, std::integral_constant<int, (ADV & 3)>{});
                if constexpr (J >= 4) {
                    constexpr int Q = slot_piece(NP, I, (J - 4) >> 1);
                    if constexpr (Q >= 0) {
                        constexpr PieceSel ps = piece_sel<AKM, BKM>(S, Q);
                        if constexpr ((J & 1) == 0)
                            set_m0(std::integral_constant<int, ps.stage>{}, std::integral_constant<int, ps.oper>{}, std::integral_constant<int, ps.idx>{},
                                   std::integral_constant<int, ps.imm>{});
                        else
                            load_piece(std::integral_constant<int, ps.oper>{}, std::integral_constant<int, ps.idx>{}, std::integral_constant<int, ps.imm>{});
                    }
                }
            });
        });
        // The offsets moved on to the next k-step (pair) of this tile in their gaps. Behind the tile's fourth-last step, where both kinds
        // of operand have requested everything of this tile, they go back by the tile's whole k advance and the corner becomes the next
        // tile's (once per tile: these eight adds may stand together)
        if (S == 0 && last_block) {
            pa = na;
            pb = nb;
            pin();
            advance(kA, 0u - a_span);
            advance(kB, 0u - b_span);
        }
        asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(NP) : "memory");
        __builtin_amdgcn_s_barrier();
    };
    constexpr std::integral_constant<int, 0> k0{};
    constexpr std::integral_constant<int, 1> k1{};
    constexpr std::integral_constant<int, 2> k2{};
    constexpr std::integral_constant<int, 3> k3{};
    auto block = [&](auto firstc, bool last_block) __attribute__((always_inline)) { // four k-steps
        step(k0, firstc, last_block);
        step(k1, std::false_type{}, last_block);
        step(k2, std::false_type{}, last_block);
        step(k3, std::false_type{}, last_block);
    };
    // (clock stamps: the diagnostic build only, workgroup-uniform scalars until wave 0 stores them behind the final wait)
    unsigned long long tc_first = 0, tr_first = 0, tc_mfma = 0, tr_mfma = 0, tc_store = 0;
    if constexpr (kDiag) {
        tc_first = __builtin_amdgcn_s_memtime();
        tr_first = __builtin_amdgcn_s_memrealtime();
    }
    const unsigned total = (unsigned)pw.total_tiles;
    const long ldc2 = (long)p.n * 2;
    // ---- the final block: k-steps L-3 .. L-1 of a workgroup's LAST tile, behind step 0 of its last block (which requested the last
    // M/N-major pieces and read k-step L-3's fragments into set 1). No requests are left and no next tile, so the order turns ROW-major:
    // for accumulator row I the 3 x 8 MFMAs of k-steps L-3, L-2, L-1 (ascending k into the same accumulator: the sums are the k-outer
    // order's, bit for bit), after which row I is final — and its epilogue (epi_unit: 32 reads, 16 converts, 8 swaps, 4 stores) is issued
    // two or three instructions per gap between row I + 1's 24 MFMAs, so that C leaves the CU while the matrix pipe still works; row 7's
    // stays exposed. Fragments: B of all three k-steps (set 1 as read; L-2 -> set 0 and L-1 -> set 2, read under row 0's first sixteen
    // MFMAs), A of k-step L-3 as read (set 1), A of L-2 / L-1 per row into slots (I & 1) * 2 + {0, 1} of set 0, read under row I - 1's
    // last eight MFMAs. Row 0 holds the two waits that have no distance: for everything in flight plus the one barrier in front of the
    // first read of stage 3, and for B of k-step L-1 in front of its first use; behind the barrier nothing writes LDS any more.
    auto final_block = [&]() __attribute__((always_inline)) {
        const int ln = (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
        const unsigned c_lane = (unsigned)(((long)(ln & 15) * p.n + ((ln >> 4) & 1) * 16 + (ln >> 5) * 8) * 2);
        char *cw = (char *)p.c + (c_elem + (long)wr * 128 * p.n + wc * 128) * 2;
        cw = (char *)uniform(cw);
        unsigned pu[8], pv[8]; // the retiring row's packed halves (epilogue below: u / v)
        float t0 = 0.f, t1 = 0.f;
        sfor<8>([&](auto ic) {
            constexpr int I = decltype(ic)::value;
            constexpr int SA = (I & 1) * 2, SN = ((I + 1) & 1) * 2; // this row's / the next row's A slots in set 0
            char *cb = cw + (long)(I > 0 ? I - 1 : 0) * 16 * ldc2; // the retiring row's base: pinned here, first read five MFMAs on
            asm volatile("" : "+s"(cb));
            if constexpr (I > 0) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); // this row's A slots, read six gaps ago
            sfor<24>([&](auto mc) {
                constexpr int M = decltype(mc)::value, KS = M >> 3, J = M & 7;
                if constexpr (I == 0 && M == 8) {
                    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
                    __builtin_amdgcn_s_barrier();
                }
                if constexpr (I == 0 && M == 16) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                if constexpr (KS == 0) mfma_a<Tr, false>(acc[I][J], fb.template get<1, J>(), fa.template get<1, I>());
                if constexpr (KS == 1) mfma_a<Tr, false>(acc[I][J], fb.template get<0, J>(), fa.template get<0, SA>());
                if constexpr (KS == 2) mfma_a<Tr, false>(acc[I][J], fb.template get<2, J>(), fa.template get<0, SA + 1>());
                if constexpr (I == 0 && KS == 0) {
                    fb.template read0<0, J, 2>();
                    fb.template read1<0, J, 2>();
                    if constexpr (J == 0) {
                        fa.template read0<0, 0, 2, 0>();
                        fa.template read1<0, 0, 2, 0>();
                    }
                }
                if constexpr (I == 0 && KS == 1) {
                    fb.template read0<2, J, 3>();
                    fb.template read1<2, J, 3>();
                    if constexpr (J == 0) {
                        fa.template read0<0, 0, 3, 1>();
                        fa.template read1<0, 0, 3, 1>();
                    }
                }
                if constexpr (I < 7 && M == 16) {
                    fa.template read0<0, I + 1, 2, SN>();
                    fa.template read1<0, I + 1, 2, SN>();
                }
                if constexpr (I < 7 && M == 17) {
                    fa.template read0<0, I + 1, 3, SN + 1>();
                    fa.template read1<0, I + 1, 3, SN + 1>();
                }
                if constexpr (I > 0) {
                    constexpr int R = I - 1, E0 = M * kEpiUnits / 24, E1 = (M + 1) * kEpiUnits / 24;
                    sfor<E1 - E0>([&](auto uc) {
                        constexpr EpiUnit un = epi_unit(E0 + decltype(uc)::value);
                        if constexpr (un.kind == 0) {
                            constexpr int Q = 2 * un.jp + un.t / 6, H = (un.t % 6) / 3, RR = un.t % 3;
                            if constexpr (RR < 2) {
                                const float src = acc[R][Q][2 * H + RR];
                                float dst;
                                asm volatile("v_accvgpr_read_b32 %0, %1" : "=v"(dst) : "a"(src));
                                if constexpr (RR == 0) t0 = dst;
                                else t1 = dst;
                            } else if constexpr (un.t < 6) {
                                pu[2 * un.jp + H] = cvt_pk_a<Tr>(t0, t1);
                            } else {
                                pv[2 * un.jp + H] = cvt_pk_a<Tr>(t0, t1);
                            }
                        } else if constexpr (un.kind == 1) {
                            unsigned x = pu[2 * un.jp + un.t], y = pv[2 * un.jp + un.t];
                            asm volatile("v_permlane16_swap_b32 %0, %1" : "+v"(x), "+v"(y));
                            pu[2 * un.jp + un.t] = x;
                            pv[2 * un.jp + un.t] = y;
                        } else {
                            const u32x4_t d = u32x4_t{pu[2 * un.jp], pu[2 * un.jp + 1], pv[2 * un.jp], pv[2 * un.jp + 1]};
                            const unsigned cl = c_lane;
                            char *cbs = cb;
                            asm volatile("global_store_dwordx4 %0, %1, %2 offset:%3" W128_ST_MOD ::"v"(cl), "v"(d), "s"(cbs), "i"(un.jp * 64) : "memory");
                        }
                    });
                }
            });
        });
    };
    auto epilogue = [&](auto firstrowc) __attribute__((always_inline)) { // rows FIRSTROW .. 7 (the final block leaves row 7 only)
        constexpr int FIRSTROW = decltype(firstrowc)::value;
        if constexpr (kDiag) {
            tc_mfma = __builtin_amdgcn_s_memtime();
            tr_mfma = __builtin_amdgcn_s_memrealtime();
        }
        // ---- epilogue: lane l holds, of tile (i, j), row l15 and the four columns g4 * 4 ...; a permlane16 swap between the packed
        // halves of tiles j and j + 1 leaves every lane eight consecutive columns: one 16-byte store per tile pair. Per accumulator row
        // in BATCHES — the row's 32 reads and 16 converts (the compiler's), then its 8 swaps, then its 4 stores, each batch ONE asm
        // statement — so that distance keeps the hazards a pad kept per instruction before: the only pads left are the two wait states
        // in front of a row's first swap (the compiler orders the converts and may put the one a swap reads right in front of the
        // statement) and behind its last store (the next row's first convert may write that store's data registers) -------------------
        asm volatile("s_nop 15\n\ts_nop 15" ::: "memory"); // the last MFMAs' results (inline asm: no hazard bookkeeping by the compiler)
        // (the lane's store offset is rebuilt from mbcnt here: carried across the K loop it is the register the M/N x M/N build spills)
        const int ln = (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
        const unsigned c_lane = (unsigned)(((long)(ln & 15) * p.n + ((ln >> 4) & 1) * 16 + (ln >> 5) * 8) * 2);
        char *cw = (char *)p.c + (c_elem + (long)wr * 128 * p.n + wc * 128) * 2;
        cw = (char *)uniform(cw);
        if (!(pw.dbg & 1))
        sfor<8>([&](auto ic) {
            constexpr int I = decltype(ic)::value;
            if constexpr (I < FIRSTROW) return;
            char *cb = cw + (long)I * 16 * ldc2;
            asm volatile("s_nop 4" : "+s"(cb)); // (the row block's base was just computed by SALU: five wait states ahead of a VMEM read)
            unsigned u[8], v[8]; // packed halves of tiles 2 JP (u) and 2 JP + 1 (v): columns 0 1 | 2 3 of the lane's four
#pragma unroll
            for (int jp = 0; jp < 4; ++jp) {
                const f32x4 x = acc[I][2 * jp], y = acc[I][2 * jp + 1];
                u[2 * jp] = Tr::pack2(x[0], x[1]);
                u[2 * jp + 1] = Tr::pack2(x[2], x[3]);
                v[2 * jp] = Tr::pack2(y[0], y[1]);
                v[2 * jp + 1] = Tr::pack2(y[2], y[3]);
            }
            asm volatile("s_nop 1\n\t"
                         "v_permlane16_swap_b32 %0, %8\n\tv_permlane16_swap_b32 %1, %9\n\tv_permlane16_swap_b32 %2, %10\n\t"
                         "v_permlane16_swap_b32 %3, %11\n\tv_permlane16_swap_b32 %4, %12\n\tv_permlane16_swap_b32 %5, %13\n\t"
                         "v_permlane16_swap_b32 %6, %14\n\tv_permlane16_swap_b32 %7, %15"
                         : "+v"(u[0]), "+v"(u[1]), "+v"(u[2]), "+v"(u[3]), "+v"(u[4]), "+v"(u[5]), "+v"(u[6]), "+v"(u[7]), "+v"(v[0]), "+v"(v[1]),
                           "+v"(v[2]), "+v"(v[3]), "+v"(v[4]), "+v"(v[5]), "+v"(v[6]), "+v"(v[7]));
            // (asm: a store the compiler knows about makes it guard the tile loop with s_waitcnt vmcnt(0), i.e. wait out the next tile's
            // pieces; a store has read its registers once it has issued. The first store reads what swaps 0 and 1 wrote, six swaps back.)
            const u32x4_t d0 = u32x4_t{u[0], u[1], v[0], v[1]}, d1 = u32x4_t{u[2], u[3], v[2], v[3]};
            const u32x4_t d2 = u32x4_t{u[4], u[5], v[4], v[5]}, d3 = u32x4_t{u[6], u[7], v[6], v[7]};
            const unsigned cl = c_lane; // (copies: clang does not capture a variable a generic lambda names only in an asm operand)
            asm volatile("global_store_dwordx4 %0, %1, %5" W128_ST_MOD "\n\tglobal_store_dwordx4 %0, %2, %5 offset:64" W128_ST_MOD "\n\t"
                         "global_store_dwordx4 %0, %3, %5 offset:128" W128_ST_MOD "\n\tglobal_store_dwordx4 %0, %4, %5 offset:192" W128_ST_MOD "\n\ts_nop 1" ::"v"(cl),
                         "v"(d0), "v"(d1), "v"(d2), "v"(d3), "s"(cb)
                         : "memory");
        });
        if constexpr (kDiag) tc_store = __builtin_amdgcn_s_memtime();
    };
    // Every tile but the workgroup's last: the k-step stream runs through into the next tile, whose first pieces stay in flight under
    // the epilogue. The LAST tile is separate code behind the loop, not a branch inside it: the 256 accumulator registers meet at no
    // join but the K loops' own back edges (hipcc answers a join of two inline-asm paths with hundreds of copies and spills).
    for (; tile + grid < total; tile += grid) {
        {
            long dummy;
            decode(tile + grid, na, nb, dummy);
            na = uniform(na);
            nb = uniform(nb);
        }
        block(std::true_type{}, nkb == 1);
        for (int kb = 1; kb < nkb; ++kb) block(std::false_type{}, kb == nkb - 1);
        epilogue(k0);
        const char *ta, *tb;
        decode(tile + grid, ta, tb, c_elem);
    }
    // The last tile: step 0 of its last block requests the last M/N-major pieces, the final block behind it requests nothing.
    if (nkb == 1) {
        step(k0, std::true_type{}, false);
        final_block();
        epilogue(std::integral_constant<int, 7>{});
    } else {
        block(std::true_type{}, false);
        for (int kb = 1; kb < nkb - 1; ++kb) block(std::false_type{}, false);
        step(k0, std::false_type{}, false);
        final_block();
        epilogue(std::integral_constant<int, 7>{});
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // the last tile's stores (and, where dbg & 1 dropped them, nothing)
    if constexpr (kDiag) {
        const bool lane0 = w == 0 && __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)) == 0;
        if ((pw.dbg & 16) && lane0) { // tools/gemm_tail_ledger.py
            unsigned long long *d = pw.stamps + (size_t)blockIdx.x * kStamps;
            d[0] = tc0, d[1] = tc_first, d[2] = tc_mfma, d[3] = tc_store, d[4] = __builtin_amdgcn_s_memtime();
            d[5] = tr0, d[6] = tr_mfma, d[7] = __builtin_amdgcn_s_memrealtime();
        }
        if ((pw.dbg & 8) && blockIdx.x == 0 && lane0) { // tools/gemm_wave128.py --clock: the K loops' length on the core clock and on the
            unsigned long long *d = (unsigned long long *)p.c; // 100 MHz reference, over the first 16 bytes of C
            d[0] = __builtin_amdgcn_s_memtime() - tc_first;
            d[1] = __builtin_amdgcn_s_memrealtime() - tr_first;
        }
    }
}

template <typename Tr> static int launch_t(infiniRocmRuntime_t rt, GemmArgs p, bool akm, bool bkm) {
    WArgs w;
    p.tiles_m = p.m / 256;
    p.tiles_n = p.n / 256;
    w.g = p;
    w.total_tiles = p.tiles_m * p.tiles_n * p.batch;
    const char *dbg = diag_getenv("IROCM_W128_DBG"); // (diagnostic build only: diag.h)
    w.dbg = dbg ? atoi(dbg) : 0;
    w.stamps = nullptr;
    const unsigned grid = (unsigned)(w.total_tiles < rt->num_cu ? w.total_tiles : rt->num_cu);
    if (w.dbg & 16) {
        void *ws = nullptr;
        if (int st = infini_rocm_workspace(rt, (size_t)grid * kStamps * sizeof(unsigned long long), &ws))
            return st;
        w.stamps = (unsigned long long *)ws;
    }
    return with_layout(akm, bkm, [&](auto ak, auto bk) -> int {
        auto kern = gemm128w_kernel<Tr, decltype(ak)::value, decltype(bk)::value>;
        IROCM_LDS_ATTR(kern, kLds, rt);
        hipLaunchKernelGGL(kern, dim3(grid), dim3(256), kLds, rt->stream, w);
        IROCM_LAUNCH_CHECK("gemm128w");
        return INFINI_ROCM_OK;
    });
}

int launch_gemm128w(infiniRocmRuntime_t rt, int dtype, const GemmArgs &p, bool akm, bool bkm) {
    if (!wave128_supported(gemm_problem(p, dtype, akm, bkm)))
        IROCM_FAIL(INFINI_ROCM_UNSUPPORTED, "gemm128w: this problem is outside the four-wave kernel's contract (gemm_route.h)");
    return dtype == INFINI_DT_BF16 ? launch_t<Bf16Traits>(rt, p, akm, bkm) : launch_t<F16Traits>(rt, p, akm, bkm);
}

} // namespace g128w
} // namespace irocm
