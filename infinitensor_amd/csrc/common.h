// Shared host-side plumbing for the C-ABI implementation (gfx950 only; no CUDA compatibility paths).
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <hip/hip_fp16.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "infini_rocm.h"

namespace irocm {

// ---- thread-local error message ---------------------------------------------------------------
void set_error(const char *fmt, ...);

#define IROCM_FAIL(code, ...)                                                                      \
    do {                                                                                           \
        ::irocm::set_error(__VA_ARGS__);                                                           \
        return (code);                                                                             \
    } while (0)

#define IROCM_CHECK_ARG(cond, ...)                                                                 \
    do {                                                                                           \
        if (!(cond))                                                                               \
            IROCM_FAIL(INFINI_ROCM_INVALID_ARGUMENT, __VA_ARGS__);                                 \
    } while (0)

#define IROCM_HIP(expr)                                                                            \
    do {                                                                                           \
        hipError_t _e = (expr);                                                                    \
        if (_e != hipSuccess)                                                                      \
            IROCM_FAIL(_e == hipErrorOutOfMemory ? INFINI_ROCM_OUT_OF_MEMORY : INFINI_ROCM_HIP_ERROR, \
                       "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
    } while (0)

// Check the launch that was just enqueued (reference: checkCudaError(cudaGetLastError()),
// src/cuda/cuda_runtime.cc:198).
#define IROCM_LAUNCH_CHECK(what)                                                                   \
    do {                                                                                           \
        hipError_t _e = hipGetLastError();                                                         \
        if (_e != hipSuccess)                                                                      \
            IROCM_FAIL(INFINI_ROCM_HIP_ERROR, "launch of %s failed: %s", what,                     \
                       hipGetErrorString(_e));                                                     \
    } while (0)

inline size_t dtype_size(int dt) {
    switch (dt) {
    case INFINI_DT_F32: case INFINI_DT_I32: case INFINI_DT_U32: return 4;
    case INFINI_DT_U8: case INFINI_DT_I8: case INFINI_DT_BOOL: return 1;
    case INFINI_DT_U16: case INFINI_DT_I16: case INFINI_DT_F16: case INFINI_DT_BF16: return 2;
    case INFINI_DT_I64: case INFINI_DT_U64: case INFINI_DT_F64: return 8;
    default: return 0;
    }
}

inline const char *dtype_name(int dt) {
    switch (dt) {
    case INFINI_DT_F32: return "Float32";
    case INFINI_DT_U8: return "UInt8";
    case INFINI_DT_I8: return "Int8";
    case INFINI_DT_U16: return "UInt16";
    case INFINI_DT_I16: return "Int16";
    case INFINI_DT_I32: return "Int32";
    case INFINI_DT_I64: return "Int64";
    case INFINI_DT_BOOL: return "Bool";
    case INFINI_DT_F16: return "Float16";
    case INFINI_DT_F64: return "Double";
    case INFINI_DT_U32: return "UInt32";
    case INFINI_DT_U64: return "UInt64";
    case INFINI_DT_BF16: return "BFloat16";
    default: return "Unknown";
    }
}

// hipFuncSetAttribute(MaxDynamicSharedMemorySize) is a per-DEVICE property of a kernel: one flag per (call site,
// device), set under a lock, with the runtime's device made current first (a second RocmRuntime on another GPU of the
// same process gets its own attribute call; launches below it then run with that device current).
struct DeviceOnce {
    std::mutex mu;
    uint64_t done = 0;
};
#define IROCM_LDS_ATTR(kern, bytes, rt)                                                            \
    do {                                                                                           \
        static ::irocm::DeviceOnce _once;                                                          \
        IROCM_HIP(hipSetDevice((rt)->device));                                                     \
        std::lock_guard<std::mutex> _lk(_once.mu);                                                 \
        const uint64_t _bit = 1ull << ((rt)->device & 63);                                         \
        if (!(_once.done & _bit)) {                                                                \
            IROCM_HIP(hipFuncSetAttribute((const void *)(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)(bytes))); \
            _once.done |= _bit;                                                                    \
        }                                                                                          \
    } while (0)

// Gelu for a GEMM epilogue WITHOUT transcendentals (round 4): erf(x / sqrt 2) ~ xc * P(xc^2) on |x| <= 4 with P an odd-minimax
// fit of degree 13 (7 coefficients, weighted by the 0.5 |x| the error is multiplied with; P(16) * 4 = 1 + 2e-5 so that the
// clamp to [-1, 1] returns EXACTLY +-1 from |x| = 4 on: x for large positive inputs, 0 for large negative ones, +-inf / NaN
// carried by the final fma). Max |error| against 0.5 x (1 + erf(x / sqrt 2)): 1.96e-4 < 2^-12 inside the fit range (fp32
// Horner, tools/gelu_fit.py), 1.3e-4 from the truncation at x < -4. That is an ABSOLUTE bound: below half an f16 ulp only where
// |gelu(x)| >= 0.25; in the negative tail the value shrinks towards the bound — relative error <= 2.5 % on [-3, -2], <= 12 % on
// [-3.5, -3], of the order of the value itself below -3.5 — tens of f16 ulps away from the erf form (the round-4 advisor's finding; the contract in include/infini_rocm.h states it). The standalone
// 16-bit Gelu uses the SAME function on purpose: MatMul -> Gelu is bit-identical fused or unfused (the fuzzers assert that). 12 plain fp32 VALU operations (10 of them mul / fma that hipcc pairs into v_pk_* forms) against 14 + v_rcp +
// v_exp (quarter-rate each) of gelu_erf_as: the FFN1 epilogue of BERT was VALU-bound on exactly those.
__device__ inline float gelu_poly(float v) {
    const float xc = __builtin_amdgcn_fmed3f(v, -4.0f, 4.0f);
    const float u = xc * xc;
    float p = fmaf(4.563833937e-08f, u, -3.201370338e-06f);
    p = fmaf(p, u, 9.599663829e-05f);
    p = fmaf(p, u, -1.628826435e-03f);
    p = fmaf(p, u, 1.754786860e-02f);
    p = fmaf(p, u, -1.291485240e-01f);
    p = fmaf(p, u, 7.957602372e-01f);
    const float e = __builtin_amdgcn_fmed3f(xc * p, -1.0f, 1.0f);
    const float hx = 0.5f * v;
    return fmaf(hx, e, hx);
}

constexpr int kNumXcd = 8; // MI355X: 8 XCDs, block b is dispatched to XCD b % 8 (speed only)

inline int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

} // namespace irocm

// The runtime object behind infiniRocmRuntime_t.
struct infiniRocmRuntime {
    int device = 0;
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr; // the stream kernels launch on (own or adopted)
    void *workspace = nullptr;
    size_t workspace_bytes = 0;
    std::vector<void *> retired;  // outgrown workspace blocks, kept alive for the graph execs that captured them
    uint64_t workspace_epoch = 0; // bumped whenever `workspace` changes
    bool capturing = false;
    int matmul_variant = -1;
    int matmul_compute_type = 0; // 0 exact fp32 products, 1 bf16, 2 fp16 (fp32 MatMul only; MatmulObj::getComputeType())
    int last_matmul_variant = -1; // the variant the most recent matmul call actually launched
    const char *last_conv_route = "none"; // which implementation the most recent conv2d call launched
    char last_rowop_route[40] = "none"; // the route of the most recent row-op call (rowops_route.h: rowop_route_name)
    int conv_variant = -1;
    // conv weights declared constant by the caller: their re-packed images are cached (WCacheEntry) instead of rebuilt
    int conv_const_weights = 0;
    struct WCacheEntry {
        const void *src;   // the operator's weight tensor (FCRS)
        size_t src_bytes;
        int f, c, rs, kind; // kind 0: [RS][F][C], 1: [F][Kpad]
        void *packed;
        size_t packed_bytes;
    };
    std::vector<WCacheEntry> wcache;
    uint64_t wcache_epoch = 0;      // bumped whenever an entry is dropped (captured graphs may still address it)
    hipStream_t side_stream = nullptr; // non-captured helper stream (packs weights while the main stream records)
    void *zeros = nullptr; // 256 zero bytes (K-tail source for the LDS-DMA GEMM staging)
    // hand-off flag words of kernels whose workgroups exchange data inside a launch (the split-K form of the conv tap GEMM):
    // zeroed at creation, every kernel leaves them zero (each word's single consumer resets it)
    unsigned *sync_flags = nullptr;
    static constexpr size_t kSyncFlagWords = 32768;
    // A wait on such a flag is bounded (2 s): a partner that never shows up ends the kernel with wrong sums instead of a hung GPU.
    // The waiting wave then sets this word — pinned HOST memory mapped into the device, so infini_rocm_runtime_sync reads it
    // without a copy — and the sync that follows fails, re-zeroes every flag (the late producer may still have set one) and clears it.
    // The residency argument behind these exchanges (grid <= CUs, so every slice of a tile is running) holds for kernels of ONE
    // stream; a kernel that spins on another stream (comm_stream's direct-transport collectives, side_stream packs do not spin)
    // can hold the CUs a slice needs — that is what the time limit and this word are for.
    volatile unsigned *sync_err_host = nullptr; // host view
    unsigned *sync_err_dev = nullptr;           // device view of the same word
    int num_cu = 256;
    void *comm = nullptr; // rcclComm_t, owned by comm.hip
    void *dcomm = nullptr; // irocm::DirectComm (the hand-written IPC / xGMI transport), owned by comm_direct.hip
    int dcomm_dirty = 0;   // a direct-transport collective was enqueued since the error word was last read (runtime_sync reads it)
    int comm_algo = 0;     // 0: RCCL when it is initialised, else the direct transport; 1: the direct transport
    int comm_world = 1, comm_rank = 0;
    // overlapped collectives (comm.hip: *_async / comm_join): a second stream and a small ring of fork / join events
    hipStream_t comm_stream = nullptr;
    std::vector<hipEvent_t> comm_events;
    size_t comm_event_next = 0;
    int comm_pending = 0; // async collectives issued since the last join
    std::mutex mu;
};

namespace irocm {
// packed-weight cache (runtime.hip)
const void *wcache_lookup(infiniRocmRuntime *rt, const void *src, int f, int c, int rs, int kind);
// allocates the packed buffer and tells on which stream to launch the pack kernel (the runtime stream, or the side stream
// while the runtime stream is capturing); wcache_commit makes the image usable (waits for the side stream if it was used)
int wcache_insert(infiniRocmRuntime *rt, const void *src, size_t src_bytes, int f, int c, int rs, int kind, size_t packed_bytes,
                  void **packed, hipStream_t *stream);
int wcache_commit(infiniRocmRuntime *rt, hipStream_t stream);
// removes the entry whose packed image is `packed` (a pack that failed after wcache_insert); the buffer is retired
void wcache_forget(infiniRocmRuntime *rt, const void *packed);
// drops every entry whose SOURCE overlaps [ptr, ptr + bytes); the packed buffers are retired, not freed
void wcache_invalidate(infiniRocmRuntime *rt, const void *ptr, size_t bytes);
} // namespace irocm

namespace irocm {
// the hand-written one-hop transport (comm_direct.hip); all on the given stream
int direct_init(infiniRocmRuntime *rt, const char *name, int world, int rank);
int direct_destroy(infiniRocmRuntime *rt);
int direct_check(infiniRocmRuntime *rt);
int direct_all_reduce(infiniRocmRuntime *rt, int op, int dtype, const void *x, void *y, int64_t count, hipStream_t st);
int direct_reduce_scatter(infiniRocmRuntime *rt, int dtype, const void *x, void *y, int64_t count, hipStream_t st);
int direct_all_gather(infiniRocmRuntime *rt, const void *x, void *y, size_t bytes, hipStream_t st);
int direct_broadcast(infiniRocmRuntime *rt, const void *x, void *y, size_t bytes, int root, hipStream_t st);
int direct_send(infiniRocmRuntime *rt, const void *x, size_t bytes, int peer, hipStream_t st);
int direct_recv(infiniRocmRuntime *rt, void *y, size_t bytes, int peer, hipStream_t st);
} // namespace irocm

struct infiniRocmGraph {
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
};

struct infiniRocmEvent {
    hipEvent_t ev = nullptr;
};
