"""AttentionKVCache decode steps at head dims 32, 64 and 96 (csrc/attention_kvcache.hip): narrow rows put fewer lanes on a key,
so a workgroup takes more keys per iteration and the chunk arithmetic of the split kernel moves with it. Oracle:
oracle/ref_ops.py::attention_kvcache on the host copies of the rounded inputs; tolerances: the operator's own
(test_gpu_attention.py::test_attention_kvcache_vs_oracle), for rtol and atol alike — shorter rows only shorten the sums. Every
case also compares both caches bit for bit with the oracle's appended caches: nothing but row n - 1 may be touched."""
import ctypes
import functools
from pathlib import Path

import numpy as np
import pytest
import torch

from infinitensor_amd import lib, ops
from infinitensor_amd._lib import check
from oracle import ref_ops as R

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).resolve().parent / "golden" / "kvcache_d128_parent.npy"
DTS = [(torch.float32, 1e-5), (torch.float16, 2e-3), (torch.bfloat16, 1.6e-2)]
DT_IDS = ["f32", "f16", "bf16"]
WIDTHS = [32, 64, 96]
B_, H_ = 2, 3
DT_I32, DT_U32, DT_I64, DT_F16 = 6, 12, 7, 10  # include/infini_rocm.h


def host(t):
    return t.float().cpu().numpy().astype(np.float64)


@functools.lru_cache(maxsize=2)
def _case(d, dt, pos, ms):
    """Rounded host inputs and the oracle's answer for one (width, dtype, position, capacity): computed once, shared by the
    splits that run it, never modified (every test uploads fresh device copies)."""
    rng = np.random.default_rng(1000 * d + 7 * pos + ms)
    arrs = [torch.from_numpy(rng.standard_normal(s).astype(np.float32)).to(dt)
            for s in [(B_, H_, ms, d), (B_, H_, ms, d), (B_, H_, 1, d), (B_, H_, 1, d), (B_, H_, 1, d)]]
    want = R.attention_kvcache(*(host(a) for a in arrs), pos)
    return arrs, want


def run_and_check(rt, d, dt, tol, pos, ms, pos_dtype=torch.int32):
    arrs, (want, kc_w, vc_w) = _case(d, dt, pos, ms)
    kc, vc, q, k, v = (a.cuda() for a in arrs)
    p = torch.tensor([[pos]], dtype=pos_dtype).cuda()
    y = ops.attention_kvcache(rt, kc, vc, q, k, v, p)
    err = np.abs(host(y) - want).max()
    print(f"d {d} {dt} pos {pos} max_seq {ms}: max abs error {err:.3e} (tolerance {tol})")
    assert np.allclose(host(y), want, rtol=tol, atol=tol), err
    assert np.array_equal(host(kc), kc_w) and np.array_equal(host(vc), vc_w)  # appended in place, nothing else touched


@pytest.mark.parametrize("dt,tol", DTS, ids=DT_IDS)
@pytest.mark.parametrize("d", WIDTHS)
@pytest.mark.parametrize("pos,ms", [(0, 1), (5, 16), (16, 17), (100, 128), (511, 512)])
def test_kvcache_narrow_heads_vs_oracle(rt, dt, tol, d, pos, ms):
    """The heuristic split (no test hook), the cases of test_attention_kvcache_vs_oracle at the new widths."""
    run_and_check(rt, d, dt, tol, pos, ms)


# positions relative to K, the keys a workgroup takes per iteration: (pos, max_seq) as functions of K
EDGES = {
    "0": lambda K: (0, 64),
    "K-2": lambda K: (K - 2, K),
    "K-1": lambda K: (K - 1, K),
    "K": lambda K: (K, K + 16),
    "3K+1": lambda K: (3 * K + 1, 4 * K + 8),
    "130of4096": lambda K: (130, 4096),  # empty chunks at split 16
}


@pytest.mark.parametrize("split", [0, 1, 2, 5, 16])  # (the top decorator varies fastest: the five splits of a case share its oracle)
@pytest.mark.parametrize("edge", list(EDGES))
@pytest.mark.parametrize("d", WIDTHS)
@pytest.mark.parametrize("dt,tol", DTS, ids=DT_IDS)
def test_kvcache_narrow_heads_chunk_edges(rt, dt, tol, d, edge, split, monkeypatch):
    """IROCM_KVCACHE_SPLIT forces the number of chunks G (0 = the element-wise one-workgroup kernel, which must append the new key
    as well). K, the keys a workgroup takes per iteration in that build, comes from the module: ops.kvcache_keys_per_iteration
    (256 threads / lanes per key x 4 keys per group, the rule of csrc/attention_kvcache.hip::kv_lpk) — 64 to 256 for these widths.
    Chunk lengths are rounded to K, so the positions sit on either side of one iteration, of one chunk boundary at every G, and far
    below the capacity (chunks without a key)."""
    K = ops.kvcache_keys_per_iteration(dt, d)
    assert K in (64, 128, 256) and 256 % (K // 4) == 0
    pos, ms = EDGES[edge](K)
    monkeypatch.setenv("IROCM_KVCACHE_SPLIT", str(split))
    run_and_check(rt, d, dt, tol, pos, ms, torch.int64)


def call_abi(rt, dtype, kc, vc, q, k, v, pos_dtype, p, out, bh, ms, d):
    check(lib().infini_rocm_attention_kvcache(rt.handle, dtype, *(ctypes.c_void_p(t.data_ptr()) for t in (kc, vc, q, k, v)),
                                              pos_dtype, ctypes.c_void_p(p.data_ptr()), ctypes.c_void_p(out.data_ptr()), bh, ms, d))


@pytest.mark.parametrize("pos_dtype", ["int32", "uint32", "int64"])
def test_kvcache_d64_position_dtypes(rt, pos_dtype):
    """int32 and int64 through ops; uint32 through the C ABI on the bits of an int32 tensor (torch storage for U32)."""
    d, dt, tol, pos, ms = 64, torch.float16, 2e-3, 300, 512
    if pos_dtype != "uint32":
        return run_and_check(rt, d, dt, tol, pos, ms, getattr(torch, pos_dtype))
    arrs, (want, kc_w, vc_w) = _case(d, dt, pos, ms)
    kc, vc, q, k, v = (a.cuda() for a in arrs)
    p = torch.tensor([pos], dtype=torch.int32).cuda()
    y = torch.empty_like(q)
    call_abi(rt, DT_F16, kc, vc, q, k, v, DT_U32, p, y, B_ * H_, ms, d)
    assert np.allclose(host(y), want, rtol=tol, atol=tol), np.abs(host(y) - want).max()
    assert np.array_equal(host(kc), kc_w) and np.array_equal(host(vc), vc_w)


@pytest.mark.parametrize("pos,ms", [(5, 16), (300, 512)])
def test_kvcache_d64_unaligned_tensors_take_the_elementwise_kernel(rt, pos, ms):
    """q, k and v as views 8 bytes into a larger buffer: no 16-byte vector loads are possible, the call (straight through the C
    ABI) must fall back to the element-wise kernel whatever split the heuristic would pick, and match the oracle."""
    d, dt, tol = 64, torch.float16, 2e-3
    arrs, (want, kc_w, vc_w) = _case(d, dt, pos, ms)
    kc, vc = arrs[0].cuda(), arrs[1].cuda()
    n = B_ * H_ * d
    q, k, v = (torch.zeros(n + 8, dtype=dt, device="cuda")[4:4 + n].view(B_, H_, 1, d).copy_(a) for a in arrs[2:])
    assert all(t.data_ptr() % 16 == 8 for t in (q, k, v)) and kc.data_ptr() % 16 == 0
    y = torch.empty(B_, H_, 1, d, dtype=dt, device="cuda")
    call_abi(rt, DT_F16, kc, vc, q, k, v, DT_I32, torch.tensor([pos], dtype=torch.int32).cuda(), y, B_ * H_, ms, d)
    assert np.allclose(host(y), want, rtol=tol, atol=tol), np.abs(host(y) - want).max()
    assert np.array_equal(host(kc), kc_w) and np.array_equal(host(vc), vc_w)


def test_kvcache_d64_three_decode_steps_through_reference_executor(plugin_backend):
    """The reference's graph executor on Device::ROCM (as test_gpu_plugin.py::test_attention_kvcache_through_reference_executor):
    one AttentionKVCache graph with caches [1, 4, 32, 64] f32, run three times with new q / k / v / position 0, 1, 2 and the caches
    left alone — the oracle applied step by step agrees only if each run's in-place append is still there in the next."""
    Bk = plugin_backend
    F32, U32 = 1, 12
    b, h, ms, d = 1, 4, 32, 64
    rng = np.random.default_rng(64)
    kc_h, vc_h = (rng.standard_normal((b, h, ms, d)).astype(np.float32) for _ in range(2))
    g = Bk.GraphHandler(Bk.RocmRuntime(0))
    ts = [g.tensor([b, h, ms, d], F32), g.tensor([b, h, ms, d], F32)] + [g.tensor([b, h, 1, d], F32) for _ in range(3)] + [g.tensor([1, 1], U32)]
    out = g.attentionKVCache(*ts, None)
    g.data_malloc()
    ts[0].copyin_numpy(kc_h)
    ts[1].copyin_numpy(vc_h)
    for pos in range(3):
        q, k, v = (rng.standard_normal((b, h, 1, d)).astype(np.float32) for _ in range(3))
        for t, a in zip(ts[2:], (q, k, v, np.full((1, 1), pos, np.uint32))):
            t.copyin_numpy(np.ascontiguousarray(a))
        g.run()
        want, kc_h, vc_h = R.attention_kvcache(kc_h, vc_h, q, k, v, pos)
        got = out.copyout_numpy().reshape(b, h, 1, d)
        assert np.allclose(got, want, rtol=1e-5, atol=1e-5), (pos, np.abs(got - want).max())
    assert np.array_equal(ts[0].copyout_numpy().reshape(b, h, ms, d), kc_h.astype(np.float32))
    assert np.array_equal(ts[1].copyout_numpy().reshape(b, h, ms, d), vc_h.astype(np.float32))


@pytest.mark.parametrize("d", [48, 512])
def test_kvcache_other_widths_are_still_rejected(rt, d):
    mk = lambda *s: torch.zeros(s, dtype=torch.float16, device="cuda")  # noqa: E731
    with pytest.raises(RuntimeError, match="head dim"):
        ops.attention_kvcache(rt, mk(1, 2, 8, d), mk(1, 2, 8, d), mk(1, 2, 1, d), mk(1, 2, 1, d), mk(1, 2, 1, d),
                              torch.zeros(1, dtype=torch.int32, device="cuda"))


def golden_inputs():
    """The D = 128 case of the golden file: f16, B x H = 2 x 3, position 700 of 1024; values m / 256 from integer arithmetic alone
    (exact in f16, the same on every machine and library version)."""
    def det(shape, salt):
        i = np.arange(int(np.prod(shape)), dtype=np.uint64)
        x = ((i * np.uint64(2654435761) + np.uint64(salt) * np.uint64(40503)) >> np.uint64(7)) % np.uint64(1024)
        return torch.from_numpy(((x.astype(np.float32) - 512.0) / 256.0).reshape(shape)).to(torch.float16)

    b, h, ms, d = 2, 3, 1024, 128
    shapes = [(b, h, ms, d), (b, h, ms, d), (b, h, 1, d), (b, h, 1, d), (b, h, 1, d)]
    return [det(s, salt + 1) for salt, s in enumerate(shapes)], 700


GOLDEN_SPLITS = [None, 0, 1, 5]  # the heuristic, the element-wise kernel, one chunk, five chunks + merge


def golden_outputs(rt, monkeypatch_env):
    """[len(GOLDEN_SPLITS), 2, 3, 1, 128] f16 bits (as uint16) of the outputs; monkeypatch_env(name, value or None) sets the hook."""
    arrs, pos = golden_inputs()
    outs = []
    for split in GOLDEN_SPLITS:
        monkeypatch_env("IROCM_KVCACHE_SPLIT", None if split is None else str(split))
        kc, vc, q, k, v = (a.cuda() for a in arrs)
        y = ops.attention_kvcache(rt, kc, vc, q, k, v, torch.tensor([pos], dtype=torch.int32).cuda())
        outs.append(y.cpu().numpy().view(np.uint16))
    return np.stack(outs)


def test_kvcache_d128_output_is_bit_identical_to_the_recorded_one(rt, monkeypatch):
    """tests/golden/kvcache_d128_parent.npy was recorded on an MI355X with the commit before the narrow widths were added: the
    D = 128 builds keep their template arguments and launch geometry, so every bit of the output must still be the same, through
    the heuristic split, the element-wise kernel, one chunk, and five chunks with the merge kernel."""
    def env(name, value):
        monkeypatch.delenv(name, raising=False) if value is None else monkeypatch.setenv(name, value)

    got = golden_outputs(rt, env)
    want = np.load(GOLDEN)
    assert got.shape == want.shape and got.dtype == want.dtype
    assert np.array_equal(got, want), [int((g != w).sum()) for g, w in zip(got, want)]
