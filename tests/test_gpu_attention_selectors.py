"""Prefill attention (csrc/attention.hip) and the decode step (csrc/attention_kvcache.hip) on the selector inputs of
tests/attention_cases.py — one key, or an exact pair, carries the whole weight of a query row, so one dropped, duplicated or
wrongly admitted key is an O(1) error — and on the random inputs of tests/test_gpu_attention.py, every element against the
bound  u |want| + (2 u + 2^-16) A  (f32 decode: u |want| + 2^-17 A) derived in attention_cases.py instead of an allclose.
tests/test_attention_selectors_cpu.py shows on the oracle alone that these inputs and this bound catch each of the mistakes
they are meant for by a factor of at least 8.

Worst err / bound per (kernel, dtype, D); 1.0 is the limit. Every test prints its own figure as a line "worst <kernel>
<dtype> d<D> ... <ratio>" (pytest -s). NOT YET MEASURED ON AN MI355X: no GPU could be had while these tests were written, so
the table below has no GPU column; it is to be filled from the first run of this file. What stands in it is a numpy replay of
attention.hip's roundings on the selector cases (scores and sums in fp32, P rounded to the storage type, both forms of the
normaliser, one output rounding) — a statement about the bound, not about the kernel:
  prefill, selectors  f16 D=64 : replay 0.68     prefill, selectors  f16 D=128: replay 0.79
  prefill, selectors bf16 D=64 : replay 0.46     prefill, selectors bf16 D=128: replay 0.35
  prefill, random inputs; decode f32 / f16 / bf16 at D = 32 .. 256: no figure yet
"""
import numpy as np
import pytest
import torch

import attention_cases as C
from infinitensor_amd import ops
from oracle import ref_ops as R
from test_gpu_attention import CASES, MASK2D_CASES

pytestmark = pytest.mark.gpu
TD = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}


def dev(a, dt):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(TD[dt]).cuda()


def host(t):
    return t.float().cpu().numpy().astype(np.float64)


@pytest.mark.parametrize("p", C.prefill_params(), ids=C.prefill_id)
def test_prefill_selectors(rt, p):
    c = C.prefill_case(*p)
    q, k, v = (dev(a[None], c.dt) for a in (c.q, c.k, c.v))
    mask = None if c.mask is None else dev(c.mask, c.dt)
    if c.scale_kind == "div":
        y = ops.attention(rt, q, k, v, dev(np.array([c.scale_div]), c.dt), mask, c.causal, scale_is_div=True)
    else:
        y = ops.attention(rt, q, k, v, float(c.scale), mask, c.causal)
    got = host(y)[0]
    worst, idx = C.worst_ratio(got, c.want, c.bound)
    print(f"worst prefill {c.dt} d{c.d} causal{int(c.causal)} mask{c.mask_form} {worst:.3f} at {idx} ({C.prefill_id(p)})")
    C.assert_within(got, c.want, c.bound, C.prefill_id(p))
    assert (got[c.dead] == 0).all()  # fully masked rows produce 0


def same_bits(a, b):
    ints = {2: torch.int16, 4: torch.int32}[a.element_size()]
    return torch.equal(a.contiguous().view(ints), b.contiguous().view(ints))


def _random_inputs(case_key, shapes):
    rng = np.random.default_rng(abs(hash(case_key)) % 2 ** 32)
    return rng, [rng.standard_normal(s).astype(np.float32) for s in shapes]


@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("case", CASES)
def test_prefill_random_inputs_per_element(rt, case, dt):
    """The inputs of test_gpu_attention.py::test_attention_vs_oracle (same generator, same order of draws)."""
    b, h, sq, sk, d, use_mask, causal = case
    rng, (q, k, v) = _random_inputs(case, [(b, h, sq, d), (b, h, sk, d), (b, h, sk, d)])
    scale = 1.0 / np.sqrt(d)
    mask = None
    if use_mask:
        mask = np.where(rng.random((b, sk)) < 0.8, 0.0, -10000.0).astype(np.float32)
        mask[:, 0] = 0.0
    y = ops.attention(rt, dev(q, dt), dev(k, dt), dev(v, dt), scale, None if mask is None else dev(mask, dt), causal)
    want, bound = C.random_reference(dt, R.round_to(q, dt), R.round_to(k, dt), R.round_to(v, dt), scale,
                                     None if mask is None else R.round_to(mask, dt)[:, None, None, :], causal)
    worst, idx = C.worst_ratio(host(y), want, bound)
    print(f"worst random {dt} d{d} causal{int(causal)} mask{int(use_mask)} {worst:.3f} at {idx} ({case})")
    C.assert_within(host(y), want, bound, str(case))


@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("case", MASK2D_CASES)
def test_prefill_random_full_mask_per_element(rt, case, dt):
    """The inputs of test_gpu_attention.py::test_attention_full_additive_mask."""
    b, h, sq, sk, d, mb, mh = case
    rng, (q, k, v) = _random_inputs(case, [(b, h, sq, d), (b, h, sk, d), (b, h, sk, d)])
    m = (0.5 * rng.standard_normal((mb, mh, sq, sk))).astype(np.float32)
    m = np.where(np.tril(np.ones((sq, sk), dtype=bool), k=sk - sq), m, -10000.0).astype(np.float32)
    m[..., 0] = np.minimum(m[..., 0], 0) * 0
    scale = 1.0 / np.sqrt(d)
    y = ops.attention(rt, dev(q, dt), dev(k, dt), dev(v, dt), scale, dev(m.reshape(mb * mh, sq, sk), dt))
    want, bound = C.random_reference(dt, R.round_to(q, dt), R.round_to(k, dt), R.round_to(v, dt), scale, R.round_to(m, dt), False)
    worst, idx = C.worst_ratio(host(y), want, bound)
    print(f"worst random {dt} d{d} causal0 mask2 {worst:.3f} at {idx} ({case})")
    C.assert_within(host(y), want, bound, str(case))


@pytest.mark.parametrize("split", C.DECODE_SPLITS)  # (varies fastest: splits with the same chunks share a built case)
@pytest.mark.parametrize("pos,ms", C.DECODE_POSITIONS)
@pytest.mark.parametrize("d", ops.KVCACHE_HEAD_DIMS)
@pytest.mark.parametrize("dt", ["f32", "f16", "bf16"])
def test_decode_selectors(rt, dt, d, pos, ms, split, monkeypatch):
    """IROCM_KVCACHE_SPLIT forces the number of chunks (0: the element-wise one-workgroup kernel); the targets sit on key 0, the
    new key, the one before it and both ends of every chunk of that split. After each call: the output within the bound, cache
    row `pos` the new k / v bit for bit, every other row — the ones that hold V = 1000 included — untouched."""
    monkeypatch.setenv("IROCM_KVCACHE_SPLIT", str(split))
    chunk_len = C.decode_chunk_len(pos + 1, split, ops.kvcache_keys_per_iteration(TD[dt], d))
    p = torch.tensor([pos], dtype=torch.int32).cuda()
    for n_, r in enumerate(C.decode_case(dt, d, pos, ms, chunk_len)):
        kc, vc, q, kn, vn = (dev(a[None], dt) for a in (r.kc, r.vc, r.q, r.kn, r.vn))
        kc0, vc0 = kc.clone(), vc.clone()
        y = ops.attention_kvcache(rt, kc, vc, q, kn, vn, p)
        got = host(y)[0]
        worst, idx = C.worst_ratio(got, r.want, r.bound)
        print(f"worst decode {dt} d{d} split{split} {worst:.3f} at {idx} (pos {pos} of {ms}, call {n_}, g {r.g})")
        C.assert_within(got, r.want, r.bound, f"decode {dt} d{d} pos {pos} split {split} call {n_}")
        assert same_bits(kc[:, :, pos], kn[:, :, 0]) and same_bits(vc[:, :, pos], vn[:, :, 0])
        assert same_bits(kc[:, :, :pos], kc0[:, :, :pos]) and same_bits(vc[:, :, :pos], vc0[:, :, :pos])
        assert same_bits(kc[:, :, pos + 1:], kc0[:, :, pos + 1:]) and same_bits(vc[:, :, pos + 1:], vc0[:, :, pos + 1:])
