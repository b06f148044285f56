"""The four-wave GEMM's two tile endings (gemm128w.hip, variant "wave128"). A workgroup's LAST tile ends in the final block: behind step
0 of its last block of four k-steps nothing is requested any more, the last three k-steps run row-major (per accumulator row the
3 x 8 MFMAs of k-steps L-3 .. L-1) and a finished row's converts, swaps and stores are issued between the next row's MFMAs; every other
tile streams through into the next one and stores behind its last MFMA, row by row in batches.

Inputs are selectors: op(A) is one-hot in k — row m has a single 1 at k = sigma(m), and sigma visits every k-step of 32, the last four
in particular — and op(B)[k, n] is a small integer, exact in bf16 and f16 and never 0, that differs between neighbouring k and n. Then
C[m, n] = B[sigma(m), n] EXACTLY: a dropped k-step gives 0, a row retired before its last k-step too, a fragment from the wrong stage
or register slot or a store at the wrong row / column another integer. One N(0,1) case per shape is held to tests/test_gpu_matmul.py's
per-element bound against the fp64 product. (No bit-equality test against a forced stream-through ending: the library keeps no such
switch. The final block adds into each accumulator in the K loop's own order, ascending k; tools/gemm_ab_libs.py compares the bits of
two builds and found the parent's on 4096^3, 8192 x 4096 x 4096 and 16384 x 3072 x 768: profiles/gemm128w_final_block_ab.txt.)
C is written into the middle of a buffer pre-filled with a sentinel: every element of C must have changed, every guard element not."""
import pytest
import torch

from infinitensor_amd import ops

pytestmark = pytest.mark.gpu

SHAPES = [
    # b, m, n, k
    (1, 256, 256, 128),    # K is one block: the final block follows the prologue directly
    (1, 256, 256, 256),    # one stream-through block, then the final block
    (1, 256, 512, 384),    # two blocks, then the final block; two workgroups
    (1, 4096, 4352, 256),  # 272 tiles on 256 CUs: sixteen workgroups run a stream-through tile and then their last tile
    (3, 512, 256, 384),    # batch strides
]
LAYOUTS = [(False, False), (False, True), (True, False), (True, True)]
DTYPES = [torch.bfloat16, torch.float16]
GUARD = 4096     # elements in front of and behind C
SENTINEL = -776.0  # exact in bf16 and f16; no selector result (1 .. 251) equals it


def sigma(b, m, k):
    """[b, m] -> k index of the row's single 1: row r sits in k-step r % (k / 32), so every k-step is hit by every 16-row block."""
    steps = k // 32
    r = torch.arange(m, device="cuda").unsqueeze(0) + 5 * torch.arange(b, device="cuda").unsqueeze(1)
    s = (r % steps) * 32 + (r // steps * 7 + r) % 32
    assert set((s // 32).flatten().tolist()) == set(range(steps))
    return s


def selector_inputs(b, m, n, k, ta, tb, dtype):
    s = sigma(b, m, k)
    a = torch.zeros(b, m, k, device="cuda", dtype=dtype)
    a.scatter_(2, s.unsqueeze(2), 1.0)
    kk = torch.arange(k, device="cuda").view(1, k, 1)
    nn = torch.arange(n, device="cuda").view(1, 1, n)
    bb = torch.arange(b, device="cuda").view(b, 1, 1)
    bm = ((kk * 131 + nn * 7 + bb * 3) % 251 + 1).to(dtype)  # integers 1 .. 251: exact in both formats
    want = torch.gather(bm, 1, s.unsqueeze(2).expand(b, m, n))
    return a, bm, want


def run_wave128(rt, a, bm, ta, tb, shape, dtype):
    """a [b, m, k], bm [b, k, n] (logical); stored transposed where the layout says so. Returns C and checks the guards."""
    b, m, n, k = shape
    da = a.transpose(1, 2).contiguous() if ta else a.contiguous()
    db = bm.transpose(1, 2).contiguous() if tb else bm.contiguous()
    if b == 1:
        da, db = da[0], db[0]
    buf = torch.full((2 * GUARD + b * m * n,), SENTINEL, device="cuda", dtype=dtype)
    out = buf[GUARD:GUARD + b * m * n].view((b, m, n) if b > 1 else (m, n))
    ops.set_matmul_variant(rt, ops.matmul_variants().index("wave128"))
    try:
        ops.matmul(rt, da, db, None, ta, tb, out=out)
        assert ops.matmul_last_variant(rt) == "wave128"
    finally:
        ops.set_matmul_variant(rt, -1)
    rt.sync()
    assert bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[GUARD + b * m * n:] == SENTINEL).all()), "a store outside C"
    c = out.view(b, m, n)
    untouched = int((c == SENTINEL).sum().item())
    assert untouched == 0, f"{untouched} elements of C were never stored"
    return c


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("ta,tb", LAYOUTS)
@pytest.mark.parametrize("shape", SHAPES)
def test_wave128_tile_endings_select_exactly(rt, shape, ta, tb, dtype):
    b, m, n, k = shape
    a, bm, want = selector_inputs(b, m, n, k, ta, tb, dtype)
    c = run_wave128(rt, a, bm, ta, tb, shape, dtype)
    wrong = c != want
    if bool(wrong.any()):
        idx = wrong.nonzero()[0].tolist()
        ib, im, in_ = idx
        raise AssertionError(f"{int(wrong.sum().item())} wrong elements; first at {idx}: got {c[ib, im, in_].item()}, want {want[ib, im, in_].item()} "
                             f"(sigma = {sigma(b, m, k)[ib, im].item()}, k-step {sigma(b, m, k)[ib, im].item() // 32} of {k // 32})")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("ta,tb", LAYOUTS)
@pytest.mark.parametrize("shape", SHAPES)
def test_wave128_tile_endings_normal_operands(rt, shape, ta, tb, dtype):
    b, m, n, k = shape
    g = torch.Generator(device="cuda").manual_seed(hash((shape, ta, tb)) % 2 ** 31)
    a = torch.randn(b, m, k, device="cuda", generator=g).to(dtype)
    bm = torch.randn(b, k, n, device="cuda", generator=g).to(dtype)
    c = run_wave128(rt, a, bm, ta, tb, shape, dtype)
    a64, b64 = a.double(), bm.double()
    want = a64 @ b64
    # the per-element bound of tests/test_gpu_matmul.py: one storage ulp of the result plus 2^-17 of the element's sum of magnitudes
    tol = 2.0 ** -7 if dtype == torch.bfloat16 else 2.0 ** -10
    err = (c.double() - want).abs()
    bound = tol * want.abs() + 2.0 ** -17 * (a64.abs() @ b64.abs())
    over = err > bound
    assert not bool(over.any()), f"{int(over.sum().item())} elements over the bound; max err {err.max().item()} at {over.nonzero()[0].tolist()}"
