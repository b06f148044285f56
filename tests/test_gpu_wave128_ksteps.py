"""The four-wave GEMM's steady K loop (gemm128w.hip, variant "wave128"): the loop `for kb = 1 .. nkb - 2` of a workgroup's last tile
and `for kb = 1 .. nkb - 1` of a stream-through tile, four k-steps per trip. In it every lane offset of the LDS-DMA pieces moves on by
ONE add in a gap of the step's MFMA stream (the gap map in the kernel's header: behind the step's last piece that reads the offset, or —
both operands K-major — in the first gaps of the following step), and the fragment reads of the next step are packed into the step's
earliest rows. tests/test_gpu_wave128_final_block.py stops at K = 384, which never takes the loop's back edge; the shapes here are the
smallest that do: K = 512 takes it once, K = 640 twice, 4096 x 4352 sends sixteen workgroups through a stream-through tile (with the
once-per-tile rewind of the offsets) and then a last tile, and a batch of two checks the batch strides. One shape more, 4096 x 4352
with K = 128, has no loop at all: there the rewind follows the prologue directly, which is where an add that the prologue leaves to
step 0 (both operands K-major) could go wrong on its own.

Inputs are selectors, and there are two of them, so that a wrong offset names its operand:
  * A-selector: op(A) is one-hot in k (row m has a single 1 at k = sigma(m)), op(B)[k, n] a small non-zero integer that differs between
    neighbouring k and n: C[m, n] = B[sigma(m), n] EXACTLY. A B piece or fragment from the wrong k-step gives another integer, an A
    piece from the wrong k-step or row a 0 or the integer of another k.
  * B-selector, the mirror: op(B) is one-hot in k (column n has a single 1 at k = sigma(n)), op(A)[m, k] the small integers:
    C[m, n] = A[m, sigma(n)] EXACTLY.
sigma visits every k-step of 32 with consecutive rows / columns, so every wave meets every k-step. One N(0,1) case per shape is held to tests/test_gpu_matmul.py's
per-element bound against the fp64 product (computed once per shape and dtype, shared by the four layouts). C is written into the
middle of a buffer pre-filled with a sentinel: every element of C must have changed, every guard element not."""
import functools

import pytest
import torch

from infinitensor_amd import ops

pytestmark = pytest.mark.gpu

SHAPES = [
    # b, m, n, k
    (1, 256, 256, 512),    # four blocks: the steady loop's back edge is taken once
    (1, 256, 256, 640),    # five blocks: twice
    (1, 4096, 4352, 512),  # 272 tiles on 256 CUs: sixteen workgroups run a stream-through tile (rewind included), then their last tile
    (2, 256, 256, 512),    # batch strides
    (1, 4096, 4352, 128),  # K is one block: a stream-through tile's rewind follows the prologue directly (no loop; the adds the prologue
                           # leaves to step 0 when both operands are K-major, then the rewind)
]
LAYOUTS = [(False, False), (False, True), (True, False), (True, True)]
DTYPES = [torch.bfloat16, torch.float16]
GUARD = 4096     # elements in front of and behind C
SENTINEL = -776.0  # exact in bf16 and f16; no selector result (1 .. 251) equals it


def sigma(b, m, k):
    """[b, m] -> k index of the row's single 1: row r sits in k-step r % (k / 32), so any k / 32 consecutive rows hit every k-step."""
    steps = k // 32
    r = torch.arange(m, device="cuda").unsqueeze(0) + 5 * torch.arange(b, device="cuda").unsqueeze(1)
    s = (r % steps) * 32 + (r // steps * 7 + r) % 32
    assert set((s // 32).flatten().tolist()) == set(range(steps))
    return s


def small_integers(b, rows, cols, dtype, k_is_row):
    """[b, rows, cols] of integers 1 .. 251 (exact in both formats, never 0) that differ between neighbouring k and m / n."""
    rr = torch.arange(rows, device="cuda").view(1, rows, 1)
    cc = torch.arange(cols, device="cuda").view(1, 1, cols)
    bb = torch.arange(b, device="cuda").view(b, 1, 1)
    kk, xx = (rr, cc) if k_is_row else (cc, rr)
    return ((kk * 131 + xx * 7 + bb * 3) % 251 + 1).to(dtype)


def a_selector_inputs(b, m, n, k, dtype):
    s = sigma(b, m, k)
    a = torch.zeros(b, m, k, device="cuda", dtype=dtype)
    a.scatter_(2, s.unsqueeze(2), 1.0)
    bm = small_integers(b, k, n, dtype, k_is_row=True)
    want = torch.gather(bm, 1, s.unsqueeze(2).expand(b, m, n))
    return a, bm, want, s


def b_selector_inputs(b, m, n, k, dtype):
    s = sigma(b, n, k)
    bm = torch.zeros(b, k, n, device="cuda", dtype=dtype)
    bm.scatter_(1, s.unsqueeze(1), 1.0)
    a = small_integers(b, m, k, dtype, k_is_row=False)
    want = torch.gather(a, 2, s.unsqueeze(1).expand(b, m, n))
    return a, bm, want, s


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


def assert_selected(c, want, s, k, which):
    wrong = c != want
    if bool(wrong.any()):
        idx = wrong.nonzero()[0].tolist()
        ib, im, in_ = idx
        sel = s[ib, im if which == "A" else in_].item()
        raise AssertionError(f"{which}-selector: {int(wrong.sum().item())} wrong elements; first at {idx}: got {c[ib, im, in_].item()}, "
                             f"want {want[ib, im, in_].item()} (sigma = {sel}, k-step {sel // 32} of {k // 32})")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("ta,tb", LAYOUTS)
@pytest.mark.parametrize("shape", SHAPES)
def test_wave128_ksteps_a_selects_exactly(rt, shape, ta, tb, dtype):
    b, m, n, k = shape
    a, bm, want, s = a_selector_inputs(b, m, n, k, dtype)
    c = run_wave128(rt, a, bm, ta, tb, shape, dtype)
    assert_selected(c, want, s, k, "A")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("ta,tb", LAYOUTS)
@pytest.mark.parametrize("shape", SHAPES)
def test_wave128_ksteps_b_selects_exactly(rt, shape, ta, tb, dtype):
    b, m, n, k = shape
    a, bm, want, s = b_selector_inputs(b, m, n, k, dtype)
    c = run_wave128(rt, a, bm, ta, tb, shape, dtype)
    assert_selected(c, want, s, k, "B")


@functools.lru_cache(maxsize=2)  # (the cases of a shape follow each other, the two dtypes alternating)
def normal_case(shape, dtype):
    """N(0,1) operands of a shape and dtype with their fp64 product and its per-element bound: computed once, shared by the layouts."""
    b, m, n, k = shape
    g = torch.Generator(device="cuda").manual_seed(1000 * SHAPES.index(shape) + DTYPES.index(dtype))
    a = torch.randn(b, m, k, device="cuda", generator=g).to(dtype)
    bm = torch.randn(b, k, n, device="cuda", generator=g).to(dtype)
    a64, b64 = a.double(), bm.double()
    want = a64 @ b64
    # the per-element bound of tests/test_gpu_matmul.py: one storage ulp of the result plus 2^-17 of the element's sum of magnitudes
    tol = 2.0 ** -7 if dtype == torch.bfloat16 else 2.0 ** -10
    bound = tol * want.abs() + 2.0 ** -17 * (a64.abs() @ b64.abs())
    return a, bm, want, bound


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("ta,tb", LAYOUTS)
@pytest.mark.parametrize("shape", SHAPES)
def test_wave128_ksteps_normal_operands(rt, shape, ta, tb, dtype):
    a, bm, want, bound = normal_case(shape, dtype)
    c = run_wave128(rt, a, bm, ta, tb, shape, dtype)
    err = (c.double() - want).abs()
    over = err > bound
    assert not bool(over.any()), f"{int(over.sum().item())} elements over the bound; max err {err.max().item()} at {over.nonzero()[0].tolist()}"
