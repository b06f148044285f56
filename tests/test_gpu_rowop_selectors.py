"""Softmax, LayerNorm, RMSNorm and add_norm / bias_add_norm (csrc/rowops.hip) on a real MI355X against the selector inputs and the
per-element bound of tests/rowop_cases.py (proved on the oracle alone in tests/test_rowop_selectors_cpu.py): every route the mirror
of the dispatch can return, in f32, f16 and bf16, one test per (operator, dtype, route) with the cases of that route inside — its
smallest and largest n and one with a partial last chunk, 1 row and 5, the ALIGNED = false kernels through an odd n and through
views one element off a 16-byte boundary, the row groups R = 2 and R = 4 at 4096 + 3 rows and a second trip of every persistent or
grid-stride loop. After every launch ops.rowop_last_route must name the route the case declares ("chain" for the add-norm chain).

Every launch: the operands and the output (given through out=) are views into blocks with SLACK elements on both sides, the
operand blocks filled with 1000, the output block with 7. Asserted in this order: the whole output is within the bound of its row
(equal to the expectation where the family is exact); no NaN; both output guards still hold 7; every operand block, slack
included, is bit-identical to its copy (the aliased operand of the in-place add-norm forms apart, whose slack must still hold
1000). The in-place forms must also equal the out-of-place launch bit for bit. A failure names the first wrong element, its row
and column, the route and the (p, q) of a selector row.

Found on the MI355X. Before this file no test ran softmax_wave_kernel<T, 8, false, 1>, any ALIGNED = false kernel through an
unaligned pointer, softmax_block_kernel / norm_block_kernel on unaligned long rows, the row groups R = 2 and R = 4 at more than one
n, bias_size == 1, a second trip of a persistent loop at a small n, or the grid-stride loop of the block kernels. All of them meet
the oracle, the eps = 0 rows of LayerNorm exactly in f32. One defect: softmax_block_kernel (aligned rows above 2048 VEC elements and
unaligned ones above 512 VEC) and softmax_strided_kernel returned NaN for a whole row / column as soon as the first element a thread
saw was -inf, in f32, f16 and bf16 alike (9 failing tests: pair, single and mask rows) — the online recurrence computed
exp(-inf + inf). Both kernels now skip the update while the running maximum is -inf; the wave and block kernels that find the
maximum first were never affected.

Worst err / bound on the random inputs (test_rowop_random_inputs_per_element, pytest -s): f32 0.30 softmax, 0.48 LayerNorm, 0.17
RMSNorm; f16 and bf16 0.995 - 0.999 everywhere: one rounding to a 16-bit type IS u_out |want| for a value just above a power of two.

Cost: 366 tests, 10.0 s of the 173 s of the whole GPU suite on the MI355X (163 s without this file: + 6 %), the slowest test 0.35 s.
"""
import numpy as np
import pytest
import torch

import rowop_cases as C
from infinitensor_amd import ops

pytestmark = pytest.mark.gpu
TD = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
CHUNK = 1 << 22  # elements compared at a time (fp64 temporaries of 32 MiB)


@pytest.fixture(scope="module", autouse=True)
def leave_nothing_behind():
    """After the last test of this file: the cached families and references go, and the device blocks torch still holds."""
    yield
    C.release()
    torch.cuda.empty_cache()


def bits(t):
    return t.view(torch.int32 if t.element_size() == 4 else torch.int16)


def in_block(t, fill, off=0):
    """The device tensor t as a view into a block of `fill` with SLACK (+ off) elements in front and SLACK behind -> view, block."""
    if t is None:
        return None, None
    lo = C.SLACK + off
    block = torch.full((t.numel() + lo + C.SLACK,), fill, device="cuda", dtype=t.dtype)
    view = block[lo: lo + t.numel()].view(t.shape)
    view.copy_(t)
    assert (view.data_ptr() & 15 == 0) == (off == 0)
    return view, block


def dev(a, dt):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float32))).cuda().to(TD[dt])


class Kept:
    def __init__(self, *blocks):
        self.blocks = [b for b in blocks if b is not None]
        self.before = [b.clone() for b in self.blocks]

    def unchanged(self):
        return all(torch.equal(bits(b), bits(k)) for b, k in zip(self.blocks, self.before))


def guards_hold(block, numel, off, fill):
    lo = C.SLACK + off
    return bool((block[:lo] == fill).all().item()) and bool((block[lo + numel:] == fill).all().item())


def first_wrong(cs, fam, rows2d, idx_d, want_d, bound_d, what):
    """rows2d [rows, n] against the patterns idx_d of the family; raises with the first wrong element named."""
    n = rows2d.shape[1]
    step = max(1, CHUNK // n)
    for r0 in range(0, rows2d.shape[0], step):
        got = rows2d[r0: r0 + step].double()
        sel = idx_d[r0: r0 + step]
        ok = (got - want_d[sel]).abs() <= bound_d[sel]  # NaN fails; a zero bound admits the exact value only (-0 == +0)
        if bool(ok.all().item()):
            continue
        bad = (~ok).nonzero()[0]
        r, c = int(bad[0]), int(bad[1])
        pat = int(sel[r])
        pq = "" if fam.p is None else f", the row selects p = {int(fam.p[pat])}, q = {int(fam.q[pat])}"
        raise AssertionError(f"{what}: {int((~ok).sum())} wrong elements in rows {r0}.., the first at row {r0 + r}, column {c} (pattern "
                             f"{pat}): got {float(got[r, c])!r}, want {float(want_d[pat, c])!r}, bound {float(bound_d[pat, c]):.3e}; "
                             f"route {cs.route}{pq}")
    assert not bool(torch.isnan(rows2d).any().item()), f"{what}: NaN"


def run_family(rt, cs, fam):
    dt, n = cs.dt, cs.n
    off = 1 if cs.form == "offset" else 0
    want_d = torch.from_numpy(fam.want).cuda()
    bound_d = torch.from_numpy(C.bound_of(fam)).cuda()
    xp = dev(fam.x if cs.op != "add_norm" else fam.a, dt)
    bp = dev(fam.b2, dt) if cs.op == "add_norm" else None
    g, gb = in_block(dev(getattr(fam, "g", None), dt), C.SLACK_FILL)
    b, bb = in_block(dev(getattr(fam, "b", None), dt), C.SLACK_FILL)
    pre, pb = in_block(dev(getattr(fam, "pre", None), dt), C.SLACK_FILL)
    for rnd, idx in enumerate(C.launches(cs, fam)):
        what = f"{cs.name} {fam.kind} {getattr(fam, 'form', '')} round {rnd}"
        idx_d = torch.from_numpy(idx).cuda()
        shape = (cs.outer, n) if cs.inner == 1 else (cs.outer, n, cs.inner)

        def laid(pat):
            rows = pat[idx_d]
            return rows if cs.inner == 1 else rows.view(cs.outer, cs.inner, n).permute(0, 2, 1).contiguous()
        x, xb = in_block(laid(xp), C.SLACK_FILL, off)
        x2, x2b = in_block(laid(bp), C.SLACK_FILL, off) if bp is not None else (None, None)
        kept = Kept(xb, x2b, gb, bb, pb)
        out, ob = in_block(torch.full(shape, C.OUT_FILL, device="cuda", dtype=TD[dt]), C.OUT_FILL, off)

        def launch(a_, b_, out_):
            if cs.op == "softmax":
                got = ops.softmax(rt, a_, 1, out=out_)
            elif cs.op == "add_norm":
                got = ops.add_layer_norm(rt, a_, b_, g, b, cs.eps, cs.rms, out=out_, pre=pre)
            else:
                got = ops.rms_norm(rt, a_, g, cs.eps, out=out_) if cs.rms else ops.layer_norm(rt, a_, g, b, cs.eps, -1, out=out_)
            assert ops.rowop_last_route(rt) == cs.route, f"{what}: launched {ops.rowop_last_route(rt)}, the case is built for {cs.route}"
            return got

        def rows_of(t):
            return t if cs.inner == 1 else t.permute(0, 2, 1).reshape(cs.outer * cs.inner, n)
        launch(x, x2, out)
        first_wrong(cs, fam, rows_of(out), idx_d, want_d, bound_d, what)
        assert guards_hold(ob, out.numel(), off, C.OUT_FILL), f"{what}: written outside the output ({cs.route})"
        assert kept.unchanged(), f"{what}: an operand changed ({cs.route})"
        if cs.op == "add_norm" and cs.outer <= 5000:  # in place over b and over a
            for alias in ("b", "a"):
                tgt, tb = in_block((x2 if alias == "b" else x).clone(), C.SLACK_FILL, off)
                kept = Kept(x2b if alias == "a" else xb, gb, bb, pb)
                got = launch(tgt if alias == "a" else x, tgt if alias == "b" else x2, tgt)
                assert got.data_ptr() == tgt.data_ptr()
                assert torch.equal(bits(tgt), bits(out)), f"{what}: in place over {alias} differs from the out-of-place result ({cs.route})"
                first_wrong(cs, fam, tgt, idx_d, want_d, bound_d, f"{what} in place over {alias}")
                assert guards_hold(tb, tgt.numel(), off, C.SLACK_FILL), f"{what}: in place over {alias} wrote outside its rows"
                assert kept.unchanged(), f"{what}: in place over {alias} changed another operand"


def groups():
    out = {}
    for cs in C.CASES.values():
        out.setdefault((cs.op, cs.rms, cs.add, cs.dt, cs.route), []).append(cs.name)
    return out


GROUPS = groups()


@pytest.mark.parametrize("key", list(GROUPS), ids=lambda k: f"{k[0]}{'-rms' if k[1] else ''}{'-add%d' % k[2] if k[2] else ''}-{k[3]}-{k[4]}")
def test_rowop_selectors(rt, key):
    assert rt.device_info()["compute_units"] <= C.NUM_CU  # the row counts of the second trips are sized for that many
    for name in GROUPS[key]:
        cs = C.CASES[name]
        for fam in C.families(cs):
            run_family(rt, cs, fam)


@pytest.mark.parametrize("params", C.random_params(), ids=lambda p: f"{p[0]}-{p[1]}-{'x'.join(map(str, p[2]))}-ax{p[3]}-{'bias' if p[4] else 'nobias'}")
def test_rowop_random_inputs_per_element(rt, params):
    """The random inputs of test_softmax_vs_oracle, test_layernorm_vs_oracle and test_rmsnorm_vs_oracle held to the per-element bound."""
    op, dt, shape, axis, with_bias, route = params
    ref = C.random_reference(*params)
    x, xb = in_block(dev(ref.x, dt), C.SLACK_FILL)
    g, gb = in_block(dev(ref.g, dt), C.SLACK_FILL)
    b, bb = in_block(dev(ref.b, dt), C.SLACK_FILL)
    kept = Kept(xb, gb, bb)
    out, ob = in_block(torch.full(shape, C.OUT_FILL, device="cuda", dtype=TD[dt]), C.OUT_FILL)
    if op == "softmax":
        ops.softmax(rt, x, axis, out=out)
    elif op == "rms_norm":
        ops.rms_norm(rt, x, g, C.EPS, out=out)
    else:
        ops.layer_norm(rt, x, g, b, C.EPS, axis, out=out)
    got = out.double().cpu().numpy()
    worst, idx = C.worst_ratio(got, ref.want, ref.bound)
    print(f"random {op} {dt} {shape} {route}: worst err/bound {worst:.3f} at {idx}")
    assert worst <= 1.0, f"{params}: worst err/bound {worst:.3g} at {idx}: got {got[idx]!r}, want {ref.want[idx]!r}, bound {ref.bound[idx]:.3e}"
    assert not np.isnan(got).any()
    assert guards_hold(ob, out.numel(), 0, C.OUT_FILL) and kept.unchanged(), params
