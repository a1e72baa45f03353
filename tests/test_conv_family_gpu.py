"""Every SPADE convolution kernel of csrc/spade.hip, named by the route it is reached through, against answers that are right in
every summation order (run with -m gpu).  The cases (tests/conv_cases.py) go through the public entry points -
sln_spade_conv_sums / sln_spade_conv / sln_spade_modulate_up and their _f16 forms - with weights packed by _pack, _pack_gamma_beta
and split_f16; before each launch sln_debug_conv_route says which kernel the library will run and the test holds it to the table.

  integer   x, w in {-2 .. 2}, bias in {-8 .. 8}, power-of-two slope: all 39 kernels return the fp64 answer bit for bit, and so do
            the fp64 LayerNorm / pixel sums.  The detector for indexing: tiles, halos, reflections, tails, shares, row blocks.
  lattice   h + l with h in {-1, 0, 1}, l = +-2^-12: the hi x lo and lo x hi products of the three-product mode, bit for bit.
            Rests on the 16-bit MFMA adding exactly representable sums exactly.
  Gaussian  ordinary data against |y - ref| <= gamma_n (conv(|x|, |w|) + |b|), n = 9 Cin + shares + 2, u = 2^-24: a bound derived
            from the arithmetic; no kernel's own error stands in it.
  padding   NaN in the packed rows nobody owns must change no byte.
  switches  the whole file again in a child process under SLN_CONV_STAGED and under SLN_CONV_DMA.
Outputs stand between 4 096 sentinel floats on each side and over a second sentinel no answer can equal."""
import ctypes as C
import os
import subprocess
import sys

import pytest
import torch

import conv_cases as K
import conv_ref as R
from conftest import pkg

pytestmark = pytest.mark.gpu

GUARD = 4096
SENT_GUARD, SENT_FILL = -(2.0 ** 100), -(2.0 ** 99)          # no answer of any group comes near either


def _force():
    """What the process's switches stand for in the table (the hook's force value)."""
    return 1 if os.environ.get("SLN_CONV_STAGED") is not None else 2 if os.environ.get("SLN_CONV_DMA") is not None else 0


def _route(case):
    L = pkg("_lib")
    out = L.SlnDbgConvRoute()
    L.check(L.lib().sln_debug_conv_route(case.terms, 1 if case.entry == K.MOD else 0, case.B, case.Cin, case.H, case.W, case.rows,
                                         case.rows_pad, case.ksize, -1, C.byref(out)), "sln_debug_conv_route")
    return (K.KERNEL_IDS.get(out.kernel), out.bmc, out.tile_h, out.gk, out.blk, out.terms, out.shares)


class Guarded:
    """n elements between two guards; the elements start as `fill` (SENT_FILL: must all be overwritten; 0: an accumulator)."""
    def __init__(self, n, dtype, fill):
        self.n, self.fill = n, fill
        self.buf = torch.full((n + 2 * GUARD,), SENT_GUARD, dtype=dtype, device="cuda")
        self.data = self.buf[GUARD:GUARD + n]
        self.data.fill_(fill)

    def check(self, what):
        assert bool((self.buf[:GUARD] == SENT_GUARD).all()) and bool((self.buf[GUARD + self.n:] == SENT_GUARD).all()), what + ": wrote outside its buffer"
        if self.fill != 0:
            left = int((self.data == self.fill).sum())
            assert left == 0, "%s: %d of %d elements never written" % (what, left, self.n)


class Packed:
    """The device operands of a case: x, the packed weights (fp32, or fp16 hi / lo) and bias, xin and stats of a modulation."""
    def __init__(self, case, d, nan_padding=False):
        S = pkg("host.SPADE_related")
        self.case = case
        f = lambda t: t.float().cuda().contiguous()
        self.x = f(d["x"])
        if case.entry == K.CONV:
            self.wp, rp = S._pack(f(d["w"]), rows_pad=case.rows_pad)
            self.bias = torch.zeros(rp, device="cuda"); self.bias[:case.rows] = f(d["b"])
            self.pad_rows = torch.arange(case.rows, rp, device="cuda")
        else:
            self.wp, self.bias, rp = S._pack_gamma_beta(f(d["wg"]), f(d["bg"]), f(d["wb"]), f(d["bb"]))
            self.xin, self.stats = f(d["xin"]), f(d["stats"])
            r = torch.arange(rp, device="cuda")
            self.pad_rows = r[(r // 64) * 32 + r % 32 >= case.rows]          # gamma and beta rows of the channels >= C
        assert rp == case.rows_pad
        self.hi = self.lo = None
        if case.terms:
            self.hi, self.lo = S.split_f16(self.wp)
        if nan_padding:
            assert self.pad_rows.numel() > 0
            self.bias[self.pad_rows] = float("nan")
            if case.terms:
                self.hi[:, :, self.pad_rows] = float("nan")
                self.lo[:, :, self.pad_rows] = float("nan")
            else:
                self.wp[:, :, self.pad_rows] = float("nan")

    def weights64(self, part):
        """The pack's own hi (part 0) or lo (part 1) as fp64 conv weights: [Cout, Cin, 3, 3], or (gamma, beta) of a modulation."""
        S = pkg("host.SPADE_related")
        c = self.case
        w = S.unpack_f16(self.lo if part else self.hi, None, c.Cin).cpu()                    # [9, Cin, rows_pad]
        take = lambda rows: w[:, :, rows].permute(2, 1, 0).reshape(len(rows), c.Cin, 3, 3).contiguous()
        idx = torch.arange(c.rows)
        if c.entry == K.CONV:
            return take(idx)
        return take((idx // 32) * 64 + idx % 32), take((idx // 32) * 64 + 32 + idx % 32)


def launch(p, act, slope, with_sums=False):
    """One call of the case's entry point -> (y [B, rows, H, W] on the device, ln [B, 16] or None, gap [B, rows] or None)."""
    L = pkg("_lib"); lib = L.lib()
    c = p.case
    assert _route(c) == K.route_for(c, _force()), (c.name, "force", _force(), _route(c))
    y = Guarded(c.B * c.rows * c.H * c.W, torch.float32, SENT_FILL)
    st = L.current_stream_ptr()
    wargs = (L.ptr(p.hi), L.ptr(p.lo) if c.terms == 3 else None) if c.terms else (L.ptr(p.wp),)
    ln = gap = None
    if c.entry == K.CONV:
        shape = (L.ptr(p.x), c.B, c.Cin, c.H, c.W) + wargs + (L.ptr(p.bias), c.rows, c.rows_pad, c.ksize, act, slope, L.ptr(y.data))
        if with_sums:
            ln, gap = Guarded(16 * c.B, torch.float64, 0), Guarded(c.B * c.rows, torch.float64, 0)
            fn = lib.sln_spade_conv_sums_f16 if c.terms else lib.sln_spade_conv_sums
            L.check(fn(*shape, L.ptr(ln.data), L.ptr(gap.data), st), "conv_sums " + c.name)
        else:
            fn = lib.sln_spade_conv_f16 if c.terms else lib.sln_spade_conv
            L.check(fn(*shape, st), "conv " + c.name)
    else:
        fn = lib.sln_spade_modulate_up_f16 if c.terms else lib.sln_spade_modulate_up
        L.check(fn(L.ptr(p.x), c.B, c.Cin, c.H, c.W, *wargs, L.ptr(p.bias), c.rows, c.rows_pad, L.ptr(p.xin), c.xin_up, L.ptr(p.stats),
                   act, slope, L.ptr(y.data), st), "modulate " + c.name)
    torch.cuda.synchronize()
    y.check(c.name + " output")
    for g, what in ((ln, "ln_acc"), (gap, "gap_acc")):
        if g is not None:
            g.check(c.name + " " + what)
    return (y.data.view(c.B, c.rows, c.H, c.W), None if ln is None else ln.data.view(c.B, 16), None if gap is None else gap.data.view(c.B, c.rows))


def _same_bytes(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _fits_fp32(t):
    return torch.equal(t.float().double(), t)


def _reference(case, d, conv_fn, abs_fn, acts, slope, limit):
    """-> {act: fp64 answer}.  conv_fn / abs_fn(w, b) -> the convolution and the sum of the magnitudes of its terms.  Asserts, from
    the reference alone, what the exact groups need: sum |terms| < limit and every epilogue value an fp32 number."""
    if case.entry == K.CONV:
        pre = conv_fn(d["w"], d["b"])
        assert float(abs_fn(d["w"], d["b"]).max()) < limit
        out = {act: R.activate(pre, act, slope) for act in acts}
    else:
        gamma, beta = conv_fn(d["wg"], d["bg"]), conv_fn(d["wb"], d["bb"])
        assert max(float(abs_fn(d["wg"], d["bg"]).max()), float(abs_fn(d["wb"], d["bb"]).max())) < limit
        plain = R.modulate(gamma, torch.zeros_like(beta), d["xin"], case.xin_up, d["stats"], R.ACT_NONE, slope)
        assert _fits_fp32(gamma) and _fits_fp32(1.0 + gamma) and _fits_fp32(plain)
        out = {act: R.modulate(gamma, beta, d["xin"], case.xin_up, d["stats"], act, slope) for act in acts}
    assert all(_fits_fp32(v) for v in out.values())
    return out


# ------------------------------------------------------------------------------------------------ integer operands
@pytest.mark.parametrize("case", K.CASES, ids=lambda c: c.name)
def test_integer_operands_bit_for_bit(case):
    d = K.integer_operands(case)
    p = Packed(case, d)
    if case.terms:
        assert not bool(p.lo.any())                                  # integers are fp16 numbers: hi carries all, both modes agree
    acts = (R.ACT_NONE, R.ACT_RELU, R.ACT_LEAKY) if case.entry == K.CONV else (R.ACT_NONE, R.ACT_LEAKY)
    refs = _reference(case, d, lambda w, b: R.conv(d["x"], w, b), lambda w, b: R.conv_abs(d["x"], w, b), acts, K.SLOPE, 2.0 ** 24)
    for act in acts:
        ref = refs[act]
        y, ln, gap = launch(p, act, K.SLOPE, with_sums=case.entry == K.CONV)
        bad = int((y.double().cpu() != ref).sum())
        assert bad == 0, "%s act %d: %d of %d outputs differ from the fp64 answer, max %g" % (
            case.name, act, bad, ref.numel(), float((y.double().cpu() - ref).abs().max()))
        if case.entry == K.CONV:
            ln_ref, gap_ref = R.sums(ref)
            # multiples of 1/4 (values) and 1/16 (squares): sums below 2^53 of those units are exact in fp64 in any order
            assert float(ref.abs().sum((1, 2, 3)).max()) * 4 < 2.0 ** 53 and float(ln_ref[:, 1].max()) * 16 < 2.0 ** 53
            assert torch.equal(ln.cpu()[:, :2], ln_ref), (case.name, act, "LayerNorm sums")
            assert not bool(ln[:, 2:].any())
            assert torch.equal(gap.cpu(), gap_ref), (case.name, act, "pixel sums")
            y2, _, _ = launch(p, act, K.SLOPE, with_sums=False)
            assert _same_bytes(y, y2), (case.name, act, "conv and conv_sums differ")


# ------------------------------------------------------------------------------------------------ the lo path
@pytest.mark.parametrize("lo_in_x", [True, False], ids=["lo-in-x", "lo-in-w"])
@pytest.mark.parametrize("case", K.HALF_CASES, ids=lambda c: c.name)
def test_lattice_operands_tell_the_products_apart(case, lo_in_x):
    d = K.lattice_operands(case, lo_in_x)
    p = Packed(case, d)
    x = d["x"]
    hi = p.weights64(0)
    lo = p.weights64(1)
    by_w = {}                                                        # reference weights are looked up by the operand they stand for
    if case.entry == K.CONV:
        by_w[id(d["w"])] = (hi, lo)
        assert torch.equal(hi + lo, d["w"])
    else:
        by_w[id(d["wg"])], by_w[id(d["wb"])] = (hi[0], lo[0]), (hi[1], lo[1])
        assert torch.equal(hi[0] + lo[0], d["wg"]) and torch.equal(hi[1] + lo[1], d["wb"])
    xh, xl = R.f16_split(x)
    assert torch.equal(xh + xl, x) and bool(xl.any()) == lo_in_x and bool(lo[0].any() if case.entry == K.MOD else lo.any()) != lo_in_x
    three = lambda w, b: R.conv_three_products(x, *by_w[id(w)], b)
    three_abs = lambda w, b: R.conv_three_products_abs(x, *by_w[id(w)], b)
    one = lambda w, b: R.conv_one_product(x, by_w[id(w)][0], b)
    act = R.ACT_LEAKY
    ref3 = _reference(case, d, three, three_abs, (act,), K.SLOPE, 2.0 ** 6)[act]
    ref1 = _reference(case, d, one, three_abs, (act,), K.SLOPE, 2.0 ** 6)[act]
    differ = float((ref3 != ref1).double().mean())
    assert differ >= 0.25, "the data does not tell the modes apart: %.3f of the outputs differ" % differ
    ref = ref3 if case.terms == 3 else ref1
    y, _, _ = launch(p, act, K.SLOPE)
    err = (y.double().cpu() - ref).abs()
    bad = int((err != 0).sum())
    other = float((y.double().cpu() != (ref1 if case.terms == 3 else ref3)).double().mean())
    print("%s %s: %d of %d outputs off, max %g (in units of 2^-12: %g); %.3f differ from the other mode's answer" % (
        case.name, "lo in x" if lo_in_x else "lo in w", bad, ref.numel(), float(err.max()), float(err.max()) * 4096, other))
    assert bad == 0, (case.name, bad, float(err.max()))


# ------------------------------------------------------------------------------------------------ Gaussian operands
@pytest.mark.parametrize("name", K.GAUSSIAN)
def test_gaussian_operands_inside_the_derived_bound(name):
    case = K.BY_NAME[name]
    d = K.gaussian_operands(case)
    p = Packed(case, d)
    x, b = d["x"], d["b"]
    if case.terms == 0:
        ref, mag = R.conv(x, d["w"], b), R.conv_abs(x, d["w"], b)
    elif case.terms == 1:
        w_hi = p.weights64(0)
        ref, mag = R.conv_one_product(x, w_hi, b), R.conv_abs(R.f16_round(x), w_hi, b)
    else:
        w_hi, w_lo = p.weights64(0), p.weights64(1)
        ref, mag = R.conv_three_products(x, w_hi, w_lo, b), R.conv_three_products_abs(x, w_hi, w_lo, b)
    shares = K.route_for(case, _force())[6]
    bound = R.gamma_bound(9 * case.Cin + shares + 2) * mag
    y, _, _ = launch(p, R.ACT_NONE, 0.0)
    err = (y.double().cpu() - ref).abs()
    worst = float((err / bound).max())
    print("%s: max error %.3g, at most %.3f of the bound (gamma_n = %.3g)" % (name, float(err.max()), worst, R.gamma_bound(9 * case.Cin + shares + 2)))
    assert bool((err <= bound).all()), (name, "max error / bound", worst)
    if case.terms == 1:                                              # the one-product mode really rounds its operands
        assert float((y.double().cpu() - R.conv(x, d["w"], b)).abs().max()) > float(bound.max())


# ------------------------------------------------------------------------------------------------ padding
@pytest.mark.parametrize("name", K.PADDING)
def test_nan_in_the_padding_rows_changes_no_byte(name):
    case = K.BY_NAME[name]
    d = K.integer_operands(case)
    sums = case.entry == K.CONV
    clean = launch(Packed(case, d), R.ACT_LEAKY, K.SLOPE, with_sums=sums)
    dirty = launch(Packed(case, d, nan_padding=True), R.ACT_LEAKY, K.SLOPE, with_sums=sums)
    assert not bool(torch.isnan(dirty[0]).any())
    assert _same_bytes(clean[0], dirty[0])
    if sums:
        assert torch.equal(clean[1].view(torch.int64), dirty[1].view(torch.int64)) and torch.equal(clean[2].view(torch.int64), dirty[2].view(torch.int64))


# ------------------------------------------------------------------------------------------------ the forced switches
@pytest.mark.parametrize("env", ["SLN_CONV_STAGED", "SLN_CONV_DMA"])
def test_forced_switch_child_run(env):
    """The switches are read once per process: this file again in a fresh child with one of them set (the child's route assertions ask
    the hook with force = -1, so they follow the switch), without the tests that start children."""
    e = dict(os.environ)
    e.pop("SLN_CONV_STAGED", None); e.pop("SLN_CONV_DMA", None)
    e[env] = "1"
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", os.path.abspath(__file__), "-k", "not forced_switch_child_run"],
                       env=e, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
