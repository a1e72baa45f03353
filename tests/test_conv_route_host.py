"""Which convolution kernel runs (csrc/spade.hip conv_route through the host-only hook sln_debug_conv_route) against the routes the
case table of tests/conv_cases.py claims, for no switch, SLN_CONV_STAGED and SLN_CONV_DMA; the table reaches every instantiated
kernel; the hook refuses what the entry points refuse.  CPU only: the hook makes no HIP call."""
import ctypes as C

import pytest

import conv_cases as K
from conftest import pkg


def ask(case_or_args, force, terms=None):
    L = pkg("_lib")
    if isinstance(case_or_args, K.Case):
        c = case_or_args
        args = (c.terms, 1 if c.entry == K.MOD else 0, c.B, c.Cin, c.H, c.W, c.rows, c.rows_pad, c.ksize)
    else:
        args = case_or_args
    out = L.SlnDbgConvRoute()
    rc = L.lib().sln_debug_conv_route(*args, force, C.byref(out))
    return rc, (K.KERNEL_IDS.get(out.kernel), out.bmc, out.tile_h, out.gk, out.blk, out.terms, out.shares)


def test_struct_size_matches_the_library():
    L = pkg("_lib")
    sizes = (C.c_int * 4)()
    n = L.lib().sln_debug_conv_sizes(sizes, 4)
    assert n == 1 and sizes[0] == C.sizeof(L.SlnDbgConvRoute) == 28


@pytest.mark.parametrize("force", [0, 1, 2])
@pytest.mark.parametrize("case", K.CASES, ids=lambda c: c.name)
def test_every_case_takes_the_route_the_table_claims(case, force):
    rc, route = ask(case, force)
    assert rc == 0
    assert route == K.route_for(case, force), (case.name, force)
    if force == 1 and case.terms == 0:
        assert route[0] == K.STAGED and route[4] == (2 if case.entry == K.CONV and case.ksize == 3 and case.Cin >= 512 else 0)


# Every instantiation of csrc/spade.hip, checked by eye against launch_conv_f32 / launch_conv_f16 there:
# (kernel, bmc, ksize, epi, tile_h, gk, blk, terms, split).  39 kernels; 14 of them in both the split and the unsplit form.
BOTH = (False, True)
KERNELS = set(
    # conv_mfma_kernel<BMC, KS, EPI, BLK>: 8
    [(K.STAGED, bmc, ks, 0, 8, 8, 0, 0, False) for bmc in (64, 128) for ks in (1, 3)] +
    [(K.STAGED, bmc, 3, 0, 8, 8, 2, 0, False) for bmc in (64, 128)] +
    [(K.STAGED, bmc, 3, 1, 8, 8, 0, 0, False) for bmc in (64, 128)] +
    # conv_glds_kernel<BMC, KS, EPI, THT, GK, BLK>: 13
    [(K.DMA, bmc, ks, 0, 8, 4, 0, 0, s) for bmc in (64, 128) for ks in (1, 3) for s in BOTH] +
    [(K.DMA, bmc, 3, 0, 8, 4, 4, 0, s) for bmc in (64, 128) for s in BOTH] +
    [(K.DMA, 64, 3, 0, 16, 8, 2, 0, False)] +
    [(K.DMA, 64, 3, epi, 16, 8, 0, 0, False) for epi in (0, 1)] + [(K.DMA, 128, 3, epi, 16, 4, 0, 0, False) for epi in (0, 1)] +
    [(K.DMA, bmc, 3, 1, 8, 4, 0, 0, False) for bmc in (64, 128)] +
    # conv_f16_kernel<BMC, EPI, THT, TERMS, BLK>: 18
    [(K.F16, bmc, 3, 0, 8, 16, blk, t, s) for bmc in (64, 128) for blk in (0, 1) for t in (1, 3) for s in BOTH] +
    [(K.F16, bmc, 3, 1, 8, 16, 0, t, False) for bmc in (64, 128) for t in (1, 3)] +
    [(K.F16, bmc, 3, epi, 16, 16, 0, t, False) for epi in (0, 1) for (bmc, t) in ((64, 1), (64, 3), (128, 1))])


def test_the_table_reaches_every_instantiated_kernel_and_nothing_else():
    assert len(KERNELS) == 39 + 14 and len({k[:8] for k in KERNELS}) == 39
    reached = set()
    for case in K.CASES:
        for force in (0, 1, 2):
            rc, route = ask(case, force)
            assert rc == 0
            reached.add(K.kernel_of(case, route))
    assert reached == KERNELS, (sorted(KERNELS - reached), sorted(reached - KERNELS))
    # ... and with no switch set every kernel but the four unsplit 8 x 16 bias/activation DMA forms
    default = {K.kernel_of(c, c.route) for c in K.CASES}
    assert KERNELS - default == {(K.DMA, bmc, ks, 0, 8, 4, 0, 0, False) for bmc in (64, 128) for ks in (1, 3)}


def test_the_tall_three_product_128_row_form_reports_the_8x16_kernel():
    for name in ("f16-tall-128-t3", "f16-tall-mod-128-t3"):
        assert ask(K.BY_NAME[name], 0)[1][2] == 8 and ask(K.BY_NAME[name.replace("t3", "t1")], 0)[1][2] == 16


def test_the_hook_refuses_what_the_entry_points_refuse():
    BADARG, UNSUPPORTED = -1, -2
    ok = (0, 0, 2, 16, 9, 18, 33, 64, 3)               # terms, epi, B, Cin, H, W, rows, rows_pad, ksize
    assert ask(ok, 0)[0] == 0

    def with_(**kw):
        names = ("terms", "epi", "B", "Cin", "H", "W", "rows", "rows_pad", "ksize")
        return tuple(kw.get(n, v) for n, v in zip(names, ok))
    assert ask(with_(rows_pad=96), 0)[0] == BADARG                                 # rows_pad % 64
    assert ask(with_(rows_pad=96, epi=1), 0)[0] == BADARG
    assert ask(with_(rows=65), 0)[0] == BADARG                                      # rows > rows_pad
    assert ask(with_(rows=33, epi=1), 0)[0] == BADARG                               # rows_pad < 64 ceil(C / 32)
    assert ask(with_(H=1), 0)[0] == BADARG and ask(with_(W=1), 0)[0] == BADARG     # H < 2 at 3x3
    assert ask(with_(H=1, ksize=1), 0)[0] == 0
    assert ask(with_(ksize=1, terms=1), 0)[0] == UNSUPPORTED                        # a 1x1 half convolution
    assert ask(with_(ksize=1, terms=3), 0)[0] == UNSUPPORTED
    assert ask(with_(ksize=5), 0)[0] == UNSUPPORTED and ask(with_(ksize=1, epi=1), 0)[0] == UNSUPPORTED
    big = dict(Cin=1 << 15, H=256, W=256)                                           # Cin H W = 2^31
    assert ask(with_(terms=1, **big), 0)[0] == UNSUPPORTED and ask(with_(terms=3, epi=1, rows=32, **big), 0)[0] == UNSUPPORTED
    assert ask(with_(**big), 0)[0] == 0                                             # (the fp32 kernels index with 64 bits)
    assert ask(with_(terms=1, Cin=(1 << 15) - 1, H=256, W=256), 0)[0] == 0
    assert ask(with_(B=0), 0)[0] == BADARG and ask(with_(Cin=0), 0)[0] == BADARG
    assert ask(with_(terms=2), 0)[0] == BADARG and ask(with_(epi=2), 0)[0] == BADARG
    assert ask(ok, 3)[0] == BADARG and ask(ok, -2)[0] == BADARG
    assert pkg("_lib").lib().sln_debug_conv_route(*ok, 0, None) == BADARG


def test_the_process_switches_are_what_force_minus_one_reports():
    import os
    if any(os.environ.get(v) is not None for v in ("SLN_CONV_STAGED", "SLN_CONV_DMA", "SLN_CONV_KSPLIT")):
        force = 1 if os.environ.get("SLN_CONV_STAGED") is not None else 2
        if os.environ.get("SLN_CONV_KSPLIT") is not None:
            return                                     # another split bound: no claim in the table
    else:
        force = 0
    for case in K.CASES:
        assert ask(case, -1) == ask(case, force), case.name
