"""The split word of the wgrad launches (include/sln_hip.h: sln_set_tn_split) and the arithmetic of the split itself, host side only.

The plumbing: setter / getter, what the loader makes of SLN_TN_SPLIT, header / ctypes table / library agreement.
The arithmetic, restated in numpy as csrc/gemm_bodies.h::gemm_tn_split_body does it: a value v becomes p1 = bf16(v), p2 = bf16(v - p1),
p3 = bf16(v - p1 - p2) (round to nearest even), and a product g x is summed as g1 x3 + g3 x1 + g2 x2 + g1 x2 + g2 x1 + g1 x1.
  * three parts carry 3 x 8 significand bits: p1 + p2 + p3 reproduces v to 2^-24 of |v| over the whole exponent range - no scale;
  * the six products against the fp64 product at R = 705, next to a float32 matmul's error on the same operands: this is the budget
    the GPU tests (tests/test_tn_split_gpu.py) quote when they hold the split body to the bounds of the fp32 one."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import test_abi
from conftest import ROOT, pkg

OFF, ON = 0, 1               # csrc/sln_common.h: SLN_TN_SPLIT_OFF, SLN_TN_SPLIT_ON (the shipped default)


@pytest.fixture
def lib():
    h = pkg("_lib").lib()
    before = h.sln_get_tn_split()
    yield h
    assert h.sln_set_tn_split(before) == 0


def test_setter_and_getter_round_trip(lib):
    for v in (OFF, ON, OFF, ON):
        assert lib.sln_set_tn_split(v) == 0
        assert lib.sln_get_tn_split() == v


@pytest.mark.parametrize("bad", [2, 3, 4, 1 << 30, -1])
def test_another_value_is_refused_and_changes_nothing(lib, bad):
    for keep in (OFF, ON):
        assert lib.sln_set_tn_split(keep) == 0
        assert lib.sln_set_tn_split(bad) == -1, "SLN_E_BADARG"
        assert lib.sln_get_tn_split() == keep


def test_environment_parsing(lib):
    parse = lib.sln_parse_tn_split_env
    for dflt in (ON, OFF):
        assert parse(None, dflt) == dflt and parse(b"", dflt) == dflt, "unset / empty: the default"
        assert parse(b"0", dflt) == OFF and parse(b"1", dflt) == ON
        for junk in (b"2", b"3", b"-1", b"on", b"1x", b"0x", b" 1", b"1 ", b"01", b"10", b"99999999999999999999"):
            assert parse(junk, dflt) == dflt, "%r must read as the default" % junk


@pytest.mark.parametrize("value,want", [(None, ON), ("0", OFF), ("1", ON), ("7", ON)])
def test_the_word_a_fresh_process_starts_with(value, want):
    env = {k: v for k, v in os.environ.items() if k != "SLN_TN_SPLIT"}
    if value is not None:
        env["SLN_TN_SPLIT"] = value
    code = "import importlib; print(importlib.import_module('3d_sln_amd._lib').lib().sln_get_tn_split())"
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, check=True).stdout
    assert int(out.strip().splitlines()[-1]) == want, out


def test_header_declares_the_switch_and_the_abi_agreement_holds():
    text = open(test_abi.HEADER).read()
    for name in ("sln_set_tn_split", "sln_get_tn_split", "sln_parse_tn_split_env"):
        assert re.search(r"\b%s\s*\(" % name, text), name + " missing from include/sln_hip.h"
        assert name in pkg("_lib").SIGNATURES, name + " missing from the ctypes table"
    test_abi.test_header_ctypes_table_and_library_agree()


# ---------------------------------------------------------------------------------------------- the split, in numpy
def bf16(v):
    """float32 -> the nearest bf16 (ties to even), returned as float32.  Finite inputs below bf16's largest value."""
    u = np.asarray(v, np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32)


def split3(v):
    v = np.asarray(v, np.float32)
    p1 = bf16(v)
    r1 = v - p1                     # exact in float32
    p2 = bf16(r1)
    r2 = r1 - p2                    # exact in float32
    return p1, p2, bf16(r2)


def test_three_parts_reproduce_a_value_over_the_exponent_range():
    g = np.random.default_rng(0)
    mant = g.uniform(1.0, 2.0, 200000) * g.choice([-1.0, 1.0], 200000)
    expo = g.uniform(np.log2(1e-30), np.log2(1e30), 200000)
    v = (mant * np.exp2(np.floor(expo))).astype(np.float32)
    p1, p2, p3 = split3(v)
    # the differences the split relies on are exact: each part is the float32 subtraction's own result, rounded
    assert np.array_equal((v.astype(np.float64) - p1).astype(np.float32).astype(np.float64), v.astype(np.float64) - p1)
    err = np.abs(v.astype(np.float64) - (p1.astype(np.float64) + p2 + p3)) / np.abs(v)
    print("largest |v - (p1 + p2 + p3)| / |v| = %.3e (2^-24 = %.3e)" % (err.max(), 2.0 ** -24))
    assert err.max() <= 2.0 ** -24
    # ... and a scaling by a power of two commutes with the split, bit for bit (what the GPU tests' range cases rest on)
    for s in (2.0 ** -40, 2.0 ** 40):
        w = v[(np.abs(v) > 1e-20) & (np.abs(v) < 1e20)]
        for a, b in zip(split3(w), split3((w * np.float32(s)).astype(np.float32))):
            assert np.array_equal(a * np.float32(s), b)


def test_six_products_against_fp64_next_to_a_float32_matmul():
    R, N = 705, 64
    g = np.random.default_rng(1)
    G = g.standard_normal((R, N)).astype(np.float32)
    X = g.standard_normal((R, N)).astype(np.float32)
    ref = G.astype(np.float64).T @ X.astype(np.float64)
    g1, g2, g3 = (p.astype(np.float64) for p in split3(G))
    x1, x2, x3 = (p.astype(np.float64) for p in split3(X))
    six = g1.T @ x3 + g3.T @ x1 + g2.T @ x2 + g1.T @ x2 + g2.T @ x1 + g1.T @ x1
    f32 = (G.T @ X).astype(np.float64)
    mag = np.abs(G.astype(np.float64)).T @ np.abs(X.astype(np.float64))            # sum |g| |x| per element
    e_six, e_f32 = np.abs(six - ref), np.abs(f32 - ref)
    print("six products, fp64 sums : max err %.3e = %.3e of sum|g||x|" % (e_six.max(), (e_six / mag).max()))
    print("float32 matmul          : max err %.3e = %.3e of sum|g||x|" % (e_f32.max(), (e_f32 / mag).max()))
    # the three dropped products are below 3 x 2^-24 of |g||x| each (|p2| <= 2^-8 |v|, |p3| <= 2^-16 |v|: 2^-24 + 2^-24 + 2^-32),
    # and what p1 + p2 + p3 leaves of each operand another 2 x 2^-24
    # (the fp32 accumulators of the device add their own rounding on top, as the fp32 route's do; the float32 matmul's figure above
    #  is printed for comparison only - its sum order is the BLAS library's)
    assert (e_six / mag).max() <= 5.0 * 2.0 ** -24
