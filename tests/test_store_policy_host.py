"""The store policy switch of the NT GEMM epilogues (include/sln_hip.h: sln_set_store_policy), host side only: no GPU is touched.

The policy word never changes a value, so what can go wrong here is the plumbing: the setter and the getter, what the loader makes of
SLN_STORE_POLICY, and the header / ctypes table / library agreement of tests/test_abi.py with the three new entry points in it."""
import re

import pytest

import test_abi
from conftest import pkg

PLAIN, NT_WT = 0, 1          # csrc/sln_common.h: SLN_STORE_PLAIN, SLN_STORE_NT_WT (the shipped default)


@pytest.fixture
def lib():
    h = pkg("_lib").lib()
    before = h.sln_get_store_policy()
    yield h
    assert h.sln_set_store_policy(before) == 0


def test_setter_and_getter_round_trip(lib):
    for v in (PLAIN, NT_WT, PLAIN, NT_WT):
        assert lib.sln_set_store_policy(v) == 0
        assert lib.sln_get_store_policy() == v


@pytest.mark.parametrize("bad", [2, 3, 4, 8, 1 << 30, -1])
def test_an_unknown_bit_is_refused_and_changes_nothing(lib, bad):
    for keep in (PLAIN, NT_WT):
        assert lib.sln_set_store_policy(keep) == 0
        assert lib.sln_set_store_policy(bad) == -1, "SLN_E_BADARG"
        assert lib.sln_get_store_policy() == keep


def test_environment_default_parsing(lib):
    parse = lib.sln_parse_store_policy_env
    # both defaults: with the shipped one alone a "1x" taken for 1 could not be told from a "1x" that was refused
    for dflt in (NT_WT, PLAIN):
        assert parse(None, dflt) == dflt and parse(b"", dflt) == dflt, "unset / empty: the default"
        assert parse(b"0", dflt) == PLAIN, "one value restores plain stores everywhere"
        assert parse(b"1", dflt) == NT_WT
        for junk in (b"2", b"3", b"7", b"-1", b"on", b"1x", b"0x", b" 1 ", b"1 ", b"0x1", b"99999999999999999999"):
            assert parse(junk, dflt) == dflt, "%r must fall back to the default" % junk


def test_the_loader_ships_write_through(lib):
    """The word a fresh process starts with (no SLN_STORE_POLICY in its environment): asked of a child, which touches no GPU."""
    import os
    import subprocess
    import sys
    from conftest import ROOT
    env = {k: v for k, v in os.environ.items() if k != "SLN_STORE_POLICY"}
    code = "import importlib; print(importlib.import_module('3d_sln_amd._lib').lib().sln_get_store_policy())"
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, check=True).stdout
    assert int(out.strip().splitlines()[-1]) == NT_WT, out


def test_header_declares_the_switch_and_the_abi_agreement_holds():
    text = open(test_abi.HEADER).read()
    for name in ("sln_set_store_policy", "sln_get_store_policy", "sln_parse_store_policy_env"):
        assert re.search(r"\b%s\s*\(" % name, text), name + " missing from include/sln_hip.h"
        assert name in pkg("_lib").SIGNATURES, name + " missing from the ctypes table"
    test_abi.test_header_ctypes_table_and_library_agree()
