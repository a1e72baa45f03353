"""What the operand-level GPU suites (test_gemm_family_gpu.py, test_vae_kernels_gpu.py) share."""
import pytest
import torch

from conftest import pkg

SENT = -777.25          # prefill of everything a kernel must not touch


def _lib():
    L = pkg("_lib")
    assert L.lib().sln_device_ok() == 0
    return L


class Dev:
    """Uploads each CPU tensor once and keeps both alive; device tensors pass through."""

    def __init__(self):
        self.m = {}

    def __call__(self, t):
        if t is None:
            return None
        if t.is_cuda:
            return t.data_ptr()
        k = id(t)
        if k not in self.m:
            assert t.is_contiguous()
            self.m[k] = (t, t.cuda())
        return self.m[k][1].data_ptr()


def _sync(what):
    """A HIP error after a launch is a fault of the device context: nothing more may run on the GPU in this session."""
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit("GPU fault after %s: %s" % (what, e), returncode=3)


def _first_bad(err, tol):
    bad = (err > tol).nonzero()
    return tuple(int(v) for v in bad[0]) if bad.numel() else None


def _assert_close(got, ref, rtol, atol, what, route):
    ref = ref.double()
    scale = float(ref.abs().max()) if ref.numel() else 0.0
    tol = atol * max(1.0, scale) + rtol * scale
    err = (got.double() - ref).abs()
    e = float(err.max()) if err.numel() else 0.0
    assert e == e and e <= tol, "%s: max err %.3e > %.3e (scale %.3e), first failing (row, column) %s; route: %s" % (
        what, e, tol, scale, _first_bad(err, tol), route)
    return e, tol
