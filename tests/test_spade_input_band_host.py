"""The banded form of the resize operator the device input builder applies (host/spade_input.py::band_table) against the dense
``resize_matrix``, and the label <-> mask helpers.  CPU only: what the kernels in csrc/spade_input.hip compute is held to the dense
path in tests/test_spade_input_gpu.py."""
import numpy as np
import pytest
import torch

from conftest import pkg
from oracle import spade_input_ref as R

SHAPES = ((1024, 256), (1000, 256), (768, 256), (512, 256), (96, 32), (40, 40))


def _dense(first, weights, n_in):
    D = np.zeros((len(first), n_in))
    for o, f in enumerate(first):
        D[o, f:f + weights.shape[1]] = weights[o]
    return D


@pytest.mark.parametrize("n_in,n_out", SHAPES)
def test_band_table_against_dense_matrix(n_in, n_out):
    S = pkg("host.spade_input")
    eps = 1e-12
    first, weights = S.band_table(n_in, n_out, eps)
    assert first.dtype == np.int32 and first.shape == (n_out,) and weights.dtype == np.float64 and weights.shape[0] == n_out
    width = weights.shape[1]
    assert first.min() >= 0 and (first + width).max() <= n_in, (first.min(), (first + width).max(), n_in)
    full = S.resize_matrix(n_in, n_out)
    D = _dense(first, weights, n_in)
    kept = _dense(first, np.ones_like(weights), n_in) > 0
    assert np.array_equal(D[kept], full[kept])                                   # what is kept is the matrix entry itself
    dropped = np.abs(np.where(kept, 0.0, full))
    assert dropped.max() <= eps, "largest dropped entry %.3e" % dropped.max()
    row_err, width_dropped = dropped.sum(1).max(), n_in - width
    print("band %d -> %d: width %d, largest dropped entry %.3e, largest row sum of dropped magnitudes %.3e" % (n_in, n_out, width, dropped.max(),
                                                                                                      row_err))
    assert row_err < width_dropped * eps, "row sum of dropped magnitudes %.3e, bound %d * eps" % (row_err, width_dropped)
    assert S.band_table(n_in, n_out, eps)[1] is weights                          # cached like resize_matrix


def test_band_width_of_the_flagship_shape():
    S = pkg("host.spade_input")
    width = S.band_table(1024, 256)[1].shape[1]
    assert width <= 64, width
    assert S.band_table(40, 40)[1].shape[1] == 1 and np.array_equal(S.band_table(40, 40)[0], np.arange(40))
    assert S.band_table(1024, 256, 1e-17)[1].shape[1] >= width


def _apply_banded(first, weights, X):
    """rows of the band applied to axis 0 of X, k ascending like the kernel"""
    out = np.zeros((len(first),) + X.shape[1:])
    for k in range(weights.shape[1]):
        out += weights[:, k].reshape((-1,) + (1,) * (X.ndim - 1)) * X[first + k]
    return out


def test_banded_resize_equals_dense_on_the_synthetic_scene():
    S = pkg("host.spade_input")
    depth, masks = R.synth_scene(256)
    total = np.zeros((41, 256, 256), np.float32)
    total[0] = S.normalise_depth(torch.from_numpy(depth)).numpy()
    for name, m in masks.items():
        total[1 + S.NYU40.index(name)] = np.where(m < 120, 0.0, np.where(m > 120, 1.0, m))
    M = S.resize_matrix(256, 64)
    want = np.einsum("oi,cij,pj->cop", M, total.astype(np.float64), M)
    first, weights = S.band_table(256, 64)
    rows = _apply_banded(first, weights, total.astype(np.float64).transpose(1, 0, 2))          # [64, 41, 256]
    got = _apply_banded(first, weights, rows.transpose(2, 1, 0)).transpose(1, 2, 0)            # [41, 64, 64]
    err = np.abs(got - want) / np.maximum(1.0, np.abs(want))
    assert err.max() <= 1e-9, err.max()
    assert np.abs(want[1 + S.NYU40.index("bed")]).max() > 2                              # the row held at 120 is in the comparison


def test_labels_and_masks_round_trip():
    S = pkg("host.spade_input")
    rng = np.random.default_rng(4)
    labels = torch.from_numpy(rng.choice(np.array([0, 1, 4, 32, 40], np.uint8), size=(24, 20)))
    masks = S.masks_from_labels(labels)
    assert sorted(masks) == sorted(["wall", "bed", "night_stand", "otherprop"])
    for name, m in masks.items():
        assert m.dtype == torch.uint8 and set(m.unique().tolist()) <= {0, 255}
        assert torch.equal(m == 255, labels == 1 + S.NYU40.index(name))
    assert sum(int((m == 255).sum()) for m in masks.values()) == int((labels > 0).sum())
    back = S.labels_from_masks(masks)
    assert back.dtype == torch.uint8 and torch.equal(back, labels)
    with pytest.raises(ValueError):
        S.labels_from_masks({"bed": masks["bed"], "wall": masks["bed"]})
