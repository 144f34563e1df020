"""Host side of the comparison of two uint8 volumes: compare_from_joint and regression_lut on joint histograms built
with numpy, against direct numpy on the voxels and against known answers, and the argument checks of `compare=` that
are made before any GPU work.  No GPU is needed."""
import math

import numpy as np
import pytest

from transfer_em_amd import debug
from transfer_em_amd.utils import compare_from_joint, predict_cube, predict_volume, regression_lut


def _joint(a, b):
    return np.bincount(a.ravel().astype(np.int64) * 256 + b.ravel(), minlength=65536).reshape(256, 256)


def _entropy(counts):
    p = counts[counts > 0].astype(np.float64) / counts.sum()
    return float(-(p * np.log2(p)).sum())


@pytest.fixture(scope="module")
def pair():
    rng = np.random.default_rng(41)
    a = np.clip(rng.normal(120, 30, (40, 50, 70)), 0, 255).astype(np.uint8)
    b = np.clip(a.astype(np.int64) + rng.integers(-6, 7, a.shape), 0, 255).astype(np.uint8)
    return a, b


def test_compare_from_joint_equals_numpy_on_the_voxels(pair):
    a, b = pair
    J = _joint(a, b)
    m = compare_from_joint(J)
    d = b.astype(np.int64) - a.astype(np.int64)
    assert m["n"] == a.size and isinstance(m["sum_sq_diff"], int) and isinstance(m["sum_abs_diff"], int)
    assert m["sum_abs_diff"] == int(np.abs(d).sum()) and m["sum_sq_diff"] == int((d * d).sum())
    assert m["rmse"] == math.sqrt(m["sum_sq_diff"] / m["n"]) and m["mae"] == m["sum_abs_diff"] / m["n"]
    assert m["bias"] == pytest.approx(d.mean(), rel=1e-12)
    assert m["psnr"] == pytest.approx(20 * math.log10(255 / m["rmse"]), rel=1e-12)
    scaled = lambda v: v.astype(np.float64) / 127.5 - 1.0
    assert m["rmse_scaled"] == pytest.approx(debug.accuracy(scaled(a), scaled(b)), rel=1e-12)
    assert m["pearson"] == pytest.approx(np.corrcoef(a.ravel().astype(np.float64), b.ravel().astype(np.float64))[0, 1],
                                         rel=1e-12)
    h_a, h_b, h_ab = _entropy(np.bincount(a.ravel(), minlength=256)), _entropy(np.bincount(b.ravel(), minlength=256)), \
        _entropy(J.ravel())
    assert m["entropy_a"] == pytest.approx(h_a, rel=1e-12) and m["entropy_b"] == pytest.approx(h_b, rel=1e-12)
    assert m["mutual_information"] == pytest.approx(h_a + h_b - h_ab, rel=1e-12) and m["mutual_information"] > 1
    assert m["hist_a"].dtype == np.int64 and np.array_equal(m["hist_a"], np.bincount(a.ravel(), minlength=256))
    assert np.array_equal(m["hist_b"], np.bincount(b.ravel(), minlength=256))
    assert compare_from_joint(J.astype(np.uint32))["sum_sq_diff"] == m["sum_sq_diff"]


def test_compare_from_joint_known_answers(pair):
    a, _ = pair
    same = compare_from_joint(_joint(a, a))
    assert same["rmse"] == 0 and same["mae"] == 0 and same["bias"] == 0 and same["psnr"] == math.inf
    assert same["mutual_information"] == same["entropy_a"] == same["entropy_b"] and same["entropy_a"] > 5
    assert same["pearson"] == pytest.approx(1.0, abs=1e-12)
    inv = compare_from_joint(_joint(a, 255 - a))
    assert inv["pearson"] == pytest.approx(-1.0, abs=1e-12) and inv["rmse"] > 0
    const = compare_from_joint(_joint(a, np.full_like(a, 77)))
    assert const["mutual_information"] == 0 and const["entropy_b"] == 0 and math.isnan(const["pearson"])
    assert math.isnan(compare_from_joint(_joint(np.full_like(a, 3), a))["pearson"])
    one = np.zeros((256, 256), np.int64)
    one[10, 13] = 2 ** 40                                                # sums past 2^53 stay exact integers
    m = compare_from_joint(one)
    assert m["n"] == 2 ** 40 and m["sum_sq_diff"] == 9 * 2 ** 40 and m["sum_abs_diff"] == 3 * 2 ** 40
    assert m["bias"] == 3 and m["rmse"] == 3


def test_regression_lut(pair):
    a, _ = pair
    t = (255 - (np.arange(256) // 2) * 2).astype(np.uint8)               # the non-bijective table of test_gpu_histogram
    got = regression_lut(_joint(a, t[a]))
    seen = np.unique(a)
    assert got.dtype == np.uint8 and got.shape == (256,) and len(seen) > 100
    assert np.array_equal(got[seen], t[seen])
    got = regression_lut(_joint(np.array([5, 5, 9], np.uint8), np.array([10, 11, 3], np.uint8)))
    assert got[5] == 11 and got[9] == 3                                  # 10.5 rounds up
    assert got[7] == 11                                                  # the tie goes to the lower value
    assert got[6] == 11 and got[8] == 3 and got[0] == 11 and got[255] == 3


@pytest.mark.parametrize("fn", [compare_from_joint, regression_lut])
def test_joint_tables_are_checked(fn):
    good = np.zeros((256, 256), np.int64)
    good[1, 2] = 1
    fn(good)
    neg = good.copy()
    neg[0, 0] = -1
    for bad in (np.zeros((256, 256), np.int64), neg, good.astype(np.float64), good[:255], good.ravel(), good[None]):
        with pytest.raises(ValueError):
            fn(bad)


class _NoGenerator:
    """Enough of a model for the checks made ahead of the GPU: every one of them must raise before it is used."""
    outdimsize, buffer, device, generator_g = 36, 19, "cpu", None


@pytest.mark.parametrize("predict", [predict_cube, predict_volume])
def test_compare_is_checked_before_any_gpu_work(predict):
    vol = np.zeros((8, 9, 10), np.uint8)
    cases = [(vol, None), (vol, []),                                     # stats must be a dict
             (vol.astype(np.float32), {}), (vol[:7], {}), (vol[0], {}), (vol.tolist(), {}), (True, {})]
    for compare, stats in cases:
        with pytest.raises(ValueError, match="compare"):
            predict(vol, (0, 0, 0), (10, 9, 8), _NoGenerator(), (0, 1), (0, 1), compare=compare, stats=stats)
