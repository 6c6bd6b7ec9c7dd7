"""Golden fixture for ``filters.fill_masked``, generated FROM THE REFERENCE's ``fill_placeholder_with_nearest``
(datasets.py:222-250):

    python tests/golden/make_golden_filters.py          (needs the reference checkout make_golden_data.py points at)

``datasets.py`` is loaded the way ``make_golden_data.py`` loads it.  Nothing of the reference is copied: the fixture
holds the input (T, H, W, V) = (6, 20, 18, 2) in fp64 with 20 % of the points set to -9999 from a fixed seed, the array the
reference function returned for it, and ``d_min`` -- the smallest value of the smoothed valid mask at a gap, per variable
the same ``gaussian_filter(valid_mask, sigma=3)`` the function divides by.  The tests' tolerance divides by ``d_min``, so
the fixture is only written when ``d_min >= 0.5``.
"""
from __future__ import annotations

import os

import numpy as np
from scipy.ndimage import gaussian_filter

from make_golden_data import load_reference_datasets

HERE = os.path.dirname(os.path.abspath(__file__))
SEED, PLACEHOLDER, SIGMA = 2025, -9999.0, 3


def main():
    ds_mod = load_reference_datasets()
    rs = np.random.RandomState(SEED)
    t, h, w, v = 6, 20, 18, 2
    x = rs.randn(t, h, w, v) * np.array([3.0, 0.5]) + np.array([10.0, -2.0])     # two variables of different scale
    x[rs.rand(t, h, w, v) < 0.2] = PLACEHOLDER
    out = ds_mod.fill_placeholder_with_nearest(x.copy(), placeholder=PLACEHOLDER, sigma=SIGMA)
    gaps = x <= PLACEHOLDER
    d_min = min(gaussian_filter(1.0 - gaps[..., i].astype(float), sigma=SIGMA)[gaps[..., i]].min() for i in range(v))
    assert d_min >= 0.5, f"d_min {d_min}: pick another seed"
    assert np.array_equal(out[~gaps], x[~gaps]) and not (out <= PLACEHOLDER).any()
    np.savez_compressed(os.path.join(HERE, "fill_nearest_6x20x18x2.npz"), input=x, output=out, d_min=np.float64(d_min),
                        placeholder=np.float64(PLACEHOLDER), sigma=np.float64(SIGMA), seed=np.int64(SEED))
    print(f"wrote fill_nearest_6x20x18x2.npz: {int(gaps.sum())} gaps of {x.size}, d_min {d_min:.4f}")


if __name__ == "__main__":
    main()
