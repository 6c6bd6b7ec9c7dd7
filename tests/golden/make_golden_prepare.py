"""Golden fixtures for the dataset preparation (gan_danet_amd/prepare.py), generated FROM THE REFERENCE:

    python tests/golden/make_golden_prepare.py            (build container only: needs the reference checkout)

``datasets.py`` is imported with the stand-ins of ``make_golden_data.py`` and its own ``frequency_domain_augmentation``
is run.  The function draws its noise from numpy's global generator, so numpy is seeded, the function is called, and the
same seed and the same ``np.random.normal(scale, size=shape)`` call give the draw it used.  The scalers the reference keeps
in ``cache/*.joblib`` are recorded as their plain ``mean_`` / ``scale_`` / ``var_`` / ``n_samples_seen_`` numbers.  Nothing
of the reference is copied: the fixtures hold inputs, noise, outputs and recorded results.
"""
from __future__ import annotations

import os
import warnings

import numpy as np

from make_golden_data import HERE, REF, load_reference_datasets

# name -> (shape, axis, seasonal_freq, dtype)
FREQ_CASES = {
    "t181": ((181, 6, 5, 3), 0, 12, np.float64),
    "clip": ((5, 4, 3), 0, 12, np.float64),              # L <= seasonal_freq: the bins are clipped to L
    "inner_axis": ((7, 13, 2), 1, 3, np.float64),
    "len1": ((1, 9), 0, 2, np.float64),
    "t25": ((25, 3), 0, 12, np.float64),
    "f32": ((24, 3), 0, 12, np.float32),
}
NOISE_LEVEL = 0.1


def main():
    ds_mod = load_reference_datasets()
    out = {"noise_level": np.float64(NOISE_LEVEL)}
    for i, (name, (shape, axis, freq, dtype)) in enumerate(sorted(FREQ_CASES.items())):
        x = (np.random.RandomState(100 + i).randn(*shape) * 4.0 + 1.0).astype(dtype)
        seed = 7000 + i
        np.random.seed(seed)
        want = ds_mod.frequency_domain_augmentation(x.copy(), seasonal_freq=freq, noise_level=NOISE_LEVEL, axis=axis)
        np.random.seed(seed)
        noise = np.random.normal(scale=NOISE_LEVEL, size=shape)
        out.update({f"{name}_input": x, f"{name}_noise": noise, f"{name}_output": want,
                    f"{name}_axis": np.int64(axis), f"{name}_freq": np.int64(freq)})
    np.savez_compressed(os.path.join(HERE, "prepare_freq.npz"), **out)
    print("wrote prepare_freq.npz:", len(out), "arrays")

    import joblib
    rec = {}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        loaded = {"aux": joblib.load(os.path.join(REF, "cache", "aux_scalers.joblib")),
                  "grace05": [joblib.load(os.path.join(REF, "cache", "grace_scaler_05.joblib"))],
                  "grace025": [joblib.load(os.path.join(REF, "cache", "grace_scaler_025.joblib"))]}
    for name, scalers in loaded.items():
        for attr in ("mean_", "scale_", "var_"):
            rec[f"{name}_{attr}"] = np.concatenate([np.asarray(getattr(s, attr), np.float64).reshape(-1) for s in scalers])
        rec[f"{name}_n_samples_seen_"] = np.array([int(s.n_samples_seen_) for s in scalers], np.int64)
    np.savez_compressed(os.path.join(HERE, "prepare_scalers.npz"), **rec)
    print("wrote prepare_scalers.npz:", {k: v.shape for k, v in rec.items()})


if __name__ == "__main__":
    main()
