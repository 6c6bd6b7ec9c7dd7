"""Dataset preparation on the device: what ``load_data()`` / ``load_data_with_augmentation()`` of the reference's
``datasets.py`` do in numpy on the host between reading the arrays and handing them to the dataset.

* ``ChannelScaler`` -- sklearn's ``StandardScaler`` per channel of a channel-last tensor: ``load_data``'s
  ``scaler.fit_transform(hr_aux[..., i].reshape(-1, 1))`` loop over the last axis in one fit and one transform, and, with
  ``channel_axis=None``, the two single-feature scalers of the GRACE fields.
* ``frequency_domain_augmentation`` and ``augment_dataset`` -- the FFT / perturb / inverse FFT augmentation and the
  concatenation and tiling ``load_data_with_augmentation`` builds around it.
* ``split_indices`` / ``train_test_split`` -- the trainer's ``train_test_split(..., random_state=rand)`` with sklearn's
  indices, as a device gather.

The kernels are ``csrc/prepare.hip``: fp32 or fp64 CUDA tensors, all arithmetic fp64, one rounding to the output type, no
atomics (the same bits on every run).  There is no CPU path.

The STL decomposition that ends ``load_data()`` (``detrend_and_compare``) is ``gan_danet_amd.stl``: its trend and
detrended arrays are what ``augment_dataset`` takes.  It follows the published algorithm and is held to closed-form cases
and an independent fp64 oracle; agreement with statsmodels itself is unverified (statsmodels is not available, and the
reference's ``cache/dataset_cache.npz`` holds no recorded trend).
"""
from __future__ import annotations

import math
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import kern as K

Tensor = torch.Tensor
L = K.L


def _input(x, name: str) -> Tensor:
    if not isinstance(x, Tensor) or not x.is_cuda:
        raise L.GandanetError(f"{name}: expected a GPU tensor (there is no CPU path)")
    if x.dtype not in (torch.float32, torch.float64):
        raise L.GandanetError(f"{name}: expected float32 or float64, got {x.dtype}")
    if x.numel() == 0:
        raise L.GandanetError(f"{name}: empty tensor")
    return x if x.is_contiguous() else x.contiguous()


class ChannelScaler:
    """``sklearn.preprocessing.StandardScaler`` for every channel of a channel-last device tensor.

    ``mean_``, ``var_``, ``scale_`` (fp64 numpy, one entry per channel) and ``n_samples_seen_`` live on the host like
    sklearn's; ``fit`` reduces on the device and copies the 3 C numbers of the result once.  The variance is the
    population variance and ``scale_`` is 1 where sklearn calls the channel constant."""

    def __init__(self):
        self.mean_ = self.var_ = self.scale_ = self.n_samples_seen_ = None
        self._single = False
        self._dev = {}

    # ---- fit ---------------------------------------------------------------------------------------------------------
    def _channels(self, x: Tensor, channel_axis) -> int:
        if channel_axis is None:
            return 1
        if x.dim() == 0 or channel_axis not in (-1, x.dim() - 1):
            raise L.GandanetError("ChannelScaler: the channels are the last axis (channel_axis=-1) or there is a single "
                                  "feature (channel_axis=None)")
        return x.shape[-1]

    def fit(self, x: Tensor, channel_axis: Optional[int] = -1) -> "ChannelScaler":
        x = _input(x, "ChannelScaler.fit")
        c = self._channels(x, channel_axis)
        rec = K.channel_moments(x, c).cpu().numpy()               # the one host copy of the fit
        self._set(*K.scale_from_moments_host(rec), int(rec[0, 0]), channel_axis is None)
        return self

    def _set(self, mean, var, scale, n, single: bool) -> None:
        as64 = lambda a: np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(-1))
        self.mean_, self.var_, self.scale_ = as64(mean), as64(var), as64(scale)
        if not (self.mean_.size == self.var_.size == self.scale_.size >= 1):
            raise ValueError("mean_, var_ and scale_ must hold one value per channel")
        self.n_samples_seen_, self._single, self._dev = n, bool(single), {}

    def _params(self, device) -> Tuple[Tensor, Tensor]:
        if self.mean_ is None:
            raise L.GandanetError("ChannelScaler: not fitted")
        key = str(device)
        if key not in self._dev:
            self._dev = {key: (torch.from_numpy(self.mean_).to(device), torch.from_numpy(self.scale_).to(device))}
        return self._dev[key]

    def _check(self, x: Tensor, name: str) -> Tensor:
        x = _input(x, name)
        c = self.mean_.size if self.mean_ is not None else 0
        if not self._single and (x.dim() == 0 or x.shape[-1] != c):
            raise L.GandanetError(f"{name}: fitted on {c} channels, got a tensor of shape {tuple(x.shape)}")
        return x

    # ---- transform -----------------------------------------------------------------------------------------------------
    def transform(self, x: Tensor, out_dtype=None, to_nchw: bool = False) -> Tensor:
        """``(x - mean_) / scale_`` per channel -- sklearn's two operations in its order, in fp64 -- as a new tensor of
        ``out_dtype`` (default: the dtype of ``x``).  ``to_nchw``: an (N, H, W, C) input comes out in the dataset's stored
        (N, C, H, W) layout, the ``.float().permute(0, 3, 1, 2)`` of ``CustomDataset`` in the same pass with one rounding."""
        x = self._check(x, "ChannelScaler.transform")
        if to_nchw and self._single:
            raise L.GandanetError("ChannelScaler.transform: to_nchw needs a channel-last fit")
        mean, scale = self._params(x.device)
        return K.channel_affine(x, mean, scale, False, out_dtype, to_nchw)

    def inverse_transform(self, x: Tensor) -> Tensor:
        """``x * scale_ + mean_`` per channel of a channel-last tensor, a new tensor of the dtype of ``x``"""
        x = self._check(x, "ChannelScaler.inverse_transform")
        mean, scale = self._params(x.device)
        return K.channel_affine(x, mean, scale, True)

    def fit_transform(self, x: Tensor, channel_axis: Optional[int] = -1, out_dtype=None, to_nchw: bool = False) -> Tensor:
        return self.fit(x, channel_axis).transform(x, out_dtype, to_nchw)

    # ---- sklearn -------------------------------------------------------------------------------------------------------
    @classmethod
    def from_sklearn(cls, scalers) -> "ChannelScaler":
        """from a fitted ``StandardScaler`` (its features are the channels; a single feature is the ``channel_axis=None``
        case) or a list of single-feature ones, one per channel, as ``load_data`` returns in ``aux_scalers``.  Anything
        with ``mean_``, ``var_``, ``scale_`` and ``n_samples_seen_`` will do."""
        single = not isinstance(scalers, (list, tuple))
        items = [scalers] if single else list(scalers)
        if not items:
            raise ValueError("from_sklearn: no scalers")
        cat = lambda name: np.concatenate([np.asarray(getattr(s, name), dtype=np.float64).reshape(-1) for s in items])
        seen = [int(np.max(s.n_samples_seen_)) for s in items]
        out = cls()
        mean = cat("mean_")
        out._set(mean, cat("var_"), cat("scale_"), seen[0] if len(set(seen)) == 1 else np.array(seen), single and mean.size == 1)
        return out

    def to_sklearn(self):
        """one ``StandardScaler`` whose features are the channels"""
        from sklearn.preprocessing import StandardScaler
        if self.mean_ is None:
            raise L.GandanetError("ChannelScaler: not fitted")
        s = StandardScaler()
        s.mean_, s.var_, s.scale_ = self.mean_.copy(), self.var_.copy(), self.scale_.copy()
        s.n_samples_seen_ = self.n_samples_seen_
        s.n_features_in_ = self.mean_.size
        return s


# ---- frequency-domain augmentation --------------------------------------------------------------------------------------
def used_bins(seasonal_freq: int, n: int) -> int:
    """K1: the reference perturbs the FFT bins ``0 .. min(seasonal_freq, n - 1)`` -- its loop runs over
    ``-seasonal_freq .. seasonal_freq`` but keeps ``0 <= idx < n`` only, so the negative half never fires"""
    if int(seasonal_freq) != seasonal_freq or seasonal_freq < 0:
        raise ValueError("seasonal_freq must be a non-negative integer")
    return min(int(seasonal_freq), n - 1) + 1


def _noise_slices(noise, data: Tensor, axis: int, k1: int) -> Tensor:
    t = torch.from_numpy(np.asarray(noise)) if not isinstance(noise, Tensor) else noise
    full, want = tuple(data.shape), tuple(data.shape[:axis]) + (k1,) + tuple(data.shape[axis + 1:])
    if tuple(t.shape) not in (full, want):
        raise ValueError(f"noise must have the shape of the data {full} or hold the {k1} used slices {want}, got {tuple(t.shape)}")
    return t.narrow(axis, 0, k1).to(device=data.device, dtype=torch.float64).contiguous()


def frequency_domain_augmentation(data: Tensor, seasonal_freq: int, noise_level: float = 0.1, axis: int = 0, *, noise=None,
                                  generator: Optional[torch.Generator] = None, out: Optional[Tensor] = None) -> Tensor:
    """``frequency_domain_augmentation(data, seasonal_freq, noise_level, axis)`` of ``datasets.py``.

    The reference adds real Gaussian noise to the FFT bins ``0 .. K1 - 1`` (``K1 = min(seasonal_freq, L - 1) + 1``) along
    ``axis`` and keeps the real part of the inverse FFT; by linearity that is ``data[t] + sum_k noise[k] cos(2 pi k t / L)
    / L``, which is what the kernel evaluates, in fp64, without any transform.

    ``noise=None`` draws ``noise_level * randn`` in fp64 on the device (``generator``: a CUDA generator) for the K1 used
    bins only.  The reference draws the whole shape with numpy's global generator and uses K1 slices of it: the same
    distribution, a different stream.  ``noise=`` takes the reference's full-shape ``random_perturbation`` (numpy or
    tensor; only its first K1 slices along ``axis`` are read) or those K1 slices themselves.  The result has the dtype of
    ``data``, which is never modified; ``out=`` names a dense tensor of the same shape and dtype to write instead, for
    instance one slab of a larger buffer."""
    data = _input(data, "frequency_domain_augmentation")
    if not -data.dim() <= axis < data.dim():
        raise ValueError(f"axis {axis} is out of range for a {data.dim()}-D tensor")
    axis %= data.dim()
    n = data.shape[axis]
    k1 = used_bins(seasonal_freq, n)
    if k1 > L.FREQ_MAX_BINS:
        raise L.GandanetError(f"frequency_domain_augmentation: seasonal_freq {seasonal_freq} uses {k1} bins, more than "
                              f"{L.FREQ_MAX_BINS}")
    shape = tuple(data.shape[:axis]) + (k1,) + tuple(data.shape[axis + 1:])
    if noise is None:
        nz = torch.randn(shape, device=data.device, dtype=torch.float64, generator=generator) * float(noise_level)
    else:
        nz = _noise_slices(noise, data, axis, k1)
    if out is None:
        out = torch.empty_like(data)
    elif not isinstance(out, Tensor) or out.shape != data.shape or out.dtype != data.dtype or out.device != data.device:
        raise L.GandanetError("frequency_domain_augmentation: out must match the data in shape, dtype and device")
    coef = torch.from_numpy(K.freq_cos_table_host(n, k1)).to(data.device)
    return K.freq_augment_axis(data, out, axis, nz, coef)


def augment_dataset(detrended05: Tensor, trend05: Tensor, detrended25: Tensor, trend25: Tensor, hr_aux: Tensor,
                    augmentation_factor: int = 2, seasonal_freq: int = 12, noise_level: float = 0.1, *,
                    noise: Optional[Sequence] = None, generator: Optional[torch.Generator] = None):
    """``load_data_with_augmentation`` behind its ``load_data()`` call: every array is followed along the time axis by
    ``augmentation_factor`` frequency-augmented copies of itself, and the trends are tiled to match (``np.tile``).

    Each (1 + f) T output is allocated once; the original goes into slab 0 and the kernel writes every augmented copy
    straight into its slab (no ``cat``).  ``noise``: None (drawn on the device), or one entry per round, each a triple
    of ``noise=`` arguments for (detrended05, detrended25, hr_aux), the order the reference draws in.
    Returns ``[detrended05_aug, trend05_rep], [detrended25_aug, trend25_rep], hr_aux_aug``."""
    f = int(augmentation_factor)
    if f < 0:
        raise ValueError("augmentation_factor must be >= 0")
    arrays = [_input(a, "augment_dataset") for a in (detrended05, detrended25, hr_aux)]
    trends = [_input(a, "augment_dataset trend") for a in (trend05, trend25)]
    t = arrays[0].shape[0]
    if any(a.shape[0] != t for a in arrays + trends):
        raise ValueError("all arrays must share the length of the time axis")
    if noise is not None and (len(noise) != f or any(len(r) != 3 for r in noise)):
        raise ValueError("noise must hold one (detrended05, detrended25, hr_aux) triple per augmentation")
    outs = []
    for a in arrays:
        buf = torch.empty(((1 + f) * t,) + tuple(a.shape[1:]), device=a.device, dtype=a.dtype)
        buf[:t].copy_(a)
        outs.append(buf)
    for r in range(f):                                              # the reference's order: per round, the three arrays
        for i, a in enumerate(arrays):
            frequency_domain_augmentation(a, seasonal_freq, noise_level, 0, noise=None if noise is None else noise[r][i],
                                          generator=generator, out=outs[i][(1 + r) * t:(2 + r) * t])
    reps = [tr.repeat((1 + f,) + (1,) * (tr.dim() - 1)) for tr in trends]
    return [outs[0], reps[0]], [outs[1], reps[1]], outs[2]


# ---- the trainer's split ---------------------------------------------------------------------------------------------------
def split_indices(n: int, test_size: float = 0.2, random_state: int = 42) -> Tuple[np.ndarray, np.ndarray]:
    """(train, test) indices of ``sklearn.model_selection.train_test_split(..., test_size, random_state)`` on ``n`` samples:
    ``perm = RandomState(random_state).permutation(n)``, test = its first ``ceil(test_size * n)`` entries, train = the rest"""
    n = int(n)
    if not 0.0 < test_size < 1.0:
        raise ValueError("test_size must be a fraction in (0, 1)")
    n_test = int(math.ceil(test_size * n))
    if n_test >= n or n_test < 1:
        raise ValueError(f"test_size {test_size} leaves an empty train or test set for n = {n}")
    perm = np.random.RandomState(random_state).permutation(n)
    return perm[n_test:], perm[:n_test]


def train_test_split(*tensors: Tensor, test_size: float = 0.2, random_state: int = 42) -> List[Tensor]:
    """sklearn's ``train_test_split(*arrays, test_size=, random_state=)`` on device tensors: for every tensor its train and
    test parts, gathered on the device along axis 0"""
    if not tensors:
        raise ValueError("at least one tensor is required")
    for t in tensors:
        if not isinstance(t, Tensor) or not t.is_cuda:
            raise L.GandanetError("train_test_split: expected GPU tensors (there is no CPU path)")
    n = tensors[0].shape[0]
    if any(t.shape[0] != n for t in tensors):
        raise ValueError("all tensors must hold the same number of samples")
    train, test = split_indices(n, test_size, random_state)
    out = []
    for t in tensors:
        for idx in (train, test):
            out.append(t.index_select(0, torch.from_numpy(idx).to(t.device)))
    return out
