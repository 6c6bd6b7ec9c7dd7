"""Shared by the histogram-matching tests (test_cabi_histmatch.py, test_gpu_histmatch.py, test_gpu_modules.py): the numpy
restatement of the notebook's apply_mild_histogram_matching, a bitwise comparison, and the case builders.

Why zero tolerance: the per-element code (csrc/histmatch_core.h) performs the same IEEE double divisions, products and sums
as numpy's cumsum / interp, with contraction into FMA switched off, and its bracket decisions are integer comparisons; the
(1 - weight) * source term is a float32 product on both sides.  So equal bits are a property of the arithmetic."""
import functools

import numpy as np

WEIGHTS = (0.0, 0.35, 0.6, 1.0)
GRID_STRIDE_NS = 2048 * 256 + 257      # the grid is capped at 2048 workgroups of 256 threads: 257 threads take a second item


def restatement(source, reference, weight):
    """one sample, test.ipynb c1:69-85 as the notebook writes it; float32 in, float64 out, shaped like ``source``"""
    oldshape = source.shape
    source, reference = source.ravel(), reference.ravel()
    s_vals, bin_idx, s_counts = np.unique(source, return_inverse=True, return_counts=True)
    t_vals, t_counts = np.unique(reference, return_counts=True)
    s_q = np.cumsum(s_counts).astype(np.float64) / np.sum(s_counts)
    t_q = np.cumsum(t_counts).astype(np.float64) / np.sum(t_counts)
    matched = np.interp(s_q, t_q, t_vals)[bin_idx].reshape(oldshape)
    return ((1 - weight) * source + weight * matched.ravel()).reshape(oldshape)


def restatement_batch(src, ref, weight):
    return np.array([restatement(s, r, weight) for s, r in zip(src, ref)])


def same_bits(a, b) -> bool:
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ---- data ----------------------------------------------------------------------------------------------------------------------
def quantised(rng, B, ns, nt):
    """source values k / 4, reference values k / 3, k in -3 .. 3: runs of equal values on both sides"""
    src = (rng.integers(-3, 4, size=(B, ns)) / 4).astype(np.float32)
    ref = (rng.integers(-3, 4, size=(B, nt)).astype(np.float32) / np.float32(3)).astype(np.float32)
    return src, ref


def continuous(rng, B, ns, nt):
    return rng.standard_normal((B, ns)).astype(np.float32), (rng.standard_normal((B, nt)) * 2 + 1).astype(np.float32)


def distinct(rng, B, n, scale=1.0, shift=0.0):
    """(B, n) float32, all values of a sample different: a shuffled grid with a spacing no float32 rounding can close"""
    base = (np.arange(n, dtype=np.float64) - n / 3) * 0.37 * scale + shift
    out = np.stack([rng.permutation(base) for _ in range(B)]).astype(np.float32)
    assert all(np.unique(row).size == n for row in out)
    return out


def small_pairs():
    """every (ns, nt) in 1 .. 12 x 1 .. 12, quantised and continuous, two samples each: (kind, src, ref)"""
    rng = np.random.default_rng(20240611)
    for ns in range(1, 13):
        for nt in range(1, 13):
            yield ("quantised", *quantised(rng, 2, ns, nt))
            yield ("continuous", *continuous(rng, 2, ns, nt))


def random_cases(count=3000, seed=7):
    """seeded cases with ns, nt < 40, alternately heavily tied and continuous: (src, ref, weight)"""
    rng = np.random.default_rng(seed)
    for k in range(count):
        ns, nt = int(rng.integers(1, 40)), int(rng.integers(1, 40))
        src, ref = (quantised if k % 2 == 0 else continuous)(rng, 1, ns, nt)
        yield src, ref, WEIGHTS[int(rng.integers(0, 4))]


def with_nans(src, rng, share=0.05):
    """``share`` of every sample replaced by NaN, every second one of them with the sign bit set (the negation of a NaN);
    returns (src, mask of the NaN positions)"""
    src = src.copy()
    mask = np.zeros(src.shape, dtype=bool)
    for b in range(src.shape[0]):
        pos = rng.permutation(src.shape[1])[:max(2, int(round(share * src.shape[1])))]
        src[b, pos] = np.float32(np.nan)
        src[b, pos[1::2]] = -src[b, pos[1::2]]
        mask[b, pos] = True
    bits = src.view(np.uint32)[mask]
    assert np.isnan(src[mask]).all() and (bits >> 31 == 1).any() and (bits >> 31 == 0).any()
    return src, mask


@functools.lru_cache(maxsize=None)
def nan_cases():
    """(name, src, ref, weight, nan mask): 5 % NaNs of both signs in a continuous and in a heavily tied source"""
    rng = np.random.default_rng(99)
    out = []
    for name, maker, ns, nt, w in (("continuous", continuous, 4001, 997, 0.35), ("quantised", quantised, 3000, 500, 1.0),
                                   ("short", continuous, 40, 17, 0.6)):
        src, ref = maker(rng, 2, ns, nt)
        src, mask = with_nans(src, rng)
        out.append((f"nan {name}", src, ref, w, mask))
    return tuple(out)


def _extremes(rng):
    tiny, big = np.float32(1e-45), np.finfo(np.float32).max           # the smallest denormal, FLT_MAX
    special = np.array([0.0, -0.0, 0.0, -0.0, tiny, -tiny, 3 * tiny, np.float32(1e-39), np.float32(-1e-39), big, -big, big,
                        np.finfo(np.float32).tiny, 1.0, -1.0], dtype=np.float32)
    src = np.concatenate([special, special[:6], rng.standard_normal(70).astype(np.float32)])
    ref = np.concatenate([special[::-1], rng.standard_normal(40).astype(np.float32) * np.float32(1e-38)])
    return np.stack([rng.permutation(src), rng.permutation(src)]), np.stack([rng.permutation(ref), rng.permutation(ref)])


@functools.lru_cache(maxsize=None)
def device_cases():
    """the cases of test_gpu_histmatch.py: name -> (src (B, ns), ref (B, nt), weight, exact zero signs?).  Built once."""
    rng = np.random.default_rng(314159)
    cases = {}
    # grid-stride: the smallest size at which a thread takes a second item
    s, r = quantised(rng, 1, GRID_STRIDE_NS, 7)
    cases["grid-stride nt=7 tied"] = (s, r, 0.35, True)
    s, r = continuous(rng, 1, GRID_STRIDE_NS, 49999)
    cases["grid-stride nt=49999 continuous"] = (s, r, 0.6, True)
    # a source quantile equal to a reference quantile: the xpj == x branch
    cases["ties ns=nt=4096 distinct"] = (distinct(rng, 1, 4096), distinct(rng, 1, 4096, 1.7, 2.0), 0.6, True)
    cases["ties ns=4nt distinct"] = (distinct(rng, 1, 4096), distinct(rng, 1, 1024, 0.9, -1.0), 1.0, True)
    # x * nt rounds across an integer.  At the last six pairs floor((k / ns) * nt) is one below the largest c with
    # c / nt <= k / ns for 7, 2, 3, 5, 7 and 6 values of k (numpy, float64), so the upward correction loop decides the bracket
    for ns, nt in ((3, 49), (49, 3), (7, 1000), (1000, 7), (997, 991), (49, 49), (11, 55), (22, 110), (47, 47), (55, 55), (71, 71)):
        cases[f"rounding {ns}x{nt}"] = (distinct(rng, 2, ns), distinct(rng, 2, nt, 1.3, 0.5), 0.35, True)
    # the same six pairs on a reference spread over twelve decades: there a bracket one too low, which interpolates up to the
    # value that the right bracket returns as it is, shows in the last bits (neighbours differ by orders of magnitude)
    for ns, nt in ((49, 49), (11, 55), (22, 110), (47, 47), (55, 55), (71, 71)):
        wide = (rng.standard_normal((4, nt)) * 10.0 ** rng.uniform(-6, 6, size=(4, nt))).astype(np.float32)
        assert all(np.unique(row).size == nt for row in wide)
        cases[f"rounding {ns}x{nt} wide"] = (distinct(rng, 4, ns), wide, 1.0, True)
    # degenerate sizes, constant inputs
    cases["degenerate ns=1"] = (*continuous(rng, 2, 1, 50), 0.6, True)
    cases["degenerate nt=1"] = (*continuous(rng, 2, 50, 1), 0.6, True)
    cases["degenerate ns=nt=1"] = (*continuous(rng, 2, 1, 1), 0.35, True)
    s, r = continuous(rng, 2, 300, 64)
    cases["constant reference"] = (s, np.full_like(r, 0.5), 0.6, True)
    cases["constant source"] = (np.full_like(s, 1.25), r, 0.35, True)
    # batch: another permutation and scale per sample, one sample sorted descending
    base, rbase = rng.standard_normal(1000), rng.standard_normal(777)
    s = np.stack([rng.permutation(base) * 1.0, rng.permutation(base) * 3.5, np.sort(base)[::-1] * 0.25]).astype(np.float32)
    r = np.stack([rng.permutation(rbase) * 2.0, np.sort(rbase)[::-1] * 0.5, rng.permutation(rbase) * 7.0]).astype(np.float32)
    cases["batch of 3"] = (s, r, 0.35, True)
    s, r = quantised(rng, 3, 1000, 300)
    cases["batch of 3 tied"] = (s * np.array([[1.0], [2.0], [0.5]], dtype=np.float32), r, 1.0, True)
    # denormals, +-FLT_MAX, mixed zeros: values only, numpy does not define which of the equal zeros np.unique keeps
    cases["extremes"] = (*_extremes(rng), 0.35, False)
    return cases


@functools.lru_cache(maxsize=None)
def device_want(name):
    """the restatement of one device case, computed once and shared (read only)"""
    src, ref, w, _ = device_cases()[name]
    want = restatement_batch(src, ref, w)
    want.setflags(write=False)
    return want


def agree(got, want, exact_zero_sign: bool) -> bool:
    """bit for bit; ``exact_zero_sign`` False: == on the values (the extremes case)"""
    if exact_zero_sign:
        return same_bits(got, want)
    return got.dtype == want.dtype and got.shape == want.shape and bool(np.all(got == want))
