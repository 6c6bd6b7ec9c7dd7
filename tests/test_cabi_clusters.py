"""CPU: the connected-component entry points of the C ABI (include/gandanet.h, "Connected components") are declared, bound
and re-exported, refuse every bad argument before any launch, and the host twins -- plain C++ over csrc/ccl_core.h -- give
scipy.ndimage.label's labels and count exactly on every case and structure of tests/clusters_util.py, exact integer tables,
and fp64 fields inside the summation bound derived there.  Each test prints its largest error over its bound (pytest -s)."""
import os

import numpy as np
import pytest
import torch

import clusters_util as U

NAMES = ("gd_ccl_label", "gd_ccl_filter", "gd_ccl_relabel", "gd_ccl_bounds", "gd_ccl_offsets", "gd_ccl_tracks", "gd_ccl_totals")


def _lib():
    from gan_danet_amd import _lib
    return _lib, _lib.load()


def test_cluster_symbols_are_declared_and_bound():
    import gan_danet_amd
    from gan_danet_amd import build, clusters, kern
    L, lib = _lib()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "include", "gandanet.h")).read()
    assert "Connected components (ccl.hip, csrc/ccl_core.h)" in src
    for name in NAMES + ("gd_ccl_ws_bytes",):
        for nm in ((name,) if name == "gd_ccl_ws_bytes" else (name, name + "_host")):
            assert nm + "(" in src and nm in L.SIGNATURES and hasattr(lib, nm), nm
            assert nm == "gd_ccl_ws_bytes" or hasattr(kern, nm[3:]), nm
    for nm, v in (("TILE_T", L.CCL_TILE_T), ("TILE_H", L.CCL_TILE_H), ("TILE_W", L.CCL_TILE_W), ("U8", L.CCL_U8),
                  ("STRUCT_BITS", L.CCL_STRUCT_BITS)):
        assert f"#define GD_CCL_{nm} {v}" in src, nm
    assert L.CCL_TILE_T * L.CCL_TILE_H * L.CCL_TILE_W == 1024 and L.CCL_STRUCT_BITS == 13
    assert f"GD_CCL_NO_TILES = {L.CCL_NO_TILES}" in src and f"GD_CCL_SEVERITY = {L.CCL_SEVERITY}" in src
    for prefix, table, total in (("B", L.CCL_BOUNDS, "BOUNDS"), ("TR", L.CCL_TRACK, "TRACK"), ("TO", L.CCL_TOTALS, "TOTALS")):
        for k, name in enumerate(table):
            assert f"GD_CCL_{prefix}_{name.upper()} = {k}" in src, name
        assert f"GD_CCL_{total} = {len(table)}" in src
    assert "ccl.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "ccl_core.h"))
    assert gan_danet_amd.clusters is clusters
    for name in ("DroughtClusters", "drought_clusters", "label_components", "structure_word"):
        assert getattr(gan_danet_amd, name) is getattr(clusters, name)
    assert lib.gd_ccl_ws_bytes(0) == 0 and lib.gd_ccl_ws_bytes(100_000) >= 4 * 100_000


def test_structure_words():
    from gan_danet_amd import _lib as L
    from gan_danet_amd import clusters as C
    for s in U.STRUCTURES:
        assert C.structure_word(s) == U.word_oracle(s), U.structure_id(s)
        assert C.structure_word(U.structure_array(s)) == U.word_oracle(s)
    assert C.structure_word(1) == (1 << 4) | (1 << 10) | (1 << 12) and C.structure_word(3) == (1 << 13) - 1
    assert C.structure_word("planar4") == (1 << 10) | (1 << 12) and C.structure_word("planar8") == 0x1E00 == C.PLANAR_BITS
    one_sided = U.structure_array(1).copy()
    one_sided[0, 1, 1] = False
    no_centre = U.structure_array(2).copy()
    no_centre[1, 1, 1] = False
    for bad in (one_sided, no_centre, 0, 4, "planar6", np.ones((3, 3), dtype=bool), True):
        with pytest.raises(L.GandanetError):
            C.structure_word(bad)


def _refused(L, fn, order, good, rules, host, tail=(None,), drop=()):
    for kw, word in rules:
        v = dict(good, **kw)
        args = [v[k] for k in order if not (host and k in drop)]
        rc = fn(*args) if host else fn(*args, *tail)
        assert rc == -1, (fn.__name__, kw, rc)
        assert word in L.last_error(), (fn.__name__, kw, L.last_error())


def test_cluster_argument_errors_before_any_launch():
    """-1 + gd_last_error with no GPU: validation comes first, so the pointers (never-dereferenced addresses) are not
    touched"""
    L, lib = _lib()
    a, b, c, d, e, f = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 0x6000
    big = 1 << 20
    cube = [(dict(T=0), "<= 0"), (dict(H=0), "<= 0"), (dict(W=0), "<= 0"), (dict(T=-3), "<= 0"), (dict(H=-1), "<= 0"), (dict(W=-7), "<= 0"),
            (dict(T=1 << 11, H=1 << 10, W=1 << 10), "2^31"), (dict(T=1 << 31, H=1, W=1), "2^31"), (dict(T=1 << 40, H=1 << 40, W=1 << 40), "2^31")]
    for host in (False, True):
        sfx = "_host" if host else ""
        order = ("x", "dtype", "T", "H", "W", "threshold", "mask", "structure", "flags", "parent")
        good = dict(x=a, dtype=1, T=9, H=17, W=65, threshold=-0.8, mask=None, structure=0x1FFF, flags=0, parent=b)
        rules = [(dict(x=None), "null"), (dict(parent=None), "null"), (dict(dtype=3), "dtype"), (dict(dtype=-1), "dtype"),
                 (dict(threshold=float("nan")), "threshold"), (dict(structure=1 << 13), "structure"), (dict(structure=-1), "structure"),
                 (dict(structure=0x3FFF), "structure"), (dict(flags=2), "flags"), (dict(x=a + 4), "aligned"),
                 (dict(x=a + 2, dtype=0), "aligned"), (dict(parent=b + 2), "aligned")]
        _refused(L, getattr(lib, "gd_ccl_label" + sfx), order, good, rules + cube, host)

        order = ("parent", "n", "min_size", "ws", "ws_bytes")
        good = dict(parent=a, n=1000, min_size=2, ws=b, ws_bytes=big)
        rules = [(dict(parent=None), "null"), (dict(n=0), "n <= 0"), (dict(n=-5), "n <= 0"), (dict(n=1 << 31), "2^31"),
                 (dict(min_size=0), "min_size"), (dict(min_size=-1), "min_size"), (dict(parent=a + 1), "aligned")]
        dev = [(dict(ws=None), "workspace"), (dict(ws=b + 2), "workspace"), (dict(ws_bytes=4000), "workspace")]
        _refused(L, getattr(lib, "gd_ccl_filter" + sfx), order, good, rules + ([] if host else dev), host, drop=("ws", "ws_bytes"))

        order = ("parent", "n", "labels", "count", "ws", "ws_bytes")
        good = dict(parent=a, n=1000, labels=b, count=c, ws=d, ws_bytes=big)
        rules = [(dict(parent=None), "null"), (dict(labels=None), "null"), (dict(count=None), "null"), (dict(n=0), "n <= 0"),
                 (dict(n=1 << 31), "2^31"), (dict(labels=b + 2), "aligned"), (dict(count=c + 1), "aligned")]
        _refused(L, getattr(lib, "gd_ccl_relabel" + sfx), order, good, rules + ([] if host else dev), host, drop=("ws", "ws_bytes"))

        order = ("labels", "T", "H", "W", "K", "bounds")
        good = dict(labels=a, T=9, H=17, W=65, K=5, bounds=b)
        rules = [(dict(labels=None), "null"), (dict(bounds=None), "null"), (dict(K=0), "K <= 0"), (dict(K=-2), "K <= 0"),
                 (dict(labels=a + 2), "aligned"), (dict(bounds=b + 1), "aligned")]
        _refused(L, getattr(lib, "gd_ccl_bounds" + sfx), order, good, rules + cube, host)

        order = ("bounds", "K", "offsets", "ws", "ws_bytes")
        good = dict(bounds=a, K=5, offsets=b, ws=c, ws_bytes=big)
        rules = [(dict(bounds=None), "null"), (dict(offsets=None), "null"), (dict(K=0), "K <= 0"), (dict(offsets=b + 2), "aligned")]
        dev = [(dict(ws=None), "workspace"), (dict(ws_bytes=8), "workspace")]
        _refused(L, getattr(lib, "gd_ccl_offsets" + sfx), order, good, rules + ([] if host else dev), host, drop=("ws", "ws_bytes"))

        order = ("x", "dtype", "T", "H", "W", "threshold", "labels", "bounds", "offsets", "K", "R", "weights", "flags", "tracks", "index")
        good = dict(x=a, dtype=1, T=9, H=17, W=65, threshold=-0.8, labels=b, bounds=c, offsets=d, K=5, R=12, weights=None, flags=1, tracks=e,
                    index=f)
        rules = [(dict(labels=None), "null"), (dict(bounds=None), "null"), (dict(offsets=None), "null"), (dict(tracks=None), "null"),
                 (dict(index=None), "null"), (dict(dtype=3), "dtype"), (dict(K=0), "K <= 0"), (dict(R=4), "R outside"),
                 (dict(R=9 * 17 * 65 + 1), "R outside"), (dict(flags=2), "flags"),
                 (dict(dtype=2, weights=a, flags=1), "uint8"), (dict(dtype=2, flags=1), "uint8"), (dict(x=None, flags=1), "without x"),
                 (dict(threshold=float("nan")), "threshold"), (dict(x=a + 4), "aligned"), (dict(weights=a + 4), "aligned"),
                 (dict(tracks=e + 4), "aligned"), (dict(index=f + 2), "aligned")]
        _refused(L, getattr(lib, "gd_ccl_tracks" + sfx), order, good, rules + cube, host)

        order = ("tracks", "bounds", "offsets", "K", "totals")
        good = dict(tracks=a, bounds=b, offsets=c, K=5, totals=d)
        rules = [(dict(tracks=None), "null"), (dict(totals=None), "null"), (dict(bounds=None), "null"), (dict(offsets=None), "null"),
                 (dict(K=0), "K <= 0"), (dict(totals=d + 4), "aligned"), (dict(tracks=a + 4), "aligned")]
        _refused(L, getattr(lib, "gd_ccl_totals" + sfx), order, good, rules, host)


def test_the_cases_have_their_properties():
    U.check_case_properties()


@pytest.mark.parametrize("case", U.CASES, ids=repr)
def test_host_twins_against_the_oracles(case):
    from gan_danet_amd import kern as K
    worst = 0.0
    counts = []
    for s in U.STRUCTURES:
        want, kw = U.labels_oracle(case, s)
        for weights in (None, U.weights_of(case.x.shape)):
            parent, labels, k, bounds, offsets, tracks, index, totals = U.host_pipeline(K, case, s, weights)
            assert k == kw and np.array_equal(labels, want), (case, U.structure_id(s))
            # parent is the smallest raster index of the component
            fg = labels > 0
            flat = parent.reshape(-1)
            assert np.all(flat[~fg.reshape(-1)] == -1) and np.all(flat[fg.reshape(-1)] <= np.flatnonzero(fg))
            assert np.array_equal(np.unique(flat[flat >= 0]), np.flatnonzero(flat == np.arange(flat.size)))
            if k == 0:
                continue
            assert np.array_equal(bounds, U.bounds_oracle(want, k)), (case, U.structure_id(s))
            values = case.x.dtype != np.uint8
            worst = max(worst, U.check_tracks(case, want, bounds, offsets, tracks, index, weights, values),
                        U.check_totals(bounds, offsets, tracks, totals, values))
        counts.append(kw)
    print(f"{case}: K = {counts} over {[U.structure_id(s) for s in U.STRUCTURES]}; labels, K and integer tables exact; "
          f"fp64 fields at most {worst:.3f} of the summation bound")


@pytest.mark.parametrize("name", ["random0.35", "index-f64", "serpentine"])
def test_host_label_without_tiles_flag_is_the_same(name):
    from gan_danet_amd import kern as K
    case = {c.name: c for c in U.CASES}[name]
    for s in U.STRUCTURES:
        assert np.array_equal(U.host_pipeline(K, case, s, tiles=False)[0], U.host_pipeline(K, case, s)[0])


@pytest.mark.parametrize("name", ["random0.35", "index-f64", "index-f32"])
def test_per_step_patch_filter_recipe_on_the_host(name):
    """min_step_pixels: label every step with the spatial part of the structure, drop the small patches, link the rest in
    3-D -- the twins chained as drought_clusters chains the device entries, against the same recipe done with scipy"""
    from gan_danet_amd import clusters as C
    from gan_danet_amd import kern as K
    case = {c.name: c for c in U.CASES}[name]
    values = case.x.dtype != np.uint8
    dropped = 0
    for s in (1, 2, 3, U.SPACE8_TIME1):
        for min_step, min_size in ((3, 1), (5, 8)):
            word = C.structure_word(s)
            parent = K.ccl_label_host(case.x, case.threshold if values else 0.0, word & C.PLANAR_BITS, case.mask if values else None)
            planar, _ = K.ccl_relabel_host(K.ccl_filter_host(parent, min_step))
            kept = (planar > 0).astype(np.uint8)
            dropped += int(case.fg.sum() - kept.sum())
            parent = K.ccl_label_host(kept, 0.0, word)
            labels, k = K.ccl_relabel_host(K.ccl_filter_host(parent, min_size))
            want, kw = U.andreadis_oracle(case, s, min_step, min_size)
            assert k == kw and np.array_equal(labels, want), (case, U.structure_id(s), min_step, min_size)
    assert dropped > 0


def test_cpu_and_bad_arguments_are_refused():
    from gan_danet_amd import _lib as L
    from gan_danet_amd import clusters as C
    x = torch.zeros(4, 5, 6, dtype=torch.float64)
    e = torch.zeros(4, 5, 6, dtype=torch.uint8)
    for call in (lambda: C.label_components(x, -0.8), lambda: C.label_components(e), lambda: C.drought_clusters(x),
                 lambda: C.drought_clusters(e), lambda: C.label_components(x.numpy(), -0.8), lambda: C.drought_clusters(x.numpy())):
        with pytest.raises(L.GandanetError):
            call()
    for doc in (C.__doc__, C.drought_clusters.__doc__):
        assert "eriodic longitude" in doc and "minimum-overlap" in doc and "across two grids" in doc
