"""CPU: the PAM attention probe's entry points (include/gandanet.h, "PAM attention probe") are declared with the argument
count the ctypes binding passes, and each rejects bad arguments on the host, before any GPU call, with gd_last_error naming
the argument (the pointers are never dereferenced: validation comes first)."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("gd_pam_attn_stats", "gd_pam_attn_received", "gd_pam_attn_rows", "gd_round_to_16")


def _lib():
    from gan_danet_amd import _lib
    return _lib, _lib.load()


def test_header_declares_the_probe_symbols_as_bound():
    L, lib = _lib()
    src = open(os.path.join(ROOT, "include", "gandanet.h")).read()
    assert "PAM attention probe" in src
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    protos = {m.group(1): m.group(2) for m in re.finditer(r"\bint\s+(gd_[a-z0-9_]+)\s*\(([^;]*?)\)\s*;", src, flags=re.S)}
    for name in NAMES:
        assert name in protos and name in L.SIGNATURES and hasattr(lib, name), name
        args = [a.strip() for a in protos[name].split(",") if a.strip()]
        assert len(args) == len(L.SIGNATURES[name][1]), (name, args)
        assert args[-1] == "void* stream", (name, args[-1])
    want = {"gd_pam_attn_stats": ["float logit_scale", "float* lse", "float* entropy", "float* peak"],
            "gd_pam_attn_received": ["const float* lse", "float logit_scale", "float* received"],
            "gd_pam_attn_rows": ["const int* idx", "int S", "float logit_scale", "float* rows", "float* lse_rows"],
            "gd_round_to_16": ["const float* x", "float* y", "long n", "float scale", "int f16"]}
    for name, params in want.items():
        args = [" ".join(a.split()) for a in protos[name].split(",")]
        for p in params:
            assert p in args, (name, p, args)
        if name != "gd_round_to_16":
            assert args[:4] == ["const float* q", "long q_bs", "const float* k", "long k_bs"], (name, args[:4])


def test_probe_source_is_built():
    from gan_danet_amd import build
    assert build.SOURCES[-1] == "pam_probe.hip"
    assert os.path.exists(os.path.join(build.CSRC, "pam_probe.hip"))


def test_probe_argument_errors_before_any_launch():
    L, lib = _lib()
    p = 0x1000                      # a non-null, 16-byte aligned address that is never touched

    def stats(q=p, q_bs=0, k=p, k_bs=0, B=1, N=16, Npad=256, r=3, lse=p):
        return lib.gd_pam_attn_stats(q, q_bs, k, k_bs, B, N, Npad, r, 1.0, lse, None, None, None)

    def received(q=p, q_bs=0, k=p, k_bs=0, B=1, N=16, Npad=256, r=3, lse=p, out=p):
        return lib.gd_pam_attn_received(q, q_bs, k, k_bs, lse, B, N, Npad, r, 1.0, out, None)

    def rows(q=p, q_bs=0, k=p, k_bs=0, B=1, N=16, Npad=256, r=3, idx=p, S=4, out=p):
        return lib.gd_pam_attn_rows(q, q_bs, k, k_bs, idx, S, B, N, Npad, r, 1.0, out, None, None)

    def bad(rc, word):
        assert rc == -1, rc
        assert word in L.last_error(), (word, L.last_error())

    for call in (stats, received, rows):
        bad(call(q=None), "null pointer")
        bad(call(k=None), "null pointer")
        bad(call(r=0), "r (")
        bad(call(r=64), "r (")
        bad(call(Npad=250), "Npad")
        bad(call(N=300, Npad=256), "Npad")
        bad(call(Npad=0), "Npad")
        bad(call(q=p + 4), "unaligned plane")
        bad(call(k=p + 8), "unaligned plane")
        bad(call(q_bs=258), "unaligned plane")
        bad(call(q_bs=-256), "negative batch stride")
        bad(call(k_bs=-4), "negative batch stride")
        bad(call(B=0), "B ")
    bad(stats(lse=None), "null pointer")
    bad(received(lse=None), "null pointer")
    bad(received(out=None), "null pointer")
    bad(rows(idx=None), "null pointer")
    bad(rows(out=None), "null pointer")
    bad(rows(S=0), "S (")
    bad(rows(S=257), "S (")

    bad(lib.gd_round_to_16(None, p, 4, 1.0, 0, None), "null pointer")
    bad(lib.gd_round_to_16(p, None, 4, 1.0, 0, None), "null pointer")
    bad(lib.gd_round_to_16(p, p, 0, 1.0, 0, None), "n <= 0")
    bad(lib.gd_round_to_16(p, p, 4, 1.0, 2, None), "f16")


def test_python_wrapper_checks_the_points():
    """an out-of-range index cannot be seen from the host entry point: attention._point_index refuses it"""
    import pytest
    from gan_danet_amd import attention
    for pts in ([(0, 8)], [(8, 0)], [(-1, 0)], [], [(0, 0)] * 257):
        with pytest.raises(ValueError):
            attention._point_index(pts, 8, 8, "cpu")
    assert attention._point_index([(0, 0), (7, 7), (1, 2)], 8, 8, "cpu").tolist() == [0, 63, 10]
