"""CPU: the "ordered" deterministic reduction mode at the ABI level -- header against binding, the mode switch, and the
host-only plan queries (no GPU call anywhere in this file)."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["gd_set_det_reduce", "gd_get_det_reduce", "gd_conv3x3_wgrad_ws", "gd_gemm_nt_ws", "gd_disc_stem_wgrad_ws",
       "gd_nhwc_to_nchw16_ws", "gd_conv3x3_wgrad_plan", "gd_gemm_nt_plan"]
MIB = 1 << 20


def _header_prototypes():
    src = open(os.path.join(ROOT, "include", "gandanet.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return {m.group(1): m.group(2) for m in re.finditer(r"\b(gd_[a-z0-9_]+)\s*\(([^;{}]*?)\)\s*;", src, flags=re.S)}


def _nargs(proto):
    args = [a.strip() for a in proto.split(",") if a.strip()]
    return 0 if args == ["void"] else len(args)


def test_header_declares_every_new_symbol_with_the_bound_argument_count():
    from gan_danet_amd import _lib
    protos = _header_prototypes()
    for name in NEW:
        assert name in _lib.SIGNATURES, f"{name} is not bound in _lib.py"
        assert name in protos, f"{name} bound in _lib.py but not declared in gandanet.h"
        assert _nargs(protos[name]) == len(_lib.SIGNATURES[name][1]), name
    # a _ws entry point = the old argument list + (ws, ws_bytes)
    for name in ("gd_conv3x3_wgrad", "gd_gemm_nt", "gd_disc_stem_wgrad", "gd_nhwc_to_nchw16"):
        old, new = _lib.SIGNATURES[name][1], _lib.SIGNATURES[name + "_ws"][1]
        assert new[:len(old)] == old and new[len(old):] == [_lib.c_fp, C.c_size_t], name


def test_det_reduce_source_is_built():
    from gan_danet_amd import build
    assert "det_reduce.hip" in build.SOURCES
    assert os.path.exists(os.path.join(build.CSRC, "det_reduce.hip"))


@pytest.fixture
def modes():
    """hands out the library and the kern module; puts both flags back afterwards"""
    import gan_danet_amd as gd
    from gan_danet_amd import _lib, kern
    lib = _lib.load()
    yield gd, kern, lib
    kern.set_deterministic(False, reduce="unsplit")
    assert lib.gd_get_deterministic() == 0 and lib.gd_get_det_reduce() == 0


def test_mode_switch_round_trip(modes):
    gd, kern, lib = modes
    from gan_danet_amd._lib import GandanetError
    assert kern.DET_REDUCE == "unsplit" and lib.gd_get_det_reduce() == 0      # the initial setting
    assert lib.gd_set_det_reduce(1) == 0 and lib.gd_get_det_reduce() == 1
    assert lib.gd_set_det_reduce(0) == 0 and lib.gd_get_det_reduce() == 0
    assert lib.gd_set_det_reduce(7) != 0 and lib.gd_get_det_reduce() == 0     # refused, unchanged
    gd.set_deterministic(True)
    assert kern.DETERMINISTIC and kern.DET_REDUCE == "unsplit"
    assert lib.gd_get_deterministic() == 1 and lib.gd_get_det_reduce() == 0
    gd.set_deterministic(True, reduce="ordered")
    assert kern.DETERMINISTIC and kern.DET_REDUCE == "ordered"
    assert lib.gd_get_deterministic() == 1 and lib.gd_get_det_reduce() == 1
    gd.set_deterministic(False)                                               # None keeps the reduce setting
    assert not kern.DETERMINISTIC and kern.DET_REDUCE == "ordered" and lib.gd_get_det_reduce() == 1
    with pytest.raises(GandanetError):
        gd.set_deterministic(True, reduce="nonsense")
    assert kern.DET_REDUCE == "ordered" and not kern.DETERMINISTIC            # a refused call changes nothing
    assert kern.det_ws() == (None, 0)                                         # no workspace outside ordered mode


WGRAD_SHAPES = [(32, 24, 136, 256, 256, 1), (32, 184, 368, 256, 256, 1)]     # the dense layer and the fuse conv


@pytest.mark.parametrize("shape", WGRAD_SHAPES, ids=["136to24", "368to184"])
def test_conv3x3_wgrad_plan(modes, shape):
    gd, kern, lib = modes
    B, Cout, Cin, H, W, stride = shape
    out_bytes = Cout * Cin * 9 * 4
    gd.set_deterministic(False)
    s_default, need = kern.conv3x3_wgrad_plan(B, Cout, Cin, H, W, stride, ws_bytes=256 * MIB)
    assert s_default > 1 and need == 0                       # the atomic path does not touch the workspace
    gd.set_deterministic(True, reduce="unsplit")
    assert kern.conv3x3_wgrad_plan(B, Cout, Cin, H, W, stride, ws_bytes=256 * MIB) == (1, 0)
    gd.set_deterministic(True, reduce="ordered")
    s, need = kern.conv3x3_wgrad_plan(B, Cout, Cin, H, W, stride, ws_bytes=256 * MIB)
    assert s > 1 and need == s * out_bytes and need <= 256 * MIB
    if s_default * out_bytes <= 256 * MIB:
        assert s == s_default
    else:
        assert s < s_default and s <= 256 * MIB // out_bytes
    s_free, need_free = kern.conv3x3_wgrad_plan(B, Cout, Cin, H, W, stride, ws_bytes=(1 << 64) - 1)
    assert s_free == s_default and need_free == s_default * out_bytes
    # fewer than two slabs: unsplit
    assert kern.conv3x3_wgrad_plan(B, Cout, Cin, H, W, stride, ws_bytes=2 * out_bytes - 1) == (1, 0)
    assert kern.conv3x3_wgrad_plan(B, Cout, Cin, H, W, stride, ws_bytes=0) == (1, 0)
    assert kern.conv3x3_wgrad_plan(B, Cout, Cin, H, W, stride, ws_bytes=2 * out_bytes) == (2, 2 * out_bytes)
    # the same question twice gives the same answer
    assert kern.conv3x3_wgrad_plan(B, Cout, Cin, H, W, stride, ws_bytes=256 * MIB) == (s, need)


def test_gemm_nt_plan_gram(modes):
    gd, kern, lib = modes
    g = dict(B=32, M=184, N=184, kseg=1, klen=65536)        # CAM's Gram matrix, C = 184 at 256 x 256, batch 32
    out_bytes = 32 * 184 * 184 * 4
    gd.set_deterministic(False)
    s_default, need = kern.gemm_nt_plan(**g, ws_bytes=256 * MIB)
    assert s_default > 1 and need == 0
    gd.set_deterministic(True, reduce="unsplit")
    assert kern.gemm_nt_plan(**g, ws_bytes=256 * MIB) == (1, 0)
    gd.set_deterministic(True, reduce="ordered")
    s, need = kern.gemm_nt_plan(**g, ws_bytes=256 * MIB)
    assert s > 1 and need == s * out_bytes and need <= 256 * MIB
    assert s == s_default or s_default * out_bytes > 256 * MIB
    assert kern.gemm_nt_plan(**g, ws_bytes=2 * out_bytes - 1) == (1, 0)
    assert kern.gemm_nt_plan(**g, ws_bytes=2 * out_bytes)[0] == 2
    assert kern.gemm_nt_plan(**g, splits=1, ws_bytes=256 * MIB) == (1, 0)     # an explicit unsplit request stays unsplit
    # a bad descriptor is an error, not a plan
    from gan_danet_amd._lib import GandanetError
    with pytest.raises(GandanetError):
        kern.gemm_nt_plan(B=0, M=1, N=1, kseg=1, klen=1)


def test_disc1_trunk_eligibility_follows_the_reduce_mode(modes):
    import torch
    gd, kern, lib = modes
    from gan_danet_amd import ops
    x = torch.zeros(1, 1, 8, 8)
    ws = [torch.zeros(64, 1, 3, 3), torch.zeros(128, 64, 3, 3)]
    with gd.precision("bf16"):
        gd.set_deterministic(False)
        assert ops.disc1_trunk_eligible(x, ws)
        gd.set_deterministic(True, reduce="unsplit")
        assert not ops.disc1_trunk_eligible(x, ws)
        gd.set_deterministic(True, reduce="ordered")
        assert ops.disc1_trunk_eligible(x, ws)
