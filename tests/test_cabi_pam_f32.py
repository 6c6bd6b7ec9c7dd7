"""CPU: include/gandanet.h declares every gd_pam_f32_* symbol the ctypes binding knows, with the argument count the
binding passes (text checks on the header, no library call)."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_prototypes():
    src = open(os.path.join(ROOT, "include", "gandanet.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return {m.group(1): m.group(2) for m in re.finditer(r"\b(gd_pam_f32_[a-z0-9_]+)\s*\(([^;]*?)\)\s*;", src, flags=re.S)}


def test_header_declares_every_bound_pam_f32_symbol():
    from gan_danet_amd import _lib
    bound = sorted(n for n in _lib.SIGNATURES if n.startswith("gd_pam_f32_"))
    assert {"gd_pam_f32_fwd", "gd_pam_f32_bwd"} <= set(bound)
    protos = _header_prototypes()
    for name in bound:
        assert name in protos, f"{name} bound in _lib.py but not declared in gandanet.h"
        nargs = len([a for a in protos[name].split(",") if a.strip()])
        assert nargs == len(_lib.SIGNATURES[name][1]), f"{name}: header takes {nargs} arguments, the binding passes {len(_lib.SIGNATURES[name][1])}"


def test_pam_f32_source_is_built():
    from gan_danet_amd import build
    assert "pam_f32.hip" in build.SOURCES
    assert os.path.exists(os.path.join(build.CSRC, "pam_f32.hip"))
