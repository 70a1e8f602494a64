"""Without a GPU: the queued shadow pass's entry points (bbr_queue_shadow_caster, bbr_shadow_queue_counts) are declared in
include/bibim_hip.h, exported by the library and bound by the package, and the scene shim can carry casters to queue."""
import ctypes as C
import os
import re

import pytest

from conftest import ROOT
from bibim_renderer_amd import Renderer, _capi

NEW_SYMBOLS = ("bbr_queue_shadow_caster", "bbr_shadow_queue_counts")


def header(name):
    txt = open(os.path.join(ROOT, "include", name)).read()
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", txt, flags=re.S))


@pytest.mark.parametrize("symbol", NEW_SYMBOLS)
def test_new_symbols_are_declared_exported_and_bound(symbol):
    assert re.search(r"\b%s\s*\(" % symbol, header("bibim_hip.h")), "not declared in include/bibim_hip.h"
    assert hasattr(C.CDLL(_capi.LIB_PATH), symbol), "declared but not exported"
    assert symbol in _capi.SIGNATURES, "not in the binding table"


def test_the_queue_call_has_the_synchronous_calls_arguments():
    assert _capi.SIGNATURES["bbr_queue_shadow_caster"] == _capi.SIGNATURES["bbr_render_shadow_caster"]
    for m in ("queue_shadow_caster", "shadow_queue_counts"):
        assert callable(getattr(Renderer, m, None)), m


def test_the_scene_shim_has_a_list_of_casters_to_queue():
    assert re.search(r"std::vector<QueuedShadowCaster>\s+QueuedShadowCasters\s*;", header("bibim_scene.h"))
