"""i3d_fusion_render / i3d_fusion_track without a device: the two symbols are declared and exported, their ctypes signatures are set, and a Fusion cannot be made
without a GPU (no CPU fallback)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


NAMES = ("i3d_fusion_render", "i3d_fusion_track")


def _lib():
    from intrinsic3d_amd import binding
    if not os.path.exists(binding.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return binding, binding.load()


def test_symbols_declared_and_exported():
    binding, L = _lib()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "intrinsic3d_hip.h")).read(), flags=re.S)
    assert re.search(r"int\s+i3d_fusion_render\s*\(\s*i3d_fusion\s*\*\s*\w+\s*,\s*const\s+i3d_render_desc\s*\*", hdr)
    assert re.search(r"int\s+i3d_fusion_track\s*\(\s*i3d_fusion\s*\*\s*\w+\s*,\s*const\s+i3d_track_desc\s*\*", hdr)
    for n in NAMES:
        assert n in binding.EXPORTS
        assert hasattr(L, n)


def test_argtypes_set():
    binding, L = _lib()
    r, t = L.i3d_fusion_render, L.i3d_fusion_track
    assert r.restype is ctypes.c_int32 and t.restype is ctypes.c_int32
    assert len(r.argtypes) == 5 and r.argtypes[1] is ctypes.POINTER(binding.RenderDesc) and r.argtypes[4] is ctypes.POINTER(binding.RenderStats)
    assert len(t.argtypes) == 7 and t.argtypes[1] is ctypes.POINTER(binding.TrackDesc) and t.argtypes[6] is ctypes.POINTER(binding.TrackStats)
    assert t.argtypes[2] is ctypes.c_int32 and t.argtypes[3] is ctypes.c_int32
    assert callable(binding.Fusion.render) and callable(binding.Fusion.track)


def test_null_handle_is_an_invalid_argument():
    binding, L = _lib()
    d = binding.RenderDesc(); d.frame = -1
    assert L.i3d_fusion_render(None, d, None, None, None) == 1
    td = binding.track_desc_default(intr=[100.0, 100.0, 50.0, 40.0])
    assert L.i3d_fusion_track(None, td, 4, 4, None, None, None) == 1


def test_no_fusion_without_device():
    import helpers
    binding, _ = _lib()
    if helpers.visible_devices() > 0:
        pytest.skip("a GPU is visible")
    with pytest.raises(binding.I3DError):
        binding.Fusion(0.004, 0.1, 3.0)
