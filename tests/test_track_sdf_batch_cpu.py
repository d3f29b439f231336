"""-m "not gpu": what i3d_track_frames_sdf / i3d_track_keyframes_sdf / i3d_debug_track_batch_frames show without a device: the header
declares them, the built library exports them, the binding's argument types are the header's, a null handle is an argument error."""
import ctypes as C
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


SYMBOLS = ("i3d_track_frames_sdf", "i3d_track_keyframes_sdf", "i3d_debug_track_batch_frames")


def _lib():
    from intrinsic3d_amd import binding
    if not os.path.exists(binding.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return binding, binding.load()


def _declared(name):
    """the parameter types of the header's declaration of `name`, comments removed, parameter names dropped"""
    text = open(os.path.join(ROOT, "include", "intrinsic3d_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
    assert m, f"{name} is not declared in include/intrinsic3d_hip.h"
    out = []
    for par in m.group(1).split(","):
        words = par.replace("*", " * ").split()
        assert len(words) >= 2, par
        out.append(" ".join(words[:-1]))                  # the last word is the parameter's name
    return out


def test_batch_symbols_are_declared_exported_and_bound_with_the_headers_types():
    binding, L = _lib()
    vp, i32 = C.c_void_p, C.c_int32
    desc = C.POINTER(binding.TrackSdfDesc)
    # pointers to arrays and handles travel as void pointers through the binding; the descriptor is typed
    ctype_of = {"i3d_context *": vp, "const i3d_track_sdf_desc *": desc, "int32_t": i32, "const float *": vp, "double *": vp, "const int32_t *": vp,
                "i3d_track_sdf_stats *": vp}
    want = {"i3d_track_frames_sdf": ["i3d_context *", "const i3d_track_sdf_desc *", "int32_t", "int32_t", "int32_t", "const float *", "double *",
                                     "i3d_track_sdf_stats *"],
            "i3d_track_keyframes_sdf": ["i3d_context *", "const i3d_track_sdf_desc *", "int32_t", "int32_t", "const int32_t *", "double *", "i3d_track_sdf_stats *"],
            "i3d_debug_track_batch_frames": ["i3d_context *", "int32_t"]}
    for s in SYMBOLS:
        assert hasattr(L, s) and s in binding.EXPORTS, s
        decl = _declared(s)
        assert decl == want[s], (s, decl)
        fn = getattr(L, s)
        assert fn.restype is i32 and list(fn.argtypes) == [ctype_of[t] for t in decl], (s, fn.argtypes)
    for m in ("track_frames_sdf", "track_keyframes_sdf", "debug_track_batch_frames"):
        assert callable(getattr(binding.Context, m))


def test_batch_null_handle_is_an_argument_error():
    binding, L = _lib()
    d = binding.track_sdf_desc_default()
    dep = np.zeros((2, 2, 2), np.float32); poses = np.full((2, 6), 7.0); p = binding._p
    st = (binding.TrackSdfStats * 2)()
    assert L.i3d_track_frames_sdf(None, d, 2, 2, 2, p(dep), p(poses), C.cast(st, C.c_void_p)) == 1
    assert L.i3d_track_keyframes_sdf(None, d, 0, 2, None, p(poses), C.cast(st, C.c_void_p)) == 1
    assert L.i3d_debug_track_batch_frames(None, 2) == 1
    assert np.all(poses == 7.0) and all(s.status == 0 and s.valid == 0 for s in st)
