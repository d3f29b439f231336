"""ctypes binding of libintrinsic3d_hip.so (include/intrinsic3d_hip.h).

Python is only the test / bench harness here: the host side of the product (Optimizer::optimize mirror, LM/PCG
control, lighting solve) is C++ inside the library.  Loading fails loudly when the HIP library is missing — there is
no CPU fallback anywhere on the product path.

The ABI itself (struct mirrors, one prototype per function) is data in abi.py; this file is the marshalling: numpy arrays and keyword arguments in, the
library's structs and pointers across, numpy arrays and dicts out.  Every name of abi.py a caller needs is re-exported here.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from .abi import (EXPORTS, PROTOTYPES, REFINE_CALLBACK, Stats, GridView, OptimizerConfig, IterationStats, ShStats, RefineConfig, RenderDesc, RenderStats,  # noqa: F401
                  TrackDesc, TrackStats, TrackRgbdDesc, TrackRgbdStats, MergeStats, QueryDesc, QueryStats, RegisterDesc, RegisterStats, RegisterVolumeDesc,
                  RegisterVolumeStats, FusionMeshDesc, FusionMeshStats, TrackSdfDesc, TrackSdfStats, TrackSdfRgbdDesc, TrackSdfRgbdStats, LmScriptDesc)

_HERE = os.path.dirname(os.path.abspath(__file__))
# I3D_LIB: load another build of the SAME C ABI instead (same-box A/B of kernel variants in one GPU session; never a CPU substitute)
LIB_PATH = os.environ.get("I3D_LIB") or os.path.join(_HERE, "libintrinsic3d_hip.so")

K_NAMES = ["classify", "observe", "build", "eg_pass", "gather", "cost", "vector", "sh", "eg_aux", "comm", "eg_mr2", "eg_mr3"]
RENDER_PLANES = ("depth", "normal", "albedo", "shading", "intensity", "residual")
QUERY_OUTPUTS = ("sdf", "normal", "albedo", "foot", "distance", "status")
CAST_OUTPUTS = ("t", "position", "normal", "albedo", "shading", "intensity", "status")
COLOR_CAST_OUTPUTS = ("t", "color", "status")
LM_SCRIPT_GUARD = 64
LM_RECORD_DTYPE = np.dtype([("seq", np.int32), ("final_", np.int32), ("accepted", np.int32), ("pcg_it", np.int32), ("termination", np.int32), ("kind", np.int32),
                            ("cost", np.float64), ("cand_cost", np.float64), ("model_change", np.float64), ("rel", np.float64), ("radius_after", np.float64),
                            ("ngrad", np.float64), ("nfree", np.float64)])

_lib = None


def load():
    """Load the HIP library; raises if it has not been built (no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(f"{LIB_PATH} is missing: build it with `make -C intrinsic3d_amd/csrc` "
                           "(or __graft_entry__.build()); the product path has no CPU fallback")
    L = C.CDLL(LIB_PATH)
    for name, restype, argtypes in PROTOTYPES:
        fn = getattr(L, name)
        fn.restype, fn.argtypes = restype, argtypes
    _lib = L
    return L


class I3DError(RuntimeError):
    pass


def _io_check(rc, what):
    if rc != 0:
        raise I3DError(f"{what} failed ({rc})")


def _io(name, *args):
    """an entry point without a handle to ask for the error text (the host-only ones, the constructors): the status alone"""
    _io_check(getattr(load(), name)(*args), name)


class _Handle:
    """What Context and Fusion share: the handle, its release, and the status check, which differ only in the names of *_destroy and *_last_error."""
    _destroy = _last_error = None

    def _check(self, rc, what):
        if rc != 0:
            raise I3DError(f"{what} failed ({rc}): {getattr(self.L, self._last_error)(self.h).decode()}")

    def _call(self, name, *args):
        """the entry point `name` on this handle, its status checked"""
        self._check(getattr(self.L, name)(self.h, *args), name)

    def close(self):
        if self.h:
            getattr(self.L, self._destroy)(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


# ---- one marshalling path per argument shape ------------------------------------------------------------------------------------------------
def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _pose(p, *shape):
    """a pose6 (default), a batch (-1, 6) or a pivot (3) as a contiguous float64 copy of the caller's: the library writes its result into the copy"""
    return np.ascontiguousarray(np.asarray(p, np.float64).reshape(shape or 6)).copy()


def _images(depth, *lum, bad=None, batch=False, none_ok=False):
    """A frame as the library takes it: depth [h, w] and the luminance planes given with it, contiguous float32 -> ((w, h), [arrays]); batch: [B, h, w] ->
    ((B, w, h), [arrays]).  bad: the ValueError text for a luminance of another shape (and for a batch that is not 3-d); None: the shapes are not compared and
    the library reads every plane at the depth's size.  none_ok: a luminance of None stays None for the library to report."""
    img = [np.ascontiguousarray(depth, np.float32)] + [None if x is None and none_ok else np.ascontiguousarray(x, np.float32) for x in lum]
    if batch:
        if img[0].ndim != 3:
            raise ValueError(bad)
        n, h, w = img[0].shape
    else:
        n = None
        h, w = img[0].shape
    if bad and any(x is not None and x.shape != img[0].shape for x in img[1:]):
        raise ValueError(bad)
    return (int(w), int(h)) if n is None else (int(n), int(w), int(h)), img


def _debug_sums(n, counters, fill, call):
    """The return of a debug_*_sums entry: call(sums, *counters) fills n doubles and `counters` int64 counts -> (sums, count, ...).  fill: what the outputs hold
    before the call, 0 in the ray-cast and register-volume probes and -1 in the probes on the field, whose tests tell "not written" from a count of 0 by it."""
    sums = np.full(n, float(fill)); c = [C.c_int64(fill) for _ in range(counters)]
    call(_p(sums), *[C.byref(x) for x in c])
    return (sums, *[int(x.value) for x in c])


def _render_desc(camera, depth_range, frame=-1, level=0, refined=False):
    """i3d_render_desc: the view of a keyframe (camera None) or the free camera = dict(width, height, intr, dist, pose); depth_range = (min, max) or None"""
    d = RenderDesc(); d.frame = int(frame); d.level = int(level); d.use_refined_sdf = int(bool(refined))
    if camera is not None:
        d.width, d.height = int(camera["width"]), int(camera["height"])
        d.intrinsics4[:] = [float(x) for x in camera["intr"]]
        d.distortion5[:] = [float(x) for x in camera.get("dist", np.zeros(5))]
        d.pose6[:] = [float(x) for x in camera["pose"]]
    if depth_range is not None:
        d.min_depth, d.max_depth = float(depth_range[0]), float(depth_range[1])
    return d


def _planes(planes, w, h):
    """the output images of a ray cast: {plane: zeros (h, w), normal (h, w, 3)}; none for an empty view"""
    return {k: np.zeros((h, w, 3) if k == "normal" else (h, w), np.float32) for k in planes if w > 0 and h > 0}


def _color_out(out, as_uint8):
    """the colour of a colour call as it is handed back: float32 in units of the stored byte, or (as_uint8) rounded to nearest and clipped to uint8 on the host"""
    if as_uint8 and "color" in out:
        out["color"] = np.clip(np.rint(out["color"]), 0, 255).astype(np.uint8)
    return out


def _render_color(obj, name, d, w, h, planes, as_uint8):
    """the shared body of Context.render_view_color / Fusion.render_color: d the descriptor, planes out of ("color", "depth")"""
    unknown = set(planes) - {"color", "depth"}
    if unknown:
        raise ValueError(f"{name}: unknown planes {sorted(unknown)}")
    out = {k: np.zeros((h, w, 3) if k == "color" else (h, w), np.float32) for k in planes if w > 0 and h > 0}
    st = RenderStats()
    obj._call(name, C.byref(d), _p(out.get("color")), _p(out.get("depth")), C.byref(st))
    out["stats"] = st.as_dict()
    return _color_out(out, as_uint8)


def _pyramid_sizes(w, h, levels):
    """(width, height) of every pyramid level: cv::pyrDown halves with truncation (levels.cpp)"""
    out = [(int(w), int(h))]
    for _ in range(1, int(levels)):
        out.append((out[-1][0] // 2, out[-1][1] // 2))
    return out


# ---- descriptors: the C default, then the caller's fields -------------------------------------------------------------------------------------
_REFINED = {"refined": "use_refined_sdf"}
_CAMERA = {**_REFINED, "intr": "intrinsics4", "dist": "distortion5"}
_RGBD_OWN = ("geometric_weight", "photo_weight", "max_photo_residual")
# builder (i3d_<builder> is the C default function): struct; aliases {keyword: field}; arrays {field: element type}, `pad` among them filled up with zeros;
# own_camera: the fields that switch use_context_camera off when given (i3d_track_desc alone: i3d_track_sdf_desc defaults to its own camera and an explicit
# use_context_camera = 1 there survives an intr / dist); base: the builder of the nested `base` (the *_rgbd descriptors)
_DESC = {
    "query_desc_default": dict(struct=QueryDesc, aliases=_REFINED),
    "register_desc_default": dict(struct=RegisterDesc, aliases=_REFINED),
    "register_volume_desc_default": dict(struct=RegisterVolumeDesc),
    "fusion_mesh_desc_default": dict(struct=FusionMeshDesc),
    "track_desc_default": dict(struct=TrackDesc, aliases=_CAMERA, arrays={"iterations": int, "intrinsics4": float, "distortion5": float}, pad=("iterations",),
                               own_camera=("intrinsics4", "distortion5")),
    "track_sdf_desc_default": dict(struct=TrackSdfDesc, aliases=_CAMERA, arrays={"intrinsics4": float, "distortion5": float}),
    "track_rgbd_desc_default": dict(struct=TrackRgbdDesc, base="track_desc_default"),
    "track_sdf_rgbd_desc_default": dict(struct=TrackSdfRgbdDesc, base="track_sdf_desc_default"),
}


def _desc_default(name, kw):
    """the one body of the *_desc_default functions, driven by _DESC[name]"""
    t = _DESC[name]
    d = t["struct"]()
    getattr(load(), "i3d_" + name)(C.byref(d))
    if "base" in t:                                 # the three own fields as floats; `base` is rebuilt only when one of its fields is given
        for k in _RGBD_OWN:
            if k in kw:
                setattr(d, k, float(kw[k]))
        base = {k: v for k, v in kw.items() if k not in _RGBD_OWN}
        if base:
            d.base = _desc_default(t["base"], base)
        return d
    fields, arrays = dict(t["struct"]._fields_), t.get("arrays", {})
    for k, v in kw.items():
        f = t.get("aliases", {}).get(k, k)
        if f not in fields:
            raise ValueError(f"{name}: unknown field {k}")
        if f in arrays:
            v = [arrays[f](x) for x in v]
            if f in t.get("pad", ()):
                n = fields[f]._length_
                v = (v + [0] * (n - len(v)))[:n]
            getattr(d, f)[:] = v
            if f in t.get("own_camera", ()):
                d.use_context_camera = 0
        else:
            setattr(d, f, int(bool(v)) if k == "refined" else v)
    return d


def query_desc_default(**kw) -> QueryDesc:
    """i3d_query_desc_default, then the given fields (refined: use_refined_sdf)."""
    return _desc_default("query_desc_default", kw)


def register_desc_default(**kw) -> RegisterDesc:
    """i3d_register_desc_default, then the given fields (refined: use_refined_sdf)."""
    return _desc_default("register_desc_default", kw)


def register_volume_desc_default(**kw) -> RegisterVolumeDesc:
    """i3d_register_volume_desc_default, then the given fields."""
    return _desc_default("register_volume_desc_default", kw)


def fusion_mesh_desc_default(**kw) -> FusionMeshDesc:
    """i3d_fusion_mesh_desc_default, then the given fields."""
    return _desc_default("fusion_mesh_desc_default", kw)


def track_desc_default(**kw) -> TrackDesc:
    """i3d_track_desc_default, then the given fields.  iterations: a list (padded with zeros); intr / dist: the level-0 camera (sets use_context_camera = 0);
    refined: use_refined_sdf."""
    return _desc_default("track_desc_default", kw)


def track_rgbd_desc_default(**kw) -> TrackRgbdDesc:
    """i3d_track_rgbd_desc_default, then the given fields: geometric_weight, photo_weight, max_photo_residual; every other one goes to the base
    descriptor as in track_desc_default."""
    return _desc_default("track_rgbd_desc_default", kw)


def track_sdf_desc_default(**kw) -> TrackSdfDesc:
    """i3d_track_sdf_desc_default, then the given fields.  intr / dist: the level-0 camera (the default use_context_camera = 0 reads them); refined:
    use_refined_sdf."""
    return _desc_default("track_sdf_desc_default", kw)


def track_sdf_rgbd_desc_default(**kw) -> TrackSdfRgbdDesc:
    """i3d_track_sdf_rgbd_desc_default, then the given fields: geometric_weight, photo_weight, max_photo_residual; every other one goes to the base descriptor
    as in track_sdf_desc_default."""
    return _desc_default("track_sdf_rgbd_desc_default", kw)


def default_config(**kw) -> OptimizerConfig:
    cfg = OptimizerConfig()
    load().i3d_optimizer_config_default(C.byref(cfg))
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


# ---- bodies Context and Fusion share: obj is either, name the entry point of its kind ----------------------------------------------------------
def _query(obj, name, points, outputs, has_albedo, desc):
    """the shared body of Context.query_points / Fusion.query_points"""
    d = query_desc_default(**desc)
    pts = np.ascontiguousarray(points, np.float64).reshape(-1, 3)
    n = pts.shape[0]
    names = tuple(k for k in QUERY_OUTPUTS if has_albedo or k != "albedo")
    if outputs is None:
        outputs = tuple(k for k in names if d.project or k not in ("foot", "distance"))
    unknown = set(outputs) - set(names)
    if unknown:
        raise ValueError(f"{name}: unknown outputs {sorted(unknown)}")
    shape = {"sdf": ((n,), np.float64), "normal": ((n, 3), np.float32), "albedo": ((n,), np.float32), "foot": ((n, 3), np.float64),
             "distance": ((n,), np.float64), "status": ((n,), np.uint8)}
    out = {k: np.zeros(*shape[k]) for k in outputs}
    st = QueryStats()
    obj._call(name, C.byref(d), n, _p(pts), *[_p(out.get(k)) for k in names], C.byref(st))
    out["stats"] = st.as_dict()
    return out


def _cast_rays(obj, name, head, origins, directions, t_min, t_max, outputs, names, order):
    """the shared body of Context.cast_rays / Fusion.cast_rays; head: the arguments before `order`, names: the outputs the entry point has, in its order"""
    o = np.ascontiguousarray(origins, np.float64).reshape(-1, 3)
    d = np.ascontiguousarray(directions, np.float64).reshape(-1, 3)
    n = o.shape[0]
    if d.shape[0] != n:
        raise ValueError(f"{name}: {n} origins and {d.shape[0]} directions")
    rng = [None if x is None else np.ascontiguousarray(x, np.float64).reshape(-1) for x in (t_min, t_max)]
    if any(x is not None and x.shape[0] != n for x in rng):
        raise ValueError(f"{name}: t_min / t_max must hold one value per ray")
    if outputs is None:
        outputs = tuple(k for k in names if k not in ("shading", "intensity"))
    unknown = set(outputs) - set(names)
    if unknown:
        raise ValueError(f"{name}: unknown outputs {sorted(unknown)}")
    shape = {"t": ((n,), np.float64), "position": ((n, 3), np.float64), "normal": ((n, 3), np.float32), "albedo": ((n,), np.float32),
             "shading": ((n,), np.float32), "intensity": ((n,), np.float32), "status": ((n,), np.uint8), "color": ((n, 3), np.float32)}
    out = {k: np.zeros(*shape[k]) for k in outputs}
    st = RenderStats()
    obj._call(name, *head, int(order), n, _p(o), _p(d), _p(rng[0]), _p(rng[1]), *[_p(out.get(k)) for k in names], C.byref(st))
    out["stats"] = st.as_dict()
    return out


def _register(obj, name, points, pose, desc):
    """the shared body of Context.register_points / Fusion.register_points"""
    d = register_desc_default(**desc)
    pts = np.ascontiguousarray(points, np.float64).reshape(-1, 3)
    p6 = _pose(pose); st = RegisterStats()
    obj._call(name, C.byref(d), pts.shape[0], _p(pts), _p(p6), C.byref(st))
    return p6, st.as_dict()


def _track(obj, name, d, stats_t, images, pose6):
    """the shared body of the single-frame trackers of Context and Fusion: images = _images(..) -> (pose6, stats dict)"""
    (w, h), img = images
    pose = _pose(pose6); st = stats_t()
    obj._call(name, C.byref(d), w, h, *map(_p, img), _p(pose), C.byref(st))
    return pose, st.as_dict()


class Context(_Handle):
    """One device context (i3d_context)."""
    _destroy, _last_error = "i3d_destroy", "i3d_last_error"

    def __init__(self, device: int = 0):
        self.L = load()
        h = C.c_void_p()
        rc = self.L.i3d_create(int(device), C.byref(h))
        if rc != 0:
            raise I3DError(f"i3d_create failed ({rc}): {self.L.i3d_last_error(None).decode()}")
        self.h = h
        self.N = 0
        self.K = 0
        self._keep = []

    # ---- uploads -------------------------------------------------------------------------------------------
    def set_grid(self, voxel_size, keys, sdf, sdf_refined, albedo, weight, color, truncation=None):
        keys = np.ascontiguousarray(keys, np.int32); sdf = np.ascontiguousarray(sdf, np.float64)
        sr = np.ascontiguousarray(sdf_refined, np.float64); al = np.ascontiguousarray(albedo, np.float64)
        w = np.ascontiguousarray(weight, np.float32); col = np.ascontiguousarray(color, np.uint8)
        gv = GridView(keys.shape[0], float(voxel_size), float(np.float32(voxel_size) * np.float32(5.0)) if truncation is None else float(truncation),
                      _p(keys), _p(sdf), _p(sr), _p(al), _p(w), _p(col))
        self._call("i3d_set_grid", C.byref(gv))
        self.N = keys.shape[0]

    def set_frames(self, frames, levels):
        K = len(frames); self.K = K
        ws = np.array([frames[0]["lum"][l].shape[1] for l in range(levels)], np.int32)
        hs = np.array([frames[0]["lum"][l].shape[0] for l in range(levels)], np.int32)
        self._sizes = [(int(w), int(h)) for w, h in zip(ws, hs)]
        arr_t = C.c_void_p * (K * levels)
        lum = arr_t(); dep = arr_t(); bgr = arr_t(); keep = []
        for f in range(K):
            for l in range(levels):
                a = np.ascontiguousarray(frames[f]["lum"][l], np.float32); b = np.ascontiguousarray(frames[f]["depth"][l], np.float32)
                c = frames[f].get("bgr")
                c = np.ascontiguousarray(c[l], np.uint8) if c is not None else None
                keep += [a, b, c]
                lum[f * levels + l] = a.ctypes.data; dep[f * levels + l] = b.ctypes.data
                bgr[f * levels + l] = c.ctypes.data if c is not None else None
        self._call("i3d_set_frames", K, levels, _p(ws), _p(hs), C.cast(lum, C.c_void_p), C.cast(dep, C.c_void_p), C.cast(bgr, C.c_void_p))

    def set_frames_rgbd(self, bgr_list, depth_list, levels):
        """level-0 colour (uint8 HxWx3, BGR) + depth (float32 HxW) per keyframe; the pyramids are built on the device"""
        K = len(bgr_list); h, w = depth_list[0].shape
        self._keep = [np.ascontiguousarray(b, np.uint8) for b in bgr_list] + [np.ascontiguousarray(d, np.float32) for d in depth_list]
        pb = (C.c_void_p * K)(*[a.ctypes.data for a in self._keep[:K]]); pd = (C.c_void_p * K)(*[a.ctypes.data for a in self._keep[K:]])
        self._call("i3d_set_frames_rgbd", K, int(levels), int(w), int(h), pb, pd)
        self._sizes = _pyramid_sizes(w, h, levels)
        self.K = K

    def get_frame_image(self, frame, level, w, h):
        lum = np.zeros((h, w), np.float32); dep = np.zeros((h, w), np.float32)
        self._call("i3d_get_frame_image", int(frame), int(level), _p(lum), _p(dep))
        return lum, dep

    def set_camera(self, intr, dist, poses):
        a = np.ascontiguousarray(intr, np.float64); b = np.ascontiguousarray(dist, np.float64); c = np.ascontiguousarray(poses, np.float64)
        self._call("i3d_set_camera", _p(a), _p(b), _p(c))

    def get_camera(self):
        a = np.zeros(4); b = np.zeros(5); c = np.zeros((self.K, 6))
        self._call("i3d_get_camera", _p(a), _p(b), _p(c))
        return a, b, c

    def set_voxel_sh(self, sh):
        s = np.ascontiguousarray(sh, np.float64)
        self._call("i3d_set_voxel_sh", _p(s))

    def get_voxel_sh(self):
        s = np.zeros((self.N, 9))
        self._call("i3d_get_voxel_sh", _p(s))
        return s

    def get_grid(self):
        a = np.zeros(self.N); b = np.zeros(self.N)
        self._call("i3d_get_grid", _p(a), _p(b))
        return a, b

    def update_grid(self, sdf_refined=None, albedo=None, color=None):
        a = None if sdf_refined is None else np.ascontiguousarray(sdf_refined, np.float64)
        b = None if albedo is None else np.ascontiguousarray(albedo, np.float64)
        c = None if color is None else np.ascontiguousarray(color, np.uint8)
        self._call("i3d_update_grid", _p(a), _p(b), _p(c))

    # ---- level transitions / refine schedule ------------------------------------------------------------
    def set_grid_from_tsdf_records(self, voxel_size, keys, sdf, weight, color):
        keys = np.ascontiguousarray(keys, np.int32); sdf = np.ascontiguousarray(sdf, np.float32)
        weight = np.ascontiguousarray(weight, np.float32); color = np.ascontiguousarray(color, np.uint8)
        self._call("i3d_set_grid_from_tsdf_records", float(voxel_size), len(sdf), _p(keys), _p(sdf), _p(weight), _p(color))
        self.grid_info()

    def grid_info(self):
        n = C.c_int64(0); vs = C.c_float(0); tr = C.c_float(0)
        self._call("i3d_grid_info", C.byref(n), C.byref(vs), C.byref(tr))
        self.N = int(n.value)
        return self.N, float(vs.value), float(tr.value)

    def export_grid(self):
        N = self.grid_info()[0]
        out = dict(keys=np.zeros((N, 3), np.int32), sdf=np.zeros(N), sdf_refined=np.zeros(N), albedo=np.zeros(N),
                   weight=np.zeros(N, np.float32), color=np.zeros((N, 3), np.uint8))
        self._call("i3d_export_grid", *[_p(out[k]) for k in ("keys", "sdf", "sdf_refined", "albedo", "weight", "color")])
        return out

    def recompute_colors(self, occlusion_distance, num_observations):
        self._call("i3d_recompute_colors", float(occlusion_distance), int(num_observations))

    def clear_outside_thin_shell(self, thres_shell):
        n = C.c_int64(0)
        self._call("i3d_clear_outside_thin_shell", float(thres_shell), C.byref(n))
        self.N = int(n.value)
        return self.N

    def upsample(self):
        n = C.c_int64(0)
        self._call("i3d_upsample", C.byref(n))
        self.N = int(n.value)
        return self.N

    def refine(self, rcfg: "RefineConfig", ocfg: OptimizerConfig, callback=None):
        """Intrinsic3D::refine; callback(grid_level, num_grid_levels, pyramid_level, num_pyramid_levels) may call export_grid()."""
        cb = REFINE_CALLBACK((lambda user, a, b, c_, d: callback(a, b, c_, d)) if callback else (lambda *a: None))
        self._call("i3d_refine", C.byref(rcfg), C.byref(ocfg), cb, None)
        self.grid_info()

    # ---- mesh export ------------------------------------------------------------------------------------------
    def extract_mesh(self, use_refined_sdf=True, color_mode=0, largest_component_only=False):
        nv, nf = C.c_int64(0), C.c_int64(0)
        self._call("i3d_extract_mesh", int(bool(use_refined_sdf)), int(color_mode), int(bool(largest_component_only)), C.byref(nv), C.byref(nf))
        v = np.zeros((nv.value, 3), np.float32); c = np.zeros((nv.value, 3), np.uint8); f = np.zeros((nf.value, 3), np.int32)
        self._call("i3d_get_mesh", _p(v), _p(c), _p(f))
        return v, c, f

    def export_mesh_ply(self, path, use_refined_sdf=True, color_mode=0, largest_component_only=False):
        self._call("i3d_export_mesh_ply", str(path).encode(), int(bool(use_refined_sdf)), int(color_mode), int(bool(largest_component_only)))

    # ---- image-space view ----------------------------------------------------------------------------------
    def render_view(self, frame=0, level=0, refined=True, planes=RENDER_PLANES, camera=None, depth_range=None):
        """Ray-casts the resident grid into keyframe `frame` at pyramid `level`, or (frame=-1) into camera = dict(width, height, intr, dist, pose) with pose
        world->camera (angle-axis | t).  depth_range = (min, max) camera z, <= 0 open.  Returns {plane: array} for the requested planes ((h, w), normal (h, w, 3))
        plus "stats": {hits, samples, residual_sq_sum}."""
        if frame < 0 and camera is None:
            raise ValueError("render_view: frame < 0 needs a camera")
        d = _render_desc(camera if frame < 0 else None, depth_range, frame, level, refined)
        w, h = (d.width, d.height) if frame < 0 else self._level_size(level)
        unknown = set(planes) - set(RENDER_PLANES)
        if unknown:
            raise ValueError(f"render_view: unknown planes {sorted(unknown)}")
        out = _planes(planes, w, h)
        st = RenderStats()
        self._call("i3d_render_view", C.byref(d), *[_p(out.get(k)) for k in RENDER_PLANES], C.byref(st))
        if frame >= 0 and (w, h) == (0, 0) and planes:
            raise I3DError("render_view: the keyframe image size is unknown (keyframes not set through this Context)")
        out["stats"] = st.as_dict()
        return out

    def track_frame(self, depth, pose6, **desc):
        """Registers a depth frame ([h, w] metres, colour geometry, 0 = invalid) against the resident model from the initial guess pose6 (world->camera,
        angle-axis | t).  desc: fields of i3d_track_desc (see track_desc_default).  Returns (pose6, stats dict)."""
        return _track(self, "i3d_track_frame", track_desc_default(**desc), TrackStats, _images(depth), pose6)

    def debug_track_sums(self, depth, level, pose_ref6, pose_cur6, **desc):
        """The 29 sums and the inlier count of one association pass at `level` (i3d_debug_track_sums)."""
        d = track_desc_default(**desc)
        (w, h), (dep,) = _images(depth)
        pr = _pose(pose_ref6); pc = _pose(pose_cur6)
        return _debug_sums(29, 1, 0, lambda *out: self._call("i3d_debug_track_sums", C.byref(d), w, h, _p(dep), int(level), _p(pr), _p(pc), *out))

    def track_frame_rgbd(self, depth, lum, pose6, **desc):
        """track_frame with the photometric term (i3d_track_frame_rgbd): lum is the frame's luminance ([h, w] float, the keyframes' convention).  desc: fields of
        i3d_track_rgbd_desc (see track_rgbd_desc_default).  Returns (pose6, stats dict: those of track_frame plus photo_samples, photo_rms_initial / _final)."""
        # lum=None goes through to the library, which reports it (I3DError); every other luminance taker converts it first, and None fails the shape check there
        return _track(self, "i3d_track_frame_rgbd", track_rgbd_desc_default(**desc), TrackRgbdStats,
                      _images(depth, lum, bad="track_frame_rgbd: depth and luminance differ in shape", none_ok=True), pose6)

    def debug_track_rgbd_sums(self, depth, lum, level, pose_ref6, pose_cur6, **desc):
        """The 31 sums (27 weighted entries, geometric r^2 and count, photometric r^2 and count), the inlier count and the photometric sample count of one
        association pass at `level` (i3d_debug_track_rgbd_sums)."""
        d = track_rgbd_desc_default(**desc)
        (w, h), (dep, lu) = _images(depth, lum, bad="debug_track_rgbd_sums: depth and luminance differ in shape")
        pr = _pose(pose_ref6); pc = _pose(pose_cur6)
        return _debug_sums(31, 2, 0, lambda *out: self._call("i3d_debug_track_rgbd_sums", C.byref(d), w, h, _p(dep), _p(lu), int(level), _p(pr), _p(pc), *out))

    def query_points(self, points, outputs=None, **desc):
        """The model at world points [n, 3] (i3d_query_points).  desc: fields of i3d_query_desc (see query_desc_default).  outputs: names out
        of QUERY_OUTPUTS, default all the descriptor allows.  Returns {name: array} (sdf, distance [n] float64; foot [n, 3] float64; normal [n, 3], albedo [n]
        float32; status [n] uint8) plus "stats": the fields of i3d_query_stats."""
        return _query(self, "i3d_query_points", points, outputs, True, desc)

    def cast_rays(self, origins, directions, t_min=None, t_max=None, outputs=None, refined=True, order=0):
        """The caller's own rays on the model (i3d_cast_rays).  origins, directions [n, 3] world (a direction need not be unit); the ray is
        o + t d over [t_min, t_max) per ray (None or <= 0: open on that side).  A segment A -> B is occluded iff the ray (A, B - A, t_max = 1) hits.  outputs:
        names out of CAST_OUTPUTS, default all but shading / intensity (which need the per-voxel SH).  order: 0 marches the rays as given, 1 in the coherent
        order (the same bits; it pays for large sets, from about a million rays).  Returns {name: array} (t [n], position [n, 3] float64; normal [n, 3], albedo, shading, intensity [n]
        float32; status [n] uint8: bit 0 marched, bit 1 hit, bit 2 out of samples) plus "stats": the fields of i3d_render_stats."""
        return _cast_rays(self, "i3d_cast_rays", (int(bool(refined)),), origins, directions, t_min, t_max, outputs, CAST_OUTPUTS, order)

    def render_view_color(self, frame=0, level=0, refined=True, planes=("color", "depth"), camera=None, depth_range=None, as_uint8=False):
        """The colour view of render_view's camera (i3d_render_view_color): "color" (h, w, 3) R, G, B, the stored colour interpolated in
        the hit's cell, float32 in units of the stored byte (0 without a hit), and "depth" (h, w) as render_view's.  No per-voxel SH is needed.  as_uint8: the
        colour rounded to nearest and clipped to uint8 on the host.  Returns {plane: array} plus "stats"."""
        if frame < 0 and camera is None:
            raise ValueError("render_view_color: frame < 0 needs a camera")
        d = _render_desc(camera if frame < 0 else None, depth_range, frame, level, refined)
        w, h = (d.width, d.height) if frame < 0 else self._level_size(level)
        out = _render_color(self, "i3d_render_view_color", d, w, h, planes, as_uint8)
        if frame >= 0 and (w, h) == (0, 0) and planes:
            raise I3DError("render_view_color: the keyframe image size is unknown (keyframes not set through this Context)")
        return out

    def cast_rays_color(self, origins, directions, t_min=None, t_max=None, outputs=None, refined=True, order=0, as_uint8=False):
        """The stored colour at the hits of the caller's own rays (i3d_cast_rays_color): rays, ranges and order as cast_rays.  outputs:
        names out of COLOR_CAST_OUTPUTS, default all.  Returns {name: array} (t [n] float64 and status [n] uint8 as cast_rays; color [n, 3] R, G, B float32 in
        units of the stored byte, or uint8 with as_uint8) plus "stats"."""
        return _color_out(_cast_rays(self, "i3d_cast_rays_color", (int(bool(refined)),), origins, directions, t_min, t_max, outputs, COLOR_CAST_OUTPUTS, order), as_uint8)

    def register_points(self, points, pose, **desc):
        """Rigid alignment of the points [n, 3] to the model (i3d_register_points).  pose: angle-axis | t, the points' frame -> world
        (x = R p + t; for camera-frame points camera -> world, the inverse of track_frame's pose).  desc: fields of i3d_register_desc (see
        register_desc_default).  Returns (pose6, stats dict)."""
        return _register(self, "i3d_register_points", points, pose, desc)

    def track_frame_sdf(self, depth, pose6, **desc):
        """Registers a depth frame ([h, w] metres, 0 = invalid) on the stored field, no ray cast (i3d_track_frame_sdf), from the initial guess
        pose6 (world->camera, angle-axis | t, as track_frame).  desc: fields of i3d_track_sdf_desc (see track_sdf_desc_default): intr / dist for the frame's camera,
        or use_context_camera=1.  Returns (pose6, stats dict)."""
        return _track(self, "i3d_track_frame_sdf", track_sdf_desc_default(**desc), TrackSdfStats, _images(depth), pose6)

    def _track_batch(self, name, stats_t, d, head, po, n):
        """the call and the return of the batch trackers: n poses in and out, one stats struct per frame -> (poses [n, 6], [stats dict per frame])"""
        st = (stats_t * max(n, 1))()
        self._call(name, C.byref(d), *head, _p(po), C.cast(st, C.c_void_p))
        return po, [st[i].as_dict() for i in range(n)]

    def _track_frames(self, name, stats_t, d, images, poses):
        """the shared body of track_frames_sdf / track_frames_sdf_rgbd: images = _images(.., batch=True)"""
        (n, w, h), img = images
        po = _pose(poses, -1, 6)
        if po.shape[0] != n:
            raise ValueError(f"{name[4:]}: one pose per frame")
        return self._track_batch(name, stats_t, d, (n, w, h, *map(_p, img)), po, n)

    def _track_keyframes(self, name, stats_t, d, poses, level, frames):
        """the shared body of track_keyframes_sdf / track_keyframes_sdf_rgbd"""
        po = _pose(poses, -1, 6)
        n = po.shape[0]
        idx = None if frames is None else np.ascontiguousarray(frames, np.int32).reshape(-1)
        if idx is not None and idx.shape[0] != n:
            raise ValueError(f"{name[4:]}: one pose per frame index")
        return self._track_batch(name, stats_t, d, (int(level), int(n), _p(idx)), po, n)

    def track_frames_sdf(self, depths, poses, **desc):
        """Registers a batch of depth frames ([B, h, w] metres, one size and one camera) on the stored field in one loop (i3d_track_frames_sdf, DESIGN.md section
        20) from the initial guesses poses [B, 6] (world->camera).  Frame b's result is track_frame_sdf's for that frame, bit for bit.  desc as track_frame_sdf.
        Returns (poses [B, 6], [stats dict per frame])."""
        return self._track_frames("i3d_track_frames_sdf", TrackSdfStats, track_sdf_desc_default(**desc),
                                  _images(depths, batch=True, bad="track_frames_sdf: depths must be [B, h, w]"), poses)

    def track_keyframes_sdf(self, poses, level=0, frames=None, **desc):
        """track_frames_sdf on the context's resident keyframe depth of pyramid level `level`, no upload (i3d_track_keyframes_sdf): the context's camera of that
        level (use_context_camera is set to 1 unless given), the start poses [num, 6] the caller's.  frames: keyframe indices, default all K in order; they may
        repeat.  The context's own poses are neither read nor written.  Returns (poses [num, 6], [stats dict per frame])."""
        return self._track_keyframes("i3d_track_keyframes_sdf", TrackSdfStats, track_sdf_desc_default(**dict(dict(use_context_camera=1), **desc)), poses, level, frames)

    def track_frame_sdf_rgbd(self, depth, lum, pose6, **desc):
        """track_frame_sdf with the photometric term on the field (i3d_track_frame_sdf_rgbd): lum [h, w] is the frame's luminance in the
        keyframes' convention, as track_frame_rgbd.  desc: geometric_weight, photo_weight, max_photo_residual and the fields of track_frame_sdf.  Returns (pose6,
        stats dict with photo_samples, photo_rms_initial, photo_rms_final)."""
        return _track(self, "i3d_track_frame_sdf_rgbd", track_sdf_rgbd_desc_default(**desc), TrackSdfRgbdStats,
                      _images(depth, lum, bad="track_frame_sdf_rgbd: depth and luminance must have one size"), pose6)

    def track_frames_sdf_rgbd(self, depths, lums, poses, **desc):
        """track_frames_sdf with the photometric term (i3d_track_frames_sdf_rgbd): depths and lums [B, h, w].  Frame b's result is track_frame_sdf_rgbd's for that
        frame, bit for bit.  Returns (poses [B, 6], [stats dict per frame])."""
        return self._track_frames("i3d_track_frames_sdf_rgbd", TrackSdfRgbdStats, track_sdf_rgbd_desc_default(**desc),
                                  _images(depths, lums, batch=True, bad="track_frames_sdf_rgbd: depths and lums must be [B, h, w]"), poses)

    def track_keyframes_sdf_rgbd(self, poses, level=0, frames=None, **desc):
        """track_keyframes_sdf with the photometric term (i3d_track_keyframes_sdf_rgbd): the resident depth and luminance of the level, no upload."""
        return self._track_keyframes("i3d_track_keyframes_sdf_rgbd", TrackSdfRgbdStats, track_sdf_rgbd_desc_default(**dict(dict(use_context_camera=1), **desc)),
                                     poses, level, frames)

    def debug_track_sdf_rgbd_sums(self, depth, lum, pose6, pivot3, **desc):
        """The 31 sums, the valid count and the photometric sample count of one pass at pose6 (world->camera) about pivot3 (i3d_debug_track_sdf_rgbd_sums)."""
        d = track_sdf_rgbd_desc_default(**desc)
        (w, h), (dep, lu) = _images(depth, lum)         # the two shapes are not compared here, unlike track_frame_sdf_rgbd
        po = _pose(pose6); pv = _pose(pivot3, 3)
        return _debug_sums(31, 2, -1, lambda *out: self._call("i3d_debug_track_sdf_rgbd_sums", C.byref(d), w, h, _p(dep), _p(lu), _p(po), _p(pv), *out))

    def debug_voxel_intensity(self, refined=True):
        """The per-voxel intensity a call of track_frame_sdf_rgbd would build now, [N] in visit order, NaN where undefined (i3d_debug_voxel_intensity)."""
        N, *_ = self.grid_info()
        c = np.zeros(int(N))
        self._call("i3d_debug_voxel_intensity", int(bool(refined)), _p(c))
        return c

    def debug_track_batch_frames(self, n):
        """Frames per internal chunk of track_frames_sdf / track_keyframes_sdf on this context (i3d_debug_track_batch_frames; <= 0: the default rule)."""
        self._call("i3d_debug_track_batch_frames", int(n))

    def debug_track_sdf_sums(self, depth, pose6, pivot3, **desc):
        """The 29 sums, the valid count and the usable-sample count of one pass at pose6 (world->camera) about pivot3 (i3d_debug_track_sdf_sums)."""
        d = track_sdf_desc_default(**desc)
        (w, h), (dep,) = _images(depth)
        po = _pose(pose6); pv = _pose(pivot3, 3)
        return _debug_sums(29, 2, -1, lambda *out: self._call("i3d_debug_track_sdf_sums", C.byref(d), w, h, _p(dep), _p(po), _p(pv), *out))

    def _level_size(self, level):
        """(width, height) of a pyramid level of the keyframes set through this object (0, 0 when unknown: the library reports the error)"""
        return self._sizes[level] if 0 <= level < len(getattr(self, "_sizes", ())) else (0, 0)

    # ---- sharding -----------------------------------------------------------------------------------------
    @staticmethod
    def comm_unique_id() -> bytes:
        buf = C.create_string_buffer(256); n = C.c_int32(0)
        _io("i3d_comm_unique_id", buf, C.byref(n))
        return buf.raw[:n.value]

    def comm_init(self, rank: int, world: int, unique_id: bytes):
        self._call("i3d_comm_init", int(rank), int(world), unique_id, len(unique_id))

    def comm_stats(self):
        """traffic log of the sharded path: dict(halo_calls, halo_bytes_sent, reduce_calls, reduce_bytes, halo_send, halo_recv, ghost_tiles, compute_list)"""
        a = [C.c_int64() for _ in range(4)]; b = [C.c_int32() for _ in range(4)]
        self._call("i3d_comm_stats", *[C.byref(x) for x in a], *[C.byref(x) for x in b])
        return dict(zip(["halo_calls", "halo_bytes_sent", "reduce_calls", "reduce_bytes", "halo_send", "halo_recv", "ghost_tiles", "compute_list"], [x.value for x in a + b]))

    def comm_transport(self) -> str:
        return (self.L.i3d_comm_transport(self.h) or b"").decode()

    def comm_init_sim(self, shared, rank: int):
        self._call("i3d_comm_init_sim", shared, int(rank))

    # ---- the path ------------------------------------------------------------------------------------------
    def optimize(self, cfg: OptimizerConfig):
        stats = (IterationStats * cfg.iterations)()
        self._call("i3d_optimize", C.byref(cfg), C.cast(stats, C.c_void_p))
        return list(stats)

    def estimate_sh(self, subvolume_size, lambda_reg, thres_shell, cap=8192):
        S = C.c_int32(0); sh = np.zeros((cap, 9)); idx = np.zeros((cap, 3), np.int32); st = ShStats()
        self._call("i3d_estimate_sh", float(subvolume_size), float(lambda_reg), float(thres_shell), C.byref(S), _p(sh), _p(idx), cap, C.byref(st))
        return sh[:S.value].copy(), idx[:S.value].copy(), st

    def debug_sh_stages(self, subvolume_size, thres_shell, cap=8192):
        """The device stage of estimate_sh before any solve (i3d_debug_sh_stages): dict(indices [S, 3] in the order estimate_sh reports them, gram [S, 10, 10],
        weight_sum [S], voxel_subvolume [N] in visit order, -1 = not eligible for the data term)."""
        cap = int(cap); n = max(cap, 0)
        S = C.c_int32(0); idx = np.zeros((n, 3), np.int32); G = np.zeros((n, 100)); w = np.zeros(n); vs = np.zeros(self.N, np.int32)
        self._call("i3d_debug_sh_stages", float(subvolume_size), float(thres_shell), cap, C.byref(S), _p(idx), _p(G), _p(w), _p(vs))
        s = S.value
        return dict(indices=idx[:s].copy(), gram=G[:s].reshape(s, 10, 10).copy(), weight_sum=w[:s].copy(), voxel_subvolume=vs)

    # ---- measurement ---------------------------------------------------------------------------------------
    def timing_enable(self, on=True):
        self._call("i3d_timing_enable", 1 if on else 0)

    def timing_select(self, names):
        """HIP events only around the launches of these categories (K_NAMES)"""
        mask = 0
        for n in names:
            mask |= 1 << K_NAMES.index(n)
        self._call("i3d_timing_select", mask)

    def timing_get_work(self):
        """like timing_get (no reset), restricted to launches that did work (>= 25 % of the category's longest launch)"""
        ms = np.zeros(len(K_NAMES)); n = np.zeros(len(K_NAMES), np.int64)
        self._call("i3d_timing_get_work", _p(ms), _p(n))
        return {k: (ms[i], int(n[i])) for i, k in enumerate(K_NAMES)}

    def timing_get_work_ex(self):
        """timing_get_work plus the launches its upper cut-off (> 4x the 90th percentile) removed: {category: (ms, launches, slow_ms, slow_launches)}"""
        ms = np.zeros(len(K_NAMES)); n = np.zeros(len(K_NAMES), np.int64); sms = np.zeros(len(K_NAMES)); sn = np.zeros(len(K_NAMES), np.int64)
        self._call("i3d_timing_get_work_ex", _p(ms), _p(n), _p(sms), _p(sn))
        return {k: (ms[i], int(n[i]), sms[i], int(sn[i])) for i, k in enumerate(K_NAMES)}

    def timing_get(self, reset=True):
        ms = np.zeros(len(K_NAMES)); n = np.zeros(len(K_NAMES), np.int64)
        self._call("i3d_timing_get", _p(ms), _p(n), 1 if reset else 0)
        return {k: (ms[i], int(n[i])) for i, k in enumerate(K_NAMES)}

    def problem_sizes(self):
        o = np.zeros(6, np.int64)
        self._call("i3d_problem_sizes", _p(o))
        return dict(zip(["active", "eg", "er", "es", "ea", "free"], [int(x) for x in o]))

    # ---- parity probes -------------------------------------------------------------------------------------
    def debug_assemble(self, cfg, iteration=0):
        s = C.c_int32(0)
        self._call("i3d_debug_assemble", C.byref(cfg), int(iteration), C.byref(s))
        self.slots = s.value
        return s.value

    def debug_flags(self):
        f = np.zeros(self.N, np.uint8)
        self._call("i3d_debug_flags", _p(f))
        return f

    def debug_eg_rows(self, jac=True):
        S = self.slots
        fr = np.zeros((self.N, S), np.int32); w = np.zeros((self.N, S), np.float32); r = np.zeros((self.N, S), np.float32)
        J = np.zeros((self.N, S, 29), np.float32) if jac else None
        self._call("i3d_debug_eg_rows", _p(fr), _p(w), _p(r), _p(J))
        return fr, w, r, J

    def debug_reg_rows(self):
        er = np.zeros(self.N, np.uint8); es = np.zeros(self.N, np.uint8); ea = np.zeros((self.N, 6), np.float32)
        self._call("i3d_debug_reg_rows", _p(er), _p(es), _p(ea))
        return er, es, ea

    def debug_neighbors(self):
        nb = np.zeros((self.N, 18), np.int32)
        self._call("i3d_debug_neighbors", _p(nb))
        return nb

    def debug_normal_eq(self):
        NP = 2 * self.N + 6 * self.K + 9
        g = np.zeros(NP); d = np.zeros(NP); cost = C.c_double(0)
        self._call("i3d_debug_normal_eq", _p(g), _p(d), C.byref(cost))
        return g, d, cost.value

    def debug_counters(self):
        """stream synchronisations of the solver path since the context was created"""
        n = C.c_int64(0)
        self._call("i3d_debug_counters", C.byref(n))
        return {"stream_syncs": int(n.value)}

    def debug_ladder_stats(self):
        """the damping ladder since the context was created: batches, row streams, system passes (= the streams of the serial loop), re-solved batches, unused systems, depth"""
        a = (C.c_int64 * 6)()
        self._call("i3d_debug_ladder_stats", a)
        return {"batches": int(a[0]), "row_streams": int(a[1]), "system_passes": int(a[2]), "resyncs": int(a[3]), "unused_systems": int(a[4]), "depth": int(a[5])}

    def debug_ladder_passes(self):
        """operator passes of the damping ladder by the number of live systems (index 0 .. 6), and how many of them were ONE paired launch"""
        a = (C.c_int64 * 8)()
        self._call("i3d_debug_ladder_passes", a)
        return {"live": [int(a[n]) for n in range(7)], "paired": int(a[7])}

    def debug_cull_stats(self):
        """(group, keyframe) pairs of the last assemble and how many the observation pass skipped (-1: culling off)."""
        a = C.c_int64(0); b = C.c_int64(0)
        self._call("i3d_debug_cull_stats", C.byref(a), C.byref(b))
        return int(a.value), int(b.value)

    def debug_jtj_apply(self, x):
        x = np.ascontiguousarray(x, np.float64); y = np.zeros_like(x)
        self._call("i3d_debug_jtj_apply", _p(x), _p(y))
        return y

    def debug_lm_script(self, cost, ngrad, nfree, radius0, lm_steps, attempts, plan=(), K=0, fix=(0, 0, 0), cdiag=None, tri=None, tail_c=None, tail_S=None):
        """The controller kernels of the trust-region loop on a scripted solve (i3d_debug_lm_script).  attempts: dict of per-attempt arrays xbr, d2xx, pcg_it,
        pcg_done, norms2 [n][2], cand_cost, debug_invalid.  plan: () = the serial loop, else the ladder's batch sizes.  Returns records (LM_RECORD_DTYPE), the final
        state and, per attempt begun / system of a batch, meta [attempt, j, B, done], radius, inv_radius, blocks / d2 / minv WITH their guards of LM_SCRIPT_GUARD floats."""
        NS, NB, NT, G = 6 * K + 9, 36 * K + 41, 21 * K + 25, LM_SCRIPT_GUARD
        f64 = lambda a, n, fill: np.full(n, fill, np.float64) if a is None else np.ascontiguousarray(a, np.float64).reshape(n)
        f32 = lambda a, n, fill: np.full(n, fill, np.float32) if a is None else np.ascontiguousarray(a, np.float32).reshape(n)
        cdiag = f64(cdiag, NS, 1.0); tail_c = f32(tail_c, NS, 1.0); tail_S = f32(tail_S, NS, 0.5)
        if tri is None:
            tri = np.zeros(NT); o = 0
            for n in [6] * K + [4, 5]:
                d = 0
                for i in range(n):
                    tri[o + d] = 1.0; d += n - i
                o += n * (n + 1) // 2
        tri = f64(tri, NT, 0.0)
        n = len(attempts["xbr"])
        a = {k: np.ascontiguousarray(attempts[k], np.float64) for k in ("xbr", "d2xx", "norms2", "cand_cost")}
        a.update({k: np.ascontiguousarray(attempts[k], np.int32) for k in ("pcg_it", "pcg_done", "debug_invalid")})
        assert all(a[k].size == (2 * n if k == "norms2" else n) for k in a)
        plan = np.ascontiguousarray(plan, np.int32)
        S = 6 * int(lm_steps) + 6 if plan.size else int(lm_steps)
        d = LmScriptDesc(float(cost), float(ngrad), float(nfree), float(radius0), int(lm_steps), int(K), int(fix[0]), int(fix[1]), int(fix[2]), n, int(plan.size), S,
                         cdiag.ctypes.data, tri.ctypes.data, tail_c.ctypes.data, tail_S.ctypes.data, a["xbr"].ctypes.data, a["d2xx"].ctypes.data, a["pcg_it"].ctypes.data,
                         a["pcg_done"].ctypes.data, a["norms2"].ctypes.data, a["cand_cost"].ctypes.data, a["debug_invalid"].ctypes.data, plan.ctypes.data if plan.size else None)
        rec = np.zeros(128, LM_RECORD_DTYPE); nrec = C.c_int32(0); nset = C.c_int32(0); state = np.zeros(25)
        meta = np.zeros((S, 4), np.int32); radius = np.zeros(S); inv_radius = np.zeros(S, np.float32)
        blocks = np.zeros((S, NB + 2 * G), np.float32); d2 = np.zeros((S, NS + 2 * G), np.float32); minv = np.zeros((S, NS + 2 * G), np.float32)
        self._call("i3d_debug_lm_script", C.byref(d), _p(rec), C.addressof(nrec), _p(state), C.addressof(nset), _p(meta), _p(radius), _p(inv_radius),
                   _p(blocks), _p(d2), _p(minv))
        ns = int(nset.value)
        names = ["cost", "radius", "decrease_factor", "ngrad", "nfree", "inv_radius", "done", "termination", "accepted", "invalid", "attempts", "successful", "lad_n"]
        st = {k: state[i] for i, k in enumerate(names)}; st["lad_radius"] = state[13:19].copy(); st["lad_inv_radius"] = state[19:25].copy()
        return {"records": rec[:int(nrec.value)].copy(), "state": st, "meta": meta[:ns], "radius": radius[:ns], "inv_radius": inv_radius[:ns],
                "blocks": blocks[:ns], "d2": d2[:ns], "minv": minv[:ns]}

    def debug_work_list(self):
        """visit-order index of every work-list entry of the last debug_assemble, in the order the row passes walk them (a wave holds 64 consecutive entries)"""
        n = C.c_int64(0)
        self._call("i3d_debug_work_list", None, 0, C.byref(n))
        out = np.zeros(max(int(n.value), 1), np.int32)
        self._call("i3d_debug_work_list", _p(out), out.shape[0], C.byref(n))
        return out[:int(n.value)]


def shard_need(A, world, anbr, active):
    """need[e] bit k: rank k's rows read entry e, which it does not own (host statement of the device plan)."""
    anbr = np.ascontiguousarray(anbr, np.int32); active = np.ascontiguousarray(active, np.uint8); need = np.zeros(A, np.uint64)
    _io("i3d_shard_need", int(A), int(world), _p(anbr), _p(active), _p(need))
    return need


def shard_plan(A, world, rank, anbr, active):
    """Host-side sharding plan (no GPU): returns chunk, own0, own1 and the compute-list mask of `rank`."""
    anbr = np.ascontiguousarray(anbr, np.int32); active = np.ascontiguousarray(active, np.uint8)
    ch = C.c_int32(); o0 = C.c_int32(); o1 = C.c_int32(); mask = np.zeros(A, np.uint8)
    _io("i3d_shard_plan", int(A), int(world), int(rank), _p(anbr), _p(active), C.byref(ch), C.byref(o0), C.byref(o1), _p(mask))
    return ch.value, o0.value, o1.value, mask.astype(bool)


# ---- on-disk formats (host-only entry points) -----------------------------------------------------------------------------
def tsdf_read(path):
    """-> dict(voxel_size, truncation, integration_weight_sample, max_load_factor, keys, sdf, weight, color) in FILE order."""
    p = str(path).encode()
    vs, tr, iw, ml = C.c_float(), C.c_float(), C.c_float(), C.c_float(); n = C.c_uint64()
    _io("i3d_tsdf_read_header", p, C.byref(vs), C.byref(tr), C.byref(iw), C.byref(n), C.byref(ml))
    N = int(n.value)
    out = dict(voxel_size=np.float32(vs.value), truncation=np.float32(tr.value), integration_weight_sample=np.float32(iw.value),
               max_load_factor=np.float32(ml.value), keys=np.zeros((N, 3), np.int32), sdf=np.zeros(N, np.float32),
               weight=np.zeros(N, np.float32), color=np.zeros((N, 3), np.uint8))
    _io("i3d_tsdf_read_records", p, N, _p(out["keys"]), _p(out["sdf"]), _p(out["weight"]), _p(out["color"]))
    return out


def tsdf_write(path, voxel_size, keys, sdf, weight, color, truncation=None, integration_weight_sample=0.0, max_load_factor=0.6):
    keys = np.ascontiguousarray(keys, np.int32); sdf = np.ascontiguousarray(sdf, np.float32)
    weight = np.ascontiguousarray(weight, np.float32); color = np.ascontiguousarray(color, np.uint8)
    tr = float(np.float32(voxel_size) * np.float32(5.0)) if truncation is None else float(truncation)
    _io("i3d_tsdf_write", str(path).encode(), float(voxel_size), tr, float(integration_weight_sample), float(max_load_factor), len(sdf),
        _p(keys), _p(sdf), _p(weight), _p(color))


def sbr_write(path, voxel_size, grid, truncation=None, integration_weight_sample=0.0, max_load_factor=0.6):
    """grid: the dict of Context.export_grid() (visit order)."""
    tr = float(np.float32(voxel_size) * np.float32(5.0)) if truncation is None else float(truncation)
    g = {k: np.ascontiguousarray(v) for k, v in grid.items() if isinstance(v, np.ndarray)}
    _io("i3d_sbr_write", str(path).encode(), float(voxel_size), tr, float(integration_weight_sample), float(max_load_factor), len(g["sdf"]),
        _p(g["keys"]), _p(g["sdf"]), _p(g["sdf_refined"]), _p(g["albedo"]), _p(g["weight"]), _p(g["color"]))


def sbr_read(path):
    p = str(path).encode()
    vs = C.c_float(); n = C.c_uint64()
    _io("i3d_tsdf_read_header", p, C.byref(vs), None, None, C.byref(n), None)
    N = int(n.value)
    out = dict(voxel_size=np.float32(vs.value), keys=np.zeros((N, 3), np.int32), sdf=np.zeros(N), sdf_refined=np.zeros(N), albedo=np.zeros(N),
               weight=np.zeros(N, np.float32), color=np.zeros((N, 3), np.uint8))
    _io("i3d_sbr_read", p, N, _p(out["keys"]), _p(out["sdf"]), _p(out["sdf_refined"]), _p(out["albedo"]), _p(out["weight"]), _p(out["color"]))
    return out


def write_poses(path, timestamps, poses_world_to_cam):
    t = np.ascontiguousarray(timestamps, np.float64); p = np.ascontiguousarray(poses_world_to_cam, np.float64).reshape(-1, 6)
    _io("i3d_write_poses", str(path).encode(), len(t), _p(t), _p(p))


def write_intrinsics(path, width, height, intr, dist):
    a = np.ascontiguousarray(intr, np.float64); d = np.ascontiguousarray(dist, np.float64)
    _io("i3d_write_intrinsics", str(path).encode(), int(width), int(height), _p(a), _p(d))


def read_intrinsics(path):
    w, h = C.c_int32(), C.c_int32(); a = np.zeros(4); d = np.zeros(5)
    rc = load().i3d_read_intrinsics(str(path).encode(), C.byref(w), C.byref(h), _p(a), _p(d))
    return rc == 0, int(w.value), int(h.value), a, d


def load_yaml_config(path):
    rc = RefineConfig(); oc = default_config()
    _io("i3d_config_load_yaml", str(path).encode(), C.byref(rc), C.byref(oc))
    return rc, oc


def yaml_get(path, key, default=None):
    buf = C.create_string_buffer(4096)
    rc = load().i3d_yaml_get(str(path).encode(), key.encode(), buf, 4096)
    if rc == 1 and default is not None:
        return default
    _io_check(rc, f"i3d_yaml_get({key})")
    return buf.value.decode()


def mesh_remove_loose_components(vertices, colors, faces):
    """MeshUtil::removeLooseComponents on arrays -> (vertices, colors or None, faces) of the largest connected component"""
    v = np.array(vertices, np.float32, copy=True).reshape(-1, 3); f = np.array(faces, np.int32, copy=True).reshape(-1, 3)
    c = None if colors is None else np.array(colors, np.uint8, copy=True).reshape(-1, 3)
    nv, nf = C.c_int64(len(v)), C.c_int64(len(f))
    _io("i3d_mesh_remove_loose_components", C.byref(nv), _p(v), _p(c), C.byref(nf), _p(f))
    return v[:nv.value].copy(), (None if c is None else c[:nv.value].copy()), f[:nf.value].copy()


COLOR_MODES = {"": 0, "albedo": 1, "normals": 2, "lap": 3, "lum": 4, "lum_grad": 5, "shading_sv": 6, "shading_sv_const": 7, "chroma": 8}   # SDFVisualization::getOutputModes' names


def visualization_colors(mode, voxel_size, keys, sdf_refined, albedo, weight, color, subvolume_size=0.0, sub_index=None, sub_sh=None, visit_rank=None):
    """SDFVisualization::applyColor<mode> on arrays (host instantiation of the export kernel's function) -> colours [n, 3]"""
    k = np.ascontiguousarray(keys, np.int32); n = len(k); out = np.zeros((n, 3), np.uint8)
    s = np.ascontiguousarray(sdf_refined, np.float64); a = np.ascontiguousarray(albedo, np.float64); w = np.ascontiguousarray(weight, np.float32); c = np.ascontiguousarray(color, np.uint8)
    si = None if sub_index is None else np.ascontiguousarray(sub_index, np.int32); ss = None if sub_sh is None else np.ascontiguousarray(sub_sh, np.float64)
    vr = None if visit_rank is None else np.ascontiguousarray(visit_rank, np.int64)
    _io("i3d_visualization_colors", COLOR_MODES[mode] if isinstance(mode, str) else int(mode), float(voxel_size), n, _p(k), _p(s), _p(a), _p(w), _p(c), _p(vr), float(subvolume_size),
        0 if si is None else len(si), _p(si), _p(ss), _p(out))
    return out


def write_ply(path, vertices, colors, faces):
    v = np.ascontiguousarray(vertices, np.float32); f = np.ascontiguousarray(faces, np.int32)
    c = None if colors is None else np.ascontiguousarray(colors, np.uint8)
    _io("i3d_write_ply", str(path).encode(), len(v), _p(v), _p(c), len(f), _p(f))


def mc_tables():
    ntri = np.zeros(256, np.uint8); tri = np.zeros((256, 16), np.int8)
    mx = load().i3d_mc_tables(_p(ntri), _p(tri))
    return ntri, tri, mx


def optimize_host(cfg, voxel_size, keys, sdf, sdf_refined, albedo, weight, color, frames, levels, intr, dist, poses, voxel_sh, device=0):
    """i3d_optimize_host: the one-call form of Optimizer::optimize (host arrays in, unknowns written back in place).  Returns
    (sdf_refined, albedo, intr, dist, poses, stats)."""
    keys = np.ascontiguousarray(keys, np.int32); sdf = np.ascontiguousarray(sdf, np.float64)
    sr = np.array(sdf_refined, np.float64); al = np.array(albedo, np.float64)
    w = np.ascontiguousarray(weight, np.float32); col = np.ascontiguousarray(color, np.uint8)
    gv = GridView(keys.shape[0], float(voxel_size), float(np.float32(voxel_size) * np.float32(5.0)), _p(keys), _p(sdf), _p(sr), _p(al), _p(w), _p(col))
    K = len(frames)
    ws = np.array([frames[0]["lum"][l].shape[1] for l in range(levels)], np.int32); hs = np.array([frames[0]["lum"][l].shape[0] for l in range(levels)], np.int32)
    arr_t = C.c_void_p * (K * levels); lum = arr_t(); dep = arr_t(); keep = []
    for f in range(K):
        for l in range(levels):
            a = np.ascontiguousarray(frames[f]["lum"][l], np.float32); b = np.ascontiguousarray(frames[f]["depth"][l], np.float32); keep += [a, b]
            lum[f * levels + l] = a.ctypes.data; dep[f * levels + l] = b.ctypes.data
    i4 = np.array(intr, np.float64); d5 = np.array(dist, np.float64); p6 = np.array(poses, np.float64); sh = np.ascontiguousarray(voxel_sh, np.float64)
    stats = (IterationStats * cfg.iterations)()
    _io("i3d_optimize_host", int(device), C.byref(cfg), C.byref(gv), _p(sr), _p(al), K, int(levels), _p(ws), _p(hs), C.cast(lum, C.c_void_p), C.cast(dep, C.c_void_p),
        _p(i4), _p(d5), _p(p6), _p(sh), C.cast(stats, C.c_void_p))
    return sr, al, i4, d5, p6, list(stats)


def resize_depth(depth, in_intr, out_w, out_h, out_intr, device=0):
    d = np.ascontiguousarray(depth, np.float32); a = np.ascontiguousarray(in_intr, np.float32); b = np.ascontiguousarray(out_intr, np.float32)
    out = np.zeros((out_h, out_w), np.float32)
    _io("i3d_resize_depth", int(device), d.shape[1], d.shape[0], _p(d), _p(a), int(out_w), int(out_h), _p(b), _p(out))
    return out


def png_decode(data: bytes):
    """cv::imdecode(buf, IMREAD_UNCHANGED) for PNG: HxW or HxWxC array (uint8 / uint16), colour in B,G,R[,A] order"""
    buf = np.frombuffer(data, np.uint8)
    w = C.c_int32(); h = C.c_int32(); ch = C.c_int32(); bd = C.c_int32()
    _io("i3d_png_info", _p(buf), buf.size, C.byref(w), C.byref(h), C.byref(ch), C.byref(bd))
    out = np.zeros((h.value, w.value, ch.value), np.uint16 if bd.value == 16 else np.uint8)
    _io("i3d_png_decode", _p(buf), buf.size, _p(out), out.nbytes)
    return out[:, :, 0] if ch.value == 1 else out


def pose_mat_to_vec6(cam_to_world):
    m = np.ascontiguousarray(cam_to_world, np.float32).reshape(16); out = np.zeros(6)
    _io("i3d_pose_mat_to_vec6", _p(m), _p(out))
    return out


def keyframes_load(path):
    """KeyframeSelection::load -> (window_size, scores, is_keyframe)"""
    win = C.c_int32(0); n = C.c_uint64(0)
    _io("i3d_keyframes_load", path.encode(), C.byref(win), 0, None, None, C.byref(n))
    scores = np.zeros(n.value); kf = np.zeros(n.value, np.uint8)
    _io("i3d_keyframes_load", path.encode(), C.byref(win), n.value, _p(scores), _p(kf), C.byref(n))
    return win.value, scores, kf.astype(bool)


def keyframes_save(path, window_size, scores, is_keyframe):
    s = np.ascontiguousarray(scores, np.float64); k = np.ascontiguousarray(is_keyframe, np.uint8)
    _io("i3d_keyframes_save", path.encode(), int(window_size), s.size, _p(s), _p(k))


def keyframes_select(window_size, scores):
    s = np.ascontiguousarray(scores, np.float64); k = np.zeros(s.size, np.uint8)
    _io("i3d_keyframes_select", int(window_size), s.size, _p(s), _p(k))
    return k.astype(bool)


class Sensor:
    """Sensor::create on an Intrinsic3D dataset folder (rgbd/sensor_i3d.cpp); decoding happens on demand, like the reference"""

    def __init__(self, folder=None, max_frames=0, min_depth=0.0, max_depth=0.0, yml=None):
        self.L = load(); self.h = C.c_void_p(); self.depth_range = (float(min_depth), float(max_depth))
        if yml is not None:                                           # Sensor::create(Settings(sensor.yml))
            lo = C.c_float(); hi = C.c_float()
            _io("i3d_sensor_open_yaml", str(yml).encode(), C.byref(self.h), C.byref(lo), C.byref(hi))
            self.depth_range = (lo.value, hi.value)
        else:
            _io("i3d_sensor_open", str(folder).encode(), int(max_frames), float(min_depth), float(max_depth), C.byref(self.h))
        nf = C.c_int32(); nl = C.c_int32(); cwh = np.zeros(2, np.int32); dwh = np.zeros(2, np.int32); ci = np.zeros(4, np.float32); di = np.zeros(4, np.float32)
        _io("i3d_sensor_info", self.h, C.byref(nf), C.byref(nl), _p(cwh), _p(dwh), _p(ci), _p(di))
        self.num_frames, self.num_loaded = nf.value, nl.value
        self.color_size, self.depth_size, self.color_intrinsics, self.depth_intrinsics = tuple(cwh), tuple(dwh), ci, di

    def close(self):
        if self.h:
            self.L.i3d_sensor_close(self.h); self.h = None

    def __del__(self):
        self.close()

    def color(self, i):
        out = np.zeros((self.color_size[1], self.color_size[0], 3), np.uint8)
        _io("i3d_sensor_color", self.h, int(i), _p(out)); return out

    def depth(self, i):
        out = np.zeros((self.depth_size[1], self.depth_size[0]), np.float32)
        _io("i3d_sensor_depth", self.h, int(i), _p(out)); return out

    def pose(self, i):
        out = np.zeros((4, 4), np.float32)
        _io("i3d_sensor_pose", self.h, int(i), _p(out)); return out

    def set_pose(self, i, cam_to_world):
        m = np.ascontiguousarray(cam_to_world, np.float32)
        _io("i3d_sensor_set_pose", self.h, int(i), _p(m))

    def set_pose_vec6(self, i, pose_world_to_cam):
        p = np.ascontiguousarray(pose_world_to_cam, np.float64)
        _io("i3d_sensor_set_pose_vec6", self.h, int(i), _p(p))

    def save_poses(self, path):
        _io("i3d_sensor_save_poses", self.h, str(path).encode())


def init_frames_from_sensor(ctx: "Context", sensor: Sensor, is_keyframe, levels, device=0):
    """Intrinsic3D::init's keyframe loop; returns the frame ids of the keyframes (ImageFormationModel::frame_ids)"""
    kf = np.ascontiguousarray(is_keyframe, np.uint8); ids = np.zeros(max(1, int(kf.sum())), np.int32); nk = C.c_int32(0)
    ctx._call("i3d_init_frames_from_sensor", int(device), sensor.h, kf.size, _p(kf), int(levels), ids.size, _p(ids), C.byref(nk))
    ctx.K = nk.value
    ctx._sizes = _pyramid_sizes(sensor.color_size[0], sensor.color_size[1], levels)
    return ids[:nk.value]


class Fusion(_Handle):
    """AppFusion::fuseSDF's volume on the device: integrate() per frame, then finish() = correctSDF + clearInvalidVoxels"""
    _destroy, _last_error = "i3d_fusion_destroy", "i3d_fusion_last_error"

    def __init__(self, voxel_size, depth_min, depth_max, clip=None, initial_capacity=1 << 20, device=0):
        self.L = load(); self.h = C.c_void_p()
        c = None if clip is None else np.ascontiguousarray(clip, np.float32)
        _io("i3d_fusion_create", int(device), float(voxel_size), float(depth_min), float(depth_max), _p(c), int(initial_capacity), C.byref(self.h))

    @staticmethod
    def _frame(depth, dcam, bgr, ccam):
        d = np.ascontiguousarray(depth, np.float32); b = np.ascontiguousarray(bgr, np.uint8)
        dc = np.ascontiguousarray(dcam, np.float32); cc = np.ascontiguousarray(ccam, np.float32)
        return (d.shape[1], d.shape[0], _p(dc), b.shape[1], b.shape[0], _p(cc), _p(d), _p(b)), (d, b, dc, cc)

    def integrate(self, depth, dcam, bgr, ccam, pose_c2w, erode_window=2):
        """Fuses one frame; returns its ordinal (info()["frames"] before the call), the name deintegrate / reintegrate know it by."""
        args, keep = self._frame(depth, dcam, bgr, ccam); T = np.ascontiguousarray(pose_c2w, np.float32)
        ordinal = C.c_uint64(0)
        self._call("i3d_fusion_info", C.byref(ordinal), None, None, None)
        self._call("i3d_fusion_integrate", *args, _p(T), int(erode_window))
        return int(ordinal.value)

    def deintegrate(self, ordinal, depth, dcam, bgr, ccam, pose_c2w, erode_window=2):
        """Takes the frame of that ordinal out again (i3d_fusion_deintegrate); the frame arguments must be those it was fused with."""
        args, keep = self._frame(depth, dcam, bgr, ccam); T = np.ascontiguousarray(pose_c2w, np.float32)
        self._call("i3d_fusion_deintegrate", int(ordinal), *args, _p(T), int(erode_window))

    def reintegrate(self, ordinal, depth, dcam, bgr, ccam, old_pose_c2w, new_pose_c2w, erode_window=2):
        """Moves the frame of that ordinal from the pose it was fused at to new_pose_c2w in one pass over the table (i3d_fusion_reintegrate); returns its new
        ordinal.  Bit-identical to deintegrate followed by integrate."""
        args, keep = self._frame(depth, dcam, bgr, ccam)
        T0 = np.ascontiguousarray(old_pose_c2w, np.float32); T1 = np.ascontiguousarray(new_pose_c2w, np.float32); new = C.c_uint64(0)
        self._call("i3d_fusion_reintegrate", int(ordinal), *args, _p(T0), int(erode_window), _p(T1), C.byref(new))
        return int(new.value)

    def merge(self, src, pose6=None):
        """Fuses the volume src into this one under x_self = R x_src + t, pose6 = angle-axis | t (None = identity): the pose register_points(points in src's
        frame) returns (i3d_fusion_merge).  src is left as it is.  Returns dict(ordinal, source_voxels, sampled, allocated, aligned,
        rotation [3, 3], translation_voxels [3]) - the motion exactly as the kernels used it."""
        if not isinstance(src, Fusion) or not src.h:
            raise ValueError("Fusion.merge: src must be an open Fusion")
        p = None if pose6 is None else _pose(pose6)
        st = MergeStats()
        self._call("i3d_fusion_merge", src.h, _p(p), C.byref(st))
        return dict(ordinal=int(st.ordinal), source_voxels=int(st.source_voxels), sampled=int(st.sampled), allocated=int(st.allocated), aligned=int(st.aligned),
                    rotation=np.array(st.rotation[:], np.float64).reshape(3, 3), translation_voxels=np.array(st.translation_voxels[:], np.float64))

    def prune(self, min_weight=0.0, max_abs_sdf=0.0, box=None, box_mode=None, shrink=False):
        """Drops the stored voxels that fail a criterion and moves the rest into a fresh table (i3d_fusion_prune): weight not above
        min_weight (off when negative), |sdf| above max_abs_sdf (off when 0), outside box = (x0, x1, y0, y1, z0, z1) in metres with box_mode 1 or inside it with
        box_mode 2 (a given box with box_mode None means 1).  The defaults remove exactly the weightless voxels.  shrink: the table of a fresh volume sized for the
        survivors.  Returns dict(stored, removed, failed_weight, failed_sdf, failed_box), stored = the count before the call."""
        b = None if box is None else np.ascontiguousarray(box, np.float32).reshape(6)
        mode = (0 if box is None else 1) if box_mode is None else int(box_mode)
        counts = np.zeros(5, np.int64)
        self._call("i3d_fusion_prune", float(min_weight), float(max_abs_sdf), mode, _p(b), int(bool(shrink)), _p(counts))
        return dict(zip(("stored", "removed", "failed_weight", "failed_sdf", "failed_box"), (int(c) for c in counts)))

    def components(self, min_weight=0.0, max_abs_sdf=0.0):
        """The 6-connected components of the stored voxels that pass prune()'s weight and |sdf| criteria, the volume left as it is (i3d_fusion_components, DESIGN.md
        section 39).  Returns dict(nodes, components, largest, keys [nodes, 3] int32 in ascending packed key, label [nodes] int32, sizes [components] int64):
        components are numbered by descending size, ties by ascending smallest packed key."""
        counts = np.zeros(3, np.int64)
        self._call("i3d_fusion_components", float(min_weight), float(max_abs_sdf), _p(counts))
        keys = np.zeros((int(counts[0]), 3), np.int32); label = np.zeros(int(counts[0]), np.int32); sizes = np.zeros(int(counts[1]), np.int64)
        self._call("i3d_fusion_get_components", _p(keys), _p(label), _p(sizes))
        return dict(nodes=int(counts[0]), components=int(counts[1]), largest=int(counts[2]), keys=keys, label=label, sizes=sizes)

    def prune_components(self, min_weight=0.0, max_abs_sdf=0.0, min_voxels=0, keep_largest=0, shrink=False):
        """Drops every node of the components with fewer than min_voxels nodes (off when 0) or numbered keep_largest and above (off when 0), as prune() drops
        voxels (i3d_fusion_prune_components).  Returns dict(stored, removed, nodes, components, components_removed)."""
        counts = np.zeros(5, np.int64)
        self._call("i3d_fusion_prune_components", float(min_weight), float(max_abs_sdf), int(min_voxels), int(keep_largest), int(bool(shrink)), _p(counts))
        return dict(zip(("stored", "removed", "nodes", "components", "components_removed"), (int(c) for c in counts)))

    def register_volume(self, src, pose, **desc):
        """The pose merge(src, pose) takes, found on the two stored fields: src's voxels near its surface placed into this volume, r = field here - value stored
        there (i3d_fusion_register_volume).  pose = the start, angle-axis | t, x_self = R x_src + t.  Both volumes are left as they are.
        Returns (pose6, stats dict: the fields of register_points' and `selected`)."""
        if not isinstance(src, Fusion) or not src.h:
            raise ValueError("Fusion.register_volume: src must be an open Fusion")
        d = register_volume_desc_default(**desc)
        p6 = _pose(pose); st = RegisterVolumeStats()
        self._call("i3d_fusion_register_volume", src.h, C.byref(d), _p(p6), C.byref(st))
        return p6, st.as_dict()

    def debug_register_volume_selection(self, **desc):
        """The samples register_volume(src=self) would take, in the order of its sums (i3d_fusion_debug_register_volume_selection): dict(keys [n, 3] int32, sdf [n])."""
        d = register_volume_desc_default(**desc)
        n = C.c_int64(0)
        self._call("i3d_fusion_debug_register_volume_selection", C.byref(d), 0, None, None, C.byref(n))
        keys = np.zeros((n.value, 3), np.int32); sdf = np.zeros(n.value, np.float32)
        if n.value:
            self._call("i3d_fusion_debug_register_volume_selection", C.byref(d), n.value, _p(keys), _p(sdf), C.byref(n))
        return dict(keys=keys, sdf=sdf)

    def debug_register_volume_sums(self, src, pose6, pivot3, limit=0, row_cap=0, **desc):
        """One pass of register_volume's sums at pose6 about pivot3 over the first `limit` samples (0: all) with at most row_cap slab rows (0: 8192)
        (i3d_fusion_debug_register_volume_sums): (sums [29], valid, selected)."""
        d = register_volume_desc_default(**desc)
        po = _pose(pose6); pv = _pose(pivot3, 3)
        return _debug_sums(29, 2, 0, lambda *out: self._call("i3d_fusion_debug_register_volume_sums", src.h, C.byref(d), _p(po), _p(pv), int(limit), int(row_cap), *out))

    def debug_voxels(self, keys):
        """The live table at the voxel keys [n, 3] without finishing the volume (i3d_fusion_debug_voxels): dict(found, sdf, weight, color, first_frame), first_frame =
        the ordinal of the frame that first inserted the voxel, -1 where the key is not stored."""
        k = np.ascontiguousarray(keys, np.int32).reshape(-1, 3); n = k.shape[0]
        out = dict(found=np.zeros(n, np.uint8), sdf=np.zeros(n, np.float32), weight=np.zeros(n, np.float32), color=np.zeros((n, 3), np.uint8),
                   first_frame=np.full(n, -1, np.int64))
        self._call("i3d_fusion_debug_voxels", n, _p(k), *[_p(a) for a in out.values()])
        out["found"] = out["found"].astype(bool)
        return out

    def debug_poke_voxels(self, keys, sdf, weight, color):
        """Overwrites sdf, weight and colour of the voxels that are stored at the distinct keys [n, 3]; nothing is inserted (i3d_fusion_debug_poke_voxels).  Returns
        found [n] bool: False where the key is not stored and nothing was written."""
        k = np.ascontiguousarray(keys, np.int32).reshape(-1, 3); n = k.shape[0]
        s = np.ascontiguousarray(sdf, np.float32).reshape(n); w = np.ascontiguousarray(weight, np.float32).reshape(n)
        c = np.ascontiguousarray(color, np.uint8).reshape(n, 3); found = np.zeros(n, np.uint8)
        self._call("i3d_fusion_debug_poke_voxels", n, _p(k), _p(s), _p(w), _p(c), _p(found))
        return found.astype(bool)

    def debug_frame_samples(self, keys, depth, dcam, bgr, ccam, pose_c2w, erode_window=2):
        """What the frame contributes to the voxels at keys [n, 3], stored or not, with no table write (i3d_fusion_debug_frame_samples): dict(on, sample, wu,
        has_color, rgb)."""
        k = np.ascontiguousarray(keys, np.int32).reshape(-1, 3); n = k.shape[0]
        args, keep = self._frame(depth, dcam, bgr, ccam); T = np.ascontiguousarray(pose_c2w, np.float32)
        out = dict(on=np.zeros(n, np.uint8), sample=np.zeros(n, np.float32), wu=np.zeros(n, np.float32), has_color=np.zeros(n, np.uint8), rgb=np.zeros((n, 3), np.uint8))
        self._call("i3d_fusion_debug_frame_samples", *args, _p(T), int(erode_window), n, _p(k), *[_p(a) for a in out.values()])
        out["on"] = out["on"].astype(bool); out["has_color"] = out["has_color"].astype(bool)
        return out

    # ---- resume a volume ------------------------------------------------------------------------------------------
    _snapshot_count = None          # records of the last snapshot() of the open volume; finish() replaces them

    @classmethod
    def load(cls, path, depth_min, depth_max, clip=None, device=0):
        """The volume saved at path (a .tsdf), open for further frames (i3d_fusion_load): voxel size, truncation and integration weight sample are the file's."""
        self = cls.__new__(cls)
        self.L = load(); self.h = C.c_void_p()
        c = None if clip is None else np.ascontiguousarray(clip, np.float32)
        _io("i3d_fusion_load", int(device), str(path).encode(), float(depth_min), float(depth_max), _p(c), C.byref(self.h))
        return self

    def insert_records(self, keys, sdf, weight, color):
        """The records keys [n, 3], sdf, weight, color [n, 3] R,G,B stored as given into this empty, untouched volume (i3d_fusion_insert_records); the load is
        ordinal 0.  What follows (snapshot, finish, save) has the reference's record order after load, not the order given here."""
        k = np.ascontiguousarray(keys, np.int32).reshape(-1, 3); n = k.shape[0]
        s = np.ascontiguousarray(sdf, np.float32).reshape(n); w = np.ascontiguousarray(weight, np.float32).reshape(n)
        c = np.ascontiguousarray(color, np.uint8).reshape(n, 3)
        self._call("i3d_fusion_insert_records", n, _p(k), _p(s), _p(w), _p(c))

    def snapshot(self):
        """The records finish(0) would produce, with the volume left open (i3d_fusion_snapshot): returns their count; export() and save() then give these records
        until the next snapshot() or finish()."""
        n = C.c_uint64(0)
        self._call("i3d_fusion_snapshot", C.byref(n))
        self._snapshot_count = int(n.value)
        return self._snapshot_count

    def debug_insertion_order(self):
        """The keys [m, 3] of the stored voxels, weight-0 ones included, in the order of their first insertion (i3d_fusion_debug_insertion_order)."""
        n = C.c_uint64(0)
        rc = self.L.i3d_fusion_debug_insertion_order(self.h, 0, None, C.byref(n))
        if rc not in (0, 5):                        # I3D_ERR_CAPACITY: the count has been written
            self._check(rc, "i3d_fusion_debug_insertion_order")
        keys = np.zeros((n.value, 3), np.int32)
        if n.value:
            self._call("i3d_fusion_debug_insertion_order", n.value, _p(keys), C.byref(n))
        return keys

    def finish(self, correct_iterations=10):
        n = C.c_uint64(0)
        self._call("i3d_fusion_finish", int(correct_iterations), C.byref(n))
        self._snapshot_count = None
        return n.value

    def info(self):
        fr = C.c_uint64(); al = C.c_uint64(); cap = C.c_uint64(); cl = C.c_int32()
        self._call("i3d_fusion_info", C.byref(fr), C.byref(al), C.byref(cap), C.byref(cl))
        return dict(frames=fr.value, allocated=al.value, capacity=cap.value, correct_launches=cl.value)

    def export(self):
        """The records of the finished volume (finish() with its default runs first if it has not), or of the last snapshot() of a volume that is still open."""
        n = self.finish() if self._snapshot_count is None else self._snapshot_count
        keys = np.zeros((n, 3), np.int32); sdf = np.zeros(n, np.float32); w = np.zeros(n, np.float32); col = np.zeros((n, 3), np.uint8)
        self._call("i3d_fusion_get", _p(keys), _p(sdf), _p(w), _p(col))
        return dict(keys=keys, sdf=sdf, weight=w, color=col)

    def save(self, path):
        self._call("i3d_fusion_save", str(path).encode())

    def extract_mesh(self, min_weight=0.0, largest_component_only=False, stats=False):
        """An indexed, welded mesh of the volume as it stands, before or after finish() (i3d_fusion_extract_mesh): (vertices [nv, 3] float32,
        colors [nv, 3] uint8 R,G,B, faces [nf, 3] int32[, stats dict])."""
        d = fusion_mesh_desc_default(min_weight=float(min_weight), largest_component_only=int(largest_component_only))
        nv = C.c_int64(0); nf = C.c_int64(0); st = FusionMeshStats()
        self._call("i3d_fusion_extract_mesh", C.byref(d), C.byref(nv), C.byref(nf), C.byref(st))
        v = np.zeros((nv.value, 3), np.float32); c = np.zeros((nv.value, 3), np.uint8); f = np.zeros((nf.value, 3), np.int32)
        self._call("i3d_fusion_get_mesh", _p(v), _p(c), _p(f))
        return (v, c, f, st.as_dict()) if stats else (v, c, f)

    def export_mesh_ply(self, path, **desc):
        """extract_mesh(**desc) written as a binary PLY (i3d_fusion_export_mesh_ply); an empty mesh is an error."""
        d = fusion_mesh_desc_default(**{k: (float(v) if k == "min_weight" else int(v)) for k, v in desc.items()})
        self._call("i3d_fusion_export_mesh_ply", C.byref(d), str(path).encode())

    # ---- the volume as a model while it is being fused ----------------------------------------------------------
    def render(self, camera, planes=("depth", "normal"), depth_range=None):
        """Ray-casts the volume as it stands into camera = dict(width, height, intr, dist, pose) (pose world->camera, angle-axis | t).  planes: "depth" and / or
        "normal"; depth_range = (min, max) camera z, <= 0 open.  Returns the dict of Context.render_view (residual_sq_sum is 0)."""
        unknown = set(planes) - {"depth", "normal"}
        if unknown:
            raise ValueError(f"Fusion.render: unknown planes {sorted(unknown)} (a fusion volume has depth and normal only)")
        d = _render_desc(camera, depth_range)
        out = _planes(planes, d.width, d.height)
        st = RenderStats()
        self._call("i3d_fusion_render", C.byref(d), _p(out.get("depth")), _p(out.get("normal")), C.byref(st))
        out["stats"] = st.as_dict()
        return out

    def track(self, depth, pose6, intrinsics, **desc):
        """Registers a depth frame ([h, w] metres, depth geometry, 0 = invalid) against the volume as it stands from the initial guess pose6 (world->camera,
        angle-axis | t); intrinsics = the depth camera's fx, fy, cx, cy.  desc: other fields of i3d_track_desc (see track_desc_default; dist for a distortion).
        Returns (pose6, stats dict), as Context.track_frame."""
        d = track_desc_default(intr=intrinsics, **desc)
        d.use_context_camera = 0
        return _track(self, "i3d_fusion_track", d, TrackStats, _images(depth), pose6)

    def query_points(self, points, outputs=None, **desc):
        """Context.query_points over the volume as it stands, before or after finish() (i3d_fusion_query_points): no albedo, use_refined_sdf ignored."""
        return _query(self, "i3d_fusion_query_points", points, outputs, False, desc)

    def cast_rays(self, origins, directions, t_min=None, t_max=None, outputs=None, order=0):
        """Context.cast_rays over the volume as it stands, before or after finish() (i3d_fusion_cast_rays): t, position, normal and status only."""
        return _cast_rays(self, "i3d_fusion_cast_rays", (), origins, directions, t_min, t_max, outputs, ("t", "position", "normal", "status"), order)

    def render_color(self, camera, planes=("color", "depth"), depth_range=None, as_uint8=False):
        """Context.render_view_color over the volume as it stands, before or after finish() (i3d_fusion_render_color): the fused colour interpolated in the hit's
        cell; a voxel that received depth but never colour counts as black."""
        d = _render_desc(camera, depth_range)
        return _render_color(self, "i3d_fusion_render_color", d, d.width, d.height, planes, as_uint8)

    def cast_rays_color(self, origins, directions, t_min=None, t_max=None, outputs=None, order=0, as_uint8=False):
        """Context.cast_rays_color over the volume as it stands, before or after finish() (i3d_fusion_cast_rays_color)."""
        return _color_out(_cast_rays(self, "i3d_fusion_cast_rays_color", (), origins, directions, t_min, t_max, outputs, COLOR_CAST_OUTPUTS, order), as_uint8)

    def track_sdf(self, depth, pose6, intrinsics, **desc):
        """Context.track_frame_sdf against the volume as it stands, before or after finish() (i3d_fusion_track_sdf); intrinsics = the depth camera's fx, fy, cx,
        cy; use_refined_sdf ignored.  Returns (pose6, stats dict)."""
        return _track(self, "i3d_fusion_track_sdf", track_sdf_desc_default(intr=intrinsics, **desc), TrackSdfStats, _images(depth), pose6)

    def track_sdf_rgbd(self, depth, lum, pose6, intrinsics, **desc):
        """Context.track_frame_sdf_rgbd against the volume as it stands, with the luminance of its fused colour for the appearance (i3d_fusion_track_sdf_rgbd,
        DESIGN.md section 22); lum [h, w] is the frame's luminance at the depth camera's geometry, NaN where there is none; intrinsics = the depth camera's fx,
        fy, cx, cy.  Returns (pose6, stats dict with photo_samples, photo_rms_initial, photo_rms_final)."""
        return _track(self, "i3d_fusion_track_sdf_rgbd", track_sdf_rgbd_desc_default(intr=intrinsics, **desc), TrackSdfRgbdStats,
                      _images(depth, lum, bad="Fusion.track_sdf_rgbd: depth and luminance must have one size"), pose6)

    def debug_voxel_luminance(self, keys):
        """The luminance volume a call of track_sdf_rgbd would build now at the voxel keys [n, 3]: [n], NaN where the key is not stored or the voxel has weight 0
        (i3d_fusion_debug_voxel_luminance)."""
        k = np.ascontiguousarray(keys, np.int32).reshape(-1, 3)
        c = np.zeros(k.shape[0])
        self._call("i3d_fusion_debug_voxel_luminance", int(k.shape[0]), _p(k), _p(c))
        return c

    def debug_track_sdf_rgbd_sums(self, depth, lum, pose6, pivot3, intrinsics, **desc):
        """The 31 sums, the valid count and the photometric sample count of one pass at pose6 (world->camera) about pivot3 (i3d_fusion_debug_track_sdf_rgbd_sums)."""
        d = track_sdf_rgbd_desc_default(intr=intrinsics, **desc)
        (w, h), (dep, lu) = _images(depth, lum)         # the two shapes are not compared here, unlike track_sdf_rgbd
        po = _pose(pose6); pv = _pose(pivot3, 3)
        return _debug_sums(31, 2, -1, lambda *out: self._call("i3d_fusion_debug_track_sdf_rgbd_sums", C.byref(d), w, h, _p(dep), _p(lu), _p(po), _p(pv), *out))

    def register_points(self, points, pose, **desc):
        """Context.register_points against the volume as it stands, before or after finish() (i3d_fusion_register_points): use_refined_sdf ignored."""
        return _register(self, "i3d_fusion_register_points", points, pose, desc)


def debug_map_order(keys, mode=0):
    k = np.ascontiguousarray(keys, np.int32); out = np.zeros(k.shape[0], np.int32)
    n = load().i3d_debug_map_order(_p(k), k.shape[0], int(mode), _p(out))
    return out[:n]


def blur_score(image):
    """KeyframeSelection::estimateBlur of an HxW (grey) or HxWx3 (B,G,R) uint8 image"""
    a = np.ascontiguousarray(image, np.uint8); out = C.c_double(0)
    _io("i3d_blur_score", _p(a), a.shape[1], a.shape[0], 1 if a.ndim == 2 else a.shape[2], C.byref(out))
    return out.value
