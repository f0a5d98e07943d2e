"""ctypes binding of ``libyart_hip.so`` and a host-side mirror of the reference's
renderer interface.

The reference's seam is the abstract class ``yart::Renderer`` (reference
``src/core/renderer.hpp:17-104``) implemented by ``yart::cpu::TileRenderer``
(``src/cpu/tile-renderer.hpp:22-310``).  :class:`HipTileRenderer` keeps that
surface — public knobs ``samples / first_wave_samples / max_wave_samples /
tile_size / background_color / scene``, methods ``render() / abort() / wait() /
render_sync()`` returning a ``RenderData`` — on top of the C ABI declared in
``include/yart_hip.h``.

There is no CPU fallback: if the shared library is missing, or no HIP device is
visible, every entry point raises.
"""
from __future__ import annotations

import ctypes as C
import os
import threading
import time
from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np

from . import yscn
from .denoise import (DEFAULT_ITERATIONS, DEFAULT_SIGMA_COLOR, DEFAULT_SIGMA_DEPTH, DEFAULT_SIGMA_NORMAL, FLAG_DEMODULATE,
                      atrous_reference)  # noqa: F401 (atrous_reference: the NumPy statement of denoise / denoise_into)
from .denoise import (DEFAULT_VAR_ITERATIONS, DEFAULT_VAR_SIGMA_DEPTH, DEFAULT_VAR_SIGMA_LUMA, DEFAULT_VAR_SIGMA_NORMAL,
                      atrous_var_reference)  # noqa: F401 (the NumPy statement of denoise_var / denoise_var_into)
from .moments import moments_reference  # noqa: F401 (the NumPy statement of render_moments / probe_moments)
from .temporal import (DEFAULT_ALPHA_MIN, DEFAULT_CLIP_GAMMA, DEFAULT_CLIP_RADIUS, DEFAULT_MAX_HISTORY, DEFAULT_MIN_MOMENT_HISTORY, DEFAULT_NORMAL_COS_MIN,
                       DEFAULT_PLANE_TOLERANCE, MOTION_WORDS, clip_of, node_motion, temporal_moments_reference,
                       temporal_reference)  # noqa: F401 (the NumPy statement of TemporalAccumulator.accumulate / accumulate_into)
from .exposure import (ExposureState, apply_reference, exposure_reference, look_index,
                       params_of as exposure_params_of)  # noqa: F401 (the NumPy statement of AutoExposure.meter / apply)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libyart_hip.so")
if os.environ.get("YART_LIB_VARIANT"):      # experiment builds of tools/build_variant.sh (yart_amd/_variants/NAME.so)
    LIB_PATH = os.path.join(_HERE, "_variants", os.environ["YART_LIB_VARIANT"] + ".so")

YART_OK, YART_E_INVALID, YART_E_NO_DEVICE, YART_E_HIP, YART_E_IO, YART_E_RCCL = 0, -1, -2, -3, -4, -5
ABI_VERSION = 3          # include/yart_hip.h: YART_HIP_ABI_VERSION (struct layouts below)
FLAG_MEGAKERNEL = 1
FLAG_SHADE_SORT = 2
FLAG_GENERAL_TRACE = 4
FLAG_DIRECT_SAMPLER = 8
FLAG_NO_REFILL = 16
FLAG_NO_COMPACTION = 32
FLAG_NO_SHADE_SORT = 64
FLAG_NO_RESUME = 128
FLAG_PATH_POOL = 512


class YartError(RuntimeError):
    def __init__(self, code, message):
        super().__init__(f"yart_hip error {code}: {message}")
        self.code = code


# ---------------------------------------------------------------------------
# POD mirrors of include/yart_hip.h
# ---------------------------------------------------------------------------
class TextureDesc(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("channels", C.c_uint32),
                ("is_float", C.c_uint32), ("type", C.c_uint32), ("data", C.c_void_p)]


class MaterialDesc(C.Structure):
    _fields_ = [("base", C.c_float * 3), ("emission", C.c_float * 3),
                ("metallic", C.c_float), ("roughness", C.c_float), ("transmission", C.c_float),
                ("ior", C.c_float), ("anisotropic", C.c_float), ("aniso_rotation", C.c_float),
                ("clearcoat", C.c_float), ("clearcoat_roughness", C.c_float),
                ("normal_scale", C.c_float), ("thin_transmission", C.c_uint32),
                ("volume_color", C.c_float * 3), ("volume_density", C.c_float),
                ("tex_base", C.c_int32), ("tex_mr", C.c_int32), ("tex_transmission", C.c_int32),
                ("tex_normal", C.c_int32), ("tex_clearcoat", C.c_int32), ("tex_emission", C.c_int32)]


class MeshDesc(C.Structure):
    _fields_ = [("n_vertices", C.c_uint32), ("n_faces", C.c_uint32),
                ("positions", C.c_void_p), ("normals", C.c_void_p), ("tangents", C.c_void_p),
                ("uvs", C.c_void_p), ("faces", C.c_void_p), ("face_light", C.c_void_p)]


class NodeDesc(C.Structure):
    _fields_ = [("parent", C.c_int32), ("mesh", C.c_int32), ("fwd", C.c_float * 16), ("inv", C.c_float * 16)]


class LightDesc(C.Structure):
    _fields_ = [("type", C.c_uint32), ("mesh", C.c_int32), ("tri", C.c_uint32), ("two_sided", C.c_uint32),
                ("texture", C.c_int32), ("radius", C.c_float), ("emission", C.c_float * 3),
                ("fwd", C.c_float * 16), ("inv", C.c_float * 16)]


class SceneUpdate(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("n_nodes", C.c_uint32), ("nodes", C.POINTER(NodeDesc)),
                ("n_lights", C.c_uint32), ("lights", C.POINTER(LightDesc)), ("flags", C.c_uint32)]


class SceneGraphUpdate(C.Structure):                # YartSceneGraphUpdate: the fields of YartSceneUpdate, n_nodes / nodes the NEW list
    _fields_ = SceneUpdate._fields_


class SceneUpdateStats(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("launches", C.c_uint32), ("ms_total", C.c_double), ("ms_device", C.c_double)]


class MeshUpdate(C.Structure):
    _fields_ = [("mesh", C.c_uint32), ("n_vertices", C.c_uint32), ("positions", C.c_void_p), ("normals", C.c_void_p),
                ("tangents", C.c_void_p)]


class SceneMeshUpdate(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("n_meshes", C.c_uint32), ("meshes", C.POINTER(MeshUpdate)), ("flags", C.c_uint32)]


class MeshReplace(C.Structure):                     # YartMeshReplace: a mesh index and what create takes for a mesh
    _fields_ = [("mesh", C.c_uint32), ("desc", MeshDesc)]


class SceneMeshReplace(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("n_meshes", C.c_uint32), ("meshes", C.POINTER(MeshReplace)), ("flags", C.c_uint32)]


GEOMETRY_PROBE_ARRAYS = ("bvh_nodes", "leaf_tris", "shade_tris", "tri_verts", "tri_light", "vpos", "vnormal", "vtangent", "vuv", "meshes")


class GeometryProbe(C.Structure):
    _fields_ = ([("struct_size", C.c_uint32), ("stack_bound", C.c_uint32)] + [("n_" + n, C.c_uint64) for n in GEOMETRY_PROBE_ARRAYS] +
                [(n, C.c_void_p) for n in GEOMETRY_PROBE_ARRAYS])


class EnvImageUpdate(C.Structure):
    _fields_ = [("texture", C.c_uint32), ("width", C.c_uint32), ("height", C.c_uint32), ("pixels", C.c_void_p)]


class SceneLightingUpdate(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("n_materials", C.c_uint32), ("materials", C.POINTER(MaterialDesc)),
                ("n_lights", C.c_uint32), ("lights", C.POINTER(LightDesc)), ("n_images", C.c_uint32),
                ("images", C.POINTER(EnvImageUpdate)), ("flags", C.c_uint32)]


LIGHTING_PROBE_ARRAYS = ("materials", "mat_class", "lights", "envs", "env_data", "env_guide", "area_power_cdf", "tex_f32", "tex_quads",
                         "textures")


class LightingProbe(C.Structure):
    _fields_ = ([("struct_size", C.c_uint32), ("total_power", C.c_float)] +
                [(n, C.c_uint64) for n in ("n_materials", "n_mat_class", "n_lights", "n_envs", "n_env_data", "n_env_guide",
                                           "n_area_power_cdf", "n_tex_f32", "n_tex_quad_bytes", "n_textures")] +
                [(n, C.c_void_p) for n in LIGHTING_PROBE_ARRAYS])


class TextureUpdate(C.Structure):
    _fields_ = [("texture", C.c_uint32), ("width", C.c_uint32), ("height", C.c_uint32), ("channels", C.c_uint32), ("pixels", C.c_void_p),
                ("flags", C.c_uint32)]


class SceneTextureUpdate(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("n_textures", C.c_uint32), ("textures", C.POINTER(TextureUpdate)), ("flags", C.c_uint32)]


class TexturesProbe(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("n_tex_u8", C.c_uint64), ("n_textures", C.c_uint64), ("tex_u8", C.c_void_p),
                ("textures", C.c_void_p)]


UPDATE_REBUILD_TOP = 1
UPDATE_REBUILD_TOP_DEVICE = 2
TLAS_LOCAL_LEAVES = 2048            # csrc/tlas_build.hpp kTlasLocalLeaves: the leaves a subtree of the device build holds at most
TEXELS_ON_DEVICE = 1
# the records of DeviceScene.lighting_records(): csrc/scene_types.hpp MaterialDev (flags: 1 thin, 2 alpha-tested, 4 emissive,
# 8 transparent), LightDev, EnvDev and TexDev (quad_offset in 16-byte units, 0xffffffff: no footprint records of its own)
MATERIAL_DEV_DTYPE = np.dtype([("base", np.float32, 3), ("transmission", np.float32), ("emission", np.float32, 3), ("metallic", np.float32),
                               ("ior", np.float32), ("roughness", np.float32), ("anisotropic", np.float32), ("clearcoat", np.float32),
                               ("clearcoat_roughness", np.float32), ("flags", np.uint32), ("volume_density", np.float32),
                               ("tex_base", np.int32), ("volume_color", np.float32, 3), ("tex_mr", np.int32),
                               ("tex_transmission", np.int32), ("tex_normal", np.int32), ("tex_clearcoat", np.int32),
                               ("tex_emission", np.int32), ("local_rot", np.float32, 9), ("inv_rot", np.float32, 9), ("pad", np.uint32, 2)])
LIGHT_DEV_DTYPE = np.dtype([("type", np.uint32), ("mesh", np.int32), ("tri", np.uint32), ("two_sided", np.uint32),
                            ("emission", np.float32, 3), ("area", np.float32), ("power", np.float32), ("radius", np.float32),
                            ("texture", np.int32), ("env", np.uint32), ("fwd", np.float32, 16), ("inv", np.float32, 16)])
ENV_DEV_DTYPE = np.dtype([("w", np.uint32), ("h", np.uint32), ("func_offset", np.uint32), ("cdf_offset", np.uint32),
                          ("row_int_offset", np.uint32), ("marg_cdf_offset", np.uint32), ("marg_integral", np.float32),
                          ("surface_area", np.float32), ("guide_offset", np.uint32), ("guide_kw", np.uint32), ("guide_kh", np.uint32),
                          ("pair_offset", np.uint32)])
TEX_DEV_DTYPE = np.dtype([("offset", np.uint32), ("width", np.uint32), ("height", np.uint32), ("channels", np.uint32), ("type", np.uint32),
                          ("is_float", np.uint32), ("quad_offset", np.uint32), ("quad_stride", np.uint32)])
assert (MATERIAL_DEV_DTYPE.itemsize, LIGHT_DEV_DTYPE.itemsize, ENV_DEV_DTYPE.itemsize, TEX_DEV_DTYPE.itemsize) == (176, 176, 48, 32)
# the records of DeviceScene.mesh_records(): csrc/scene_types.hpp MeshDev, BvhNode (link: index | alpha bit 26 | span << 27),
# LeafTri (mat_flags: MAT_* of the material; a leaf's first record: | span << 8) and ShadeTri
MESH_DTYPE = np.dtype([("node_offset", np.uint32), ("leaf_offset", np.uint32), ("tri_offset", np.uint32), ("vert_offset", np.uint32),
                       ("n_tris", np.uint32), ("n_verts", np.uint32), ("n_nodes", np.uint32), ("has_alpha", np.uint32),
                       ("pad", np.uint32, 8)])
BVH_NODE_DTYPE = np.dtype([("bmin", np.float32, 3), ("bmax", np.float32, 3), ("link", np.uint32), ("span", np.uint32)])
LEAF_TRI_DTYPE = np.dtype([("p0", np.float32, 3), ("tri", np.uint32), ("e1", np.float32, 3), ("mat_flags", np.uint32),
                           ("e2", np.float32, 3), ("material", np.uint32)])
SHADE_TRI_DTYPE = np.dtype([("n", np.float32, (3, 3)), ("t", np.float32, (3, 4)), ("uv", np.float32, (3, 2)), ("material", np.uint32),
                            ("light", np.int32), ("pad", np.uint32, 3)])
# the records of DeviceScene.scene_graph(): csrc/scene_types.hpp NodeDev and TlasNode
NODE_DTYPE = np.dtype([("fwd", np.float32, 16), ("inv", np.float32, 16), ("bmin", np.float32, 3), ("mesh", np.int32),
                       ("bmax", np.float32, 3), ("skip", np.uint32), ("parent", np.int32), ("depth", np.uint32),
                       ("flags", np.uint32), ("pad", np.uint32)])
TLAS_DTYPE = np.dtype([("lo", np.float32, 3), ("a", np.uint32), ("hi", np.float32, 3), ("b", np.uint32)])
NODE_WORLD_DTYPE = np.dtype([("lo", np.float32, 3), ("lo_w", np.uint32), ("hi", np.float32, 3), ("hi_w", np.uint32)])


class SceneDesc(C.Structure):
    _fields_ = [("n_textures", C.c_uint32), ("n_materials", C.c_uint32), ("n_meshes", C.c_uint32),
                ("n_nodes", C.c_uint32), ("n_lights", C.c_uint32),
                ("textures", C.POINTER(TextureDesc)), ("materials", C.POINTER(MaterialDesc)),
                ("meshes", C.POINTER(MeshDesc)), ("nodes", C.POINTER(NodeDesc)),
                ("lights", C.POINTER(LightDesc))]


class CameraDesc(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("focal_length", C.c_float),
                ("f_number", C.c_float), ("sensor", C.c_float * 2), ("position", C.c_float * 3),
                ("target", C.c_float * 3), ("up", C.c_float * 3), ("exposure", C.c_float),
                ("aperture_sides", C.c_uint32)]


class RenderParams(C.Structure):
    _fields_ = [("samples", C.c_uint32), ("first_wave_samples", C.c_uint32),
                ("max_wave_samples", C.c_uint32), ("tile_size", C.c_uint32), ("max_depth", C.c_uint32),
                ("background", C.c_float * 3), ("rank", C.c_uint32), ("world_size", C.c_uint32),
                ("flags", C.c_uint32), ("start_sample", C.c_uint32), ("stop_sample", C.c_uint32),
                ("estimator", C.c_uint32), ("shard_tile", C.c_uint32), ("max_batch_paths", C.c_uint32),
                ("pool_paths", C.c_uint32)]


def _plain(v):
    return list(v) if hasattr(v, "__len__") else v


class Stats(C.Structure):
    _fields_ = [("samples", C.c_uint64), ("rays", C.c_uint64), ("ms_total", C.c_double),
                ("ms_device", C.c_double), ("ms_traverse", C.c_double), ("traversals", C.c_uint64),
                ("box_tests", C.c_uint64), ("tri_tests", C.c_uint64), ("waves", C.c_uint32),
                ("launches_traverse", C.c_uint32), ("shaded_hits", C.c_uint64),
                ("ms_extend", C.c_double), ("ms_shade", C.c_double), ("ms_connect", C.c_double),
                ("ms_gmon", C.c_double), ("launches_extend", C.c_uint32), ("launches_connect", C.c_uint32),
                ("ms_extend_lean", C.c_double), ("lean_traversals", C.c_uint64), ("lean_box_tests", C.c_uint64),
                ("lean_tri_tests", C.c_uint64), ("launches_extend_lean", C.c_uint32), ("reserved0", C.c_uint32),
                ("ms_shade_kernel", C.c_double), ("ms_shadow_lean", C.c_double),
                ("launches_shade_kernel", C.c_uint32), ("launches_shadow_lean", C.c_uint32),
                ("shadow_lean_traversals", C.c_uint64), ("shadow_lean_box_tests", C.c_uint64),
                ("shadow_lean_tri_tests", C.c_uint64), ("shade_entries", C.c_uint64),
                ("texture_tap_bytes", C.c_uint64), ("pipeline_flags", C.c_uint32), ("reserved1", C.c_uint32),
                ("retry_extend_traversals", C.c_uint64), ("retry_shadow_traversals", C.c_uint64),
                ("wide_extend_nodes", C.c_uint64), ("wide_extend_tris", C.c_uint64),
                ("wide_shadow_nodes", C.c_uint64), ("wide_shadow_tris", C.c_uint64),
                ("wide_extend_handed", C.c_uint64 * 4), ("wide_shadow_handed", C.c_uint64 * 4),
                ("paths_at_bounce", C.c_uint64 * 16)]

    def asdict(self):
        return {k: _plain(getattr(self, k)) for k, _ in self._fields_}


# YartRenderParams.estimator (core/estimator.hpp; the reference picks one at compile time, integrator.cpp:17-18)
ESTIMATOR_GMON, ESTIMATOR_MEAN, ESTIMATOR_MON, ESTIMATOR_GMONB = 0, 1, 2, 3


YART_ABORTED = 1
# int on_wave(void* user, const YartStats* wave_stats, wave, wave_samples, samples_taken, total_samples)
WAVE_CALLBACK = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32)


class TileInfo(C.Structure):
    """YartTileInfo (include/yart_hip.h): Renderer::TileData of a finished pixel block (renderer.hpp:40-50)."""
    _fields_ = [("x", C.c_uint32), ("y", C.c_uint32), ("width", C.c_uint32), ("height", C.c_uint32),
                ("index", C.c_uint32), ("total", C.c_uint32), ("wave", C.c_uint32), ("wave_samples", C.c_uint32),
                ("samples_taken", C.c_uint32), ("total_samples", C.c_uint32), ("rays", C.c_uint64), ("ms", C.c_double)]

    def asdict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


# int on_tile(void* user, const YartTileInfo* tile)
TILE_CALLBACK = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(TileInfo))


class AovBuffers(C.Structure):
    """YartAovBuffers (include/yart_hip.h): the first-hit feature buffers a render fills next to the frame."""
    _fields_ = [("struct_size", C.c_uint32), ("mask", C.c_uint32),
                ("albedo", C.c_void_p), ("normal", C.c_void_p), ("position", C.c_void_p), ("depth", C.c_void_p),
                ("coverage", C.c_void_p), ("ids", C.c_void_p), ("rays", C.c_void_p)]


# name -> (YART_AOV_* bit, values per pixel, dtype)
AOVS = {"albedo": (1, 3, np.float32), "normal": (2, 3, np.float32), "position": (4, 3, np.float32), "depth": (8, 1, np.float32),
        "coverage": (16, 1, np.float32), "ids": (32, 4, np.int32), "rays": (64, 1, np.uint32)}
AOV_ALL = tuple(AOVS)


def reduce_aov_samples(values, hit, samples=None):
    """The definition of an averaged feature buffer, in numpy: ``values`` [..., S, C] per-sample values, ``hit`` [..., S]
    bool. The float32 sum over the hitting samples in ascending sample order (misses contribute nothing), then one
    division by float32(samples). Returns [..., C] float32."""
    values = np.asarray(values, np.float32)
    hit = np.asarray(hit, bool)
    n = values.shape[-2] if samples is None else samples
    acc = np.zeros(values.shape[:-2] + values.shape[-1:], np.float32)
    for s in range(values.shape[-2]):
        acc = np.where(hit[..., s, None], acc + values[..., s, :], acc).astype(np.float32)
    return (acc / np.float32(n)).astype(np.float32)


def reduce_aov_coverage(hit, samples=None):
    """coverage: hitting samples (an integer count) / samples, one float32 division."""
    hit = np.asarray(hit, bool)
    n = hit.shape[-1] if samples is None else samples
    return (hit.sum(axis=-1).astype(np.float32) / np.float32(n)).astype(np.float32)


class MomentBuffers(C.Structure):
    """YartMomentBuffers (include/yart_hip.h): the per-pixel sample moments a render fills next to the frame."""
    _fields_ = [("struct_size", C.c_uint32), ("mask", C.c_uint32),
                ("mean", C.c_void_p), ("variance", C.c_void_p), ("count", C.c_void_p)]


# name -> (YART_MOMENT_* bit, values per pixel, dtype)
MOMENTS = {"mean": (1, 3, np.float32), "variance": (2, 1, np.float32), "count": (4, 1, np.uint32)}
MOMENT_ALL = tuple(MOMENTS)


class DenoiseVarParams(C.Structure):
    """YartDenoiseVarParams (include/yart_hip.h): the knobs of the variance-guided à-trous filter."""
    _fields_ = [("struct_size", C.c_uint32), ("iterations", C.c_uint32), ("sigma_luma", C.c_float),
                ("sigma_normal", C.c_float), ("sigma_depth", C.c_float), ("flags", C.c_uint32)]


def make_denoise_var_params(iterations=DEFAULT_VAR_ITERATIONS, sigma_luma=DEFAULT_VAR_SIGMA_LUMA,
                            sigma_normal=DEFAULT_VAR_SIGMA_NORMAL, sigma_depth=DEFAULT_VAR_SIGMA_DEPTH,
                            demodulate=False) -> DenoiseVarParams:
    return DenoiseVarParams(C.sizeof(DenoiseVarParams), int(iterations), float(sigma_luma), float(sigma_normal),
                            float(sigma_depth), FLAG_DEMODULATE if demodulate else 0)


class TemporalParams(C.Structure):
    """YartTemporalParams (include/yart_hip.h): the knobs of the temporal accumulator."""
    _fields_ = [("struct_size", C.c_uint32), ("alpha_min", C.c_float), ("max_history", C.c_uint32),
                ("normal_cos_min", C.c_float), ("plane_tolerance", C.c_float), ("flags", C.c_uint32)]


class TemporalMomentParams(C.Structure):
    """YartTemporalMomentParams (include/yart_hip.h): the knobs of the temporal accumulator's moments form."""
    _fields_ = [("struct_size", C.c_uint32), ("alpha_min", C.c_float), ("max_history", C.c_uint32),
                ("normal_cos_min", C.c_float), ("plane_tolerance", C.c_float), ("min_moment_history", C.c_uint32),
                ("flags", C.c_uint32)]


class TemporalMotion(C.Structure):
    """YartTemporalMotion (include/yart_hip.h): the per-node motion records for the next accumulate call."""
    _fields_ = [("struct_size", C.c_uint32), ("n_nodes", C.c_uint32), ("records", C.c_void_p)]


class TemporalPixelMotion(C.Structure):
    """YartTemporalPixelMotion (include/yart_hip.h): the per-pixel motion records for the next accumulate call."""
    _fields_ = [("struct_size", C.c_uint32), ("records", C.c_void_p)]


class TemporalClip(C.Structure):
    """YartTemporalClip (include/yart_hip.h): the clip of the history to the frame's neighbourhood, a setting of the handle."""
    _fields_ = [("struct_size", C.c_uint32), ("radius", C.c_uint32), ("gamma", C.c_float)]


class ExposureParams(C.Structure):
    """YartExposureParams (include/yart_hip.h): the knobs of the auto-exposure's meter call."""
    _fields_ = [("struct_size", C.c_uint32), ("ev_min", C.c_float), ("ev_max", C.c_float), ("trim_low", C.c_float),
                ("trim_high", C.c_float), ("key", C.c_float), ("compensation_ev", C.c_float), ("gain_ev_min", C.c_float),
                ("gain_ev_max", C.c_float), ("speed_up", C.c_float), ("speed_down", C.c_float),
                ("x0", C.c_uint32), ("y0", C.c_uint32), ("x1", C.c_uint32), ("y1", C.c_uint32)]


class ExposureStateRecord(C.Structure):
    """YartExposureState (include/yart_hip.h): what yart_hip_exposure_get reports."""
    _fields_ = [("struct_size", C.c_uint32), ("cur_ev", C.c_float), ("target_ev", C.c_float), ("mean_ev", C.c_float),
                ("gain", C.c_float), ("n_counted", C.c_uint32), ("n_ignored", C.c_uint32), ("frames", C.c_uint32),
                ("flags", C.c_uint32)]


def make_exposure_params(**params) -> ExposureParams:
    """``yart_amd.exposure.params_of``'s names (``window``: (x0, y0, x1, y1) or None for the whole frame)."""
    p = exposure_params_of(**params)
    win = p["window"] or (0, 0, 0, 0)
    return ExposureParams(C.sizeof(ExposureParams), *(float(p[k]) for k in ("ev_min", "ev_max", "trim_low", "trim_high", "key",
                                                                            "compensation_ev", "gain_ev_min", "gain_ev_max",
                                                                            "speed_up", "speed_down")), *(int(v) for v in win))


PIXEL_MOTION_AOVS = ("position", "normal", "coverage", "ids")      # what yart_hip_scene_pixel_motion_* reads
FLAG_TEMPORAL_DEMODULATE = 1
TEMPORAL_AOVS = ("position", "normal", "depth", "coverage", "ids")     # + "albedo" when demodulating


def make_temporal_params(alpha_min=DEFAULT_ALPHA_MIN, max_history=DEFAULT_MAX_HISTORY, normal_cos_min=DEFAULT_NORMAL_COS_MIN,
                         plane_tolerance=DEFAULT_PLANE_TOLERANCE, demodulate=False) -> TemporalParams:
    return TemporalParams(C.sizeof(TemporalParams), float(alpha_min), int(max_history), float(normal_cos_min),
                          float(plane_tolerance), FLAG_TEMPORAL_DEMODULATE if demodulate else 0)


def make_temporal_moment_params(alpha_min=DEFAULT_ALPHA_MIN, max_history=DEFAULT_MAX_HISTORY, normal_cos_min=DEFAULT_NORMAL_COS_MIN,
                                plane_tolerance=DEFAULT_PLANE_TOLERANCE, min_moment_history=DEFAULT_MIN_MOMENT_HISTORY,
                                demodulate=False) -> TemporalMomentParams:
    return TemporalMomentParams(C.sizeof(TemporalMomentParams), float(alpha_min), int(max_history), float(normal_cos_min),
                                float(plane_tolerance), int(min_moment_history), FLAG_TEMPORAL_DEMODULATE if demodulate else 0)


class DenoiseParams(C.Structure):
    """YartDenoiseParams (include/yart_hip.h): the knobs of the à-trous filter."""
    _fields_ = [("struct_size", C.c_uint32), ("iterations", C.c_uint32), ("sigma_color", C.c_float),
                ("sigma_normal", C.c_float), ("sigma_depth", C.c_float), ("flags", C.c_uint32)]


def make_denoise_params(iterations=DEFAULT_ITERATIONS, sigma_color=DEFAULT_SIGMA_COLOR, sigma_normal=DEFAULT_SIGMA_NORMAL,
                        sigma_depth=DEFAULT_SIGMA_DEPTH, demodulate=False) -> DenoiseParams:
    return DenoiseParams(C.sizeof(DenoiseParams), int(iterations), float(sigma_color), float(sigma_normal), float(sigma_depth),
                         FLAG_DEMODULATE if demodulate else 0)


class ImportOptions(C.Structure):
    """YartImportOptions (include/yart_hip.h): the environment the frontend adds after gltf::load."""
    _fields_ = [("env_hdr_path", C.c_char_p), ("env_radius", C.c_float), ("uniform_env", C.c_uint32),
                ("uniform_emission", C.c_float * 3), ("reserved", C.c_uint32 * 4)]


def import_options(env_hdr=None, env_radius=100.0, uniform_env=None) -> ImportOptions:
    o = ImportOptions()
    o.env_hdr_path = os.fspath(env_hdr).encode() if env_hdr else None
    o.env_radius = float(env_radius)
    if uniform_env is not None:
        o.uniform_env = 1
        o.uniform_emission = _f(uniform_env, 3)
    return o


def is_gltf_path(path) -> bool:
    return os.fspath(path).lower().endswith((".glb", ".gltf"))


def gltf_to_yscn(gltf_path, yscn_path, env_hdr=None, env_radius=100.0, uniform_env=None):
    """Import a glTF 2.0 / GLB asset the way the reference's loader does (src/gltf/gltf.cpp:319-358, plus the
    environment of src/main.cpp:80-86) and write it as a ``.yscn`` container. Host only: needs no device."""
    L = lib()
    o = import_options(env_hdr, env_radius, uniform_env)
    _check(L.yart_hip_gltf_to_yscn(os.fspath(gltf_path).encode(), C.byref(o), os.fspath(yscn_path).encode()), L)


EXPORTS = ["yart_hip_abi_version", "yart_hip_device_count", "yart_hip_last_error",
           "yart_hip_scene_create", "yart_hip_scene_load", "yart_hip_scene_destroy",
           "yart_hip_scene_load_gltf", "yart_hip_gltf_to_yscn",
           "yart_hip_render", "yart_hip_render_waves", "yart_hip_render_tiles", "yart_hip_render_device", "yart_hip_probe_samples",
           "yart_hip_probe_hits", "yart_hip_probe_sampler", "yart_hip_bvh_info", "yart_hip_bvh_copy", "yart_hip_scene_create_flags", "yart_hip_bvh_build_device", "yart_hip_bvh_build_host",
           "yart_hip_tlas_build_device", "yart_hip_tlas_build_host", "yart_hip_tlas_build_launches", "yart_hip_debug_counters", "yart_hip_debug_shade_regions",
           "yart_hip_tonemap_agx", "yart_hip_encode_rgb8", "yart_hip_tonemap_host",
           "yart_hip_multi_create", "yart_hip_multi_load", "yart_hip_multi_destroy", "yart_hip_multi_device_count", "yart_hip_multi_failed_devices",
           "yart_hip_multi_render", "yart_hip_multi_render_tiles", "yart_hip_multi_rccl_selftest",
           "yart_hip_render_aovs", "yart_hip_render_aovs_device", "yart_hip_probe_camera_rays",
           "yart_hip_probe_math", "yart_hip_probe_math_pairs",
           "yart_hip_denoise_atrous_device", "yart_hip_denoise_atrous_host",
           "yart_hip_render_moments", "yart_hip_render_moments_device", "yart_hip_probe_moments",
           "yart_hip_probe_estimator",
           "yart_hip_denoise_atrous_var_device", "yart_hip_denoise_atrous_var_host",
           "yart_hip_temporal_create", "yart_hip_temporal_destroy", "yart_hip_temporal_reset",
           "yart_hip_temporal_accumulate_device", "yart_hip_temporal_accumulate_host",
           "yart_hip_temporal_accumulate_moments_device", "yart_hip_temporal_accumulate_moments_host",
           "yart_hip_temporal_set_motion",
           "yart_hip_scene_update", "yart_hip_probe_scene_graph", "yart_hip_scene_update_graph",
           "yart_hip_scene_update_meshes", "yart_hip_probe_mesh",
           "yart_hip_scene_replace_meshes", "yart_hip_probe_geometry",
           "yart_hip_scene_update_lighting", "yart_hip_probe_lighting", "yart_hip_probe_texel_sum",
           "yart_hip_scene_update_textures", "yart_hip_probe_textures",
           "yart_hip_scene_keep_previous", "yart_hip_scene_pixel_motion_device", "yart_hip_scene_pixel_motion_host",
           "yart_hip_temporal_set_pixel_motion",
           "yart_hip_probe_rays",
           "yart_hip_temporal_set_clip",
           "yart_hip_probe_shading",
           "yart_hip_exposure_create", "yart_hip_exposure_destroy", "yart_hip_exposure_reset",
           "yart_hip_exposure_meter_device", "yart_hip_exposure_meter_host",
           "yart_hip_exposure_apply_device", "yart_hip_exposure_apply_host", "yart_hip_exposure_get",
           "yart_hip_debug_exposure_time"]

# ---------------------------------------------------------------------------
# The signature of every export of include/yart_hip.h: name -> (argtypes, restype), applied by lib(). An export without
# argtypes would take a Python int as a C int and cut a 64-bit pointer in half, so every name of EXPORTS has its entry.
# ---------------------------------------------------------------------------
def _sig(*argtypes, restype=C.c_int):
    return argtypes, restype


_P, _U32, _U64, _INT, _FLT = C.c_void_p, C.c_uint32, C.c_uint64, C.c_int, C.c_float
_U32_OUT, _HANDLE_OUT = C.POINTER(C.c_uint32), C.POINTER(C.c_void_p)
# the heads the families share
_RENDER = (_P, C.POINTER(CameraDesc), C.POINTER(RenderParams), _P)                      # scene / multi, camera, parameters, frame
_PROGRESSIVE = _RENDER + (C.POINTER(Stats), WAVE_CALLBACK)                                # ... statistics, on_wave
_MESH_ARRAYS = (_P, _U32, _P, _U32, _U32)                                                 # positions, n_verts, faces, face_stride, n_faces
_BVH_OUT = (_P, _P, _U32_OUT, C.POINTER(C.c_double))                                      # nodes, indices, n_nodes, milliseconds
_TLAS_BUILD = (_P, _P, _U32, _P, _U32_OUT, _U32_OUT)                                      # node_world, mesh, n_nodes, tlas, n_tlas, height
_IMAGE = (_P, _U32, _U32)                                                                 # pixels, width, height
_HANDLE_IMAGE = (_P,) + _IMAGE                                                            # exposure handle, pixels, width, height


def _update(desc):                  # yart_hip_scene_update*: scene, update, stream, statistics
    return _sig(_P, C.POINTER(desc), _P, C.POINTER(SceneUpdateStats))


def _denoise(n_inputs, params, *stream):      # frame (, variance), albedo, normal, depth, width, height, parameters, out (, stream)
    return _sig(*(_P,) * n_inputs, _U32, _U32, C.POINTER(params), _P, *stream)


def _accumulate(params, *stream):   # handle, camera, frame, variance, features, parameters, out, out variance, out length (, stream)
    return _sig(_P, C.POINTER(CameraDesc), _P, _P, C.POINTER(AovBuffers), C.POINTER(params), _P, _P, _P, *stream)


SIGNATURES = {
    "yart_hip_abi_version": _sig(),
    "yart_hip_device_count": _sig(),
    "yart_hip_last_error": _sig(restype=C.c_char_p),
    "yart_hip_scene_create": _sig(C.POINTER(SceneDesc), _INT, _HANDLE_OUT),
    "yart_hip_scene_create_flags": _sig(C.POINTER(SceneDesc), _INT, _U32, _HANDLE_OUT),
    "yart_hip_scene_load": _sig(C.c_char_p, _INT, _HANDLE_OUT),
    "yart_hip_scene_load_gltf": _sig(C.c_char_p, C.POINTER(ImportOptions), _INT, _HANDLE_OUT),
    "yart_hip_gltf_to_yscn": _sig(C.c_char_p, C.POINTER(ImportOptions), C.c_char_p),
    "yart_hip_scene_destroy": _sig(_P, restype=None),
    "yart_hip_render": _sig(*_RENDER, C.POINTER(Stats)),
    "yart_hip_render_waves": _sig(*_PROGRESSIVE, _P),
    "yart_hip_render_tiles": _sig(*_PROGRESSIVE, TILE_CALLBACK, _P),
    "yart_hip_render_device": _sig(*_RENDER, _P, C.POINTER(Stats)),
    "yart_hip_render_aovs": _sig(*_RENDER, C.POINTER(AovBuffers), C.POINTER(Stats)),
    "yart_hip_render_aovs_device": _sig(*_RENDER, C.POINTER(AovBuffers), _P, C.POINTER(Stats)),
    "yart_hip_render_moments": _sig(*_RENDER, C.POINTER(AovBuffers), C.POINTER(MomentBuffers), C.POINTER(Stats)),
    "yart_hip_render_moments_device": _sig(*_RENDER, C.POINTER(AovBuffers), C.POINTER(MomentBuffers), _P, C.POINTER(Stats)),
    "yart_hip_multi_create": _sig(C.POINTER(SceneDesc), C.POINTER(C.c_int), _U32, _HANDLE_OUT),
    "yart_hip_multi_load": _sig(C.c_char_p, C.POINTER(ImportOptions), C.POINTER(C.c_int), _U32, _HANDLE_OUT),
    "yart_hip_multi_destroy": _sig(_P, restype=None),
    "yart_hip_multi_device_count": _sig(_P),
    "yart_hip_multi_failed_devices": _sig(_P, _P, _U32),
    "yart_hip_multi_rccl_selftest": _sig(_INT, _U32),
    "yart_hip_multi_render": _sig(*_RENDER, C.POINTER(Stats)),
    "yart_hip_multi_render_tiles": _sig(*_PROGRESSIVE, TILE_CALLBACK, _P),
    "yart_hip_scene_update": _update(SceneUpdate),
    "yart_hip_scene_update_graph": _update(SceneGraphUpdate),
    "yart_hip_scene_update_meshes": _update(SceneMeshUpdate),
    "yart_hip_scene_replace_meshes": _update(SceneMeshReplace),
    "yart_hip_scene_update_lighting": _update(SceneLightingUpdate),
    "yart_hip_scene_update_textures": _update(SceneTextureUpdate),
    "yart_hip_scene_keep_previous": _sig(_P, _P),
    "yart_hip_scene_pixel_motion_device": _sig(_P, C.POINTER(AovBuffers), _U32, _U32, _P, _P),
    "yart_hip_scene_pixel_motion_host": _sig(_P, C.POINTER(AovBuffers), _U32, _U32, _P),
    "yart_hip_probe_samples": _sig(*_RENDER[:3], _U32, _P, _P, C.POINTER(C.c_uint64)),
    "yart_hip_probe_camera_rays": _sig(*_RENDER[:3], _U32, _P, _P),
    "yart_hip_probe_hits": _sig(_P, _U32, _P, _P),
    "yart_hip_probe_rays": _sig(_P, C.POINTER(RenderParams), _U32, _P, _INT, _P),
    "yart_hip_probe_shading": _sig(_P, _U32, _P, _U32, _P),
    "yart_hip_probe_sampler": _sig(_P, _U32, _U32, _U32, _P, _U32, _P, _INT, _P),
    "yart_hip_probe_math": _sig(_INT, _U32, _U64, _FLT, _P),
    "yart_hip_probe_math_pairs": _sig(_INT, _U64, _P, _P, _P),
    "yart_hip_probe_moments": _sig(_P, _U32, _U32, _P, _U32, _FLT, _P, _P, _P),
    "yart_hip_probe_estimator": _sig(_P, _U32, _U32, _INT, _FLT, _P, _U32, _U32, _FLT, _FLT, _P, _P),
    "yart_hip_probe_scene_graph": _sig(_P, _P, _P, _P, _U32_OUT),
    "yart_hip_probe_mesh": _sig(_P, _U32, *(_P,) * 7, _U32_OUT),
    "yart_hip_probe_geometry": _sig(_P, C.POINTER(GeometryProbe)),
    "yart_hip_probe_lighting": _sig(_P, C.POINTER(LightingProbe)),
    "yart_hip_probe_texel_sum": _sig(_P, _U64, _P),
    "yart_hip_probe_textures": _sig(_P, C.POINTER(TexturesProbe)),
    "yart_hip_debug_counters": _sig(_P, _P),
    "yart_hip_debug_shade_regions": _sig(_P),
    "yart_hip_bvh_info": _sig(_P, _U32, _U32_OUT, _U32_OUT),
    "yart_hip_bvh_copy": _sig(_P, _U32, _P, _P),
    "yart_hip_bvh_build_device": _sig(_INT, *_MESH_ARRAYS, *_BVH_OUT),
    "yart_hip_bvh_build_host": _sig(*_MESH_ARRAYS, _U32, *_BVH_OUT),
    "yart_hip_tlas_build_device": _sig(_INT, *_TLAS_BUILD),
    "yart_hip_tlas_build_host": _sig(*_TLAS_BUILD),
    "yart_hip_tlas_build_launches": _sig(_U32),
    "yart_hip_tonemap_agx": _sig(*_IMAGE, _INT, _P, _P),
    "yart_hip_encode_rgb8": _sig(*_IMAGE, _P, _P),
    "yart_hip_tonemap_host": _sig(*_IMAGE, _INT, _P, _P),
    "yart_hip_denoise_atrous_device": _denoise(4, DenoiseParams, _P),
    "yart_hip_denoise_atrous_host": _denoise(4, DenoiseParams),
    "yart_hip_denoise_atrous_var_device": _denoise(5, DenoiseVarParams, _P),
    "yart_hip_denoise_atrous_var_host": _denoise(5, DenoiseVarParams),
    "yart_hip_temporal_create": _sig(_U32, _U32, _INT, _HANDLE_OUT),
    "yart_hip_temporal_destroy": _sig(_P, restype=None),
    "yart_hip_temporal_reset": _sig(_P),
    "yart_hip_temporal_set_motion": _sig(_P, C.POINTER(TemporalMotion)),
    "yart_hip_temporal_set_pixel_motion": _sig(_P, C.POINTER(TemporalPixelMotion)),
    "yart_hip_temporal_set_clip": _sig(_P, C.POINTER(TemporalClip)),
    "yart_hip_temporal_accumulate_device": _accumulate(TemporalParams, _P),
    "yart_hip_temporal_accumulate_host": _accumulate(TemporalParams),
    "yart_hip_temporal_accumulate_moments_device": _accumulate(TemporalMomentParams, _P),
    "yart_hip_temporal_accumulate_moments_host": _accumulate(TemporalMomentParams),
    "yart_hip_exposure_create": _sig(_INT, _HANDLE_OUT),
    "yart_hip_exposure_destroy": _sig(_P, restype=None),
    "yart_hip_exposure_reset": _sig(_P),
    "yart_hip_exposure_meter_device": _sig(*_HANDLE_IMAGE, C.POINTER(ExposureParams), _FLT, _P),
    "yart_hip_exposure_meter_host": _sig(*_HANDLE_IMAGE, C.POINTER(ExposureParams), _FLT),
    "yart_hip_exposure_apply_device": _sig(*_HANDLE_IMAGE, _INT, _P, _P, _P),
    "yart_hip_exposure_apply_host": _sig(*_HANDLE_IMAGE, _INT, _P, _P),
    "yart_hip_exposure_get": _sig(_P, C.POINTER(ExposureStateRecord), _P),
    "yart_hip_debug_exposure_time": _sig(*_HANDLE_IMAGE, C.POINTER(ExposureParams), _INT, _U32, _P, _P, C.POINTER(C.c_float)),
}
assert set(SIGNATURES) == set(EXPORTS)

LIB_COUNT_PATH = os.path.join(_HERE, "libyart_hip_count.so")   # instrumented twin (exact test counters)
_libs = {}


def lib(instrumented: bool = False):
    """Load libyart_hip.so (built by ``__graft_entry__.build()``); raises if absent.
    ``instrumented=True`` loads libyart_hip_count.so, the same code compiled with
    -DYART_COUNT_TRAVERSAL (exact box / triangle test counters; never timed)."""
    path = LIB_COUNT_PATH if instrumented else LIB_PATH
    if path not in _libs:
        if not os.path.exists(path):
            raise YartError(YART_E_NO_DEVICE, f"{path} not built (run __graft_entry__.build()); "
                                              "there is no CPU fallback")
        L = C.CDLL(path)
        if L.yart_hip_abi_version() != ABI_VERSION:
            raise YartError(YART_E_INVALID, f"{path} has ABI {L.yart_hip_abi_version()}, this module binds ABI {ABI_VERSION} "
                                            "(include/yart_hip.h: YART_HIP_ABI_VERSION); rebuild the library")
        for name, (argtypes, restype) in SIGNATURES.items():
            fn = getattr(L, name)
            fn.argtypes, fn.restype = argtypes, restype
        _libs[path] = L
    return _libs[path]


def _check(code, L):
    """``L``: the library whose entry returned ``code`` — the last error is per library (the instrumented twin has its own)."""
    if code != YART_OK:
        raise YartError(code, L.yart_hip_last_error().decode())


def _device_tensor(t, what, *, shape=None, numel=None, dtype=None, element_size=None, optional=False):
    """The device pointer of the torch tensor ``t`` after the check every ``_into`` call makes of it — on the device, contiguous
    and, where given, of that ``shape`` / ``numel`` / ``dtype`` / ``element_size`` —, ``what`` being the assertion's message.
    ``optional``: None gives None."""
    if t is None and optional:
        return None
    assert (t.is_cuda and t.is_contiguous() and (shape is None or tuple(t.shape) == tuple(shape)) and
            (numel is None or t.numel() == numel) and (dtype is None or t.dtype == dtype) and
            (element_size is None or t.element_size() == element_size)), what
    return C.c_void_p(t.data_ptr())


def _stream_of(stream, tensor=None):
    """A call's stream argument: the integer handle ``stream``; None: torch's current stream of ``tensor``'s device — or, without
    a tensor, the null stream, as 0 is."""
    if stream is None and tensor is not None:
        import torch
        stream = torch.cuda.current_stream(tensor.device).cuda_stream
    return C.c_void_p(stream) if stream else None


def _buffer_struct(cls, table, h, w, names=None, *, host=None, device=None, required=True):
    """One YartAovBuffers / YartMomentBuffers (``cls``; ``table``: AOVS / MOMENTS) of an h x w image -> (struct, {name: buffer}).
    The buffers of ``names`` come in one of three forms: neither ``host`` nor ``device``: new NumPy outputs, (h, w, channels) or
    (h, w) for one channel; ``host``: {name: array}, made contiguous in the table's dtype (the returned copies keep the pointers
    alive); ``device``: {name: torch tensor}. ``names`` None: every name of that mapping. ``required`` False: a name the mapping
    lacks, or holds None for, is left out; True: it is a KeyError."""
    source = host if host is not None else device
    st, bufs = cls(C.sizeof(cls)), {}
    for name in (source if names is None else names):
        bit, ch, dt = table[name]
        if source is None:
            a = np.empty((h, w, ch) if ch > 1 else (h, w), dt)
        else:
            a = source[name] if required else source.get(name)
            if a is None and not required:
                continue
        if device is not None:
            ptr = _device_tensor(a, name, numel=h * w * ch, element_size=np.dtype(dt).itemsize)
        else:
            a = np.ascontiguousarray(a, dt)
            assert a.size == h * w * ch, name
            ptr = a.ctypes.data_as(C.c_void_p)
        bufs[name] = a
        st.mask |= bit
        setattr(st, name, ptr)
    return st, bufs


def _render_call(p, rank=0, world_size=1, flags=0, accumulated=None, into=None):
    """What every render entry starts from -> (cam, head, st, frame): the CameraDesc, ``head`` = the (camera, parameters, frame)
    arguments of the C call, a Stats to fill, and the frame: a new (H, W, 4) float32 array holding ``accumulated`` (the frame of
    the samples before p["start_sample"]) if that is given — or ``into``, a device tensor of H*W*4 elements."""
    cam, rp = make_camera(p), make_params(p, rank, world_size, flags)
    if into is None:
        frame = np.empty((cam.height, cam.width, 4), np.float32)
        if accumulated is not None:
            frame[...] = accumulated
        ptr = frame.ctypes.data_as(C.c_void_p)
    else:
        frame, ptr = into, _device_tensor(into, "frame", numel=cam.width * cam.height * 4)
    return cam, (C.byref(cam), C.byref(rp), ptr), Stats(), frame


def _run_progressive(fn, L, handle, p, on_wave, on_tile=None, *, tiles=True, rays=True, **call):
    """A progressive render through ``fn``, a bound yart_hip_*render_waves (``tiles`` False: the entry takes no tile callback) or
    *render_tiles: ``on_wave(frame, info)`` / ``on_tile(frame, tile)`` behind trampolines (None: a null callback), ``info`` with
    the wave's ``rays`` if ``rays``; ``call``: ``_render_call``'s. An exception of a callback stops the render and is raised
    after the C call has returned. Returns (frame, stats, aborted)."""
    _cam, head, st, out = _render_call(p, **call)
    errors = []

    def trampoline(callback, info):
        def tr(_user, *args):
            try:
                return 1 if callback(out, info(*args)) else 0
            except BaseException as e:          # an exception must not unwind through the C frames
                errors.append(e)
                return 1
        return tr

    def wave_info(stats, wave, wave_samples, taken, total):
        info = dict(wave=wave, wave_samples=wave_samples, samples_taken=taken, total_samples=total)
        if rays:
            info["rays"] = int(C.cast(stats, C.POINTER(Stats)).contents.rays) if stats else 0
        return info
    wave_tr, tile_tr = trampoline(on_wave, wave_info), trampoline(on_tile, lambda tile: tile.contents.asdict())
    callbacks = [WAVE_CALLBACK(wave_tr) if on_wave else WAVE_CALLBACK()]
    if tiles:
        callbacks.append(TILE_CALLBACK(tile_tr) if on_tile else TILE_CALLBACK())
    rc = fn(handle, *head, C.byref(st), *callbacks, None)
    if errors:
        raise errors[0]
    if rc != YART_ABORTED:
        _check(rc, L)
    return out, st.asdict(), rc == YART_ABORTED


# enum YartMathFn (include/yart_hip.h): what yart_hip_probe_math[_pairs] evaluates
MATH_FNS = {"sinf": 0, "cosf": 1, "sinf2pi": 2, "cosf2pi": 3, "logf": 4, "expf": 5, "log2f": 6, "powf": 7, "div": 8, "sqrt": 9,
            "brev": 10}


def probe_math(fn, first_bits=None, count=None, y=0.0, a=None, b=None, out=None):
    """One math function of the device code (csrc/ymath.hpp, csrc/tonemap.hpp; ``fn`` a key of MATH_FNS) on device 0.
    Range form: ``first_bits`` and ``count`` — fn at every float whose bits are first_bits + i; ``y`` is powf's exponent.
    Pairs form: ``a`` (and ``b``) — arrays of float32 values or uint32 bit patterns. Returns the results as a uint32 array
    of bit patterns (``out``, if given: a C-contiguous uint32 / float32 array of that many elements, is filled and returned)."""
    L = lib()
    code = MATH_FNS[fn]

    def words(v):
        v = np.asarray(v)
        if v.dtype != np.uint32:
            v = v.astype(np.float32)
        return np.ascontiguousarray(v).reshape(-1)
    if a is None:
        n = int(count)
        res = np.empty(n, np.uint32) if out is None else out
        assert res.size == n and res.itemsize == 4 and res.flags.c_contiguous
        _check(L.yart_hip_probe_math(code, int(first_bits), n, float(y), res.ctypes.data_as(C.c_void_p)), L)
    else:
        wa = words(a)
        wb = None if b is None else words(b)
        assert wb is None or wb.size == wa.size
        res = np.empty(wa.size, np.uint32) if out is None else out
        assert res.size == wa.size and res.itemsize == 4 and res.flags.c_contiguous
        _check(L.yart_hip_probe_math_pairs(code, wa.size, wa.ctypes.data_as(C.c_void_p),
                                           None if wb is None else wb.ctypes.data_as(C.c_void_p), res.ctypes.data_as(C.c_void_p)), L)
    return res


def bvh_build(positions, faces, device=None, threads=0):
    """The reference's binned-SAH BVH of one mesh, built outside a scene: on HIP device ``device`` (csrc/bvh_build_device.inc)
    or, with ``device=None``, on the host (csrc/bvh_build.hpp, ``threads`` workers, 0 = all). Returns (nodes (n, 8) u32 —
    bounds as float bits, left|first, span —, indices (n_faces,) u32, milliseconds); both builds give the same bytes."""
    L = lib()
    pos = np.ascontiguousarray(positions, np.float32).reshape(-1, 3)
    f = np.ascontiguousarray(faces, np.uint32)
    f = f.reshape(len(f), -1)
    nodes = np.zeros((2 * len(f), 8), np.uint32)
    idx = np.zeros(len(f), np.uint32)
    n, ms = C.c_uint32(0), C.c_double(0)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    if device is None:
        _check(L.yart_hip_bvh_build_host(vp(pos), len(pos), vp(f), f.shape[1], len(f), threads, vp(nodes), vp(idx), C.byref(n), C.byref(ms)), L)
    else:
        _check(L.yart_hip_bvh_build_device(int(device), vp(pos), len(pos), vp(f), f.shape[1], len(f), vp(nodes), vp(idx), C.byref(n), C.byref(ms)), L)
    return nodes[:n.value].copy(), idx, ms.value


def tlas_build(node_world, mesh, device=0):
    """The top-level hierarchy of a node list, built outside a scene: on HIP device ``device`` (csrc/tlas_build_kernels.inc) or, with
    ``device=None``, on the host (host_scene.hpp::buildTopLevel). ``node_world``: (n, 8) float32, the nodes' padded world boxes as
    lo.xyz, -, hi.xyz, -; ``mesh``: (n,) int32, < 0 = not a mesh node. Returns (tlas as TLAS_DTYPE, height); both builds give the
    same bytes, and fewer than 64 nodes give no records."""
    L = lib()
    world = np.ascontiguousarray(node_world, np.float32).reshape(-1, 8)
    m = np.ascontiguousarray(mesh, np.int32).reshape(-1)
    if len(m) != len(world):
        raise YartError(YART_E_INVALID, "tlas_build: node_world and mesh differ in their node counts")
    tlas = np.zeros(max(2 * int((m >= 0).sum()) - 1, 1), TLAS_DTYPE)
    n, height = C.c_uint32(0), C.c_uint32(0)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    if device is None:
        _check(L.yart_hip_tlas_build_host(vp(world), vp(m), len(m), vp(tlas), C.byref(n), C.byref(height)), L)
    else:
        _check(L.yart_hip_tlas_build_device(int(device), vp(world), vp(m), len(m), vp(tlas), C.byref(n), C.byref(height)), L)
    return tlas[:n.value].copy(), height.value


def _top_flags(rebuild_top):
    """rebuild_top of update / update_meshes -> YART_UPDATE_* flags: False refit, True or "host" the host rebuild, "device" the device's"""
    if rebuild_top is False or rebuild_top is True:
        return UPDATE_REBUILD_TOP if rebuild_top else 0
    if isinstance(rebuild_top, str) and rebuild_top in ("host", "device"):
        return UPDATE_REBUILD_TOP if rebuild_top == "host" else UPDATE_REBUILD_TOP_DEVICE
    raise YartError(YART_E_INVALID, f"rebuild_top is {rebuild_top!r}: False, True, 'host' or 'device'")


def _f(arr, n):
    return (C.c_float * n)(*[float(v) for v in np.asarray(arr, np.float32).reshape(-1)[:n]])


def _light_descs(lights):
    """the LightDesc array of a :class:`yscn.Scene` light list (one unused element for an empty list)"""
    ld = (LightDesc * max(len(lights), 1))()
    for i, l in enumerate(lights):
        ld[i] = LightDesc(l.type, l.mesh, l.tri, int(l.two_sided), l.texture, l.radius, _f(l.emission, 3), _f(l.fwd, 16), _f(l.inv, 16))
    return ld


def make_camera(p: dict) -> CameraDesc:
    """``p`` uses the vocabulary of oracle/params.hpp / yart_amd.scenes."""
    c = CameraDesc()
    c.width, c.height = int(p["size"][0]), int(p["size"][1])
    c.focal_length = float(p.get("focal", 35.0)); c.f_number = float(p.get("fnumber", 0.0))
    c.sensor = _f(p.get("sensor", (36.0, 24.0)), 2)
    c.position = _f(p["eye"], 3); c.target = _f(p["target"], 3); c.up = _f(p.get("up", (0, 1, 0)), 3)
    c.exposure = float(p.get("exposure", 0.0)); c.aperture_sides = int(p.get("aperture_sides", 0))
    return c


def make_params(p: dict, rank=0, world_size=1, flags=0) -> RenderParams:
    r = RenderParams()
    r.samples = int(p["spp"])
    r.first_wave_samples = int(p.get("first_wave", p["spp"]))     # single wave, as main.cpp:97-99
    r.max_wave_samples = int(p.get("max_wave", p["spp"]))
    r.tile_size = int(p.get("tile", 64)); r.max_depth = int(p.get("depth", 30))
    r.background = _f(p.get("background", (0, 0, 0)), 3)
    r.rank, r.world_size, r.flags = int(rank), int(world_size), int(flags)
    r.start_sample, r.stop_sample = int(p.get("start_sample", 0)), int(p.get("stop_sample", 0))
    r.estimator = int(p.get("estimator", ESTIMATOR_GMON))
    r.shard_tile = int(p.get("shard_tile", 0))
    r.max_batch_paths = int(p.get("max_batch_paths", 0))
    r.pool_paths = int(p.get("pool_paths", 0))
    return r


def _motion_snapshot(nodes):
    """(parent, copy of fwd as binary32) per node: what yart_amd.temporal.node_motion needs of a node list, detached from it"""
    return [(int(n.parent), np.array(n.fwd, np.float32, copy=True)) for n in nodes]


def describe_scene(s: "yscn.Scene"):
    """A :class:`yscn.Scene` as the C ABI's YartSceneDesc -> (desc, keep): `keep` owns every array the descriptor points into
    and must outlive the calls that read `desc` (yart_hip_scene_create copies what it needs)."""
    keep = []
    return DeviceScene._describe_into(s, keep), keep


class DeviceScene:
    """Owns a ``YartScene*`` (device-resident flattened scene + BVHs)."""

    def __init__(self, scene, device: int = -1, instrumented: bool = False, env_hdr=None, env_radius=100.0,
                 uniform_env=None, host_bvh: bool = False):
        """scene: a :class:`yscn.Scene`, the path of a ``.yscn`` container, or the path of a ``.glb`` / ``.gltf``
        asset (then env_hdr / env_radius / uniform_env give the environment light, as main.cpp:80-86)."""
        self._h = C.c_void_p()
        self._keep = []
        self._L = lib(instrumented)
        # what the scene last held, where it is known: (parent, copy of fwd) per node — a snapshot, so that a caller who moves the
        # nodes of their own yscn.Scene in place and hands them to update(motion=True) is compared with what was, not with itself
        self._nodes, self._n_nodes = None, None
        self.last_update = None                     # statistics of the last update(): dict(launches, ms_total, ms_device)
        if isinstance(scene, (str, os.PathLike)) and is_gltf_path(scene):
            o = import_options(env_hdr, env_radius, uniform_env)
            _check(self._L.yart_hip_scene_load_gltf(os.fspath(scene).encode(), C.byref(o), device, C.byref(self._h)),
                   self._L)
        elif isinstance(scene, (str, os.PathLike)):
            _check(self._L.yart_hip_scene_load(os.fspath(scene).encode(), device, C.byref(self._h)), self._L)
        else:
            desc = self._describe(scene)
            self._nodes, self._n_nodes = _motion_snapshot(scene.nodes), len(scene.nodes)
            if host_bvh:      # YART_SCENE_HOST_BVH: the meshes' BVHs from the host builder instead of the device build (same bytes)
                _check(self._L.yart_hip_scene_create_flags(C.byref(desc), device, 2, C.byref(self._h)), self._L)
            else:
                _check(self._L.yart_hip_scene_create(C.byref(desc), device, C.byref(self._h)), self._L)
        self._keep = []     # the library copies everything it needs

    def _describe(self, s: yscn.Scene) -> SceneDesc:
        return self._describe_into(s, self._keep)

    @staticmethod
    def _describe_into(s: yscn.Scene, keep) -> SceneDesc:

        def ptr(a, dtype):
            a = np.ascontiguousarray(a, dtype=dtype); keep.append(a)
            return a.ctypes.data_as(C.c_void_p)
        tex = (TextureDesc * max(len(s.textures), 1))()
        for i, t in enumerate(s.textures):
            tex[i] = TextureDesc(t.width, t.height, t.channels, int(t.is_float), t.type,
                                 ptr(t.data, np.float32 if t.is_float else np.uint8))
        mats = (MaterialDesc * max(len(s.materials), 1))()
        for i, m in enumerate(s.materials):
            C.memmove(C.byref(mats[i]), m.pack(), C.sizeof(MaterialDesc))
        meshes = (MeshDesc * max(len(s.meshes), 1))()
        for i, m in enumerate(s.meshes):
            meshes[i] = MeshDesc(len(m.positions), len(m.faces), ptr(m.positions, np.float32),
                                 ptr(m.normals, np.float32), ptr(m.tangents, np.float32),
                                 ptr(m.uvs, np.float32), ptr(m.faces, np.uint32), ptr(m.face_light, np.int32))
        nodes = (NodeDesc * len(s.nodes))()
        for i, n in enumerate(s.nodes):
            nodes[i] = NodeDesc(n.parent, n.mesh, _f(n.fwd, 16), _f(n.inv, 16))
        lights = _light_descs(s.lights)
        keep += [tex, mats, meshes, nodes, lights]
        return SceneDesc(len(s.textures), len(s.materials), len(s.meshes), len(s.nodes), len(s.lights),
                         tex, mats, meshes, nodes, lights)

    # -- animation ----------------------------------------------------------------
    def _update(self, entry, up, stream):
        """one of the yart_hip_scene_update* entries on this scene; its statistics into ``self.last_update``"""
        st = SceneUpdateStats(C.sizeof(SceneUpdateStats))
        _check(getattr(self._L, entry)(self._h, C.byref(up), stream, C.byref(st)), self._L)
        self.last_update = dict(launches=st.launches, ms_total=st.ms_total, ms_device=st.ms_device)

    def _probe(self, entry, pr, shape):
        """a probe entry's two calls: the first fills ``pr``'s sizes, ``shape()`` -> {field: (size, dtype)}, the second fills the arrays"""
        _check(getattr(self._L, entry)(self._h, C.byref(pr)), self._L)
        out = {name: np.zeros(int(n), dt) for name, (n, dt) in shape().items()}
        for name, a in out.items():
            setattr(pr, name, a.ctypes.data_as(C.c_void_p) if len(a) else None)
        _check(getattr(self._L, entry)(self._h, C.byref(pr)), self._L)
        return out

    def update(self, nodes, lights=None, rebuild_top=False, motion=False, stream=None):
        """yart_hip_scene_update: new transforms for the scene in place. ``nodes`` / ``lights``: the node / light lists of a
        :class:`yscn.Scene` — parent and mesh, and every light field but fwd / inv, as at create; ``lights=None`` leaves the lights
        untouched. ``rebuild_top``: rebuild the top-level hierarchy instead of refitting its boxes — True or "host" on the host,
        "device" on the device on the update's stream (the same bytes; anything else raises). With ``motion=True`` returns
        ``yart_amd.temporal.node_motion(the node list the scene held before, nodes)``. The call's statistics are in
        ``self.last_update``."""
        nodes = list(nodes)
        nd = (NodeDesc * max(len(nodes), 1))()
        for i, n in enumerate(nodes):
            nd[i] = NodeDesc(n.parent, n.mesh, _f(n.fwd, 16), _f(n.inv, 16))
        lights = list(lights) if lights is not None else []
        ld = _light_descs(lights)
        up = SceneUpdate(C.sizeof(SceneUpdate), len(nodes), nd, len(lights), ld if lights else None, _top_flags(rebuild_top))
        if motion and self._nodes is None:
            raise YartError(YART_E_INVALID, "update(motion=True): the scene was loaded from a file, its previous node list is not known")
        self._update("yart_hip_scene_update", up, stream)
        previous, self._nodes, self._n_nodes = self._nodes, _motion_snapshot(nodes), len(nodes)
        if motion:
            from . import temporal
            return temporal.node_motion(previous, self._nodes)
        return None

    def update_graph(self, nodes, lights=None, rebuild_top="device", stream=None):
        """yart_hip_scene_update_graph: a new node list for the scene in place — nodes added, removed, hidden (``mesh = -1``),
        re-meshed or re-parented. ``nodes``: the whole new list of a :class:`yscn.Scene`, in pre-order; ``lights``: as for
        :meth:`update` (None: untouched). ``rebuild_top``: where the top-level hierarchy is built — "device" (on the update's
        stream) or "host"; there is no refit, the leaf set changed. Discards the frame :meth:`keep_previous` kept. The call's
        statistics are in ``self.last_update``."""
        if rebuild_top not in ("device", "host"):
            raise YartError(YART_E_INVALID, f"update_graph: rebuild_top is {rebuild_top!r}: 'device' or 'host'")
        nodes = list(nodes)
        nd = (NodeDesc * max(len(nodes), 1))()
        for i, n in enumerate(nodes):
            nd[i] = NodeDesc(n.parent, n.mesh, _f(n.fwd, 16), _f(n.inv, 16))
        lights = list(lights) if lights is not None else []
        ld = _light_descs(lights)
        up = SceneGraphUpdate(C.sizeof(SceneGraphUpdate), len(nodes), nd, len(lights), ld if lights else None, _top_flags(rebuild_top))
        self._update("yart_hip_scene_update_graph", up, stream)
        self._nodes, self._n_nodes = _motion_snapshot(nodes), len(nodes)

    def update_meshes(self, meshes, rebuild_top=False, stream=None):
        """yart_hip_scene_update_meshes: new vertices for meshes of the scene in place. ``meshes``: {mesh index: positions} or
        {mesh index: (positions, normals, tangents)} with (n, 3) / (n, 3) / (n, 4) arrays for the mesh's n vertices; normals /
        tangents may be None or left out: kept. Faces, uvs, materials and the node list stay. ``rebuild_top``: rebuild the top-level
        hierarchy instead of refitting its boxes, as for :meth:`update`. The call's statistics are in ``self.last_update``."""
        keep, md = [], (MeshUpdate * max(len(meshes), 1))()
        for k, (mesh, arrays) in enumerate(meshes.items()):
            if isinstance(arrays, np.ndarray) or not isinstance(arrays, (tuple, list)):
                arrays = (arrays,)
            arrays = tuple(arrays) + (None,) * (3 - len(arrays))
            ptrs, n = [], None
            for a, width in zip(arrays, (3, 3, 4)):
                if a is None:
                    ptrs.append(None)
                    continue
                a = np.ascontiguousarray(a, np.float32).reshape(-1, width)
                if n is not None and len(a) != n:
                    raise YartError(YART_E_INVALID, f"update_meshes: mesh {mesh}: the arrays differ in their vertex counts")
                n = len(a)
                keep.append(a)
                ptrs.append(a.ctypes.data_as(C.c_void_p))
            n = n or 0
            md[k] = MeshUpdate(int(mesh), n, ptrs[0], ptrs[1], ptrs[2])
        up = SceneMeshUpdate(C.sizeof(SceneMeshUpdate), len(meshes), md, _top_flags(rebuild_top))
        self._update("yart_hip_scene_update_meshes", up, stream)

    def replace_meshes(self, meshes, rebuild_top=False, stream=None):
        """yart_hip_scene_replace_meshes: whole new meshes for the scene in place — faces, vertex counts, uvs and per-face materials
        may all differ from the mesh's. ``meshes``: {mesh index: a :class:`yscn.Mesh`, or (positions, normals, tangents, uvs, faces)}
        with (n, 3) / (n, 3) / (n, 4) / (n, 2) float arrays and an (m, 4) unsigned array of i0, i1, i2, material. A mesh with lights
        is refused. ``rebuild_top``: as for :meth:`update_meshes`. Discards the frame :meth:`keep_previous` kept. The call's
        statistics are in ``self.last_update``."""
        keep, md = [], (MeshReplace * max(len(meshes), 1))()
        for k, (mesh, m) in enumerate(meshes.items()):
            light = None
            if not isinstance(m, (tuple, list)):
                light = getattr(m, "face_light", None)
                m = (m.positions, m.normals, m.tangents, m.uvs, m.faces)
            if len(m) != 5:
                raise YartError(YART_E_INVALID, f"replace_meshes: mesh {mesh}: not a mesh and not (positions, normals, tangents, uvs, faces)")
            arrays = [np.ascontiguousarray(a, np.float32).reshape(-1, w) for a, w in zip(m[:4], (3, 3, 4, 2))]
            faces = np.ascontiguousarray(m[4], np.uint32).reshape(-1, 4)
            if len({len(a) for a in arrays}) != 1:
                raise YartError(YART_E_INVALID, f"replace_meshes: mesh {mesh}: the arrays differ in their vertex counts")
            if light is not None:
                light = np.ascontiguousarray(light, np.int32).reshape(-1)
                if len(light) != len(faces):
                    raise YartError(YART_E_INVALID, f"replace_meshes: mesh {mesh}: face_light and faces differ in their counts")
            keep += arrays + [faces, light]
            vp = lambda a: a.ctypes.data_as(C.c_void_p)
            md[k] = MeshReplace(int(mesh), MeshDesc(len(arrays[0]), len(faces), *(vp(a) for a in arrays), vp(faces),
                                                    vp(light) if light is not None else None))
        up = SceneMeshReplace(C.sizeof(SceneMeshReplace), len(meshes), md, _top_flags(rebuild_top))
        self._update("yart_hip_scene_replace_meshes", up, stream)

    def geometry(self):
        """yart_hip_probe_geometry: the pools ``replace_meshes`` repacks, read back whole from the device: dict(bvh_nodes:
        BVH_NODE_DTYPE (the zero pad records and the two tail records included), leaf_tris: LEAF_TRI_DTYPE, shade_tris:
        SHADE_TRI_DTYPE, tri_verts: (n, 4) uint32, tri_light: int32, vpos / vnormal / vtangent: (n, 4) float32, vuv: (n, 2)
        float32, meshes: MESH_DTYPE, stack_bound: the scene's current traversal stack bound)."""
        pr = GeometryProbe(C.sizeof(GeometryProbe))
        f4, f2, u4 = np.dtype((np.float32, 4)), np.dtype((np.float32, 2)), np.dtype((np.uint32, 4))
        out = self._probe("yart_hip_probe_geometry", pr, lambda: dict(
            bvh_nodes=(pr.n_bvh_nodes, BVH_NODE_DTYPE), leaf_tris=(pr.n_leaf_tris, LEAF_TRI_DTYPE), shade_tris=(pr.n_shade_tris, SHADE_TRI_DTYPE),
            tri_verts=(pr.n_tri_verts, u4), tri_light=(pr.n_tri_light, np.int32), vpos=(pr.n_vpos, f4), vnormal=(pr.n_vnormal, f4),
            vtangent=(pr.n_vtangent, f4), vuv=(pr.n_vuv, f2), meshes=(pr.n_meshes, MESH_DTYPE)))
        out["stack_bound"] = int(pr.stack_bound)
        return out

    def update_lighting(self, materials=None, lights=None, images=None, stream=None):
        """yart_hip_scene_update_lighting: new material values, new light emission / radius / transforms and new environment images
        for the scene in place. ``materials`` / ``lights``: the material / light lists of a :class:`yscn.Scene` (all of them; texture
        slots, thin_transmission and the lights' type / mesh / tri / two_sided / texture as at create), None: untouched. ``images``:
        {texture index: (H, W, 3) float32 array} — new texels, of the same size, for the maps of image lights; their sampling tables
        are rebuilt on the device. The call's statistics are in ``self.last_update``."""
        keep = []
        materials = list(materials) if materials is not None else []
        md = (MaterialDesc * max(len(materials), 1))()
        for i, m in enumerate(materials):
            C.memmove(C.byref(md[i]), m.pack(), C.sizeof(MaterialDesc))
        lights = list(lights) if lights is not None else []
        ld = _light_descs(lights)
        images = dict(images) if images is not None else {}
        im = (EnvImageUpdate * max(len(images), 1))()
        for k, (tex, px) in enumerate(images.items()):
            px = np.ascontiguousarray(px, np.float32)
            if px.ndim != 3 or px.shape[2] != 3:
                raise YartError(YART_E_INVALID, f"update_lighting: image {tex}: not an (H, W, 3) array")
            keep.append(px)
            im[k] = EnvImageUpdate(int(tex), px.shape[1], px.shape[0], px.ctypes.data_as(C.c_void_p))
        up = SceneLightingUpdate(C.sizeof(SceneLightingUpdate), len(materials), md if materials else None, len(lights),
                                 ld if lights else None, len(images), im if images else None, 0)
        self._update("yart_hip_scene_update_lighting", up, stream)

    def lighting_records(self):
        """yart_hip_probe_lighting: what ``update_lighting`` re-derives, read back from the device: dict(materials:
        MATERIAL_DEV_DTYPE, mat_class: uint8 lobe classes, lights: LIGHT_DEV_DTYPE, envs: ENV_DEV_DTYPE, env_data: float32, env_guide:
        uint32, area_power_cdf: float32, total_power: float, tex_f32: float32, tex_quads: uint8 (the footprint-record array, empty
        where the scene has none; bytes outside the records are unspecified), textures: TEX_DEV_DTYPE)."""
        pr = LightingProbe(C.sizeof(LightingProbe))
        out = self._probe("yart_hip_probe_lighting", pr, lambda: dict(
            materials=(pr.n_materials, MATERIAL_DEV_DTYPE), mat_class=(pr.n_mat_class, np.uint8), lights=(pr.n_lights, LIGHT_DEV_DTYPE),
            envs=(pr.n_envs, ENV_DEV_DTYPE), env_data=(pr.n_env_data, np.float32), env_guide=(pr.n_env_guide, np.uint32),
            area_power_cdf=(pr.n_area_power_cdf, np.float32), tex_f32=(pr.n_tex_f32, np.float32),
            tex_quads=(pr.n_tex_quad_bytes, np.uint8), textures=(pr.n_textures, TEX_DEV_DTYPE)))
        out["total_power"] = float(pr.total_power)
        return out

    def update_textures(self, textures, stream=None):
        """yart_hip_scene_update_textures: new texels for 8-bit material textures of the scene in place. ``textures``: {texture index:
        pixels} with the texture's size and channel count as at create — a NumPy uint8 array of shape (H, W, C), or (H, W) for one
        channel, is taken from host memory; a torch uint8 tensor of that shape on the scene's device (contiguous) is taken from device
        memory. Footprint records, the materials' alpha-test flag and what the meshes derive from it follow. The call's statistics
        are in ``self.last_update``."""
        keep, td = [], (TextureUpdate * max(len(textures), 1))()
        for k, (tex, px) in enumerate(dict(textures).items()):
            if hasattr(px, "data_ptr"):                       # a torch tensor: device pixels
                import torch
                if px.dtype != torch.uint8 or not px.is_cuda or not px.is_contiguous():
                    raise YartError(YART_E_INVALID, f"update_textures: texture {tex}: a tensor has to be contiguous uint8 on the scene's device")
                shape, ptr, flags = tuple(px.shape), px.data_ptr(), TEXELS_ON_DEVICE
            else:
                px = np.ascontiguousarray(px)
                if px.dtype != np.uint8:
                    raise YartError(YART_E_INVALID, f"update_textures: texture {tex}: not a uint8 array")
                shape, ptr, flags = px.shape, px.ctypes.data, 0
            if len(shape) == 2:
                shape = shape + (1,)
            if len(shape) != 3:
                raise YartError(YART_E_INVALID, f"update_textures: texture {tex}: not an (H, W, C) or (H, W) array")
            keep.append(px)
            td[k] = TextureUpdate(int(tex), shape[1], shape[0], shape[2], ptr, flags)
        up = SceneTextureUpdate(C.sizeof(SceneTextureUpdate), len(textures), td, 0)
        self._update("yart_hip_scene_update_textures", up, stream)

    def texture_records(self):
        """yart_hip_probe_textures: the 8-bit texels and the texture records, read back from the device: dict(tex_u8: uint8 (every
        texture padded to a multiple of 4 bytes), textures: TEX_DEV_DTYPE (offset: a texture's first byte of tex_u8; behind the
        scene's textures the entries creation adds for bundles))."""
        pr = TexturesProbe(C.sizeof(TexturesProbe))
        return self._probe("yart_hip_probe_textures", pr, lambda: dict(tex_u8=(pr.n_tex_u8, np.uint8), textures=(pr.n_textures, TEX_DEV_DTYPE)))

    def keep_previous(self, stream=None):
        """yart_hip_scene_keep_previous: the scene remembers the frame it holds (node transforms and vertex positions) as its
        previous frame. Once per frame, before that frame's ``update`` / ``update_meshes``."""
        _check(self._L.yart_hip_scene_keep_previous(self._h, stream), self._L)

    def pixel_motion(self, aovs: dict):
        """yart_hip_scene_pixel_motion_host: the per-pixel motion records between the frame ``keep_previous`` kept and the scene
        as it is now, from the feature buffers (``render_aovs``: position, normal, coverage, ids) of a frame rendered from the
        scene as it is now -> (H, W, 8) float32, what ``TemporalAccumulator.accumulate(pixel_motion=)`` takes.
        yart_amd.scene_motion.scene_motion_reference states the arithmetic in NumPy."""
        h, w = np.asarray(aovs["coverage"]).shape[:2]
        ab, _keep = _buffer_struct(AovBuffers, AOVS, h, w, PIXEL_MOTION_AOVS, host=aovs)
        rec = np.empty((h, w, 8), np.float32)
        _check(self._L.yart_hip_scene_pixel_motion_host(self._h, C.byref(ab), w, h, rec.ctypes.data_as(C.c_void_p)), self._L)
        return rec

    def pixel_motion_into(self, records_tensor, aov_tensors: dict, stream=None):
        """``pixel_motion`` on CUDA/HIP torch tensors (yart_hip_scene_pixel_motion_device) on ``stream`` (an integer handle; None:
        torch's current stream): ``records_tensor`` is a contiguous float32 device tensor of H*W*8 elements, (H, W, ...) its first
        two dimensions; what ``TemporalAccumulator.accumulate_into(pixel_motion=)`` takes."""
        import torch
        h, w = int(records_tensor.shape[0]), int(records_tensor.shape[1])
        rec = _device_tensor(records_tensor, "records", numel=h * w * 8, dtype=torch.float32)
        ab, _ = _buffer_struct(AovBuffers, AOVS, h, w, PIXEL_MOTION_AOVS, device=aov_tensors)
        _check(self._L.yart_hip_scene_pixel_motion_device(self._h, C.byref(ab), w, h, rec, _stream_of(stream, records_tensor)), self._L)
        return records_tensor

    def mesh_records(self, mesh):
        """yart_hip_probe_mesh: one mesh as the kernels see it, read back from the device: dict(mesh: MESH_DTYPE record, nodes:
        BVH_NODE_DTYPE, leaves: LEAF_TRI_DTYPE, shade: SHADE_TRI_DTYPE, positions / normals / tangents: (n_verts, 4) float32,
        stack_bound: the scene's current traversal stack bound)."""
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        md, bound = np.zeros(1, MESH_DTYPE), C.c_uint32()
        _check(self._L.yart_hip_probe_mesh(self._h, int(mesh), vp(md), None, None, None, None, None, None, C.byref(bound)), self._L)
        nt, nv, nn = int(md["n_tris"][0]), int(md["n_verts"][0]), int(md["n_nodes"][0])
        nodes, leaves, shade = np.zeros(nn, BVH_NODE_DTYPE), np.zeros(nt, LEAF_TRI_DTYPE), np.zeros(nt, SHADE_TRI_DTYPE)
        pos, nrm, tan = (np.zeros((nv, 4), np.float32) for _ in range(3))
        _check(self._L.yart_hip_probe_mesh(self._h, int(mesh), vp(md), vp(nodes), vp(leaves), vp(shade), vp(pos), vp(nrm), vp(tan),
                                           C.byref(bound)), self._L)
        return dict(mesh=md[0], nodes=nodes, leaves=leaves, shade=shade, positions=pos, normals=nrm, tangents=tan,
                    stack_bound=int(bound.value))

    def scene_graph(self):
        """yart_hip_probe_scene_graph: what an update re-derives, read back from the device: (nodes, node_world, tlas) as
        structured arrays of NODE_DTYPE, NODE_WORLD_DTYPE and TLAS_DTYPE (tlas: empty for a scene of fewer than 64 nodes). Only for a scene
        made from a :class:`yscn.Scene` (or updated since): for one loaded from a file the node count is not known here, and
        the call raises."""
        n = C.c_uint32()
        if self._n_nodes is None:                       # (the probe does not report the node count: scenes made from a yscn.Scene only)
            raise YartError(YART_E_INVALID, "scene_graph(): the scene was loaded from a file, its node count is not known")
        nodes, world = np.zeros(self._n_nodes, NODE_DTYPE), np.zeros(self._n_nodes, NODE_WORLD_DTYPE)
        tlas = np.zeros(max(2 * self._n_nodes - 1, 1), TLAS_DTYPE)
        _check(self._L.yart_hip_probe_scene_graph(self._h, nodes.ctypes.data_as(C.c_void_p), world.ctypes.data_as(C.c_void_p),
                                                  tlas.ctypes.data_as(C.c_void_p), C.byref(n)), self._L)
        return nodes, world, tlas[:n.value].copy()

    @property
    def handle(self):
        return self._h

    def close(self):
        if self._h:
            self._L.yart_hip_scene_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- rendering ----------------------------------------------------------------
    def render(self, p: dict, rank=0, world_size=1, flags=0, accumulated=None):
        """Blocking render to a host array (H, W, 4) float32 + stats dict. `accumulated`: the frame of the
        samples before p["start_sample"] when resuming (YartRenderParams.start_sample)."""
        _cam, head, st, out = _render_call(p, rank, world_size, flags, accumulated)
        _check(self._L.yart_hip_render(self._h, *head, C.byref(st)), self._L)
        return out, st.asdict()

    def render_waves(self, p: dict, on_wave=None, rank=0, world_size=1, flags=0, accumulated=None):
        """Like :meth:`render`, one wave of the schedule at a time (tile-renderer.hpp:264-289).
        ``on_wave(frame, info)`` is called after every wave with the frame blended so far (a view of the output
        array) and ``info = dict(wave, wave_samples, samples_taken, total_samples)``; returning a true value stops
        the render after that wave (Renderer::abort). Returns (frame, stats, aborted)."""
        return _run_progressive(self._L.yart_hip_render_waves, self._L, self._h, p, on_wave, tiles=False, rays=False,
                                rank=rank, world_size=world_size, flags=flags, accumulated=accumulated)

    def render_tiles(self, p: dict, on_tile=None, on_wave=None, rank=0, world_size=1, flags=0, accumulated=None):
        """Like :meth:`render_waves`, with tile granularity (Renderer::onRenderTileComplete): ``on_tile(frame, tile)``
        is called for every pixel block a batch of a wave has finished, ``frame`` being the output array (holding the
        blended values of that block) and ``tile`` a dict of YartTileInfo; a true return stops the render.
        ``p["max_batch_paths"]`` bounds a batch, i.e. how many blocks arrive together. Returns (frame, stats, aborted)."""
        return _run_progressive(self._L.yart_hip_render_tiles, self._L, self._h, p, on_wave, on_tile,
                                rank=rank, world_size=world_size, flags=flags, accumulated=accumulated)

    def render_into(self, tensor, p: dict, rank=0, world_size=1, flags=0, stream=None):
        """Render into a CUDA/HIP torch tensor of shape (H, W, 4) float32 (device memory)."""
        _cam, head, st, _ = _render_call(p, rank, world_size, flags, into=tensor)
        _check(self._L.yart_hip_render_device(self._h, *head, _stream_of(stream), C.byref(st)), self._L)
        return st.asdict()

    def _render_buffers(self, p, aovs, moments, rank, world_size, flags):
        """``render_moments``, and with ``moments`` None ``render_aovs``: the same call but for the entry and its moments argument"""
        _cam, head, st, out = _render_call(p, rank, world_size, flags)
        h, w = out.shape[:2]
        ab, bufs = _buffer_struct(AovBuffers, AOVS, h, w, aovs)
        mb, moms = _buffer_struct(MomentBuffers, MOMENTS, h, w, moments or ())
        if moments is None:
            _check(self._L.yart_hip_render_aovs(self._h, *head, C.byref(ab), C.byref(st)), self._L)
        else:
            _check(self._L.yart_hip_render_moments(self._h, *head, C.byref(ab), C.byref(mb), C.byref(st)), self._L)
        return out, bufs, moms, st.asdict()

    def _render_buffers_into(self, tensor, aov_tensors, moment_tensors, p, rank, world_size, flags, stream):
        """``render_moments_into``, and with ``moment_tensors`` None ``render_aovs_into``"""
        cam, head, st, _ = _render_call(p, rank, world_size, flags, into=tensor)
        ab, _ = _buffer_struct(AovBuffers, AOVS, cam.height, cam.width, device=aov_tensors)
        mb, _ = _buffer_struct(MomentBuffers, MOMENTS, cam.height, cam.width, device=moment_tensors or {})
        if moment_tensors is None:
            _check(self._L.yart_hip_render_aovs_device(self._h, *head, C.byref(ab), _stream_of(stream), C.byref(st)), self._L)
        else:
            _check(self._L.yart_hip_render_moments_device(self._h, *head, C.byref(ab), C.byref(mb), _stream_of(stream), C.byref(st)),
                   self._L)
        return st.asdict()

    def render_aovs(self, p: dict, aovs: Sequence[str] = AOV_ALL, rank=0, world_size=1, flags=0):
        """``render`` + first-hit feature buffers (include/yart_hip.h: YartAovBuffers) from the same camera samples.
        Returns (frame HxWx4 float32, {name: ndarray HxWxC (HxW for one channel)}, stats dict); names from ``AOVS``."""
        out, bufs, _, st = self._render_buffers(p, aovs, None, rank, world_size, flags)
        return out, bufs, st

    def render_aovs_into(self, tensor, aov_tensors: dict, p: dict, rank=0, world_size=1, flags=0, stream=None):
        """``render_into`` + feature buffers written into CUDA/HIP torch tensors: ``aov_tensors`` maps names of ``AOVS`` to
        contiguous device tensors of H*W*channels elements (float32; ids int32; rays int32 holding the uint32 counts)."""
        return self._render_buffers_into(tensor, aov_tensors, None, p, rank, world_size, flags, stream)

    def render_moments(self, p: dict, moments: Sequence[str] = MOMENT_ALL, aovs: Sequence[str] = (), rank=0, world_size=1, flags=0):
        """``render_aovs`` + per-pixel sample moments (include/yart_hip.h: YartMomentBuffers) of the frame's own samples.
        Returns (frame HxWx4 float32, {aov name: ndarray}, {moment name: ndarray HxWx3 / HxW}, stats dict); moment names
        from ``MOMENTS``. yart_amd.moments.moments_reference states the arithmetic in NumPy."""
        return self._render_buffers(p, aovs, tuple(moments), rank, world_size, flags)

    def render_moments_into(self, tensor, aov_tensors: dict, moment_tensors: dict, p: dict, rank=0, world_size=1, flags=0,
                            stream=None):
        """``render_aovs_into`` + sample moments written into CUDA/HIP torch tensors: ``moment_tensors`` maps names of
        ``MOMENTS`` to contiguous device tensors of H*W*channels 4-byte elements (float32; count int32 holding the uint32)."""
        return self._render_buffers_into(tensor, aov_tensors or {}, moment_tensors or {}, p, rank, world_size, flags, stream)

    def render_denoised(self, p: dict, iterations=None, sigma_color=DEFAULT_SIGMA_COLOR, sigma_normal=None, sigma_depth=None,
                        demodulate=True, rank=0, world_size=1, flags=0, device="cuda", variance_guided=False,
                        sigma_luma=DEFAULT_VAR_SIGMA_LUMA, temporal=None, motion=None, pixel_motion=False, exposure=None, dt=0.0,
                        look=None):
        """``render_aovs_into`` for albedo, normal and depth, then the à-trous filter (``denoise_into``) on the same device
        buffers, on torch's current stream: no host round trip. Returns (noisy frame, denoised frame, {name: guide}) as torch
        tensors of ``device`` ((H, W, 4); guides (H, W, 3) / (H, W)).
        ``variance_guided=True``: ``render_moments_into`` with the variance buffer as well, then the variance-guided filter
        (``denoise_var_into``) with ``sigma_luma`` in place of ``sigma_color`` (which is not used then); the guides returned
        then include "variance" (H, W). ``iterations``, ``sigma_normal`` and ``sigma_depth`` left at None take the defaults
        of the filter that runs (DEFAULT_* of the plain one, DEFAULT_VAR_* of the variance-guided one).
        ``temporal``: a :class:`TemporalAccumulator` of the frame's size — one frame of a sequence: ``render_moments_into`` with
        the variance and the feature buffers the accumulator needs, then ``temporal.accumulate_into`` (at the accumulator's own
        parameters and in its own form — plain or moments —, demodulating as ``demodulate`` says), then the variance-guided
        filter on the accumulated frame and variance (``variance_guided`` is implied). Returns (noisy frame, denoised frame, guides) with "accumulated" (H, W, 4),
        "accumulated_variance" (H, W) and "length" (H, W, int32 holding the uint32) among the guides. None: as before.
        ``motion`` (with ``temporal``): how this scene's nodes moved since the previous frame's scene — the records of
        yart_amd.temporal.node_motion(previous nodes, these nodes) —, handed to ``temporal.accumulate_into``.
        ``pixel_motion=True`` (with ``temporal``, not with ``motion``): the scene was updated in place since ``keep_previous``:
        the per-pixel records are computed from the frame's own feature buffers (``pixel_motion_into``, on the same stream) and
        handed to ``temporal.accumulate_into``; they are returned among the guides as "pixel_motion" (H, W, 8).
        ``exposure``: an :class:`AutoExposure` — the display stage: the denoised frame is metered (``exposure.meter_into``,
        ``dt`` seconds after the previous frame) and applied (``exposure.apply_into`` with ``look``: None = no tonemapper, or an
        AgX look's name) on the same stream; "display" (H, W, 4) and "display_rgb8" (H, W, 3 uint8) are added to the guides.
        None: as before."""
        noisy, clean, guides = self._render_denoised(p, iterations, sigma_color, sigma_normal, sigma_depth, demodulate, rank, world_size,
                                                     flags, device, variance_guided, sigma_luma, temporal, motion, pixel_motion)
        if exposure is None:
            return noisy, clean, guides
        import torch
        display = torch.empty_like(clean)
        rgb8 = torch.empty(tuple(clean.shape[:2]) + (3,), dtype=torch.uint8, device=clean.device)
        stream = torch.cuda.current_stream(clean.device).cuda_stream
        exposure.meter_into(clean, dt, stream=stream)
        exposure.apply_into(display, rgb8, clean, look, stream=stream)
        return noisy, clean, dict(guides, display=display, display_rgb8=rgb8)

    def _render_denoised(self, p, iterations, sigma_color, sigma_normal, sigma_depth, demodulate, rank, world_size, flags, device,
                         variance_guided, sigma_luma, temporal, motion, pixel_motion):
        import torch
        assert motion is None or temporal is not None, "render_denoised: motion needs a temporal accumulator"
        assert not pixel_motion or temporal is not None, "render_denoised: pixel_motion needs a temporal accumulator"
        assert not pixel_motion or motion is None, "render_denoised: one motion at a time, motion= or pixel_motion=True"
        if temporal is not None:
            variance_guided = True
        dflt = ((DEFAULT_VAR_ITERATIONS, DEFAULT_VAR_SIGMA_NORMAL, DEFAULT_VAR_SIGMA_DEPTH) if variance_guided else
                (DEFAULT_ITERATIONS, DEFAULT_SIGMA_NORMAL, DEFAULT_SIGMA_DEPTH))
        iterations = dflt[0] if iterations is None else iterations
        sigma_normal = dflt[1] if sigma_normal is None else sigma_normal
        sigma_depth = dflt[2] if sigma_depth is None else sigma_depth
        w, h = int(p["size"][0]), int(p["size"][1])
        noisy = torch.empty((h, w, 4), dtype=torch.float32, device=device)
        guides = {"albedo": torch.empty((h, w, 3), dtype=torch.float32, device=device),
                  "normal": torch.empty((h, w, 3), dtype=torch.float32, device=device),
                  "depth": torch.empty((h, w), dtype=torch.float32, device=device)}
        stream = torch.cuda.current_stream(noisy.device).cuda_stream
        if temporal is not None:
            variance = torch.empty((h, w), dtype=torch.float32, device=device)
            feats = dict(guides, position=torch.empty((h, w, 3), dtype=torch.float32, device=device),
                         coverage=torch.empty((h, w), dtype=torch.float32, device=device),
                         ids=torch.empty((h, w, 4), dtype=torch.int32, device=device))
            self.render_moments_into(noisy, feats, {"variance": variance}, p, rank, world_size, flags, stream=stream)
            acc, acc_var = torch.empty_like(noisy), torch.empty_like(variance)
            length = torch.empty((h, w), dtype=torch.int32, device=device)
            extra, records = {}, None
            if pixel_motion:
                records = torch.empty((h, w, 8), dtype=torch.float32, device=device)
                self.pixel_motion_into(records, feats, stream=stream)
                extra["pixel_motion"] = records
            temporal.accumulate_into(acc, acc_var, length, p, noisy, variance, feats, demodulate=demodulate, stream=stream,
                                     motion=motion, pixel_motion=records)
            clean = torch.empty_like(noisy)
            denoise_var_into(clean, acc, acc_var, guides, iterations, sigma_luma, sigma_normal, sigma_depth, demodulate)
            return noisy, clean, dict(feats, variance=variance, accumulated=acc, accumulated_variance=acc_var, length=length, **extra)
        if variance_guided:
            variance = torch.empty((h, w), dtype=torch.float32, device=device)
            self.render_moments_into(noisy, guides, {"variance": variance}, p, rank, world_size, flags, stream=stream)
            clean = torch.empty_like(noisy)
            denoise_var_into(clean, noisy, variance, guides, iterations, sigma_luma, sigma_normal, sigma_depth, demodulate)
            return noisy, clean, dict(guides, variance=variance)
        self.render_aovs_into(noisy, guides, p, rank, world_size, flags, stream=stream)
        clean = torch.empty_like(noisy)
        denoise_into(clean, noisy, guides, iterations, sigma_color, sigma_normal, sigma_depth, demodulate)
        return noisy, clean, guides

    # -- diagnostics ----------------------------------------------------------------
    def probe_camera_rays(self, p: dict, xys: Sequence[Sequence[int]]):
        """The camera ray (origin, direction: 6 floats) of each (x, y, sample), drawn as bounce 0 of that sample draws it."""
        cam, rp = make_camera(p), make_params(p)
        a = np.ascontiguousarray(xys, np.uint32).reshape(-1, 3)
        out = np.empty((len(a), 6), np.float32)
        _check(self._L.yart_hip_probe_camera_rays(self._h, C.byref(cam), C.byref(rp), len(a), a.ctypes.data_as(C.c_void_p),
                                                  out.ctypes.data_as(C.c_void_p)), self._L)
        return out

    def probe_samples(self, p: dict, xys: Sequence[Sequence[int]]):
        cam, rp = make_camera(p), make_params(p)
        a = np.ascontiguousarray(xys, np.uint32).reshape(-1, 3)
        out = np.empty((len(a), 3), np.float32)
        rays = C.c_uint64()
        _check(self._L.yart_hip_probe_samples(self._h, C.byref(cam), C.byref(rp), len(a),
                                              a.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p),
                                              C.byref(rays)), self._L)
        return out, rays.value

    def probe_hits(self, rays):
        a = np.ascontiguousarray(rays, np.float32).reshape(-1, 6)
        out = np.empty((len(a), 16), np.float32)
        _check(self._L.yart_hip_probe_hits(self._h, len(a), a.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)), self._L)
        return out

    def probe_rays(self, p: dict, rays, walk: int = 0):
        """One walk of the scene per ray record (include/yart_hip.h yart_hip_probe_rays): `rays` holds 12 32-bit words per ray
        (origin, direction, tMax, kind, x, y, s, pad — any dtype of that size), `walk` selects TRAV_GENERAL (0), TRAV_FAST (1) or
        TRAV_FAST | TRAV_IDENTITY (2); the sampler is the one a render with `p` constructs. Returns uint32 [n, 20] result words."""
        a = np.ascontiguousarray(rays).view(np.uint32).reshape(-1, 12)
        out = np.empty((len(a), 20), np.uint32)
        rp = make_params(p)
        _check(self._L.yart_hip_probe_rays(self._h, C.byref(rp), len(a), a.ctypes.data_as(C.c_void_p), int(walk),
                                           out.ctypes.data_as(C.c_void_p)), self._L)
        return out

    def probe_shading(self, cases, form: int = 0):
        """One call of the shading code per case record (include/yart_hip.h yart_hip_probe_shading, oracle/shaderec.hpp):
        `cases` holds 32 32-bit words per case (any dtype of that size), `form` is the bit set 1 (GGX tables in LDS) | 2 (scene
        records in LDS) | 4 (matEvaluate + *ImplE). Returns uint32 [n, 32] result words."""
        a = np.ascontiguousarray(cases).view(np.uint32).reshape(-1, 32)
        out = np.empty((len(a), 32), np.uint32)
        _check(self._L.yart_hip_probe_shading(self._h, len(a), a.ctypes.data_as(C.c_void_p), int(form),
                                              out.ctypes.data_as(C.c_void_p)), self._L)
        return out

    def probe_sampler(self, spp, tile, cases, pattern, use_tables=False):
        """Device-side sampler draws (diagnostic): cases = [(px, py, sample)], pattern = sequence of 1 (get1D) / 2 (get2D);
        returns float32 [n_cases, sum(pattern)]."""
        cs = np.ascontiguousarray(np.asarray(cases, np.uint32).reshape(-1, 3))
        pat = np.ascontiguousarray(np.asarray(pattern, np.uint8))
        out = np.empty((len(cs), int(pat.sum())), np.float32)
        _check(self._L.yart_hip_probe_sampler(self._h, int(spp), int(tile), len(cs), cs.ctypes.data_as(C.c_void_p), len(pat),
                                              pat.ctypes.data_as(C.c_void_p), 1 if use_tables else 0, out.ctypes.data_as(C.c_void_p)), self._L)
        return out

    def debug_counters(self):
        out = (C.c_uint64 * 32)()
        _check(self._L.yart_hip_debug_counters(self._h, out), self._L)
        return [int(v) for v in out]

    def bvh(self, mesh: int):
        nn, nt = C.c_uint32(), C.c_uint32()
        _check(self._L.yart_hip_bvh_info(self._h, mesh, C.byref(nn), C.byref(nt)), self._L)
        nodes = np.empty((nn.value, 8), np.uint32); idx = np.empty(nt.value, np.uint32)
        _check(self._L.yart_hip_bvh_copy(self._h, mesh, nodes.ctypes.data_as(C.c_void_p), idx.ctypes.data_as(C.c_void_p)), self._L)
        return nodes, idx


class MultiDeviceScene:
    """Owns a ``YartMulti*``: the scene replicated on several GPUs of this node, one host thread per device, pixel
    blocks dealt round-robin, the devices' own pixels merged on ``devices[0]`` with RCCL send / recv (include/yart_hip.h;
    stands where TileRenderer's worker pool and finishTile's merge stand, tile-renderer.hpp:150-197, 225-241)."""

    def __init__(self, scene, devices: Sequence[int], env_hdr=None, env_radius=100.0, uniform_env=None):
        self._h = C.c_void_p()
        self._L = lib()
        devs = (C.c_int * len(devices))(*[int(d) for d in devices])
        if isinstance(scene, (str, os.PathLike)):
            o = import_options(env_hdr, env_radius, uniform_env)
            _check(self._L.yart_hip_multi_load(os.fspath(scene).encode(), C.byref(o), devs, len(devices), C.byref(self._h)), self._L)
        else:
            desc, _keep = describe_scene(scene)
            _check(self._L.yart_hip_multi_create(C.byref(desc), devs, len(devices), C.byref(self._h)), self._L)

    @property
    def n_devices(self):
        return int(self._L.yart_hip_multi_device_count(self._h))

    def failed_replicas(self):
        """Replicas taken out of service by a device failure (their blocks are rendered on devices[0]); [] normally."""
        out = (C.c_int * 64)()
        n = int(self._L.yart_hip_multi_failed_devices(self._h, out, 64))
        return [int(out[k]) for k in range(min(n, 64))]

    def render(self, p: dict, rank=0, world_size=1, flags=0, accumulated=None):
        _cam, head, st, out = _render_call(p, rank, world_size, flags, accumulated)
        _check(self._L.yart_hip_multi_render(self._h, *head, C.byref(st)), self._L)
        return out, st.asdict()

    def render_tiles(self, p: dict, on_tile=None, on_wave=None, rank=0, world_size=1, flags=0, accumulated=None):
        """The progressive form (yart_hip_multi_render_tiles): every wave rendered by all devices, merged, reported through
        ``on_wave(frame, info)``; with ``on_tile(frame, tile)`` every block of the frame once per wave (Morton order, its own
        ray count). Returns (frame, stats, aborted)."""
        return _run_progressive(self._L.yart_hip_multi_render_tiles, self._L, self._h, p, on_wave, on_tile,
                                rank=rank, world_size=world_size, flags=flags, accumulated=accumulated)

    def close(self):
        if self._h:
            self._L.yart_hip_multi_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


@dataclass
class RenderData:
    """Mirror of ``yart::Renderer::RenderData`` (reference src/core/renderer.hpp:22-28)."""
    buffer: np.ndarray
    samples_taken: int
    total_samples: int
    total_rays: int
    total_time_ms: float
    stats: dict


class HipTileRenderer:
    """Drop-in for ``yart::cpu::TileRenderer<SobolSampler<FastOwenScrambler>, MISIntegrator>``
    (reference src/cpu/tile-renderer.hpp:25-115): same knobs, same blocking / async calls.

    ``camera`` is a dict in the vocabulary of ``oracle/params.hpp`` (size, focal, fnumber,
    sensor, eye, target, up, exposure, aperture_sides)."""

    def __init__(self, width: int, height: int, camera: dict, device: int = -1):
        self.samples = 64                 # DEFAULT_SAMPLE_COUNT, tile-renderer.hpp:10-13
        self.first_wave_samples = 64
        self.max_wave_samples = 128
        self.tile_size = 64
        self.max_depth = 30               # RayIntegrator::m_maxDepth, ray-integrator.hpp:14
        self.background_color = (0.0, 0.0, 0.0)
        self.scene: Optional[DeviceScene] = None
        self.tonemapper = None            # AgX look name ("none" / "golden" / "punchy") or None: linear HDR buffer
        self.estimator = ESTIMATOR_GMON   # integrator.cpp:17-18 fixes it at compile time
        self.on_render_complete = None    # callbacks of renderer.hpp:55-58
        self.on_render_aborted = None
        self.on_render_wave_complete = None   # f(RenderData, dict(wave, wave_samples, samples_taken, total_samples))
        self.on_render_tile_complete = None   # f(RenderData, dict of YartTileInfo): per finished pixel block of a batch
        self.max_batch_paths = 0              # YartRenderParams.max_batch_paths: how many blocks finish together (0: all)
        self._camera = dict(camera, size=(width, height))
        self._device = device
        self._thread: Optional[threading.Thread] = None
        self._abort = False
        self._result: Optional[RenderData] = None

    def _params(self):
        return dict(self._camera, spp=self.samples, first_wave=min(self.first_wave_samples, self.samples),
                    max_wave=self.max_wave_samples, tile=self.tile_size, depth=self.max_depth,
                    background=self.background_color, estimator=self.estimator, max_batch_paths=self.max_batch_paths)

    def render_sync(self) -> RenderData:
        if self.scene is None:           # Integrator::render: "if (!scene) return" (integrator.cpp:6)
            w, h = self._camera["size"]
            return RenderData(np.zeros((h, w, 4), np.float32), 0, self.samples, 0, 0.0, {})
        t0 = time.perf_counter()
        taken = [0]
        self._abort = False

        def shown(frame):                 # tile-renderer.hpp:234-239: the exposed buffer is the tonemapped one
            return tonemap(frame, self.tonemapper)[0] if self.tonemapper else frame

        def on_wave(frame, info):
            taken[0] = info["samples_taken"]
            if self.on_render_wave_complete:
                self.on_render_wave_complete(RenderData(shown(frame), info["samples_taken"], self.samples, 0,
                                                        (time.perf_counter() - t0) * 1e3, {}), info)
            return self._abort
        if self.on_render_tile_complete:
            display = [None]               # ONE persistent display buffer per render (integration/hip-renderer.hpp::expose does the same)

            def on_tile(frame, tile):
                x, y, w, h = tile["x"], tile["y"], tile["width"], tile["height"]
                view = frame
                if self.tonemapper:        # tile-renderer.hpp:234-239 maps the finished tile only, into the buffer it exposes
                    if display[0] is None:
                        display[0] = np.zeros_like(frame)
                    view = display[0]
                    view[y:y + h, x:x + w] = tonemap(np.ascontiguousarray(frame[y:y + h, x:x + w]), self.tonemapper)[0]
                self.on_render_tile_complete(RenderData(view, tile["samples_taken"] - tile["wave_samples"], self.samples, 0,
                                                        (time.perf_counter() - t0) * 1e3, {}), tile)
                return self._abort
            buf, st, _ = self.scene.render_tiles(self._params(), on_tile, on_wave)
        else:
            buf, st, _ = self.scene.render_waves(self._params(), on_wave)
        ms = (time.perf_counter() - t0) * 1e3
        self._result = RenderData(shown(buf), taken[0], self.samples, st["rays"], ms, st)
        return self._result

    def render(self):
        def run():
            r = self.render_sync()
            cb = self.on_render_aborted if self._abort else self.on_render_complete
            if cb:
                cb(r)
        self._thread = threading.Thread(target=run, daemon=True)
        self._thread.start()

    def abort(self):
        self._abort = True               # takes effect after the wave in flight (the reference: after the tiles in flight)

    def wait(self):
        if self._thread:
            self._thread.join()


AGX_LOOKS = {"none": 0, "golden": 1, "punchy": 2}


def tonemap(hdr: np.ndarray, look: Optional[str] = "none"):
    """AgX tonemap (reference core/tonemapping.hpp; look None = no tonemapper) + the 8-bit encoding of
    output/ppm.cpp of an (H, W, 4) float32 frame, on the device. Returns (ldr float32 (H,W,4), rgb8 (H,W,3))."""
    hdr = np.ascontiguousarray(hdr, np.float32)
    h, w = hdr.shape[:2]
    ldr = np.empty_like(hdr)
    rgb = np.empty((h, w, 3), np.uint8)
    L = lib()
    _check(L.yart_hip_tonemap_host(hdr.ctypes.data_as(C.c_void_p), w, h, -1 if look is None else AGX_LOOKS[look],
                                   ldr.ctypes.data_as(C.c_void_p), rgb.ctypes.data_as(C.c_void_p)), L)
    return ldr, rgb


def _denoise_host(var, frame, variance, albedo, normal, depth, dp, demodulate, out):
    """``denoise`` (``var`` False: ``variance`` is not looked at) and ``denoise_var``: NumPy arrays through the _host entry point.
    ``dp(demodulate)`` makes the form's parameter struct."""
    frame = np.ascontiguousarray(frame, np.float32)
    h, w = frame.shape[:2]
    assert frame.shape == (h, w, 4)
    if demodulate is None:
        demodulate = albedo is not None

    def guide(a, ch):
        if a is None:
            return None, None
        a = np.ascontiguousarray(a, np.float32)
        assert a.size == h * w * ch
        return a, a.ctypes.data_as(C.c_void_p)
    (kv, pv), (ka, pa), (kn, pn), (kd, pd) = guide(variance, 1), guide(albedo, 3), guide(normal, 3), guide(depth, 1)
    if out is None:
        out = np.empty_like(frame)
    assert out.dtype == np.float32 and out.flags.c_contiguous and out.shape == frame.shape
    L = lib()
    fn = L.yart_hip_denoise_atrous_var_host if var else L.yart_hip_denoise_atrous_host
    _check(fn(frame.ctypes.data_as(C.c_void_p), *([pv] if var else []), pa, pn, pd, w, h, C.byref(dp(demodulate)),
              out.ctypes.data_as(C.c_void_p)), L)
    return out


def _denoise_device(var, out_tensor, frame_tensor, variance_tensor, guides, dp, demodulate, stream):
    """``denoise_into`` (``var`` False: ``variance_tensor`` is not looked at) and ``denoise_var_into``: torch tensors through the
    _device entry point. ``dp(demodulate)`` makes the form's parameter struct."""
    import torch
    h, w = int(frame_tensor.shape[0]), int(frame_tensor.shape[1])
    if demodulate is None:
        demodulate = (guides or {}).get("albedo") is not None
    guides = guides or {}
    ptrs = [_device_tensor(guides.get(name), name, numel=h * w * ch, dtype=torch.float32, optional=True)
            for name, ch in (("albedo", 3), ("normal", 3), ("depth", 1))]
    unknown = set(guides) - {"albedo", "normal", "depth"}
    assert not unknown, f"{'denoise_var_into' if var else 'denoise_into'}: unknown guides {sorted(unknown)}"
    frame, out = (_device_tensor(t, what, shape=(h, w, 4), dtype=torch.float32) for t, what in ((frame_tensor, "frame"), (out_tensor, "out")))
    first = [frame, _device_tensor(variance_tensor, "variance", numel=h * w, dtype=torch.float32)] if var else [frame]
    L = lib()
    fn = L.yart_hip_denoise_atrous_var_device if var else L.yart_hip_denoise_atrous_device
    with torch.cuda.device(frame_tensor.device):
        _check(fn(*first, *ptrs, w, h, C.byref(dp(demodulate)), out, _stream_of(stream, frame_tensor)), L)
    return out_tensor


def denoise(frame, albedo=None, normal=None, depth=None, iterations=DEFAULT_ITERATIONS, sigma_color=DEFAULT_SIGMA_COLOR,
            sigma_normal=DEFAULT_SIGMA_NORMAL, sigma_depth=DEFAULT_SIGMA_DEPTH, demodulate=None, out=None):
    """The edge-avoiding à-trous filter (include/yart_hip.h: yart_hip_denoise_atrous_host) of an (H, W, 4) float32 linear-HDR
    frame on the device, guided by whichever of ``albedo`` (H, W, 3), ``normal`` (H, W, 3) and ``depth`` (H, W) are given;
    ``demodulate`` divides by the albedo before and multiplies after (None: whenever ``albedo`` is given). ``out``: a C-contiguous float32 array to fill (may be
    ``frame``). yart_amd.denoise.atrous_reference states the same arithmetic in NumPy."""
    return _denoise_host(False, frame, None, albedo, normal, depth,
                         lambda dm: make_denoise_params(iterations, sigma_color, sigma_normal, sigma_depth, dm), demodulate, out)


def denoise_into(out_tensor, frame_tensor, guides=None, iterations=DEFAULT_ITERATIONS, sigma_color=DEFAULT_SIGMA_COLOR,
                 sigma_normal=DEFAULT_SIGMA_NORMAL, sigma_depth=DEFAULT_SIGMA_DEPTH, demodulate=None, stream=None):
    """``denoise`` on CUDA/HIP torch tensors through ``data_ptr()`` (yart_hip_denoise_atrous_device): ``frame_tensor`` and
    ``out_tensor`` (H, W, 4) float32 (they may be the same tensor), ``guides`` a dict with any of "albedo", "normal" (H*W*3
    elements) and "depth" (H*W). Runs on ``stream`` (a raw hipStream_t), by default torch's current stream of the frame's
    device, and returns after completion there."""
    return _denoise_device(False, out_tensor, frame_tensor, None, guides,
                           lambda dm: make_denoise_params(iterations, sigma_color, sigma_normal, sigma_depth, dm), demodulate, stream)


def denoise_var(frame, variance, albedo=None, normal=None, depth=None, iterations=DEFAULT_VAR_ITERATIONS,
                sigma_luma=DEFAULT_VAR_SIGMA_LUMA, sigma_normal=DEFAULT_VAR_SIGMA_NORMAL, sigma_depth=DEFAULT_VAR_SIGMA_DEPTH,
                demodulate=None, out=None):
    """The variance-guided à-trous filter (include/yart_hip.h: yart_hip_denoise_atrous_var_host): ``denoise`` with the per-pixel
    ``variance`` (H, W) of ``render_moments`` as a fourth input and ``sigma_luma`` in place of ``sigma_color``.
    yart_amd.denoise.atrous_var_reference states the same arithmetic in NumPy."""
    return _denoise_host(True, frame, variance, albedo, normal, depth,
                         lambda dm: make_denoise_var_params(iterations, sigma_luma, sigma_normal, sigma_depth, dm), demodulate, out)


def denoise_var_into(out_tensor, frame_tensor, variance_tensor, guides=None, iterations=DEFAULT_VAR_ITERATIONS,
                     sigma_luma=DEFAULT_VAR_SIGMA_LUMA, sigma_normal=DEFAULT_VAR_SIGMA_NORMAL, sigma_depth=DEFAULT_VAR_SIGMA_DEPTH,
                     demodulate=None, stream=None):
    """``denoise_var`` on CUDA/HIP torch tensors through ``data_ptr()`` (yart_hip_denoise_atrous_var_device): as
    ``denoise_into``, with ``variance_tensor`` (H*W float32 elements)."""
    return _denoise_device(True, out_tensor, frame_tensor, variance_tensor, guides,
                           lambda dm: make_denoise_var_params(iterations, sigma_luma, sigma_normal, sigma_depth, dm), demodulate, stream)


class TemporalAccumulator:
    """Temporal accumulation with camera reprojection for a sequence of frames of one scene (include/yart_hip.h:
    yart_hip_temporal_*): the stage between ``render_moments`` and ``denoise_var``. Holds the history (96 bytes per pixel on the
    device, allocated by the first frame) and the last frame's camera. ``alpha_min`` / ``max_history`` / ``normal_cos_min`` /
    ``plane_tolerance`` are the parameters of every frame unless a call overrides them. ``device`` < 0: the device current at
    the first frame. yart_amd.temporal.temporal_reference states the same arithmetic in NumPy.
    ``moments=True``: the moments form (yart_hip_temporal_accumulate_moments_*; 128 bytes per pixel): the returned variance is
    estimated from the accumulated luminance moments, and from the 7 x 7 neighbourhood where the history is shorter than
    ``min_moment_history`` — the form for low sample counts, where the rendered variance is 0 or nearly so.
    yart_amd.temporal.temporal_moments_reference states it. A handle is in one form between resets.
    ``clip``: the clip of the history to the frame's neighbourhood, against ghosting when the lighting changes
    (yart_hip_temporal_set_clip): None (off), True (the defaults) or (radius, gamma); see ``set_clip``."""

    def __init__(self, width: int, height: int, device: int = 0, alpha_min=DEFAULT_ALPHA_MIN, max_history=DEFAULT_MAX_HISTORY,
                 normal_cos_min=DEFAULT_NORMAL_COS_MIN, plane_tolerance=DEFAULT_PLANE_TOLERANCE, moments=False,
                 min_moment_history=DEFAULT_MIN_MOMENT_HISTORY, clip=None):
        self._L = lib()
        self.width, self.height, self.device = int(width), int(height), int(device)
        self.moments = bool(moments)
        self.params = dict(alpha_min=alpha_min, max_history=max_history, normal_cos_min=normal_cos_min,
                           plane_tolerance=plane_tolerance)
        if self.moments:
            self.params["min_moment_history"] = min_moment_history
        h = C.c_void_p()
        _check(self._L.yart_hip_temporal_create(self.width, self.height, self.device, C.byref(h)), self._L)
        self._h = h
        self.clip = None
        if clip is not None and clip is not False:
            self.set_clip(clip)

    @property
    def handle(self):
        return self._h

    def close(self):
        if getattr(self, "_h", None):
            self._L.yart_hip_temporal_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reset(self):
        """Forget the history (and a pending motion; not the clip): the next frame is a first frame."""
        _check(self._L.yart_hip_temporal_reset(self._h), self._L)

    def set_clip(self, clip):
        """The clip of every following frame (yart_hip_temporal_set_clip): None turns it off, True sets the defaults
        (DEFAULT_CLIP_RADIUS, DEFAULT_CLIP_GAMMA), (radius, gamma) sets radius 1 .. 3 and a finite gamma >= 0. The setting stays,
        across ``reset`` too, until it is set again; a refused one keeps the previous setting. ``self.clip`` is the setting as
        the references' ``clip=`` takes it."""
        if clip is None or clip is False:
            _check(self._L.yart_hip_temporal_set_clip(self._h, None), self._L)
            self.clip = None
            return
        radius, gamma = (DEFAULT_CLIP_RADIUS, DEFAULT_CLIP_GAMMA) if clip is True else clip
        assert int(radius) == radius and 0 <= int(radius) < 1 << 32, "clip: radius is an unsigned integer"
        tc = TemporalClip(C.sizeof(TemporalClip), int(radius), float(gamma))
        _check(self._L.yart_hip_temporal_set_clip(self._h, C.byref(tc)), self._L)
        self.clip = (int(radius), float(gamma))

    def set_motion(self, motion):
        """Per-node motion for the next ``accumulate`` / ``accumulate_into`` (yart_hip_temporal_set_motion), which consumes it:
        an (n_nodes, 24) float32 array as yart_amd.temporal.node_motion builds it. None clears a pending motion."""
        if motion is None:
            _check(self._L.yart_hip_temporal_set_motion(self._h, None), self._L)
            return
        rec = np.ascontiguousarray(motion)
        assert rec.dtype == np.float32 and rec.size % MOTION_WORDS == 0, "motion: (n_nodes, 24) float32 records"
        tm = TemporalMotion(C.sizeof(TemporalMotion), rec.size // MOTION_WORDS, rec.ctypes.data_as(C.c_void_p))
        _check(self._L.yart_hip_temporal_set_motion(self._h, C.byref(tm)), self._L)

    def set_pixel_motion(self, records):
        """Per-pixel motion for the next ``accumulate`` / ``accumulate_into`` (yart_hip_temporal_set_pixel_motion), which consumes
        it: ``DeviceScene.pixel_motion``'s (H, W, 8) float32 NumPy array for ``accumulate``, ``pixel_motion_into``'s device tensor
        for ``accumulate_into``. The records are NOT copied: the caller keeps them alive until that call has returned. None clears
        a pending motion; a motion set by ``set_motion`` is replaced."""
        if records is None:
            _check(self._L.yart_hip_temporal_set_pixel_motion(self._h, None), self._L)
            return
        if isinstance(records, np.ndarray):
            assert records.dtype == np.float32 and records.flags.c_contiguous, "pixel motion: a contiguous float32 array"
            ptr = records.ctypes.data
        else:
            ptr = _device_tensor(records, "pixel motion: a contiguous float32 device tensor", element_size=4).value
        n = records.size if isinstance(records, np.ndarray) else records.numel()
        assert n == self.width * self.height * 8, "pixel motion: (H, W, 8) records"
        pm = TemporalPixelMotion(C.sizeof(TemporalPixelMotion), C.c_void_p(ptr))
        _check(self._L.yart_hip_temporal_set_pixel_motion(self._h, C.byref(pm)), self._L)

    def _camera(self, cam):
        return cam if isinstance(cam, CameraDesc) else make_camera(cam)

    def _params(self, demodulate, over):
        unknown = set(over) - set(self.params)
        assert not unknown, f"TemporalAccumulator: unknown parameters {sorted(unknown)}"
        make = make_temporal_moment_params if self.moments else make_temporal_params
        return make(demodulate=demodulate, **dict(self.params, **over))

    def accumulate(self, cam, frame, variance, aovs: dict, demodulate=None, out=None, out_variance=None, motion=None,
                   pixel_motion=None, **over):
        """One frame on NumPy arrays (yart_hip_temporal_accumulate_host, or _moments_host in the moments form). ``cam``: the frame's camera (a params dict as
        ``render`` takes it, or a CameraDesc); ``frame`` (H, W, 4); ``variance`` (H, W); ``aovs``: the feature buffers by name —
        position, normal, depth, coverage, ids, and albedo when demodulating (``demodulate`` None: whenever albedo is given).
        ``out`` / ``out_variance`` may be ``frame`` / ``variance``. ``motion``: this frame's per-node motion records
        (``set_motion`` is called first); None: whatever is pending. ``pixel_motion``: this frame's per-pixel records, an
        (H, W, 8) float32 array (``set_pixel_motion`` is called first; not together with ``motion``). Returns (accumulated frame,
        its variance, history length (H, W) uint32)."""
        h, w = self.height, self.width
        frame = np.ascontiguousarray(frame, np.float32)
        variance = np.ascontiguousarray(variance, np.float32)
        assert frame.shape == (h, w, 4) and variance.size == h * w
        if demodulate is None:
            demodulate = aovs.get("albedo") is not None
        ab, _keep = _buffer_struct(AovBuffers, AOVS, h, w, TEMPORAL_AOVS + (("albedo",) if demodulate else ()), host=aovs, required=False)
        if out is None:
            out = np.empty_like(frame)
        if out_variance is None:
            out_variance = np.empty((h, w), np.float32)
        for o, size in ((out, h * w * 4), (out_variance, h * w)):
            assert o.dtype == np.float32 and o.flags.c_contiguous and o.size == size
        length = np.empty((h, w), np.uint32)
        tp = self._params(demodulate, over)
        assert motion is None or pixel_motion is None, "one motion at a time: motion= or pixel_motion="
        if motion is not None:
            self.set_motion(motion)
        if pixel_motion is not None:
            assert isinstance(pixel_motion, np.ndarray), "accumulate: pixel_motion is host data (accumulate_into takes a device tensor)"
            pixel_motion = np.ascontiguousarray(pixel_motion)
            self.set_pixel_motion(pixel_motion)
        fn = self._L.yart_hip_temporal_accumulate_moments_host if self.moments else self._L.yart_hip_temporal_accumulate_host
        _check(fn(self._h, C.byref(self._camera(cam)), frame.ctypes.data_as(C.c_void_p), variance.ctypes.data_as(C.c_void_p),
                  C.byref(ab), C.byref(tp), out.ctypes.data_as(C.c_void_p), out_variance.ctypes.data_as(C.c_void_p),
                  length.ctypes.data_as(C.c_void_p)), self._L)
        return out, out_variance, length

    def accumulate_into(self, out_tensor, out_variance_tensor, out_length_tensor, cam, frame_tensor, variance_tensor,
                        aov_tensors: dict, demodulate=None, stream=None, motion=None, pixel_motion=None, **over):
        """``accumulate`` on CUDA/HIP torch tensors through ``data_ptr()`` (yart_hip_temporal_accumulate[_moments]_device), on ``stream``
        (an integer handle; None: torch's current stream): no host round trip. ``out_variance_tensor`` and
        ``out_length_tensor`` (H*W 4-byte elements: int32 holding the uint32) may be None; ``out_tensor`` may be
        ``frame_tensor`` and ``out_variance_tensor`` may be ``variance_tensor``. ``motion``: as ``accumulate`` takes it (a
        NumPy array: the records are host data). ``pixel_motion``: this frame's per-pixel records as a device tensor
        (``DeviceScene.pixel_motion_into``), written on ``stream`` or complete; not together with ``motion``."""
        import torch
        h, w = self.height, self.width
        if demodulate is None:
            demodulate = aov_tensors.get("albedo") is not None
        frame, out = (_device_tensor(t, what, numel=h * w * 4, dtype=torch.float32) for t, what in ((frame_tensor, "frame"), (out_tensor, "out")))
        variance, out_variance, out_length = (_device_tensor(t, what, numel=h * w, element_size=4, optional=True) for t, what in
                                              ((variance_tensor, "variance"), (out_variance_tensor, "out variance"), (out_length_tensor, "out length")))
        ab, _ = _buffer_struct(AovBuffers, AOVS, h, w, TEMPORAL_AOVS + (("albedo",) if demodulate else ()), device=aov_tensors, required=False)
        tp = self._params(demodulate, over)
        assert motion is None or pixel_motion is None, "one motion at a time: motion= or pixel_motion="
        if motion is not None:
            self.set_motion(motion)
        if pixel_motion is not None:
            assert not isinstance(pixel_motion, np.ndarray), "accumulate_into: pixel_motion is a device tensor"
            self.set_pixel_motion(pixel_motion)
        with torch.cuda.device(frame_tensor.device):
            fn = self._L.yart_hip_temporal_accumulate_moments_device if self.moments else self._L.yart_hip_temporal_accumulate_device
            _check(fn(self._h, C.byref(self._camera(cam)), frame, variance, C.byref(ab), C.byref(tp), out, out_variance, out_length,
                      _stream_of(stream, frame_tensor)), self._L)
        return out_tensor


class AutoExposure:
    """Auto-exposure for a sequence of frames (include/yart_hip.h: yart_hip_exposure_*), the stage after the denoiser: ``meter``
    builds a log-luminance histogram of a linear-HDR frame on the device and steps the exposure towards its target with eye-style
    adaptation over ``dt`` seconds; ``apply`` multiplies a frame by the gain, tonemaps it (AgX) and encodes it to 8 bits in one
    kernel. The state stays on the device (about 2 KB per handle). ``params``: yart_amd.exposure.DEFAULTS' names — ``ev_min``,
    ``ev_max``, ``trim_low``, ``trim_high``, ``key``, ``compensation_ev``, ``gain_ev_min``, ``gain_ev_max``, ``speed_up``,
    ``speed_down``, ``window`` (x0, y0, x1, y1) —, the parameters of every meter call. ``device`` < 0: the device current at the
    first frame. yart_amd.exposure.exposure_reference / apply_reference state the same arithmetic in NumPy."""

    def __init__(self, device: int = 0, **params):
        self._L = lib()
        self.device = int(device)
        self.params = exposure_params_of(**params)
        h = C.c_void_p()
        _check(self._L.yart_hip_exposure_create(self.device, C.byref(h)), self._L)
        self._h = h

    @property
    def handle(self):
        return self._h

    def close(self):
        if getattr(self, "_h", None):
            self._L.yart_hip_exposure_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reset(self):
        """Back to a new handle: the next ``meter`` snaps to its target; until then ``apply`` uses gain 1."""
        _check(self._L.yart_hip_exposure_reset(self._h), self._L)

    def meter(self, frame, dt):
        """Meter an (H, W, 4) float32 NumPy frame (yart_hip_exposure_meter_host) and step the state by ``dt`` seconds.
        Returns ``state()``."""
        frame = np.ascontiguousarray(frame, np.float32)
        h, w = frame.shape[:2]
        assert frame.shape == (h, w, 4)
        ep = make_exposure_params(**self.params)
        _check(self._L.yart_hip_exposure_meter_host(self._h, frame.ctypes.data_as(C.c_void_p), w, h, C.byref(ep), float(dt)), self._L)
        return self.state()

    def apply(self, frame, look="none"):
        """Gain, tonemap (``look``: None = no tonemapper, "none" / "golden" / "punchy") and 8-bit encoding of an (H, W, 4) float32
        NumPy frame (yart_hip_exposure_apply_host). Returns (ldr float32 (H, W, 4), rgb8 (H, W, 3))."""
        frame = np.ascontiguousarray(frame, np.float32)
        h, w = frame.shape[:2]
        assert frame.shape == (h, w, 4)
        ldr, rgb = np.empty_like(frame), np.empty((h, w, 3), np.uint8)
        _check(self._L.yart_hip_exposure_apply_host(self._h, frame.ctypes.data_as(C.c_void_p), w, h, look_index(look),
                                                    ldr.ctypes.data_as(C.c_void_p), rgb.ctypes.data_as(C.c_void_p)), self._L)
        return ldr, rgb

    def meter_into(self, frame_tensor, dt, stream=None):
        """``meter`` of an (H, W, 4) float32 CUDA/HIP torch tensor (yart_hip_exposure_meter_device) on ``stream`` (a raw
        hipStream_t), by default torch's current stream of the frame's device; returns after completion there. Nothing is
        copied to the host: read ``state()`` when it is wanted."""
        import torch
        t = frame_tensor
        h, w = int(t.shape[0]), int(t.shape[1])
        frame = _device_tensor(t, "frame", shape=(h, w, 4), dtype=torch.float32)
        ep = make_exposure_params(**self.params)
        with torch.cuda.device(t.device):
            _check(self._L.yart_hip_exposure_meter_device(self._h, frame, w, h, C.byref(ep), float(dt), _stream_of(stream, t)), self._L)

    def apply_into(self, ldr_tensor, rgb8_tensor, frame_tensor, look="none", stream=None):
        """``apply`` on torch tensors (yart_hip_exposure_apply_device): ``ldr_tensor`` (H, W, 4) float32 or None (it may be
        ``frame_tensor``), ``rgb8_tensor`` (H, W, 3) uint8 or None; not both None."""
        import torch
        t = frame_tensor
        h, w = int(t.shape[0]), int(t.shape[1])
        frame = _device_tensor(t, "frame", shape=(h, w, 4), dtype=torch.float32)
        ldr = _device_tensor(ldr_tensor, "ldr", shape=(h, w, 4), dtype=torch.float32, optional=True)
        rgb8 = _device_tensor(rgb8_tensor, "rgb8", shape=(h, w, 3), dtype=torch.uint8, optional=True)
        with torch.cuda.device(t.device):
            _check(self._L.yart_hip_exposure_apply_device(self._h, frame, w, h, look_index(look), ldr, rgb8, _stream_of(stream, t)), self._L)

    def state(self, histogram=False):
        """The state record as a dict (``cur_ev``, ``target_ev``, ``mean_ev``, ``gain`` as np.float32; ``n_counted``,
        ``n_ignored``, ``frames``, ``flags``); with ``histogram=True`` also ``"histogram"``: the last meter call's 256 bins."""
        rec = ExposureStateRecord(C.sizeof(ExposureStateRecord))
        hist = np.zeros(256, np.uint32) if histogram else None
        _check(self._L.yart_hip_exposure_get(self._h, C.byref(rec), None if hist is None else hist.ctypes.data_as(C.c_void_p)), self._L)
        d = {k: np.float32(getattr(rec, k)) for k in ("cur_ev", "target_ev", "mean_ev", "gain")}
        d.update({k: int(getattr(rec, k)) for k in ("n_counted", "n_ignored", "frames", "flags")})
        if histogram:
            d["histogram"] = hist
        return d


def probe_moments(L_samples, chunks=None, exposure_scale=1.0):
    """The moment kernels alone (yart_hip_probe_moments), without a scene: ``L_samples`` [n_pixels, spp, 3 or 4] float32
    per-sample radiance, ``chunks`` sample counts that sum to spp (one accumulate launch each, as a render launches one per
    wave; None: one chunk). Returns (mean [n, 3] float32, variance [n] float32, count [n] uint32)."""
    a = np.asarray(L_samples, np.float32)
    n, spp = a.shape[:2]
    rec = np.zeros((n, spp, 4), np.float32)
    rec[..., :3] = a[..., :3]
    ch = np.ascontiguousarray([spp] if chunks is None else chunks, np.uint32)
    mean, var, cnt = np.empty((n, 3), np.float32), np.empty(n, np.float32), np.empty(n, np.uint32)
    L = lib()
    _check(L.yart_hip_probe_moments(rec.ctypes.data_as(C.c_void_p), n, spp, ch.ctypes.data_as(C.c_void_p), len(ch),
                                    float(exposure_scale), mean.ctypes.data_as(C.c_void_p), var.ctypes.data_as(C.c_void_p),
                                    cnt.ctypes.data_as(C.c_void_p)), L)
    return mean, var, cnt


def probe_estimator(samples, kind, exposure_scale=1.0, rays=None, pixels=None, size=None, current=None, weights=(0.0, 1.0)):
    """The estimator kernel alone (yart_hip_probe_estimator: k_gmon_blend with the render's launch geometry), without a scene.
    ``samples`` [n_pixels, spp, 3] float32 per-sample radiance; ``kind`` 0..3 (YART_ESTIMATOR_*); ``rays`` [n_pixels, spp] uint32
    ray counts of the records (None: 0). ``pixels`` [n_pixels, 2] distinct (x, y) of a ``size`` = (width, height) frame (None:
    pixel i at (i % width, i / width); ``size`` None: an n_pixels x 1 frame). ``current`` [height, width, 4] float32 is the frame
    before the wave (None: zeros) and ``weights`` = (w_current, w_wave) of the blend. Returns (frame [height, width, 4] float32,
    pix_rays [n_pixels] uint32)."""
    a = np.asarray(samples, np.float32)
    n, spp = a.shape[:2]
    rec = np.zeros((n, spp, 4), np.float32)
    rec[..., :3] = a[..., :3]
    if rays is not None:
        rec.view(np.uint32)[..., 3] = np.asarray(rays, np.uint32).reshape(n, spp)
    w, h = (n, 1) if size is None else (int(size[0]), int(size[1]))
    px = None
    if pixels is not None:
        xy = np.asarray(pixels, np.uint32).reshape(n, 2)
        px = np.ascontiguousarray(xy[:, 0] | (xy[:, 1] << np.uint32(16)), np.uint32)
    frame = np.zeros((h, w, 4), np.float32) if current is None else np.array(current, np.float32, order="C").reshape(h, w, 4)
    pix_rays = np.empty(n, np.uint32)
    L = lib()
    _check(L.yart_hip_probe_estimator(rec.ctypes.data_as(C.c_void_p), n, spp, int(kind), float(exposure_scale),
                                      None if px is None else px.ctypes.data_as(C.c_void_p), w, h, float(weights[0]),
                                      float(weights[1]), frame.ctypes.data_as(C.c_void_p), pix_rays.ctypes.data_as(C.c_void_p)), L)
    return frame, pix_rays


def write_ppm(path, rgb8: np.ndarray):
    """P6 file as output/ppm.cpp:10 writes it."""
    h, w = rgb8.shape[:2]
    with open(path, "wb") as f:
        f.write(b"P6\n%d %d\n255\n" % (w, h))
        f.write(np.ascontiguousarray(rgb8, np.uint8).tobytes())
