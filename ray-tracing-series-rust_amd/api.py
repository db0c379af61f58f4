"""ctypes binding of include/rtx_abi.h plus a host-side mirror of the reference's scene API.

The reference's host code is Rust; neither Rust nor a Rust binding can be built in this image,
so the compiled-language mirror lives in C++ (csrc/host, apps/rtx_render.cpp) and this module
is the Python face of the same C ABI: same names, same argument orders as the reference's
constructors (src/hit.rs, src/texture.rs, src/camera.rs, src/world.rs), so tests read like the
reference's own call sites.

There is no CPU render path here: if the HIP library is missing this module raises at import;
if no GPU is present, upload/render raise RtxError(RTX_EHIP).
"""
import ctypes as C
import os
import re
import sys

import numpy as np

_PKG_DIR = os.path.dirname(os.path.abspath(__file__))
# RTX_LIBRARY: another build of the same library (scripts/ab_builds.sh: two builds timed in one session on one GPU)
_LIB_PATH = os.environ.get("RTX_LIBRARY") or os.path.join(_PKG_DIR, "lib", "librtx_hip.so")

RTX_OK, RTX_EINVAL, RTX_ENOMEM, RTX_EHIP, RTX_EUNSUPPORTED, RTX_EIO, RTX_ENCCL = 0, 1, 2, 3, 4, 5, 6
_STATUS_NAMES = {0: "RTX_OK", 1: "RTX_EINVAL", 2: "RTX_ENOMEM", 3: "RTX_EHIP", 4: "RTX_EUNSUPPORTED", 5: "RTX_EIO", 6: "RTX_ENCCL"}

SCENE_CHECKERED_SPHERES, SCENE_TWO_PERLIN, SCENE_EARTH, SCENE_SIMPLE_LIGHT = 0, 1, 2, 3
SCENE_CORNELL_BOX, SCENE_CORNELL_SMOKE, SCENE_BOOK2_FINAL, SCENE_MOVING_TEST = 4, 5, 6, 7
SCENE_RANDOM_MOVING, SCENE_BENCHMARK_TEST, SCENE_TRIANGLE_TEST, SCENE_STANFORD_DRAGON = 8, 9, 10, 11
SCENE_TRIANGULAR_PRISM, SCENE_BOOK1_HEAD, SCENE_BOOK1_CANONICAL, SCENE_EMPTY = 12, 13, 100, 101


class RtxError(RuntimeError):
    def __init__(self, status, message):
        super().__init__("%s: %s" % (_STATUS_NAMES.get(status, status), message))
        self.status = status


class RtxCamera(C.Structure):
    _fields_ = [(n, C.c_double * 3) for n in ("origin", "lower_left_corner", "horizontal", "vertical", "u", "v", "w")] + \
               [("lens_radius", C.c_double), ("time1", C.c_double), ("time2", C.c_double)]


class RtxConfig(C.Structure):
    _fields_ = [("aspect_ratio", C.c_double), ("image_width", C.c_int32), ("samples_per_pixel", C.c_int32),
                ("max_depth", C.c_int32), ("threads", C.c_int32), ("seed", C.c_uint64),
                ("background", C.c_double * 3), ("row_chunk_compat", C.c_int32), ("reserved", C.c_int32),
                ("sample_buffer_bytes", C.c_uint64)]


class RtxSceneOptions(C.Structure):
    _fields_ = [("camera_aspect", C.c_double), ("earth_ppm", C.c_char_p), ("dragon_ply", C.c_char_p),
                ("mesh_triangles", C.c_int64), ("book2_boxes_per_side", C.c_int32), ("book2_spheres", C.c_int32)]


class RtxBuildOptions(C.Structure):
    _fields_ = [("max_leaf", C.c_int32), ("sah_bins", C.c_int32), ("reference_bvh", C.c_int32), ("gpu_builder", C.c_int32),
                ("bvh_seed", C.c_uint64)]


class RtxFlatInfo(C.Structure):
    _fields_ = [(n, C.c_int64) for n in ("n_spheres", "n_moving_spheres", "n_rects", "n_triangles", "n_nodes",
                                         "n_refs", "n_entries", "n_top_level", "n_materials", "n_textures",
                                         "n_perlins", "n_images", "n_texels", "total_bytes")] + \
               [("max_stack", C.c_int32), ("n_bvh", C.c_int32), ("sah_cost", C.c_double), ("bvh_build_ms", C.c_double),
                ("bvh_device_ms", C.c_double), ("n_gravity_spheres", C.c_int64)]


class RtxFrame(C.Structure):
    _fields_ = [("accum_rgb", C.POINTER(C.c_double)), ("rgb8", C.POINTER(C.c_uint8))]


class RtxRenderStats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("samples", "rays", "box_tests", "sphere_tests", "moving_sphere_tests",
                                          "rect_tests", "triangle_tests", "scatters", "texels", "perlin_calls")] + \
               [("trace_ms", C.c_double), ("reduce_ms", C.c_double), ("tonemap_ms", C.c_double),
                ("trace_launches", C.c_int32), ("passes", C.c_int32), ("sample_buffer_bytes", C.c_uint64),
                ("trace_kernel", C.c_int32), ("trace_variant", C.c_int32)]


class RtxMultiStats(C.Structure):
    _fields_ = [("render_ms_max", C.c_double), ("total_ms", C.c_double), ("gathered_bytes", C.c_uint64),
                ("n_shards", C.c_int32), ("n_devices", C.c_int32), ("used_rccl", C.c_int32), ("rccl_ranks", C.c_int32),
                ("gather_ms", C.c_double), ("render_ms", C.c_double * 16)]


class RtxShard(C.Structure):
    _fields_ = [("shard_index", C.c_int32), ("shard_count", C.c_int32), ("block_rows", C.c_int32), ("reserved", C.c_int32)]


class RtxNoiseStats(C.Structure):
    _fields_ = [("spp_done", C.c_int32), ("pixels", C.c_int32), ("pixels_above", C.c_int32), ("reserved", C.c_int32),
                ("max_rel_err", C.c_double), ("mean_rel_err", C.c_double), ("target_rel_err", C.c_double)]


class RtxAdaptiveStats(C.Structure):
    _fields_ = [("spp_done", C.c_int32), ("min_spp", C.c_int32), ("pixels", C.c_int32), ("pixels_active", C.c_int32),
                ("pixels_above", C.c_int32), ("reserved", C.c_int32), ("samples", C.c_uint64),
                ("max_rel_err", C.c_double), ("mean_rel_err", C.c_double), ("target_rel_err", C.c_double)]


class RtxDenoiseParams(C.Structure):
    _fields_ = [("iterations", C.c_int32), ("feature_spp", C.c_int32), ("demodulate", C.c_int32), ("reserved", C.c_int32),
                ("sigma_luminance", C.c_double), ("sigma_normal", C.c_double), ("sigma_albedo", C.c_double)]


class RtxIntegratorOptions(C.Structure):
    _fields_ = [("light_sampling", C.c_int32), ("reserved", C.c_int32 * 3)]


class RtxLightInfo(C.Structure):
    _fields_ = [("n_lights", C.c_int32), ("n_rect_lights", C.c_int32), ("n_sphere_lights", C.c_int32),
                ("n_unsampled_emitters", C.c_int32), ("total_area", C.c_double)]


class RtxInstanceInfo(C.Structure):
    _fields_ = [("n_trees", C.c_int32), ("n_members", C.c_int32), ("n_nodes", C.c_int32), ("max_depth", C.c_int32)]


class RtxRayBatch(C.Structure):
    _fields_ = [("n", C.c_int64), ("origin", C.c_void_p), ("direction", C.c_void_p), ("time", C.c_void_p),
                ("t_max", C.c_void_p), ("t_min", C.c_double), ("t_max_all", C.c_double), ("seed", C.c_uint64),
                ("stream_step", C.c_uint64)]


class RtxRayHits(C.Structure):
    _fields_ = [("t", C.c_void_p), ("p", C.c_void_p), ("normal", C.c_void_p), ("uv", C.c_void_p), ("ids", C.c_void_p)]


class RtxRadianceRays(C.Structure):
    _fields_ = [("n", C.c_int64), ("origin", C.c_void_p), ("direction", C.c_void_p), ("time", C.c_void_p),
                ("first_ray", C.c_uint64), ("first_sample", C.c_uint32), ("samples", C.c_int32), ("max_depth", C.c_int32),
                ("accumulate", C.c_int32), ("seed", C.c_uint64), ("background", C.c_double * 3),
                ("light_sampling", C.c_int32), ("reserved", C.c_int32), ("sample_buffer_bytes", C.c_uint64)]


class RtxGatherPoints(C.Structure):
    _fields_ = [("n", C.c_int64), ("position", C.c_void_p), ("normal", C.c_void_p), ("time", C.c_void_p),
                ("first_point", C.c_uint64), ("first_sample", C.c_uint32), ("samples", C.c_int32), ("max_depth", C.c_int32),
                ("accumulate", C.c_int32), ("seed", C.c_uint64), ("background", C.c_double * 3),
                ("light_sampling", C.c_int32), ("sh_order", C.c_int32), ("sample_buffer_bytes", C.c_uint64),
                ("reserved", C.c_int32 * 2)]


class RtxPointBatch(C.Structure):
    _fields_ = [("n", C.c_int64), ("points", C.c_void_p), ("time", C.c_void_p), ("r_max", C.c_void_p),
                ("r_max_all", C.c_double), ("media", C.c_int32), ("reserved", C.c_int32)]


class RtxNearest(C.Structure):
    _fields_ = [("d", C.c_void_p), ("q", C.c_void_p), ("ids", C.c_void_p)]


class _RtxSlotOp(C.Structure):
    _fields_ = [("op", C.c_int32), ("pad", C.c_int32), ("v", C.c_double * 3)]


class RtxSlotOps(C.Structure):
    _fields_ = [("slot", C.c_int32), ("n_ops", C.c_int32), ("ops", _RtxSlotOp * 4)]


class RtxInstanceTree(C.Structure):
    _fields_ = [("first_slot", C.c_int32), ("n_slots", C.c_int32), ("n_nodes", C.c_int32), ("depth", C.c_int32)]


class RtxRebuildStats(C.Structure):
    _fields_ = [("trees_rebuilt", C.c_int32), ("max_depth", C.c_int32), ("max_stack_before", C.c_int32), ("max_stack_after", C.c_int32),
                ("reserved", C.c_int32 * 4)]


class RtxShadingEdit(C.Structure):
    _fields_ = [("what", C.c_int32), ("index", C.c_int32), ("v", C.c_double * 4)]


class RtxMaterialInfo(C.Structure):
    _fields_ = [("kind", C.c_int32), ("tex", C.c_int32), ("albedo", C.c_double * 3), ("param", C.c_double)]


class RtxTextureInfo(C.Structure):
    _fields_ = [("kind", C.c_int32), ("a", C.c_int32), ("b", C.c_int32), ("pad", C.c_int32), ("color", C.c_double * 3),
                ("scale", C.c_double)]


class RtxMediumInfo(C.Structure):
    _fields_ = [("material", C.c_int32), ("pad", C.c_int32), ("neg_inv_density", C.c_double)]


RTX_SHADE_SOLID_COLOR, RTX_SHADE_NOISE_SCALE, RTX_SHADE_METAL, RTX_SHADE_DIELECTRIC, RTX_SHADE_MEDIUM_DENSITY = 0, 1, 2, 3, 4
_SHADE_NAMES = ("solid_color", "noise_scale", "metal", "dielectric", "medium_density")
RTX_MAT_LAMBERTIAN, RTX_MAT_METAL, RTX_MAT_DIELECTRIC, RTX_MAT_DIFFUSE_LIGHT, RTX_MAT_ISOTROPIC = 0, 1, 2, 3, 4
MATERIAL_KINDS = ("lambertian", "metal", "dielectric", "diffuse_light", "isotropic")
RTX_TEX_SOLID, RTX_TEX_CHECKER, RTX_TEX_NOISE, RTX_TEX_IMAGE = 0, 1, 2, 3
TEXTURE_KINDS = ("solid_color", "checker", "noise", "image")
RTX_REBUILD_MORTON, RTX_REBUILD_SAH = 0, 1
_REBUILD_NAMES = ("morton", "sah")
RTX_XFORM_TRANSLATE, RTX_XFORM_ROTATE_Y = 0, 1
_XFORM_NAMES = ("translate", "rotate_y")
# rtx_flat_array / rtx_device_scene_array: `which` and the element size in an f64 and in an f32 scene
SCENE_ARRAYS = {"entries": (0, 160, 104), "nodes": (1, 112, 64), "nodes32": (2, 64, 64), "motion32": (3, 96, 96),
                "world_desc": (4, 192, 136), "top_level": (5, 4, 4), "member_local_box": (6, 8, 8), "nodes4": (7, 128, 128),
                "triangles": (10, 104, 56), "top_box32": (11, 4, 4), "triangle_id": (12, 4, 4), "spheres": (13, 40, 24),
                "lights": (14, 40, 40), "materials": (15, 48, 32), "textures": (16, 48, 32), "moving_spheres": (17, 80, 44),
                "rects": (19, 48, 28)}

RTX_KERNEL_RAYS = 9  # RtxRenderStats.trace_kernel of a radiance query (k_trace_rays)
# RtxRenderStats.trace_variant: which k_trace_lds ran (0 for every other kernel)
RTX_LDS_VARIANT_TIME_BOXES, RTX_LDS_VARIANT_ONE_AXIS, RTX_LDS_VARIANT_COMMON_RATIO = 1, 2, 4
RAY_COLUMNS = ("t", "p", "normal", "uv", "ids")  # the columns of RtxRayHits, in its order
NEAREST_COLUMNS = ("d", "q", "ids")  # the columns of RtxNearest, in its order


def _integrator_options(light_sampling):
    return RtxIntegratorOptions(1 if light_sampling else 0)


# Every symbol include/rtx_abi.h declares: (restype, argtypes).  tests/test_abi_symbols.py checks
# this table against the header and against the loaded library.
_D3 = C.POINTER(C.c_double)
_F3 = C.POINTER(C.c_float)
_VP = C.c_void_p
_H = C.c_int32
ABI = {
    "rtx_abi_version": (C.c_int32, []),
    "rtx_last_error": (C.c_char_p, []),
    "rtx_trace_kernel_name": (C.c_char_p, [C.c_int32]),
    "rtx_builder_create": (C.c_int32, [C.c_uint64, C.POINTER(_VP)]),
    "rtx_builder_destroy": (None, [_VP]),
    "rtx_builder_random": (C.c_double, [_VP]),
    "rtx_solid_color": (_H, [_VP, _D3]),
    "rtx_checker": (_H, [_VP, _H, _H]),
    "rtx_noise": (_H, [_VP, C.c_double]),
    "rtx_image_from_ppm": (_H, [_VP, C.c_char_p]),
    "rtx_image_from_texels": (_H, [_VP, C.c_int32, C.c_int32, _D3]),
    "rtx_lambertian": (_H, [_VP, _H]),
    "rtx_metal": (_H, [_VP, _D3, C.c_double]),
    "rtx_dielectric": (_H, [_VP, C.c_double]),
    "rtx_diffuse_light": (_H, [_VP, _H]),
    "rtx_isotropic": (_H, [_VP, _H]),
    "rtx_sphere": (_H, [_VP, _D3, C.c_double, _H]),
    "rtx_moving_sphere": (_H, [_VP, _D3, _D3, C.c_double, C.c_double, C.c_double, _H]),
    "rtx_triangle": (_H, [_VP, _D3, _D3, _D3, _H]),
    "rtx_gravity_sphere": (_H, [_VP, _D3, C.c_double, C.c_double, _H]),
    "rtx_render_scene_with_time": (C.c_int32, [_VP, C.c_double, C.c_double, C.c_char_p, C.c_int32, C.POINTER(RtxConfig)]),
    "rtx_xy_rect": (_H, [_VP] + [C.c_double] * 5 + [_H]),
    "rtx_xz_rect": (_H, [_VP] + [C.c_double] * 5 + [_H]),
    "rtx_yz_rect": (_H, [_VP] + [C.c_double] * 5 + [_H]),
    "rtx_rect_prism": (_H, [_VP, _D3, _D3, _H]),
    "rtx_hittable_list_new": (_H, [_VP]),
    "rtx_hittable_list_add": (C.c_int32, [_VP, _H, _H]),
    "rtx_bvh_from_list": (_H, [_VP, _H, C.c_double, C.c_double]),
    "rtx_instance_bvh_from_list": (_H, [_VP, _H]),
    "rtx_translate": (_H, [_VP, _D3, _H]),
    "rtx_rotate_y": (_H, [_VP, C.c_double, _H]),
    "rtx_constant_medium": (_H, [_VP, _D3, C.c_double, _H]),
    "rtx_triangle_model": (_H, [_VP, C.c_char_p, C.c_double]),
    "rtx_triangle_mesh": (_H, [_VP, _D3, C.c_int64, C.POINTER(C.c_int64), C.c_int64, _H]),
    "rtx_camera_new": (C.c_int32, [_D3, _D3, _D3] + [C.c_double] * 6 + [C.POINTER(RtxCamera)]),
    "rtx_config_new": (C.c_int32, [C.c_double, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(RtxConfig)]),
    "rtx_image_height": (C.c_int32, [C.POINTER(RtxConfig)]),
    "rtx_flat_top_level_kind": (C.c_int32, [_VP, C.c_int32]),
    "rtx_scene_trim": (C.c_int32, [_VP]),
    "rtx_multi_create": (C.c_int32, [_VP, C.c_int32, C.POINTER(C.c_int32), C.c_int32, C.POINTER(_VP)]),
    "rtx_multi_create_f32": (C.c_int32, [_VP, C.c_int32, C.POINTER(C.c_int32), C.c_int32, C.POINTER(_VP)]),
    "rtx_multi_destroy": (None, [_VP]),
    "rtx_multi_render": (C.c_int32, [_VP, C.POINTER(RtxCamera), C.POINTER(RtxConfig), C.POINTER(RtxFrame), C.POINTER(RtxMultiStats)]),
    "rtx_render_multi": (C.c_int32, [_VP, C.POINTER(RtxCamera), C.POINTER(RtxConfig), C.c_int32, C.POINTER(RtxFrame)]),
    "rtx_get_world_cam": (C.c_int32, [_VP, C.c_int32, C.POINTER(RtxSceneOptions), C.POINTER(_H), C.POINTER(RtxCamera), _D3]),
    "rtx_flatten": (C.c_int32, [_VP, _H, C.POINTER(RtxBuildOptions), C.POINTER(_VP)]),
    "rtx_flat_destroy": (None, [_VP]),
    "rtx_flat_info": (C.c_int32, [_VP, C.POINTER(RtxFlatInfo)]),
    "rtx_scene_upload": (C.c_int32, [_VP, C.POINTER(_VP)]),
    "rtx_scene_upload_f32": (C.c_int32, [_VP, C.POINTER(_VP)]),
    "rtx_scene_is_f32": (C.c_int32, [_VP]),
    "rtx_scene_destroy": (None, [_VP]),
    "rtx_render": (C.c_int32, [_VP, C.POINTER(RtxCamera), C.POINTER(RtxConfig), C.POINTER(RtxFrame)]),
    "rtx_shard_rows": (C.c_int32, [C.POINTER(RtxConfig), C.POINTER(RtxShard)]),
    "rtx_render_device": (C.c_int32, [_VP, C.POINTER(RtxCamera), C.POINTER(RtxConfig), C.POINTER(RtxShard),
                                      _VP, _VP, _VP, C.POINTER(RtxRenderStats)]),
    "rtx_render_count": (C.c_int32, [_VP, C.POINTER(RtxCamera), C.POINTER(RtxConfig), C.POINTER(RtxShard),
                                     C.POINTER(RtxRenderStats)]),
    "rtx_write_ppm": (C.c_int32, [C.c_char_p, C.c_int32, C.c_int32, C.POINTER(C.c_uint8)]),
    "rtx_device_math": (C.c_int32, [C.c_int32, _D3, _D3, C.c_int64, _D3]),
    "rtx_device_stream": (C.c_int32, [C.c_uint64, C.c_uint64, C.c_uint32, C.c_int32, _D3]),
    "rtx_device_cull_verdicts": (C.c_int32, [C.c_int32, C.c_int64, _D3, _D3, _F3, _F3, C.POINTER(C.c_uint32)]),
    "rtx_device_walk_steps": (C.c_int32, [C.c_int32, C.c_int32, C.c_int32, _VP, C.c_int64, C.c_int32, C.c_int64, _VP, C.POINTER(C.c_int32)]),
    "rtx_device_retire": (C.c_int32, [_D3, _D3, C.c_uint32, C.POINTER(C.c_uint32), C.c_uint32, C.c_uint32, C.c_double,
                                      C.POINTER(C.c_int32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "rtx_device_noise_reduce": (C.c_int32, [_D3, _D3, C.POINTER(C.c_int32), C.c_uint32, C.c_uint32, C.c_double, _D3, _D3,
                                            C.POINTER(C.c_uint64)]),
    "rtx_progressive_create": (C.c_int32, [_VP, C.POINTER(RtxCamera), C.POINTER(RtxConfig), C.POINTER(RtxShard), C.POINTER(_VP)]),
    "rtx_progressive_destroy": (None, [_VP]),
    "rtx_progressive_spp": (C.c_int32, [_VP]),
    "rtx_progressive_add": (C.c_int32, [_VP, C.c_int32, _VP, C.POINTER(RtxRenderStats)]),
    "rtx_progressive_read": (C.c_int32, [_VP, C.POINTER(RtxFrame), _D3]),
    "rtx_progressive_stats": (C.c_int32, [_VP, C.c_double, C.POINTER(RtxNoiseStats)]),
    "rtx_progressive_until": (C.c_int32, [_VP, C.c_int32, C.c_double, C.POINTER(RtxNoiseStats)]),
    "rtx_progressive_add_adaptive": (C.c_int32, [_VP, C.c_int32, C.c_int32, C.c_double, _VP, C.POINTER(RtxRenderStats)]),
    "rtx_progressive_until_adaptive": (C.c_int32, [_VP, C.c_int32, C.c_int32, C.c_double, C.POINTER(RtxAdaptiveStats)]),
    "rtx_progressive_pixel_spp": (C.c_int32, [_VP, C.POINTER(C.c_int32)]),
    "rtx_progressive_features": (C.c_int32, [_VP, C.c_int32, _F3, _F3]),
    "rtx_progressive_denoise": (C.c_int32, [_VP, C.POINTER(RtxDenoiseParams), _D3, C.POINTER(C.c_uint8)]),
    "rtx_device_denoise": (C.c_int32, [_D3, _D3, _F3, _F3, C.c_int32, C.c_int32, C.POINTER(RtxDenoiseParams), _D3,
                                       C.POINTER(C.c_uint8)]),
    "rtx_flat_lights": (C.c_int32, [_VP, C.POINTER(RtxLightInfo)]),
    "rtx_flat_instances": (C.c_int32, [_VP, C.POINTER(RtxInstanceInfo)]),
    "rtx_render_ex": (C.c_int32, [_VP, C.POINTER(RtxCamera), C.POINTER(RtxConfig), C.POINTER(RtxIntegratorOptions),
                                  C.POINTER(RtxFrame), C.POINTER(RtxRenderStats)]),
    "rtx_progressive_create_ex": (C.c_int32, [_VP, C.POINTER(RtxCamera), C.POINTER(RtxConfig), C.POINTER(RtxShard),
                                              C.POINTER(RtxIntegratorOptions), C.POINTER(_VP)]),
    "rtx_ray_batch_defaults": (None, [C.POINTER(RtxRayBatch)]),
    "rtx_scene_cast_rays": (C.c_int32, [_VP, C.POINTER(RtxRayBatch), C.POINTER(RtxRayHits)]),
    "rtx_scene_cast_rays_device": (C.c_int32, [_VP, C.POINTER(RtxRayBatch), C.POINTER(RtxRayHits), _VP]),
    "rtx_scene_occlusion": (C.c_int32, [_VP, C.POINTER(RtxRayBatch), _VP]),
    "rtx_scene_occlusion_device": (C.c_int32, [_VP, C.POINTER(RtxRayBatch), _VP, _VP]),
    "rtx_radiance_rays_defaults": (None, [C.POINTER(RtxRadianceRays)]),
    "rtx_scene_trace_rays": (C.c_int32, [_VP, C.POINTER(RtxRadianceRays), _VP, _VP, C.POINTER(RtxRenderStats)]),
    "rtx_scene_trace_rays_device": (C.c_int32, [_VP, C.POINTER(RtxRadianceRays), _VP, _VP, _VP, C.POINTER(RtxRenderStats)]),
    "rtx_gather_points_defaults": (None, [C.POINTER(RtxGatherPoints)]),
    "rtx_scene_gather": (C.c_int32, [_VP, C.POINTER(RtxGatherPoints), _VP, _VP, C.POINTER(RtxRenderStats)]),
    "rtx_scene_gather_device": (C.c_int32, [_VP, C.POINTER(RtxGatherPoints), _VP, _VP, _VP, C.POINTER(RtxRenderStats)]),
    "rtx_gather_directions": (C.c_int32, [C.POINTER(RtxGatherPoints), C.c_int32, _VP]),
    "rtx_point_batch_defaults": (None, [C.POINTER(RtxPointBatch)]),
    "rtx_scene_nearest": (C.c_int32, [_VP, C.POINTER(RtxPointBatch), C.POINTER(RtxNearest)]),
    "rtx_scene_nearest_device": (C.c_int32, [_VP, C.POINTER(RtxPointBatch), C.POINTER(RtxNearest), _VP]),
    "rtx_flat_slot_chain": (C.c_int32, [_VP, C.c_int32, C.POINTER(C.c_int32)]),
    "rtx_flat_instance_tree": (C.c_int32, [_VP, C.c_int32, C.POINTER(RtxInstanceTree)]),
    "rtx_flat_set_transforms": (C.c_int32, [_VP, C.POINTER(RtxSlotOps), C.c_int64]),
    "rtx_scene_set_transforms": (C.c_int32, [_VP, C.POINTER(RtxSlotOps), C.c_int64, _VP]),
    "rtx_flat_instance_tree_cost": (C.c_int32, [_VP, C.c_int32, C.POINTER(C.c_double)]),
    "rtx_scene_instance_tree_cost": (C.c_int32, [_VP, C.c_int32, C.POINTER(C.c_double)]),
    "rtx_flat_rebuild_instance_trees": (C.c_int32, [_VP, C.POINTER(C.c_int32), C.c_int32, C.c_int32]),
    "rtx_scene_rebuild_instance_trees": (C.c_int32, [_VP, C.POINTER(C.c_int32), C.c_int32, _VP, C.POINTER(RtxRebuildStats)]),
    "rtx_flat_triangle_ids": (C.c_int64, [_VP, _VP, _H, C.POINTER(C.c_int32), C.c_int64]),
    "rtx_flat_set_triangles": (C.c_int32, [_VP, C.POINTER(C.c_int32), C.c_int64, _D3]),
    "rtx_scene_set_triangles": (C.c_int32, [_VP, C.POINTER(C.c_int32), C.c_int64, _D3, _VP]),
    "rtx_scene_set_triangles_device": (C.c_int32, [_VP, C.POINTER(C.c_int32), C.c_int64, _VP, _VP]),
    "rtx_flat_sphere_ids": (C.c_int64, [_VP, _VP, _H, C.POINTER(C.c_int32), C.c_int64]),
    "rtx_flat_set_spheres": (C.c_int32, [_VP, C.POINTER(C.c_int32), C.c_int64, _D3]),
    "rtx_scene_set_spheres": (C.c_int32, [_VP, C.POINTER(C.c_int32), C.c_int64, _D3, _VP]),
    "rtx_scene_set_spheres_device": (C.c_int32, [_VP, C.POINTER(C.c_int32), C.c_int64, _VP, _VP]),
    "rtx_flat_moving_sphere_ids": (C.c_int64, [_VP, _VP, _H, C.POINTER(C.c_int32), C.c_int64]),
    "rtx_flat_set_moving_spheres": (C.c_int32, [_VP, C.POINTER(C.c_int32), C.c_int64, _D3]),
    "rtx_scene_set_moving_spheres": (C.c_int32, [_VP, C.POINTER(C.c_int32), C.c_int64, _D3, _VP]),
    "rtx_scene_set_moving_spheres_device": (C.c_int32, [_VP, C.POINTER(C.c_int32), C.c_int64, _VP, _VP]),
    "rtx_flat_rect_ids": (C.c_int64, [_VP, _VP, _H, C.POINTER(C.c_int32), C.c_int64]),
    "rtx_flat_set_rects": (C.c_int32, [_VP, C.POINTER(C.c_int32), C.c_int64, _D3]),
    "rtx_scene_set_rects": (C.c_int32, [_VP, C.POINTER(C.c_int32), C.c_int64, _D3, _VP]),
    "rtx_scene_set_rects_device": (C.c_int32, [_VP, C.POINTER(C.c_int32), C.c_int64, _VP, _VP]),
    "rtx_flat_material_info": (C.c_int32, [_VP, C.c_int32, C.POINTER(RtxMaterialInfo)]),
    "rtx_flat_texture_info": (C.c_int32, [_VP, C.c_int32, C.POINTER(RtxTextureInfo)]),
    "rtx_flat_medium_info": (C.c_int32, [_VP, C.c_int32, C.POINTER(RtxMediumInfo)]),
    "rtx_flat_set_shading": (C.c_int32, [_VP, C.POINTER(RtxShadingEdit), C.c_int64]),
    "rtx_scene_set_shading": (C.c_int32, [_VP, C.POINTER(RtxShadingEdit), C.c_int64, _VP]),
    "rtx_device_scene_array": (C.c_int32, [_VP, C.c_int32, _VP, C.c_size_t]),
    "rtx_flat_array": (C.c_int32, [_VP, C.c_int32, _VP, C.c_size_t]),
    "rtx_builder_graph": (_VP, [_VP]),
    "rtx_flat_arrays": (_VP, [_VP]),
}


def _load():
    if not os.path.exists(_LIB_PATH):
        raise ImportError(
            "HIP library %s is missing: run `python __graft_entry__.py` (or ray-tracing-series-rust_amd/build.py). "
            "This package has no CPU fallback." % _LIB_PATH)
    lib = C.CDLL(_LIB_PATH)
    for name, (res, args) in ABI.items():
        fn = getattr(lib, name)  # AttributeError here = library/header drift: fail loudly
        fn.restype = res
        fn.argtypes = args
    return lib


lib = _load()
LIB_PATH = _LIB_PATH


def last_error():
    return (lib.rtx_last_error() or b"").decode("utf-8", "replace")


def _check(status):
    if status != RTX_OK:
        raise RtxError(status, last_error())


def _v3(v):
    a = (C.c_double * 3)(float(v[0]), float(v[1]), float(v[2]))
    return a


def _handle(h):
    if h < 0:
        raise RtxError(RTX_EINVAL, last_error())
    return h


class Camera:
    """Camera::new(lookfrom, lookat, vup, vfov, aspect_ratio, aperture, focus_dist, time1, time2) -- camera.rs:20-57"""

    @staticmethod
    def new(lookfrom, lookat, vup, vfov, aspect_ratio, aperture, focus_dist, time1, time2):
        cam = RtxCamera()
        _check(lib.rtx_camera_new(_v3(lookfrom), _v3(lookat), _v3(vup), vfov, aspect_ratio, aperture, focus_dist,
                                  time1, time2, C.byref(cam)))
        return cam


class Config:
    """Config::new(aspect_ratio, image_width, samples_per_pixel, max_depth, threads) -- world.rs:29-50"""

    @staticmethod
    def new(aspect_ratio, image_width, samples_per_pixel, max_depth, threads, seed=1, background=(0.7, 0.8, 1.0),
            row_chunk_compat=False, sample_buffer_bytes=0):
        cfg = RtxConfig()
        _check(lib.rtx_config_new(aspect_ratio, image_width, samples_per_pixel, max_depth, threads, C.byref(cfg)))
        cfg.seed = seed
        cfg.background[0], cfg.background[1], cfg.background[2] = background
        cfg.row_chunk_compat = 1 if row_chunk_compat else 0
        cfg.sample_buffer_bytes = sample_buffer_bytes
        return cfg


def image_height(cfg):
    return lib.rtx_image_height(C.byref(cfg))


class Builder:
    """Scene construction: one method per reference constructor (argument order kept)."""

    def __init__(self, scene_seed=1):
        p = _VP()
        _check(lib.rtx_builder_create(scene_seed, C.byref(p)))
        self._p = p

    def __del__(self):
        p, self._p = getattr(self, "_p", None), None
        if p:
            lib.rtx_builder_destroy(p)

    @property
    def ptr(self):
        return self._p

    def graph_ptr(self):
        return lib.rtx_builder_graph(self._p)

    def random(self):
        return lib.rtx_builder_random(self._p)

    # textures (texture.rs)
    def solid_color(self, rgb):
        return _handle(lib.rtx_solid_color(self._p, _v3(rgb)))

    def checker(self, even, odd):
        return _handle(lib.rtx_checker(self._p, even, odd))

    def checker_from_colors(self, even_rgb, odd_rgb):  # Checker::from_colors, texture.rs:46-51
        return self.checker(self.solid_color(even_rgb), self.solid_color(odd_rgb))

    def noise(self, scale):
        return _handle(lib.rtx_noise(self._p, scale))

    def image_from_ppm(self, path):
        return _handle(lib.rtx_image_from_ppm(self._p, os.fsencode(path)))

    def image_from_texels(self, texels):
        t = np.ascontiguousarray(texels, dtype=np.float64)
        h, w = t.shape[0], t.shape[1]
        return _handle(lib.rtx_image_from_texels(self._p, w, h, t.ctypes.data_as(_D3)))

    # materials (hit.rs:992-1152)
    def lambertian(self, albedo):
        """Lambertian::new(color) when given an rgb triple, Lambertian::from_pointer(texture) for a handle."""
        tex = albedo if isinstance(albedo, int) else self.solid_color(albedo)
        return _handle(lib.rtx_lambertian(self._p, tex))

    def metal(self, albedo, fuzz):
        return _handle(lib.rtx_metal(self._p, _v3(albedo), fuzz))

    def dielectric(self, ir):
        return _handle(lib.rtx_dielectric(self._p, ir))

    def diffuse_light(self, emit):
        tex = emit if isinstance(emit, int) else self.solid_color(emit)
        return _handle(lib.rtx_diffuse_light(self._p, tex))

    def isotropic(self, albedo):
        tex = albedo if isinstance(albedo, int) else self.solid_color(albedo)
        return _handle(lib.rtx_isotropic(self._p, tex))

    # hittables (hit.rs, bvh.rs, model.rs)
    def sphere(self, center, radius, mat):
        return _handle(lib.rtx_sphere(self._p, _v3(center), radius, mat))

    def moving_sphere(self, center0, center1, time0, time1, radius, mat):
        return _handle(lib.rtx_moving_sphere(self._p, _v3(center0), _v3(center1), time0, time1, radius, mat))

    def gravity_sphere(self, start, time0, radius, mat):  # GravitySphere::new, hit.rs:340-367
        return _handle(lib.rtx_gravity_sphere(self._p, _v3(start), time0, radius, mat))

    def triangle(self, v0, v1, v2, mat):
        return _handle(lib.rtx_triangle(self._p, _v3(v0), _v3(v1), _v3(v2), mat))

    def xy_rect(self, x0, x1, y0, y1, k, mat):
        return _handle(lib.rtx_xy_rect(self._p, x0, x1, y0, y1, k, mat))

    def xz_rect(self, x0, x1, y0, y1, k, mat):
        return _handle(lib.rtx_xz_rect(self._p, x0, x1, y0, y1, k, mat))

    def yz_rect(self, x0, x1, y0, y1, k, mat):
        return _handle(lib.rtx_yz_rect(self._p, x0, x1, y0, y1, k, mat))

    def rect_prism(self, p0, p1, mat):
        return _handle(lib.rtx_rect_prism(self._p, _v3(p0), _v3(p1), mat))

    def hittable_list(self, objects=()):
        lst = _handle(lib.rtx_hittable_list_new(self._p))
        for o in objects:
            self.list_add(lst, o)
        return lst

    def list_add(self, lst, obj):
        _check(lib.rtx_hittable_list_add(self._p, lst, obj))

    def bvh_from_list(self, lst, time0, time1):
        return _handle(lib.rtx_bvh_from_list(self._p, lst, time0, time1))

    def instance_bvh(self, lst):
        """An instance tree (rtx_instance_bvh_from_list): the list of lst's members, culled by their true transformed boxes."""
        return _handle(lib.rtx_instance_bvh_from_list(self._p, lst))

    def translate(self, offset, obj):
        return _handle(lib.rtx_translate(self._p, _v3(offset), obj))

    def rotate_y(self, angle_degrees, obj):
        return _handle(lib.rtx_rotate_y(self._p, angle_degrees, obj))

    def constant_medium(self, rgb, density, boundary):
        return _handle(lib.rtx_constant_medium(self._p, _v3(rgb), density, boundary))

    def triangle_model(self, path, scale):
        return _handle(lib.rtx_triangle_model(self._p, os.fsencode(path), scale))

    def triangle_mesh(self, vertices, faces, mat):
        v = np.ascontiguousarray(vertices, dtype=np.float64).reshape(-1, 3)
        f = np.ascontiguousarray(faces, dtype=np.int64).reshape(-1, 3)
        return _handle(lib.rtx_triangle_mesh(self._p, v.ctypes.data_as(_D3), v.shape[0],
                                             f.ctypes.data_as(C.POINTER(C.c_int64)), f.shape[0], mat))

    # scene catalogue (world.rs:876-1179)
    def get_world_cam(self, scene_id, camera_aspect=0.0, earth_ppm=None, dragon_ply=None, mesh_triangles=0,
                      book2_boxes_per_side=0, book2_spheres=0):
        opt = RtxSceneOptions(camera_aspect, os.fsencode(earth_ppm) if earth_ppm else None,
                              os.fsencode(dragon_ply) if dragon_ply else None, mesh_triangles,
                              book2_boxes_per_side, book2_spheres)
        world = _H()
        cam = RtxCamera()
        bg = (C.c_double * 3)()
        _check(lib.rtx_get_world_cam(self._p, scene_id, C.byref(opt), C.byref(world), C.byref(cam), bg))
        return world.value, cam, (bg[0], bg[1], bg[2])

    def flatten(self, world, max_leaf=0, sah_bins=0, reference_bvh=False, bvh_seed=0, gpu_builder=False):
        return Flat(self, world, max_leaf, sah_bins, reference_bvh, bvh_seed, gpu_builder)


class Flat:
    """Flattened scene in host memory (rtx_flat)."""

    def __init__(self, builder, world, max_leaf=0, sah_bins=0, reference_bvh=False, bvh_seed=0, gpu_builder=False):
        opt = RtxBuildOptions(max_leaf, sah_bins, 1 if reference_bvh else 0, 1 if gpu_builder else 0, bvh_seed)
        p = _VP()
        _check(lib.rtx_flatten(builder.ptr, world, C.byref(opt), C.byref(p)))
        self._p = p
        self._builder = builder  # keep images/perlin tables alive for the oracle's views

    def __del__(self):
        p, self._p = getattr(self, "_p", None), None
        if p:
            lib.rtx_flat_destroy(p)

    @property
    def ptr(self):
        return self._p

    def arrays_ptr(self):
        return lib.rtx_flat_arrays(self._p)

    def info(self):
        info = RtxFlatInfo()
        _check(lib.rtx_flat_info(self._p, C.byref(info)))
        return {n: getattr(info, n) for n, _ in RtxFlatInfo._fields_}

    def lights(self):
        """Census of next-event estimation's light table (rtx_flat_lights): n_lights, n_rect_lights, n_sphere_lights,
        n_unsampled_emitters, total_area."""
        info = RtxLightInfo()
        _check(lib.rtx_flat_lights(self._p, C.byref(info)))
        return {n: getattr(info, n) for n, _ in RtxLightInfo._fields_}

    def instances(self):
        """Census of the instance trees (rtx_flat_instances): n_trees, n_members, n_nodes, max_depth."""
        info = RtxInstanceInfo()
        _check(lib.rtx_flat_instances(self._p, C.byref(info)))
        return {n: getattr(info, n) for n, _ in RtxInstanceInfo._fields_}

    def top_level_kinds(self):
        """Entry kinds of the flattened world list, in HittableList order (rtx_flat_top_level_kind)."""
        n = self.info()["n_top_level"]
        return [lib.rtx_flat_top_level_kind(self._p, i) for i in range(n)]

    def slot_chain(self, slot):
        """The Translate / RotateY chain of a top-level slot, outermost first (rtx_flat_slot_chain): a list of "translate" /
        "rotate_y", [] for a slot without a chain.  IndexError when the slot is out of range."""
        kinds = (C.c_int32 * 4)()
        n = lib.rtx_flat_slot_chain(self._p, int(slot), kinds)
        if n < 0:
            raise IndexError("slot %r is out of range" % (slot,))
        return [_XFORM_NAMES[kinds[k]] for k in range(n)]

    def instance_tree(self, k):
        """Instance tree k (rtx_flat_instance_tree): first_slot, n_slots, n_nodes, depth.  Its members are the n_slots
        consecutive slots from first_slot."""
        info = RtxInstanceTree()
        _check(lib.rtx_flat_instance_tree(self._p, int(k), C.byref(info)))
        return {n: getattr(info, n) for n, _ in RtxInstanceTree._fields_}

    def set_transforms(self, updates):
        """New parameters for the chains of top-level slots, in place (rtx_flat_set_transforms): the flat scene becomes the one
        flattened from scratch with these offsets and angles.  updates: {slot: [("translate", (x, y, z)) | ("rotate_y",
        degrees), ...]}, every op of the slot's chain, outermost first.  ValueError for input the chain does not admit."""
        arr = _slot_ops(self, updates)
        _check(lib.rtx_flat_set_transforms(self._p, arr, len(arr)))

    def triangle_ids(self, builder, handle):
        """The ids of the triangles below `handle` (a triangle, a mesh's list, a BvhNode, a wrapper or medium around those) in
        list order, a mesh's faces in face order (rtx_flat_triangle_ids) -> int32 array.  A triangle's id is the ordinal of its
        first emission by the flattener; Flat.array("triangle_id") holds the id of every flat triangle."""
        return _prim_ids(lib.rtx_flat_triangle_ids, self, builder, handle)

    def set_triangles(self, ids, vertices):
        """New vertices for the triangles `ids`, in place (rtx_flat_set_triangles): the flat scene becomes the one flattened from
        scratch with these vertices, its BVHs refitted with their topology kept.  vertices: n x 9 (or n x 3 x 3) doubles, v0 v1 v2
        of ids[i]."""
        ids, vertices = _prim_update(ids, vertices, *_TRIANGLE_VALUES)
        _check(lib.rtx_flat_set_triangles(self._p, ids.ctypes.data_as(C.POINTER(C.c_int32)), len(ids), vertices.ctypes.data_as(_D3)))

    def sphere_ids(self, builder, handle):
        """The ids of the static spheres below `handle` (a sphere, a list, a BvhNode, an instance tree, a wrapper or medium
        around those) in list order (rtx_flat_sphere_ids) -> int32 array.  A sphere's id is its index in Flat.array("spheres");
        moving and gravity spheres have none and are skipped."""
        return _prim_ids(lib.rtx_flat_sphere_ids, self, builder, handle)

    def set_spheres(self, ids, spheres):
        """A new centre and radius for the static spheres `ids`, in place (rtx_flat_set_spheres): the flat scene becomes the one
        flattened from scratch with these spheres, its BVHs refitted with their topology kept.  spheres: n x 4 doubles,
        cx cy cz radius of ids[i]."""
        ids, spheres = _prim_update(ids, spheres, *_SPHERE_VALUES)
        _check(lib.rtx_flat_set_spheres(self._p, ids.ctypes.data_as(C.POINTER(C.c_int32)), len(ids), spheres.ctypes.data_as(_D3)))

    def moving_sphere_ids(self, builder, handle):
        """The ids of the MovingSpheres below `handle` (a mover, a list, a BvhNode, a wrapper or medium around those) in list
        order (rtx_flat_moving_sphere_ids) -> int32 array.  A mover's id is its index in Flat.array("moving_spheres"); every
        other kind is skipped."""
        return _prim_ids(lib.rtx_flat_moving_sphere_ids, self, builder, handle)

    def set_moving_spheres(self, ids, movers):
        """New end centres and a radius for the MovingSpheres `ids`, in place (rtx_flat_set_moving_spheres): the flat scene
        becomes the one flattened from scratch with these values, its BVHs and their time-aware boxes refitted with their
        topology kept.  movers: n x 7 doubles, c0 xyz, c1 xyz, radius of ids[i]; time0, time1 and the material stay."""
        ids, movers = _prim_update(ids, movers, *_MOVER_VALUES)
        _check(lib.rtx_flat_set_moving_spheres(self._p, ids.ctypes.data_as(C.POINTER(C.c_int32)), len(ids), movers.ctypes.data_as(_D3)))

    def rect_ids(self, builder, handle):
        """The ids of every rectangle emitted from the handles below `handle` (a rectangle, a RectPrism, a list, a BvhNode, an
        instance tree, a wrapper or medium around those), handle by handle in list order (rtx_flat_rect_ids) -> int32 array.  A
        rectangle's id is its index in Flat.array("rects"); a RectPrism gives six per emission in the order of prism_rects --
        twelve for one prism under two Translates -- and no id is returned twice."""
        return _prim_ids(lib.rtx_flat_rect_ids, self, builder, handle)

    def set_rects(self, ids, rects):
        """New extents for the rectangles `ids`, in place (rtx_flat_set_rects): the flat scene becomes the one flattened from
        scratch with these rectangles, its BVHs refitted with their topology kept.  rects: n x 5 doubles, a0 a1 b0 b1 k of
        ids[i] -- the constructor's (x0, x1, y0, y1, k); the axis and the material stay."""
        ids, rects = _prim_update(ids, rects, *_RECT_VALUES)
        _check(lib.rtx_flat_set_rects(self._p, ids.ctypes.data_as(C.POINTER(C.c_int32)), len(ids), rects.ctypes.data_as(_D3)))

    def set_shading(self, edits):
        """New shading parameters, in place (rtx_flat_set_shading): the flat scene becomes the one flattened from scratch when
        the builder calls are made with the new values.  edits: a list of ("solid_color", tex, (r, g, b)) | ("noise_scale", tex,
        s) | ("metal", mat, (r, g, b), fuzz) | ("dielectric", mat, ir) | ("medium_density", slot, d); tex and mat are the
        builder's handles (what cast_rays reports in ids[:, 1] is a mat), slot an index in the world list.  ValueError for a
        malformed tuple; RtxError for what the scene does not admit."""
        arr = _shading_edits(edits)
        _check(lib.rtx_flat_set_shading(self._p, arr, len(arr)))

    def material(self, index):
        """Material `index` as the flat scene holds it (rtx_flat_material_info): kind (a name of MATERIAL_KINDS), tex, albedo,
        param."""
        info = RtxMaterialInfo()
        _check(lib.rtx_flat_material_info(self._p, int(index), C.byref(info)))
        return {"kind": MATERIAL_KINDS[info.kind], "tex": info.tex, "albedo": tuple(info.albedo), "param": info.param}

    def texture(self, index):
        """Texture `index` as the flat scene holds it (rtx_flat_texture_info): kind (a name of TEXTURE_KINDS), a, b, color,
        scale."""
        info = RtxTextureInfo()
        _check(lib.rtx_flat_texture_info(self._p, int(index), C.byref(info)))
        return {"kind": TEXTURE_KINDS[info.kind], "a": info.a, "b": info.b, "color": tuple(info.color), "scale": info.scale}

    def medium(self, slot):
        """The ConstantMedium in top-level slot `slot` (rtx_flat_medium_info): material (its phase material, whose tex is the
        fog's colour) and neg_inv_density as stored."""
        info = RtxMediumInfo()
        _check(lib.rtx_flat_medium_info(self._p, int(slot), C.byref(info)))
        return {"material": info.material, "neg_inv_density": info.neg_inv_density}

    def rebuild_instance_trees(self, trees=None, builder="morton"):
        """A new topology for instance trees from their members' boxes at the current pose, in place
        (rtx_flat_rebuild_instance_trees).  trees: tree indices, None for every tree.  builder: "morton" -- what
        Scene.rebuild_instance_trees does on the device, restated on the host -- or "sah", the flattener's own builder: the
        flat scene then equals a fresh flatten of the pose."""
        if builder not in _REBUILD_NAMES:
            raise ValueError('builder must be "morton" or "sah", not %r' % (builder,))
        arr, n = _tree_list(trees)
        _check(lib.rtx_flat_rebuild_instance_trees(self._p, arr, n, _REBUILD_NAMES.index(builder)))

    def instance_tree_cost(self, k):
        """How well instance tree k culls as it stands (rtx_flat_instance_tree_cost): the summed surface area of every node's
        two child boxes over the area of the tree's box.  Smaller is better; compare a refitted tree with a rebuilt one."""
        cost = C.c_double(0.0)
        _check(lib.rtx_flat_instance_tree_cost(self._p, int(k), C.byref(cost)))
        return cost.value

    def array(self, name):
        """A copy of one host array as bytes (rtx_flat_array; a test hook): a name of SCENE_ARRAYS but "world_desc" and "nodes4"."""
        return _scene_array(lambda out, n: lib.rtx_flat_array(self._p, SCENE_ARRAYS[name][0], out, n), self, name, False)

    def upload(self, f32=False):
        """f32=True: the statistical fast mode (rtx_scene_upload_f32): float arithmetic, no bit-exactness claim."""
        return Scene(self, f32=f32)


_TRIANGLE_VALUES = (9, "vertices", "v0 v1 v2")        # width, name, each: what a set_* call holds per id
_SPHERE_VALUES = (4, "spheres", "cx cy cz radius")
_MOVER_VALUES = (7, "movers", "c0 xyz, c1 xyz, radius")
_RECT_VALUES = (5, "rects", "a0 a1 b0 b1 k")


def prism_rects(p0, p1):
    """The (6, 5) values a0 a1 b0 b1 k of the six rectangles of Builder.rect_prism(p0, p1), in the order the flattener emits them
    (RectPrism::new: front, back, top, bottom, right, left -- two XY, two XZ, two YZ rectangles).  Moving a box of a resident
    scene is scene.set_rects(flat.rect_ids(b, box), prism_rects(p0, p1))."""
    (x0, y0, z0), (x1, y1, z1) = [float(v) for v in p0], [float(v) for v in p1]
    return np.array([[x0, x1, y0, y1, z1], [x0, x1, y0, y1, z0], [x0, x1, z0, z1, y1], [x0, x1, z0, z1, y0],
                     [y0, y1, z0, z1, x1], [y0, y1, z0, z1, x0]], dtype=np.float64)


def _prim_ids(fn, flat, builder, handle):
    """rtx_flat_triangle_ids / rtx_flat_sphere_ids: once for the count, once for the ids -> int32 array."""
    n = fn(flat.ptr, builder.ptr, int(handle), None, 0)
    if n < 0:
        raise RtxError(RTX_EINVAL, last_error())
    out = np.zeros(n, dtype=np.int32)
    if n and fn(flat.ptr, builder.ptr, int(handle), out.ctypes.data_as(C.POINTER(C.c_int32)), n) != n:
        raise RtxError(RTX_EINVAL, last_error())
    return out


def _prim_update(ids, values, width, name, each):
    """ids, values of a set_* call -> (contiguous int32 array of n ids, contiguous float64 array of width * n values)."""
    ids = np.ascontiguousarray(np.asarray(ids, dtype=np.int32).reshape(-1))
    values = np.ascontiguousarray(np.asarray(values, dtype=np.float64).reshape(-1))
    if values.size != width * ids.size:
        raise ValueError("%s holds %d values, %d ids need %d (%s each)" % (name, values.size, ids.size, width * ids.size, each))
    if ids.size == 0:  # a pointer the library may compare with NULL
        return np.zeros(1, dtype=np.int32)[:0], np.zeros(1, dtype=np.float64)[:0]
    return ids, values


def _scene_set_prims(scene, host_fn, device_fn, ids, values, stream, width, name, each):
    """Scene.set_triangles / set_spheres: a torch tensor on the GPU goes to the device entry as it is, anything else is staged."""
    raw = getattr(stream, "cuda_stream", stream)
    if hasattr(values, "data_ptr"):  # a torch tensor
        import torch
        if not values.is_cuda or values.dtype != torch.float64 or not values.is_contiguous():
            raise ValueError("a tensor of %s must be a contiguous float64 tensor on the GPU" % name)
        ids = np.ascontiguousarray(np.asarray(ids, dtype=np.int32).reshape(-1))
        if values.numel() != width * ids.size:
            raise ValueError("%s holds %d values, %d ids need %d (%s each)" % (name, values.numel(), ids.size, width * ids.size, each))
        if ids.size == 0:
            return  # n = 0 is RTX_OK with nothing launched; an empty tensor has no pointer to hand over
        _check(device_fn(scene.ptr, ids.ctypes.data_as(C.POINTER(C.c_int32)), len(ids), _VP(values.data_ptr() or None), _VP(raw or None)))
        return
    ids, values = _prim_update(ids, values, width, name, each)
    _check(host_fn(scene.ptr, ids.ctypes.data_as(C.POINTER(C.c_int32)), len(ids), values.ctypes.data_as(_D3), _VP(raw or None)))


def _tree_list(trees):
    """trees of rebuild_instance_trees -> (ctypes int32 array or None, n)."""
    if trees is None:
        return None, 0
    trees = [int(k) for k in trees]
    return (C.c_int32 * max(len(trees), 1))(*trees), len(trees)


def _slot_ops(flat, updates):
    """updates of Flat.set_transforms / Scene.set_transforms -> a ctypes array of RtxSlotOps, checked against the chains of
    `flat`.  Raises ValueError before the library sees anything."""
    if not isinstance(updates, dict):
        raise ValueError("updates must be a dict {slot: [op, ...]}")
    arr = (RtxSlotOps * max(len(updates), 1))()
    n_top = flat.info()["n_top_level"]
    for i, (slot, ops) in enumerate(updates.items()):
        if isinstance(slot, bool) or not isinstance(slot, (int, np.integer)):
            raise ValueError("slot %r is not an integer" % (slot,))
        if not 0 <= slot < n_top:
            raise ValueError("slot %d is out of range (the world list has %d slots)" % (slot, n_top))
        chain = flat.slot_chain(slot)
        if not chain:
            raise ValueError("slot %d has no Translate / RotateY chain" % slot)
        ops = list(ops)
        if len(ops) != len(chain):
            raise ValueError("slot %d: %d ops given, its chain has %d (%s)" % (slot, len(ops), len(chain), ", ".join(chain)))
        arr[i].slot, arr[i].n_ops = int(slot), len(ops)
        for k, op in enumerate(ops):
            if not isinstance(op, (tuple, list)) or len(op) != 2 or op[0] not in _XFORM_NAMES:
                raise ValueError('slot %d, op %d: expected ("translate", (x, y, z)) or ("rotate_y", degrees), got %r' % (slot, k, op))
            if op[0] != chain[k]:
                raise ValueError("slot %d, op %d is a %s in the scene, not a %s" % (slot, k, chain[k], op[0]))
            try:
                vals = [float(x) for x in op[1]] if op[0] == "translate" else [float(op[1])]
            except (TypeError, ValueError):
                raise ValueError("slot %d, op %d: %r is not %s" % (slot, k, op[1], "three numbers" if op[0] == "translate" else "a number"))
            if len(vals) != (3 if op[0] == "translate" else 1) or not all(np.isfinite(vals)):
                raise ValueError("slot %d, op %d: %r is not %s" % (slot, k, op[1], "three finite numbers" if op[0] == "translate" else "a finite number"))
            arr[i].ops[k].op = _XFORM_NAMES.index(op[0])
            for a, x in enumerate(vals):
                arr[i].ops[k].v[a] = x
    return (RtxSlotOps * len(updates)).from_buffer(arr) if len(updates) else (RtxSlotOps * 0)()


def _shading_edits(edits):
    """edits of Flat.set_shading / Scene.set_shading -> a ctypes array of RtxShadingEdit.  Raises ValueError for a tuple of the
    wrong shape before the library sees anything; what the scene decides (ranges, kinds, finiteness) is the library's."""
    if isinstance(edits, (dict, str, bytes)) or not hasattr(edits, "__iter__"):
        raise ValueError("edits must be a list of tuples")
    edits = list(edits)
    arr = (RtxShadingEdit * max(len(edits), 1))()
    shapes = {"solid_color": '("solid_color", tex, (r, g, b))', "noise_scale": '("noise_scale", tex, scale)',
              "metal": '("metal", mat, (r, g, b), fuzz)', "dielectric": '("dielectric", mat, ir)',
              "medium_density": '("medium_density", slot, density)'}
    for i, e in enumerate(edits):
        if not isinstance(e, (tuple, list)) or len(e) < 2 or e[0] not in _SHADE_NAMES:
            raise ValueError("edit %d: expected one of %s, got %r" % (i, " | ".join(shapes.values()), e))
        what, index = e[0], e[1]
        if len(e) != (4 if what == "metal" else 3):
            raise ValueError("edit %d: expected %s, got %r" % (i, shapes[what], e))
        if isinstance(index, bool) or not isinstance(index, (int, np.integer)):
            raise ValueError("edit %d: index %r is not an integer" % (i, index))
        try:
            if what in ("solid_color", "metal"):
                vals = [float(x) for x in e[2]]
                if len(vals) != 3:
                    raise TypeError
                if what == "metal":
                    vals.append(float(e[3]))
            else:
                vals = [float(e[2])]
        except (TypeError, ValueError):
            raise ValueError("edit %d: expected %s, got %r" % (i, shapes[what], e))
        arr[i].what, arr[i].index = _SHADE_NAMES.index(what), int(index)
        for a, x in enumerate(vals):
            arr[i].v[a] = x
    return (RtxShadingEdit * len(edits)).from_buffer(arr) if edits else (RtxShadingEdit * 0)()


def _scene_array(call, flat, name, f32):
    """One array through rtx_flat_array / rtx_device_scene_array as a uint8 numpy array; the size comes from Flat.info()."""
    info = flat.info()
    elem = SCENE_ARRAYS[name][2 if f32 else 1]
    count = {"entries": info["n_entries"], "nodes": info["n_nodes"], "nodes32": info["n_nodes"], "top_level": info["n_top_level"]}.get(name)
    if count is None:  # motion32 (n_nodes or none), world_desc, member_local_box: ask with 0 bytes, the refusal names the size
        if call(None, 0) == RTX_OK:
            return np.zeros(0, dtype=np.uint8)
        m = re.search(r"holds (\d+) bytes", last_error())
        if not m:
            raise RtxError(RTX_EINVAL, last_error())
        count = int(m.group(1)) // elem
    out = np.zeros(count * elem, dtype=np.uint8)
    _check(call(out.ctypes.data_as(_VP), out.size))
    return out


class Scene:
    """Scene resident on the current HIP device (rtx_scene)."""

    def __init__(self, flat, f32=False):
        p = _VP()
        _check((lib.rtx_scene_upload_f32 if f32 else lib.rtx_scene_upload)(flat.ptr, C.byref(p)))
        self._p = p
        self._flat = flat  # set_transforms checks its input against the slots' chains, whose shape never changes

    @property
    def is_f32(self):
        return bool(lib.rtx_scene_is_f32(self._p))

    def __del__(self):
        p, self._p = getattr(self, "_p", None), None
        if p:
            lib.rtx_scene_destroy(p)

    @property
    def ptr(self):
        return self._p

    def render(self, cam, cfg, want_accum=True, light_sampling=False, want_stats=False):
        """Whole image on the current device -> Screen (host arrays).  light_sampling=True: next-event estimation with MIS
        (rtx_render_ex; statistical, f64 scenes only).  want_stats=True: Screen.stats holds the RtxRenderStats."""
        w, h = cfg.image_width, image_height(cfg)
        accum = np.zeros((h, w, 3), dtype=np.float64) if want_accum else None
        rgb8 = np.zeros((h, w, 3), dtype=np.uint8)
        frame = RtxFrame(accum.ctypes.data_as(C.POINTER(C.c_double)) if want_accum else None,
                         rgb8.ctypes.data_as(C.POINTER(C.c_uint8)))
        if light_sampling or want_stats:
            stats = RtxRenderStats() if want_stats else None
            opt = _integrator_options(light_sampling)
            _check(lib.rtx_render_ex(self._p, C.byref(cam), C.byref(cfg), C.byref(opt), C.byref(frame),
                                     C.byref(stats) if stats else None))
            screen = Screen(w, h, rgb8, accum)
            screen.stats = stats
            return screen
        _check(lib.rtx_render(self._p, C.byref(cam), C.byref(cfg), C.byref(frame)))
        return Screen(w, h, rgb8, accum)

    def set_transforms(self, updates, stream=None):
        """New parameters for the chains of top-level slots of the RESIDENT scene (rtx_scene_set_transforms): every later call
        answers as on a scene flattened and uploaded from scratch with these offsets and angles.  updates as in
        Flat.set_transforms.  Enqueued on `stream` (a raw hipStream_t, an object with .cuda_stream such as a torch stream, or
        None for the default stream); ordering against work on other streams is the caller's."""
        arr = _slot_ops(self._flat, updates)
        raw = getattr(stream, "cuda_stream", stream)
        _check(lib.rtx_scene_set_transforms(self._p, arr, len(arr), _VP(raw or None)))

    def set_triangles(self, ids, vertices, stream=None):
        """New vertices for the triangles `ids` of the RESIDENT f64 scene: every later call answers as on the scene built from
        scratch with these vertices (its BVHs are refitted on the device, their topology kept).  vertices: n x 9 doubles as a
        numpy array (rtx_scene_set_triangles, staged with one copy) or as a torch float64 tensor on the GPU
        (rtx_scene_set_triangles_device: e.g. the output of a skinning kernel on `stream`).  ids: host integers either way.
        Enqueued on `stream` as in set_transforms."""
        _scene_set_prims(self, lib.rtx_scene_set_triangles, lib.rtx_scene_set_triangles_device, ids, vertices, stream, *_TRIANGLE_VALUES)

    def set_spheres(self, ids, spheres, stream=None):
        """A new centre and radius for the static spheres `ids` of the RESIDENT f64 scene: every later call answers as on the
        scene built from scratch with these spheres (its BVHs are refitted on the device, their topology kept; the light table
        follows a sphere light).  spheres: n x 4 doubles cx cy cz radius as a numpy array (rtx_scene_set_spheres, staged with
        one copy) or as a torch float64 tensor on the GPU (rtx_scene_set_spheres_device: e.g. an animation computed on
        `stream`).  ids: host integers either way.  Enqueued on `stream` as in set_transforms."""
        _scene_set_prims(self, lib.rtx_scene_set_spheres, lib.rtx_scene_set_spheres_device, ids, spheres, stream, *_SPHERE_VALUES)

    def set_moving_spheres(self, ids, movers, stream=None):
        """New end centres and a radius for the MovingSpheres `ids` of the RESIDENT f64 scene -- a frame of an animation with
        motion blur: c0 / c1 are the poses at shutter open and close.  Every later call answers as on the scene built from
        scratch with these values (its BVHs and time-aware boxes are refitted on the device, their topology kept).  movers:
        n x 7 doubles c0 xyz, c1 xyz, radius as a numpy array (rtx_scene_set_moving_spheres, staged with one copy) or as a
        torch float64 tensor on the GPU (rtx_scene_set_moving_spheres_device).  ids: host integers either way.  Enqueued on
        `stream` as in set_transforms; the first k_trace_lds launch afterwards waits once on the host where that kernel's plan
        hangs on the slopes (include/rtx_abi.h).  A tensor without a `stream` is taken on torch's current stream."""
        if stream is None and hasattr(movers, "data_ptr") and getattr(movers, "is_cuda", False):
            import torch
            stream = torch.cuda.current_stream(movers.device)
        _scene_set_prims(self, lib.rtx_scene_set_moving_spheres, lib.rtx_scene_set_moving_spheres_device, ids, movers, stream, *_MOVER_VALUES)

    def set_rects(self, ids, rects, stream=None):
        """New extents for the rectangles `ids` of the RESIDENT f64 scene -- a wall, the faces of a box (prism_rects), the boundary
        of a fog, an area light that slides or shrinks.  Every later call answers as on the scene built from scratch with these
        values (BVHs and instance trees are refitted on the device, their topology kept; slot boxes and the light table follow).
        rects: n x 5 doubles a0 a1 b0 b1 k as a numpy array (rtx_scene_set_rects, staged with one copy) or as a torch float64
        tensor on the GPU (rtx_scene_set_rects_device).  ids: host integers either way.  Enqueued on `stream` as in
        set_transforms; a tensor without a `stream` is taken on torch's current stream."""
        if stream is None and hasattr(rects, "data_ptr") and getattr(rects, "is_cuda", False):
            import torch
            stream = torch.cuda.current_stream(rects.device)
        _scene_set_prims(self, lib.rtx_scene_set_rects, lib.rtx_scene_set_rects_device, ids, rects, stream, *_RECT_VALUES)

    def set_shading(self, edits, stream=None):
        """New shading parameters for the RESIDENT scene of either precision (rtx_scene_set_shading): every later call answers as
        on a scene flattened and uploaded from scratch with the new colours, scales, metal / glass parameters and densities
        (the light table follows an emitted colour).  edits as in Flat.set_shading.  Enqueued on `stream` as in set_transforms.
        A progressive handle made earlier holds the old look."""
        arr = _shading_edits(edits)
        raw = getattr(stream, "cuda_stream", stream)
        _check(lib.rtx_scene_set_shading(self._p, arr, len(arr), _VP(raw or None)))

    def rebuild_instance_trees(self, trees=None, stream=None):
        """A new topology for instance trees of the RESIDENT scene from their members' boxes at the current pose
        (rtx_scene_rebuild_instance_trees; Morton codes, a radix sort and Karras' tree on the device).  trees: tree indices,
        None for every tree.  The kernels run on `stream` (as in set_transforms) and the call waits on it once, for the new
        depths.  -> {"trees_rebuilt", "max_depth", "max_stack_before", "max_stack_after"}."""
        arr, n = _tree_list(trees)
        raw = getattr(stream, "cuda_stream", stream)
        stats = RtxRebuildStats()
        _check(lib.rtx_scene_rebuild_instance_trees(self._p, arr, n, _VP(raw or None), C.byref(stats)))
        return {k: getattr(stats, k) for k in ("trees_rebuilt", "max_depth", "max_stack_before", "max_stack_after")}

    def instance_tree_cost(self, k):
        """Flat.instance_tree_cost of the resident tree k as it stands (rtx_scene_instance_tree_cost; blocking)."""
        cost = C.c_double(0.0)
        _check(lib.rtx_scene_instance_tree_cost(self._p, int(k), C.byref(cost)))
        return cost.value

    def max_stack(self):
        """The max_stack the scene's binary walks are now launched with (rtx_device_scene_array 9): Flat.info()["max_stack"]
        at upload, changed by rebuild_instance_trees."""
        v = C.c_int32(0)
        _check(lib.rtx_device_scene_array(self._p, 9, C.byref(v), 4))
        return v.value

    def array(self, name):
        """A copy of one resident array as bytes, after everything enqueued (rtx_device_scene_array; a test hook): "entries",
        "nodes", "nodes32", "motion32", "world_desc", "triangles", "top_box32", "spheres", "moving_spheres", "lights" (the light table of
        next-event estimation; empty without sampled lights), "materials", "textures" or "nodes4" (the 4-wide tree; empty when
        the scene has none)."""
        return _scene_array(lambda out, n: lib.rtx_device_scene_array(self._p, SCENE_ARRAYS[name][0], out, n), self._flat, name, self.is_f32)

    def wide_levels(self):
        """Stack levels the scene's 4-wide walks are launched with; 0 when it walks its binary tree (rtx_device_scene_array 8)."""
        v = C.c_int32(0)
        _check(lib.rtx_device_scene_array(self._p, 8, C.byref(v), 4))
        return v.value

    def trim(self):
        """Release the render workspace (sample buffer, accumulators); the geometry stays resident."""
        _check(lib.rtx_scene_trim(self._p))

    def render_scene_with_time(self, t0, t1, path, row_chunk_compat=True, overrides=None):
        """render_scene_with_time(t0, t1, path, world) of world.rs:1249-1330 on this resident scene: one 500x500 PPM frame."""
        _check(lib.rtx_render_scene_with_time(self._p, t0, t1, path.encode(), 1 if row_chunk_compat else 0,
                                              C.byref(overrides) if overrides is not None else None))

    def render_device(self, cam, cfg, shard=None, d_accum=0, d_rgb8=0, stream=0, want_stats=False):
        """Asynchronous render of one shard into DEVICE buffers (raw pointers, e.g. torch .data_ptr())."""
        sh = RtxShard(*shard, 0) if shard is not None else None
        stats = RtxRenderStats() if want_stats else None
        _check(lib.rtx_render_device(self._p, C.byref(cam), C.byref(cfg), C.byref(sh) if sh else None,
                                     _VP(d_accum or None), _VP(d_rgb8 or None), _VP(stream or None),
                                     C.byref(stats) if stats else None))
        return stats

    def progressive(self, cam, cfg, shard=None, light_sampling=False):
        """A frame accumulated over several calls (rtx_progressive); cfg.samples_per_pixel is the sample budget.
        light_sampling=True: every add traces with next-event estimation (rtx_progressive_create_ex)."""
        return Progressive(self, cam, cfg, shard, light_sampling=light_sampling)

    def render_count(self, cam, cfg, shard=None):
        sh = RtxShard(*shard, 0) if shard is not None else None
        stats = RtxRenderStats()
        _check(lib.rtx_render_count(self._p, C.byref(cam), C.byref(cfg), C.byref(sh) if sh else None, C.byref(stats)))
        return stats

    def cast_rays(self, origins, directions, times=None, t_max=None, *, t_min=0.001, t_max_all=float("inf"), seed=1,
                  stream_step=0, want=RAY_COLUMNS):
        """Closest hits of a batch of rays (rtx_scene_cast_rays*): ray r is one world_hit(Ray(origins[r], directions[r],
        times[r]), t_min, t_max[r]) on the stream of seed + r * stream_step -> RayHits holding the columns named in `want`.
        numpy arrays go through the host entry and come back as numpy arrays.  torch tensors on the GPU are passed by
        data_ptr(), without a copy: the results are torch tensors on that device and the call is only ENQUEUED on torch's
        current stream for it.  Every array is float64 and C-contiguous: origins and directions (n, 3), times and t_max (n,)."""
        return _cast_rays(self, origins, directions, times, t_max, t_min, t_max_all, seed, stream_step, want)

    def occlusion(self, origins, directions, times=None, t_max=None, *, t_min=0.001, t_max_all=float("inf"), stream=None):
        """Any-hit casts of a batch of segments (rtx_scene_occlusion*): tau[r] is +inf when a surface lies on
        [t_min, t_max[r]] of Ray(origins[r], directions[r], times[r]), else the summed optical depth of the ConstantMedia on
        it (0 when the segment is clear), NaN for a ray past a GravitySphere scene's time limit -> Occlusion with .tau,
        .blocked and .transmittance.  Deterministic: no stream is drawn from.  Arrays as in cast_rays: numpy goes through the
        host entry; torch tensors on the GPU are passed by data_ptr() and the call is only ENQUEUED, on `stream` (a
        torch.cuda.Stream or a raw hipStream_t) or, when None, on torch's current stream for that device."""
        return _occlusion(self, origins, directions, times, t_max, t_min, t_max_all, stream)

    def occlusion_between(self, a, b, eps=1e-6):
        """occlusion of the segments from a[r] to b[r]: direction = b - a, t_max_all = 1 - eps -- the interval next-event
        estimation gives its shadow ray (RT_NEE_SHADOW_EPS), so a surface AT b does not block."""
        _ray_arrays([("a", a, 3), ("b", b, 3)])
        if not 0.0 <= eps < 1.0:
            raise ValueError("eps: expected 0 <= eps < 1, got %r" % (eps,))
        return _occlusion(self, a, b - a, None, None, 0.001, 1.0 - eps, None)

    def trace_rays(self, origins, directions, times=None, *, spp=1, max_depth=50, background=(0.7, 0.8, 1.0), seed=1,
                   first_sample=0, first_ray=0, light_sampling=False, sumsq=False, out=None, sample_buffer_bytes=0,
                   want_stats=False):
        """The estimator's radiance along a batch of rays (rtx_scene_trace_rays*): samples first_sample .. first_sample + spp - 1
        of every ray, each a whole path that starts from Ray(origins[r], directions[r], times[r]) as given, on the stream of
        (seed, first_ray + r, sample) -> RadianceSums with .sum (n, 3), .sumsq (n, 3) or None, .spp and .mean.  Arrays as in
        cast_rays: numpy goes through the host entry; torch tensors on the GPU are passed by data_ptr() and the call is only
        ENQUEUED on torch's current stream (want_stats=True synchronises).  out=: a RadianceSums of the same rays whose sums
        are continued in place; first_sample must then be out.spp.  Uses the scene's render workspace: one render or radiance
        query in flight per Scene."""
        return _trace_rays(self, origins, directions, times, spp, max_depth, background, seed, first_sample, first_ray,
                           light_sampling, sumsq, out, sample_buffer_bytes, want_stats)

    def gather(self, points, normals=None, times=None, *, spp=1, max_depth=50, background=(0.7, 0.8, 1.0), seed=1,
               light_sampling=False, sh_order=0, first_point=0, first_sample=0, sumsq=True, out=None, stream=None,
               sample_buffer_bytes=0, want_stats=False):
        """Light arriving at a batch of points (rtx_scene_gather*): samples first_sample .. first_sample + spp - 1 of every
        point, each a whole path whose start direction is drawn on the device from the stream of (seed, first_point + r,
        sample).  With normals (n, 3) -- taken as given, not normalised -- the path starts as if it had scattered off a white
        Lambertian surface there (the surface form: .irradiance = pi * mean); without, the direction is uniform over the
        sphere (the probe form), and sh_order = 1 | 2 projects every sample onto 4 | 9 real spherical harmonics per channel
        (.sum is then (n, K, 3) and .sh = 4 pi * sum / spp the coefficient estimates).  -> GatherSums with .sum, .sumsq (or
        None), .spp, .mean, .irradiance, .sh.  Arrays as in trace_rays: numpy goes through the host entry; torch tensors on
        the GPU are passed by data_ptr() and the call is only ENQUEUED, on `stream` or torch's current one (want_stats=True
        synchronises).  out=: a GatherSums of the same points whose sums are continued in place; first_sample must then be
        out.spp.  Uses the scene's render workspace: one render, radiance or gather query in flight per Scene."""
        return _gather(self, points, normals, times, spp, max_depth, background, seed, light_sampling, sh_order, first_point,
                       first_sample, sumsq, out, stream, sample_buffer_bytes, want_stats)

    def nearest(self, points, times=None, r_max=None, *, r_max_all=float("inf"), media=False, want=NEAREST_COLUMNS, stream=None):
        """The closest surface point of the scene per point (rtx_scene_nearest*): over every primitive of the world list
        (a ConstantMedium's boundary only with media=True), the point q that minimises |points[r] - q|^2 at times[r] within
        r_max[r] (or r_max_all) -> Nearest with the columns named in `want`: .d (n,) +inf when nothing is found, .q (n, 3),
        .ids (n, 4) int32 {material, top-level slot, PrimType, index in that type's array}, all -1 when nothing is found;
        and .found, .material, .slot, .prim_type, .prim_index.  Deterministic, no stream is drawn from; scenes with
        GravitySpheres raise RtxError (RTX_EUNSUPPORTED).  Arrays as in occlusion: numpy goes through the host entry; torch
        tensors on the GPU are passed by data_ptr() and the call is only ENQUEUED, on `stream` or torch's current one."""
        return _nearest(self, points, times, r_max, r_max_all, media, want, stream)


_RAY_COLUMN_SHAPES = {"t": (), "p": (3,), "normal": (3,), "uv": (2,), "ids": (4,)}


class RayHits:
    """What Scene.cast_rays returns: n and, for each requested column, an attribute of that name (None when not asked for).
    t (n,) +inf on a miss; p, normal (n, 3); uv (n, 2); ids (n, 4) int32 {hit, material index, top-level slot, front_face},
    {0, -1, -1, 0} on a miss."""

    def __init__(self, n, columns):
        self.n = n
        self.columns = tuple(columns)
        for name in RAY_COLUMNS:
            setattr(self, name, columns.get(name))

    @property
    def hit(self):
        return self.ids[:, 0] != 0 if self.ids is not None else None


def _is_torch(a):
    return type(a).__module__.split(".")[0] == "torch"


def _ray_arrays(given):
    """Checks the arrays of a ray batch -- (name, array or None, width: 3 for an (n, 3) column, 0 for an (n,) one), origins
    first -- and returns (n, on_device): float64, contiguous, of one kind (numpy, or torch on one GPU) and one length."""
    origins = given[0][1]
    on_device = _is_torch(origins)
    if on_device:
        import torch  # only when the caller already holds tensors: the binding loads without torch
    n = None
    for name, a, width in given:
        if a is None:
            if width:
                raise ValueError("%s: required" % name)
            continue
        if _is_torch(a) != on_device:
            raise ValueError("%s: torch tensors and numpy arrays cannot be mixed in one call" % name)
        if on_device:
            if not a.is_cuda or a.device != origins.device:
                raise ValueError("%s: must be a tensor on the GPU of origins (%s)" % (name, origins.device))
            ok_dtype, contiguous = a.dtype == torch.float64, a.is_contiguous()
        else:
            if not isinstance(a, np.ndarray):
                raise ValueError("%s: expected a numpy array or a torch tensor on the GPU" % name)
            ok_dtype, contiguous = a.dtype == np.float64, a.flags["C_CONTIGUOUS"]
        if not ok_dtype:
            raise ValueError("%s: must be float64, not %s" % (name, a.dtype))
        if not contiguous:
            raise ValueError("%s: must be contiguous" % name)
        shape = tuple(a.shape)
        if len(shape) != (2 if width else 1) or (width and shape[1] != width):
            raise ValueError("%s: expected shape %s, got %s" % (name, "(n, 3)" if width else "(n,)", shape))
        if n is None:
            n = shape[0]
        elif shape[0] != n:
            raise ValueError("%s: %d rays, but origins has %d" % (name, shape[0], n))
    return n, on_device


class _QueryArrays:
    """Of a batch that _ray_arrays has checked: column addresses, result arrays of the rays' kind, the choice of the entry point."""

    def __init__(self, given):
        self.n, self.on_device = _ray_arrays(given)
        if self.on_device:
            import torch
            self.torch, self.device = torch, given[0][1].device

    def addr(self, a):
        return a.data_ptr() if self.on_device else a.ctypes.data

    def ptr(self, a):
        """The address of a column; None for a column that was left out, and for every column of an empty batch."""
        return self.addr(a) if a is not None and self.n else None

    def empty(self, shape, dtype="float64"):
        if self.on_device:
            return self.torch.empty(shape, device=self.device, dtype=getattr(self.torch, dtype))
        return np.empty(shape, dtype=getattr(np, dtype))

    def call(self, host_fn, device_fn, args, tail=(), stream=None):
        """numpy: host_fn(*args, *tail).  torch: device_fn(*args, stream or torch's current one, *tail), the rays' GPU current."""
        if not self.on_device:
            return _check(host_fn(*args, *tail))
        with self.torch.cuda.device(self.device):
            if stream is None:
                stream = self.torch.cuda.current_stream(self.device)
            handle = getattr(stream, "cuda_stream", stream)
            _check(device_fn(*args, _VP(handle or None), *tail))


def _cast_rays(scene, origins, directions, times, t_max, t_min, t_max_all, seed, stream_step, want):
    want = tuple(want)
    for name in want:
        if name not in RAY_COLUMNS:
            raise ValueError("want: unknown column %r (expected some of %s)" % (name, ", ".join(RAY_COLUMNS)))
    io = _QueryArrays([("origins", origins, 3), ("directions", directions, 3), ("times", times, 0), ("t_max", t_max, 0)])
    batch = RtxRayBatch()
    lib.rtx_ray_batch_defaults(C.byref(batch))
    batch.n, batch.t_min, batch.t_max_all, batch.seed, batch.stream_step = io.n, t_min, t_max_all, seed, stream_step
    cols = {name: io.empty((io.n,) + _RAY_COLUMN_SHAPES[name], "int32" if name == "ids" else "float64") for name in want}
    batch.origin, batch.direction, batch.time, batch.t_max = io.ptr(origins), io.ptr(directions), io.ptr(times), io.ptr(t_max)
    hits = RtxRayHits(*[io.ptr(cols.get(name)) for name in RAY_COLUMNS])
    io.call(lib.rtx_scene_cast_rays, lib.rtx_scene_cast_rays_device, (scene.ptr, C.byref(batch), C.byref(hits)))
    return RayHits(io.n, cols)


class Occlusion:
    """What Scene.occlusion returns: n and tau (n,) float64 -- a numpy array, or a torch tensor on the rays' device.
    blocked = isinf(tau): a surface on the segment (or a medium of infinite density).  transmittance = exp(-tau), computed
    here in the caller's array library, never on the scene's kernels: 0 where blocked, 1 where clear, NaN where tau is."""

    def __init__(self, n, tau):
        self.n, self.tau = n, tau

    @property
    def blocked(self):
        return self.tau.isinf() if _is_torch(self.tau) else np.isinf(self.tau)

    @property
    def transmittance(self):
        return (-self.tau).exp() if _is_torch(self.tau) else np.exp(-self.tau)


def _occlusion(scene, origins, directions, times, t_max, t_min, t_max_all, stream):
    io = _QueryArrays([("origins", origins, 3), ("directions", directions, 3), ("times", times, 0), ("t_max", t_max, 0)])
    if t_min != t_min:
        raise ValueError("t_min: NaN")
    if t_max_all != t_max_all:
        raise ValueError("t_max_all: NaN")
    if stream is not None and not io.on_device:
        raise ValueError("stream: only for torch tensors on the GPU (numpy arrays go through the blocking host entry)")
    batch = RtxRayBatch()
    lib.rtx_ray_batch_defaults(C.byref(batch))
    batch.n, batch.t_min, batch.t_max_all = io.n, t_min, t_max_all
    store = io.empty((max(io.n, 1),))  # (tau may not be NULL, even for n = 0)
    batch.origin, batch.direction, batch.time, batch.t_max = io.ptr(origins), io.ptr(directions), io.ptr(times), io.ptr(t_max)
    io.call(lib.rtx_scene_occlusion, lib.rtx_scene_occlusion_device, (scene.ptr, C.byref(batch), _VP(io.addr(store))), stream=stream)
    return Occlusion(io.n, store[:io.n])


_NEAREST_COLUMN_SHAPES = {"d": (), "q": (3,), "ids": (4,)}


class Nearest:
    """What Scene.nearest returns: n and, for each requested column, an attribute of that name (None when not asked for): d (n,)
    +inf when nothing is found; q (n, 3); ids (n, 4) int32 {material index, top-level slot, PrimType, index in that type's
    array}, all -1 when nothing is found -- numpy arrays, or torch tensors on the points' device."""

    def __init__(self, n, columns):
        self.n = n
        self.columns = tuple(columns)
        for name in NEAREST_COLUMNS:
            setattr(self, name, columns.get(name))

    def _id(self, k):
        return self.ids[:, k] if self.ids is not None else None

    @property
    def found(self):
        return self.ids[:, 1] >= 0 if self.ids is not None else None

    material = property(lambda self: self._id(0))
    slot = property(lambda self: self._id(1))
    prim_type = property(lambda self: self._id(2))
    prim_index = property(lambda self: self._id(3))


def _nearest(scene, points, times, r_max, r_max_all, media, want, stream):
    want = tuple(want)
    for name in want:
        if name not in NEAREST_COLUMNS:
            raise ValueError("want: unknown column %r (expected some of %s)" % (name, ", ".join(NEAREST_COLUMNS)))
    io = _QueryArrays([("points", points, 3), ("times", times, 0), ("r_max", r_max, 0)])
    if stream is not None and not io.on_device:
        raise ValueError("stream: only for torch tensors on the GPU (numpy arrays go through the blocking host entry)")
    batch = RtxPointBatch()
    lib.rtx_point_batch_defaults(C.byref(batch))
    batch.n, batch.r_max_all, batch.media = io.n, r_max_all, 1 if media else 0
    batch.points, batch.time, batch.r_max = io.ptr(points), io.ptr(times), io.ptr(r_max)
    cols = {name: io.empty((io.n,) + _NEAREST_COLUMN_SHAPES[name], "int32" if name == "ids" else "float64") for name in want}
    out = RtxNearest(*[io.ptr(cols.get(name)) for name in NEAREST_COLUMNS])
    io.call(lib.rtx_scene_nearest, lib.rtx_scene_nearest_device, (scene.ptr, C.byref(batch), C.byref(out)), stream=stream)
    return Nearest(io.n, cols)


class RadianceSums:
    """What Scene.trace_rays returns: n rays, spp samples summed per ray so far; sum (n, 3) and sumsq (n, 3) or None (numpy
    arrays, or torch tensors on the rays' device); mean = sum / spp."""

    def __init__(self, n, spp, sum, sumsq, stats=None):
        self.n, self.spp, self.sum, self.sumsq, self.stats = n, spp, sum, sumsq, stats

    @property
    def mean(self):
        return self.sum / self.spp


def _trace_rays(scene, origins, directions, times, spp, max_depth, background, seed, first_sample, first_ray, light_sampling,
                sumsq, out, sample_buffer_bytes, want_stats):
    io = _QueryArrays([("origins", origins, 3), ("directions", directions, 3), ("times", times, 0)])
    n, on_device = io.n, io.on_device
    for name, v, lo in (("spp", spp, 1), ("max_depth", max_depth, 1), ("first_sample", first_sample, 0), ("first_ray", first_ray, 0)):
        if int(v) != v or v < lo:
            raise ValueError("%s: must be an integer >= %d, not %r" % (name, lo, v))
    if first_sample + spp > 2 ** 32:
        raise ValueError("first_sample: first_sample + spp is past 2^32")
    background = tuple(float(c) for c in background)
    if len(background) != 3 or any(c != c for c in background):
        raise ValueError("background: three numbers, none a NaN")
    if out is not None:
        if not isinstance(out, RadianceSums):
            raise ValueError("out: expected what an earlier trace_rays call returned")
        if out.n != n or _is_torch(out.sum) != on_device or (on_device and out.sum.device != origins.device):
            raise ValueError("out: holds %d rays of another kind or device, the batch has %d" % (out.n, n))
        if first_sample != out.spp:
            raise ValueError("out: holds %d samples per ray, so first_sample must be %d, not %d" % (out.spp, out.spp, first_sample))
        if sumsq and out.sumsq is None:
            raise ValueError("out: has no sumsq to continue")
        s_arr, q_arr = out.sum, out.sumsq
    else:
        s_arr = io.empty((n, 3))
        q_arr = io.empty((n, 3)) if sumsq else None
    q = RtxRadianceRays()
    lib.rtx_radiance_rays_defaults(C.byref(q))
    q.n, q.origin, q.direction, q.time = n, io.ptr(origins), io.ptr(directions), io.ptr(times)
    q.first_ray, q.first_sample, q.samples, q.max_depth = first_ray, first_sample, spp, max_depth
    q.accumulate, q.seed, q.light_sampling, q.sample_buffer_bytes = 1 if out is not None else 0, seed, 1 if light_sampling else 0, sample_buffer_bytes
    q.background[:] = background
    stats = RtxRenderStats() if want_stats else None
    # (n = 0: the entry still wants a sum pointer; any non-NULL one does, nothing is written)
    io.call(lib.rtx_scene_trace_rays, lib.rtx_scene_trace_rays_device,
            (scene.ptr, C.byref(q), _VP(io.addr(s_arr) or 8), _VP(io.ptr(q_arr))), tail=(C.byref(stats) if stats else None,))
    if out is not None:
        out.spp += spp
        out.stats = stats
        return out
    return RadianceSums(n, spp, s_arr, q_arr, stats)


class GatherSums:
    """What Scene.gather returns: n points, spp samples summed per point so far, the form ("surface" or "probe") and sh_order;
    sum and sumsq (or None) of shape (n, 3), or (n, K, 3) with sh_order > 0 (numpy arrays, or torch tensors on the points'
    device).  mean = sum / spp; irradiance = pi * mean (the surface form, else None); sh = 4 pi * sum / spp, the coefficient
    estimates (sh_order > 0, else None)."""

    def __init__(self, n, spp, sum, sumsq, surface, sh_order, stats=None):
        self.n, self.spp, self.sum, self.sumsq, self.surface, self.sh_order, self.stats = n, spp, sum, sumsq, surface, sh_order, stats

    @property
    def form(self):
        return "surface" if self.surface else "probe"

    @property
    def mean(self):
        return self.sum / self.spp

    @property
    def irradiance(self):
        return self.sum * (np.pi / self.spp) if self.surface else None

    @property
    def sh(self):
        return self.sum * (4.0 * np.pi / self.spp) if self.sh_order > 0 else None


def _gather_scalars(spp, max_depth, first_sample, first_point, sh_order):
    for name, v, lo in (("spp", spp, 1), ("max_depth", max_depth, 1), ("first_sample", first_sample, 0), ("first_point", first_point, 0)):
        if int(v) != v or v < lo:
            raise ValueError("%s: must be an integer >= %d, not %r" % (name, lo, v))
    if first_sample + spp > 2 ** 32:
        raise ValueError("first_sample: first_sample + spp is past 2^32")
    if sh_order not in (0, 1, 2):
        raise ValueError("sh_order: must be 0, 1 or 2, not %r" % (sh_order,))


def _gather(scene, points, normals, times, spp, max_depth, background, seed, light_sampling, sh_order, first_point, first_sample,
            sumsq, out, stream, sample_buffer_bytes, want_stats):
    # (normals may be left out: the probe form; a column that is given is checked like any other)
    io = _QueryArrays([("points", points, 3)] + ([("normals", normals, 3)] if normals is not None else []) + [("times", times, 0)])
    n, on_device = io.n, io.on_device
    _gather_scalars(spp, max_depth, first_sample, first_point, sh_order)
    surface = normals is not None
    if sh_order and surface:
        raise ValueError("sh_order: spherical harmonics are for the probe form (normals=None)")
    background = tuple(float(c) for c in background)
    if len(background) != 3 or any(c != c for c in background):
        raise ValueError("background: three numbers, none a NaN")
    if stream is not None and not on_device:
        raise ValueError("stream: only for torch tensors on the GPU (numpy arrays go through the blocking host entry)")
    shape = (n, 3) if sh_order == 0 else (n, (sh_order + 1) ** 2, 3)
    if out is not None:
        if not isinstance(out, GatherSums):
            raise ValueError("out: expected what an earlier gather call returned")
        if out.n != n or _is_torch(out.sum) != on_device or (on_device and out.sum.device != points.device):
            raise ValueError("out: holds %d points of another kind or device, the batch has %d" % (out.n, n))
        if out.surface != surface or out.sh_order != sh_order:
            raise ValueError("out: holds %s sums of sh_order %d, the call asks for %s sums of sh_order %d"
                             % (out.form, out.sh_order, "surface" if surface else "probe", sh_order))
        if first_sample != out.spp:
            raise ValueError("out: holds %d samples per point, so first_sample must be %d, not %d" % (out.spp, out.spp, first_sample))
        if sumsq and out.sumsq is None:
            sumsq = False  # (what the first call asked for holds)
        s_arr, q_arr = out.sum, out.sumsq
    else:
        s_arr = io.empty(shape)
        q_arr = io.empty(shape) if sumsq else None
    q = RtxGatherPoints()
    lib.rtx_gather_points_defaults(C.byref(q))
    q.n, q.position, q.normal, q.time = n, io.ptr(points), io.ptr(normals), io.ptr(times)
    q.first_point, q.first_sample, q.samples, q.max_depth = first_point, first_sample, spp, max_depth
    q.accumulate, q.seed, q.light_sampling, q.sh_order = 1 if out is not None else 0, seed, 1 if light_sampling else 0, sh_order
    q.sample_buffer_bytes = sample_buffer_bytes
    q.background[:] = background
    if surface and n == 0:
        q.normal = 8  # (an empty batch has no column addresses; the form is still the surface one)
    stats = RtxRenderStats() if want_stats else None
    io.call(lib.rtx_scene_gather, lib.rtx_scene_gather_device,
            (scene.ptr, C.byref(q), _VP(io.addr(s_arr) or 8), _VP(io.ptr(q_arr))), tail=(C.byref(stats) if stats else None,), stream=stream)
    if out is not None:
        out.spp += spp
        out.stats = stats
        return out
    return GatherSums(n, spp, s_arr, q_arr, surface, sh_order, stats)


def gather_directions(n, normals=None, *, spp=1, seed=1, first_point=0, first_sample=0, f32=False):
    """The start directions Scene.gather draws (rtx_gather_directions; host only, no GPU): (n, spp, 3) float64, the direction of
    sample first_sample + s of point first_point + r -- normals[r] + a unit vector with normals (n, 3), a unit vector without
    -- in f64 arithmetic or, f32=True, in an f32 scene's float arithmetic, widened."""
    if int(n) != n or n < 0:
        raise ValueError("n: must be an integer >= 0, not %r" % (n,))
    _gather_scalars(spp, 1, first_sample, first_point, 0)
    if normals is not None:
        if not isinstance(normals, np.ndarray) or normals.dtype != np.float64 or not normals.flags["C_CONTIGUOUS"] or normals.shape != (n, 3):
            raise ValueError("normals: expected a contiguous float64 numpy array of shape (%d, 3)" % n)
    q = RtxGatherPoints()
    lib.rtx_gather_points_defaults(C.byref(q))
    q.n, q.first_point, q.first_sample, q.samples, q.seed = n, first_point, first_sample, spp, seed
    q.normal = normals.ctypes.data if normals is not None and n else None
    if normals is not None and n == 0:
        q.normal = 8
    out = np.empty((n, spp, 3))
    _check(lib.rtx_gather_directions(C.byref(q), 1 if f32 else 0, _VP(out.ctypes.data or 8)))
    return out


class Progressive:
    """Accumulators of one (scene, camera, config, shard) kept on the device across calls (rtx_progressive_*).

    After k samples, however they were split into add() calls, screen() and moments() are bit-identical to a one-shot
    render at k spp.  Holds a reference to its Scene, which must not render on another stream while this one does.
    add_adaptive() / until_adaptive() stop tracing the pixels that reach a target error (rtx_abi.h gives the rule); a pixel
    that stopped at n_p samples (pixel_spp()) then holds the bits of a one-shot render at n_p spp.
    """

    def __init__(self, scene, cam, cfg, shard=None, light_sampling=False):
        self.scene = scene  # the handle must be destroyed before its scene
        self.width = cfg.image_width
        self.height = shard_rows(cfg, shard) if shard is not None else image_height(cfg)
        sh = RtxShard(*shard, 0) if shard is not None else None
        p = _VP()
        if light_sampling:
            opt = _integrator_options(True)
            _check(lib.rtx_progressive_create_ex(scene.ptr, C.byref(cam), C.byref(cfg), C.byref(sh) if sh else None,
                                                 C.byref(opt), C.byref(p)))
        else:
            _check(lib.rtx_progressive_create(scene.ptr, C.byref(cam), C.byref(cfg), C.byref(sh) if sh else None,
                                              C.byref(p)))
        self._p = p

    def __del__(self):
        p, self._p = getattr(self, "_p", None), None
        if p:
            lib.rtx_progressive_destroy(p)

    @property
    def spp_done(self):
        return lib.rtx_progressive_spp(self._p)

    def add(self, n, stream=0, want_stats=False):
        """Trace the next n samples of every pixel (asynchronous on `stream` unless want_stats)."""
        stats = RtxRenderStats() if want_stats else None
        _check(lib.rtx_progressive_add(self._p, n, _VP(stream or None), C.byref(stats) if stats else None))
        return stats

    def screen(self, want_accum=True):
        """The frame at the current sample count, as Scene.render returns it (each pixel tone-mapped at its own count)."""
        accum = np.zeros((self.height, self.width, 3), dtype=np.float64) if want_accum else None
        rgb8 = np.zeros((self.height, self.width, 3), dtype=np.uint8)
        frame = RtxFrame(accum.ctypes.data_as(_D3) if want_accum else None, rgb8.ctypes.data_as(C.POINTER(C.c_uint8)))
        _check(lib.rtx_progressive_read(self._p, C.byref(frame), None))
        return Screen(self.width, self.height, rgb8, accum)

    def moments(self):
        """(S, Q): per-pixel sums of the samples' radiances and of their squares, shaped like Screen.accum."""
        s = np.zeros((self.height, self.width, 3), dtype=np.float64)
        q = np.zeros_like(s)
        frame = RtxFrame(s.ctypes.data_as(_D3), None)
        _check(lib.rtx_progressive_read(self._p, C.byref(frame), q.ctypes.data_as(_D3)))
        return s, q

    def stats(self, target_rel_err=0.0):
        out = RtxNoiseStats()
        _check(lib.rtx_progressive_stats(self._p, target_rel_err, C.byref(out)))
        return out

    def until(self, batch, target_rel_err):
        """Add `batch` samples at a time until no pixel's relative error exceeds the target, or the budget is spent."""
        out = RtxNoiseStats()
        _check(lib.rtx_progressive_until(self._p, batch, target_rel_err, C.byref(out)))
        return out

    def add_adaptive(self, n, min_spp, target_rel_err, stream=0, want_stats=False):
        """One adaptive round: retire the pixels at or below the target (once spp_done >= min_spp), then trace the next n
        samples of the others."""
        stats = RtxRenderStats() if want_stats else None
        _check(lib.rtx_progressive_add_adaptive(self._p, n, min_spp, target_rel_err, _VP(stream or None),
                                                C.byref(stats) if stats else None))
        return stats

    def until_adaptive(self, batch, min_spp, target_rel_err):
        """Adaptive rounds of `batch` samples until no pixel is active or the budget is spent -> RtxAdaptiveStats."""
        out = RtxAdaptiveStats()
        _check(lib.rtx_progressive_until_adaptive(self._p, batch, min_spp, target_rel_err, C.byref(out)))
        return out

    def pixel_spp(self):
        """Samples each pixel holds (int32, rows x width; 0 on rows row_chunk_compat never renders)."""
        out = np.zeros((self.height, self.width), dtype=np.int32)
        _check(lib.rtx_progressive_pixel_spp(self._p, out.ctypes.data_as(C.POINTER(C.c_int32))))
        return out

    def features(self, feature_spp=4):
        """First-hit (albedo, normal) averaged over feature_spp samples: float32 arrays shaped like Screen.accum."""
        albedo = np.zeros((self.height, self.width, 3), dtype=np.float32)
        normal = np.zeros_like(albedo)
        _check(lib.rtx_progressive_features(self._p, feature_spp, albedo.ctypes.data_as(_F3), normal.ctypes.data_as(_F3)))
        return albedo, normal

    def denoise(self, **params):
        """The denoised frame (rtx_progressive_denoise; keyword arguments: the fields of RtxDenoiseParams, 0 = default) ->
        Screen whose accum is the denoised per-pixel MEAN radiance and rgb8 its tone map.  S and Q are not touched."""
        prm = denoise_params(**params)
        accum = np.zeros((self.height, self.width, 3), dtype=np.float64)
        rgb8 = np.zeros((self.height, self.width, 3), dtype=np.uint8)
        _check(lib.rtx_progressive_denoise(self._p, C.byref(prm), accum.ctypes.data_as(_D3),
                                           rgb8.ctypes.data_as(C.POINTER(C.c_uint8))))
        return Screen(self.width, self.height, rgb8, accum)


class MultiScene:
    """The scene resident on several GPUs of this process (rtx_multi): row-interleaved shards, one RCCL gather."""

    def __init__(self, flat, n_shards, device_ids=None, block_rows=1, f32=False):
        ids = (C.c_int32 * n_shards)(*device_ids) if device_ids is not None else None
        p = _VP()
        _check((lib.rtx_multi_create_f32 if f32 else lib.rtx_multi_create)(flat.ptr, n_shards, ids, block_rows, C.byref(p)))
        self._p = p

    def __del__(self):
        p, self._p = getattr(self, "_p", None), None
        if p:
            lib.rtx_multi_destroy(p)

    def render(self, cam, cfg, want_accum=True):
        w, h = cfg.image_width, image_height(cfg)
        accum = np.zeros((h, w, 3), dtype=np.float64) if want_accum else None
        rgb8 = np.zeros((h, w, 3), dtype=np.uint8)
        frame = RtxFrame(accum.ctypes.data_as(C.POINTER(C.c_double)) if want_accum else None,
                         rgb8.ctypes.data_as(C.POINTER(C.c_uint8)))
        stats = RtxMultiStats()
        _check(lib.rtx_multi_render(self._p, C.byref(cam), C.byref(cfg), C.byref(frame), C.byref(stats)))
        screen = Screen(w, h, rgb8, accum)
        screen.stats = stats
        return screen


def render_multi(flat, cam, cfg, n_gpus, want_accum=True):
    """rtx_render_multi: create on devices 0..n_gpus-1, render once, destroy."""
    w, h = cfg.image_width, image_height(cfg)
    accum = np.zeros((h, w, 3), dtype=np.float64) if want_accum else None
    rgb8 = np.zeros((h, w, 3), dtype=np.uint8)
    frame = RtxFrame(accum.ctypes.data_as(C.POINTER(C.c_double)) if want_accum else None,
                     rgb8.ctypes.data_as(C.POINTER(C.c_uint8)))
    _check(lib.rtx_render_multi(flat.ptr, C.byref(cam), C.byref(cfg), n_gpus, C.byref(frame)))
    return Screen(w, h, rgb8, accum)


def trace_kernel_name(kernel):
    return (lib.rtx_trace_kernel_name(kernel) or b"").decode()


# rtx_device_math's float entries: evaluated by the f32 compilation on float(x), float(y), the float result widened.  The
# three rng_* entries take a raw 64-bit draw as the BITS of x (and, for rng_range_f32, float lo / hi as the low / high word of y).
DEVICE_MATH_F32 = {"sinf": 32, "cosf": 33, "logf": 34, "acosf": 35, "atan2f": 36, "sqrtf": 37, "divf": 38, "sin_signf": 39,
                   "rng_f32": 40, "rng_range_f32": 41, "rng_range_pm1_f32": 42, "slope_capf": 43}


def device_math(fn, x, y=None):
    """Evaluate one arithmetic building block on the GPU (see rtx_device_math)."""
    names = {"sin": 0, "cos": 1, "log": 2, "acos": 3, "atan2": 4, "tan": 5, "sqrt": 6, "div": 7, "muladd": 8, "floor": 9, "wide_key": 10}
    names.update(DEVICE_MATH_F32)
    x = np.ascontiguousarray(x, dtype=np.float64)
    y = np.ascontiguousarray(y if y is not None else np.ones_like(x), dtype=np.float64)
    out = np.empty_like(x)
    _check(lib.rtx_device_math(names[fn], x.ctypes.data_as(_D3), y.ctypes.data_as(_D3), x.size, out.ctypes.data_as(_D3)))
    return out


# rtx_device_walk_steps: RtxWalkStepItem as a numpy record (88 bytes)
WALK_STEP_ITEM = np.dtype([("node", "<i4"), ("second_node", "<i4"), ("q", "<f4", (8,)), ("dir", "<f8", (3,)), ("t_max32", "<f4"),
                           ("n_stack", "<i4"), ("stack", "<i4", (4,))])
WALK_GUARD_SLOTS, WALK_CANARY, WALK_UNWRITTEN = 4, 0x5CA1AB1E, 0x0BADF00D
CULL_VERDICT_BITS = ("may_hit", "nf", "nf_pos", "hit2_a", "hit2_b", "wide")  # bit 6: nf_pos was asked (t_min > 0)


def device_cull_verdicts(box, ray, f32=False):
    """The f32 box tests on the GPU (rtx_device_cull_verdicts): box (n, 6) lo / hi in f64, ray (n, 8) origin, direction, t_min,
    t_max in f64 -> (ray32 (n, 8) float32, key (n,) float32, verdict (n,) uint32)."""
    box = np.ascontiguousarray(box, dtype=np.float64).reshape(-1, 6)
    ray = np.ascontiguousarray(ray, dtype=np.float64).reshape(-1, 8)
    n = box.shape[0]
    if ray.shape[0] != n:
        raise ValueError("%d boxes, %d rays" % (n, ray.shape[0]))
    q, key, v = np.zeros((n, 8), dtype=np.float32), np.zeros(n, dtype=np.float32), np.zeros(n, dtype=np.uint32)
    _check(lib.rtx_device_cull_verdicts(1 if f32 else 0, n, box.ctypes.data_as(_D3), ray.ctypes.data_as(_D3), q.ctypes.data_as(_F3),
                                        key.ctypes.data_as(_F3), v.ctypes.data_as(C.POINTER(C.c_uint32))))
    return q, key, v


def device_walk_steps(kind, bottom, nodes, levels, items, f32=False):
    """One walk step per item on the GPU (rtx_device_walk_steps).  kind "step32" / "step4"; nodes: the records as a numpy array
    of 64- / 128-byte elements; items: WALK_STEP_ITEM records -> (cur (n,), n (n,), slots (n, levels + WALK_GUARD_SLOTS))."""
    k = {"step32": 0, "step4": 1}[kind]
    nodes = np.ascontiguousarray(nodes)
    if nodes.dtype.itemsize != (128 if k else 64):
        raise ValueError("%s takes %d-byte records" % (kind, 128 if k else 64))
    items = np.ascontiguousarray(items, dtype=WALK_STEP_ITEM)
    out = np.zeros((len(items), 2 + levels + WALK_GUARD_SLOTS), dtype=np.int32)
    _check(lib.rtx_device_walk_steps(1 if f32 else 0, k, 1 if bottom else 0, nodes.ctypes.data_as(_VP), len(nodes), levels, len(items),
                                     items.ctypes.data_as(_VP), out.ctypes.data_as(C.POINTER(C.c_int32))))
    return out[:, 0], out[:, 1], out[:, 2:]


def device_stream(seed, pixel, sample, n):
    out = np.empty(n, dtype=np.float64)
    _check(lib.rtx_device_stream(seed, pixel, sample, n, out.ctypes.data_as(_D3)))
    return out


def _moments_arg(S, Q):
    S = np.ascontiguousarray(S, dtype=np.float64).reshape(-1, 3)
    Q = np.ascontiguousarray(Q, dtype=np.float64).reshape(-1, 3)
    if S.shape != Q.shape:
        raise ValueError("S and Q must have the same shape")
    return S, Q


def device_retire(S, Q, active, spp, target, counts):
    """One adaptive retirement check on the GPU (see rtx_device_retire) over the pixels of S, Q (npix x 3 or rows x w x 3).
    -> (the ascending list of the pixels kept active, counts after the check); the inputs are not changed."""
    S, Q = _moments_arg(S, Q)
    active = np.ascontiguousarray(active, dtype=np.uint32).ravel()
    counts = np.array(counts, dtype=np.int32).ravel()  # a copy: written in place
    if counts.size != S.shape[0]:
        raise ValueError("counts must hold one entry per pixel")
    nxt = np.zeros(max(active.size, 1), dtype=np.uint32)
    kept = C.c_uint32()
    u32 = C.POINTER(C.c_uint32)
    _check(lib.rtx_device_retire(S.ctypes.data_as(_D3), Q.ctypes.data_as(_D3), S.shape[0], active.ctypes.data_as(u32),
                                 active.size, spp, target, counts.ctypes.data_as(C.POINTER(C.c_int32)), nxt.ctypes.data_as(u32),
                                 C.byref(kept)))
    return nxt[:kept.value].copy(), counts


def device_noise_reduce(S, Q, spp, target, counts=None):
    """The noise reduction of rtx_progressive_stats on the GPU (see rtx_device_noise_reduce) -> (max r, sum r, count above)."""
    S, Q = _moments_arg(S, Q)
    if counts is not None:
        counts = np.ascontiguousarray(counts, dtype=np.int32).ravel()
        if counts.size != S.shape[0]:
            raise ValueError("counts must hold one entry per pixel")
    max_r, sum_r, above = C.c_double(), C.c_double(), C.c_uint64()
    _check(lib.rtx_device_noise_reduce(S.ctypes.data_as(_D3), Q.ctypes.data_as(_D3),
                                       counts.ctypes.data_as(C.POINTER(C.c_int32)) if counts is not None else None,
                                       S.shape[0], spp, target, C.byref(max_r), C.byref(sum_r), C.byref(above)))
    return max_r.value, sum_r.value, above.value


def denoise_params(**params):
    """RtxDenoiseParams from keyword arguments (iterations, feature_spp, demodulate, sigma_luminance, sigma_normal,
    sigma_albedo); what is not given is 0, the default."""
    prm = RtxDenoiseParams()
    names = [n for n, _ in RtxDenoiseParams._fields_ if n != "reserved"]
    for k, v in params.items():
        if k not in names:
            raise TypeError("unknown denoise parameter %r (expected one of %s)" % (k, ", ".join(names)))
        setattr(prm, k, v)
    return prm


def device_denoise(mean, var, albedo, normal, **params):
    """The denoising filter on the GPU for host arrays (see rtx_device_denoise): mean and var (the variance of the mean) per
    pixel and channel, albedo and normal guides, each rows x width x 3 -> (denoised mean f64, its rgb8)."""
    mean = np.ascontiguousarray(mean, dtype=np.float64)
    if mean.ndim != 3 or mean.shape[2] != 3:
        raise ValueError("mean must be rows x width x 3")
    var = np.ascontiguousarray(var, dtype=np.float64)
    albedo = np.ascontiguousarray(albedo, dtype=np.float32)
    normal = np.ascontiguousarray(normal, dtype=np.float32)
    for a in (var, albedo, normal):
        if a.shape != mean.shape:
            raise ValueError("mean, var, albedo and normal must have the same shape")
    h, w = mean.shape[:2]
    prm = denoise_params(**params)
    out = np.zeros_like(mean)
    rgb8 = np.zeros(mean.shape, dtype=np.uint8)
    _check(lib.rtx_device_denoise(mean.ctypes.data_as(_D3), var.ctypes.data_as(_D3), albedo.ctypes.data_as(_F3),
                                  normal.ctypes.data_as(_F3), w, h, C.byref(prm), out.ctypes.data_as(_D3),
                                  rgb8.ctypes.data_as(C.POINTER(C.c_uint8))))
    return out, rgb8


def shard_rows(cfg, shard):
    sh = RtxShard(*shard, 0)
    return lib.rtx_shard_rows(C.byref(cfg), C.byref(sh))


class Screen:
    """Framebuffer in the reference's layout: row j = 0 is the bottom image row (screen.rs:30-48)."""

    def __init__(self, width, height, rgb8, accum=None):
        self.width, self.height, self.rgb8, self.accum = width, height, rgb8, accum

    def write_to_ppm_file(self, path):
        buf = np.ascontiguousarray(self.rgb8)
        _check(lib.rtx_write_ppm(os.fsencode(path), self.width, self.height, buf.ctypes.data_as(C.POINTER(C.c_uint8))))

    def write_to_ppm(self):
        sys.stdout.flush()
        buf = np.ascontiguousarray(self.rgb8)
        _check(lib.rtx_write_ppm(None, self.width, self.height, buf.ctypes.data_as(C.POINTER(C.c_uint8))))


def render_scene(builder, world, cam, background, config, max_leaf=0):
    """render_scene(world, cam, background, config) -- world.rs:1181-1247, on the current GPU.

    Returns the Screen instead of printing it; call .write_to_ppm() for the reference's stdout output.
    """
    cfg = RtxConfig.from_buffer_copy(config)
    cfg.background[0], cfg.background[1], cfg.background[2] = background
    scene = builder.flatten(world, max_leaf=max_leaf).upload()
    return scene.render(cam, cfg)


def render_scene_progressive(builder, world, cam, background, config, batch, target_rel_err, max_leaf=0, adaptive=False,
                             min_spp=2, denoise=False, light_sampling=False):
    """render_scene, refined `batch` samples at a time until no pixel's relative error exceeds target_rel_err or
    config.samples_per_pixel is reached.  Returns (Screen, RtxNoiseStats of the last batch).
    adaptive=True: pixels at or below the target stop receiving samples (checked from min_spp samples on); returns
    (Screen, RtxAdaptiveStats), and Screen.spp holds each pixel's sample count.
    denoise=True: the Screen is the denoised frame (Progressive.denoise with the default parameters; accum is the MEAN
    radiance, not a sum) and Screen.noisy holds the frame as accumulated.
    light_sampling=True: every batch traces with next-event estimation and MIS (statistical; rtx_progressive_create_ex)."""
    cfg = RtxConfig.from_buffer_copy(config)
    cfg.background[0], cfg.background[1], cfg.background[2] = background
    scene = builder.flatten(world, max_leaf=max_leaf).upload()
    prog = scene.progressive(cam, cfg, light_sampling=light_sampling)
    if adaptive:
        stats = prog.until_adaptive(batch, min_spp, target_rel_err)
    else:
        stats = prog.until(batch, target_rel_err)
    screen = prog.screen()
    if adaptive:
        screen.spp = prog.pixel_spp()
    if denoise:
        noisy, screen = screen, prog.denoise()
        screen.noisy = noisy
        if adaptive:
            screen.spp = noisy.spp
    return screen, stats
