"""Light sampling's C ABI and Python surface, without a GPU: struct layout, the light census of the catalogue and of
hand-built worlds (rtx_flat_lights), and the argument checks of the *_ex entry points."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["rtx_flat_lights", "rtx_render_ex", "rtx_progressive_create_ex"]


def test_symbols_are_declared_exported_and_bound(rtsr):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rtx_abi.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(rtx_[a-z0-9_]+)\s*\(", text))
    lib = C.CDLL(rtsr.LIB_PATH)
    for name in NEW:
        assert name in declared and hasattr(lib, name) and name in rtsr.ABI, name
    assert b"k_trace_nee" in open(rtsr.LIB_PATH, "rb").read()
    assert rtsr.trace_kernel_name(8) == "k_trace_nee"
    names = ["k_trace_simple", "k_trace_persistent", "k_trace_stream", "k_trace_vote", "k_trace_lds", "k_trace_wq",
             "k_trace_world", "k_wf_trace"]
    assert [rtsr.trace_kernel_name(k) for k in range(8)] == names
    assert rtsr.lib.rtx_abi_version() == 1


def test_struct_layouts(rtsr):
    o, li = rtsr.RtxIntegratorOptions, rtsr.RtxLightInfo
    assert C.sizeof(o) == 16 and C.sizeof(li) == 24
    assert [(n, getattr(o, n).offset) for n, _ in o._fields_] == [("light_sampling", 0), ("reserved", 4)]
    assert [(n, getattr(li, n).offset) for n, _ in li._fields_] == [
        ("n_lights", 0), ("n_rect_lights", 4), ("n_sphere_lights", 8), ("n_unsampled_emitters", 12), ("total_area", 16)]


def _census(rtsr, scene_id, **kw):
    b = rtsr.Builder(1)
    world, _, _ = b.get_world_cam(scene_id, **kw)
    return b.flatten(world).lights()


@pytest.mark.parametrize("scene_id,n_lights,n_rect,n_sphere,area", [
    (3, 2, 1, 1, None),
    (4, 1, 1, 0, 130.0 * 105.0),   # XzRect(213, 343, 227, 332, 554)
    (5, 1, 1, 0, 130.0 * 105.0),
    (6, 1, 1, 0, 309.0 * 265.0),   # XzRect(123, 432, 147, 412, 554), world.rs:521
    (12, 1, 1, 0, 130.0 * 105.0),
    (100, 0, 0, 0, 0.0),
])
def test_catalogue_census(rtsr, scene_id, n_lights, n_rect, n_sphere, area):
    kw = {"book2_boxes_per_side": 4, "book2_spheres": 50} if scene_id == 6 else {}
    c = _census(rtsr, scene_id, **kw)
    assert (c["n_lights"], c["n_rect_lights"], c["n_sphere_lights"], c["n_unsampled_emitters"]) == (n_lights, n_rect, n_sphere, 0)
    if area is not None:
        assert c["total_area"] == pytest.approx(area, rel=1e-12)


def test_dragon_room_census(rtsr):
    c = _census(rtsr, 11, mesh_triangles=2000)
    assert (c["n_lights"], c["n_rect_lights"], c["n_sphere_lights"], c["n_unsampled_emitters"]) == (1, 1, 0, 0)
    assert c["total_area"] == pytest.approx(200.0 * 200.0, rel=1e-12)  # XzRect(-100, 100, -100, 100, 55), world.rs:739


def test_simple_light_census_areas(rtsr):
    # world.rs simple_light: XyRect(3, 5, 1, 3, -2) and a sphere of radius 3, both DiffuseLight
    c = _census(rtsr, 3)
    assert c["total_area"] == pytest.approx(2.0 * 2.0 + 4.0 * 3.141592653589793 * 9.0, rel=1e-12)


def _hand_built(rtsr, wrap):
    b = rtsr.Builder(1)
    white = b.lambertian(b.solid_color((0.73, 0.73, 0.73)))
    light = b.diffuse_light(b.solid_color((15.0, 15.0, 15.0)))
    lst = b.hittable_list()
    b.list_add(lst, b.yz_rect(0, 555, 0, 555, 555, white))
    b.list_add(lst, b.xz_rect(0, 555, 0, 555, 0, white))
    b.list_add(lst, wrap(b, light))
    return b.flatten(lst).lights()


@pytest.mark.parametrize("name", ["translate", "bvh", "moving_sphere"])
def test_wrapped_emitters_are_unsampled(rtsr, name):
    def wrap(b, light):
        if name == "translate":
            return b.translate((0.0, 0.0, 0.0), b.xz_rect(213, 343, 227, 332, 554, light))
        if name == "bvh":
            inner = b.hittable_list()
            b.list_add(inner, b.xz_rect(213, 343, 227, 332, 554, light))
            b.list_add(inner, b.sphere((100.0, 100.0, 100.0), 20.0, b.lambertian(b.solid_color((0.5, 0.5, 0.5)))))
            return b.bvh_from_list(inner, 0.0, 1.0)
        return b.moving_sphere((200.0, 400.0, 200.0), (220.0, 400.0, 200.0), 0.0, 1.0, 30.0, light)

    c = _hand_built(rtsr, wrap)
    assert (c["n_lights"], c["n_unsampled_emitters"]) == (0, 1), c


def test_plain_light_in_hand_built_world_is_sampled(rtsr):
    c = _hand_built(rtsr, lambda b, light: b.xz_rect(213, 343, 227, 332, 554, light))
    assert (c["n_lights"], c["n_rect_lights"], c["n_unsampled_emitters"]) == (1, 1, 0)
    assert c["total_area"] == pytest.approx(130.0 * 105.0)


def test_argument_errors_before_any_device_call(rtsr):
    lib = rtsr.lib
    cam = rtsr.Camera.new((278, 278, -800), (278, 278, 0), (0, 1, 0), 40.0, 1.0, 0.0, 10.0, 0.0, 1.0)
    cfg = rtsr.Config.new(1.0, 8, 4, 5, 1)
    frame = rtsr.RtxFrame(None, None)
    out = C.c_void_p()
    bogus = C.c_void_p(1)  # never dereferenced: the options are checked first
    assert lib.rtx_flat_lights(None, C.byref(rtsr.RtxLightInfo())) == rtsr.RTX_EINVAL
    for opt in (rtsr.RtxIntegratorOptions(2), rtsr.RtxIntegratorOptions(-1), rtsr.RtxIntegratorOptions(1, (0, 1, 0)),
                rtsr.RtxIntegratorOptions(0, (0, 0, 7))):
        assert lib.rtx_render_ex(bogus, C.byref(cam), C.byref(cfg), C.byref(opt), C.byref(frame), None) == rtsr.RTX_EINVAL
        assert "light_sampling" in rtsr.last_error() or "reserved" in rtsr.last_error()
        assert lib.rtx_progressive_create_ex(bogus, C.byref(cam), C.byref(cfg), None, C.byref(opt), C.byref(out)) == \
            rtsr.RTX_EINVAL
        assert not out.value
    ok = rtsr.RtxIntegratorOptions(1)
    assert lib.rtx_render_ex(None, C.byref(cam), C.byref(cfg), C.byref(ok), C.byref(frame), None) == rtsr.RTX_EINVAL
    assert lib.rtx_render_ex(bogus, C.byref(cam), C.byref(cfg), C.byref(ok), None, None) == rtsr.RTX_EINVAL
    assert lib.rtx_progressive_create_ex(None, C.byref(cam), C.byref(cfg), None, C.byref(ok), C.byref(out)) == rtsr.RTX_EINVAL
    assert lib.rtx_progressive_create_ex(bogus, C.byref(cam), C.byref(cfg), None, C.byref(ok), None) == rtsr.RTX_EINVAL


def test_app_knows_the_flag():
    src = open(os.path.join(ROOT, "ray-tracing-series-rust_amd", "apps", "rtx_render.cpp")).read()
    assert '"--light-sampling"' in src
