"""The C ABI and the Python surface of the shading edits, without a GPU: struct layouts, the kind constants, every refusal of
the ladder in the ladder's order, and the argument checks of rtx_scene_set_shading that run before any device call."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from shading_cases import FLAT_ARRAYS, build, call_set_shading as _call, raw_edit as _edit, refusals

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["rtx_flat_set_shading", "rtx_scene_set_shading", "rtx_flat_material_info", "rtx_flat_texture_info", "rtx_flat_medium_info"]


def _header():
    return open(os.path.join(ROOT, "include", "rtx_abi.h")).read()


def test_symbols_are_declared_exported_and_bound(rtsr):
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    declared = set(re.findall(r"\b(rtx_[a-z0-9_]+)\s*\(", text))
    lib = C.CDLL(rtsr.LIB_PATH)
    for name in NEW:
        assert name in declared and hasattr(lib, name) and name in rtsr.ABI, name
    assert "} RtxShadingEdit;" in text and rtsr.lib.rtx_abi_version() == 1
    blob = open(rtsr.LIB_PATH, "rb").read()
    assert b"_ZN3rtx13k_set_shading" in blob and b"_ZN5rtx3213k_set_shading" in blob  # both compilations carry the kernel


def test_struct_layouts(rtsr):
    e, m, t, d = rtsr.RtxShadingEdit, rtsr.RtxMaterialInfo, rtsr.RtxTextureInfo, rtsr.RtxMediumInfo
    assert (C.sizeof(e), C.sizeof(m), C.sizeof(t), C.sizeof(d)) == (40, 40, 48, 16)
    offsets = lambda s: [(n, getattr(s, n).offset) for n, _ in s._fields_]
    assert offsets(e) == [("what", 0), ("index", 4), ("v", 8)]
    assert offsets(m) == [("kind", 0), ("tex", 4), ("albedo", 8), ("param", 32)]
    assert offsets(t) == [("kind", 0), ("a", 4), ("b", 8), ("pad", 12), ("color", 16), ("scale", 40)]
    assert offsets(d) == [("material", 0), ("pad", 4), ("neg_inv_density", 8)]
    assert rtsr.SCENE_ARRAYS["materials"] == (15, 48, 32) and rtsr.SCENE_ARRAYS["textures"] == (16, 48, 32)


def test_kind_constants(rtsr):
    """The header's values, the Python module's, and what the flat arrays hold for one material and texture of every kind."""
    text = _header()
    defines = {k: int(v) for k, v in re.findall(r"#define\s+(RTX_(?:MAT|TEX|SHADE)_[A-Z_]+)\s+(\d+)", text)}
    assert defines == {"RTX_SHADE_SOLID_COLOR": 0, "RTX_SHADE_NOISE_SCALE": 1, "RTX_SHADE_METAL": 2, "RTX_SHADE_DIELECTRIC": 3,
                       "RTX_SHADE_MEDIUM_DENSITY": 4, "RTX_MAT_LAMBERTIAN": 0, "RTX_MAT_METAL": 1, "RTX_MAT_DIELECTRIC": 2,
                       "RTX_MAT_DIFFUSE_LIGHT": 3, "RTX_MAT_ISOTROPIC": 4, "RTX_TEX_SOLID": 0, "RTX_TEX_CHECKER": 1, "RTX_TEX_NOISE": 2,
                       "RTX_TEX_IMAGE": 3}
    for k, v in defines.items():
        assert getattr(rtsr, k) == v, k
    b = rtsr.Builder(1)
    tex = [b.solid_color((0.1, 0.2, 0.3)), None, b.noise(2.0), b.image_from_texels(np.zeros((2, 2, 3)))]
    tex[1] = b.checker(tex[0], tex[0])
    mats = [b.lambertian(tex[0]), b.metal((0.5, 0.5, 0.5), 0.1), b.dielectric(1.5), b.diffuse_light(tex[0]), b.isotropic(tex[0])]
    flat = b.flatten(b.hittable_list([b.sphere((0.0, float(k), 0.0), 0.4, m) for k, m in enumerate(mats)]))
    assert [flat.texture(t)["kind"] for t in tex] == list(rtsr.TEXTURE_KINDS)
    assert [flat.material(m)["kind"] for m in mats] == list(rtsr.MATERIAL_KINDS)


def test_every_refusal_leaves_the_flat_scene_unchanged(rtsr):
    case = build(rtsr, "shared_texture")
    flat = case.flatten()
    before = {a: flat.array(a) for a in FLAT_ARRAYS}
    cases = refusals(rtsr, case, flat)
    assert len(cases) == 21
    for edits, n, words in cases:
        assert _call(rtsr, rtsr.lib.rtx_flat_set_shading, flat.ptr, edits, n) == rtsr.RTX_EINVAL, words
        msg = rtsr.last_error()
        assert msg.startswith("rtx_flat_set_shading: ") and all(w in msg for w in words), (words, msg)
        assert all(np.array_equal(flat.array(a), before[a]) for a in FLAT_ARRAYS), words
    good = cases[1][0]
    assert _call(rtsr, rtsr.lib.rtx_flat_set_shading, None, good) == rtsr.RTX_EINVAL and "scene is NULL" in rtsr.last_error()
    # the order of the ladder: NULL scene before n < 0 before NULL edits; `what` before `index` before the kind before the values
    # before the unused values, edit by edit; a target named twice last
    assert _call(rtsr, rtsr.lib.rtx_flat_set_shading, None, None, -1) == rtsr.RTX_EINVAL and "scene is NULL" in rtsr.last_error()
    nan = float("nan")
    S = rtsr.RTX_SHADE_SOLID_COLOR
    shared = case.targets["shared"][1]
    checker = [x for x in range(flat.info()["n_textures"]) if flat.texture(x)["kind"] == "checker"][0]
    ladder = [(_edit(rtsr, 9, -1, nan, 0.0, 0.0, 1.0), "edits[0].what"), (_edit(rtsr, S, -1, nan, 0.0, 0.0, 1.0), "edits[0].index is out of range"),
              (_edit(rtsr, S, checker, nan, 0.0, 0.0, 1.0), "not a SolidColor"), (_edit(rtsr, S, shared, nan, 0.0, 0.0, 1.0), "edits[0].v[0] is not finite"),
              (_edit(rtsr, S, shared, 0.1, 0.0, 0.0, 1.0), "edits[0].v[3]")]
    for first, word in ladder:
        assert _call(rtsr, rtsr.lib.rtx_flat_set_shading, flat.ptr, [first, _edit(rtsr, 9, 0, nan)]) == rtsr.RTX_EINVAL
        assert word in rtsr.last_error(), (word, rtsr.last_error())
    twice = [_edit(rtsr, S, shared, 0.1, 0.2, 0.3), _edit(rtsr, S, shared, 0.1, 0.2, 0.3), _edit(rtsr, S, shared, nan, 0.2, 0.3)]
    assert _call(rtsr, rtsr.lib.rtx_flat_set_shading, flat.ptr, twice) == rtsr.RTX_EINVAL and "edits[2].v[0] is not finite" in rtsr.last_error()
    assert all(np.array_equal(flat.array(a), before[a]) for a in FLAT_ARRAYS)
    # n = 0 is RTX_OK, with or without a pointer
    assert _call(rtsr, rtsr.lib.rtx_flat_set_shading, flat.ptr, None, 0) == rtsr.RTX_OK
    assert _call(rtsr, rtsr.lib.rtx_flat_set_shading, flat.ptr, good, 0) == rtsr.RTX_OK
    flat.set_shading([])
    assert all(np.array_equal(flat.array(a), before[a]) for a in FLAT_ARRAYS)
    # density 0 is no refusal: the builder applies no rule to it either
    flat.set_shading([("medium_density", case.targets["density"][1], 0.0)])
    assert flat.medium(case.targets["density"][1])["neg_inv_density"] == float("-inf")


def test_python_refuses_malformed_tuples(rtsr):
    case = build(rtsr, "shared_texture")
    flat = case.flatten()
    before = {a: flat.array(a) for a in FLAT_ARRAYS}
    for bad in [{"solid_color": 1}, "solid_color", 7, [("solid_colour", 0, (1, 2, 3))], [("solid_color", 0)], [("solid_color", 0, (1, 2))],
                [("solid_color", 0, 1.0)], [("solid_color", 0.5, (1, 2, 3))], [("solid_color", True, (1, 2, 3))], [("metal", 0, (1, 2, 3))],
                [("metal", 0, (1, 2, 3), "x")], [("dielectric", 0, (1.5,))], [("medium_density", 0, 1.0, 2.0)], [("noise_scale", 0, None)], [7]]:
        with pytest.raises(ValueError):
            flat.set_shading(bad)
    assert all(np.array_equal(flat.array(a), before[a]) for a in FLAT_ARRAYS)
    with pytest.raises(rtsr.RtxError) as e:  # well-formed, but the scene says no: the library's message
        flat.set_shading([("metal", 0, (1, 2, 3), 0.5)])
    assert e.value.status == rtsr.RTX_EINVAL and "edits[0].index" in str(e.value)


def test_argument_errors_before_any_device_call(rtsr):
    """A bogus scene pointer is never dereferenced: what needs no scene is checked first."""
    lib = rtsr.lib
    bogus = C.c_void_p(1)
    good = [_edit(rtsr, rtsr.RTX_SHADE_SOLID_COLOR, 0, 0.1, 0.2, 0.3)]
    assert _call(rtsr, lib.rtx_scene_set_shading, None, good, None, None) == rtsr.RTX_EINVAL and "scene is NULL" in rtsr.last_error()
    assert _call(rtsr, lib.rtx_scene_set_shading, bogus, good, -1, None) == rtsr.RTX_EINVAL and "n < 0" in rtsr.last_error()
    assert _call(rtsr, lib.rtx_scene_set_shading, bogus, None, 1, None) == rtsr.RTX_EINVAL and "edits is NULL" in rtsr.last_error()
    assert rtsr.last_error().startswith("rtx_scene_set_shading: ")
    assert _call(rtsr, lib.rtx_scene_set_shading, bogus, good, 0, None) == rtsr.RTX_OK  # n = 0: nothing to do, nothing read
    assert _call(rtsr, lib.rtx_scene_set_shading, bogus, None, 0, None) == rtsr.RTX_OK
    for fn, info in ((lib.rtx_flat_material_info, rtsr.RtxMaterialInfo()), (lib.rtx_flat_texture_info, rtsr.RtxTextureInfo()),
                     (lib.rtx_flat_medium_info, rtsr.RtxMediumInfo())):
        assert fn(None, 0, C.byref(info)) == rtsr.RTX_EINVAL
        assert fn(bogus, 0, None) == rtsr.RTX_EINVAL
