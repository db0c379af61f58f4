"""Posed scenes for tests/test_set_transforms_host.py and tests/test_gpu_set_transforms.py (a helper module, not a test file).

The judge of every test there is the FRESH scene: the same world built by Builder with new rtx_translate offsets and
rtx_rotate_y angles, flattened (and uploaded).  The scenes of tests/instance_scenes.py hard-code their offsets and angles, so
they are built through a recording Builder: it passes every call on and notes each translate / rotate_y in call order; built
again with `values`, the k-th such call takes values[k] instead of what the scene function wrote.  The same list, cut into the
chains of the top-level slots, is the update handed to set_transforms.  Everything here runs on the CPU.
"""
import numpy as np


class _RecordingBuilder:
    def __init__(self, real, values, calls):
        self._real, self._values, self.calls = real, values, calls

    def __getattr__(self, name):
        return getattr(self._real, name)

    def _value(self, given):
        k = len(self.calls)
        return given if self._values is None else self._values[k]

    def translate(self, offset, obj):
        v = tuple(float(x) for x in self._value(offset))
        h = self._real.translate(v, obj)
        self.calls.append(("translate", v, h, obj))
        return h

    def rotate_y(self, angle_degrees, obj):
        v = float(self._value(angle_degrees))
        h = self._real.rotate_y(v, obj)
        self.calls.append(("rotate_y", v, h, obj))
        return h


class Posed:
    """rtsr with a Builder that records (and, given `values`, replaces) the parameters of translate / rotate_y calls."""

    def __init__(self, rtsr, values=None):
        self._rtsr, self._values, self.calls = rtsr, values, []

    def __getattr__(self, name):
        return getattr(self._rtsr, name)

    def Builder(self, seed=1):
        return _RecordingBuilder(self._rtsr.Builder(seed), self._values, self.calls)


def build(rtsr, scene, values=None):
    """scene(rtsr) -> (builder, world, ...).  -> (builder, world, calls): calls[k] = (kind, value, handle, child) in call order."""
    posed = Posed(rtsr, values)
    out = scene(posed)
    return out[0], out[1], posed.calls


def values_of(calls):
    return [c[1] for c in calls]


def chains(calls):
    """The wrapper chains, outermost first, as lists of call indices, in the order their outermost wrapper was made -- which is
    list order for every scene here (members are made in the order they are listed)."""
    by_handle = {c[2]: k for k, c in enumerate(calls)}
    inner = {c[3] for c in calls if c[3] in by_handle}
    out = []
    for k, c in enumerate(calls):
        if c[2] in inner:
            continue
        chain = [k]
        while calls[chain[-1]][3] in by_handle:
            chain.append(by_handle[calls[chain[-1]][3]])
        out.append(chain)
    return out


def chain_slots(flat):
    return [s for s in range(flat.info()["n_top_level"]) if flat.slot_chain(s)]


def updates_for(flat, calls, values, only=None):
    """{slot: ops} that sets the chains of `flat` (all of them, or the slots in `only`) to `values`.  The slots with a chain,
    ascending, are the chains in creation order; the kinds must agree or the scene is not one this helper understands."""
    slots, ch = chain_slots(flat), chains(calls)
    assert len(slots) == len(ch), (len(slots), len(ch))
    out = {}
    for slot, chain in zip(slots, ch):
        assert flat.slot_chain(slot) == [calls[k][0] for k in chain], (slot, flat.slot_chain(slot))
        if only is None or slot in only:
            out[slot] = [(calls[k][0], values[k]) for k in chain]
    return out


def random_values(calls, seed, shift=0.4, only_calls=None):
    """New parameters from a fixed seed: every offset moved by up to `shift` in x and z (and up to shift / 4 upwards), every
    angle drawn anew in (-180, 180).  only_calls: the call indices that change; the others keep their value."""
    rng = np.random.default_rng(seed)
    out = []
    for k, (kind, v, _, _) in enumerate(calls):
        if kind == "translate":
            new = (v[0] + rng.uniform(-shift, shift), v[1] + rng.uniform(0.0, shift / 4), v[2] + rng.uniform(-shift, shift))
        else:
            new = float(rng.uniform(-180.0, 180.0))
        out.append(new if only_calls is None or k in only_calls else v)
    return out


def calls_of_slots(flat, calls, slots):
    """The call indices behind the chains of the given slots."""
    want = set()
    for slot, chain in zip(chain_slots(flat), chains(calls)):
        if slot in slots:
            want.update(chain)
    return want


# ---- arrays (core/flat_types.hpp), f64 and f32 layouts ----
NODE = np.dtype([("bmin", np.float64, (2, 3)), ("bmax", np.float64, (2, 3)), ("child", np.int32, (2,)), ("pad", np.int32, (2,))])
NODE32 = np.dtype([("lo", np.float32, (2, 3)), ("hi", np.float32, (2, 3)), ("child", np.int32, (2,)), ("axis", np.int32), ("pad", np.int32)])
MOTION32 = np.dtype([("lo0", np.float32, (2, 3)), ("hi0", np.float32, (2, 3)), ("dlo", np.float32, (2, 3)), ("dhi", np.float32, (2, 3))])
assert (NODE.itemsize, NODE32.itemsize, MOTION32.itemsize) == (112, 64, 96)


def narrow(x, up):
    """float64 -> float32 rounded toward +inf (up) or -inf: a round-to-nearest cast, then one step outward where it landed
    inside (host/f32_layout.hpp: narrow_down / narrow_up)."""
    x = np.asarray(x, dtype=np.float64)
    f = x.astype(np.float32)
    if up:
        return np.where(f.astype(np.float64) < x, np.nextafter(f, np.float32(np.inf)), f)
    return np.where(f.astype(np.float64) > x, np.nextafter(f, np.float32(-np.inf)), f)


def leaf_boxes(nodes, root):
    """{slot: (bmin, bmax)} of the one-slot leaves below `root`, and a list of (node, child index, child node) of the internal
    children."""
    leaves, internal, todo = {}, [], [int(root)]
    while todo:
        n = todo.pop()
        for c in range(2):
            code = int(nodes["child"][n][c])
            if code < 0:
                assert (code & 7) == 0
                leaves[(code & 0x7fffffff) >> 3] = (nodes["bmin"][n][c].copy(), nodes["bmax"][n][c].copy())
            else:
                internal.append((n, c, code))
                todo.append(code)
    return leaves, internal


def tree_roots(flat):
    """Root node of every instance tree, from the ENTRY_INSTANCE records that close the entry array."""
    e = flat.array("entries").view(np.int32).reshape(-1, 40)
    return [int(r[1]) for r in e if r[0] == 5 and r[1] >= 0]


# ---- scenes of the GPU tests ----
def prism_field(rtsr, n, line=False):
    """A ground sphere and ONE instance tree of n Translate(RotateY(RectPrism)) members.  n = 2: the tree is its root; 3: one
    internal child.  line: the members sit on a line with geometric spacing (1.5^k), which gives the builder a skewed tree."""
    b = rtsr.Builder(3)
    m = [b.lambertian((0.8, 0.3, 0.3)), b.metal((0.8, 0.8, 0.9), 0.3), b.lambertian((0.2, 0.7, 0.3))]
    cols = max(int(round(n ** 0.5)), 1)
    members = []
    for k in range(n):
        w = 0.2 + 0.01 * (k % 7)
        box = b.rect_prism((-w, 0.0, -w), (w, 0.3 + 0.05 * (k % 5), w), m[k % 3])
        x, z = (0.01 * 1.5 ** k, 0.1 * k) if line else (-0.5 * cols + 1.0 * (k % cols) + 0.013 * (k % 7), -0.5 * cols + 1.0 * (k // cols))
        members.append(b.translate((x, 0.0, z), b.rotate_y(7.0 + 5.3 * k, box)))
    return b, b.hittable_list([b.sphere((0.0, -500.0, 0.0), 500.0, m[2]), b.instance_bvh(b.hittable_list(members))])


def room(rtsr):
    """A Cornell-like room built by hand: five walls, a light, two Translate(RotateY(prism)) boxes and one
    ConstantMedium(Translate(RotateY(prism))) -- every chain a top-level slot OUTSIDE any tree (the scatter alone, and a slot
    that is both a medium and a chain)."""
    b = rtsr.Builder(9)
    red, white, green = b.lambertian((0.65, 0.05, 0.05)), b.lambertian((0.73, 0.73, 0.73)), b.lambertian((0.12, 0.45, 0.15))
    light = b.diffuse_light((7.0, 7.0, 7.0))
    box1 = b.translate((265.0, 0.0, 295.0), b.rotate_y(15.0, b.rect_prism((0.0, 0.0, 0.0), (165.0, 330.0, 165.0), white)))
    box2 = b.translate((130.0, 0.0, 65.0), b.rotate_y(-18.0, b.rect_prism((0.0, 0.0, 0.0), (165.0, 165.0, 165.0), white)))
    smoke = b.constant_medium((0.9, 0.9, 1.0), 0.01, b.translate((60.0, 200.0, 250.0), b.rotate_y(30.0, b.rect_prism((0.0, 0.0, 0.0), (120.0, 120.0, 120.0), white))))
    world = b.hittable_list([b.yz_rect(0.0, 555.0, 0.0, 555.0, 555.0, green), b.yz_rect(0.0, 555.0, 0.0, 555.0, 0.0, red),
                             b.xz_rect(113.0, 443.0, 127.0, 432.0, 554.0, light), b.xz_rect(0.0, 555.0, 0.0, 555.0, 0.0, white),
                             b.xz_rect(0.0, 555.0, 0.0, 555.0, 555.0, white), b.xy_rect(0.0, 555.0, 0.0, 555.0, 555.0, white), box1, box2, smoke])
    return b, world


def room_cam_cfg(rtsr, width=48, spp=8):
    cam = rtsr.Camera.new((278.0, 278.0, -800.0), (278.0, 278.0, 0.0), (0.0, 1.0, 0.0), 40.0, 1.5, 0.0, 10.0, 0.0, 1.0)
    cfg = rtsr.Config.new(1.5, width, spp, 12, 4, seed=21, background=(0.0, 0.0, 0.0))
    return cam, cfg, rtsr.image_height(cfg)


def two_trees(rtsr):
    """Two instance trees with a BvhNode of moving spheres between them: the scene has time-aware boxes, and the trees' nodes
    carry their static copy."""
    b = rtsr.Builder(4)
    grey, red = b.lambertian((0.5, 0.5, 0.5)), b.metal((0.8, 0.3, 0.3), 0.1)
    prism = lambda w, h, m: b.rect_prism((-w, 0.0, -w), (w, h, w), m)
    left = [b.translate((-4.0 + 0.9 * k, 0.0, -1.0 + 0.3 * (k % 3)), b.rotate_y(11.0 * k, prism(0.25, 0.4 + 0.1 * (k % 3), red))) for k in range(7)]
    right = [b.translate((0.5 + 0.8 * k, 0.0, 1.0 - 0.4 * (k % 2)), b.rotate_y(-9.0 * k, prism(0.2, 0.6, grey))) for k in range(5)] + [b.sphere((2.0, 0.4, 2.5), 0.4, red)]
    movers = b.bvh_from_list(b.hittable_list([b.moving_sphere((-2.0 + k, 1.5, 0.0), (-2.0 + k, 1.5 + 0.3 * k, 0.0), 0.0, 1.0, 0.3, grey) for k in range(5)]), 0.0, 1.0)
    world = b.hittable_list([b.sphere((0.0, -500.0, 0.0), 500.0, grey), b.instance_bvh(b.hittable_list(left)), movers, b.instance_bvh(b.hittable_list(right))])
    return b, world
