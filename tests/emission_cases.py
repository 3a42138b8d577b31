"""Case builders for the emission tests (vrt_write_emission): tables, scenes and the comparison.  TEST INFRASTRUCTURE ONLY.

tests/test_emission_cases.py counts on the reference alone (tests/emission_ref.py) that each case holds what it claims;
tests/test_gpu_emission_matrix.py renders the same cases on the GPU.  The tables are float32[256]; the scenes are
voxelraytracing_amd.scenes.Scene objects, each with a world of its own."""
import numpy as np

from voxelraytracing_amd import MODE_PATH, scenes

import step_limit_scenes as L
import test_gpu_lone_wave as lone_wave
from util import RADIANCE_TOL

SEED = 11
ID_HIT, ID_VOXEL_MASK = 1 << 16, 0x7FFF   # (VRT_ID_HIT, the voxel bits of an id word: include/vrt.h)
FLT_MAX = np.finfo(np.float32).max
HIGH_IDS = (0x7FFF, 300)                  # voxel ids above 255: they read material 255 and emission entry 255
LIMESTONE, WATER, LAVA, AIR = 4, 3, 2, 0


# ---- tables ----

def hit_counts(ids):
    """How many pixels' primary hit has each material (ids above 255 count as 255, the entry they read)."""
    hit = (ids & ID_HIT) != 0
    return np.bincount(np.minimum(ids[hit] & ID_VOXEL_MASK, 255).astype(np.int64), minlength=256)[:256]


def common(ids, n=2):
    """The n materials that the frame's id words show are hit most often, most common first."""
    counts = hit_counts(ids)
    top = np.argsort(counts)[::-1][:n]
    assert counts[top[n - 1]] > 0
    return [int(t) for t in top]


def two_common(ids):
    """Two materials that the frame's id words show are hit often, made emissive (and a third entry that no voxel of C4 uses:
    a table with only some entries in use)."""
    top = common(ids, 2)
    t = np.zeros(256, np.float32)
    t[top[0]] = 1.75
    t[top[1]] = 0.5
    t[255] = 3.0
    return t


def _table(gpu):
    """two_common of the context's own 1-spp frame."""
    gpu.render(MODE_PATH, spp=1, seed=SEED)
    _, ids, _ = gpu.read_output(rgb=False)
    return two_common(ids)


def _one(entry, value):
    t = np.zeros(256, np.float32)
    t[entry] = value
    return t


def mirror_emitter(ids):
    """(table, emitter): the most commonly hit material alone emissive — the material the mirror-emitter scenes give scatter 0."""
    emitter = common(ids, 1)[0]
    return _one(emitter, 2.25), emitter


def every_solid():
    """Every entry from 4 up (the solids; 0 to 3 are air, the pack's second air and the liquids): every hit emits."""
    t = np.zeros(256, np.float32)
    t[4:] = 1.25
    return t


def entry_255_only():
    return _one(255, 2.0)


def liquid_only():
    t = np.zeros(256, np.float32)
    t[LAVA], t[WATER] = 1.5, 0.75
    return t


def air_only():
    return _one(AIR, 4.0)


def minus_zero_only():
    """Every entry -0.0: vrt_write_emission accepts it, and it is zero (e != 0 is false)."""
    return np.full(256, -0.0, np.float32)


def denormal(ids):
    """(table, emitter): 1e-40 (a float32 denormal) on the most commonly hit material."""
    emitter = common(ids, 1)[0]
    t = _one(emitter, 1e-40)
    assert 0.0 < t[emitter] < np.finfo(np.float32).tiny
    return t, emitter


def huge(ids):
    """(table, emitter): FLT_MAX on the most commonly hit material.  One term, (mc * e) * thr with mc, thr <= 1, is finite; a
    sample that hits the material twice, or a pixel's samples together, overflow to +inf."""
    emitter = common(ids, 1)[0]
    return _one(emitter, FLT_MAX), emitter


# ---- scenes ----

BOUNCES = (0, 1, 2, 3, 4)


def c4(size, bounces=4):
    return scenes.c4(size, bounces=bounces)


def c4_all_mirrors(size, bounces=4):
    """C4 with scenes._diffuse not applied: scatter 0 on every material, as Material::construct leaves it."""
    sc = scenes.c4(size, bounces=bounces)
    for i in range(256):
        sc.materials[i].scatter = 0.0
    return sc


def c4_mirror_emitter(size, emitter, bounces=4):
    """Diffuse C4 whose `emitter` material is a mirror."""
    sc = scenes.c4(size, bounces=bounces)
    sc.materials[emitter].scatter = 0.0
    return sc


def c4_diffuse_emitter(size, emitter, bounces=4):
    """All-mirror C4 whose `emitter` material is diffuse."""
    sc = c4_all_mirrors(size, bounces)
    sc.materials[emitter].scatter = 1.0
    return sc


def c4_half_scatter(size, bounces=4):
    """C4 with scatter 0.5 everywhere: the next direction mixes the mirror's and the diffuse one."""
    sc = scenes.c4(size, bounces=bounces)
    for i in range(256):
        sc.materials[i].scatter = 0.5
    return sc


def material_scene(kind, size, emitter, bounces=4):
    if kind == "all mirrors":
        return c4_all_mirrors(size, bounces)
    if kind == "mirror emitter":
        return c4_mirror_emitter(size, emitter, bounces)
    if kind == "diffuse emitter":
        return c4_diffuse_emitter(size, emitter, bounces)
    assert kind == "half scatter"
    return c4_half_scatter(size, bounces)


MATERIAL_KINDS = ["all mirrors", "mirror emitter", "diffuse emitter", "half scatter"]


def c4_high_ids(size, bounces=4):
    """C4 with the surface voxel of every column of some 4 x 4 patches around the world's centre replaced by an id above
    255 (0x7FFF and 300 in turn): several hundred voxels in the terrain the camera looks down on.  Such a voxel has material
    255 and emission entry 255 (min(voxel, 255)); the standard pack's material 255 is black, which would make its light zero
    whatever the entry, so the scene gives it a colour."""
    sc = scenes.c4(size, bounces=bounces)
    m = sc.materials[255]
    m.color[0], m.color[1], m.color[2] = 0.9, 0.6, 0.3
    m.is_empty, m.is_liquid = 0, 0
    c = sc.world.size_in_chunks() * 16
    n = 0
    for x in range(c - 40, c + 40):
        for z in range(c - 40, c + 40):
            if ((x >> 2) + (z >> 2)) % 3:
                continue
            y = sc.world.highest_vox_at(x, z)
            if y is None:
                continue
            sc.world.set_voxel((x, y, z), HIGH_IDS[((x >> 2) ^ (z >> 2)) & 1])
            n += 1
    assert n >= 300, n
    return sc


def step_limit_table():
    return _one(LIMESTONE, 1.25)


def step_limit_table_with_water():
    """... and water: a ray that runs out of lookups on a water voxel reports a hit there (ray_tracer.wgsl:293), the one way a
    liquid's entry gives light."""
    t = step_limit_table()
    t[WATER] = 0.75
    return t


def step_limit_scenes(world, bounces):
    """tests/step_limit_scenes.py's path frames (mirror and diffuse, one tile to 256 x 144): with step_limit_table the
    limestone lattice their rays run out in is emissive."""
    return L.path_scenes(world, bounces)


LONE_SIZES = lone_wave.SIZES + [(20, 13)]   # one tile, eight tiles, and a ragged size: two whole tiles and a margin that is not traced
LONE_CAMERAS = lone_wave.CAMERAS[:3]


def lone_wave_worlds():
    c2 = scenes.c2((8, 8))
    h = float(c2.world.highest_vox_at(128, 128))
    return {"c2": (c2.world, (128.0, h + 2.0, 128.0))}


def lone_wave_scene(worlds, cam, size, bounces):
    """tests/test_gpu_lone_wave.py's path scene: a frame of a tile or a few, on a camera whose rays tie."""
    return lone_wave._scene(worlds, "c2", cam, size, MODE_PATH, bounces=bounces)


def c5_small(size=(96, 56), bounces=4):
    """Config C5's 32^3-chunk world at a small frame: too large for the direct layout, so its march cells go through the chunk
    directory without any switch."""
    return scenes.c5(size, bounces=bounces, chunks=32)


# ---- the comparison ----

def assert_emissive_parity(gpu_rgb, gpu_ids, ref_rgb, ref_ids, what=""):
    """Ids bit for bit; the masks of NaN, +inf and -inf identical; on pixels finite on both sides |gpu - ref| <=
    RADIANCE_TOL * max(1, |ref|) per channel.

    The scale: directions are bit-exact between device and reference and the emission term is three correctly rounded
    multiplies, so the only inexact term is the sky's, bounded by RADIANCE_TOL absolute at throughput <= 1; the additions and the
    division by spp add a few units of 2^-24 relative, three orders below 1e-4 relative."""
    bad = np.argwhere(gpu_ids != ref_ids)
    assert bad.size == 0, f"{what}: {len(bad)} id words differ, first at (y,x)={tuple(bad[0])}: " \
                          f"gpu={gpu_ids[tuple(bad[0])]:#x} reference={ref_ids[tuple(bad[0])]:#x}"
    for name, mask in (("NaN", np.isnan), ("+inf", np.isposinf), ("-inf", np.isneginf)):
        g, r = mask(gpu_rgb), mask(ref_rgb)
        assert np.array_equal(g, r), f"{what}: {name} in {int(g.sum())} gpu values and {int(r.sum())} reference values, " \
                                     f"{int((g != r).sum())} of them not in the same place"
    fin = np.isfinite(ref_rgb)
    g, r = gpu_rgb[fin].astype(np.float64), ref_rgb[fin].astype(np.float64)
    if g.size == 0:
        return
    excess = np.abs(g - r) / np.maximum(1.0, np.abs(r))
    assert float(excess.max()) <= RADIANCE_TOL, f"{what}: max scaled radiance error {excess.max()} (at reference value {r[excess.argmax()]})"


def assert_bit_identical(a, b, what=""):
    """(rgb, ids) pairs equal bit for bit (NaN payloads and the sign of zero included)."""
    assert np.array_equal(a[1], b[1]), f"{what}: id words differ"
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)), f"{what}: radiance differs in {(a[0].view(np.uint32) != b[0].view(np.uint32)).sum()} values"
