"""The dark voxel marks (vrt_lit.hip: accel_dark_voxels_kernel; vrt_device.h kDarkVoxel; docs/NUMERICS.md "Dark stops", the voxels
of split cells) on the GPU, 128 x 72 frames.

Marks: vrt_read_dark_voxels against the rule as tests/dark_voxel_ref.py states it over the world the device built (vrt_read_accel),
the lit voxel marks it made (vrt_read_lit_voxels) and the dark cell marks it made (vrt_get_dark_marks) — the kernel computes its
intervals in binary64 in the reference's order, so the two agree voxel for voxel: an equality, no bracket.  Frames: byte for byte
what a context without the marks renders (VRT_DARK_VOXEL_LAYERS=0), texels and ids; no tile takes more trips; the counting kernels'
counts are the same.  Edits and a change of the liquid set make the marks again.  Edges: a sun that makes the shadow waves careful,
a camera inside water, a world that holds the mark's id, a world that holds the lit mark's id.
"""
import numpy as np
import pytest

import dark_voxel_ref as V
import lit_corridor_ref as C
from test_gpu_dark_marks import CASES, PLATE, SIZE, SUNS, VIEWS, _edit, _liquid
from test_gpu_lit_voxels import _dense
from test_gpu_sun_marks import GX, GZ, LIMESTONE, SETTLE, WATER
from util import gpu_for_scene
from voxelraytracing_amd import MODE_PRIMARY_SHADOW, scenes
from voxelraytracing_amd.world import ClientWorld, gen_height, svo_build_by_set_node

pytestmark = pytest.mark.gpu

K_D = 16   # the default up to 64^3 cells (vrt_lit.hip: dark_voxel_layers)
TILES = (SIZE[0] // 8) * (SIZE[1] // 8)


def _gpu(monkeypatch, sc, layers=None, cells=True):
    for name in ("VRT_SUN_MARKS", "VRT_LIT_VOXELS", "VRT_LIT_VOXEL_LAYERS", "VRT_DARK_MARKS", "VRT_DARK_DEPTH", "VRT_DARK_VOXEL_LAYERS"):
        monkeypatch.delenv(name, raising=False)
    if layers is not None:
        monkeypatch.setenv("VRT_DARK_VOXEL_LAYERS", str(layers))
    if not cells:
        monkeypatch.setenv("VRT_DARK_MARKS", "0")
    return gpu_for_scene(sc)


def _reference(gpu, sun, liquid, layers):
    """The rule over what the device holds: its world, its lit voxel marks, its dark cell marks."""
    dense, split = _dense(*gpu.read_accel())
    lit = gpu.lit_voxels(voxels=True)["lit"]
    cells = gpu.dark_marks(cells=True)["dark"]
    return V.dark_voxels(dense, split, lit, cells, sun, layers, liquid).astype(bool)


def _counts(gpu):
    gpu.render(MODE_PRIMARY_SHADOW, stats=True)
    s = gpu.stats()
    return (s.primary_rays, s.secondary_rays, s.hits, s.steps, s.node_visits, s.primary_steps, s.primary_node_visits), gpu.read_steps().copy()


def _run(monkeypatch, sc, other, layers, reference=True, cells=True):
    """The view of `sc` with the marks made while another view is drawn (one frame in flight: the second frame of a view at rest
    notes its tiles' trips): the frame's bytes, the trips per tile, the marks, the counting kernel's counts."""
    gpu = _gpu(monkeypatch, sc, layers, cells)
    try:
        gpu.set_frames_in_flight(1)
        gpu.write_cam_data(other.cam)
        for _ in range(SETTLE):
            gpu.render(MODE_PRIMARY_SHADOW, timed=True)
        gpu.write_cam_data(sc.cam)
        for _ in range(3):
            gpu.render(MODE_PRIMARY_SHADOW, timed=True)
        rgb, ids, _ = gpu.read_output()
        out = dict(rgb=rgb.view(np.uint32).copy(), ids=ids.copy(), cost=gpu.read_tile_cost(TILES).astype(np.int64),
                   marks=gpu.dark_voxels(voxels=True), lit=gpu.lit_voxels(voxels=True), cells=gpu.dark_marks(cells=True))
        if reference and out["marks"]["layers"]:
            out["ref"] = _reference(gpu, tuple(sc.settings.sun_pos), _liquid(sc), out["marks"]["layers"])
        out["counts"], out["steps"] = _counts(gpu)
        return out
    finally:
        gpu.close()


def _same_frames(on, off, what):
    assert np.array_equal(on["rgb"], off["rgb"]) and np.array_equal(on["ids"], off["ids"]), f"{what}: the frame differs from VRT_DARK_VOXEL_LAYERS=0"
    assert off["marks"]["layers"] == 0 and off["marks"]["passes"] == 0 and not off["marks"]["dark"].any(), what
    # what the marks are made from is what it is without them
    assert np.array_equal(on["lit"]["lit"], off["lit"]["lit"]) and on["lit"]["layers"] == off["lit"]["layers"], what
    assert np.array_equal(on["cells"]["dark"], off["cells"]["dark"]), what
    assert (on["cost"] <= off["cost"]).all(), f"{what}: {int((on['cost'] > off['cost']).sum())} tiles take more trips with the marks"
    assert on["counts"] == off["counts"] and np.array_equal(on["steps"], off["steps"]), f"{what}: the counting kernel's counts differ"


_cases = {}   # (chunks, k): the two runs of a case, made once (the last test reads the trips of all of them)


def _case(monkeypatch, chunks, k):
    if (chunks, k) not in _cases:
        name, sun, _ = SUNS[k]
        sc = scenes.procedural(chunks, SIZE)
        if (chunks, name) in VIEWS:
            sc = scenes._scene(sc.name, sc.world, SIZE, *VIEWS[(chunks, name)], MODE_PRIMARY_SHADOW)
        other = scenes._scene("another view", sc.world, sc.size, sc.eye, (35.0, 120.0, 0.0), MODE_PRIMARY_SHADOW)
        sc.settings.sun_pos[:] = sun
        _cases[(chunks, k)] = (_run(monkeypatch, sc, other, None), _run(monkeypatch, sc, other, 0))
    return _cases[(chunks, k)]


@pytest.mark.parametrize("chunks,k", CASES)
def test_marks_frames_and_trips(monkeypatch, chunks, k):
    name, sun, _ = SUNS[k]
    on, off = _case(monkeypatch, chunks, k)
    plan = C.plan(chunks * 32, sun)
    dark = on["marks"]["dark"].astype(bool)
    ref = on.get("ref", np.zeros_like(dark))
    print(f"{chunks}^3 sun {name}: the rule's dark voxels {int(ref.sum())}, the kernel's {int(dark.sum())} ({int((ref != dark).sum())} differ); "
          f"trips {int(off['cost'].sum())} without, {int(on['cost'].sum())} with the marks; {on['marks']['passes']} passes, {on['marks']['layers']} layers")
    assert on["marks"]["layers"] == (K_D if plan else 0) and on["marks"]["passes"] == (1 if plan else 0)
    if plan:
        assert ref.any(), (name, "the rule marks no voxel: the case shows nothing")
    # the marks are the rule's, voxel for voxel
    assert np.array_equal(dark, ref), f"{name}: {int((ref != dark).sum())} voxels differ from the rule"
    _same_frames(on, off, f"{chunks}^3 sun {name}")


@pytest.mark.parametrize("layers", [1, 8, 32])
def test_other_depths(monkeypatch, layers):
    """VRT_DARK_VOXEL_LAYERS: the marks are the reference's at that depth, and grow with it."""
    name, sun, _ = SUNS[0]
    sc = scenes.procedural(3, SIZE)
    other = scenes._scene("another view", sc.world, sc.size, sc.eye, (35.0, 120.0, 0.0), MODE_PRIMARY_SHADOW)
    sc.settings.sun_pos[:] = sun
    on, off = _run(monkeypatch, sc, other, layers), _run(monkeypatch, sc, other, 0)
    dark, ref = on["marks"]["dark"].astype(bool), on["ref"]
    print(f"3^3 sun {name}, {layers} layers: the rule's dark voxels {int(ref.sum())}, the kernel's {int(dark.sum())} ({int((ref != dark).sum())} differ)")
    assert on["marks"]["layers"] == layers and ref.any()
    assert np.array_equal(dark, ref)
    _same_frames(on, off, f"{layers} layers")


def test_without_the_dark_cell_marks(monkeypatch):
    """VRT_DARK_MARKS=0: no cell carries the dark cell mark, and the voxel marks are the rule's with solid voxels alone — fewer than
    with the cells' marks, and some."""
    name, sun, _ = SUNS[0]
    sc = scenes.procedural(4, SIZE)
    other = scenes._scene("another view", sc.world, sc.size, sc.eye, (35.0, 120.0, 0.0), MODE_PRIMARY_SHADOW)
    sc.settings.sun_pos[:] = sun
    on, off = _run(monkeypatch, sc, other, None, cells=False), _run(monkeypatch, sc, other, 0, cells=False)
    dark, ref = on["marks"]["dark"].astype(bool), on["ref"]
    print(f"4^3 sun {name}, VRT_DARK_MARKS=0: the rule's dark voxels {int(ref.sum())}, the kernel's {int(dark.sum())} ({int((ref != dark).sum())} differ)")
    assert on["marks"]["layers"] == K_D and not on["cells"]["dark"].any() and on["cells"]["passes"] == 0
    assert np.array_equal(dark, ref) and ref.any()
    with_cells = _case(monkeypatch, 4, 0)[0]["marks"]["dark"].astype(bool)
    assert not (dark & ~with_cells).any() and dark.sum() < with_cells.sum()
    _same_frames(on, off, "VRT_DARK_MARKS=0")


def _snapshot(gpu):
    for _ in range(SETTLE):
        gpu.render(MODE_PRIMARY_SHADOW, timed=True)
    rgb, ids, _ = gpu.read_output()
    return rgb.view(np.uint32).copy(), ids.copy(), gpu.dark_voxels(voxels=True)


def _edited(monkeypatch, layers, in_flight):
    world = scenes.procedural(4, SIZE).world
    ground = gen_height(1, GX, GZ)
    sc = scenes._scene("looking down", world, SIZE, (GX + 0.5, ground + 24.5, GZ + 0.5), (89.0, 0.0, 0.0), MODE_PRIMARY_SHADOW)
    gpu = _gpu(monkeypatch, sc, layers)
    sun = tuple(sc.settings.sun_pos)
    try:
        gpu.set_frames_in_flight(in_flight)
        shots = {"bare": _snapshot(gpu)}
        if layers is None:
            shots["bare ref"] = _reference(gpu, sun, _liquid(sc), K_D)
        _edit(gpu, sc.world, PLATE, LIMESTONE)
        shots["plate"] = _snapshot(gpu)
        if layers is None:
            shots["plate ref"] = _reference(gpu, sun, _liquid(sc), K_D)
        mats = type(sc.materials).from_buffer_copy(sc.materials)
        mats[LIMESTONE].is_liquid = 1
        gpu.write_materials(mats)
        shots["liquid"] = _snapshot(gpu)
        if layers is None:
            liquid = _liquid(sc)
            liquid[LIMESTONE] = True
            shots["liquid ref"] = _reference(gpu, sun, liquid, K_D)
        return shots
    finally:
        _edit(gpu, sc.world, PLATE, 0)   # (the world object is shared by every scene of this process: whatever happened, the plate goes)
        gpu.close()


@pytest.mark.parametrize("in_flight", [1, 2])
def test_an_edit_and_a_liquid_edit_make_the_marks_again(monkeypatch, in_flight):
    """A plate of limestone in the open air, then limestone declared a liquid: after each the marks settle again, and are the rule's
    over the new world and the new liquid set."""
    on, off = _edited(monkeypatch, None, in_flight), _edited(monkeypatch, 0, in_flight)
    for what in ("bare", "plate", "liquid"):
        assert np.array_equal(on[what][0], off[what][0]) and np.array_equal(on[what][1], off[what][1]), f"{what}: the frame differs from VRT_DARK_VOXEL_LAYERS=0"
        assert not off[what][2]["dark"].any() and off[what][2]["layers"] == 0
        dark, ref = on[what][2]["dark"].astype(bool), on[what + " ref"]
        print(what, "dark voxels", int(dark.sum()), "the rule's", int(ref.sum()), "passes", on[what][2]["passes"])
        assert on[what][2]["layers"] == K_D
        assert np.array_equal(dark, ref), f"{what}: {int((ref != dark).sum())} voxels differ from the rule"
    assert not np.array_equal(on["plate"][0], on["bare"][0]), "the plate casts no shadow into the view: the case shows nothing"
    assert on["plate"][2]["dark"].sum() > on["bare"][2]["dark"].sum(), "the plate darkens no voxel"
    assert on["liquid"][2]["dark"].sum() < on["plate"][2]["dark"].sum(), "a liquid plate still darkens voxels"
    assert on["bare"][2]["passes"] < on["plate"][2]["passes"] < on["liquid"][2]["passes"]


def _on_and_off(monkeypatch, sc, what, in_flights=(1, 2)):
    got = {}
    for layers in (None, 0):
        gpu = _gpu(monkeypatch, sc, layers)
        try:
            frames = []
            for n in in_flights:
                gpu.set_frames_in_flight(n)
                frames.append(_snapshot(gpu)[:2])
            got[layers] = (frames, gpu.dark_voxels(voxels=True), gpu.lit_voxels(voxels=True), _counts(gpu))
        finally:
            gpu.close()
    for n, a, b in zip(in_flights, got[None][0], got[0][0]):
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), f"{what}, {n} in flight: the frame differs from VRT_DARK_VOXEL_LAYERS=0"
    assert got[None][3][0] == got[0][3][0] and np.array_equal(got[None][3][1], got[0][3][1]), what
    assert not got[0][1]["dark"].any()
    return got[None][1], got[None][2]


@pytest.mark.parametrize("sun", [(float("inf"), 20000.0, 5000.0), (float("nan"), 20000.0, 5000.0), (100.0, 3.0e38, 100.0)])
def test_suns_that_make_the_shadow_waves_careful(monkeypatch, sun):
    """A sun that is not finite gets no marks at all; one so far away that the shadow ray's direction overflows gets them, and its
    waves — careful ones — read the plain bricks, to which a dark voxel is the air it is."""
    sc = scenes.procedural(4, SIZE)
    sc.settings.sun_pos[:] = sun
    try:
        marks, _ = _on_and_off(monkeypatch, sc, f"sun {sun}")
    finally:
        sc.settings.sun_pos[:] = scenes.SUN_POS
    assert (marks["layers"] == K_D) == (C.plan(128, sun) is not None)


def _water_world():
    """tests/test_gpu_lit_voxels.py's: limestone under four voxels of water, a pillar, pebbles over the water — and a slab of limestone
    over a part of it, so that air voxels between the pebbles and the slab are dark."""
    x, y, z = np.meshgrid(np.arange(32), np.arange(32), np.arange(32), indexing="ij")
    dense = np.zeros(32768, dtype=np.uint16)
    at = x + 32 * (y + 32 * z)
    dense[at[y < 8]] = LIMESTONE
    dense[at[(y >= 8) & (y < 12)]] = WATER
    dense[at[(y >= 8) & (y < 20) & (x >= 12) & (x < 15) & (z >= 12) & (z < 15)]] = LIMESTONE
    dense[at[(y == 13) & (x % 5 == 0) & (z % 3 == 0)]] = LIMESTONE
    dense[at[(y == 17) & (x >= 2) & (x < 30) & (z >= 2) & (z < 30)]] = LIMESTONE
    nodes = svo_build_by_set_node(dense)
    world = ClientWorld((1, 1, 1), 1 << 20, 2)
    for cx in range(2):
        for cz in range(2):
            world.create_chunk((cx, 0, cz), nodes)
    return world


def test_a_camera_inside_water(monkeypatch):
    """The eye under water, looking down along the floor: the shadow rays start in water and climb out into dark voxels under the slab
    — lanes in water take the general step, where a dark voxel is the solid voxel the pool says: a hit, which it is."""
    sc = scenes._scene("under water", _water_world(), SIZE, (20.5, 10.5, 20.5), (25.0, 35.0, 0.0), MODE_PRIMARY_SHADOW)
    marks, _ = _on_and_off(monkeypatch, sc, "a camera inside water")
    assert marks["layers"] == K_D and marks["dark"].any(), "no voxel is dark: the case shows nothing"


def _looking_down(voxel):
    world = scenes.procedural(4, SIZE).world
    ground = gen_height(1, GX, GZ)
    at = [(GX + 2 + i, ground + 4, GZ + 1 + j) for i in range(6) for j in range(6)]   # a small roof over the ground under the eye
    sc = scenes._scene("looking down", world, SIZE, (GX + 0.5, ground + 24.5, GZ + 0.5), (89.0, 0.0, 0.0), MODE_PRIMARY_SHADOW)
    for p in at:
        world.set_voxel(p, voxel)
    return sc, world, at


def test_a_world_whose_bricks_hold_the_dark_id(monkeypatch):
    """0x7FFE in the world is a solid voxel of material 255, which is what the mark says: nothing to do.  The read-back reports
    marks on air voxels alone, so those nine are none; the marks under them are the rule's."""
    sc, world, at = _looking_down(V.DARK_VOXEL)
    try:
        marks, _ = _on_and_off(monkeypatch, sc, "0x7FFE in the world")
        assert marks["layers"] == K_D and marks["dark"].any()
        for x, y, z in at:
            assert world.get_voxel((x, y, z)) == V.DARK_VOXEL and not marks["dark"][z, y, x]
        assert any(marks["dark"][z, y - 1, x] for x, y, z in at), "no air voxel right under the roof is dark"
    finally:
        for p in at:
            world.set_voxel(p, 0)


def test_a_world_whose_bricks_hold_the_lit_id(monkeypatch):
    """0x7FFF in the world is the clash of the lit voxel marks: the pool is made a plain copy, in which those voxels hold 0x7FFE — and
    the dark voxel pass behind it writes nothing into it.  No dark voxel is left in the pool, no lit one, and the frames are the same."""
    sc, world, at = _looking_down(0x7FFF)
    try:
        marks, lit = _on_and_off(monkeypatch, sc, "0x7FFF in the world")
        assert not marks["dark"].any() and not lit["lit"].any()
        assert marks["layers"] == 0 and lit["layers"] == 0, ("the frames still read the shadow pool", marks, lit)
    finally:
        for p in at:
            world.set_voxel(p, 0)


def test_some_case_takes_fewer_trips(monkeypatch):
    """No tile takes more trips in any case (test_marks_frames_and_trips asserts it), and at least one case takes fewer."""
    saved = []
    for chunks, k in CASES:
        on, off = _case(monkeypatch, chunks, k)
        saved.append(int(off["cost"].sum() - on["cost"].sum()))
    print("trips saved per case:", saved)
    assert min(saved) >= 0 and max(saved) > 0
