"""The voxel marks (vrt_lit.hip: accel_lit_voxels_kernel; vrt_march.h (u); docs/NUMERICS.md "Lit stops") on the GPU.

Marks: the shadow pool as vrt_read_lit_voxels reads it back, against the rule as tests/lit_voxel_ref.py states it over the world
the device built (vrt_read_accel) and the cell marks the device made (vrt_get_sun_marks).  The kernel computes in binary32 and
adds 0.01 to every allowance for that (its errors stay below 2e-3: coordinates and products below 4096); the lit set shrinks as
the allowance grows, so the kernel's marks lie, voxel for voxel, between the float64 rule with 0.02 and the one with none of that
0.01 — and inside the rule without any margin.  Frames: byte for byte the frames of VRT_SUN_MARKS=0 and of VRT_LIT_VOXELS=0,
texels and presented window, one and two in flight.  Trips, the life cycle, and the edges: the reserved id in the world, a liquid
table that covers it, rays that start in water, a lone wave, and layer counts that use the step budget up.
"""
import numpy as np
import pytest

import lit_voxel_ref as R
from test_gpu_sun_marks import GX, GZ, LIMESTONE, SETTLE, WATER, render_and_check, suns
from util import gpu_for_scene
from voxelraytracing_amd import MODE_PRIMARY_SHADOW, scenes
from voxelraytracing_amd.world import ClientWorld, gen_height, svo_build_by_set_node

pytestmark = pytest.mark.gpu

AIR_LEAF = 0xFF800000
K = 8   # the default up to 64^3 cells (vrt_lit.hip: lit_voxel_layers)
_scenes = {}


def _scene(chunks, size):
    if (chunks, size) not in _scenes:
        sc = scenes.procedural(chunks, size)
        if chunks == 2:   # (an eye inside the world: just under its top face, in the water)
            sc = scenes._scene(sc.name, sc.world, size, (32.5, 62.5, 32.5), sc.rot, MODE_PRIMARY_SHADOW)
        _scenes[(chunks, size)] = sc
    sc = _scenes[(chunks, size)]
    sc.settings.sun_pos[:] = scenes.SUN_POS
    return sc


def _suns(w):
    by_name = {name: sun for name, sun, _ in suns(w)}
    return [("the bench's", tuple(scenes.SUN_POS)), ("-x", by_name["-x"]), ("+z", by_name["+z"]), ("below the horizon", by_name["below the horizon"])]


def _gpu(monkeypatch, sc, **env):
    for name in ("VRT_SUN_MARKS", "VRT_LIT_VOXELS", "VRT_LIT_VOXEL_LAYERS"):
        if name in env:
            monkeypatch.setenv(name, env[name])
        else:
            monkeypatch.delenv(name, raising=False)
    return gpu_for_scene(sc)


def _dense(grid, bricks):
    """u16 [n, n, n] = [z, y, x] voxel ids from the device's tables, and which cells are split."""
    G = grid.shape[0]
    split = (grid >= 0x80000000) & (grid < AIR_LEAF)
    leaf_voxel = np.where((grid < 0x80000000), (grid >> 16) & 0x7FFF, 0).astype(np.uint16)
    cells = np.repeat(leaf_voxel.reshape(G, G, G, 1), 64, axis=3)
    if split.any():
        cells[split] = bricks[(grid[split] & 0x7FFFFFC0) >> 6] >> 1
    dense = cells.reshape(G, G, G, 4, 4, 4).transpose(0, 3, 1, 4, 2, 5).reshape(4 * G, 4 * G, 4 * G)
    return np.ascontiguousarray(dense), split


@pytest.mark.parametrize("chunks", [2, 3, 4])
def test_marks_equal_the_reference(monkeypatch, chunks):
    sc = _scene(chunks, (64, 40))
    gpu = _gpu(monkeypatch, sc)
    try:
        gpu.set_frames_in_flight(1)
        dense = None
        for name, sun in _suns(chunks * 32):
            sc.settings.sun_pos[:] = sun
            gpu.write_settings(sc.settings)
            for _ in range(SETTLE):
                gpu.render(MODE_PRIMARY_SHADOW, timed=True)
            if dense is None:
                dense, split = _dense(*gpu.read_accel())
            cell_lit = gpu.sun_marks(cells=True)["lit"].astype(bool)
            m = gpu.lit_voxels(voxels=True)
            assert m["layers"] == K, (name, m["layers"])
            lit = m["lit"].astype(bool)
            ref = R.lit_voxels(dense, split, cell_lit, sun, K).astype(bool)
            narrow = R.lit_voxels(dense, split, cell_lit, sun, K, extra=0.01).astype(bool)
            wide = R.lit_voxels(dense, split, cell_lit, sun, K, extra=-0.01).astype(bool)
            free = R.lit_voxels(dense, split, cell_lit, sun, K, margins=False).astype(bool)
            print(f"{chunks}^3 sun {name}: lit voxels {int(lit.sum())}, the rule {int(ref.sum())} ({int((ref != lit).sum())} differ), "
                  f"bracket {int(narrow.sum())} .. {int(wide.sum())}, without margins {int(free.sum())}")
            # the kernel on this hardware is deterministic, and on these worlds and suns no interval's end falls within its rounding of a
            # voxel's face (the bracket's two ends are the same set): the marks are the rule's, voxel for voxel
            assert np.array_equal(lit, ref), f"{name}: {int((ref != lit).sum())} voxels differ from the rule"
            assert not (narrow & ~lit).any(), f"{name}: {int((narrow & ~lit).sum())} voxels the rule lights with twice the kernel's slack are not lit"
            assert not (lit & ~wide).any(), f"{name}: {int((lit & ~wide).sum())} lit voxels the rule does not light without the kernel's slack"
            assert not (lit & ~free).any() and not lit[dense != 0].any(), name
            if chunks > 2 and name != "below the horizon":
                assert lit.any(), (name, "no voxel is lit: the case shows nothing")
            elif chunks == 2:
                assert not lit.any()
    finally:
        gpu.close()


def _frames(gpu, in_flight):
    gpu.set_frames_in_flight(in_flight)
    for _ in range(SETTLE):
        gpu.render(MODE_PRIMARY_SHADOW, timed=True)
    rgb, ids, _ = gpu.read_output()
    return rgb.tobytes(), ids.tobytes(), gpu.present().tobytes()


@pytest.mark.parametrize("size", [(64, 40), (128, 72)])
@pytest.mark.parametrize("chunks", [2, 3, 4, 8])
def test_frames_unchanged(monkeypatch, chunks, size):
    sc = _scene(chunks, size)
    got = {}
    for what, env in (("voxel marks", {}), ("VRT_SUN_MARKS=0", {"VRT_SUN_MARKS": "0"}), ("VRT_LIT_VOXELS=0", {"VRT_LIT_VOXELS": "0"})):
        gpu = _gpu(monkeypatch, sc, **env)
        try:
            got[what] = [_frames(gpu, n) for n in (1, 2)]
            m = gpu.lit_voxels()
            assert (m["layers"] == K) == (what == "voxel marks"), (what, m)
        finally:
            gpu.close()
    for what in ("VRT_SUN_MARKS=0", "VRT_LIT_VOXELS=0"):
        for n in (0, 1):
            for part, a, b in zip(("radiance", "ids", "window"), got["voxel marks"][n], got[what][n]):
                assert a == b, f"{chunks}^3 {size}, {n + 1} in flight: {part} differs from {what}"


def test_no_tile_takes_more_trips_and_the_frame_takes_fewer(orc, monkeypatch):
    """vrt_read_tile_cost at 128 x 72 on the 8^3 world, as tests/test_gpu_sun_marks.py reads it: the marks are made while another
    view is drawn, then the second plain frame of the view at rest notes its tiles' trips."""
    sc = _scene(8, (128, 72))
    other = scenes._scene("another view", sc.world, sc.size, sc.eye, (35.0, 120.0, 0.0), MODE_PRIMARY_SHADOW)
    w, h = sc.size
    tiles = (h // 8) * (w // 8)
    cost = {}
    for voxels in ("0", "1"):
        gpu = _gpu(monkeypatch, sc, VRT_LIT_VOXELS=voxels)
        try:
            gpu.set_frames_in_flight(1)
            gpu.write_cam_data(other.cam)
            for _ in range(SETTLE):
                gpu.render(MODE_PRIMARY_SHADOW, timed=True)
            gpu.write_cam_data(sc.cam)
            for _ in range(3):
                gpu.render(MODE_PRIMARY_SHADOW, timed=True)
            assert gpu.sun_marks()["passes"] == 1 and gpu.lit_voxels()["passes"] == int(voxels)
            cost[voxels] = gpu.read_tile_cost(tiles).astype(np.int64)
        finally:
            gpu.close()
    print("trips per frame: cell marks alone", int(cost["0"].sum()), "with voxel marks", int(cost["1"].sum()))
    assert (cost["1"] <= cost["0"]).all()
    assert cost["1"].sum() < cost["0"].sum()


def test_life_cycle(orc, monkeypatch):
    world = scenes.procedural(4, (64, 40)).world
    ground = gen_height(1, GX, GZ)
    sc = scenes._scene("looking down", world, (64, 40), (GX + 0.5, ground + 24.5, GZ + 0.5), (89.0, 0.0, 0.0), MODE_PRIMARY_SHADOW)
    gpu = _gpu(monkeypatch, sc)

    def state():
        return gpu.lit_voxels()["passes"], gpu.lit_voxels()["layers"], gpu.sun_marks()["passes"]

    try:
        gpu.set_frames_in_flight(1)
        for _ in range(3):   # the first three still frames: no marks of either kind
            gpu.render(MODE_PRIMARY_SHADOW, timed=True)
            assert state() == (0, 0, 0)
        gpu.render(MODE_PRIMARY_SHADOW, timed=True)
        assert state() == (1, K, 1)
        m = gpu.lit_voxels()
        assert m["lit_trips"] == gpu.sun_marks()["lit_trips"] - R.budget(K) > 0, m
        render_and_check(orc, gpu, sc, "still")
        assert state() == (1, K, 1)
        # an edit: the chunk update drops the marks, four still frames bring them back
        start, n = world.set_voxel((GX + 3, ground + 6, GZ + 2), LIMESTONE)
        gpu.write_nodes(world.nodes_ptr(), start, start + n)
        for _ in range(3):
            gpu.render(MODE_PRIMARY_SHADOW, timed=True)
            assert state() == (1, 0, 1)
        gpu.render(MODE_PRIMARY_SHADOW, timed=True)
        assert state() == (2, K, 2)
        render_and_check(orc, gpu, sc, "after the edit")
        assert state() == (2, K, 2)
        # the sun moves: one pass of each kind
        sc.settings.sun_pos[:] = (9000.0, 20000.0, -6000.0)
        gpu.write_settings(sc.settings)
        render_and_check(orc, gpu, sc, "sun moved")
        assert state() == (3, K, 3)
    finally:
        gpu.close()


def test_the_reserved_id_in_the_world_builds_no_marks(orc, monkeypatch):
    """A voxel of id 0x7FFF (material 255) on the ground under the eye.  The pass meets it and leaves a pool without a mark, in which
    that voxel holds the id below — the read-back scans the pool itself, so a mark or the id left in it would show — the frames are the
    oracle's, and once the pass's flag has come back the frames read the plain bricks; a moved sun makes cell marks, and no voxel pass."""
    world = scenes.procedural(4, (64, 40)).world
    ground = gen_height(1, GX, GZ)
    at = (GX + 2, ground + 1, GZ + 1)
    sc = scenes._scene("looking down", world, (64, 40), (GX + 0.5, ground + 24.5, GZ + 0.5), (89.0, 0.0, 0.0), MODE_PRIMARY_SHADOW)
    world.set_voxel(at, R.LIT_VOXEL)
    gpu = _gpu(monkeypatch, sc)
    try:
        for in_flight in (1, 2):
            gpu.set_frames_in_flight(in_flight)
            r_ids, _ = render_and_check(orc, gpu, sc, f"reserved id, {in_flight} in flight")
        assert world.get_voxel(at) == R.LIT_VOXEL
        m = gpu.lit_voxels(voxels=True)
        assert gpu.sun_marks()["passes"] == 1 and m["passes"] == 1, (gpu.sun_marks(), m)
        assert not m["lit"].any(), "the pool of a world that holds the reserved id holds a mark, or the id"
        assert m["layers"] == 0 and m["lit_trips"] == 0, ("the frames still read the shadow pool", m)
        sc.settings.sun_pos[:] = (9000.0, 20000.0, -6000.0)
        gpu.write_settings(sc.settings)
        render_and_check(orc, gpu, sc, "reserved id, sun moved")
        m = gpu.lit_voxels()
        assert gpu.sun_marks()["passes"] == 2 and m["passes"] == 1 and m["layers"] == 0, (gpu.sun_marks(), m)
    finally:
        gpu.close()


def test_a_liquid_table_that_covers_the_reserved_id_builds_no_marks(orc, monkeypatch):
    sc = scenes.procedural(4, (64, 40))
    sc.materials[255].is_liquid = 1
    gpu = _gpu(monkeypatch, sc)
    try:
        for in_flight in (1, 2):
            gpu.set_frames_in_flight(in_flight)
            render_and_check(orc, gpu, sc, f"material 255 a liquid, {in_flight} in flight")
        m = gpu.lit_voxels(voxels=True)
        assert gpu.sun_marks()["passes"] >= 1 and m["passes"] == 0 and m["layers"] == 0 and not m["lit"].any()
    finally:
        gpu.close()


def test_rays_that_start_in_water(orc, monkeypatch):
    """Limestone under four voxels of water, a pillar that casts a shadow (tests/test_gpu_sun_marks.py): the shadow rays start in
    water — lanes that take the general step, to which a marked voxel is air — and climb out past marked voxels."""
    x, y, z = np.meshgrid(np.arange(32), np.arange(32), np.arange(32), indexing="ij")
    dense = np.zeros(32768, dtype=np.uint16)
    at = x + 32 * (y + 32 * z)
    dense[at[y < 8]] = LIMESTONE
    dense[at[(y >= 8) & (y < 12)]] = WATER
    dense[at[(y >= 8) & (y < 20) & (x >= 12) & (x < 15) & (z >= 12) & (z < 15)]] = LIMESTONE
    dense[at[(y == 13) & (x % 5 == 0) & (z % 3 == 0)]] = LIMESTONE   # pebbles over the water: split cells with lit air voxels
    nodes = svo_build_by_set_node(dense)
    world = ClientWorld((1, 1, 1), 1 << 20, 2)
    for cx in range(2):
        for cz in range(2):
            world.create_chunk((cx, 0, cz), nodes)
    sc = scenes._scene("water", world, (64, 40), (30.5, 30.5, 30.5), (40.0, 35.0, 0.0), MODE_PRIMARY_SHADOW)
    gpu = _gpu(monkeypatch, sc)
    try:
        for in_flight in (1, 2):
            gpu.set_frames_in_flight(in_flight)
            r_ids, _ = render_and_check(orc, gpu, sc, f"water, {in_flight} in flight", stats=True)
        assert ((r_ids & orc.ID_WATER) != 0).any() and ((r_ids & orc.ID_SHADOWED) != 0).any()
        m = gpu.lit_voxels(voxels=True)
        assert m["layers"] == K and m["lit"].any()
    finally:
        gpu.close()


def test_a_lone_wave(orc, monkeypatch):
    sc = scenes.procedural(4, (8, 8))
    gpu = _gpu(monkeypatch, sc)
    try:
        for in_flight in (1, 2):
            gpu.set_frames_in_flight(in_flight)
            render_and_check(orc, gpu, sc, f"8 x 8, {in_flight} in flight", stats=True)
        assert gpu.lit_voxels()["layers"] == K
    finally:
        gpu.close()


@pytest.mark.parametrize("layers", [47, 64])
def test_layer_counts_that_use_the_step_budget_up(orc, monkeypatch, layers):
    """4^3 chunks: the cell marks stop a ray below 299 trips.  48 layers take 300 of them and more: no voxel marks, the cell marks keep
    their trips.  47 leave the voxel marks 5 trips, after which the march reads the plain bricks again and the cell marks go on."""
    sc = _scene(4, (128, 72))
    gpu = _gpu(monkeypatch, sc, VRT_LIT_VOXEL_LAYERS=str(layers))
    try:
        for in_flight in (1, 2):
            gpu.set_frames_in_flight(in_flight)
            render_and_check(orc, gpu, sc, f"{layers} layers, {in_flight} in flight")
        cells, m = gpu.sun_marks(), gpu.lit_voxels()
        assert cells["lit_trips"] == 500 - (6 * (128 // 4 + 1) + 2) - 1
        if R.budget(layers) < cells["lit_trips"]:
            assert m["layers"] == layers and m["lit_trips"] == cells["lit_trips"] - R.budget(layers) == 5, m
        else:
            assert m["layers"] == 0 and m["passes"] == 0, m
    finally:
        gpu.close()
