"""Shadow rays that stop at cells with a clear path to the sun (docs/NUMERICS.md "Lit stops"), against the oracle.

The one-launch primary + shadow kernel stops a shadow ray at a LIT air leaf of the cell grid — the lit pass of vrt_lit.hip has
proven that every ray from that cell towards the sun leaves the world through air — and the frame must stay what the oracle
renders: ids bit for bit (VRT_ID_SHADOWED among them), radiance within the suite's 1e-4.  Every frame here is traced by the TIMED
kernel (the counting kernels never stop early: their step counts are the oracle's, which is checked too).  Suns on every side of
the world, below the horizon, too low beside it and inside it (no marks: the frame is still equal), a sun that moves, voxels that
come and go on lit paths, a chunk dropped to one air leaf, rays that run out of their 500 lookups in open air, and water.

The generator's sea level is 70: its 2^3-chunk world (64 voxels high) lies under water but for a few hill tops — its frames are
traced from inside the water (the standard eye of scenes.procedural is above that world) and hardly a cell of it is lit — so the
cases that need open air (the edits, the trips that get fewer) use the 4^3-chunk world.
"""
import numpy as np
import pytest

from voxelraytracing_amd import MODE_PRIMARY_SHADOW, scenes
from voxelraytracing_amd.world import ClientWorld, gen_height, svo_build_by_set_node

import step_limit_scenes as L
from util import assert_frame_parity, gpu_for_scene

pytestmark = pytest.mark.gpu

LIMESTONE, WATER = 4, 3
SETTLE = 8


def suns(w):
    """(name, sun_pos, marks expected) for a world of w voxels a side whose min corner is the origin."""
    f = float(w)
    return [
        ("+y", (10000.0, 20000.0, 5000.0), True),
        ("+x", (20000.0, 9000.0, 5000.0), True),
        ("-x", (-20000.0, 9000.0, 5000.0), True),
        ("+z", (5000.0, 9000.0, 20000.0), True),
        ("-z", (5000.0, 9000.0, -20000.0), True),
        ("below the horizon", (5000.0, -20000.0, 3000.0), True),        # (marks towards -y: nearly every ray is occluded)
        ("close over the world", (f / 2 + 0.3, 1.6 * f + 10.0, f / 2 + 0.7), True),   # rays fan out: footprints of up to 3 x 3 cells
        ("slope above 1", (20000.0, 20000.0, 5000.0), False),
        ("inside the world", (f / 2 + 0.3, f - 3.2, f / 2 + 0.7), False),
    ]


def render_and_check(orc, gpu, sc, what, oracle=None, stats=False):
    w, h = sc.size
    o = oracle or orc.from_package_scene(sc)
    r_rgb, r_ids, r_steps, _ = o.render(MODE_PRIMARY_SHADOW, w, h, want_steps=True)
    # the marks follow a change of the sun or of the tables once four frames of a table set have asked for the same ones (an edit
    # gives every frame set its own tables): eight frames, the last ones with the marks — and with two in flight, overlapping
    for _ in range(SETTLE):
        gpu.render(MODE_PRIMARY_SHADOW, timed=True)
    rgb, ids, _ = gpu.read_output()
    assert_frame_parity(rgb, ids, r_rgb, r_ids, what)
    if stats:
        gpu.render(MODE_PRIMARY_SHADOW, stats=True)
        assert np.array_equal(gpu.read_steps(), r_steps), f"{what}: step counts of the counting kernel"
    return r_ids, r_steps


@pytest.mark.parametrize("in_flight", [1, 2])
@pytest.mark.parametrize("size", [(64, 40), (128, 72)])
@pytest.mark.parametrize("chunks", [2, 4])
def test_every_sun_matches_the_oracle(orc, chunks, size, in_flight):
    sc = scenes.procedural(chunks, size)
    if chunks == 2:   # (an eye inside the world: just under its top face, in the water)
        sc = scenes._scene(sc.name, sc.world, size, (32.5, 62.5, 32.5), sc.rot, MODE_PRIMARY_SHADOW)
    gpu = gpu_for_scene(sc)
    gpu.set_frames_in_flight(in_flight)
    shadowed = lit_rays = 0
    try:
        for k, (name, sun, marks) in enumerate(suns(chunks * 32)):
            sc.settings.sun_pos[:] = sun
            gpu.write_settings(sc.settings)
            r_ids, _ = render_and_check(orc, gpu, sc, f"{chunks}^3 {size} sun {name}, {in_flight} in flight", stats=k < 2)
            m = gpu.sun_marks()
            assert (m["min_leaf"] == 4) == marks and (m["lit_trips"] > 0) == marks, (name, m)
            assert m["passes"] == sum(1 for s in suns(chunks * 32)[:k + 1] if s[2]), (name, m)   # one pass per sun that gets marks
            shadowed += int(((r_ids & orc.ID_SHADOWED) != 0).sum())
            lit_rays += int((((r_ids & orc.ID_SHADOW_RAY) != 0) & ((r_ids & orc.ID_SHADOWED) == 0)).sum())
        assert chunks == 2 or (shadowed and lit_rays)
    finally:
        gpu.close()


GX, GZ = 96, 64   # a place on dry land of the 4^3-chunk world (height 88, the sea is at 70; trees and hills around it stay below 104)
PLATE_Y = 120     # ... and open air above it
PLATE_CELL = ((GZ + 5) // 4, PLATE_Y // 4, (GX + 13) // 4)   # [z, y, x] of the cell grid


def _plate(h):
    """A 7 x 7 plate of limestone in the open air, 32 voxels above the ground under the eye and moved along the sun's direction
    (0.44, 0.87, 0.22): its shadow falls there."""
    return [(GX + 13 + i, PLATE_Y, GZ + 5 + j) for i in range(7) for j in range(7)]


def _edit(gpu, world, cells, voxel):
    for p in cells:
        start, n = world.set_voxel(p, voxel)
        gpu.write_nodes(world.nodes_ptr(), start, start + n)


@pytest.mark.parametrize("in_flight", [1, 2])
def test_moved_sun_and_edits_rebuild_the_marks(orc, in_flight):
    world = scenes.procedural(4, (128, 72)).world
    ground = gen_height(1, GX, GZ)
    sc = scenes._scene("looking down", world, (128, 72), (GX + 0.5, ground + 24.5, GZ + 0.5), (89.0, 0.0, 0.0), MODE_PRIMARY_SHADOW)
    gpu = gpu_for_scene(sc)
    gpu.set_frames_in_flight(in_flight)
    try:
        S = orc.ID_SHADOWED
        ids0, _ = render_and_check(orc, gpu, sc, "before")
        assert gpu.sun_marks()["passes"] == 1
        # equal settings, camera, roots and world data written again before every frame: no pass
        for _ in range(SETTLE + 2):
            gpu.write_settings(sc.settings)
            gpu.write_cam_data(sc.cam)
            gpu.write_chunk_roots(sc.world.chunk_roots())
            gpu.write_world_data(sc.world.world_data())
            gpu.render(MODE_PRIMARY_SHADOW, timed=True)
        assert gpu.sun_marks()["passes"] == 1
        # the sun moves: one pass, and again none while it stands
        sc.settings.sun_pos[:] = (9000.0, 20000.0, -6000.0)
        gpu.write_settings(sc.settings)
        render_and_check(orc, gpu, sc, "sun moved")
        assert gpu.sun_marks()["passes"] == 2
        sc.settings.sun_pos[:] = scenes.SUN_POS
        gpu.write_settings(sc.settings)
        render_and_check(orc, gpu, sc, "sun moved back")
        passes = gpu.sun_marks()["passes"]
        assert passes == 3
        # solid voxels on paths that were lit: the ground below is in shadow in the next frame
        plate = _plate(ground)
        BELOW = (PLATE_CELL[0], PLATE_CELL[1] - 1, PLATE_CELL[2])
        lit_before = gpu.sun_marks(cells=True)["lit"]
        assert lit_before[PLATE_CELL] == 1, "the plate's place was not lit: the case shows nothing"
        _edit(gpu, sc.world, plate, LIMESTONE)
        ids1, _ = render_and_check(orc, gpu, sc, "plate placed")
        newly = ((ids1 & S) != 0) & ((ids0 & S) == 0) & ((ids0 | S) == (ids1 | S))   # the same hit, now in shadow
        assert int(newly.sum()) >= 100
        m = gpu.sun_marks(cells=True)
        # (an edit splits the table sets: with two frames in flight each set makes its marks again)
        assert m["passes"] > passes and m["lit"][PLATE_CELL] == 0
        passes = m["passes"]
        assert lit_before[BELOW] == 1 and m["lit"][BELOW] == 0, "a cell under the plate is still marked lit"
        # ... and removed again: the frame of before, the cells lit again
        _edit(gpu, sc.world, plate, 0)
        ids2, _ = render_and_check(orc, gpu, sc, "plate removed")
        assert ((ids2 & S)[newly] == 0).all()
        m = gpu.sun_marks(cells=True)
        assert m["passes"] > passes and m["lit"][PLATE_CELL] == 1
        assert m["lit"][BELOW] == lit_before[BELOW]
        passes = m["passes"]
        # the chunk under the eye dropped to one air leaf
        n = sc.world.size_in_chunks()
        roots = sc.world.chunk_roots().copy()
        at = (GX // 32) + n * ((ground // 32) + n * (GZ // 32))
        assert roots[at] != 0
        roots[at] = 0
        gpu.write_chunk_roots(roots)
        o = orc.OracleScene(sc.world.nodes(), roots, sc.materials, sc.cam, sc.settings, sc.world.world_data())
        ids3, _ = render_and_check(orc, gpu, sc, "chunk dropped", oracle=o)
        assert not np.array_equal(ids3, ids2) and gpu.sun_marks()["passes"] > passes
    finally:
        gpu.close()


@pytest.mark.parametrize("in_flight", [1, 2])
def test_a_sun_that_swings_between_two_places_collects_no_pass(orc, in_flight):
    """The settle count is of frames IN A ROW that ask for the same marks.  A sun that is written before every frame, at B and at A
    in turn, never gets a pass: a frame at A finds the held marks and starts B's count over, a frame at B runs without marks.  A
    count that B's frames collected one at a time would launch a pass on B's fourth visit."""
    world = scenes.procedural(4, (64, 40)).world
    ground = gen_height(1, GX, GZ)
    sc = scenes._scene("looking down", world, (64, 40), (GX + 0.5, ground + 24.5, GZ + 0.5), (89.0, 0.0, 0.0), MODE_PRIMARY_SHADOW)
    sun_a, sun_b = tuple(scenes.SUN_POS), (9000.0, 20000.0, -6000.0)
    w, h = sc.size
    ref = {}
    for name, sun in (("A", sun_a), ("B", sun_b)):   # two oracle frames, each for its sun
        sc.settings.sun_pos[:] = sun
        r_rgb, r_ids, _, _ = orc.from_package_scene(sc).render(MODE_PRIMARY_SHADOW, w, h, want_steps=True)
        ref[name] = (r_rgb, r_ids)
    gpu = gpu_for_scene(sc)
    gpu.set_frames_in_flight(in_flight)

    def frame(name, sun):
        sc.settings.sun_pos[:] = sun
        gpu.write_settings(sc.settings)
        gpu.render(MODE_PRIMARY_SHADOW, timed=True)
        return gpu.sun_marks(), gpu.lit_voxels()

    try:
        for _ in range(SETTLE):
            held, held_voxels = frame("A", sun_a)
        print("after A settled:", held, held_voxels)
        assert held["passes"] == 1 and held["lit_trips"] > 0, held
        for k in range(12):
            name, sun = (("B", sun_b), ("A", sun_a))[k % 2]
            m, v = frame(name, sun)
            print(f"frame {k} at {name}:", m, v)
            assert m["passes"] == 1, (k, name, m)
            if name == "B":   # the frame ran without marks
                assert m["lit_trips"] == 0 and v["lit_trips"] == 0, (k, m, v)
            else:             # the held marks are handed out again
                assert m["lit_trips"] == held["lit_trips"] and v["lit_trips"] == held_voxels["lit_trips"], (k, m, v)
            if k >= 10:       # the last frame at B and the last at A
                rgb, ids, _ = gpu.read_output()
                assert_frame_parity(rgb, ids, *ref[name], f"swinging sun, last frame at {name}, {in_flight} in flight")
        for _ in range(SETTLE):
            m, _ = frame("B", sun_b)
        print("after B settled:", m)
        assert m["passes"] == 2, m
    finally:
        gpu.close()


def _open_air_exhaustion_world():
    """The step-limit world's limestone lattice alone (tests/step_limit_scenes.py), in rows 16..23: one-voxel air leaves between the
    voxels, and above them — rows 24..31 of the chunk layer — air leaves of 8 voxels, then missing chunks."""
    x, y, z = np.meshgrid(np.arange(32), np.arange(32), np.arange(32), indexing="ij")
    dense = np.zeros(32768, dtype=np.uint16)
    at = x + 32 * (y + 32 * z)
    dense[at[(x % 2 == 0) & (y % 2 == 0) & (z % 2 == 0) & (y >= 16) & (y < 24)]] = LIMESTONE
    nodes = svo_build_by_set_node(dense)
    world = ClientWorld((L.S // 2,) * 3, 1 << 23, L.S)
    for cx in range(L.S):
        for cz in range(L.S):
            world.create_chunk((cx, 0, cz), nodes)
    return world


@pytest.mark.parametrize("size", L.SIZES)
def test_shadow_rays_that_run_out_in_open_air_stay_occluded(orc, size):
    """The step budget (docs/NUMERICS.md "Lit stops").  The eye sinks onto the top of the lattice's last row; the sun stands 0.0029
    above the horizontal along the heading, so a shadow ray walks the all-air plane y = 23 one voxel per lookup for some 480
    lookups, rises into the 8-voxel air leaves above the lattice — LIT cells: nothing lies between them and the sun — and runs out
    of its 500 lookups there, well short of the world's face.  The reference reports such a ray as occluded.  It reaches the lit
    cells long after the wave's lit_trips (203 for this world), so the marks must let it pass; a kernel that stopped it there
    would report it lit."""
    world = _open_air_exhaustion_world()
    sc = scenes._scene(f"open-air exhaustion {size}", world, size, (1.5, 23.5, 1.5), (1.15, L.YAW, 0.0), MODE_PRIMARY_SHADOW,
                       fov=L.FOV_PER_ROW * size[1])
    sc.settings.sun_pos[:] = (74300.0, 313.0, 66900.0)
    # from the oracle: shadow rays that end after 500 lookups in a leaf of 8 voxels or more (depth <= 2) that is neither solid nor water
    o = orc.from_package_scene(sc)
    _, r_ids, r_steps, _ = o.render(MODE_PRIMARY_SHADOW, *size, want_steps=True)
    open_air = 0
    for py, px in np.argwhere(((r_steps >> 16) == 500) & ((r_ids & orc.ID_SHADOWED) != 0)):
        segs = o.trace_segments(MODE_PRIMARY_SHADOW, int(px), int(py))
        open_air += int(len(segs) == 2 and segs[1]["steps"] == 500 and not segs[1]["solid"] and not segs[1]["water"] and segs[1]["depth"] <= 2)
    assert open_air >= 8, "no shadow ray runs out in open air: the case shows nothing"
    gpu = gpu_for_scene(sc)
    try:
        for in_flight in (1, 2):
            gpu.set_frames_in_flight(in_flight)
            render_and_check(orc, gpu, sc, f"{sc.name}, {in_flight} in flight", oracle=o, stats=True)
            m = gpu.sun_marks(cells=True)
            assert m["min_leaf"] == 8 and m["lit_trips"] == 203, m
            # the rays climb from y = 23: the leaves of 8 voxels and more they can end in are the air above the lattice, rows 24 and up
            assert m["lit"][:, 6:, :].all(), "the air above the lattice is not lit"
    finally:
        gpu.close()


@pytest.mark.parametrize("size", L.SIZES)
def test_step_limit_scenes_with_marks(orc, size):
    """The step-limit world itself: its low sun gets marks (leaves of 8 voxels and up); its shadow rays run out inside the water
    lattice, on lanes in water, which never consult the marks."""
    world = L.build_world()
    sc = L.scene(world, L.CAMERAS[0], size, MODE_PRIMARY_SHADOW)
    gpu = gpu_for_scene(sc)
    ran_out = 0
    try:
        for in_flight in (1, 2):
            gpu.set_frames_in_flight(in_flight)
            for cam in L.CAMERAS:
                sc = L.scene(world, cam, size, MODE_PRIMARY_SHADOW)
                gpu.write_cam_data(sc.cam)
                gpu.write_settings(sc.settings)
                r_ids, r_steps = render_and_check(orc, gpu, sc, f"{sc.name}, {in_flight} in flight", stats=True)
                ran_out += int((((r_steps >> 16) == 500) & ((r_ids & orc.ID_SHADOWED) != 0)).sum())
                m = gpu.sun_marks()
                assert m["min_leaf"] == 8 and 0 < m["lit_trips"] < 500, m
        assert ran_out, "no shadow ray ran out"
    finally:
        gpu.close()


def test_a_grid_swept_by_one_launch_per_layer(orc):
    """10^3 chunks: 80^3 cells, more than one workgroup walks — the lit pass is a launch per layer — and open air over the terrain.
    Frames against the oracle; the marks against what the terrain allows: no lit cell below the ground, lit cells in the sky."""
    sc = scenes.procedural(10, (128, 72))
    gpu = gpu_for_scene(sc)
    try:
        for k, (name, sun, marks) in enumerate(suns(320)[:5]):
            sc.settings.sun_pos[:] = sun
            gpu.write_settings(sc.settings)
            for in_flight in (1, 2):
                gpu.set_frames_in_flight(in_flight)
                r_ids, _ = render_and_check(orc, gpu, sc, f"10^3 sun {name}, {in_flight} in flight", stats=k == 0 and in_flight == 1)
            m = gpu.sun_marks(cells=k == 0)
            assert m["min_leaf"] == 4 and m["passes"] == k + 1, (name, m)
            assert ((r_ids & orc.ID_SHADOWED) != 0).any() and (((r_ids & orc.ID_SHADOW_RAY) != 0) & ((r_ids & orc.ID_SHADOWED) == 0)).any()
            if k == 0:   # the sun high over the world
                grid, _ = gpu.read_accel()
                air = grid >= 0xFF800000
                assert not m["lit"][~air].any() and m["lit"][:, 76:, :][air[:, 76:, :]].all()   # (the top 16 voxels: nothing above them)
                col = np.argwhere(~air[:, :40, :])[0]   # some cell of the terrain: the air cell right under it on the sun's side is not lit
                assert not m["lit"][tuple(col)]
    finally:
        gpu.close()


def test_water_lanes_are_left_alone(orc):
    """Limestone under four voxels of water: the primary rays enter the water, the shadow rays start inside it — lanes in water keep
    their bookkeeping and take the general step — and climb out into lit air."""
    x, y, z = np.meshgrid(np.arange(32), np.arange(32), np.arange(32), indexing="ij")
    dense = np.zeros(32768, dtype=np.uint16)
    at = x + 32 * (y + 32 * z)
    dense[at[y < 8]] = LIMESTONE
    dense[at[(y >= 8) & (y < 12)]] = WATER
    dense[at[(y >= 8) & (y < 20) & (x >= 12) & (x < 15) & (z >= 12) & (z < 15)]] = LIMESTONE   # a pillar: something casts a shadow
    nodes = svo_build_by_set_node(dense)
    world = ClientWorld((1, 1, 1), 1 << 20, 2)
    for cx in range(2):
        for cz in range(2):
            world.create_chunk((cx, 0, cz), nodes)
    for size in [(64, 40), (128, 72)]:
        sc = scenes._scene(f"water {size}", world, size, (30.5, 30.5, 30.5), (40.0, 35.0, 0.0), MODE_PRIMARY_SHADOW)
        gpu = gpu_for_scene(sc)
        try:
            for in_flight in (1, 2):
                gpu.set_frames_in_flight(in_flight)
                r_ids, _ = render_and_check(orc, gpu, sc, f"{sc.name}, {in_flight} in flight", stats=True)
            assert ((r_ids & orc.ID_WATER) != 0).any() and ((r_ids & orc.ID_SHADOW_RAY) != 0).any()
            assert ((r_ids & orc.ID_SHADOWED) != 0).any() and gpu.sun_marks()["min_leaf"] == 4
        finally:
            gpu.close()


def test_the_marks_shorten_the_shadow_march(orc, monkeypatch):
    """4^3 chunks (see above), the sun high: the trips a tile's wave notes (vrt_read_tile_cost: a lane's trips through its primary
    and its shadow loop, the maximum over the wave) are bounded by the oracle's per-tile maxima, and the marks make them fewer;
    the counting kernel still reports the oracle's counts.  (A wave's trips are not the oracle's counts tile for tile: a lane
    that stops in the compiled step leaves with its own count, one parked in the loop with the wave's — so the frames with and
    without the marks are compared with each other, and both with the oracle's maxima as a bound: max primary + max shadow, and
    one trip per loop for the lookup a lane stops on.)"""
    sc = scenes.procedural(4, (128, 72))
    other = scenes._scene("another view", sc.world, sc.size, sc.eye, (35.0, 120.0, 0.0), MODE_PRIMARY_SHADOW)
    w, h = sc.size
    _, r_ids, r_steps, _ = orc.from_package_scene(sc).render(MODE_PRIMARY_SHADOW, w, h, want_steps=True)
    tiles = (r_steps & 0xFFFF).reshape(h // 8, 8, w // 8, 8).max(axis=(1, 3)) + (r_steps >> 16).reshape(h // 8, 8, w // 8, 8).max(axis=(1, 3))
    tiles = tiles.reshape(-1).astype(np.int64)
    cost = {}
    for marks in ("0", "1"):
        monkeypatch.setenv("VRT_SUN_MARKS", marks)
        gpu = gpu_for_scene(sc)
        try:
            gpu.set_frames_in_flight(1)
            gpu.write_cam_data(other.cam)   # another view first: the marks are made while it is drawn
            for _ in range(SETTLE):
                gpu.render(MODE_PRIMARY_SHADOW, timed=True)
            gpu.write_cam_data(sc.cam)
            for _ in range(3):      # (the second plain frame of a view at rest notes its trips)
                gpu.render(MODE_PRIMARY_SHADOW, timed=True)
            rgb, ids, _ = gpu.read_output()
            assert np.array_equal(ids, r_ids)
            cost[marks] = gpu.read_tile_cost(tiles.size).astype(np.int64)
            assert (gpu.sun_marks()["min_leaf"] == 4) == (marks == "1")
            gpu.render(MODE_PRIMARY_SHADOW, stats=True)
            assert np.array_equal(gpu.read_steps(), r_steps)
        finally:
            gpu.close()
    print("trips per frame: oracle", int(tiles.sum()), "without marks", int(cost["0"].sum()), "with marks", int(cost["1"].sum()))
    assert (cost["0"] <= tiles + 2).all()
    assert (cost["1"] <= cost["0"]).all() and (cost["1"] < cost["0"]).any()
    # (the step counts of the headline scene predict - 18 % of the shadow trips; a third of that shows the marks at work)
    shadow_trips = int((r_steps >> 16).reshape(h // 8, 8, w // 8, 8).max(axis=(1, 3)).sum())
    assert int(cost["0"].sum() - cost["1"].sum()) * 100 >= 6 * shadow_trips, "the marks save less than 6 % of the shadow trips"
