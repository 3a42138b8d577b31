"""The step-limit scenes (tests/step_limit_scenes.py) contain every way a ray can end at the 500-lookup limit — counted on the
CPU, so that a scene edited until a class drops out fails here without a GPU.  The numpy restatement's raised limit says where
a ray that runs out would have stopped; at the shader's 500 it must agree with the oracle."""
import numpy as np

from voxelraytracing_amd import MODE_PRIMARY

import step_limit_scenes as L
import wgsl_numpy

SEED = 3
NAMES = {"a": "runs out in air, no water", "b": "runs out in water", "c": "first solid at lookup 499",
         "d": "first solid at lookup 500 (shadow ray cast)", "e": "first solid at lookup 501 (no shadow ray)",
         "f": "shadow ray runs out (occluded)", "g": "8x8 tiles with exhausted and early lanes",
         "h": "bounce segment runs out on water in a split cell"}


def test_numpy_restatement_agrees_with_the_oracle_at_the_limit(orc):
    world = L.build_world()
    out_of_steps = 0
    for sc in L.primary_scenes(world)[:len(L.CAMERAS)]:
        w, h = sc.size
        _, r_ids, r_steps, _ = orc.from_package_scene(sc).render(MODE_PRIMARY, w, h, want_steps=True)
        _, n_ids, n_it = wgsl_numpy.render_primary(world.nodes(), world.chunk_roots(), sc.materials, sc.cam, sc.settings,
                                                   world.world_data(), w, h)
        assert np.array_equal(r_ids, n_ids), sc.name
        assert np.array_equal(r_steps & 0xFFFF, n_it), sc.name
        out_of_steps += int((n_it == 500).sum())
    assert out_of_steps > 0


def test_every_step_limit_class_is_present(orc):
    world = L.build_world()
    counts = dict.fromkeys(NAMES, 0)
    for sc in L.primary_scenes(world):
        for k, v in L.classify_primary(orc, sc).items():
            counts[k] += v
    for bounces in (3, 4):
        for sc in L.path_scenes(world, bounces):
            counts["h"] += L.classify_path(orc, sc, SEED)
    for k, name in NAMES.items():
        print(f"({k}) {name}: {counts[k]}")
    missing = [k for k, v in counts.items() if v == 0]
    assert not missing, f"classes without a pixel: {missing}"
