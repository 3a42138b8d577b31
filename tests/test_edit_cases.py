"""tests/edit_cases.py's table on the host: every case's claim holds on the restatement alone, and the host mirror's
vrth_edit_chunks / vrth_apply_shapes answer what the restatement does, word for word, `changed` included.  That makes the
mirror a proven reference for tests/test_gpu_edit_matrix.py on exactly these inputs."""
import numpy as np
import pytest

from voxelraytracing_amd import world as W

import edit_cases as E
import shapes_ref as R
from test_edit_chunks_ref import _pattern


def _first(a, b):
    bad = np.flatnonzero(np.asarray(a) != np.asarray(b))
    return f"{bad.size} entries differ, first at {bad[0]}: {int(a[bad[0]]):#x}, the restatement {int(b[bad[0]]):#x}"


@pytest.mark.parametrize("name", E.NAMES)
def test_the_claim_holds_and_the_mirror_is_the_restatement(name):
    case = E.get(name)
    r = E.restate(case)
    case.claim(case, r)
    nodes, offs, changed = W.edit_chunks(case.pos, case.nodes, case.offsets, case.shapes, strict=False, threads=4)
    assert (r.offsets[1:] > r.offsets[:-1]).all(), "a case whose answer the builder refuses"
    assert changed.shape == r.changed.shape and np.array_equal(changed, r.changed), "changed: " + _first(changed, r.changed)
    assert offs.shape == r.offsets.shape and np.array_equal(offs, r.offsets), "offsets: " + _first(offs, r.offsets)
    assert nodes.shape == r.nodes.shape and np.array_equal(nodes, r.nodes), "nodes: " + _first(nodes, r.nodes)
    # ... and the two halves of the mirror on their own: the tree read, and the shapes on a block
    read = set()
    for i, p in enumerate(case.pos):
        if id(r.before[i]) not in read:      # (restate reads equal trees once)
            read.add(id(r.before[i]))
            assert np.array_equal(W.svo_to_dense(case.nodes[int(case.offsets[i]):int(case.offsets[i + 1])]), r.before[i]), f"chunk {i}: the tree read"
        if i == 0 or r.after[i] is not r.before[i]:      # every chunk a placement lands in
            got = W.apply_shapes(r.before[i], p, case.shapes)
            assert np.array_equal(got, r.after[i]), f"chunk {i} at {p}: " + _first(got, r.after[i])


def test_every_tree_case_is_a_tree_the_call_accepts():
    """edit_tree_ok's rule restated: every reachable child block inside the words, no split at depth 5, at most 32761 words."""
    for name, (nodes, _) in E.trees().items():
        blocks = E.child_blocks(nodes)
        assert nodes.size <= E.MAX_TREE and all(first + 8 <= nodes.size and d < 5 for d, _, first in blocks), name
    assert set(E.trees()) == set(E.TREE_NAMES)


def test_the_tree_read_against_a_voxel_by_voxel_walk():
    """read_tree is vectorised; here 500 voxels of the deepest trees walk one at a time."""
    rng = np.random.default_rng(3)
    for name in ("voxels in the odd level-4 cells", "child blocks in descending order", "a child block shared by two parents"):
        nodes = E.trees()[name][0]
        block = E.read_tree(nodes)
        for i in rng.integers(0, 32768, 500):
            x, y, z = int(i) & 31, (int(i) >> 5) & 31, int(i) >> 10
            at = 0
            for bit in (4, 3, 2, 1, 0):
                if not nodes[at] & 0x8000:
                    break
                at = (int(nodes[at]) & 0x7FFF) + (((x >> bit) & 1) | (((y >> bit) & 1) << 1) | (((z >> bit) & 1) << 2))
            assert block[i] == nodes[at], (name, x, y, z)


def test_the_whole_pattern_is_refused_and_the_thinned_one_builds():
    for k in range(5):
        full = _pattern((k, 0, 0))
        assert E.mixed_cells(full) == 4096
        with pytest.raises(W.SetVoxelErr):
            W.svo_build_bottom_up(full)
        thin = E.thinned_pattern((k, 0, 0))
        assert E.mixed_cells(thin) == 2176      # every other level-4 cell, and all 256 of the layer y = 8, 9
        assert np.array_equal(E.read_tree(E.pattern_tree((0, k, 0))), thin)
        assert (thin != full).any() and (thin[full == 0] == 0).all() and set(np.unique(thin)) == {0, 4, 7, 11}      # thinner, nothing added


def test_the_restatement_cut_to_a_chunk_is_shapes_refs_apply():
    """edit_cases.apply cuts a sphere's and a disc's loops to the chunk; on shapes small enough for shapes_ref.apply, which
    does not, the two give the same blocks."""
    for name in E.NAMES:
        if name.startswith(("order", "sphere, r = 9.9", "sphere, r = 23.5", "disc, height 3,", "line, tie of all three", "one position")):
            case = E.get(name)
            for i, p in enumerate(case.pos):
                before = E.read_tree(case.nodes[int(case.offsets[i]):int(case.offsets[i + 1])])
                assert np.array_equal(E.apply(before, p, case.shapes), R.apply(before, p, case.shapes)), (name, p)


def test_the_sizes_that_order_the_gpu_run_are_spread():
    """... and the largest case is the largest in each of the call's three device buffers, above each one's floor, with a second
    case above the node floor: what tests/test_gpu_edit_matrix.py's two orders rely on."""
    by_size = sorted(E.NAMES, key=lambda n: E.size(E.get(n)))
    sizes = [E.size(E.get(n)) for n in by_size]
    assert sizes[0] <= 2 and len(set(sizes)) > 30
    words = [int(E.get(n).offsets[-1]) for n in by_size]
    shapes = [len(E.get(n).shapes) for n in by_size]
    entries = [sum(len(b) for b in E.bins(E.get(n).pos, E.get(n).shapes)) for n in by_size]
    assert words[-1] == max(words) > words[-2] > 1 << 20 > max(words[:-2])
    assert shapes[-1] == max(shapes) > 1024 > max(shapes[:-1]) and entries[-1] == max(entries) > 4096 > max(entries[:-1])
