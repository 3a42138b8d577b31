"""vrt_edit_chunks on the MI355X over tests/edit_cases.py's table: nodes, offsets and changed held word for word to the host
mirror's vrth_edit_chunks, which tests/test_edit_cases.py holds to the restatement on these very inputs (and where each case's
claim, what it exercises, is asserted).  No tolerance anywhere.

The table runs twice: smallest case first on one context, largest first on a second.  The largest case ("everything large at
once") is above all three floors of vrt_edit.hip — 2^20 node words, 1024 shapes, 4096 bin entries — so largest-first grows
d_edit_nodes, d_edit_shapes and d_edit_bins from empty straight past their floors, and smallest-first allocates them at the
floors and grows them later: the shapes and bins once (only that case is above their floors), the nodes twice (the 4096-long
line, then that case).  The mirror answers each case once.

A test's parameter is a rank in the order by size, not a case's name: the order needs the cases built, which needs the native
libraries, and collection has to work without them."""
import functools

import numpy as np
import pytest

from voxelraytracing_amd import Gpu
from voxelraytracing_amd import world as W

import edit_cases as E

pytestmark = pytest.mark.gpu

RANKS = range(len(E.NAMES))


@functools.lru_cache(maxsize=None)
def _by_size():
    return sorted(E.NAMES, key=lambda n: (E.size(E.get(n)), n))


@pytest.fixture(scope="module")
def gpu_a():
    g = Gpu(1 << 16, 2, (64, 64), device=0)
    yield g
    g.close()


@pytest.fixture(scope="module")
def gpu_b():
    g = Gpu(1 << 16, 2, (64, 64), device=0)
    yield g
    g.close()


@functools.lru_cache(maxsize=None)
def _mirror(name):
    case = E.get(name)
    return W.edit_chunks(case.pos, case.nodes, case.offsets, case.shapes, strict=False, threads=8)


def _same(gpu, name):
    case = E.get(name)
    want = _mirror(name)
    got = gpu.edit_chunks(case.pos, case.nodes, case.offsets, case.shapes, strict=False)
    for what, a, b in zip(("nodes", "offsets", "changed"), got, want):
        assert a.shape == b.shape, f"{name}: {what}: {a.shape} on the GPU, {b.shape} on the host"
        bad = np.flatnonzero(a != b)
        assert bad.size == 0, f"{name}: {what}: {bad.size} entries differ, first at {bad[0]}: {a[bad[0]]:#x} host {b[bad[0]]:#x}"


@pytest.mark.parametrize("rank", RANKS)
def test_smallest_first(gpu_a, rank):
    _same(gpu_a, _by_size()[rank])


@pytest.mark.parametrize("rank", RANKS)
def test_largest_first(gpu_b, rank):
    _same(gpu_b, _by_size()[::-1][rank])
