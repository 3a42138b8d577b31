"""What placing features costs (include/vrt.h vrt_edit_chunks) on one MI355X against the host mirror's vrth_edit_chunks on 16
threads: 512 generated chunks (an 8 x 8 x 8 block of seed 1's world), one tree-plus-lake set of shapes per chunk column (64
columns; the tree stands on the column's ground, the lake lies beside it), host clock around each call, which waits for its
results; the nodes, offsets and changed flags of the two are compared word for word in the same run.

    python tools/edit_shapes_cost.py [out.txt] [--quick]

Writes profiles/edit_shapes_cost.txt (or the path given first) and prints it."""
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from voxelraytracing_amd import Gpu  # noqa: E402
from voxelraytracing_amd import world as W  # noqa: E402

SEED, WOOD, LEAVES, WATER = 1, 53, 62, 3


def column_shapes(cx, cz):
    """Feature::Tree's and Feature::Lake's calls (server/src/world/gen.rs:360-391, 470-484) with fixed draws, on column (cx, cz)."""
    x, z = 32 * cx + 12, 32 * cz + 14
    y = W.gen_height(SEED, x, z)
    top = (x, y + 12, z)
    end = (x + 4, y + 9, z - 5)
    shapes = [W.shape_sphere(top, 5.0, LEAVES), W.shape_sphere(end, 3.0, LEAVES), W.shape_line((x, y + 7, z), end, WOOD),
              W.shape_line((x, y, z), top, WOOD)]
    lx, lz = x + 14, z + 12            # the lake crosses into the next column
    ly = W.gen_height(SEED, lx, lz)
    r = 8 * 0.5 - 0.1
    shapes += [W.shape_disc((lx, ly - d - 3, lz), r - d * 0.5, 1, WATER) for d in range(4)]
    shapes += [W.shape_disc((lx, ly - d, lz), r, 1, 0) for d in range(-2, 3)]
    return shapes


def timed(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts), out


def main():
    args = sys.argv[1:]
    reps = 3 if "--quick" in args else 15
    out_path = args[0] if args and not args[0].startswith("--") else os.path.join(ROOT, "profiles", "edit_shapes_cost.txt")
    pos = [(x, y, z) for z in range(8) for y in range(8) for x in range(8)]
    gpu = Gpu(1 << 16, 2, (64, 64), device=0)
    nodes, offs = gpu.generate_chunks(SEED, pos)
    shapes = W.shape_records([s for cz in range(8) for cx in range(8) for s in column_shapes(cx, cz)])
    g_med, g_best, got = timed(lambda: gpu.edit_chunks(pos, nodes, offs, shapes), reps)
    c_med, c_best, want = timed(lambda: W.edit_chunks(pos, nodes, offs, shapes, threads=16), reps)
    c1_med, _, _ = timed(lambda: W.edit_chunks(pos, nodes, offs, shapes, threads=1), max(1, reps // 5))
    same = all(np.array_equal(a, b) for a, b in zip(got, want))
    lines = [
        "# tools/edit_shapes_cost.py: vrt_edit_chunks against vrth_edit_chunks, one MI355X",
        f"512 generated chunks (seed {SEED}, 8 x 8 x 8), {nodes.size} nodes in, {shapes.size} shapes (a tree and a lake per column), "
        f"{int(want[2].sum())} chunks changed, {want[0].size} nodes out",
        f"nodes, offsets and changed of the two, word for word: {'equal' if same else 'DIFFERENT'}",
        f"Gpu.edit_chunks                       {g_med:8.2f} ms median, {g_best:8.2f} ms best of {reps} (the call waits for its results)",
        f"world.edit_chunks, 16 threads         {c_med:8.2f} ms median, {c_best:8.2f} ms best of {reps}",
        f"world.edit_chunks, 1 thread           {c1_med:8.2f} ms median",
        f"GPU / CPU 16 threads                  {g_med / c_med:8.2f} x the time",
    ]
    gpu.close()
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(text)
    print(text, end="")
    if not same:
        sys.exit("the GPU's chunks differ from the host mirror's")


if __name__ == "__main__":
    main()
