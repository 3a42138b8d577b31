"""What progressive accumulation (VRT_RENDER_ACCUMULATE, include/vrt.h) costs a path-traced frame: C4 (1920x1080, 8^3 chunks,
4-bounce diffuse path trace, 1 spp) plain against accumulating, per-frame microseconds with 1 and 2 frames in flight; and the
same at C5's shape (3840x2160, 32^3 chunks, 16 spp) on one device, where the sum's one pass is a small part of the frame.

A leg is `frames` back-to-back frames between two synchronisations (the period a game loop sees), the plain and the
accumulating legs alternate, and each figure is the median over the rounds.  Writes profiles/accum_cost.txt (or the path
given as the first argument) and prints it."""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from voxelraytracing_amd import Gpu, MODE_PATH, scenes  # noqa: E402


def leg(gpu, accumulate, spp, frames):
    if accumulate:
        gpu.reset_accumulation()
    gpu.synchronize()
    t0 = time.perf_counter()
    for _ in range(frames):
        gpu.render(MODE_PATH, spp=spp, seed=1, accumulate=accumulate)
    gpu.synchronize()
    return (time.perf_counter() - t0) / frames * 1e6


def measure(name, sc, spp, frames, rounds, warm):
    gpu = Gpu(sc.world.max_nodes(), sc.world.size_in_chunks(), sc.size, device=0)
    gpu.upload_world(sc.world, sc.materials)
    gpu.write_cam_data(sc.cam)
    gpu.write_settings(sc.settings)
    lines = []
    for in_flight in (1, 2):
        gpu.set_frames_in_flight(in_flight)
        for acc in (False, True):
            leg(gpu, acc, spp, warm)
        us = {False: [], True: []}
        for _ in range(rounds):
            for acc in (False, True):
                us[acc].append(leg(gpu, acc, spp, frames))
        plain, accum = statistics.median(us[False]), statistics.median(us[True])
        lines.append(f"{name}  {in_flight} in flight:  plain {plain:10.1f} us/frame   accumulating {accum:10.1f} us/frame   "
                     f"{(accum / plain - 1.0) * 100.0:+6.2f} %   (median of {rounds} legs of {frames} frames; "
                     f"plain {min(us[False]):.1f}..{max(us[False]):.1f}, accumulating {min(us[True]):.1f}..{max(us[True]):.1f})")
    n, _ = gpu.accumulation()
    lines.append(f"{name}  (the last accumulating leg ended at {n} samples)")
    gpu.close()
    return lines


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "accum_cost.txt")
    lines = ["# tools/accum_cost.py: VRT_RENDER_ACCUMULATE against plain path-traced frames, one device"]
    lines += measure("C4 1920x1080 8^3 1 spp ", scenes.c4(), 1, 400, 7, 100)
    lines += measure("C5 3840x2160 32^3 16 spp", scenes.c5(), 16, 8, 5, 4)
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
