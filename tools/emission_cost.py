"""What emissive materials (vrt_write_emission, include/vrt.h) cost a path-traced frame: C4 (1920x1080, 8^3 chunks, 4-bounce
diffuse path trace, 1 spp) with 1 and 2 frames in flight, and a band of C5's shape (3840 x 540 of a 32^3-chunk world, 16 spp),
each with an empty table, one emissive material (the one the frame's primary rays hit most) and eight (the eight most hit).

A leg is `frames` back-to-back frames between two synchronisations; the three tables' legs alternate within a round (the table
is rewritten between legs: an upload of 1 KiB), and each figure is the median over the rounds.  Writes
profiles/emission_cost.txt (or the path given as the first argument) and prints it."""
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from voxelraytracing_amd import Gpu, MODE_PATH, scenes  # noqa: E402


def leg(gpu, spp, frames):
    gpu.synchronize()
    t0 = time.perf_counter()
    for _ in range(frames):
        gpu.render(MODE_PATH, spp=spp, seed=1)
    gpu.synchronize()
    return (time.perf_counter() - t0) / frames * 1e6


def tables(gpu):
    gpu.render(MODE_PATH, spp=1, seed=1)
    _, ids, _ = gpu.read_output(rgb=False)
    hit = (ids & (1 << 16)) != 0
    order = np.argsort(np.bincount((ids[hit] & 0x7FFF).astype(np.int64), minlength=256)[:256])[::-1]
    one, eight = np.zeros(256, np.float32), np.zeros(256, np.float32)
    one[order[0]] = 1.5
    eight[order[:8]] = np.linspace(0.25, 2.0, 8, dtype=np.float32)
    return {"empty": np.zeros(256, np.float32), "1 emissive": one, "8 emissive": eight}


def measure(name, sc, spp, frames, rounds, warm, in_flights):
    gpu = Gpu(sc.world.max_nodes(), sc.world.size_in_chunks(), sc.size, device=0)
    gpu.upload_world(sc.world, sc.materials)
    gpu.write_cam_data(sc.cam)
    gpu.write_settings(sc.settings)
    tabs = tables(gpu)
    lines = []
    for in_flight in in_flights:
        gpu.set_frames_in_flight(in_flight)
        for t in tabs.values():
            gpu.write_emission(t)
            leg(gpu, spp, warm)
        us = {k: [] for k in tabs}
        for _ in range(rounds):
            for k, t in tabs.items():
                gpu.write_emission(t)
                us[k].append(leg(gpu, spp, frames))
        base = statistics.median(us["empty"])
        parts = []
        for k in tabs:
            m = statistics.median(us[k])
            parts.append(f"{k} {m:10.1f} us ({(m / base - 1.0) * 100.0:+5.2f} %, {min(us[k]):.1f}..{max(us[k]):.1f})")
        lines.append(f"{name}  {in_flight} in flight:  " + "   ".join(parts) + f"   (median of {rounds} legs of {frames} frames)")
    gpu.close()
    return lines


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "emission_cost.txt")
    lines = ["# tools/emission_cost.py: path-traced frames with an empty emission table, one emissive material and eight, one device"]
    lines += measure("C4 1920x1080 8^3 1 spp    ", scenes.c4(), 1, 300, 7, 60, (1, 2))
    lines += measure("C5 band 3840x540 32^3 16 spp", scenes.c5((3840, 540)), 16, 6, 5, 2, (1,))
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
