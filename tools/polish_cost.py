"""What polished materials (vrt_write_polish, include/vrt.h) cost a path-traced frame: C4 (1920x1080, 8^3 chunks, 4-bounce
diffuse path trace, 1 spp) with 1 and 2 frames in flight, with no table, with one coated material (the one the frame's primary
rays hit most: chance 0.5, a mirror) and with all 256 coated — and whether having the feature in the library costs a frame that
does not use it: the no-table figure beside that of another build of the backend (the parent commit's libvrt.so, given with
--parent), measured in the same run.

    python tools/polish_cost.py [out.txt] [--parent OLD_LIBVRT.so] [--runs N]

Every measurement is a process of its own (this file again, with --worker; the parent's through VRT_LIB, as tools/ab/ does),
the two builds' processes alternating: N runs each.  Within a process a leg is `frames` back-to-back frames between two
synchronisations, the tables' legs alternate within a round (the table is rewritten between legs: an upload of 8 KiB), and a
figure is the median over the rounds.  Across processes: the median of the runs' figures, and their spread (max - min, in per
cent of the median) — the parent build's own run-to-run spread is what a difference between the builds has to be read against.
Writes profiles/polish_cost.txt (or the path given as the first argument) and prints it."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FRAMES, ROUNDS, WARM = 300, 5, 60
NAMES = ("no table", "1 coated", "256 coated")


def leg(gpu, frames):
    from voxelraytracing_amd import MODE_PATH
    gpu.synchronize()
    t0 = time.perf_counter()
    for _ in range(frames):
        gpu.render(MODE_PATH, spp=1, seed=1)
    gpu.synchronize()
    return (time.perf_counter() - t0) / frames * 1e6


def worker(with_tables):
    """One process: {in flight: {table: median us per frame}} as a JSON line.  with_tables False: a build without
    vrt_write_polish — the no-table legs alone, at the same places in the same rounds."""
    from voxelraytracing_amd import Gpu, MODE_PATH, _ffi, scenes
    sc = scenes.c4()
    gpu = Gpu(sc.world.max_nodes(), sc.world.size_in_chunks(), sc.size, device=0)
    gpu.upload_world(sc.world, sc.materials)
    gpu.write_cam_data(sc.cam)
    gpu.write_settings(sc.settings)
    tabs = {NAMES[0]: np.zeros(256, _ffi.POLISH_DTYPE)}
    if with_tables:
        gpu.render(MODE_PATH, spp=1, seed=1)
        _, ids, _ = gpu.read_output(rgb=False)
        hit = (ids & (1 << 16)) != 0
        most = int(np.bincount((ids[hit] & 0x7FFF).astype(np.int64), minlength=256)[:256].argmax())
        one, every = np.zeros(256, _ffi.POLISH_DTYPE), np.zeros(256, _ffi.POLISH_DTYPE)
        one[most]["chance"], one[most]["color"] = 0.5, (1.0, 0.9, 0.8)
        every["chance"], every["scatter"], every["color"] = 0.5, 0.25, (1.0, 0.9, 0.8)
        tabs[NAMES[1]], tabs[NAMES[2]] = one, every
    out = {}
    for in_flight in (1, 2):
        gpu.set_frames_in_flight(in_flight)
        for t in tabs.values():
            if with_tables:
                gpu.write_polish(t)
            leg(gpu, WARM)
        us = {k: [] for k in tabs}
        for _ in range(ROUNDS):
            for k, t in tabs.items():
                if with_tables:
                    gpu.write_polish(t)
                us[k].append(leg(gpu, FRAMES))
        out[str(in_flight)] = {k: statistics.median(v) for k, v in us.items()}
    gpu.close()
    print("POLISH_COST " + json.dumps(out))


def run(lib):
    env = dict(os.environ)
    args = [sys.executable, os.path.abspath(__file__), "--worker"]
    if lib:
        env["VRT_LIB"], env["VRT_LIB_WITHOUT"] = os.path.abspath(lib), "vrt_write_polish"
        args.append("--no-tables")
    p = subprocess.run(args, env=env, capture_output=True, text=True, timeout=600)
    if p.returncode != 0:
        raise RuntimeError(f"a measuring process failed ({p.returncode}):\n{p.stdout}\n{p.stderr}")
    return json.loads(next(ln for ln in p.stdout.splitlines() if ln.startswith("POLISH_COST "))[len("POLISH_COST "):])


def spread(v):
    return (max(v) - min(v)) / statistics.median(v) * 100.0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("out", nargs="?", default=os.path.join(ROOT, "profiles", "polish_cost.txt"))
    ap.add_argument("--parent", help="libvrt.so of the build to compare the no-table figure against")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--no-tables", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        worker(not a.no_tables)
        return
    new, old = [], []
    for _ in range(a.runs):
        if a.parent:
            old.append(run(a.parent))
        new.append(run(None))
    lines = ["# tools/polish_cost.py: C4 1920x1080 8^3 1 spp, one device; us per frame: the median of %d processes, each the median of %d legs "
             "of %d frames; (spread: max - min over the processes)" % (a.runs, ROUNDS, FRAMES)]
    for in_flight in ("1", "2"):
        base = statistics.median(r[in_flight][NAMES[0]] for r in new)
        parts = []
        for k in NAMES:
            v = [r[in_flight][k] for r in new]
            m = statistics.median(v)
            parts.append(f"{k} {m:8.1f} us ({(m / base - 1.0) * 100.0:+5.2f} %, spread {spread(v):.2f} %)")
        lines.append(f"this build    {in_flight} in flight:  " + "   ".join(parts))
        if a.parent:
            v = [r[in_flight][NAMES[0]] for r in old]
            m = statistics.median(v)
            lines.append(f"parent build  {in_flight} in flight:  {NAMES[0]} {m:8.1f} us (spread {spread(v):.2f} %)   this build's no table against it: "
                         f"{(base / m - 1.0) * 100.0:+5.2f} %")
    if not a.parent:
        lines.append("(no --parent build given: the no-table figure stands alone)")
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
