"""What translucent materials (vrt_write_translucency, include/vrt.h) cost a path-traced frame: C4 (1920x1080, 8^3 chunks,
4-bounce diffuse path trace, 1 spp) with 1 and 2 frames in flight, as a plain frame (no table), as a polished and emissive
frame (the material the frame's primary rays hit most has a coat — chance 0.5, a mirror — and the second gives off light), and
as a translucent frame: the same two tables plus a chance of 0.5, tinted, on that commonest material.  The figure is the
translucent frame's time over the polished frame's, from the same context in the same run — and, so that it can be read
against something, the plain frame of another build of the backend (the parent commit's libvrt.so, given with --parent)
measured in the same run, with that build's own run-to-run spread.

    python tools/translucent_cost.py [out.txt] [--parent OLD_LIBVRT.so] [--runs N]

Every measurement is a process of its own (this file again, with --worker; the parent's through VRT_LIB, as tools/ab/ does),
the two builds' processes alternating: N runs each.  Within a process a leg is `frames` back-to-back frames between two
synchronisations, the tables' legs alternate within a round (the tables are rewritten between legs: uploads of a few KiB), and
a figure is the median over the rounds.  Across processes: the median of the runs' figures, and their spread (max - min, in
per cent of the median).  A translucent frame is not the polished frame's work: a path that passes goes on where a bounced one
would have turned, so the two frames march other rays; no cost is fixed in advance.
Writes profiles/translucent_cost.txt (or the path given as the first argument) and prints it."""
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
NAMES = ("plain", "polished + emissive", "translucent")


def leg(gpu, frames):
    from voxelraytracing_amd import MODE_PATH
    gpu.synchronize()
    t0 = time.perf_counter()
    for _ in range(frames):
        gpu.render(MODE_PATH, spp=1, seed=1)
    gpu.synchronize()
    return (time.perf_counter() - t0) / frames * 1e6


def worker(with_tables):
    """One process: {in flight: {leg: median us per frame}} as a JSON line.  with_tables False: a build without
    vrt_write_translucency — the plain legs alone, at the same places in the same rounds."""
    from voxelraytracing_amd import Gpu, MODE_PATH, _ffi, scenes
    sc = scenes.c4()
    gpu = Gpu(sc.world.max_nodes(), sc.world.size_in_chunks(), sc.size, device=0)
    gpu.upload_world(sc.world, sc.materials)
    gpu.write_cam_data(sc.cam)
    gpu.write_settings(sc.settings)
    zero = (np.zeros(256, np.float32), np.zeros(256, _ffi.POLISH_DTYPE), None)
    legs = {NAMES[0]: zero}
    if with_tables:
        zero = (zero[0], zero[1], np.zeros(256, _ffi.TRANSLUCENCY_DTYPE))
        gpu.render(MODE_PATH, spp=1, seed=1)
        _, ids, _ = gpu.read_output(rgb=False)
        hit = (ids & (1 << 16)) != 0
        top = np.argsort(np.bincount((ids[hit] & 0x7FFF).astype(np.int64), minlength=256)[:256])[::-1]
        emission, polish, through = zero[0].copy(), zero[1].copy(), zero[2].copy()
        emission[int(top[1])] = 1.5
        polish[int(top[0])]["chance"], polish[int(top[0])]["color"] = 0.5, (1.0, 0.9, 0.8)
        through[int(top[0])]["chance"], through[int(top[0])]["color"] = 0.5, (0.9, 0.6, 0.3)
        legs = {NAMES[0]: zero, NAMES[1]: (emission, polish, zero[2]), NAMES[2]: (emission, polish, through)}

    def write(t):
        if not with_tables:
            return
        gpu.write_emission(t[0])
        gpu.write_polish(t[1])
        gpu.write_translucency(t[2])

    out = {}
    for in_flight in (1, 2):
        gpu.set_frames_in_flight(in_flight)
        for t in legs.values():
            write(t)
            leg(gpu, WARM)
        us = {k: [] for k in legs}
        for _ in range(ROUNDS):
            for k, t in legs.items():
                write(t)
                us[k].append(leg(gpu, FRAMES))
        out[str(in_flight)] = {k: statistics.median(v) for k, v in us.items()}
    gpu.close()
    print("TRANSLUCENT_COST " + json.dumps(out))


def run(lib):
    env = dict(os.environ)
    args = [sys.executable, os.path.abspath(__file__), "--worker"]
    if lib:
        env["VRT_LIB"], env["VRT_LIB_WITHOUT"] = os.path.abspath(lib), "vrt_write_translucency"
        args.append("--no-tables")
    p = subprocess.run(args, env=env, capture_output=True, text=True, timeout=600)
    if p.returncode != 0:
        raise RuntimeError(f"a measuring process failed ({p.returncode}):\n{p.stdout}\n{p.stderr}")
    return json.loads(next(ln for ln in p.stdout.splitlines() if ln.startswith("TRANSLUCENT_COST "))[len("TRANSLUCENT_COST "):])


def spread(v):
    return (max(v) - min(v)) / statistics.median(v) * 100.0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("out", nargs="?", default=os.path.join(ROOT, "profiles", "translucent_cost.txt"))
    ap.add_argument("--parent", help="libvrt.so of the build to compare the plain frame against")
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
    lines = ["# tools/translucent_cost.py: C4 1920x1080 8^3 1 spp, one device; us per frame: the median of %d processes, each the median of %d "
             "legs of %d frames; (spread: max - min over the processes)" % (a.runs, ROUNDS, FRAMES)]
    for in_flight in ("1", "2"):
        parts = []
        for k in NAMES:
            v = [r[in_flight][k] for r in new]
            parts.append(f"{k} {statistics.median(v):8.1f} us (spread {spread(v):.2f} %)")
        lines.append(f"this build    {in_flight} in flight:  " + "   ".join(parts))
        ratio = [r[in_flight][NAMES[2]] / r[in_flight][NAMES[1]] for r in new]
        lines.append(f"              {in_flight} in flight:  translucent / polished + emissive = {statistics.median(ratio):.4f} "
                     f"(per process: {', '.join('%.4f' % x for x in ratio)})")
        if a.parent:
            v = [r[in_flight][NAMES[0]] for r in old]
            m = statistics.median(v)
            base = statistics.median(r[in_flight][NAMES[0]] for r in new)
            lines.append(f"parent build  {in_flight} in flight:  {NAMES[0]} {m:8.1f} us (spread {spread(v):.2f} %)   this build's plain frame against it: "
                         f"{(base / m - 1.0) * 100.0:+5.2f} %")
    if not a.parent:
        lines.append("(no --parent build given: this build's figures stand alone)")
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
