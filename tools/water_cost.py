"""What water optics (vrt_set_water_optics, include/vrt.h) cost a path-traced frame: C4 (1920x1080, 8^3 chunks, 4-bounce diffuse
path trace, 1 spp; its world holds a lake to y = 70) with 1 and 2 frames in flight.  A water frame's time over the plain frame's
of the same context and the same process — the setting off, on the default route (the pool kernel over the march cells) — beside
the same plain frame on the lane route (VRT_PATH_POOL=0: one lane = path launch per bounce, which is what a water frame is planned
onto) and, with --parent-lib, the parent build's plain frame with its run-to-run spread.  No threshold is fixed in advance.  The
ray counts are a stats frame's: vrt_stats.primary_rays and secondary_rays with the setting on and off (a surface event's
continuation is a bounce segment; tests/test_gpu_water.py holds the counts to the reference's at the sizes it runs).

    python tools/water_cost.py [out.txt] [--runs N] [--parent-lib /path/to/the/parent/build/libvrt.so]

Every measurement is a process of its own (this file again, with --worker and the leg's environment), the legs' processes
alternating: N runs each.  Within a process a leg is `frames` back-to-back frames between two synchronisations, and a figure is
the median over the rounds.  Across processes: the median of the runs' figures, and their spread (max - min, in per cent of the
median).  docs/MEASUREMENT.md has the rules.  Writes profiles/water_cost.txt (or the path given as the first argument) and
prints it."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FRAMES, ROUNDS, WARM = 200, 5, 40
OPTICS = ((0.30, 0.12, 0.05), 0.02)
# leg: (measures the water frame too, environment)
LEGS = {"this build": (True, {}), "this build, lane route": (False, {"VRT_PATH_POOL": "0"})}
PARENT = "parent build"


def leg(gpu, frames):
    from voxelraytracing_amd import MODE_PATH
    gpu.synchronize()
    t0 = time.perf_counter()
    for _ in range(frames):
        gpu.render(MODE_PATH, spp=1, seed=1)
    gpu.synchronize()
    return (time.perf_counter() - t0) / frames * 1e6


def worker(water):
    """One process, one context: {"plain": {in flight: us}, "water": {..}, ray counts} as a JSON line."""
    from voxelraytracing_amd import Gpu, MODE_PATH, scenes
    sc = scenes.c4()
    gpu = Gpu(sc.world.max_nodes(), sc.world.size_in_chunks(), sc.size, device=0)
    gpu.upload_world(sc.world, sc.materials)
    gpu.write_cam_data(sc.cam)
    gpu.write_settings(sc.settings)
    out = {"plain": {}, "water": {}}
    for name in ("plain", "water") if water else ("plain",):
        if name == "water":
            gpu.set_water_optics(*OPTICS)
        gpu.set_frames_in_flight(1)
        gpu.render(MODE_PATH, spp=1, seed=1, stats=True)
        st = gpu.stats()
        out[name + "_rays"] = [int(st.primary_rays), int(st.secondary_rays)]
        for in_flight in (1, 2):
            gpu.set_frames_in_flight(in_flight)
            leg(gpu, WARM)
            out[name][str(in_flight)] = statistics.median(leg(gpu, FRAMES) for _ in range(ROUNDS))
    gpu.close()
    print("WATER_COST " + json.dumps(out))


def run(water, extra):
    env = dict(os.environ)
    for k in ("VRT_PATH_POOL", "VRT_PATH_CELLS", "VRT_MARCH_DIRECT_MAX_S", "VRT_PATH_SAMPLES_PER_CHAIN", "VRT_LIB", "VRT_LIB_WITHOUT"):
        env.pop(k, None)
    env.update(extra)
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker"] + (["--water"] if water else []), env=env, capture_output=True, text=True,
                       timeout=600)
    if p.returncode != 0:
        raise RuntimeError(f"a measuring process failed ({p.returncode}):\n{p.stdout}\n{p.stderr}")
    return json.loads(next(ln for ln in p.stdout.splitlines() if ln.startswith("WATER_COST "))[len("WATER_COST "):])


def spread(v):
    return (max(v) - min(v)) / statistics.median(v) * 100.0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("out", nargs="?", default=os.path.join(ROOT, "profiles", "water_cost.txt"))
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--parent-lib", default=None, help="libvrt.so of the parent commit's build: its plain frame is measured beside this build's")
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--water", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        worker(a.water)
        return
    legs = dict(LEGS)
    if a.parent_lib:
        legs[PARENT] = (False, {"VRT_LIB": os.path.abspath(a.parent_lib), "VRT_LIB_WITHOUT": "vrt_set_water_optics"})
    res = {k: [] for k in legs}
    for _ in range(a.runs):
        for k, (water, extra) in legs.items():
            res[k].append(run(water, extra))
    first = res["this build"][0]
    plain_segments, water_segments = sum(first["plain_rays"]), sum(first["water_rays"])
    lines = ["# tools/water_cost.py: C4 1920x1080 8^3 4 bounces 1 spp, one device; us per frame: the median of %d processes, each the median of "
             "%d legs of %d frames; (spread: max - min over the processes).  absorb %s, reflectance %s" % (a.runs, ROUNDS, FRAMES, OPTICS[0], OPTICS[1]),
             f"path segments of a frame (a stats frame's counts on the GPU): plain {plain_segments}, water {water_segments} "
             f"(x {water_segments / plain_segments:.4f}: surface events end a segment, their continuations are segments of their own)"]
    for in_flight in ("1", "2"):
        med, parts = {}, []
        rows = [("water", "this build", "water"), ("plain", "this build", "plain"), ("plain, lane route", "this build, lane route", "plain")]
        if a.parent_lib:
            rows.append(("plain, parent build", PARENT, "plain"))
        for label, k, field in rows:
            v = [r[field][in_flight] for r in res[k]]
            med[label] = statistics.median(v)
            parts.append(f"{label} {med[label]:8.1f} us (spread {spread(v):.2f} %)")
        lines.append(f"{in_flight} in flight:  " + "   ".join(parts))
        ratios = [r["water"][in_flight] / r["plain"][in_flight] for r in res["this build"]]   # the same context, the same process
        tail = f"; plain / parent's plain = {med['plain'] / med['plain, parent build']:.4f}" if a.parent_lib else "; the parent build was not measured"
        lines.append(f"{in_flight} in flight:  water / plain of the same context = {statistics.median(ratios):.4f} (spread {spread(ratios):.2f} %); "
                     f"water / lane route = {med['water'] / med['plain, lane route']:.4f}{tail}")
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
