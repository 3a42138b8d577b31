"""What haze (vrt_set_haze, include/vrt.h) costs a path-traced frame: C4 (1920x1080, 8^3 chunks, 4-bounce diffuse path trace, 1 spp)
sun-lit (vrt_set_sun_light, strength 1), with 1 and 2 frames in flight, at density 0 — the sun-lit frame of the same context and the
same process, which is what a haze frame is planned as — and at two densities that are not 0; with --parent-lib, the parent build's
sun-lit frame beside them, with its run-to-run spread.  No speed target is set for a haze frame: it traces more rays by design — a
scatter event's continuation is a segment of its own, where a miss would have ended the path, and every event sends a sun ray.
The ray counts are a stats frame's: vrt_stats.secondary_rays with the setting on and off (path segments behind the primary ones plus
sun rays; tests/test_gpu_haze.py holds the counts to the reference's at the sizes it runs).

    python tools/haze_cost.py [out.txt] [--runs N] [--parent-lib /path/to/the/parent/build/libvrt.so]

Every measurement is a process of its own (this file again, with --worker and the leg's environment), the legs' processes
alternating: N runs each.  Within a process a leg is `frames` back-to-back frames between two synchronisations, and a figure is
the median over the rounds.  Across processes: the median of the runs' figures, and their spread (max - min, in per cent of the
median).  docs/MEASUREMENT.md has the rules.  Writes profiles/haze_cost.txt (or the path given as the first argument) and prints it."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FRAMES, ROUNDS, WARM = 100, 5, 20
SUN = 1.0
ALBEDO = 0.9
DENSITIES = (0.005, 0.02)   # mean free paths of 200 and 50 voxels in a world 256 wide
PARENT = "parent build"


def leg(gpu, frames):
    from voxelraytracing_amd import MODE_PATH
    gpu.synchronize()
    t0 = time.perf_counter()
    for _ in range(frames):
        gpu.render(MODE_PATH, spp=1, seed=1)
    gpu.synchronize()
    return (time.perf_counter() - t0) / frames * 1e3


def worker(haze):
    """One process, one context: {density: {in flight: ms}, density + "_rays": [primary, secondary]} as a JSON line."""
    from voxelraytracing_amd import Gpu, MODE_PATH, scenes
    sc = scenes.c4()
    gpu = Gpu(sc.world.max_nodes(), sc.world.size_in_chunks(), sc.size, device=0)
    gpu.upload_world(sc.world, sc.materials)
    gpu.write_cam_data(sc.cam)
    gpu.write_settings(sc.settings)
    gpu.set_sun_light(SUN)
    out = {}
    for density in (0.0,) + (DENSITIES if haze else ()):
        if density:
            gpu.set_haze(density, ALBEDO)
        key = repr(density)
        out[key] = {}
        gpu.set_frames_in_flight(1)
        gpu.render(MODE_PATH, spp=1, seed=1, stats=True)
        st = gpu.stats()
        out[key + "_rays"] = [int(st.primary_rays), int(st.secondary_rays)]
        for in_flight in (1, 2):
            gpu.set_frames_in_flight(in_flight)
            leg(gpu, WARM)
            out[key][str(in_flight)] = statistics.median(leg(gpu, FRAMES) for _ in range(ROUNDS))
    gpu.close()
    print("HAZE_COST " + json.dumps(out))


def run(haze, extra):
    env = dict(os.environ)
    for k in ("VRT_PATH_POOL", "VRT_PATH_CELLS", "VRT_MARCH_DIRECT_MAX_S", "VRT_PATH_SAMPLES_PER_CHAIN", "VRT_LIB", "VRT_LIB_WITHOUT"):
        env.pop(k, None)
    env.update(extra)
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker"] + (["--haze"] if haze else []), env=env, capture_output=True, text=True,
                       timeout=600)
    if p.returncode != 0:
        raise RuntimeError(f"a measuring process failed ({p.returncode}):\n{p.stdout}\n{p.stderr}")
    return json.loads(next(ln for ln in p.stdout.splitlines() if ln.startswith("HAZE_COST "))[len("HAZE_COST "):])


def spread(v):
    return (max(v) - min(v)) / statistics.median(v) * 100.0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("out", nargs="?", default=os.path.join(ROOT, "profiles", "haze_cost.txt"))
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--parent-lib", default=None, help="libvrt.so of the parent commit's build: its sun-lit frame is measured beside this build's")
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--haze", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        worker(a.haze)
        return
    legs = {"this build": (True, {})}
    if a.parent_lib:
        legs[PARENT] = (False, {"VRT_LIB": os.path.abspath(a.parent_lib), "VRT_LIB_WITHOUT": "vrt_set_haze"})
    res = {k: [] for k in legs}
    for _ in range(a.runs):
        for k, (haze, extra) in legs.items():
            res[k].append(run(haze, extra))
    first = res["this build"][0]
    off = repr(0.0)
    lines = ["# tools/haze_cost.py: C4 1920x1080 8^3 4 bounces 1 spp, sun-lit (strength %g), one device; ms per frame: the median of %d processes, each "
             "the median of %d legs of %d frames; (spread: max - min over the processes).  albedo %g" % (SUN, a.runs, ROUNDS, FRAMES, ALBEDO),
             f"secondary rays of a frame (a stats frame's count on the GPU: path segments behind the primary ones + sun rays): density 0 {first[off + '_rays'][1]}"
             + "".join(f", density {d:g} {first[repr(d) + '_rays'][1]} (+{first[repr(d) + '_rays'][1] - first[off + '_rays'][1]})" for d in DENSITIES)]
    for in_flight in ("1", "2"):
        parts = []
        rows = [(f"density {d:g}", "this build", repr(d)) for d in (0.0,) + DENSITIES]
        if a.parent_lib:
            rows.append(("density 0, parent build", PARENT, off))
        med = {}
        for label, k, field in rows:
            v = [r[field][in_flight] for r in res[k]]
            med[label] = statistics.median(v)
            parts.append(f"{label} {med[label]:7.3f} ms (spread {spread(v):.2f} %)")
        lines.append(f"{in_flight} in flight:  " + "   ".join(parts))
        ratios = "; ".join(f"density {d:g} / density 0 of the same context = "
                           f"{statistics.median(r[repr(d)][in_flight] / r[off][in_flight] for r in res['this build']):.4f}" for d in DENSITIES)
        tail = f"; density 0 / parent's = {med['density 0'] / med['density 0, parent build']:.4f}" if a.parent_lib else "; the parent build was not measured"
        lines.append(f"{in_flight} in flight:  {ratios}{tail}")
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
