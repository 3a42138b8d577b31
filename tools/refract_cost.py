"""What refraction (vrt_set_water_refraction, include/vrt.h) costs a water frame: C4 (1920x1080, 8^3 chunks, 4-bounce diffuse path
trace, 1 spp; its world holds a lake to y = 70) from its own eye, above the lake, and from the "underwater" camera inside it, where
every primary segment is wet and the span walk runs on every primary ray.  Three frames per camera: the refracting frame (water
optics on, ior 1.33), the same build's plain water frame (ior 0) in the same context and process, and — with --parent-lib — the
parent build's water frame, which shows what the setting costs while it is off.  No ratio is fixed in advance; the one condition is
that this build's plain water frame lies within the parent's own run-to-run spread.

    python tools/refract_cost.py [out.txt] [--runs N] [--parent-lib /path/to/the/parent/build/libvrt.so]

Every measurement is a process of its own (this file again, with --worker and the leg's environment), the legs' processes
alternating: N runs each.  Within a process a leg is `frames` back-to-back frames between two synchronisations, and a figure is
the median over the rounds.  Across processes: the median of the runs' figures, and their spread (max - min, in per cent of the
median).  docs/MEASUREMENT.md has the rules.  Writes profiles/refract_cost.txt (or the path given as the first argument) and
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

FRAMES, ROUNDS, WARM = 100, 5, 20
OPTICS = ((0.30, 0.12, 0.05), 0.02)
IOR = 1.33
# camera: (eye, rot); None: scenes.c4's own, over the terrain with the lake in view
CAMERAS = {"c4": None, "underwater": ((22.5, 55.5, 80.5), (-20.0, 40.0, 0.0))}
PARENT = "parent build"


def leg(gpu, frames):
    from voxelraytracing_amd import MODE_PATH
    gpu.synchronize()
    t0 = time.perf_counter()
    for _ in range(frames):
        gpu.render(MODE_PATH, spp=1, seed=1)
    gpu.synchronize()
    return (time.perf_counter() - t0) / frames * 1e6


def worker(refract):
    """One process, one context per camera: {camera: {"water": us, "refract": us, "rays": ...}} as a JSON line (2 frames in flight,
    the context's default)."""
    from voxelraytracing_amd import Gpu, MODE_PATH, cam_data_create, scenes
    out = {}
    for name, cam in CAMERAS.items():
        sc = scenes.c4()
        if cam is not None:
            sc.cam = cam_data_create(cam[1], cam[0], 70.0, (float(sc.size[0]), float(sc.size[1])))
        gpu = Gpu(sc.world.max_nodes(), sc.world.size_in_chunks(), sc.size, device=0)
        gpu.upload_world(sc.world, sc.materials)
        gpu.write_cam_data(sc.cam)
        gpu.write_settings(sc.settings)
        gpu.set_water_optics(*OPTICS)
        res = {}
        for kind in ("water", "refract") if refract else ("water",):
            if kind == "refract":
                gpu.set_water_refraction(IOR)
            gpu.render(MODE_PATH, spp=1, seed=1, stats=True)
            st = gpu.stats()
            res[kind + "_rays"] = [int(st.primary_rays), int(st.secondary_rays)]
            leg(gpu, WARM)
            res[kind] = statistics.median(leg(gpu, FRAMES) for _ in range(ROUNDS))
        gpu.close()
        out[name] = res
    print("REFRACT_COST " + json.dumps(out))


def run(refract, extra):
    env = dict(os.environ)
    for k in ("VRT_PATH_POOL", "VRT_PATH_CELLS", "VRT_MARCH_DIRECT_MAX_S", "VRT_PATH_SAMPLES_PER_CHAIN", "VRT_LIB", "VRT_LIB_WITHOUT"):
        env.pop(k, None)
    env.update(extra)
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker"] + (["--refract"] if refract else []), env=env, capture_output=True,
                       text=True, timeout=600)
    if p.returncode != 0:
        raise RuntimeError(f"a measuring process failed ({p.returncode}):\n{p.stdout}\n{p.stderr}")
    return json.loads(next(ln for ln in p.stdout.splitlines() if ln.startswith("REFRACT_COST "))[len("REFRACT_COST "):])


def spread(v):
    return (max(v) - min(v)) / statistics.median(v) * 100.0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("out", nargs="?", default=os.path.join(ROOT, "profiles", "refract_cost.txt"))
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--parent-lib", default=None, help="libvrt.so of the parent commit's build: its water frame is measured beside this build's")
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--refract", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        worker(a.refract)
        return
    legs = {"this build": (True, {})}
    if a.parent_lib:
        legs[PARENT] = (False, {"VRT_LIB": os.path.abspath(a.parent_lib), "VRT_LIB_WITHOUT": "vrt_set_water_refraction"})
    res = {k: [] for k in legs}
    for _ in range(a.runs):
        for k, (refract, extra) in legs.items():
            res[k].append(run(refract, extra))
    lines = ["# tools/refract_cost.py: C4 1920x1080 8^3 4 bounces 1 spp, one device, 2 frames in flight; us per frame: the median of %d processes, "
             "each the median of %d legs of %d frames; (spread: max - min over the processes).  absorb %s, reflectance %s, ior %s, max_span 64"
             % (a.runs, ROUNDS, FRAMES, OPTICS[0], OPTICS[1], IOR)]
    for cam in CAMERAS:
        first = res["this build"][0][cam]
        lines.append(f"{cam}: path segments of a frame (a stats frame's counts): water {sum(first['water_rays'])}, refracting {sum(first['refract_rays'])}")
        med, parts = {}, []
        rows = [("refracting", "this build", "refract"), ("water", "this build", "water")]
        if a.parent_lib:
            rows.append(("water, parent build", PARENT, "water"))
        for label, k, field in rows:
            v = [r[cam][field] for r in res[k]]
            med[label] = statistics.median(v)
            parts.append(f"{label} {med[label]:8.1f} us (spread {spread(v):.2f} %)")
        lines.append(f"{cam}:  " + "   ".join(parts))
        ratios = [r[cam]["refract"] / r[cam]["water"] for r in res["this build"]]   # the same context, the same process
        tail = f"; water / parent's water = {med['water'] / med['water, parent build']:.4f}" if a.parent_lib else "; the parent build was not measured"
        lines.append(f"{cam}:  refracting / water of the same context = {statistics.median(ratios):.4f} (spread {spread(ratios):.2f} %){tail}")
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
