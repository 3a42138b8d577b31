"""What the path trace's denoiser (vrt_set_denoise, include/vrt.h) costs a frame: C4 (1920x1080, 8^3 chunks, 4-bounce diffuse
path trace, 1 spp) with denoising off and with 1..5 passes, per-frame microseconds with 1 and 2 frames in flight; the guide
launch and every pass by themselves, from a kernel trace; and the off figure against another build of the library (the parent
commit's), with that build's own run-to-run spread.

    python tools/denoise_cost.py [out.txt] [--parent-lib libvrt_parent.so] [--kernel-stats kernel_stats.csv]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python3 tools/denoise_cost.py --trace-leg     (a run of its own)
    python tools/denoise_cost.py --off-only                                    (one process' off figures, for --parent-lib)

A leg is `frames` back-to-back frames between two synchronisations (the period a game loop sees); the settings alternate leg by
leg and each figure is the median over the rounds.  --parent-lib: the off legs again in fresh child processes, this build and
the other one in turn (VRT_LIB), five of each: the other build's spread is what "no slower with denoising off" is held to — a
median above the other build's slowest run ends the tool with an error, after the report is written.
--kernel-stats: a `rocprofv3 --kernel-trace --stats` CSV of the --trace-leg run (5 passes, one frame at a time), folded into the
report — a pass moves the frame once in and once out (2 x 33.2 MB at 1080p) plus the guide words, so its bytes over its time say
how far it is from a plain copy.  Writes profiles/denoise_cost.txt (or the path given first) and prints it."""
import csv
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from voxelraytracing_amd import Gpu, MODE_PATH, scenes  # noqa: E402

FRAMES, ROUNDS, WARM = 300, 5, 60


def c4_gpu():
    sc = scenes.c4()
    gpu = Gpu(sc.world.max_nodes(), sc.world.size_in_chunks(), sc.size, device=0)
    gpu.upload_world(sc.world, sc.materials)
    gpu.write_cam_data(sc.cam)
    gpu.write_settings(sc.settings)
    return gpu


def leg(gpu, passes, frames, denoise=True):
    if denoise:
        gpu.set_denoise(passes, 0.0)
    gpu.synchronize()
    t0 = time.perf_counter()
    for _ in range(frames):
        gpu.render(MODE_PATH, spp=1, seed=1)
    gpu.synchronize()
    return (time.perf_counter() - t0) / frames * 1e6


def off_only():
    """This process' library (VRT_LIB or the tree's), denoising never touched: 'in_flight median' per line."""
    gpu = c4_gpu()
    for in_flight in (1, 2):
        gpu.set_frames_in_flight(in_flight)
        leg(gpu, 0, WARM, denoise=False)
        print(in_flight, statistics.median(leg(gpu, 0, FRAMES, denoise=False) for _ in range(ROUNDS)))
    gpu.close()


def trace_leg():
    gpu = c4_gpu()
    gpu.set_frames_in_flight(1)
    leg(gpu, 5, 20)
    leg(gpu, 5, 100)
    gpu.close()


def against_parent(parent_lib, runs=5):
    res = {"this": {1: [], 2: []}, "parent": {1: [], 2: []}}
    for _ in range(runs):
        for name, lib in (("parent", parent_lib), ("this", None)):
            env = dict(os.environ)
            env.pop("VRT_LIB", None)
            env.pop("VRT_LIB_WITHOUT", None)
            if lib:   # (a build from before the denoiser has no such entry points: _ffi._load lets exactly these be absent)
                env["VRT_LIB"] = os.path.abspath(lib)
                env["VRT_LIB_WITHOUT"] = "vrt_set_denoise,vrt_read_guide"
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--off-only"], env=env, check=True, capture_output=True,
                                 text=True, timeout=300).stdout
            for line in out.splitlines():
                k, v = line.split()
                res[name][int(k)].append(float(v))
    lines, slower = [], False
    for in_flight in (1, 2):
        p, t = res["parent"][in_flight], res["this"][in_flight]
        where = "ABOVE" if statistics.median(t) > max(p) else ("below" if statistics.median(t) < min(p) else "inside")
        slower = slower or where == "ABOVE"
        lines.append(f"off against the parent build, {in_flight} in flight ({runs} fresh processes each, in turn):  parent {statistics.median(p):7.1f} us/frame "
                     f"(spread {min(p):.1f}..{max(p):.1f})   this build {statistics.median(t):7.1f} us/frame ({min(t):.1f}..{max(t):.1f})   "
                     f"{(statistics.median(t) / statistics.median(p) - 1.0) * 100.0:+5.2f} %   median {where} the parent's spread")
    return lines, slower


def kernel_lines(path, width=1920, height=1080):
    frame_mb = width * height * 16 / 1e6
    lines = [f"kernel trace of the 5-pass frame, one at a time (rocprofv3 --kernel-trace --stats, a run of its own); a pass reads and writes the "
             f"frame once, 2 x {frame_mb:.1f} MB, and reads the guide words, {width * height * 4 / 1e6:.1f} MB:"]
    for row in csv.DictReader(open(path)):
        name = row["Name"]
        if "denoise" not in name and "path_" not in name:
            continue
        avg_us = float(row["AverageNs"]) / 1e3
        note = ""
        if "denoise_pass" in name:
            note = f"   {(2 * frame_mb + width * height * 4 / 1e6) / avg_us:6.2f} TB/s effective"
        lines.append(f"  {name[:110]:110s} {int(row['Calls']):6d} calls  {avg_us:9.1f} us each{note}")
    return lines


def main():
    args = sys.argv[1:]
    if "--off-only" in args:
        return off_only()
    if "--trace-leg" in args:
        return trace_leg()
    parent = args[args.index("--parent-lib") + 1] if "--parent-lib" in args else None
    stats = args[args.index("--kernel-stats") + 1] if "--kernel-stats" in args else None
    out = args[0] if args and not args[0].startswith("--") else os.path.join(ROOT, "profiles", "denoise_cost.txt")
    lines = ["# tools/denoise_cost.py: vrt_set_denoise on C4 (1920x1080, 8^3 chunks, 4 bounces, 1 spp), one device; sigma_color 0"]
    gpu = c4_gpu()
    for in_flight in (1, 2):
        gpu.set_frames_in_flight(in_flight)
        us = {p: [] for p in range(6)}
        for p in us:
            leg(gpu, p, WARM)
        for _ in range(ROUNDS):
            for p in us:
                us[p].append(leg(gpu, p, FRAMES))
        off = statistics.median(us[0])
        for p in us:
            m = statistics.median(us[p])
            lines.append(f"C4  {in_flight} in flight  passes {p}:  {m:8.1f} us/frame   {m - off:+8.1f} us  {(m / off - 1.0) * 100.0:+7.2f} %   "
                         f"(median of {ROUNDS} legs of {FRAMES} frames, {min(us[p]):.1f}..{max(us[p]):.1f})")
    gpu.close()
    slower = False
    if parent:
        more, slower = against_parent(parent)
        lines += more
    if stats:
        lines += kernel_lines(stats)
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write(text)
    print(text, end="")
    if slower:   # "off" must cost what the parent costs: the report is written, and the run fails
        sys.exit("denoising off is slower than the parent build's slowest run")


if __name__ == "__main__":
    main()
