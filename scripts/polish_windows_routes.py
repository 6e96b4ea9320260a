#!/usr/bin/env python3
"""Wall time of cudapolish's step from window segments in hand to the POA
batch's input on the device, on its two routes:

  host    build_windows (bases copied out of the host strings), add_poa_group
          per window, upload (bases and all-ones weights sent up)
  device  build_window_slices, add_poa_group_resident per window, upload (the
          gather kernel fills bases and weights from the resident reads)

Each timed repetition ends with a synchronise of the batch's stream, so the
copies and the gather are inside it; the POA itself is not run.  The reads are
resident before the clock starts on both routes (the aligner needed them
there).  Workload: one target, error-free reads of it at random positions,
every second one reverse-complemented, and the segments such reads cut into
windows, computed here without the aligner.

  python scripts/polish_windows_routes.py --route device
  python scripts/polish_windows_routes.py --compare OTHER_TREE

--compare runs, interleaved and each in a process of its own, the host route
of another checkout of this project (built, for example the parent commit),
this tree's host route and this tree's device route, --rounds times, and
prints each one's median and range.  On this tree it first checks that both
routes leave the same bytes in the batch.
"""
import argparse
import json
import os
import random
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_COMPLEMENT = str.maketrans("ACGT", "TGCA")


def make_job(seed, target_length, num_reads, read_length, w):
    rng = random.Random(seed)
    target = "".join(rng.choice("ACGT") for _ in range(target_length))
    reads, overlaps, segments = [], [], []
    for i in range(num_reads):
        ts = rng.randint(0, target_length - read_length)
        te = ts + read_length
        reverse = i % 2 == 1
        piece = target[ts:te]
        reads.append(piece[::-1].translate(_COMPLEMENT) if reverse else piece)
        overlaps.append((i, 0, 0, read_length, ts, te, "-" if reverse else "+"))
        for k in range(ts // w, (te - 1) // w + 1):
            a, b = max(ts, k * w), min(te, (k + 1) * w)
            q = (te - b, te - a) if reverse else (a - ts, b - ts)
            segments.append((i, k, q[0], q[1], a, b, 1 if reverse else 0, 0))
    return [target], reads, overlaps, segments


def measure(args):
    sys.path.insert(0, args.tree)
    import numpy as np
    from claragenomicsanalysis_amd import cudapolish
    from claragenomicsanalysis_amd.cudamapper import DeviceReads
    from claragenomicsanalysis_amd.cudapoa import CudaPoaBatch

    targets, reads, overlaps, segments = make_job(args.seed, args.target_length, args.reads, args.read_length,
                                                  args.window_length)
    segments = np.array(segments, dtype=cudapolish.SEGMENT_DTYPE)
    cap = 100
    batch = CudaPoaBatch(cap, (args.window_length + 1 + 63) // 64 * 64, args.mem, cuda_banded_alignment=True)
    resident = [DeviceReads(targets), DeviceReads(reads)]

    def host():
        windows, _ = cudapolish.build_windows(targets, reads, overlaps, segments, args.window_length, cap)
        for w in windows:
            if batch.add_poa_group(w["sequences"])[0] != 0:
                raise RuntimeError("the batch is too small for the job")
        return len(windows)

    def device():
        windows, _, _ = cudapolish.build_window_slices(targets, reads, overlaps, segments, args.window_length, cap)
        for w in windows:
            if batch.add_poa_group_resident(resident, w["slices"])[0] != 0:
                raise RuntimeError("the batch is too small for the job")
        return len(windows)

    def once(route):
        batch.reset()
        start = time.perf_counter()
        windows = route()
        batch.upload()
        batch.synchronize()
        return time.perf_counter() - start, windows

    if args.route == "check":  # both routes leave the same bytes
        once(host)
        a = batch._download_inputs()
        once(device)
        b = batch._download_inputs()
        print(json.dumps({"route": "check", "equal": a == b, "bytes": len(a[0])}))
        return 0 if a == b else 1
    route = {"host": host, "device": device}[args.route]
    for _ in range(args.warmup):
        once(route)
    times = []
    for _ in range(args.runs):
        seconds, windows = once(route)
        times.append(seconds)
    print(json.dumps({"route": args.route, "tree": args.tree, "windows": windows, "reads": args.reads,
                      "ms": [round(1e3 * t, 3) for t in times]}))
    return 0


def compare(args):
    def child(tree, route):
        cmd = [sys.executable, os.path.abspath(__file__), "--tree", tree, "--route", route]
        for name in ("seed", "target_length", "reads", "read_length", "window_length", "mem", "warmup", "runs"):
            cmd += ["--" + name.replace("_", "-"), str(getattr(args, name))]
        out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        if out.returncode != 0:
            raise RuntimeError(out.stdout + out.stderr)
        return json.loads(out.stdout.strip().splitlines()[-1])

    print(json.dumps(child(ROOT, "check")))
    other = os.path.abspath(args.compare)
    arms = [("other tree, host route", other, "host"), ("this tree, host route", ROOT, "host"),
            ("this tree, device route", ROOT, "device")]
    samples = {name: [] for name, _, _ in arms}
    for _ in range(args.rounds):
        for name, tree, route in arms:
            samples[name].append(statistics.median(child(tree, route)["ms"]))
    for name, _, _ in arms:
        v = samples[name]
        print(json.dumps({"arm": name, "median_ms": round(statistics.median(v), 3), "min_ms": min(v),
                          "max_ms": max(v), "per_process_medians_ms": v}))
    return 0


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--route", choices=["host", "device", "check"], default="device")
    p.add_argument("--tree", default=ROOT, help="the checkout whose package is measured")
    p.add_argument("--compare", metavar="OTHER_TREE", help="interleave another built checkout's host route")
    p.add_argument("--rounds", type=int, default=3)
    p.add_argument("--seed", type=int, default=1)
    p.add_argument("--target-length", type=int, default=100000)
    p.add_argument("--reads", type=int, default=300)
    p.add_argument("--read-length", type=int, default=10000)
    p.add_argument("--window-length", type=int, default=500)
    p.add_argument("--mem", type=int, default=4 << 30)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--runs", type=int, default=7)
    args = p.parse_args()
    return compare(args) if args.compare else measure(args)


if __name__ == "__main__":
    sys.exit(main())
