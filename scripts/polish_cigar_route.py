#!/usr/bin/env python3
"""Wall time of cudapolish's window cut for overlaps that already carry CIGARs,
on the routes a caller has:

  cigar_text  window_segments_cigar from text CIGARs: the parse to packed ops
              (cigar_ops per CIGAR) is inside the clock
  cigar_ops   the same from packed ops: gwamd_window_segments_cigar alone
  expand      every run written out as states on the host (numpy, inside the
              clock), then gwamd_window_segments on the states
  resident    gwamd_window_segments_resident: the overlaps aligned again

Workloads, both from scripts/mapper_throughput.py's reads (--reads error-free
reads of --read-length bases from one genome, every second one
reverse-complemented) and its mapper settings, w = 500:

  clean  the reads against themselves: one or two runs per CIGAR
  noisy  a copy of the reads with about --error-rate errors per base (a third
         each substitutions, insertions and deletions) as queries against the
         error-free reads as targets: thousands of runs per CIGAR

The overlaps, their ctypes array and the CIGARs (one gwamd_align_overlaps_resident)
are made before the clock starts, in every process.  The parent first runs a
check process per workload (all four routes return the same bytes), then
--rounds rounds of one process per route, interleaved; a process does --warmup
warm-ups and --runs timed repetitions and reports their median.  Printed per
route: the median and the range of the process medians.

  python scripts/polish_cigar_route.py                   # both workloads
  python scripts/polish_cigar_route.py --worker cigar_ops --workload clean --runs 3
      # one process, e.g. under rocprofv3 --kernel-trace --stats for the kernel's own time
"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

K, W, FILTERING = 15, 10, 0.001  # scripts/mapper_throughput.py
WINDOW_LENGTH = 500
ROUTES = ("cigar_text", "cigar_ops", "expand", "resident")


def synthetic_reads(num_reads, length, seed=1):
    """scripts/mapper_throughput.py's reads."""
    rng = np.random.default_rng(seed)
    genome_length = max(num_reads * length // 10, 2 * length)
    letters = np.frombuffer(b"ACGT", np.uint8)
    genome = rng.integers(0, 4, genome_length, dtype=np.uint8)
    starts = rng.integers(0, genome_length - length, num_reads)
    reads = []
    for i, s in enumerate(starts):
        codes = genome[s:s + length]
        if i % 2:
            codes = 3 - codes[::-1]
        reads.append(letters[codes].tobytes())
    return reads


def with_errors(reads, rate, seed=2):
    rng = np.random.default_rng(seed)
    letters = np.frombuffer(b"ACGT", np.uint8)
    out = []
    for read in reads:
        bases = np.frombuffer(read, np.uint8)
        kind = rng.random(len(bases))
        other = letters[rng.integers(0, 4, len(bases))]
        substituted = np.where(kind < rate / 3, other, bases)
        keep = ~((kind >= rate / 3) & (kind < 2 * rate / 3))                     # deletions
        repeat = np.where((kind >= 2 * rate / 3) & (kind < rate), 2, 1) * keep  # insertions: the base twice
        out.append(np.repeat(substituted, repeat).tobytes())
    return out


def make_workload(args):
    """(overlaps as a ctypes array, n, CIGAR texts, the two DeviceReads)."""
    from claragenomicsanalysis_amd import cudamapper
    targets = synthetic_reads(args.reads, args.read_length)
    queries = with_errors(targets, args.error_rate) if args.workload == "noisy" else targets
    with cudamapper.Index(targets, K, W, filtering_parameter=FILTERING) as ti:
        if args.workload == "noisy":
            with cudamapper.Index(queries, K, W, filtering_parameter=FILTERING) as qi:
                overlaps = cudamapper.match_overlaps(qi, ti)
        else:
            overlaps = cudamapper.match_overlaps(ti, ti)
    q = cudamapper.DeviceReads(queries)
    t = cudamapper.DeviceReads(targets)
    cigars = cudamapper.align_overlaps(overlaps, q, t)
    return cudamapper._overlap_array(overlaps), len(overlaps), cigars, q, t


def states_of(ops, offsets):
    """Every run written out: the states and their n + 1 offsets (numpy; M as match)."""
    ops = ops[:offsets[-1]]
    lengths = (ops >> 4).astype(np.int64)
    code = np.array([0, 2, 3, 0, 0, 0, 0, 0, 1] + [0] * 7, np.int8)[ops & 15]
    states = np.repeat(code, lengths)
    ends = np.concatenate([[0], np.cumsum(lengths)])
    return states, np.ascontiguousarray(ends[offsets])


def worker(args):
    from claragenomicsanalysis_amd import cudapolish, load_library
    L = load_library()
    arr, n, cigars, q, t = make_workload(args)
    ops, offsets = cudapolish._pack_cigars(cigars)

    def check(rc):
        if rc != 0:
            raise RuntimeError(L.gwamd_last_error().decode())

    def take(p, m):
        out = np.empty(m.value, cudapolish.SEGMENT_DTYPE)
        if m.value:
            C.memmove(out.ctypes.data, p, m.value * cudapolish.SEGMENT_DTYPE.itemsize)
        L.gwamd_window_segments_free(p)
        return out

    def cut_ops(ops, offsets):
        p, m = C.c_void_p(), C.c_int64()
        check(L.gwamd_window_segments_cigar(arr, n, ops.ctypes.data_as(C.c_void_p), offsets.ctypes.data_as(C.c_void_p),
                                            0, WINDOW_LENGTH, 0, None, C.byref(p), C.byref(m)))
        return take(p, m)

    def cigar_text():
        return cut_ops(*cudapolish._pack_cigars(cigars))

    def cigar_ops():
        return cut_ops(ops, offsets)

    def expand():
        states, state_offsets = states_of(ops, offsets)
        p, m = C.c_void_p(), C.c_int64()
        check(L.gwamd_window_segments(arr, n, states.ctypes.data_as(C.c_void_p),
                                      state_offsets.ctypes.data_as(C.c_void_p), WINDOW_LENGTH, 0, None, C.byref(p),
                                      C.byref(m)))
        return take(p, m)

    def resident():
        p, m = C.c_void_p(), C.c_int64()
        check(L.gwamd_window_segments_resident(q._handle, t._handle, arr, n, WINDOW_LENGTH, 1, C.byref(p), C.byref(m)))
        return take(p, m)

    routes = {"cigar_text": cigar_text, "cigar_ops": cigar_ops, "expand": expand, "resident": resident}
    shape = {"workload": args.workload, "overlaps": n, "ops": int(offsets[-1]),
             "states": int((ops[:offsets[-1]] >> 4).sum())}
    if args.worker == "check":
        results = {name: fn().tobytes() for name, fn in routes.items()}
        equal = len(set(results.values())) == 1
        records = np.frombuffer(results["cigar_ops"], cudapolish.SEGMENT_DTYPE)
        print(json.dumps(dict(shape, route="check", equal=equal, records=len(records),
                              flagged=int(np.count_nonzero(records["flags"] & 12)))))
        return 0 if equal else 1
    route = routes[args.worker]
    times = []
    for i in range(args.warmup + args.runs):
        start = time.perf_counter()
        route()
        times.append(time.perf_counter() - start)
    print(json.dumps(dict(shape, route=args.worker, ms=[round(1e3 * s, 3) for s in times[args.warmup:]])))
    return 0


def parent(args):
    def child(route, workload):
        cmd = [sys.executable, os.path.abspath(__file__), "--worker", route, "--workload", workload]
        for name in ("reads", "read_length", "error_rate", "warmup", "runs"):
            cmd += ["--" + name.replace("_", "-"), str(getattr(args, name))]
        out = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        if out.returncode != 0:
            raise RuntimeError(out.stdout + out.stderr)
        return json.loads(out.stdout.strip().splitlines()[-1])

    for workload in args.workloads.split(","):
        print(json.dumps(child("check", workload)), flush=True)
        samples = {route: [] for route in ROUTES}
        for _ in range(args.rounds):
            for route in ROUTES:
                samples[route].append(statistics.median(child(route, workload)["ms"]))
        for route in ROUTES:
            v = samples[route]
            print(json.dumps({"workload": workload, "route": route, "median_ms": round(statistics.median(v), 3),
                              "min_ms": min(v), "max_ms": max(v), "per_process_medians_ms": v}), flush=True)
    return 0


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--worker", choices=ROUTES + ("check",), help="one process of one route")
    p.add_argument("--workload", choices=["clean", "noisy"], default="clean")
    p.add_argument("--workloads", default="clean,noisy")
    p.add_argument("--rounds", type=int, default=3)
    p.add_argument("--reads", type=int, default=2000)
    p.add_argument("--read-length", type=int, default=10000)
    p.add_argument("--error-rate", type=float, default=0.10)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--runs", type=int, default=5)
    args = p.parse_args()
    return worker(args) if args.worker else parent(args)


if __name__ == "__main__":
    sys.exit(main())
