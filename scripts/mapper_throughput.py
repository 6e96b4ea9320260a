#!/usr/bin/env python
"""Throughput of the minimizer index, the anchor matcher, the overlapper and the end rescue on one GPU.

Builds the index of 2,000 synthetic 10 kb reads at (k,w) = (15,10), hashed,
filtering_parameter 0.001, and matches it against itself.  The reads are
substrings of one random 2 Mb genome (10x coverage, every second one reverse
complemented), so the reads share minimizers and the anchor count is bounded
by the coverage.  Prints one JSON line with bases/s for the index, anchors/s
for the matcher and for matching and chaining in one call (default overlapper
parameters) and overlaps/s for the rescue of those overlaps' ends, then checks
a 16-read subset against the plain-Python models (tests/mapper_model.py,
tests/overlapper_model.py, tests/rescue_model.py).

Each GPU step (index, match, overlap, rescue, windows, verify) runs in a child process
of its own under a time limit; a step that fails or runs out of time ends the
run.
The timed calls are gwamd_index_create, gwamd_match_anchors (upload, kernels
and the copy of the anchors to the host) and gwamd_match_overlaps (the same
matching, the overlapper's kernels and the copy of the overlaps; the anchors
stay on the device), timed with device events on the stream the library works
on and with the host clock.  The rescue step times gwamd_rescue_overlap_ends
(upload of the reads and the overlaps, one kernel, one copy back) on the
overlaps of the overlap step, and next to it, once, the same overlaps through
three rounds each of gwamd_extend_overlap_by_sequence_similarity on one host
thread (the loop a caller without the kernel would write; the reverse
complements it needs are made before the clock starts).

The windows step times cudapolish's cut of those overlaps into target windows
of 500 bases, host clock: (i) gwamd_window_segments_resident, which aligns the
overlaps on resident reads and cuts them from the aligner's device paths; (ii)
the route without the kernel: gwamd_align_overlaps_resident (the same
alignments, the paths downloaded and turned into CIGARs) followed by
gwamd_window_segments_host per overlap on one thread, the states expanded from
the CIGARs before the clock starts.  It compares the two record for record.

    python scripts/mapper_throughput.py [--reads 2000] [--length 10000] [--steps 5] [--warmup 2]
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

K, W, FILTERING = 15, 10, 0.001
STEP_TIMEOUT = {"index": 300, "match": 300, "overlap": 300, "rescue": 300, "windows": 900, "verify": 300}
WINDOW_LENGTH = 500  # racon's default
RESCUE_EXTENSION, RESCUE_SIMILARITY, RESCUE_ROUNDS = 100, 0.9, 3  # what the reference's rescue_overlap_ends runs with


def synthetic_reads(num_reads, length, seed=1):
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


def pack(reads):
    offsets = (C.c_int64 * (len(reads) + 1))()
    for i, r in enumerate(reads):
        offsets[i + 1] = offsets[i] + len(r)
    return b"".join(reads), offsets


class Timer:
    """Device-event and host-clock time of one synchronous library call."""

    def __init__(self):
        import torch
        self.torch = torch
        torch.cuda.init()

    def run(self, fn):
        torch = self.torch
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        start.record(torch.cuda.default_stream())
        fn()
        stop.record(torch.cuda.default_stream())
        stop.synchronize()
        return start.elapsed_time(stop) * 1e-3, time.perf_counter() - t0


def create_index(L, bases, offsets, n):
    h = C.c_void_p()
    rc = L.gwamd_index_create(bases, offsets, n, 0, n, K, W, 1, FILTERING, 0, C.byref(h))
    if rc != 0:
        raise RuntimeError(L.gwamd_last_error().decode())
    return h


def reference_reverse_complement(read):
    """The reverse complement the reference's rescue makes (overlapper.cpp:94-109): A<->T, C<->G,
    the middle base of an odd length left as it is."""
    table = np.arange(256, dtype=np.uint8)
    table[list(b"ACGT")] = list(b"TGCA")
    codes = np.frombuffer(read, np.uint8)
    out = table[codes[::-1]]
    if len(read) % 2:
        out[len(read) // 2] = codes[len(read) // 2]
    return out.tobytes()


def host_rescue(L, reads, overlaps, n):
    """The first n of the overlaps (a ctypes array) through RESCUE_ROUNDS host rounds each, on
    this thread: the rescued array and the seconds the rounds took."""
    from claragenomicsanalysis_amd.cudamapper import Overlap
    out = (Overlap * max(n, 1))()
    C.memmove(out, overlaps, C.sizeof(Overlap) * n)
    reverse = {out[i].target_read_id: None for i in range(n) if out[i].strand == "-"}
    for read_id in reverse:
        reverse[read_id] = reference_reverse_complement(reads[read_id])
    extend = L.gwamd_extend_overlap_by_sequence_similarity
    t0 = time.perf_counter()
    for i in range(n):
        o = out[i]  # a view of the array's element
        query, target = reads[o.query_read_id], reads[o.target_read_id]
        flip = o.strand == "-"
        if flip:
            target = reverse[o.target_read_id]
            o.target_start, o.target_end = len(target) - o.target_end, len(target) - o.target_start
        for _ in range(RESCUE_ROUNDS):
            if extend(C.byref(o), query, len(query), target, len(target), RESCUE_EXTENSION, RESCUE_SIMILARITY) != 0:
                raise RuntimeError(L.gwamd_last_error().decode())
        if flip:
            o.target_start, o.target_end = len(target) - o.target_end, len(target) - o.target_start
    return out, time.perf_counter() - t0


def states_of_cigars(cigars):
    """The states (start -> end) the CIGARs stand for, concatenated, and their n + 1 offsets:
    M is taken as match (the cut does not tell match from mismatch), I as 2, D as 3."""
    import re
    token = re.compile(r"(\d+)([MID])")
    code = {"M": 0, "I": 2, "D": 3}
    offsets = np.zeros(len(cigars) + 1, np.int64)
    parts = []
    for i, c in enumerate(cigars):
        runs = token.findall(c)
        counts = np.array([int(r[0]) for r in runs], np.int64)
        parts.append(np.repeat(np.array([code[r[1]] for r in runs], np.int8), counts))
        offsets[i + 1] = offsets[i] + int(counts.sum())
    return (np.concatenate(parts) if parts else np.zeros(0, np.int8)), offsets


def windows_step(L, args, bases, offsets, num_reads):
    from claragenomicsanalysis_amd.cudamapper import Overlap, _take
    from claragenomicsanalysis_amd.cudapolish import SEGMENT_DTYPE
    h = create_index(L, bases, offsets, num_reads)
    found, n = C.c_void_p(), C.c_int64()
    if L.gwamd_match_overlaps(h, h, -1, 20, 50, 50, 0.9, C.byref(found), C.byref(n), None) != 0:
        raise RuntimeError(L.gwamd_last_error().decode())
    L.gwamd_index_free(h)
    overlaps = (Overlap * max(n.value, 1))()
    C.memmove(overlaps, found, C.sizeof(Overlap) * n.value)
    L.gwamd_overlaps_free(found)
    reads = C.c_void_p()
    if L.gwamd_device_reads_create(bases, offsets, num_reads, 0, None, C.byref(reads)) != 0:
        raise RuntimeError(L.gwamd_last_error().decode())

    def check(rc):
        if rc != 0:
            raise RuntimeError(L.gwamd_last_error().decode())

    def records(p, count):
        out = np.empty(count, SEGMENT_DTYPE)
        if count:
            C.memmove(out.ctypes.data, p, count * SEGMENT_DTYPE.itemsize)
        return out

    resident_s, align_s, host_s = [], [], []
    on_gpu = by_host = cigars = None
    for step in range(args.warmup + args.steps):
        p, m = C.c_void_p(), C.c_int64()
        t0 = time.perf_counter()
        check(L.gwamd_window_segments_resident(reads, reads, overlaps, n.value, WINDOW_LENGTH, 1, C.byref(p),
                                               C.byref(m)))
        resident_s.append(time.perf_counter() - t0)
        on_gpu = records(p, m.value)
        L.gwamd_window_segments_free(p)
    for step in range(args.warmup + args.steps):
        texts = C.c_void_p()
        t0 = time.perf_counter()
        check(L.gwamd_align_overlaps_resident(reads, reads, overlaps, n.value, 1, C.byref(texts)))
        align_s.append(time.perf_counter() - t0)
        if step + 1 < args.warmup + args.steps:
            L.gwamd_text_list_free(texts)
        else:
            cigars = _take(L, texts)
    L.gwamd_device_reads_free(reads)
    states, state_offsets = states_of_cigars(cigars)
    address = states.ctypes.data
    host = L.gwamd_window_segments_host
    for step in range(args.warmup + args.steps):
        held = []
        t0 = time.perf_counter()
        for i in range(n.value):
            p, m = C.c_void_p(), C.c_int64()
            if host(C.byref(overlaps[i]), address + int(state_offsets[i]),
                    int(state_offsets[i + 1] - state_offsets[i]), WINDOW_LENGTH, i, C.byref(p), C.byref(m)) != 0:
                raise RuntimeError(L.gwamd_last_error().decode())
            held.append((p, m.value))
        host_s.append(time.perf_counter() - t0)
        by_host = np.concatenate([records(p, count) for p, count in held]) if held else np.zeros(0, SEGMENT_DTYPE)
        for p, _ in held:
            L.gwamd_window_segments_free(p)
    if on_gpu.tobytes() != by_host.tobytes():
        raise RuntimeError("the cut on the GPU and the host walk differ")
    flagged = int(np.count_nonzero(on_gpu["flags"] & 12))
    med = lambda v: float(np.median(v[args.warmup:]))
    print(json.dumps({"windows_overlaps": n.value, "windows_records": len(on_gpu), "windows_flagged_records": flagged,
                      "windows_path_states": int(state_offsets[-1]), "windows_resident_s": round(med(resident_s), 6),
                      "windows_align_download_s": round(med(align_s), 6),
                      "windows_host_cut_s": round(med(host_s), 6),
                      "windows_host_route_s": round(med(align_s) + med(host_s), 6)}))


def overlap_fields(o):
    return (o.query_read_id, o.target_read_id, o.query_start, o.query_end, o.target_start, o.target_end, o.strand,
            o.num_residues, bool(o.overlap_complete))


def worker(args):
    import torch  # noqa: F401  (before libgwamd, so that both share one HIP runtime)
    from claragenomicsanalysis_amd import load_library
    from claragenomicsanalysis_amd.cudamapper import IndexInfo
    L = load_library()
    reads = synthetic_reads(args.reads, args.length)
    if args.worker == "verify":
        import mapper_model as model
        import overlapper_model
        import rescue_model
        from claragenomicsanalysis_amd import Index, match_anchors, match_overlaps, rescue_overlap_ends
        from claragenomicsanalysis_amd.cudamapper import _overlap_array
        subset = reads[:16]
        expected = model.Index(subset, K, W, filtering_parameter=FILTERING)
        with Index(subset, K, W, filtering_parameter=FILTERING) as idx:
            for name in ("representations", "read_ids", "positions_in_reads", "directions_of_reads",
                         "unique_representations", "first_occurrence_of_representations"):
                assert getattr(idx, name).tolist() == getattr(expected, name), name
            anchors = match_anchors(idx, idx)
            overlaps = match_overlaps(idx, idx)
        want = model.match_anchors(expected, expected)
        assert [tuple(int(x) for x in a) for a in anchors] == want
        want_overlaps, counts = overlapper_model.get_overlaps(want)
        assert [overlap_fields(o) for o in overlaps] == want_overlaps
        # the rescue on the GPU, the host rounds and the model agree on every field
        rescued = [overlap_fields(o) for o in rescue_overlap_ends(overlaps, subset, subset)]
        by_host, _ = host_rescue(L, subset, _overlap_array(overlaps), len(overlaps))
        assert rescued == [overlap_fields(by_host[i]) for i in range(len(overlaps))]
        assert rescued == rescue_model.rescue_overlap_ends(want_overlaps, subset, subset)
        print(json.dumps({"verified_reads": len(subset), "verified_elements": len(expected.representations),
                          "verified_anchors": len(want), "verified_chains": counts["chains"],
                          "verified_overlaps": len(want_overlaps),
                          "verified_rescued_ends": sum((a[2] != b[2]) + (a[3] != b[3])
                                                       for a, b in zip(rescued, want_overlaps))}))
        return
    bases, offsets = pack(reads)
    timer = Timer()
    info = IndexInfo()
    if args.worker == "index":
        samples = []
        for step in range(args.warmup + args.steps):
            holder = []
            ev, wall = timer.run(lambda: holder.append(create_index(L, bases, offsets, len(reads))))
            L.gwamd_index_info(holder[0], C.byref(info))
            L.gwamd_index_free(holder[0])
            if step >= args.warmup:
                samples.append((ev, wall))
        ev = float(np.median([s[0] for s in samples]))
        wall = float(np.median([s[1] for s in samples]))
        print(json.dumps({"bases": len(bases), "elements": info.num_elements,
                          "unique_representations": info.num_unique_representations,
                          "index_event_s": round(ev, 6), "index_wall_s": round(wall, 6),
                          "index_bases_per_s": round(len(bases) / ev, 1)}))
    elif args.worker == "overlap":
        h = create_index(L, bases, offsets, len(reads))
        samples, n, anchors = [], C.c_int64(), C.c_int64()
        for step in range(args.warmup + args.steps):
            p = C.c_void_p()

            def call():
                rc = L.gwamd_match_overlaps(h, h, -1, 20, 50, 50, 0.9, C.byref(p), C.byref(n), C.byref(anchors))
                if rc != 0:
                    raise RuntimeError(L.gwamd_last_error().decode())
            ev, wall = timer.run(call)
            L.gwamd_overlaps_free(p)
            if step >= args.warmup:
                samples.append((ev, wall))
        L.gwamd_index_free(h)
        ev = float(np.median([s[0] for s in samples]))
        wall = float(np.median([s[1] for s in samples]))
        print(json.dumps({"overlaps": n.value, "overlap_anchors": anchors.value, "overlap_event_s": round(ev, 6),
                          "overlap_wall_s": round(wall, 6), "overlap_anchors_per_s": round(anchors.value / ev, 1)}))
    elif args.worker == "windows":
        windows_step(L, args, bases, offsets, len(reads))
    elif args.worker == "rescue":
        from claragenomicsanalysis_amd.cudamapper import Overlap
        h = create_index(L, bases, offsets, len(reads))
        found, n = C.c_void_p(), C.c_int64()
        if L.gwamd_match_overlaps(h, h, -1, 20, 50, 50, 0.9, C.byref(found), C.byref(n), None) != 0:
            raise RuntimeError(L.gwamd_last_error().decode())
        L.gwamd_index_free(h)
        overlaps = (Overlap * max(n.value, 1))()
        C.memmove(overlaps, found, C.sizeof(Overlap) * n.value)
        L.gwamd_overlaps_free(found)
        samples, rescued, last = [], C.c_int64(), None
        for step in range(args.warmup + args.steps):
            p = C.c_void_p()

            def call():
                rc = L.gwamd_rescue_overlap_ends(bases, offsets, len(reads), bases, offsets, len(reads), overlaps,
                                                 n.value, RESCUE_EXTENSION, RESCUE_SIMILARITY, 0, C.byref(p),
                                                 C.byref(rescued))
                if rc != 0:
                    raise RuntimeError(L.gwamd_last_error().decode())
            ev, wall = timer.run(call)
            if last:
                L.gwamd_overlaps_free(last)
            last = p
            if step >= args.warmup:
                samples.append((ev, wall))
        ev = float(np.median([s[0] for s in samples]))
        wall = float(np.median([s[1] for s in samples]))
        by_host, host_s = host_rescue(L, reads, overlaps, n.value)
        on_gpu = (Overlap * n.value).from_address(last.value) if n.value else []
        same = all(overlap_fields(on_gpu[i]) == overlap_fields(by_host[i]) for i in range(n.value))
        moved = sum((on_gpu[i].query_start != overlaps[i].query_start) +
                    (on_gpu[i].query_end != overlaps[i].query_end) for i in range(n.value))
        L.gwamd_overlaps_free(last)
        if not same:
            raise RuntimeError("the rescue on the GPU and the host rounds differ")
        print(json.dumps({"rescue_overlaps": n.value, "rescue_ends_moved": moved, "rescue_event_s": round(ev, 6),
                          "rescue_wall_s": round(wall, 6), "rescue_overlaps_per_s": round(n.value / wall, 1),
                          "rescue_host_rounds_s": round(host_s, 6)}))
    else:
        h = create_index(L, bases, offsets, len(reads))
        samples, n = [], C.c_int64()
        for step in range(args.warmup + args.steps):
            p = C.c_void_p()

            def call():
                rc = L.gwamd_match_anchors(h, h, -1, C.byref(p), C.byref(n))
                if rc != 0:
                    raise RuntimeError(L.gwamd_last_error().decode())
            ev, wall = timer.run(call)
            L.gwamd_anchors_free(p)
            if step >= args.warmup:
                samples.append((ev, wall))
        L.gwamd_index_free(h)
        ev = float(np.median([s[0] for s in samples]))
        wall = float(np.median([s[1] for s in samples]))
        print(json.dumps({"anchors": n.value, "match_event_s": round(ev, 6), "match_wall_s": round(wall, 6),
                          "match_anchors_per_s": round(n.value / ev, 1)}))


def main():
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--reads", type=int, default=2000)
    p.add_argument("--length", type=int, default=10000)
    p.add_argument("--steps", type=int, default=5)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--no-verify", action="store_true")
    p.add_argument("--worker", choices=sorted(STEP_TIMEOUT), default=None, help=argparse.SUPPRESS)
    args = p.parse_args()
    if args.worker:
        worker(args)
        return 0
    result = {"metric": "mapper_throughput", "reads": args.reads, "read_length": args.length, "kmer_size": K,
              "window_size": W, "hash_representations": True, "filtering_parameter": FILTERING,
              "steps": args.steps, "warmup": args.warmup}
    for step in ("index", "match", "overlap", "rescue", "windows") + (() if args.no_verify else ("verify",)):
        cmd = [sys.executable, os.path.abspath(__file__), "--worker", step, "--reads", str(args.reads), "--length",
               str(args.length), "--steps", str(args.steps), "--warmup", str(args.warmup)]
        try:
            out = subprocess.run(cmd, timeout=STEP_TIMEOUT[step], stdout=subprocess.PIPE, check=True).stdout
        except (subprocess.TimeoutExpired, subprocess.CalledProcessError) as e:
            sys.stderr.write("mapper_throughput: step %s failed: %s\n" % (step, e))
            return 1  # nothing more is started on the GPU
        result.update(json.loads(out.decode().strip().splitlines()[-1]))
    print(json.dumps(result))
    return 0


if __name__ == "__main__":
    sys.exit(main())
