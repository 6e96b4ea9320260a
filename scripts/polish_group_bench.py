"""What cudapolish's window grouping costs, host against device ("Window
grouping on the device").

Part one groups one synthetic job of --records records with base qualities:
reads of about 10 kb, window length 500, cap 100, all from --seed.  Three
figures, each one warm-up and --repeats timed runs through the C ABI, without
any conversion to Python objects:

  host             gwamd_build_window_slices (one host thread)
  device           gwamd_build_window_slices_device: the segments go up, are
                   grouped, the grouped arrays come back
  device_resident  the grouping alone, of records that are already on the
                   device (gwamd_internal_group_repeat)

Part two times cudapolish.polish on polish_cases.e2e_input(length=20000,
reads=30) with device_windows=True and with device_grouping=True.

Prints one JSON line: median, minimum and maximum seconds of each.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from claragenomicsanalysis_amd import cudapolish  # noqa: E402
from claragenomicsanalysis_amd._lib import load_library  # noqa: E402
from claragenomicsanalysis_amd.cudamapper import DeviceReads, Overlap, _check  # noqa: E402


def synthetic_job(records, seed, w=500, read_length=10000, num_reads=20000, num_targets=50, target_length=100000):
    """(target_lengths, reads, qualities, overlaps, segments): reads of read_length +- 10 %
    with Phred 2..40, each overlap the whole of a read against a stretch of a target of the
    same length on either strand, one record per window it touches."""
    rng = np.random.default_rng(seed)
    lengths = rng.integers(read_length * 9 // 10, read_length * 11 // 10, num_reads)
    reads = [bytes(np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n)]) for n in lengths]
    qualities = [bytes(rng.integers(35, 74, n, dtype=np.uint8)) for n in lengths]
    overlaps, rows, total, i = [], [], 0, 0
    while total < records:
        q = int(rng.integers(num_reads))
        t = int(rng.integers(num_targets))
        n = int(lengths[q])
        ts = int(rng.integers(0, target_length - n))
        te = ts + n
        reverse = bool(rng.integers(2))
        overlaps.append((q, t, 0, n, ts, te, "-" if reverse else "+"))
        k = np.arange(ts // w, (te - 1) // w + 1)
        t_begin, t_end = np.maximum(k * w, ts), np.minimum((k + 1) * w, te)
        q_begin, q_end = (te - t_end, te - t_begin) if reverse else (t_begin - ts, t_end - ts)
        block = np.zeros(len(k), cudapolish.SEGMENT_DTYPE)
        block["overlap"], block["window"], block["flags"] = i, k, int(reverse)
        block["q_begin"], block["q_end"], block["t_begin"], block["t_end"] = q_begin, q_end, t_begin, t_end
        rows.append(block)
        total += len(k)
        i += 1
    return [target_length] * num_targets, reads, qualities, overlaps, np.concatenate(rows)[:records]


def timed(call, repeats):
    call()  # warm-up
    out = []
    for _ in range(repeats):
        begin = time.perf_counter()
        call()
        out.append(time.perf_counter() - begin)
    return out


def summary(seconds):
    return {"median_s": float(np.median(seconds)), "min_s": float(min(seconds)), "max_s": float(max(seconds))}


def grouping(args):
    L = load_library()
    target_lengths, reads, qualities, overlaps, segments = synthetic_job(args.records, args.seed)
    to = np.concatenate([[0], np.cumsum(target_lengths)]).astype(np.int64)
    qo = np.concatenate([[0], np.cumsum([len(r) for r in reads])]).astype(np.int64)
    arr = (Overlap * len(overlaps))(*[Overlap(*o) for o in overlaps])
    packed = b"".join(qualities)
    common = (arr, len(overlaps), segments.ctypes.data_as(C.c_void_p), len(segments), 500, 100)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    views = {}

    def take(name, h):
        v = cudapolish._WindowSlicesView()
        _check(L.gwamd_window_slices_get(h, C.byref(v)))
        views[name] = (v.num_windows, v.num_sequences, v.dropped_by_cap, v.dropped_by_quality)
        L.gwamd_window_slices_free(h)

    def host():
        h = C.c_void_p()
        _check(L.gwamd_build_window_slices(ptr(to), len(target_lengths), ptr(qo), len(reads), packed, 100, *common,
                                           C.byref(h)))
        take("host", h)

    out = {"records": len(segments), "overlaps": len(overlaps), "quality_bytes": len(packed)}
    out["host"] = summary(timed(host, args.repeats))
    with DeviceReads(reads, qualities=qualities) as resident:
        def device():
            h = C.c_void_p()
            _check(L.gwamd_build_window_slices_device(ptr(to), len(target_lengths), ptr(qo), len(reads),
                                                      resident._handle, 100, *common, 0, None, C.byref(h)))
            take("device", h)

        out["device"] = summary(timed(device, args.repeats))
        seconds = np.zeros(args.repeats + 1)
        L.gwamd_internal_group_repeat.restype = C.c_int32
        L.gwamd_internal_group_repeat.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32,
                                                  C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int32, C.c_int32,
                                                  C.c_int32, C.c_int32, C.c_void_p]
        _check(L.gwamd_internal_group_repeat(ptr(to), len(target_lengths), ptr(qo), len(reads), resident._handle, 100,
                                             *common, 0, len(seconds), ptr(seconds)))
        out["device_resident"] = summary(seconds[1:].tolist())  # the first is the warm-up
    assert views["host"] == views["device"], views
    out["windows"], out["sequences"], out["dropped_by_cap"], out["dropped_by_quality"] = views["host"]
    return out


def polish(args):
    import polish_cases as pc
    _, draft, queries, overlaps = pc.e2e_input(length=20000, reads=30)
    out = {}
    results = {}
    for name in ("device_windows", "device_grouping"):
        def call():
            results[name] = cudapolish.polish([draft], queries, overlaps, **{name: True})
        out[name] = summary(timed(call, args.repeats))
    assert results["device_windows"] == results["device_grouping"]
    out["windows"] = results["device_grouping"][1]["windows"]
    return out


def main():
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument("--records", type=int, default=1000000)
    parser.add_argument("--repeats", type=int, default=5)
    parser.add_argument("--seed", type=int, default=7)
    parser.add_argument("--skip-polish", action="store_true")
    args = parser.parse_args()
    out = {"grouping": grouping(args)}
    if not args.skip_polish:
        out["polish"] = polish(args)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
