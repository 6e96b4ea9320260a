"""CIGARs for the tests of cudapolish's cut from CIGAR runs: the run-length
encoding of a state path (polish_model.py's states) in either convention, the
expansion back, and the "sam" convention stated directly, without the
normalisation the library uses.

"genomeworks": I advances only the target (state 2), D only the query (state
3); the ops follow the path.  "sam": I advances only the query, D only the
target; for a '-' overlap the ops run along the target forward, which is the
path backwards.
"""
import os
import subprocess

import numpy as np

from polish_model import BAD_PATH, EMPTY, REVERSE, window_count

TILE = 64          # kCigarTileOps: the ops a wave covers in one step
OWN_CROSSINGS = 2  # kCigarOwnCrossings: the boundaries inside a run its own lane walks
LETTERS = "MIDNSHP=X"
MAX_LENGTH = (1 << 28) - 1

_LETTER_OF = {"genomeworks": {0: "=", 1: "X", 2: "I", 3: "D"}, "sam": {0: "=", 1: "X", 2: "D", 3: "I"}}


def runs_of(states):
    """[(state, length)] of a state path."""
    runs = []
    for s in states:
        if runs and runs[-1][0] == s:
            runs[-1][1] += 1
        else:
            runs.append([s, 1])
    return [(s, n) for s, n in runs]


def cigar_of(states, strand="+", convention="genomeworks", use_m=False):
    """The CIGAR text of a fitting state path; use_m: M for both match and mismatch."""
    letter = dict(_LETTER_OF[convention])
    if use_m:
        states = [0 if s == 1 else s for s in states]
        letter[0] = "M"
    if convention == "sam" and strand == "-":
        states = states[::-1]
    # (a state outside 0..3 has no letter of its own: N, which the cut refuses as it refuses the state)
    return "".join("%d%s" % (n, letter.get(s, "N")) for s, n in runs_of(states))


def parse(text):
    """[(length, letter)] of CIGAR text, in plain Python."""
    out, number = [], ""
    for c in text:
        if c.isdigit():
            number += c
        else:
            out.append((int(number), c))
            number = ""
    assert number == ""
    return out


def expand(text, strand="+", convention="genomeworks"):
    """The state path CIGAR text stands for (M and = as 0, X as 1); a letter
    outside MID=X as the state 9, which fits no overlap."""
    state = {letter: s for s, letter in _LETTER_OF[convention].items()}
    state["M"] = 0
    states = []
    for n, c in parse(text):
        if c not in state:
            states.append(9)
        else:
            states += [state[c]] * n
    if convention == "sam" and strand == "-":
        states = states[::-1]
    return states


def to_sam(text, strand):
    """A "genomeworks" CIGAR rewritten in the "sam" convention."""
    swap = {"I": "D", "D": "I"}
    ops = [(n, swap.get(c, c)) for n, c in parse(text)]
    if strand == "-":
        ops = ops[::-1]
    return "".join("%d%s" % op for op in ops)


def text_of(ops):
    """CIGAR text of packed ops."""
    return "".join("%d%s" % (int(op) >> 4, LETTERS[int(op) & 15]) for op in ops)


def pack(length, letter):
    return np.uint32(length << 4 | LETTERS.index(letter))


def sam_segments(index, overlap, text, w):
    """The records of one overlap from its "sam" CIGAR by SAM's own definition:
    the ops run along the target forward from target_start; for '-' the query
    region is reverse-complemented, so query offset v sits at q = query_end - 1 - v."""
    _, _, qs, qe, ts, te, strand = overlap
    reverse = strand == "-"
    base = REVERSE if reverse else 0
    k0, count = ts // w, window_count(ts, te, w)
    ops = parse(text)
    u = sum(n for n, c in ops if c in "M=XD")
    v = sum(n for n, c in ops if c in "M=XI")
    if any(c not in "M=XID" for _, c in ops) or u != te - ts or v != qe - qs:
        return [(index, k0 + j, 0, 0, 0, 0, base | EMPTY | BAD_PATH, 0) for j in range(count)]
    seen = {}
    u = v = 0
    for n, c in ops:
        for _ in range(n):
            if c in "M=X":
                seen.setdefault((ts + u) // w, []).append((qe - 1 - v if reverse else qs + v, ts + u))
            u += c in "M=XD"
            v += c in "M=XI"
    out = []
    for k in range(k0, k0 + count):
        if k not in seen:
            out.append((index, k, 0, 0, 0, 0, base | EMPTY, 0))
            continue
        qq, tt = [p[0] for p in seen[k]], [p[1] for p in seen[k]]
        out.append((index, k, min(qq), max(qq) + 1, min(tt), max(tt) + 1, base, 0))
    return out


def misfit_records(index, overlap, w):
    """Every record of the overlap empty with BAD_PATH."""
    _, _, _, _, ts, te, strand = overlap
    flag = (REVERSE if strand == "-" else 0) | EMPTY | BAD_PATH
    return [(index, ts // w + j, 0, 0, 0, 0, flag, 0) for j in range(window_count(ts, te, w))]


# sixteen runs of 2^28 - 1 and one of 116: 2^32 + 100 advances of each sequence
WRAP_CIGAR = "%dM" % MAX_LENGTH * 16 + "116M"
WRAP_SPANS = (0, 100, 0, 100)


def build_cpp_check(tmp_path):
    """tests/polish_cigar_cpp_check.cpp compiled against the built library; returns the program's path."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib = os.path.join(root, "claragenomicsanalysis_amd", "lib")
    exe = str(tmp_path / "polish_cigar_cpp_check")
    subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-std=c++17", "-O1", "-Wall",
                           "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(root, "include"), "-I", "/opt/rocm/include",
                           "-x", "c++", os.path.join(root, "tests", "polish_cigar_cpp_check.cpp"), "-L", lib,
                           "-lgwamd", "-Wl,-rpath," + lib, "-o", exe])
    return exe


CPP_HOST = ["cigar_ops", "cigar_refused", "host_walk", "host_walk_sam", "read_paf", "convention_refused",
            "no_overlaps_no_device_call"]
CPP_GPU = ["device_cut", "device_cut_sam"]
