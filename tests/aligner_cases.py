"""Shared by the aligner tie tests (test_aligner_ties.py on the GPU,
test_aligner_cases_cpu.py without one): deterministic (query, target) pairs
on which the four global aligners' results depend on their tie rules, their
letter rule and their seams, and a checker that does not use the oracle.

The kernels are exact, so two implementations can differ only where several
optimal paths exist: at the split column of Hirschberg-Myers, in the
insertion / deletion / diagonal order of the backtraces, in the base cases
and at the band edges.  Uniform random ACGT with scattered edits has few such
places; the families here have many:

  homopolymer   runs of 1..12 of one letter, 5 % edits
  two_letter    alphabet AC, 10 % edits
  tandem        a unit of 2..9 bases repeated, 3 % edits
  shifted       "AC" * n against "CA" * n, a homopolymer against a longer
                one, a homopolymer against another letter (no match at all)
  long_gap      a block of 63..200 bases present in one sequence only, at
                the start, the middle and the end
  alphabet      bytes outside ACGT on both sides (the letter rule below)
  seams(f)      tie family f at the lengths below, at and above every seam
                of the kernels (words, blocks, stripes, leaves, tiles)
  max_query     Hirschberg-Myers pairs whose result changes with the
                aligner's max_query_length
  banded        one pair list per band class of banded Myers
  ukkonen_rows  length differences on both sides of every 64-row chunk count
                of the Ukkonen band, and of the 512-row hand-over

Letter rule.  The three Myers aligners reduce a target byte c to
"ACTG"[(c >> 1) & 3] and a query byte matches only if it is that letter
exactly, so a target N matches a query G and a lowercase target matches an
uppercase query, but not the other way round.  Ukkonen compares raw bytes.
The single-query-base case of Hirschberg-Myers compares raw bytes too; paths
are checked for optimality under the rule of their aligner ("myers" / "raw").

Sequences are str where they are ASCII and bytes in the alphabet family.
Every function is pure and seeded by its arguments.
"""
import functools
import random

import numpy as np

MATCH, MISMATCH, INSERTION, DELETION = 0, 1, 2, 3
UKKONEN_P = 100  # the band parameter of the Ukkonen aligner

TIE_FAMILIES = ("homopolymer", "two_letter", "tandem", "shifted")
# query lengths around the 32-bit word, the 63-row full-Myers switch, the
# 64-lane word groups, kLeafCols / two words x 64, the 2,048-row block and
# the 4,096-row stripe of GWAMD_HM_STRIPE_BLOCKS=2
SEAM_QUERY = (31, 32, 33, 62, 63, 64, 65, 127, 128, 129, 2047, 2048, 2049, 4096, 4097)
SEAM_QUERY_8K = (8191, 8192, 8193)               # the 8,192-row stripe: full Myers only
SEAM_TARGET = (127, 128, 129, 511, 512, 513)     # kLeafCols, kSplitLds
SEAM_TARGET_TILE = (63, 64, 65, 191, 192, 193, 255, 256, 257)  # the full-Myers backtrace tile of 64 columns
MAX_QUERY_VALUES = (62, 100, 400, 5000)          # and the longest query of the batch


def _b(s):
    return s.encode("latin-1") if isinstance(s, str) else bytes(s)


# ---- sequence generators -------------------------------------------------------

def _homopolymer_seq(rng, n):
    out, last = [], ""
    while len(out) < n:
        c = rng.choice([x for x in "ACGT" if x != last])
        out.extend(c * rng.randint(1, 12))
        last = c
    return "".join(out[:n])


def _two_letter_seq(rng, n):
    return "".join(rng.choice("AC") for _ in range(n))


def _tandem_seq(rng, n):
    while True:
        unit = "".join(rng.choice("ACGT") for _ in range(rng.randint(2, 9)))
        if len(set(unit)) > 1:
            return (unit * (n // len(unit) + 1))[:n]


def _random_seq(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


_GEN = {"homopolymer": (_homopolymer_seq, "ACGT", 0.05), "two_letter": (_two_letter_seq, "AC", 0.10),
        "tandem": (_tandem_seq, "ACGT", 0.03)}


def edit(rng, s, rate, alphabet):
    """int(len * rate) single-base edits (substitution, insertion, deletion) at random places."""
    q = list(s)
    for _ in range(int(len(s) * rate)):
        k, p = rng.randrange(3), rng.randrange(len(q) + 1)
        if k == 0 and p < len(q):
            q[p] = rng.choice(alphabet)
        elif k == 1:
            q.insert(p, rng.choice(alphabet))
        elif p < len(q):
            del q[p]
    return type(s)(q) if isinstance(s, bytes) else "".join(q)


def _tie_pair(family, seed, n, exact="target"):
    """One pair of a generated tie family; the `exact` side has exactly n bases."""
    gen, alphabet, rate = _GEN[family]
    rng = random.Random("%s/%s/%d" % (family, seed, n))
    base = gen(rng, n)
    other = edit(rng, base, rate, alphabet)
    return (other, base) if exact == "target" else (base, other)


# ---- tie families ----------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def tie_family(family):
    """12 pairs (4 at each of 300, 600 and 900 bases); for "shifted" its fixed pairs."""
    if family == "shifted":
        return tuple(_shifted())
    return tuple(_tie_pair(family, k, n) for n in (300, 600, 900) for k in range(4))


def _shifted():
    out = []
    for n in (16, 150, 301):                      # one base out of phase: every diagonal ties
        out.append(("AC" * n, "CA" * n))
    out.append(("CA" * 200 + "C", "AC" * 200))
    for q, t in ((31, 40), (64, 100), (300, 330), (330, 300), (700, 640)):
        out.append(("A" * q, "A" * t))            # every placement of the gap is optimal
    for q, t in ((33, 33), (100, 90), (300, 330), (640, 700)):
        out.append(("A" * q, "C" * t))            # no match at all
    return out


# ---- long gaps --------------------------------------------------------------------

LONG_GAPS = (63, 64, 65, 127, 128, 129, 200)


@functools.lru_cache(maxsize=None)
def long_gap():
    """A 2,200-base homopolymer-run sequence (22 substitutions) against itself without
    a block of g bases, the block in the target only and in the query only, at
    the start, the middle and the end: 42 pairs, all within Ukkonen's 10 % rule
    at a max_target_length of 2,200 and more."""
    out = []
    for g in LONG_GAPS:
        for where in ("start", "middle", "end"):
            rng = random.Random("gap/%d/%s" % (g, where))
            full = _homopolymer_seq(rng, 2200)
            at = {"start": 0, "middle": 1100 - g // 2, "end": 2200 - g}[where]
            cut = _sub_only(rng, full[:at] + full[at + g:], 22)
            out.append((cut, full))               # a run of g insertions
            out.append((full, cut))               # a run of g deletions
    return tuple(out)


# ---- alphabet ---------------------------------------------------------------------

ALPHABET = b"ACGTNacgtnRYKM-*" + bytes([0x80, 0xC1, 0xC7, 0xFF])


def _alpha_seq(rng, n, alphabet=ALPHABET):
    return bytes(rng.choice(alphabet) for _ in range(n))


@functools.lru_cache(maxsize=None)
def alphabet():
    """Pairs with bytes outside ACGT on the target side as well: the whole
    alphabet at 70, 600 and 1,500 bases, both orientations of the N / G quirk,
    a lowercase target against an uppercase query, a soft-masked query against
    an uppercase target with N, and a lowercase query against an uppercase
    target (70 bases: nothing matches under either rule).  The rules coincide
    whenever the target is pure ACGT, so every longer pair has other bytes in
    its target."""
    out = []
    for n in (70, 600, 1500):
        rng = random.Random("alphabet/%d" % n)
        t = _alpha_seq(rng, n)
        out.append((edit(rng, t, 0.06, ALPHABET), t))
    rng = random.Random("alphabet/quirk")
    base = _random_seq(rng, 600).encode()
    with_n = bytes(ord("N") if c == ord("G") and rng.random() < 0.5 else c for c in base)
    near = edit(rng, base, 0.04, b"ACGT")
    out.append((near, with_n))                     # target N under query G: a match for Myers
    # query N over target G: a mismatch for both rules (the target's few lowercase bases separate them)
    some_lower = bytes(c + 32 if rng.random() < 0.05 else c for c in base)
    out.append((edit(rng, with_n, 0.04, b"ACGTN"), some_lower))
    # query N over a target N is a raw match and a Myers mismatch
    out.append((edit(rng, with_n, 0.04, b"ACGTN"), with_n))
    out.append((near, base.lower()))               # lowercase target: Myers matches, raw does not
    masked = bytearray(near)
    for lo in range(0, len(masked), 100):          # soft-masked query: lowercase blocks never match
        masked[lo:lo + 50] = bytes(masked[lo:lo + 50]).lower()
    out.append((bytes(masked), with_n))
    out.append((base.lower()[:70], base[:70]))     # lowercase query, uppercase target: no match under either rule
    return tuple(out)


def reverse_complement(s):
    """genomeutils::reverse_complement: A/C/G/T complemented, every other byte kept."""
    comp = {ord("A"): ord("T"), ord("T"): ord("A"), ord("C"): ord("G"), ord("G"): ord("C")}
    r = bytes(comp.get(c, c) for c in reversed(_b(s)))
    return r if isinstance(s, bytes) else r.decode("latin-1")


# ---- seam lengths -----------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def seams(family):
    """Tie family `family` at the seam lengths: the query at every length of
    SEAM_QUERY, the target at every length of SEAM_TARGET against a 40-base
    query cut from it (a leaf of that many columns) and against a query of
    about its own length (a split segment of that many columns), and at every
    length of SEAM_TARGET_TILE."""
    gen, letters, rate = _GEN[family]
    out = [_tie_pair(family, "sq", n, exact="query") for n in SEAM_QUERY]
    for n in SEAM_TARGET:
        q, t = _tie_pair(family, "st", n)
        rng = random.Random("%s/leaf/%d" % (family, n))
        at = rng.randrange(n - 48)
        out.append((edit(rng, t[at:at + 48], rate, letters)[:40], t))
        out.append((q, t))
    out += [_tie_pair(family, "tile", n) for n in SEAM_TARGET_TILE]
    return tuple(out)


@functools.lru_cache(maxsize=None)
def seams_8k():
    """One pair per length of SEAM_QUERY_8K (full Myers: the 8,192-row stripe)."""
    fams = ("homopolymer", "two_letter", "tandem")
    return tuple(_tie_pair(f, "8k", n, exact="query") for f, n in zip(fams, SEAM_QUERY_8K))


# ---- max_query_length ---------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def max_query():
    """Hirschberg-Myers takes the full-Myers leaf for a segment of m < 63 rows
    and Ts columns only while (Ts + 1) * ceil(m / 32) <= ((max_q + 3) / 4) * 64,
    so the same pair is split more or less often under another
    max_query_length.  Queries of 40 and 60 bases cut from tie-heavy targets of
    600 and 2,000 bases.  A 2,000-column pair has three regimes over
    MAX_QUERY_VALUES (62: two levels of splits, 100: one, 400 and more: none;
    the query sits at about column 400, so that the wider half of the first
    split has between 1,024 and 1,600 columns).  A 600-column pair has two:
    2 * 601 elements exceed the capacity at 62 and below only, and the halves
    (one word, at most 601 columns) fit every capacity."""
    out = []
    for T in (600, 2000):
        for m in (40, 60):
            rng = random.Random("maxq/%d/%d/0" % (T, m))
            t = _homopolymer_seq(rng, T)
            at = 400 if T == 2000 else 280
            q = edit(rng, t[at:at + m], 0.10, "ACGT")
            q = (q + t[at + m:at + 2 * m])[:m]
            out.append((q, t))
    return tuple(out)


def max_query_regimes(pair):
    """The least number of distinct results the pair must show over
    MAX_QUERY_VALUES and the longest query (see max_query)."""
    return 3 if len(pair[1]) >= 2000 else 2


# ---- banded Myers band classes -------------------------------------------------------

def _sub_only(rng, s, k, letters="ACGT"):
    q = list(s)
    for p in rng.sample(range(len(q)), k):
        q[p] = rng.choice([c for c in letters if c != q[p]])
    return "".join(q)


@functools.lru_cache(maxsize=None)
def banded():
    """{class: pairs}.  The first band of a pair is
    bw = min(1 + 2 * (min(T, Q) / 40) + |T - Q|, Q), accepted when the distance
    inside it is at most |T - Q| + min(T, Q) / 20, else the estimate doubles.
      bw_mod32_0   |T - Q| = 13 at 1,000 and 1,013 bases: bw = 64, accepted at once (the
                   backtrace starts in the band's last full word)
      bw_mod32_1   |T - Q| = 14: 65 rows are widened to 67
      bw_is_query  the band is the whole query (short queries, and a band
                   doubled up to it)
      tries_1 / tries_2 / tries_4   1, 2 and at least 4 estimates
      multi_chunk  bands of more than 32 words; the second pair's band is more
                   than 256 words, which a 4 KiB tile does not hold"""
    out = {}
    rng = random.Random("banded")

    def near(n, diff, subs, longer_query):
        base = _homopolymer_seq(rng, n)
        cut = sorted(rng.sample(range(n), diff), reverse=True)
        short = list(base)
        for p in cut:
            del short[p]
        short = _sub_only(rng, "".join(short), subs)
        return (base, short) if longer_query else (short, base)

    out["bw_mod32_0"] = (near(1013, 13, 20, False), near(1013, 13, 12, True), near(1013, 13, 0, False))
    out["bw_mod32_1"] = (near(1014, 14, 20, False), near(1014, 14, 12, True))
    out["bw_is_query"] = (("ACCA" * 5, "ACCA" * 12), (_two_letter_seq(rng, 33), _two_letter_seq(rng, 70)),
                          (_two_letter_seq(rng, 330), _homopolymer_seq(rng, 300)))
    out["tries_1"] = (near(600, 3, 8, False), near(1200, 0, 30, True))
    out["tries_2"] = (near(1200, 2, 85, False), near(800, 5, 60, True))
    out["tries_4"] = (near(1200, 4, 420, False), (edit(rng, _two_letter_seq(rng, 900), 0.45, "AC"),
                                                  _two_letter_seq(rng, 900)))
    big = _two_letter_seq(rng, 2600)
    huge = _homopolymer_seq(rng, 8400)
    out["multi_chunk"] = ((_homopolymer_seq(rng, 2700), big), (_homopolymer_seq(rng, 8300), huge))
    return out


# ---- Ukkonen band rows ----------------------------------------------------------------

UKKONEN_DIFFS = (54, 56, 182, 184, 310, 312, 438, 440)   # 128|129, 192|193, 256|257, 320|321 rows
UKKONEN_WIDE_DIFFS = (822, 824)                           # 512 rows | 513 rows: ukkonen_wide_kernel
UKKONEN_ROWS_MAX_TARGET = 4400                            # int(4400 * 0.1f) = 440
UKKONEN_WIDE_MAX_TARGET = 8240                            # int(8240 * 0.1f) = 824


def ukkonen_band_rows(diff):
    return (diff + 2 * UKKONEN_P + 2) // 2


def _ukkonen_pairs(diffs, short):
    out = []
    for d in diffs:
        rng = random.Random("ukkonen/%d" % d)
        long_ = _homopolymer_seq(rng, short + d)
        cut = sorted(rng.sample(range(short + d), d), reverse=True)
        s = list(long_)
        for p in cut:
            del s[p]
        s = edit(rng, "".join(s), 0.01, "ACGT")
        s = (s + long_[-8:])[:short]
        out.append((s, long_))                     # target longer
        out.append((long_, s))                     # query longer: the kernel swaps the roles
    return tuple(out)


@functools.lru_cache(maxsize=None)
def ukkonen_rows():
    return _ukkonen_pairs(UKKONEN_DIFFS, 1000)


@functools.lru_cache(maxsize=None)
def ukkonen_wide(diff):
    return _ukkonen_pairs((diff,), 1000)


def ukkonen_allowed_difference(max_target_length):
    """aligner_global_ukkonen.cpp:47-57: int(max_target_length * 0.1f) in float arithmetic."""
    return int(np.float32(max_target_length) * np.float32(0.1))


def ukkonen_max_target(pairs):
    """The smallest max_target_length that holds every target and whose 10 %
    rule admits every pair of the list."""
    mt = max([1] + [len(t) for _, t in pairs])
    diff = max([0] + [abs(len(q) - len(t)) for q, t in pairs])
    while ukkonen_allowed_difference(mt) < diff:
        mt += 1
    return mt


# ---- the batches of the tests ------------------------------------------------------------

# name, the oracle's algorithm number, the checker's rule
ALGORITHMS = (("hirschberg_myers", 0, "myers"), ("myers", 1, "myers"), ("myers_banded", 2, "myers"),
              ("ukkonen", 3, "raw"))


def batches():
    """{name: pairs} of the batches every algorithm runs (one aligner each)."""
    out = {f: tie_family(f) for f in TIE_FAMILIES}
    out["long_gap"] = long_gap()
    out["alphabet"] = alphabet()
    for f in ("homopolymer", "two_letter", "tandem"):
        out["seams_" + f] = seams(f)
    for k, v in banded().items():
        if k != "multi_chunk":  # its 8 kb pair has a test of its own
            out["banded_" + k] = v
    out["ukkonen_rows"] = ukkonen_rows()
    return out


def capacity(pairs, algorithm):
    """(max_query_length, max_target_length) of the aligner of one batch: the
    longest query and target, and for Ukkonen a max_target_length whose 10 %
    rule admits every pair."""
    mq = max([1] + [len(q) for q, _ in pairs])
    mt = max([1] + [len(t) for _, t in pairs])
    return mq, (ukkonen_max_target(pairs) if algorithm == "ukkonen" else mt)


@functools.lru_cache(maxsize=None)
def _oracle_states(q, t, oalgo, mq):
    from oracle import oracle
    return tuple(oracle.align(q, t, oalgo, mq))


def oracle_states(query, target, oalgo, max_query_length):
    """oracle.align, computed once per process (only Hirschberg-Myers depends on max_query_length)."""
    return list(_oracle_states(_b(query), _b(target), oalgo, max_query_length if oalgo == 0 else 0))


# ---- the checker ----------------------------------------------------------------------

def _letter(c):
    return b"ACTG"[(c >> 1) & 3]


def _rule_bytes(q, t, rule):
    """The query and the target as arrays that are equal exactly where `rule` says the bytes match."""
    qa = np.frombuffer(q, np.uint8)
    ta = np.frombuffer(t, np.uint8)
    if rule == "myers":
        ta = np.frombuffer(b"ACTG", np.uint8)[(ta >> 1) & 3]
    elif rule != "raw":
        raise ValueError(rule)
    return qa, ta


def _is_acgt(s):
    return not set(s) - set(b"ACGT")


@functools.lru_cache(maxsize=4096)
def _distance(q, t, rule):
    qa, ta = _rule_bytes(q, t, rule)
    n = len(ta)
    j = np.arange(n + 1, dtype=np.int64)
    row = j.copy()
    for i in range(len(qa)):
        x = np.empty(n + 1, np.int64)
        x[0] = i + 1
        np.minimum(row[:-1] + (ta != qa[i]), row[1:] + 1, out=x[1:])
        # insertions: D[i][j] = min over k <= j of x[k] + (j - k)
        row = np.minimum.accumulate(x - j) + j
    return int(row[n])


def edit_distance(query, target, rule):
    """Unit-cost edit distance by a plain row-by-row DP; a diagonal step costs 0
    where `rule` ("myers" or "raw") says the bytes are equal."""
    q, t = _b(query), _b(target)
    if _is_acgt(q) and _is_acgt(t):
        rule = "raw"  # the two rules coincide on ACGT: one DP serves both
    return _distance(q, t, rule)


def check_alignment(query, target, states, rule, band_limited=False, exact=True):
    """Asserts that `states` (start -> end) is an alignment of exactly the
    query and the target whose cost under `rule` is the edit distance, and on
    ACGT-only input that a diagonal step is a match exactly where the bytes
    are equal.  Returns the cost.
    band_limited (Ukkonen): the band holds every optimal path only while the
    distance is at most UKKONEN_P; past that the cost may exceed it.
    exact=False (banded Myers with a band of more than 32 words that is not
    the whole query): the cost may exceed the distance and the match /
    mismatch condition is dropped.  Where such a band runs diagonally the
    reference hands the vertical delta of a 32-word chunk's last row to the
    next chunk as its horizontal carry (myers_gpu.cu:595-603), so scores below
    a chunk boundary can be off, the backtrace can leave the optimal path
    there, and it labels steps by comparing such scores.  The oracle and the
    kernels restate this as it is."""
    q, t = _b(query), _b(target)
    st = np.asarray(states, np.int64)
    assert st.size == 0 or (st.min() >= 0 and st.max() <= 3), "unknown state"
    diag = st <= MISMATCH
    in_q = diag | (st == DELETION)
    in_t = diag | (st == INSERTION)
    assert int(in_q.sum()) == len(q) and int(in_t.sum()) == len(t), \
        "path consumes (%d, %d) of (%d, %d)" % (in_q.sum(), in_t.sum(), len(q), len(t))
    qi = np.cumsum(in_q)[diag] - 1
    ti = np.cumsum(in_t)[diag] - 1
    qa, ta = _rule_bytes(q, t, rule)
    neq = qa[qi] != ta[ti]
    cost = int(neq.sum()) + int((~diag).sum())
    if exact and _is_acgt(q) and _is_acgt(t):
        assert np.array_equal(st[diag] == MISMATCH, neq), "match / mismatch states do not follow the bytes"
    dist = edit_distance(q, t, rule)
    if not exact or (band_limited and dist > UKKONEN_P):
        assert cost >= dist, (cost, dist)
    else:
        assert cost == dist, (cost, dist)
    return cost
