"""Plain-Python model of the (k,w)-minimizer index and the anchor matcher
(reference cudamapper/src/minimizer.cu, index_gpu.cuh, matcher_gpu.cu).

Written window by window with Python ints and lists, for checking the GPU
implementation; nothing here is meant to be fast.  Not collected as a test.
"""

FORWARD, REVERSE = 0, 1
MASK32 = (1 << 32) - 1
MASK64 = (1 << 64) - 1
# complement codes by (byte & 7), what minimizer.cu:147-154, 186 yields:
# A(1)->3, C(3)->2, T(4)->0, G(7)->1 and 0 for every other byte
COMPLEMENT_BY_LOW3 = [0, 3, 0, 2, 0, 0, 0, 1]


def base_code(b):
    return 3 & ((b >> 2) ^ (b >> 1))


def complement_code(b):
    return COMPLEMENT_BY_LOW3[b & 7]


def wang_hash(key):
    """minimizer.cu:55-66 (Thomas Wang's 64-bit hash masked to 32 bits)."""
    key = (~key + (key << 21)) & MASK32
    key = key ^ (key >> 24)
    key = ((key + (key << 3)) + (key << 8)) & MASK32
    key = key ^ (key >> 14)
    key = ((key + (key << 2)) + (key << 4)) & MASK32
    key = key ^ (key >> 28)
    key = (key + (key << 31)) & MASK32
    return key


def _bytes(read):
    return read.encode() if isinstance(read, str) else bytes(read)


def kmer_representations(read, k, hash_representations):
    """[(representation, direction)] of every k-mer of the read."""
    b = _bytes(read)
    out = []
    for p in range(len(b) - k + 1):
        fwd = 0
        rev = 0
        for i in range(k):
            fwd = (fwd << 2) | base_code(b[p + i])
            rev |= complement_code(b[p + i]) << (2 * i)
        if hash_representations:
            fwd, rev = wang_hash(fwd), wang_hash(rev)
        out.append((fwd, FORWARD) if fwd <= rev else (rev, REVERSE))
    return out


def sketch(read, k, w, hash_representations):
    """[(representation, position, direction)] in increasing position."""
    kmers = kmer_representations(read, k, hash_representations)
    K = len(kmers)
    if len(_bytes(read)) < w + k - 1:
        return []
    chosen = set()
    for j in range(K + w - 1):
        lo, hi = max(0, j - w + 1), min(K - 1, j)
        best = lo
        for p in range(lo + 1, hi + 1):
            if kmers[p][0] <= kmers[best][0]:
                best = p
        chosen.add(best)
    return [(kmers[p][0], p, kmers[p][1]) for p in sorted(chosen)]


def first_occurrences(representations):
    unique, first = [], []
    for i, r in enumerate(representations):
        if i == 0 or r != representations[i - 1]:
            unique.append(r)
            first.append(i)
    if representations:
        first.append(len(representations))
    return unique, first


def filter_arrays(representations, read_ids, positions, directions, filtering_parameter):
    """index_gpu.cuh:354-381, 420-422: drops every representation with
    count >= threshold; returns the six arrays."""
    unique, first = first_occurrences(representations)
    threshold = int(len(representations) * filtering_parameter + 0.001)
    keep = []
    for u in range(len(unique)):
        if first[u + 1] - first[u] < threshold:
            keep.extend(range(first[u], first[u + 1]))
    rep = [representations[i] for i in keep]
    unique, first = first_occurrences(rep)
    return (rep, [read_ids[i] for i in keep], [positions[i] for i in keep], [directions[i] for i in keep],
            unique, first)


class Index:
    def __init__(self, reads, kmer_size, window_size, first_read_id=0, past_the_last_read_id=None,
                 hash_representations=True, filtering_parameter=1.0, device_id=0):
        if past_the_last_read_id is None:
            past_the_last_read_id = len(reads)
        elements = []
        longest = 0
        for read_id in range(first_read_id, past_the_last_read_id):
            s = sketch(reads[read_id], kmer_size, window_size, hash_representations)
            if len(_bytes(reads[read_id])) >= window_size + kmer_size - 1:
                longest = max(longest, len(_bytes(reads[read_id])))
            for rep, pos, direction in s:
                elements.append((rep, read_id, pos, direction))
        any_read = longest > 0
        elements.sort(key=lambda e: (e[0], e[1], e[2]))
        rep = [e[0] for e in elements]
        ids = [e[1] for e in elements]
        pos = [e[2] for e in elements]
        dirs = [e[3] for e in elements]
        unique, first = first_occurrences(rep)
        if filtering_parameter < 1.0:
            rep, ids, pos, dirs, unique, first = filter_arrays(rep, ids, pos, dirs, filtering_parameter)
        self.representations = rep
        self.read_ids = ids
        self.positions_in_reads = pos
        self.directions_of_reads = dirs
        self.unique_representations = unique
        self.first_occurrence_of_representations = first
        self.number_of_reads = past_the_last_read_id - first_read_id if any_read else 0
        self.smallest_read_id = first_read_id if any_read else 0
        self.largest_read_id = past_the_last_read_id - 1 if any_read else 0
        self.number_of_basepairs_in_longest_read = longest


def match_anchors(query_index, target_index, max_anchors=None):
    """Sorted list of (query_read_id, target_read_id, query_position_in_read,
    target_position_in_read)."""
    by_representation = {}
    for ti, trep in enumerate(target_index.representations):
        by_representation.setdefault(trep, []).append(ti)
    anchors = []
    for qi, qrep in enumerate(query_index.representations):
        for ti in by_representation.get(qrep, []):
            anchors.append((query_index.read_ids[qi], target_index.read_ids[ti],
                            query_index.positions_in_reads[qi], target_index.positions_in_reads[ti]))
    anchors.sort()
    if max_anchors is not None and len(anchors) > max_anchors:
        raise RuntimeError("more anchors than max_anchors")
    return anchors
