"""Plain-Python restatement of cudamapper's index descriptors and batches of
indices (reference cudamapper/src/index_descriptor.cpp:76-109 and
index_batcher.cu).  A descriptor is (first_read, number_of_reads); a batch is a
dict of "query" and "target" descriptor lists; a host batch also has
"device_batches"."""


def descriptor_hash(first_read, number_of_reads):
    return (first_read & 0xFFFFFFFF) | ((number_of_reads & 0xFFFFFFFF) << 32)


def group_reads_into_indices(lengths, max_basepairs_per_index=1000000):
    """The current index is closed before it is known to hold a read: read 0
    over the limit gives a leading (0, 0), no reads give [(0, 0)]."""
    out = []
    first, reads, basepairs = 0, 0, 0
    for read_id, length in enumerate(lengths):
        if length + basepairs > max_basepairs_per_index:
            out.append((first, reads))
            first, reads, basepairs = read_id, 1, length
        else:
            basepairs += length
            reads += 1
    out.append((first, reads))
    return out


def group_into_batches(query, target, query_per_batch, target_per_batch, same_query_and_target):
    if same_query_and_target and query_per_batch != target_per_batch:
        raise ValueError("indices per batch differ")
    if query_per_batch < 1 or target_per_batch < 1:
        raise ValueError("indices per batch below 1")
    batches = []
    for q in range(0, len(query), query_per_batch):
        # same query and target: the upper triangle only
        for t in range(q if same_query_and_target else 0, len(target), target_per_batch):
            batches.append({"query": query[q:q + query_per_batch], "target": target[t:t + target_per_batch]})
    return batches


def generate_batches_of_indices(query_per_host, query_per_device, target_per_host, target_per_device, query_lengths,
                                target_lengths, query_basepairs, target_basepairs, same_query_and_target):
    """One parser on both sides is one object given for both lists of lengths."""
    if same_query_and_target:
        if query_per_host != target_per_host or query_per_device != target_per_device:
            raise ValueError("indices per batch differ")
        if query_lengths is not target_lengths:
            raise ValueError("two parsers")
        if query_basepairs != target_basepairs:
            raise ValueError("basepairs per index differ")
    query = group_reads_into_indices(query_lengths, query_basepairs)
    target = group_reads_into_indices(target_lengths, target_basepairs)
    batches = group_into_batches(query, target, query_per_host, target_per_host, same_query_and_target)
    for batch in batches:
        same_in_batch = same_query_and_target and batch["query"] == batch["target"]
        batch["device_batches"] = group_into_batches(batch["query"], batch["target"], query_per_device,
                                                     target_per_device, same_in_batch)
    return batches
