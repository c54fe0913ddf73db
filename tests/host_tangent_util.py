"""Where a point of a host call falls in the pipeline of the rebuilt tangent (csrc/fcamd_hosttangent.cpp): a Python restatement of
host_tangent_plan and of the split of ExpandPool::post, for the diagnosis of tests/test_gpu_host_tangent_default.py.  Both are
checked against the C++ (tests/host_tangent_harness.cpp) in tests/test_host_tangent_pool.py."""

RING_BYTES = 256 << 20
MAX_SLOTS = 16           # fcamd_context::kTangentSlots
MIN_PART_PIPELINE = 2048  # ExpandPool::kMinPartPipeline
MIN_PART_CONST = 16384    # ExpandPool::kMinPart


def up64(x):
    return (x + 63) // 64 * 64


def plan(n, opt_chunk=0, prm=8):
    """(chunk, nslots, starts): host_tangent_plan"""
    chunk = opt_chunk if opt_chunk > 0 else max(1 << 16, min(1 << 20, up64(n // 12)))
    chunk = max(64, chunk // 64 * 64)
    chunk = min(chunk, RING_BYTES // (4 * prm * 8) // 64 * 64)
    chunk = min(chunk, up64(n))
    taper_min = chunk if opt_chunk > 0 else 1 << 16
    start, p = [], 0
    while p < n:
        start.append(p)
        left = n - p
        take = chunk
        if left <= chunk:
            take = up64(left // 2) if left > 2 * taper_min else left
        p += min(take, left)
    start.append(n)
    return chunk, max(4, min(MAX_SLOTS, RING_BYTES // (chunk * prm * 8))), start


def parts(np_, threads, const=False):
    """[(a, b)]: the tasks ExpandPool::post cuts a chunk of np_ points into"""
    k = max(1, min(4 * threads, np_ // (MIN_PART_CONST if const else MIN_PART_PIPELINE)))
    return [((np_ * i // k) & ~63, np_ if i + 1 == k else (np_ * (i + 1) // k) & ~63) for i in range(k)]


def locate(p, n, threads, opt_chunk=0, prm=8, const=False):
    """chunk, ring slot, tile, lane and pool task of point p of a call of n points"""
    if const:
        start, nslots = [0, n], 0
    else:
        _, nslots, start = plan(n, opt_chunk, prm)
    k = max(i for i in range(len(start) - 1) if start[i] <= p)
    q = p - start[k]
    task = next(i for i, (a, b) in enumerate(parts(start[k + 1] - start[k], threads, const)) if a <= q < b)
    return {"chunk": k, "slot": k % nslots if nslots else 0, "tile": p >> 6, "tile_in_chunk": q >> 6, "lane": p & 63, "task": task}
