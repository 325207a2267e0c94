def chunk_evenly(iterable, n):
    """Consecutive chunks of ``iterable`` (a sequence) of about ``n`` elements each, as the reference's
    ``eeyore.itertools.chunk_evenly`` cuts them: ``len // n`` chunks when ``n`` divides the length, otherwise one chunk per
    multiple of ``n`` below ``len - n``, the first ``len % n`` chunks one element longer.  So 4 elements with n = 3 give
    ONE chunk of 4; a remainder larger than the number of chunks loses the tail (5 elements with n = 3: one chunk of 4)
    and a sequence shorter than ``n`` gives no chunk at all, as there.  The behaviour is pinned by recorded pairs in
    tests/golden/g12_gibbs_traces.npz."""
    if n < 1:
        raise ValueError(f"chunk_evenly: the chunk size must be >= 1, got {n}")
    total = len(iterable)
    rest = total % n
    count = total // n if rest == 0 else len(range(0, total - n, n))
    start = 0
    for k in range(count):
        size = n + 1 if k < rest else n
        yield iterable[start:start + size]
        start += size
