"""The length-bucket rule of a pool admission (csrc/ttx_admit.h: admit_chunks), restated in Python for the tests that check the
library against it: tests/test_admit_host.py on the CPU and tests/test_gpu_admit_buckets.py through the pool's counters.

The rule: an admission of n rows whose n x width is below the budget stays one chunk.  Otherwise rows join the open sub-chunk
until its rows x (longest row so far, at least 2) reaches the budget, which closes it; what is left at the end becomes a sub-chunk
of its own, or joins the one before it when its rows x width is below half the budget."""


def chunk_ends(lens, budget):
    n = len(lens)
    if budget <= 0 or n * max(2, max(lens)) < budget:
        return [n]
    ends, first, w = [], 0, 2
    for r in range(n):
        w = max(w, lens[r])
        if (r + 1 - first) * w >= budget:
            ends.append(r + 1)
            first, w = r + 1, 2
    if first < n:
        if ends and (n - first) * max(2, max(lens[first:])) * 2 < budget:
            ends[-1] = n
        else:
            ends.append(n)
    return ends


def padded_rows(lens, budget):
    """(rows x width summed over the sub-chunks of ONE admission, number of sub-chunks)."""
    ends = chunk_ends(lens, budget)
    return sum((e - f) * max(2, max(lens[f:e])) for f, e in zip([0] + ends[:-1], ends)), len(ends)
