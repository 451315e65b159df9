"""CPU suite: the index arithmetic of the radius search's long-row sort (radius_sort_kernel, csrc/radius_kernels.hip), restated step for
step in Python and run as the kernel runs it: the row padded in thought to a power of two, every chunk sorted by the merges up to the
chunk's width, then the merges that span chunks -- their first steps on the whole row with a partner at or beyond the row's end skipped,
the steps inside a chunk on the chunk's image again.  It must sort every length, at a small chunk (many chunk-spanning merges at lengths a
test can afford) and at the kernel's own chunk around its limits.  What this cannot show is the kernel's barriers and memory; the GPU suite
(tests/test_gpu_radius.py) runs the kernel at the same limits."""
import numpy as np
import pytest

PAD = 2 ** 64 - 1


def lower(t, j):
    """slot t of a step at distance j -> the lower index of its pair (sort_lower)"""
    return ((t & ~(j - 1)) << 1) | (t & (j - 1))


def exchange(a, i, p):
    if a[p] < a[i]:
        a[i], a[p] = a[p], a[i]


def lds_steps(image, width, j_hi):
    j = j_hi
    while j >= 1:
        for t in range(width // 2):
            i = lower(t, j)
            exchange(image, i, i + j)
        j >>= 1


def sort_row(row, chunk):
    L = len(row)
    if L < 2:
        return
    P = 1 << (L - 1).bit_length()
    width = min(P, chunk)
    for cb in range(0, L, chunk):
        image = [row[cb + t] if cb + t < L else PAD for t in range(width)]
        k = 2
        while k <= width:
            for t in range(width // 2):
                i = lower(t, k >> 1)
                exchange(image, i, i ^ (k - 1))
            lds_steps(image, width, k >> 2)
            k <<= 1
        assert all(v == PAD for v in image[max(L - cb, 0):])                          # no step moved a pad
        row[cb:min(cb + width, L)] = image[:min(width, L - cb)]
    k = 2 * chunk
    while k <= P:
        for t in range(P // 2):
            i = lower(t, k >> 1)
            p = i ^ (k - 1)
            if p < L:
                exchange(row, i, p)
        j = k >> 2
        while j >= chunk:
            for t in range(P // 2):
                i = lower(t, j)
                if i + j < L:
                    exchange(row, i, i + j)
            j >>= 1
        for cb in range(0, L, chunk):
            image = [row[cb + t] if cb + t < L else PAD for t in range(chunk)]
            lds_steps(image, chunk, chunk >> 1)
            row[cb:min(cb + chunk, L)] = image[:min(chunk, L - cb)]
        k <<= 1


def rows_of(lengths, seed):
    rng = np.random.default_rng(seed)
    for L in lengths:
        yield [int(v) for v in rng.permutation(3 * L + 1)[:L]]


def test_every_length_at_a_small_chunk():
    for row in rows_of(list(range(0, 200)) + [255, 256, 257, 511, 513], 1):
        want = sorted(row)
        sort_row(row, 16)
        assert row == want, len(row)


def test_the_kernels_chunk_at_its_limits(capi):
    chunk = capi.RADIUS_SORT_CHUNK
    lengths = [capi.RADIUS_WAVE_ROW + 1, chunk - 1, chunk, chunk + 1, 2 * chunk - 1, 2 * chunk, 2 * chunk + 1]
    for row in rows_of(lengths, 2):
        want = sorted(row)
        sort_row(row, chunk)
        assert row == want, len(row)


@pytest.mark.parametrize("j", [1, 2, 8, 64])
def test_lower_enumerates_each_pair_once(j):
    pairs = {(lower(t, j), lower(t, j) + j) for t in range(128)}
    assert len(pairs) == 128 and sorted(i for p in pairs for i in p) == list(range(256))
