"""Plain numpy statements of what the hand-written scan and radix sort of skm_quant_setup.hip compute
(exclusive_scan_with_total, sort_pairs<K>): what tests/test_gpu_scan_sort.py compares the kernels with, bit for bit.
Checked itself against sorted() and itertools.accumulate in tests/test_sort_scan_reference.py."""
import numpy as np

RADIX_BITS = 9                      # key bits per pass of the sort


def scan(values):
    """int64[n + 1]: the exclusive prefix sums of values[n], and their total in the last entry."""
    return np.concatenate(([0], np.cumsum(values, dtype=np.int64)))


def passes(end_bit):
    return max(1, -(-int(end_bit) // RADIX_BITS))


def sort_mask(end_bit, width):
    """The key bits the sort orders by: whole passes of nine bits, as many as cover end_bit, cut at the key's width."""
    return (1 << min(int(width), RADIX_BITS * passes(end_bit))) - 1


def sort_pairs(keys, vals, end_bit, width):
    """(keys, vals) in the stable order of keys & sort_mask(end_bit, width); the FULL keys are carried."""
    keys = np.asarray(keys)
    vals = np.asarray(vals)
    assert keys.size == 0 or keys.min() >= 0            # (signed keys are non-negative: the kernels' contract)
    mask = np.uint64(sort_mask(end_bit, width))         # (in 64 bits: 2^32 - 1 is no int32)
    order = np.argsort(keys.astype(np.uint64) & mask, kind='stable')
    return keys[order], vals[order]
