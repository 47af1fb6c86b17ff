"""The fragment-length model in numpy: the weights of --fragment-length MEAN --sd SD and the effective-length
rule (seekmer/mapper.py:134-141) with those weights in place of fld / fld.sum().  The product makes the weights
on the host by the same expression and accumulates on the device in the same order with separate multiplies
and adds, so both are compared with array_equal."""
import numpy as np

MAX_FRAGMENT_LENGTH = 2000

# (mean, sd): a usual library; mass on bins 1 and 2; cut at the top bin; a handful of non-zero bins around one;
# all 1999 bins non-zero, so the packed list of the kernel is full
MODELS = ((200, 20), (1.5, 0.4), (1999, 50), (187.3, 0.05), (1000, 1e4))


def weights(mean, sd):
    i = np.arange(2000.0)
    w = np.exp(-0.5 * ((i - mean) / sd) ** 2)
    w[0] = 0
    return w / w.sum()


def effective_lengths(p, lengths):
    """eff_t = sum_i max(len_t - i, 1) * p_i, accumulated for i = 0..1999 in order."""
    length = np.asarray(lengths, dtype='f8')
    eff = np.zeros(length.shape, dtype='f8')
    for i in range(MAX_FRAGMENT_LENGTH):
        eff += (length - i).clip(min=1) * p[i]
    return eff


def transcript_lengths(n_tx=302):
    """The edges of the clamp and of the histogram, then seeded random lengths: f8[n_tx], n_tx <= 302."""
    edges = [1, 24, 25, 150, 199, 200, 201, 1999, 2000, 2001, 10_000, 100_000]
    more = np.random.default_rng(20).integers(1, 5001, 290)
    return np.concatenate([edges, more]).astype('f8')[:n_tx]
