"""The component labels of the set-up (skm_quant_setup.hip: cc_hook_kernel, cc_label_kernel) against a plain
union-find on tables that are made of walks: one chain of 5 000 classes of two transcripts, its classes in
ascending, descending and shuffled order -- paths far longer than any bound a walk may put on its steps before it
starts halving them -- and 300 disjoint classes of three.  A label is the smallest transcript id of the component."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LINKS = 5000


def _union_find_labels(n_tx, classes):
    parent = list(range(n_tx))

    def root(v):
        while parent[v] != v:
            parent[v] = parent[parent[v]]         # (halving: the chains are long for a plain walk too)
            v = parent[v]
        return v

    for members in classes:
        for t in members[1:]:
            a, b = root(members[0]), root(t)
            if a != b:
                parent[max(a, b)] = min(a, b)
    return np.array([root(t) for t in range(n_tx)], dtype=np.int64)


def _tables():
    chain = [[t, t + 1] for t in range(LINKS)]
    shuffled = [chain[i] for i in np.random.default_rng(3).permutation(LINKS)]
    triples = [[3 * i + 2, 3 * i, 3 * i + 1] for i in range(300)]
    return {'ascending': (LINKS + 1, chain), 'descending': (LINKS + 1, chain[::-1]), 'shuffled': (LINKS + 1, shuffled),
            'triples': (900, triples)}


@pytest.mark.parametrize('name', ['ascending', 'descending', 'shuffled', 'triples'])
def test_labels(native_libs, name):
    from seekmer_amd import infer
    n_tx, classes = _tables()[name]
    offsets = np.concatenate([[0], np.cumsum([len(c) for c in classes])]).astype(np.int64)
    targets = np.concatenate([np.asarray(c, dtype=np.int32) for c in classes]).astype(np.int32)
    expected = _union_find_labels(n_tx, classes)
    if name == 'triples':
        np.testing.assert_array_equal(expected, np.repeat(3 * np.arange(300), 3))
    else:
        assert not expected.any()
    quant = infer._QuantHandle.from_csr(n_tx, offsets, targets, np.ones(len(classes)))
    try:
        info, label, tile, _ = quant.components()
        assert info['built']
        np.testing.assert_array_equal(label, expected)
        if name == 'triples':
            assert info['oversize'] == 0 and info['tiles'] > 0 and (tile < n_tx).all()
        else:
            assert info['oversize'] == 1 and info['tiles'] == 0 and (tile == n_tx).all()
    finally:
        quant.close()
