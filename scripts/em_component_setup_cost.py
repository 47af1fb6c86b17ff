#!/usr/bin/env python
"""What the components and tiles cost where they give nothing back: the set-up of a quantification
handle (skm_quant_create) on tables that are ONE component, with the tiles and with
SKM_EM_NO_COMPONENTS=1, wall time, best of several.  Needs a GPU.

    python scripts/em_component_setup_cost.py
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def table(kind, n_tx, n_classes, rng):
    chain = np.stack([np.arange(n_tx - 1), np.arange(1, n_tx)], axis=1).astype(np.int32)     # one component for certain
    if kind == 'chain':            # nothing but the chain: the longest walks the union-find can be given
        rows = chain
        lens = np.full(rows.shape[0], 2, dtype=np.int64)
        targets = rows.reshape(-1)
    else:                          # the benchmark's shape glued together: classes of 5 random transcripts + the chain
        extra = rng.integers(0, n_tx, (n_classes, 5)).astype(np.int32)
        lens = np.concatenate([np.full(chain.shape[0], 2), np.full(n_classes, 5)]).astype(np.int64)
        targets = np.concatenate([chain.reshape(-1), extra.reshape(-1)])
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    return offsets, targets.astype(np.int32), rng.integers(1, 30, lens.size).astype('f8')


def main():
    from seekmer_amd import infer
    rng = np.random.default_rng(1)
    for kind, n_tx, n_classes in (('random', 190_402, 660_000), ('chain', 190_402, 0)):
        offsets, targets, counts = table(kind, n_tx, n_classes, rng)
        best = {}
        for switch in (None, '1', None, '1', None, '1', None, '1'):
            if switch is None:
                os.environ.pop('SKM_EM_NO_COMPONENTS', None)
            else:
                os.environ['SKM_EM_NO_COMPONENTS'] = switch
            t0 = time.perf_counter()
            quant = infer._QuantHandle.from_csr(n_tx, offsets, targets, counts)
            dt = time.perf_counter() - t0
            info = quant.components(arrays=False)[0]
            quant.close()
            best[switch] = min(best.get(switch, 1e9), dt)
            if switch is None:
                assert info['tiles'] == 0 and info['oversize'] == 1 and not info['em_uses_tiles'], info
        os.environ.pop('SKM_EM_NO_COMPONENTS', None)
        print('%s: %d transcripts, %d classes, %d pairs, one component: handle set-up %.3f ms with the components, '
              '%.3f ms without: %.3f ms for labels and tiles that are not used'
              % (kind, n_tx, offsets.size - 1, targets.size, best[None] * 1e3, best['1'] * 1e3, (best[None] - best['1']) * 1e3),
              flush=True)


if __name__ == '__main__':
    main()
