"""The replay argument behind orbfe_fuse_search_keyframes, pinned on the CPU with the oracle on both sides (tests/neighbors_model.py):
searching all K targets of a SearchInNeighbors loop on the state at the START of the loop, masking the pairs that are skipped by
the time their turn comes and re-searching only the points whose descriptor changed, gives the per-target results and the final
graph of the K sequential searches.  Here the dirty points are re-searched with the oracle (it returns no candidate lists); the
scenes must really exercise the argument: points go bad mid-loop, descriptors change, and the start-of-loop rows of dirty points
are really stale."""
import numpy as np
import pytest

import neighbors_model as NM

K, M, TH = 20, 1200, 10.0


def _run(name):
    sc = NM.scene(seed=5, K=K, M=M)
    kw = NM.SCENES[name]
    seq, final_seq, st = NM.sequential(sc, TH, **kw)

    def search_all(mps):
        return [NM.oracle_search(sc, TH, mps, k) for k in range(K)]

    def resolve(k, dirty, mps):
        return NM.oracle_search(sc, TH, mps, k, dirty)

    used, final_rep, st2, cnt = NM.replay(sc, TH, search_all, resolve, **kw)
    for k in range(K):
        assert np.array_equal(used[k][0], seq[k][0]) and np.array_equal(used[k][1], seq[k][1]), "target %d" % k
    assert final_rep == final_seq and st2 == st
    print(name, st, cnt)
    return st, cnt


def test_replay_equals_sequential_default_scene(built):
    st, cnt = _run("default")
    assert st["fused"] >= 2000 and st["bad"] >= 100 and st["dirty"] >= 100 and cnt["stale_differs"] >= 100


def test_replay_equals_sequential_sparse_scene(built):
    st, cnt = _run("sparse")
    assert st["dirty"] >= 10
