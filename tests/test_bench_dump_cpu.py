"""bench.py --dump-outputs: drive StepRunner on CPU tensors with a stub in place of the HIP calls (same buffer layout) and check what
dump_outputs writes -- the last step's results, integers exact in float32 / float64, nothing of what the buffers held past a frame's
count, a sample of the frames that depends on the arguments only, and at most 64 MB at the headline batch."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "orb_slam3_v1.0_amd", "python"))


def _runner(B, cap, nl, M):
    import bench
    import orbfe
    rng = np.random.default_rng(5)
    counts = rng.integers(0, cap + 1, B)

    def extract_fn(b, fs):
        if fs == 0:  # the first step fills every slot: what a later step leaves past its counts is stale
            b["n"][:] = cap
            b["kp"][:] = 7
            b["desc"][:] = 9
            b["per"][:] = 1
            return
        for i in range(B):
            n = int(counts[i])
            b["n"][i] = n
            b["per"][i] = torch.arange(nl, dtype=torch.int32) + i
            kp = np.zeros(n, orbfe.KP_DTYPE)
            kp["x"], kp["y"] = np.arange(n) + 0.25, i + 0.5
            kp["response"], kp["size"], kp["octave"], kp["angle"] = np.arange(n) * 3, 31.0, np.arange(n) % nl, 359.5
            b["kp"][i, :n] = torch.from_numpy(kp.view(np.uint8).reshape(n, 24))
            b["desc"][i, :n] = torch.from_numpy(((np.arange(n * 32) + i) % 256).astype(np.uint8).reshape(n, 32))

    def match_fn(b, fs):
        if fs == 0:
            b["match"][:] = 5
            b["nmatch"][:] = cap
            return
        for i in range(B):
            n = int(counts[i])
            b["match"][i, :n] = torch.from_numpy(np.where(np.arange(n) % 3 == 0, -1, np.arange(n) % M).astype(np.int32))
            b["nmatch"][i] = int((np.arange(n) % 3 != 0).sum())

    r = bench.StepRunner(torch.device("cpu"), B, cap, nl, extract_fn, match_fn, None, 1, False, True, frame_sets=2)
    r.step()
    r.step()
    assert r.last[1] == 1
    return r, counts


def _load(path):
    return {f[:-4]: np.load(os.path.join(path, f)) for f in sorted(os.listdir(path))}


def test_dump_outputs_writes_the_last_step_exactly(tmp_path):
    import bench
    B, cap, nl, M = 6, 40, 3, 50
    r, counts = _runner(B, cap, nl, M)
    bench.dump_outputs(str(tmp_path), r, B, cap, nl, M)
    d = _load(tmp_path)
    assert set(d) == {"n_keypoints", "keypoints_per_level", "n_matches", "keypoints", "descriptors", "matches"}
    assert all(a.dtype in (np.float32, np.float64) for a in d.values())
    assert np.array_equal(d["n_keypoints"], counts) and d["keypoints"].shape == (B, cap, 6) and d["descriptors"].shape == (B, cap, 32)
    assert np.array_equal(d["keypoints_per_level"], np.arange(nl)[None, :] + np.arange(B)[:, None])
    for i in range(B):
        n = int(counts[i])
        k = d["keypoints"][i]
        assert np.array_equal(k[:n, 0], np.arange(n) + 0.25) and (k[:n, 1] == i + 0.5).all() and (k[:n, 2] == 31.0).all()
        assert (k[:n, 3] == 359.5).all() and np.array_equal(k[:n, 4], np.arange(n) * 3) and np.array_equal(k[:n, 5], np.arange(n) % nl)
        assert np.array_equal(d["descriptors"][i, :n].reshape(-1), (np.arange(n * 32) + i) % 256)
        assert np.array_equal(d["matches"][i, :n], np.where(np.arange(n) % 3 == 0, -1, np.arange(n) % M))
        assert d["n_matches"][i] == (d["matches"][i] >= 0).sum()
        # past the count: nothing of the first step's stale slots
        assert (k[n:] == 0).all() and (d["descriptors"][i, n:] == 0).all() and (d["matches"][i, n:] == -1).all()


def test_dump_of_the_headline_batch_is_a_fixed_sample_within_64_mb(tmp_path):
    import bench
    B, cap, nl, M = 512, 1024, 8, 2000  # the default workload: 512 frames, cap = 1000 + 3 x 8
    idx = bench.dump_sample(B, cap, nl)
    assert 0 < len(idx) < B and np.array_equal(idx, np.unique(idx)) and np.array_equal(idx, bench.dump_sample(B, cap, nl))
    assert np.array_equal(bench.dump_sample(16, cap, nl), np.arange(16))
    r, counts = _runner(B, cap, nl, M)
    bench.dump_outputs(str(tmp_path), r, B, cap, nl, M)
    assert sum(os.path.getsize(os.path.join(tmp_path, f)) for f in os.listdir(tmp_path)) <= 64e6
    d = _load(tmp_path)
    assert d["keypoints"].shape == (len(idx), cap, 6) and d["n_keypoints"].shape == (B,)
    j = len(idx) // 2
    n = int(counts[idx[j]])
    assert (d["keypoints"][j, :n, 1] == idx[j] + 0.5).all() and (d["keypoints"][j, n:] == 0).all()
