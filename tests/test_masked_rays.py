"""tools/masked_work.py, host part: the per-wave and per-tile predicates by which the fp32 fused training kernel leaves
out the work of rays the loss masks out, and the MFMA count it expects per launch, against a
brute-force restatement that walks every (object, tile, wave, lane).  S = 64 is the compile-time instantiation (two rays
per tile, a wave inside one ray), 10 / 16 / 33 the any-S one (12 / 8 / 3 rays per tile; at 10 and 33 waves straddle
rays, at 33 the tile's last 29 slots have no ray); every R leaves a ragged last tile."""
import importlib.util
import os

import numpy as np
import pytest

_spec = importlib.util.spec_from_file_location(
    "masked_work", os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools", "masked_work.py"))
mw = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(mw)


def _brute(labels, S):
    K, R = labels.shape
    TR = 128 // S
    NT = (R + TR - 1) // TR
    wave_dead = np.zeros((K, NT, 8), bool)
    wave_nocol = np.zeros((K, NT, 8), bool)
    tile_dead = np.zeros((K, NT), bool)
    tile_nocol = np.zeros((K, NT), bool)
    total = 0
    for k in range(K):
        for t in range(NT):
            rays = [r for r in range(t * TR, (t + 1) * TR) if r < R]
            tile_dead[k, t] = all(labels[k, r] == 2 for r in rays)
            tile_nocol[k, t] = all(labels[k, r] != 1 for r in rays)
            for w in range(8):
                labs = []
                for lane in range(64):
                    slot = 16 * w + (lane & 15)          # the four lane groups of a wave share its 16 samples
                    q = slot // S
                    ray = t * TR + q
                    labs.append(int(labels[k, ray]) if (q < TR and ray < R) else 2)
                wave_dead[k, t, w] = all(v == 2 for v in labs)
                wave_nocol[k, t, w] = all(v != 1 for v in labs)
            if tile_dead[k, t]:
                continue
            for w in range(8):
                if wave_dead[k, t, w]:
                    pass
                elif wave_nocol[k, t, w]:
                    total += (184 - 40) + (192 - 40)
                else:
                    total += 184 + 192
                # weight gradients: round A (colour pairs on waves 0..4, mid2 on 5, 6), rounds B and C on every wave
                if w < 5:
                    total += 0 if tile_nocol[k, t] else 64
                elif w < 7:
                    total += 64
                total += 128
    return dict(wave_dead=wave_dead, wave_nocol=wave_nocol, tile_dead=tile_dead, tile_nocol=tile_nocol), total, K * NT * 8 * 560


def _labels(K, R, seed):
    rs = np.random.RandomState(seed)
    lab = rs.choice(np.array([0, 1, 2], np.uint8), size=(K, R), p=[0.35, 0.3, 0.35])
    lab[0, : R // 2] = 2                 # runs of unknown rays: dead waves and dead tiles at every S
    lab[1, R // 3:] = 0
    return lab


@pytest.mark.parametrize("S,R", [(64, 13), (10, 29), (16, 19), (33, 10)])
def test_predicates_and_mfma_count_against_brute_force(S, R):
    lab = _labels(3, R, seed=S)
    want, total, full = _brute(lab, S)
    got = mw.predicates(lab, S)
    for name in want:
        assert np.array_equal(got[name], want[name]), name
    m = mw.expected_mfma(lab, S)
    assert m["full"] == full and m["with_skips"] == total
    assert want["wave_dead"].any() and (want["wave_nocol"] & ~want["wave_dead"]).any() and want["tile_nocol"].any()


def test_expected_ratio_at_the_benchmark_mix():
    """55 / 35 / 10 at S = 64 (two rays per tile, independent labels): 560 - 0.10 * 376 - 0.35 * 80 - 0.2025 * 40
    - 0.01 * 144 of 560 = 0.866; the sample of 50 x 4096 rays is within half a per cent of it.  All label 1: nothing left out."""
    rs = np.random.RandomState(1)
    u = rs.rand(50, 4096)
    lab = np.where(u < 0.55, 1, np.where(u < 0.90, 0, 2)).astype(np.uint8)
    r = mw.expected_mfma(lab, 64)["ratio"]
    assert abs(r - (560 - 0.10 * 376 - 0.35 * 80 - 0.2025 * 40 - 0.01 * 144) / 560) < 5e-3
    assert mw.expected_mfma(np.ones((2, 8), np.uint8), 64)["ratio"] == 1.0
    dead = mw.expected_mfma(np.full((2, 8), 2, np.uint8), 64)
    assert dead["with_skips"] == 0
