"""The weight-gradient k-slot maps of the fp32 fused training kernel (objnerf_train32.hip: wg_pair over both rays of a
two-ray tile, wg_pair_ray over one of them alone) and the per-ray rule by which its S = 64 skipping instantiation runs the
weight-gradient rounds, restated in tools/masked_work.py (wg_column, wg_ray_column, expected_mfma_rays)
and held here against a brute-force walk over every (object, tile, wave, round, step, lane group).  No GPU."""
import importlib.util
import os

import numpy as np
import pytest

_spec = importlib.util.spec_from_file_location(
    "masked_work", os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools", "masked_work.py"))
mw = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(mw)

PAIRS = [(1, 2), (2, 1), (0, 2), (2, 0), (1, 0), (0, 1), (0, 0), (2, 2), (1, 1)]


def pair_labels():
    """[2, 19]: every pair of labels as the two rays of a tile, object 1 in reversed pair order; the last tile has one ray."""
    lab = np.zeros((2, 19), np.uint8)
    lab[0, :18] = np.array(PAIRS, np.uint8).reshape(-1)
    lab[1, :18] = np.array(PAIRS[::-1], np.uint8).reshape(-1)
    lab[0, 18], lab[1, 18] = 1, 0
    return lab


# (round, wave) -> "col" (a colour pair: d_hc is zero unless the ray is this object's), "any" (zero only for label 2) or None
def _round_kind(rnd, w):
    if rnd == "A":
        return "col" if w < 5 else ("any" if w < 7 else None)
    return "any"


def _chain(cols_of_step, steps):
    """Samples in the order an accumulator takes them in: step by step, lane groups 0..3 inside a step."""
    return [cols_of_step(st, g) for st in range(steps) for g in range(4)]


def test_one_ray_loop_is_the_full_loop_without_the_other_rays_slots():
    full = _chain(mw.wg_column, 32)
    assert sorted(full) == list(range(128))
    for h in range(2):
        ray = _chain(lambda j, g: mw.wg_ray_column(j, g, h), 16)
        assert sorted(ray) == list(range(64 * h, 64 * h + 64))            # every sample of ray h once, none of the other
        assert ray == [c for c in full if c // 64 == h]                    # in the order the full chain takes them in
        # groups g and g + 2 read one aligned pair of columns (8-byte reads have 64 banks and are served by half waves): the
        # half wave g = 0, 1 covers the 64 banks once with the 130-float pitch, the half wave g = 2, 3 repeats its addresses
        pair = lambda c, g: 130 * c + mw.wg_ray_column(0, g, h) - (g >> 1)
        assert all(pair(c, g) % 2 == 0 and pair(c, g) == pair(c, g + 2) for c in range(16) for g in range(2))
        assert sorted((pair(c, g) + d) % 64 for c in range(16) for g in range(2) for d in range(2)) == list(range(64))


def test_left_out_slots_are_zero_contributions_and_the_count_matches():
    lab = pair_labels()
    S = 64
    sl = mw.slot_labels(lab, S)                       # [K, NT, 128]
    K, NT, _ = sl.shape
    assert NT == 10 and (sl[:, 9, 64:] == 2).all()    # one ray in the last tile
    seen = set()
    total = 0
    for k in range(K):
        for t in range(NT):
            ray = [int(sl[k, t, 0]), int(sl[k, t, 64])]
            seen.add(tuple(ray))
            for w in range(8):
                mine = ray[w >> 2]
                total += 0 if mine == 2 else (376 if mine == 1 else 376 - 80)
                for rnd in "ABC":
                    kind = _round_kind(rnd, w)
                    if kind is None:
                        continue
                    live = [(r == 1) if kind == "col" else (r != 2) for r in ray]
                    if all(live):
                        read = set(_chain(mw.wg_column, 32))
                        total += 64
                    elif any(live):
                        h = live.index(True)
                        read = set(_chain(lambda j, g: mw.wg_ray_column(j, g, h), 16))
                        total += 32
                    else:
                        read = set()
                    for col in set(range(128)) - read:                  # every slot left out gives an exact zero
                        v = int(sl[k, t, col])
                        assert (v != 1) if kind == "col" else (v == 2)
                    for ww in range(8):                                  # nothing reads a dead wave's columns
                        if int(sl[k, t, 16 * ww]) != 2:
                            continue
                        assert not (read & set(range(16 * ww, 16 * ww + 16)))
    assert seen >= set(PAIRS)
    m = mw.expected_mfma_rays(lab, S)
    assert m["with_skips"] == total and m["full"] == K * NT * 8 * 560
    assert m["with_skips"] < mw.expected_mfma(lab, S)["with_skips"]


@pytest.mark.parametrize("S,R", [(10, 29), (33, 10)])
def test_other_sample_counts_keep_the_per_tile_rule(S, R):
    rs = np.random.RandomState(S)
    lab = rs.choice(np.array([0, 1, 2], np.uint8), size=(3, R), p=[0.35, 0.3, 0.35])
    lab[0, : R // 2] = 2
    assert mw.expected_mfma_rays(lab, S) == mw.expected_mfma(lab, S)


def test_expected_ratio_at_the_benchmark_mix():
    """55 / 35 / 10 at S = 64: a wave loses its forward pass and input gradients (376) with probability 0.10 and their
    colour part (40 + 40) with 0.35; a half of a tile pair is one ray's, so the 184 weight-gradient MFMAs per wave fall by
    0.10 and the 40 of them that are the colour pairs' by a further 0.35: 462 of 560 = 0.825."""
    rs = np.random.RandomState(1)
    u = rs.rand(50, 4096)
    lab = np.where(u < 0.55, 1, np.where(u < 0.90, 0, 2)).astype(np.uint8)
    r = mw.expected_mfma_rays(lab, 64)["ratio"]
    assert abs(r - (560 - 0.10 * 376 - 0.35 * 80 - 0.10 * 184 - 0.35 * 40) / 560) < 5e-3
    assert mw.expected_mfma_rays(np.ones((2, 8), np.uint8), 64)["ratio"] == 1.0
    assert mw.expected_mfma_rays(np.full((2, 8), 2, np.uint8), 64)["with_skips"] == 0
