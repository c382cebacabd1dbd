#!/usr/bin/env python3
"""What the fp32 fused training kernel (train_fused32_kernel, no feature loss) leaves out for rays the loss masks out,
restated on the host, and the time of the step under chosen label mixes.

Host part (no GPU; tests/test_masked_rays.py holds it against a brute-force restatement):

  predicates(labels [K,R], S)   -> wave_dead / wave_nocol [K,NT,8], tile_dead / tile_nocol [K,NT]
  expected_mfma(labels, S)      -> MFMA instructions (per wave) of one launch with and without the skips, weight-gradient
                                   rounds left out per tile (the kernel's rule at S != 64)
  expected_mfma_rays(labels, S) -> the kernel's count: at S = 64 the rounds are left out per ray (below)
  wg_column(st, g)              -> staged sample column that weight-gradient MFMA step st reads in lane group g
  wg_ray_column(j, g, h)        -> the same for step j of the 16 that run over ray h of a two-ray tile alone

A tile is 128 sample slots = 128 // S rays (a slot behind the last ray of the tile, or behind ray R - 1, has no ray and
counts as label 2); wave w of the eight holds slots 16 w .. 16 w + 15.

  wave_dead    every slot of the wave is label 2          no forward pass, no input gradients
  wave_nocol   every slot of the wave is label 0 or 2     no colour layer, forward or backward
  tile_nocol   every ray of the tile is label 0 or 2      round A runs only the two mid2 tile pairs
  tile_dead    every ray of the tile is label 2           the tile is skipped

At S = 64 a tile is two rays (columns 0..63 and 64..127).  A tile pair is 32 steps x 2 accumulators; step st adds the
samples of lane groups 0..3 (wg_column) to the accumulator one after the other.  Where only ray h of the tile has
something to give, the other ray's slots add exact zeros, and the kernel runs the live slots alone, four to an MFMA, in the
same order (wg_ray_column): 16 steps x 2, the same bits.  Per tile pair:

  colour pairs (round A, waves 0..4)       32 MFMAs per ray that is label 1
  mid2 pairs (waves 5, 6), rounds B, C     32 MFMAs per ray that is not label 2

MFMAs per wave and tile, from the kernel's source (objnerf_mlp32.h mlp32_trunk, objnerf_train32.hip phases A / B and the
weight-gradient rounds): forward 184 of which the colour layer 40, input gradients 192 of which 40, weight gradients
64 per tile pair: round A 5 colour pairs (waves 0..4) + 2 mid2 pairs (waves 5, 6), rounds B and C 8 pairs each.

GPU part:  python tools/masked_work.py [--steps N] [--out FILE]
times ops.train_step at the benchmark's c2 shape (50 x 4096 x 64, the benchmark's first batch) with its labels replaced
by: all 1 (nothing to skip: the price of the predicates), the benchmark's own 55 / 35 / 10, all 0, 45 % label 2.
"""
import argparse
import json
import os
import sys

import numpy as np

TS, NWAVE = 128, 8
FWD, FWD_COL = 184, 40
DGRAD, DGRAD_COL = 192, 40
PAIR = 64                       # MFMAs of one weight-gradient tile pair (32 k-steps x 2 accumulators)
ROUND_A_COL, ROUND_A_MID2, ROUND_B, ROUND_C = 5, 2, 8, 8
FULL_PER_TILE = NWAVE * (FWD + DGRAD) + PAIR * (ROUND_A_COL + ROUND_A_MID2 + ROUND_B + ROUND_C)


def tile_geometry(R, S):
    """(rays per tile, tiles per object) as objnerf_train_step lays them out."""
    assert 1 <= S <= 64
    TR = TS // S
    return TR, (R + TR - 1) // TR


def slot_labels(labels, S):
    """[K, NT, 128] uint8: the label of every sample slot (2 where the slot has no ray)."""
    labels = np.asarray(labels)
    K, R = labels.shape
    TR, NT = tile_geometry(R, S)
    slot = np.arange(TS)
    q = slot // S
    ray = np.arange(NT)[:, None] * TR + q[None, :]                 # [NT, 128]
    ok = (q[None, :] < TR) & (ray < R)
    out = np.full((K, NT, TS), 2, np.uint8)
    out[:, ok] = labels[:, ray[ok]]
    return out


def predicates(labels, S):
    sl = slot_labels(labels, S)
    K, NT, _ = sl.shape
    per_wave = sl.reshape(K, NT, NWAVE, TS // NWAVE)
    return dict(wave_dead=(per_wave == 2).all(-1), wave_nocol=(per_wave != 1).all(-1),
                tile_dead=(sl == 2).all(-1), tile_nocol=(sl != 1).all(-1))


def expected_mfma(labels, S):
    """MFMA instructions per launch, summed over waves: dict(full, with_skips, ratio): the count without and with the skips."""
    p = predicates(labels, S)
    K, NT = p["tile_dead"].shape
    live_tile = ~p["tile_dead"]
    dead = p["wave_dead"]
    nocol = p["wave_nocol"] & ~dead
    full_w = ~p["wave_nocol"]
    per_wave = full_w * (FWD + DGRAD) + nocol * (FWD - FWD_COL + DGRAD - DGRAD_COL)      # dead waves: 0
    chain = (per_wave.sum(-1) * live_tile).sum()
    rounds = (live_tile * PAIR * (ROUND_A_MID2 + ROUND_B + ROUND_C)).sum() + \
             (live_tile & ~p["tile_nocol"]).sum() * PAIR * ROUND_A_COL
    full = K * NT * FULL_PER_TILE
    return dict(full=int(full), with_skips=int(chain + rounds), ratio=float(chain + rounds) / float(full))


def wg_column(st, g):
    """Column (sample slot of the tile) of MFMA k-slot (step st of 32, lane group g of 4) in wg_pair / wg_half /
    wg_quarter of objnerf_train32.hip."""
    return 32 * g + st


def wg_ray_column(j, g, h):
    """Column of MFMA k-slot (step j of 16, lane group g) in wg_pair_ray over ray h of a two-ray tile."""
    return 64 * h + 32 * (g & 1) + 2 * j + (g >> 1)


def expected_mfma_rays(labels, S):
    """expected_mfma with the weight-gradient rounds as the kernel runs them: 32 MFMAs per pair and contributing ray of the
    tile at S = 64, per tile otherwise."""
    if S != 64:
        return expected_mfma(labels, S)
    p = predicates(labels, S)
    sl = slot_labels(labels, S)
    K, NT, _ = sl.shape
    ray = sl[:, :, ::S]                                    # [K, NT, 2]: the label of ray h of the tile (2: no such ray)
    dead = p["wave_dead"]
    nocol = p["wave_nocol"] & ~dead
    per_wave = (~p["wave_nocol"]) * (FWD + DGRAD) + nocol * (FWD - FWD_COL + DGRAD - DGRAD_COL)
    chain = per_wave.sum()                                 # (a dead tile has only dead waves)
    half = PAIR // 2
    rounds = (ray == 1).sum() * half * ROUND_A_COL + (ray != 2).sum() * half * (ROUND_A_MID2 + ROUND_B + ROUND_C)
    full = K * NT * FULL_PER_TILE
    return dict(full=int(full), with_skips=int(chain + rounds), ratio=float(chain + rounds) / float(full))


MIXES = ("all1", "bench", "all0", "unknown45")


def mix_labels(name, bench_labels, seed=0):
    lab = np.array(bench_labels, copy=True)
    if name == "all1":
        lab[:] = 1
    elif name == "all0":
        lab[:] = 0
        lab[:, 0] = 1                         # (one counted ray per object keeps the cross-object early return out)
    elif name == "unknown45":
        u = np.random.RandomState(seed).rand(*lab.shape)
        lab[:] = np.where(u < 0.45, 2, 1)
        lab[:, 0] = 1
    elif name != "bench":
        raise ValueError(name)
    return lab


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch
    from openobj_amd import init as obj_init, ops, synthetic
    dev = torch.device("cuda:0")
    K, R, n1, n2 = 50, 4096, 16, 48
    S = n1 + n2
    arena = ops.ParamArena(K, ops.NetShape(32, 512, 6), dev)
    arena.load_stacked(obj_init.init_stacked(K, 32, 512, seed=1000))
    b = synthetic.random_batch(K, R, n1, n2, seed=4242)
    keys = ["pts", "z", "gt_depth", "gt_rgb"]
    base = {k: torch.from_numpy(b[k]).to(dev) for k in keys}
    ws = ops.TrainWorkspace(arena, K, R, S, False)
    lines = []
    for name in MIXES:
        lab = mix_labels(name, b["labels"])
        batch = dict(base, labels=torch.from_numpy(lab).to(dev))
        for _ in range(args.warmup):
            ops.train_step(arena, ws, batch)
        torch.cuda.synchronize()
        ev = []
        for _ in range(args.steps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            ops.train_step(arena, ws, batch)
            e1.record()
            ev.append((e0, e1))
        torch.cuda.synchronize()
        ms = sorted(e0.elapsed_time(e1) for e0, e1 in ev)
        m = expected_mfma_rays(lab, S)
        lines.append(dict(mix=name, step_ms_median=round(ms[len(ms) // 2], 4), step_ms_min=round(ms[0], 4),
                          step_ms_max=round(ms[-1], 4), mfma_ratio_expected=round(m["ratio"], 4),
                          status=int(ws.status.item())))
        print(json.dumps(lines[-1]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
