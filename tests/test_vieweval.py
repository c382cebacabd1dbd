"""CPU: the definition behind objnerf_view_compare (tests/vieweval_util.py) and the host side of
openobj_amd/map_view_eval.py -- the tap table, the deviation of the integer-tap SSIM from the canonical float-tap one,
result()'s derived figures, the lut rules, the CLI's argument errors and the --renders reader."""
import math
import os
import re

import numpy as np
import pytest
import torch

import vieweval_util as U
from conftest import ROOT
from openobj_amd import map_view, map_view_eval as E, ops
from openobj_amd.render_view import ViewBuffers

# The largest per-pixel |integer-tap SSIM - float-tap SSIM| over PAIRS below is 6.03e-5 (the noisy 33 x 47 pair; the
# smooth pairs give 3.6e-6, the inverted ones 1.4e-5, constant images 1.5e-13).  The bound is four times that: the
# margin is for image content the pairs do not cover.  DESIGN.md 4.26 quotes both.
MEASURED = 6.03e-5
BOUND = 4 * MEASURED
PAIRS = [(kind, W, H) for kind in ("smooth", "noisy", "inverted", "constant") for (W, H) in ((80, 60), (33, 47))]


def test_taps():
    g = U.gaussian()
    t = np.asarray(U.TAPS)
    assert list(E.TAPS) == U.TAPS
    assert int(t.sum()) == 65536 and np.array_equal(t, t[::-1])
    assert float(np.abs(t - 65536 * g).max()) < 1.0
    want = np.rint(65536 * g).astype(int)
    want[5] += 1
    assert np.array_equal(t, want)


def test_first_pass_fits_32_bits():
    assert sum(U.TAPS) * 255 * 255 == 4261478400 < 2 ** 32
    x, y = U.images(11, 11, "extreme")
    q, value = U.integer_ssim(y, y)                       # all 255 against itself: the largest moments
    assert int(q[5, 5]) == 2 ** 32 and float(value[5, 5]) == 1.0
    assert 65536 * 65536 * 65025 < 2 ** 48


@pytest.mark.parametrize("kind,W,H", PAIRS)
def test_integer_taps_stay_close_to_the_canonical_ssim(kind, W, H):
    x, y = U.images(W, H, kind, seed=3)
    q, value = U.integer_ssim(x, y)
    canon = U.float_ssim(x, y)
    dev = float((value[5:W - 5, 5:H - 5] - canon).abs().max())
    mean_dev = abs(float(value[5:W - 5, 5:H - 5].mean() - canon.mean()))
    print(f"\n{kind} {W} x {H}: per pixel {dev:.3e}, mean {mean_dev:.3e}, SSIM {float(canon.mean()):.5f}")
    assert dev < BOUND
    assert torch.equal(q[5:W - 5, 5:H - 5], torch.floor(value[5:W - 5, 5:H - 5] * 2.0 ** 32).long())


def test_identical_and_inverted_images():
    x, _ = U.images(20, 17, "identical", seed=1)
    q, value = U.integer_ssim(x, x)
    assert bool((q[5:15, 5:12] == 2 ** 32).all()) and bool((q[:5] == 0).all()) and bool(torch.isnan(value[:5]).all())
    q, _ = U.integer_ssim(x, 255 - x)
    assert int(q[5:15, 5:12].max()) < 0
    q, value = U.integer_ssim(x[:10], x[:10])             # W < 11: no interior
    assert not bool(q.any()) and bool(torch.isnan(value).all())


def test_lut_rules():
    lut = E.build_lut([7, 3, 0])
    assert lut.dtype == np.int32 and lut.tolist() == [2, -1, -1, 1, -1, -1, -1, 0]
    for bad in ([], [1, 1], [-1, 2], [E.MAX_ID]):
        with pytest.raises(ValueError):
            E.build_lut(bad)
    ids = torch.tensor([-5, -1, 0, 3, 7, 8, 1 << 30, 2])
    assert U.rows_of(ids, lut, 3).tolist() == [3, 3, 2, 1, 0, 3, 3, 3]
    assert U.rows_of(ids, lut, 2).tolist() == [2, 2, 2, 1, 0, 2, 2, 2]         # a lut entry >= G has no row either
    assert U.rows_of(ids, np.zeros(0, np.int32), 2).tolist() == [2] * 8


def test_the_specification_tables_add_up():
    W, H, G = 23, 19, 3
    x, y = U.images(W, H, "noisy", seed=5)
    dr, dg = U.depths(W, H)
    ir, ig = U.id_images(W, H, [0, 3, 7, 9, -1])
    s = U.compare(x, dr, ir, None, y, dg, ig, E.build_lut([7, 3, 0]), G)
    acc, conf = s["acc"], s["conf"]
    assert int(acc[:, 0].sum()) == W * H == int(acc[:, 1].sum()) and int(acc[:, 7].sum()) == (W - 10) * (H - 10)
    assert torch.equal(acc[:, 2], acc[:, 3]) and torch.equal(conf.sum(1), acc[:G, 0])
    assert int(acc[:, 8].sum()) == int(s["q"].sum()) and 0 < int(acc[:, 5].sum()) < int(acc[:, 4].sum()) < W * H
    assert int(acc[G, 0]) == int(((ig == 9) | (ig == -1)).sum())


def test_result_figures_from_hand_made_tables():
    ev = E.ViewEval([3, 7], "cpu")
    half_metre = 40 * (1 << 20) // 2
    ev.acc = torch.tensor([[100, 50, 0, 0, 80, 40, half_metre, 10, 10 << 32],
                           [0] * 9,
                           [200, 0, 390150, 0, 0, 0, 0, 4, -(1 << 31)]], dtype=torch.int64)
    ev.conf = torch.tensor([[60, 30, 10], [0, 0, 0]], dtype=torch.int64)
    r = ev.result()
    a = r["per_id"][3]
    assert a["psnr"] == math.inf and a["psnr_painted"] == math.inf and a["ssim"] == 1.0 and a["depth_l1"] == 0.5
    assert a["depth_coverage"] == 0.5 and a["painted_share"] == 0.5 and a["iou"] == 0.6
    b = r["per_id"][7]                                     # an empty row: NaN throughout, IoU 0 (predicted, never true)
    assert all(math.isnan(b[k]) for k in ("psnr", "psnr_painted", "ssim", "depth_l1", "depth_coverage", "painted_share"))
    assert b["iou"] == 0.0
    o = r["other"]
    assert o["psnr"] == 20.0 and math.isnan(o["psnr_painted"]) and o["ssim"] == -0.125 and o["painted_share"] == 0.0
    assert math.isnan(o["depth_l1"]) and math.isnan(o["depth_coverage"])
    img = r["image"]
    assert img["psnr"] == 10.0 * math.log10(65025.0 * 3.0 * 300.0 / 390150.0)
    assert img["ssim"] == float((10 << 32) - (1 << 31)) / (14.0 * 2.0 ** 32) and img["depth_l1"] == 0.5
    assert img["depth_coverage"] == 0.5 and img["painted_share"] == 50.0 / 300.0
    assert r["miou"] == 0.3 and r["accuracy"] == 0.6 and r["ids"] == [3, 7] and r["iou"] == [0.6, 0.0]
    assert r["acc"].dtype == np.int64 and np.array_equal(r["acc"], ev.acc.numpy()) and np.array_equal(r["conf"], ev.conf.numpy())
    ev.depth_scored = False                                # what add_images(depth_r=None) leaves
    r = ev.result()
    assert r["image"]["depth_l1"] is None and r["per_id"][3]["depth_coverage"] is None and r["image"]["psnr"] == img["psnr"]
    plain = E._plain(ev.result())
    assert plain["per_id"]["7"]["psnr"] is None and plain["per_id"]["3"]["psnr"] == "inf" and plain["acc"][0][8] == 10 << 32
    with pytest.raises(ValueError):
        E.derive(np.zeros((3, 9), np.int64), np.zeros((2, 2), np.int64), [3, 7])


def test_exported_constants_match_the_header():
    src = open(os.path.join(ROOT, "include", "objnerf_hip.h")).read()
    val = lambda n: int(re.search(r"#define %s (\d+)" % n, src).group(1))
    assert val("OBJNERF_VIEW_EVAL_TILE") == ops.VIEW_EVAL_TILE
    assert val("OBJNERF_VIEW_EVAL_LDS_ROWS") == ops.VIEW_EVAL_LDS_ROWS
    assert val("OBJNERF_VIEW_EVAL_MAX_ROWS") == ops.VIEW_EVAL_MAX_ROWS
    assert ",".join(map(str, U.TAPS)) in src.replace(" ", "")


def test_view_compare_has_no_cpu_path():
    from openobj_amd import _lib
    z = torch.zeros(11, 11, 3, dtype=torch.uint8)
    with pytest.raises(_lib.ObjnerfError):
        ops.view_compare(z, torch.zeros(11, 11), torch.zeros(11, 11, dtype=torch.int32), None, z, torch.zeros(11, 11),
                         torch.zeros(11, 11, dtype=torch.int32), torch.zeros(1, dtype=torch.int32), 1,
                         torch.zeros(2, 9, dtype=torch.int64))


@pytest.mark.parametrize("argv", [
    ["--config", "c.json", "--out", "o"],                                                      # no --logdir
    ["--logdir", "l", "--config", "c.json"],                                                  # no --out
    ["--logdir", "l", "--config", "c.json", "--out", "o", "--depth-scale", "1000"],           # nothing to scale
    ["--logdir", "l", "--config", "c.json", "--out", "o", "--renders", ".", "--write-images"],
    ["--logdir", "l", "--config", "c.json", "--out", "o", "--renders", "no/such/dir"],
    ["--logdir", "l", "--config", "c.json", "--out", "o", "--renders", ".", "--depth-scale", "0"],
    ["--logdir", "l", "--config", "c.json", "--out", "o", "--frames", "1:2:3:4"],
])
def test_cli_argument_errors(argv, capsys):
    with pytest.raises(SystemExit) as e:
        E.main(argv)
    assert e.value.code == 2 and "error:" in capsys.readouterr().err


def test_renders_reader_reads_what_write_view_writes(tmp_path):
    W, H = 13, 9
    g = torch.Generator().manual_seed(0)
    buf = ViewBuffers.__new__(ViewBuffers)
    buf.rgb = torch.randint(0, 256, (W, H, 3), generator=g, dtype=torch.uint8).numpy()
    buf.maskid = torch.randint(0, 300, (W, H), generator=g, dtype=torch.int32).numpy()
    buf.depth = (6 * torch.rand(W, H, generator=g)).numpy().astype(np.float32)
    buf.depth[2, 3] = 100.0
    map_view.write_view(str(tmp_path / "a"), 7, buf)                     # 8-bit depth
    map_view.write_view(str(tmp_path / "b"), 7, buf, depth_scale=1000.0)
    rgb, depth, mid = E.read_view(str(tmp_path / "a"), 7, None)
    assert rgb.dtype == np.uint8 and np.array_equal(rgb, buf.rgb) and depth is None
    assert mid.dtype == np.int32 and np.array_equal(mid, buf.maskid & 255)          # ids above 255 wrapped in the file
    rgb, depth, mid = E.read_view(str(tmp_path / "b"), 7, 1000.0)
    assert np.array_equal(rgb, buf.rgb) and depth.dtype == np.float32 and depth.shape == (W, H) and depth.flags.c_contiguous
    assert depth[2, 3] == 100.0                                          # the saturated 65535 = nothing wrote depth
    keep = buf.depth < 100
    assert float(np.abs(depth[keep] - buf.depth[keep]).max()) <= 0.5e-3 + 1e-6
    with pytest.raises(ValueError):
        E.read_view(str(tmp_path / "a"), 7, 1000.0)                      # 8-bit files cannot be scaled
    with pytest.raises(FileNotFoundError):
        E.read_view(str(tmp_path / "a"), 8, None)
    png = E.ssim_png(np.array([[np.nan, 1.0, 0.5], [-0.2, 0.0, 2.0]]))
    assert png.shape == (3, 2) and png.dtype == np.uint8 and png.T.tolist() == [[0, 255, 128], [0, 0, 255]]
