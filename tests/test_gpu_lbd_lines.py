"""GPU parity of the line descriptor kernel (k_lbd) on lines chosen for ITS paths: sample counts on both sides of every trip, tail and chunk edge, all
eight directions, bands that lie inside the image, touch its border or leave it (the kernel picks a clamp-free loop per line), more lines in a frame than
the frame has waves, frames of unequal line counts in one batch, and a frame size whose last Sobel tiles are partial.  tests/lbd_line_frames.py draws
the frames: bright bars on a flat background, so that most of every band projects to zeros of both signs.  Every frame goes through
test_gpu_line.compare_stages against oracle_lib.LineOracle (DBG_ALL_LBD at Hamming distance 0, the kept rows, every earlier stage); each test first
asserts on the ORACLE's output that the frames contain the cases it is about.  Stable seed order, automatic growing mode: the descriptor depends on neither."""
import numpy as np
import pytest

import lbd_line_frames as F
import oracle_lib as O
from plp import plp
from test_gpu_line import compare_stages
from test_gpu_line_passes import run_batch

pytestmark = pytest.mark.gpu


def oracles(frames):
    return [O.LineOracle(f, stable_order=True) for f in frames]


def check_batch(frames, oras, names):
    """one batched call over `frames`, every frame stage by stage against its oracle"""
    import torch
    frames = np.stack(frames)
    assert len({f.tobytes() for f in frames}) == len(frames), "the frames of the batch must differ: a frame mix-up has to show"
    lt = plp.LineFeatureTracker()
    lt.set_seed_order(plp.SEED_ORDER_STABLE)
    cnt, kl, lbd, fn = run_batch(lt, torch.from_numpy(frames).to("cuda:0"))
    for f, (ora, name) in enumerate(zip(oras, names)):
        w = f"frame {f} ({name}): "
        assert cnt[f] == len(ora.keylsd), w + f"{cnt[f]} kept lines, oracle {len(ora.keylsd)}"
        compare_stages(lt, ora, frames[f].shape, kl[f, :cnt[f]], lbd[f, :cnt[f]], fn[f, :cnt[f]], frame=f, what=w, need_lines=len(ora.all_kl) > 0)


def test_directions_and_lengths():
    """eight directions x eight bar lengths, two key lines per frame: sample counts of every residue mod 8 and on both sides of 32, 64, 72, 128 and 136"""
    sweep = F.sweep_frames()
    assert len(sweep) <= 64
    oras = oracles([img for _, _, img in sweep])
    for (a, n, _), ora in zip(sweep, oras):
        assert len(ora.all_kl) == 2, f"{a} deg, bar of {n} px: {len(ora.all_kl)} key lines"
    counts = set(np.concatenate([o.all_kl["numOfPixels"] for o in oras]).tolist())
    assert {c % 8 for c in counts} == set(range(8)), sorted(counts)
    for lo, hi in ((22, 31), (57, 64), (65, 72), (121, 128), (129, 136)):
        assert any(lo <= c <= hi for c in counts), (lo, hi, sorted(counts))
    check_batch([img for _, _, img in sweep], oras, [f"{a} deg, bar of {n} px" for a, n, _ in sweep])


def test_bands_that_leave_the_image():
    """bars 6 px from each border and in two corners (clamped rows and columns), and a bar stepped pixel by pixel through the positions at which the band of
    one of its lines just fits / just leaves, at the top (rows) and at the right (columns): both loop bodies and the choice between them"""
    edge = F.edge_frames()
    oras = oracles([img for _, img in edge])
    h, w = F.SHAPE
    ext = [F.band_extent(o.all_kl) for o in oras]
    for (name, _), o in zip(edge, oras):
        assert len(o.all_kl) == 2, f"{name}: {len(o.all_kl)} key lines"
    assert oras[0].all_kl["numOfPixels"].tolist() == [149, 149] and sorted(oras[3].all_kl["numOfPixels"].tolist()) == [115, 119]
    y_min = np.concatenate([e[1] for e in ext]); x_max = np.concatenate([e[2] for e in ext])
    x_min = np.concatenate([e[0] for e in ext]); y_max = np.concatenate([e[3] for e in ext])
    assert y_min.min() < -20 and x_min.min() < -20 and y_max.max() > h + 19 and x_max.max() > w + 19, "a band far outside on every side"
    assert np.any((y_min > -1.5) & (y_min < -0.5)) and np.any((y_min > 0.5) & (y_min < 1.5)), ("a band one pixel outside / inside at the top", np.sort(y_min))
    assert np.any((x_max - (w - 1) > 0.5) & (x_max - (w - 1) < 1.5)) and np.any((w - 1 - x_max > 0.5) & (w - 1 - x_max < 1.5)), ("... at the right", np.sort(x_max))
    check_batch([img for _, img in edge], oras, [name for name, _ in edge])


def test_ragged_frames_in_one_batch():
    """B = 5: no line, two lines, and three frames of 24 or more lines of mixed lengths -- more than the eight waves a frame has"""
    frames = F.ragged_frames()
    oras = oracles(frames)
    n = [len(o.all_kl) for o in oras]
    assert n[0] == 0 and n[1] == 2 and min(n[2:]) >= 24, n
    for o in oras[2:]:
        assert o.all_kl["numOfPixels"].min() < 40 and o.all_kl["numOfPixels"].max() > 110, sorted(o.all_kl["numOfPixels"].tolist())
    check_batch(frames, oras, ["flat", "one bar", "twelve bars", "thirteen upright bars", "twelve bars at 7 deg"])


def test_odd_geometry():
    """171 x 221: the width is no multiple of 8 and the height no multiple of 4; bars at the right and bottom edges, whose clamped samples lie in the last,
    partial tiles of the Sobel plane"""
    odd = F.odd_frames()
    h, w = F.ODD_SHAPE
    assert w % 8 and h % 4
    oras = oracles([img for _, img in odd])
    ext = [F.band_extent(o.all_kl) for o in oras]
    assert ext[0][2].max() > w and ext[1][3].max() > h and ext[2][2].max() > w and ext[2][3].max() > h, "bands past the right and the bottom edge"
    assert len(oras[4].all_kl) >= 24
    check_batch([img for _, img in odd], oras, [name for name, _ in odd])


def test_the_single_frame_entry():
    """extract_LSD_LBD (one frame: sixteen workgroups of k_lbd) on one frame of each kind above"""
    frames = [("sweep, 45 deg", F.centred(45, 138)), ("edge, top", F.edge_frames()[0][1]), ("band edge", F.edge_frames()[9][1]), ("thirteen bars", F.ragged_frames()[3]),
              ("odd size, corner", F.odd_frames()[2][1]), ("odd size, twelve bars", F.odd_frames()[4][1]), ("flat", F.flat())]
    lt = plp.LineFeatureTracker()
    lt.set_seed_order(plp.SEED_ORDER_STABLE)
    for name, img in frames:
        ora = O.LineOracle(img, stable_order=True)
        kl, lbd, fn = lt.extract_LSD_LBD(img)
        compare_stages(lt, ora, img.shape, kl, lbd, fn, what=f"{name}: ", need_lines=name != "flat")
