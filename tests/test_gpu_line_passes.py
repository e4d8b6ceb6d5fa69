"""GPU parity of the line front end on the frame sizes its tile layouts make special (tests/line_pass_frames.py derives them: widths and heights around
the 128 x 32 blur tile, the 120 x 30 Sobel block, the inside-x and rows_inside switches, all four classes of w % 4 and h % 4 through k_blur_half and through
k_blur_plane<5> + k_resize_exact, and frames below the 48 rows / columns of blur_reflect101's single reflection down to 16 x 16).  Every stage is compared
with the oracle bit for bit (test_gpu_line.compare_stages: scaled plane, seed order, segments, KeyLine records, the full Sobel planes, LBD bits, kept lines
and line functions) and every failure names the shape, the setting and the stage.  tests/test_line_passes_cpu.py holds the oracle itself to a plain
restatement at the same sizes and checks that every image has key lines, so that no Sobel comparison is skipped."""
import numpy as np
import pytest

import line_pass_frames as F
import oracle_lib as O
from plp import plp
from test_gpu_line import compare_one, compare_stages

pytestmark = pytest.mark.gpu

ORDERS = ((plp.SEED_ORDER_LIBSTDCXX, False, "libstdc++ order"), (plp.SEED_ORDER_STABLE, True, "stable order"))


def sweep(shape, images, grow_waves):
    for name, img in images:
        assert img.shape == tuple(shape)
        for order, stable, oname in ORDERS:
            ora = O.LineOracle(img, stable_order=stable)
            for waves in grow_waves:
                compare_one(img, ora, waves, order, what=f"{shape[0]} x {shape[1]} {name}, {oname}, grow waves {waves}: ", need_lines=True)


def shape_id(s):
    return f"{s[0]}x{s[1]}"


@pytest.mark.parametrize("shape", F.width_shapes(), ids=shape_id)
def test_widths_around_the_tile_edges(shape):
    """the front passes do not depend on the grower (one setting); k_lsd_gradient writes another g2 plane under the exact seed order (both orders)"""
    sweep(shape, F.images(shape), (0,))


@pytest.mark.parametrize("shape", F.height_shapes(), ids=shape_id)
def test_heights_around_the_tile_edges(shape):
    sweep(shape, F.images(shape), (0,))


@pytest.mark.parametrize("shape", F.TINY, ids=shape_id)
def test_tiny_frames(shape):
    """the loop of blur_reflect101, k_lsd_order with one to a few 64-pixel groups, the exact seed sort on a handful of entries, both growers on a handful of groups"""
    sweep(shape, F.images(shape), (0, 1))


def test_one_context_walks_through_sizes():
    """build() resets the batch capacity, the fused / fallback switch, the row divisor and the resize tables when the size changes: one context, sizes
    that flip each of them, in both seed orders; the first and the last frame are the same and must give the same result"""
    walk = F.WALK
    imgs = {s: F.canvas(s) for s in walk}
    lt = plp.LineFeatureTracker()
    for order, stable, oname in ORDERS:
        lt.set_seed_order(order)
        oras = {s: O.LineOracle(imgs[s], stable_order=stable) for s in imgs}
        results = []
        for i, s in enumerate(walk):
            kl, lbd, fn = lt.extract_LSD_LBD(imgs[s])
            compare_stages(lt, oras[s], s, kl, lbd, fn, what=f"step {i} of the walk, {s[0]} x {s[1]}, {oname}: ", need_lines=True)
            results.append((kl, lbd, fn))
        for a, b in zip(results[0], results[-1]):
            assert np.array_equal(a, b), f"{oname}: the same frame at both ends of the walk"


def run_batch(lt, d, cap=512):
    import torch
    B, dev = d.shape[0], d.device
    d_kl = torch.zeros((B, cap, 68), dtype=torch.uint8, device=dev)
    d_lbd = torch.zeros((B, cap, 32), dtype=torch.uint8, device=dev)
    d_fn = torch.zeros((B, cap, 3), dtype=torch.float64, device=dev)
    d_cnt = torch.zeros(B, dtype=torch.int32, device=dev)
    lt.extract_batch(d, d_kl, d_lbd, d_fn, d_cnt)
    torch.cuda.synchronize()
    lt.last_batch_status()
    return d_cnt.cpu().numpy(), d_kl.cpu().numpy().view(plp.KL_DTYPE).reshape(B, cap), d_lbd.cpu().numpy(), d_fn.cpu().numpy()


def compare_batch(lt, frames, out, what):
    cnt, kl, lbd, fn = out
    assert len({f.tobytes() for f in frames}) == len(frames), "the frames of the batch must differ: a frame mix-up has to show"
    for f in range(len(frames)):
        ora = O.LineOracle(frames[f])      # (a new context's seed order is the oracle's default: libstdc++)
        w = f"{what}, frame {f}: "
        assert cnt[f] == len(ora.keylsd), w + f"{cnt[f]} kept lines, oracle {len(ora.keylsd)}"
        compare_stages(lt, ora, frames[f].shape, kl[f, :cnt[f]], lbd[f, :cnt[f]], fn[f, :cnt[f]], frame=f, what=w, need_lines=True)


@pytest.mark.parametrize("shape, B", F.BATCHES, ids=lambda v: shape_id(v) if isinstance(v, tuple) else f"B{v}")
def test_batches_stage_by_stage_in_every_frame(shape, B):
    import torch
    frames = F.batch_frames(shape, B)
    lt = plp.LineFeatureTracker()
    out = run_batch(lt, torch.from_numpy(frames).to("cuda:0"))
    compare_batch(lt, frames, out, f"batch of {B} frames {shape[0]} x {shape[1]}")


def test_batch_of_unaligned_frames_goes_through_the_aligned_copy():
    """a view with an odd base address and a row step that is no multiple of 4: run() copies every frame to an aligned plane first"""
    import torch
    (H, W), B = F.UNALIGNED_BATCH
    frames = F.batch_frames((H, W), B)
    dev = torch.device("cuda:0")
    big = torch.zeros((B, H, W + 5), dtype=torch.uint8, device=dev)
    big[:, :, 1:W + 1] = torch.from_numpy(frames).to(dev)
    d = big[:, :, 1:W + 1]                                       # base address odd, row step 249
    assert d.data_ptr() % 4 != 0 and d.stride(1) % 4 != 0
    lt = plp.LineFeatureTracker()
    compare_batch(lt, frames, run_batch(lt, d), f"batch of {B} unaligned frames {H} x {W}")


@pytest.mark.parametrize("i", range(len(F.BORDER_SHAPES)), ids=[shape_id(s) for s in F.BORDER_SHAPES])
def test_lines_hugging_the_image_border(i):
    """bars along all four borders: the 63-row LBD band of their lines leaves the image on one side (rows and columns clamped in k_lbd)"""
    shape, img = F.BORDER_SHAPES[i], F.border_frames()[i]
    for order, stable, oname in ORDERS:
        ora = O.LineOracle(img, stable_order=stable)
        hug = F.border_hugging(ora.keylsd, shape)
        assert len(hug) >= 4, f"{len(hug)} kept lines within 3 px of a border"
        for waves in (0, 1, 3):
            compare_one(img, ora, waves, order, what=f"{shape[0]} x {shape[1]} edges, {oname}, grow waves {waves}: ", need_lines=True)
