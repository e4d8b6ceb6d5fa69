"""GPU parity of the ORB stencil passes on the geometries their strip layouts make special: k_blur7 blurs strips of 248 columns x 64 rows, one per wave,
with lanes 0 / 63 as side halo and the image border reflected in registers.  Every pyramid level, the FAST candidates, the quadtree selection and the complete
blurred level are compared with the oracle bit for bit (test_gpu_orb.compare_full), and so are key points and descriptors."""
import numpy as np
import pytest
from PIL import Image

import oracle_lib as O
from plp import plp, synth
from test_gpu_orb import compare_full

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("w", [45, 46, 47, 61, 247, 248, 249, 251, 252, 253, 255, 256, 257, 496, 499, 500, 503, 504, 505, 506, 507, 744, 745])
def test_one_level_widths_around_the_strip_edges(w):
    """one level: widths below one strip, at and around the strip width and the test that picks a strip's border path (x0 + 256 > w), not a multiple of 4"""
    h = max(45, w // 8) + w % 37   # (the quadtree takes at most 32 initial nodes: w / h <= 32 inside the border)
    compare_full(synth.canvas(300 + w, h, w), 500, num_levels=1)


@pytest.mark.parametrize("h", [45, 46, 63, 64, 65, 66, 71, 127, 128, 129, 130, 135])
def test_one_level_heights_around_the_row_blocks(h):
    """one level: heights around the 64-row blocks and the 8-row trips of a strip, even and odd"""
    w = 201 if h < 63 else 333     # (the quadtree takes at most 32 initial nodes)
    compare_full(synth.canvas(900 + h, h, w), 500, num_levels=1)


@pytest.mark.parametrize("shape, levels", [((480, 641), 8), ((481, 643), 8), ((250, 250), 4), ((300, 497), 5), ((333, 517), 8), ((200, 1001), 6)])
def test_pyramids_with_narrow_and_odd_levels(shape, levels):
    """whole pyramids whose levels are narrower than a strip or not a multiple of 4 wide"""
    h, w = shape
    compare_full(synth.canvas(11 * h + w, h, w), 1000, num_levels=levels)


def test_masks_on_an_odd_width(golden_dir):
    img = np.ascontiguousarray(np.asarray(Image.open(golden_dir / "equirect1_640x480.png"))[:, :637])
    rows, cols = img.shape
    m = np.ones_like(img); m[:, 0:cols // 3] = 0
    compare_full(img, 2000, mask=m)
    compare_full(img, 2000, mask_rects=[[0.0, 0.3, 0.0, 1.0], [0.0, 1.0, 0.9, 1.0]])


def test_one_level_k2000():
    rng = np.random.default_rng(5)
    compare_full(rng.integers(0, 256, (480, 642), dtype=np.uint8), 2000, num_levels=1)


@pytest.mark.parametrize("h, w, K", [(2160, 3840, 5000), (480, 4000, 2000)])
def test_large_frames_stage_by_stage(h, w, K):
    compare_full(synth.canvas(17 + h, h, w), K)


def test_batched_unaligned_frames_go_through_the_level0_copy():
    """frames whose rows are not 4-byte aligned are copied to the aligned level-0 plane first (l0copy); every frame's blurred levels equal the oracle's"""
    import torch
    frames = synth.replay(23, 5)
    B, H, W = frames.shape
    W = W - 3                                                    # 637 columns: a width that is not a multiple of 4
    dev = torch.device("cuda:0")
    big = torch.zeros((B, H, W + 5), dtype=torch.uint8, device=dev)
    big[:, :, 1:W + 1] = torch.from_numpy(np.ascontiguousarray(frames[:, :, :W])).to(dev)
    d = big[:, :, 1:W + 1]                                       # base address odd, row step 642
    assert d.data_ptr() % 4 != 0
    K, cap = 1000, 2100
    ex = plp.orb_extractor(K)
    d_kps = torch.zeros((B, cap, 28), dtype=torch.uint8, device=dev)
    d_desc = torch.zeros((B, cap, 32), dtype=torch.uint8, device=dev)
    d_cnt = torch.zeros(B, dtype=torch.int32, device=dev)
    ex.extract_batch(d, d_kps, d_desc, d_cnt)
    torch.cuda.synchronize()
    ex.last_batch_status()
    cnt = d_cnt.cpu().numpy()
    kps = d_kps.cpu().numpy().view(plp.KP_DTYPE).reshape(B, cap)
    desc = d_desc.cpu().numpy()
    for f in range(B):
        img = np.ascontiguousarray(frames[f, :, :W])
        ora = O.OrbOracle(K)
        ok, od = ora.extract(img)
        for l in range(ex.get_num_scale_levels()):
            assert np.array_equal(ex.image_pyramid(l, frame=f), ora.level_image(l)), (f, l)
            assert np.array_equal(ex.debug_read(ex.DBG_BLURRED, l, frame=f), ora.level_blurred(l)), (f, l)
        assert cnt[f] == len(ok)
        assert np.array_equal(kps[f, :cnt[f]], ok)
        assert np.array_equal(desc[f, :cnt[f]], od)
