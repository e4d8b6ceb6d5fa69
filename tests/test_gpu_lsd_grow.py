"""LSD region growing on the device (k_lsd_grow: one wave per frame; k_lsd_grow_mw: one main wave + speculating helpers) against the oracle, on the frames
of tests/lsd_grow_frames.py.  tests/test_lsd_grow_cpu.py asserts on the oracle's census which branches of the growers, the rectangle fits and the
refinement those frames reach; here every stage of every frame is compared bit for bit (test_gpu_line.compare_stages) and the growers' own counters
(PLP_LINE_DBG_GROW_STATS) are checked against the census after every call:
  one wave per frame:  [0] regions grown == census.regions_grown, [1] pixels accepted == census.pixels_first, [3] == 0;
  several waves:       [0] grown by main + [1] results taken from helpers == census.regions_grown (a seed still open at the main wave's turn is either
                       taken from a helper or grown by main), [3] == the waves the launch admitted.
[1] and [2] of the several-waves kernel (taken, rejected) depend on timing and the one-wave [2] (exact decisions inside the guard band) on the kernel's
own ordering: they are summed into the messages and printed, not asserted (one run: profiles/r25_lsd_grow_paths.md).
The frame with more than 2048 segments is run by the overflow test alone: every call on it raises."""
import numpy as np
import pytest

import lsd_grow_frames as F
import oracle_lib as O
from plp import plp
from test_gpu_line import compare_stages

pytestmark = pytest.mark.gpu

WAVES = (1, 0, 2, 3, 5, 8)
TOTALS = {"taken": 0, "rejected": 0, "exact": 0, "calls": 0}


def totals():
    return f" [so far in this module: {TOTALS['calls']} calls, {TOTALS['taken']} helper results taken, {TOTALS['rejected']} rejected, {TOTALS['exact']} exact decisions]"


def admitted_waves(shape, want):
    """the waves per frame launch_line_front() admits for a frame of `shape` (csrc/line_kernels.hip): the largest w <= want whose layout fits 160 KB of LDS"""
    sh, sw = F.half_size(shape)
    n = sw * sh
    nw_al = ((n + 31) // 32 + 1) & ~1
    groups_cap = ((sw - 1) * (sh - 1) + 63) // 64 + 1
    for w in range(min(want, 8) if want > 0 else 8, 1, -1):
        if 5 * nw_al * 4 + w * (nw_al + 256 + 192 + 2) * 4 + (8 + 8 * 8) * 4 + ((groups_cap + 15) & ~15) + 16 + (w - 1) * 2 * 16 * 80 <= 160 * 1024:
            return w
    return 1


def waves_per_workgroup(shape):
    """wpb of k_lsd_grow as launch_line_front() derives it: the waves whose USED bitmap + 256-word ring fit 64 KB together, at most 4"""
    sh, sw = F.half_size(shape)
    per_wave = ((((sw * sh + 31) // 32 + 1) & ~1) + 256) * 4
    return max(1, min(4, 65536 // per_wave))


def check_stats(lt, ora, frame, waves, shape, what):
    gs = lt.debug_read(lt.DBG_GROW_STATS, frame)
    c = ora.census
    TOTALS["calls"] += 1
    if waves == 1:
        TOTALS["exact"] += int(gs[2])
        assert gs[0] == c.regions_grown and gs[1] == c.pixels_first and gs[3] == 0, \
            what + f"one wave per frame grew {gs[0]} regions of {gs[1]} points, the oracle {c.regions_grown} of {c.pixels_first} (stats {gs.tolist()})" + totals()
    else:
        TOTALS["taken"] += int(gs[1]); TOTALS["rejected"] += int(gs[2])
        assert gs[3] == admitted_waves(shape, waves), what + f"ran with {gs[3]} waves, the layout admits {admitted_waves(shape, waves)}" + totals()
        assert gs[0] + gs[1] == c.regions_grown, \
            what + f"main grew {gs[0]} regions and took {gs[1]} from helpers ({gs[2]} rejected), the oracle grew {c.regions_grown}" + totals()
    return gs


def run_one(lt, img, ora, waves, order=plp.SEED_ORDER_STABLE, what=""):
    lt.set_grow_waves(waves)
    lt.set_seed_order(order)
    kl, lbd, fn = lt.extract_LSD_LBD(img)
    what = f"{what}, grow waves {waves}, seed order {'stable' if order == plp.SEED_ORDER_STABLE else 'libstdc++'}: "
    compare_stages(lt, ora, img.shape, kl, lbd, fn, what=what)
    check_stats(lt, ora, 0, waves, img.shape, what)
    return kl, lbd, fn


def frames_of(family):
    return [(i, name, img) for i, (fam, name, img) in enumerate(F.all_frames()) if fam == family]


def run_batch(lt, frames, oracles, what):
    """one extract_batch of equal-sized frames with the context's settings; returns per frame (kl, lbd, fn); the caller checks last_batch_status()"""
    import torch
    dev = torch.device("cuda:0")
    d = torch.from_numpy(np.stack(frames)).to(dev)
    B, cap = len(frames), max(len(o.keylsd) for o in oracles) + 8
    d_kl = torch.zeros((B, cap, 68), dtype=torch.uint8, device=dev)
    d_lbd = torch.zeros((B, cap, 32), dtype=torch.uint8, device=dev)
    d_fn = torch.zeros((B, cap, 3), dtype=torch.float64, device=dev)
    d_cnt = torch.zeros(B, dtype=torch.int32, device=dev)
    lt.extract_batch(d, d_kl, d_lbd, d_fn, d_cnt)
    torch.cuda.synchronize()
    cnt = d_cnt.cpu().numpy()
    kl = d_kl.cpu().numpy().view(plp.KL_DTYPE).reshape(B, cap)
    lbd, fn = d_lbd.cpu().numpy(), d_fn.cpu().numpy()
    assert np.all(cnt <= cap), what + f"counts {cnt.tolist()} above the capacity {cap}"
    return [(kl[f, :cnt[f]], lbd[f, :cnt[f]], fn[f, :cnt[f]]) for f in range(B)]


FAMILIES = [f for f in F.FAMILY_NAMES if f != "square grid"]


@pytest.mark.parametrize("waves", WAVES)
@pytest.mark.parametrize("family", FAMILIES)
def test_every_family_under_every_waves_setting(family, waves):
    lt = plp.LineFeatureTracker()
    frames = frames_of(family)
    assert frames
    for i, name, img in frames:
        run_one(lt, img, F.oracle(i, True), waves, what=f"{family}: {name}")
    print(f"{family}, grow waves {waves}" + totals())


@pytest.mark.parametrize("family", FAMILIES)
def test_a_frame_of_every_family_in_the_libstdcxx_seed_order(family):
    """the seed order of a reference built with libstdc++ (the oracle calls std::sort, the library replays its introsort on the device)"""
    lt = plp.LineFeatureTracker()
    frames = frames_of(family)
    i, name, img = frames[len(frames) // 2]
    for w in (1, 0, 3):
        run_one(lt, img, F.oracle(i, False), w, plp.SEED_ORDER_LIBSTDCXX, what=f"{family}: {name}")
    print(f"{family}, libstdc++ order" + totals())


def test_all_base_size_frames_in_one_batch():
    """101 different frames, one wave each, four waves to a workgroup: the last workgroup holds one frame (the b >= B return of the other three waves)"""
    sel = [(i, f"{fam}: {name}", img) for i, (fam, name, img) in enumerate(F.all_frames()) if img.shape == F.SHAPE]
    assert len(sel) > 90 and len(sel) % 4 != 0 and waves_per_workgroup(F.SHAPE) == 4
    lt = plp.LineFeatureTracker()
    lt.set_grow_waves(1)
    lt.set_seed_order(plp.SEED_ORDER_STABLE)
    oracles = [F.oracle(i, True) for i, _, _ in sel]
    out = run_batch(lt, [img for _, _, img in sel], oracles, "base-size batch: ")
    lt.last_batch_status()
    for f, (i, name, img) in enumerate(sel):
        what = f"frame {f} of the base-size batch ({name}), one wave per frame: "
        compare_stages(lt, oracles[f], img.shape, *out[f], frame=f, what=what)
        check_stats(lt, oracles[f], f, 1, img.shape, what)
    print("batch" + totals())


@pytest.mark.parametrize("shape,wpb", [((724, 728), 3), ((720, 1280), 2)])
def test_waves_per_workgroup(shape, wpb):
    """k_lsd_grow with 3 and 2 waves per workgroup (4: the base-size batch; 1: test_gpu_line.test_full_hd_frame): batches of wpb + 1 and of wpb frames"""
    assert waves_per_workgroup(shape) == wpb
    frames = F.wpb_frames(shape, wpb + 1)
    oracles = [O.LineOracle(img, stable_order=True, census=True) for _, img in frames]
    assert max(o.census.n_first.max() for o in oracles) > 4096 and sum(int(o.census.refined.sum()) for o in oracles) > 20
    lt = plp.LineFeatureTracker()
    lt.set_grow_waves(1)
    lt.set_seed_order(plp.SEED_ORDER_STABLE)
    for B in (wpb + 1, wpb):
        out = run_batch(lt, [img for _, img in frames[:B]], oracles[:B], f"{shape}, batch of {B}: ")
        lt.last_batch_status()
        for f in range(B):
            what = f"{frames[f][0]}, frame {f} of a batch of {B}, {wpb} waves per workgroup: "
            compare_stages(lt, oracles[f], shape, *out[f], frame=f, what=what)
            check_stats(lt, oracles[f], f, 1, shape, what)


def test_region_above_the_helpers_list():
    """a region of more than 16 384 points: a helper that meets it runs out of list (kMwHeap) and gives up, the main wave's list holds 2 n points"""
    (i, name, img), = frames_of("big ramp")
    ora = F.oracle(i, True)
    assert ora.census.n_first.max() > 16384 and admitted_waves(F.SHAPE, 0) == 8 and 2 <= admitted_waves(img.shape, 0) <= 5
    lt = plp.LineFeatureTracker()
    for w in (0, 2, 5, 1):
        run_one(lt, img, ora, w, what=name)
    print("big ramp" + totals())


def test_overflow_is_reported_and_the_context_keeps_working():
    """more than kLineCap = 2048 segments: PLP_ERR_OVERFLOW, the first 2048 segments in place, nothing else disturbed"""
    (i, name, img), = frames_of("square grid")
    for order, stable in ((plp.SEED_ORDER_STABLE, True), (plp.SEED_ORDER_LIBSTDCXX, False)):
        assert len(F.oracle(i, stable).raw) > plp.LINE_CAP
    lt = plp.LineFeatureTracker()
    lt.set_seed_order(plp.SEED_ORDER_STABLE)
    ora = F.oracle(i, True)
    for w in (1, 0):
        lt.set_grow_waves(w)
        with pytest.raises(plp.PlpError) as e:
            lt.extract_LSD_LBD(img)
        assert e.value.status == plp.PLP_ERR_OVERFLOW, f"{name}, grow waves {w}: status {e.value.status}"
        raw = lt.debug_read(lt.DBG_RAW)
        assert raw.shape == (plp.LINE_CAP, 4) and np.array_equal(raw, ora.raw[:plp.LINE_CAP]), f"{name}, grow waves {w}: the first 2048 segments differ from the oracle's"
        check_stats(lt, ora, 0, w, img.shape, f"{name}, grow waves {w}: ")
    # a batch in which only frame 1 of 3 overflows
    frames = F.grid_batch_frames()
    oracles = [O.LineOracle(im, stable_order=True, census=True) for _, im in frames]
    assert [len(o.raw) > plp.LINE_CAP for o in oracles] == [False, True, False]
    lt.set_grow_waves(1)
    out = run_batch(lt, [im for _, im in frames], oracles, "overflow batch: ")
    with pytest.raises(plp.PlpError) as e:
        lt.last_batch_status()
    assert e.value.status == plp.PLP_ERR_OVERFLOW
    raw = lt.debug_read(lt.DBG_RAW, 1)
    assert raw.shape == (plp.LINE_CAP, 4) and np.array_equal(raw, oracles[1].raw[:plp.LINE_CAP]), "overflow batch, frame 1: the first 2048 segments differ from the oracle's"
    for f in (0, 2):
        what = f"overflow batch, frame {f} ({frames[f][0]}): "
        compare_stages(lt, oracles[f], frames[f][1].shape, *out[f], frame=f, what=what)
    for f in range(3):
        check_stats(lt, oracles[f], f, 1, frames[f][1].shape, f"overflow batch, frame {f}: ")
    # the next ordinary calls on the same context
    j, name2, img2 = frames_of("curves")[-1]
    for w in (0, 1):
        run_one(lt, img2, F.oracle(j, True), w, what=f"after the overflow, {name2}")


def test_one_context_through_the_families():
    """the helpers' lists and the claim maps of one context reused across frames, sizes and both growers; the first frame again at the end"""
    lt = plp.LineFeatureTracker()
    seq = [frames_of(fam)[-1] for fam in F.FAMILY_NAMES if fam != "square grid"]
    seq += [frames_of(fam)[0] for fam in ("gratings", "curves", "noise")] + [seq[0]]
    first = None
    for k, (i, name, img) in enumerate(seq):
        res = run_one(lt, img, F.oracle(i, True), 0 if k % 2 == 0 else 1, what=f"step {k} of one context, {name}")
        if k == 0:
            first = res
    assert all(np.array_equal(a, b) for a, b in zip(first, res)), "the first frame gives another result at the end"
    print("one context" + totals())
