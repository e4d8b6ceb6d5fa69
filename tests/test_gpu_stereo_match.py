"""k_stereo_match / k_stereo_median against the oracle on BUILT key points (tests/stereo_match_scene.py; tests/test_stereo_match_cpu.py holds the
scenes to taking every reachable decision of stereo.cc:45-301 and pins them to the reference's own stereo.cc): the host entry on every scene, the
batched entry on five different frame pairs with ragged counts, NULL counts, two streams and a 4-byte-unaligned strided view, hand-set medians,
and the refusals.

Exactness is derived, not measured: the SAD is integer, every float step of the kernel is one correctly rounded f32 operation in the reference's
order, the parabola quotient is f64 and narrowed once.  So x_right and depth are compared with array_equal."""
import ctypes as C
import functools

import numpy as np
import pytest

import oracle_lib as O
import stereo_match_ref as R
import stereo_match_scene as S
from plp import plp

pytestmark = pytest.mark.gpu


def oracle(sc):
    return O.stereo_compute(sc.ol, sc.orr, sc.kl, sc.kr, sc.dl, sc.dr, sc.fxb, sc.tb)


def extractors(sc):
    """the two extractors after extract() of the scene's eyes: their pyramids are what stereo reads"""
    el, er = plp.orb_extractor(sc.K, sc.scale, sc.levels), plp.orb_extractor(sc.K, sc.scale, sc.levels)
    (gkl, gdl), (gkr, gdr) = el.extract(sc.left), er.extract(sc.right)
    (okl, odl), (okr, odr) = sc.extracted
    assert np.array_equal(gkl, okl) and np.array_equal(gkr, okr) and np.array_equal(gdl, odl) and np.array_equal(gdr, odr)
    return el, er


def check_host(el, er, sc, tag):
    want_x, want_d = oracle(sc)
    got_x, got_d = el.stereo_compute(er, sc.kl, sc.kr, sc.dl, sc.dr, sc.fxb, sc.tb)
    assert np.array_equal(got_x >= 0, want_x >= 0) and np.array_equal(got_d >= 0, want_d >= 0), tag
    bad = np.nonzero((got_x != want_x) | (got_d != want_d))[0]
    assert len(bad) == 0, (tag, bad[:5], got_x[bad[:5]], want_x[bad[:5]], got_d[bad[:5]], want_d[bad[:5]])
    return want_x


@pytest.mark.parametrize("name", S.GPU_NAMES)
def test_host_entry_equals_the_oracle_on_built_key_points(name):
    sc = S.scene(name)
    el, er = extractors(sc)
    want_x = check_host(el, er, sc, name)
    assert (want_x >= 0).sum() >= 20, "vacuous"
    # the same frames under another disparity range: max_disp <= disp and the x gate move
    other = sc.with_lists(sc.kl, sc.kr, sc.dl, sc.dr, built=False)
    other.fxb, other.tb = 7.25, 1.0
    check_host(el, er, other, name + " fxb/tb 7.25")


def test_host_entry_single_row_of_65_right_key_points():
    """regression by name for the 64-lane pass over the right list: index 64 wins alone, index 0 wins its tie with index 64"""
    base = S.scene("160x208")
    lists, want = S.single_row_lists(base)
    sc = base.with_lists(*lists)
    r = R.compute(sc.levels_l, sc.levels_r, sc.kl, sc.kr, sc.dl, sc.dr, sc.sf, sc.isf, sc.fxb, sc.tb)
    assert r["best_right"].tolist() == [want["A"], want["B"], want["C"]]
    el, er = extractors(base)
    check_host(el, er, sc, "single row")
    assert r["x_right"][0] != r["x_right"][1]                              # A and B share a position: only the winner tells them apart


def test_the_extractor_refuses_the_38_row_top_level():
    """240x400 under three levels of 2.5: held against the oracle and the reference on the CPU; the device extractor refuses a level of 44 px or less"""
    for name in S.GPU_REFUSED:
        sc = S.scene(name)
        with pytest.raises(plp.PlpError) as e:
            plp.orb_extractor(sc.K, sc.scale, sc.levels).extract(sc.left)
        assert e.value.status == plp.PLP_ERR_INVALID_ARG


def test_median_of_hand_set_subsets():
    """1, 2, 33, 34 and 16 key points reach the median step; for 33 / 34 the median is one of three equal correlations, the correlations span more than
    8 high bytes and some exceed twice the median; the 16 are distinct, with four between twice sorted[7] and twice sorted[8] (asserted on the
    restatement in tests/test_stereo_match_cpu.py::test_census_median_subsets)"""
    sc = S.noise_with_forced_pairs()
    full = R.compute(sc.levels_l, sc.levels_r, sc.kl, sc.kr, sc.dl, sc.dr, sc.sf, sc.isf, sc.fxb, sc.tb)
    el, er = extractors(sc)
    check_host(el, er, sc, "noise + forced pairs")
    for n, sub in S.median_subsets(sc, full["corr"]):
        r = R.compute(sub.levels_l, sub.levels_r, sub.kl, sub.kr, sub.dl, sub.dr, sub.sf, sub.isf, sub.fxb, sub.tb)
        reached = r["corr"][r["corr"] >= 0]
        assert len(reached) == n
        if n > 16:
            assert len(set((reached >> 8).tolist())) >= 8 and (reached == r["median"]).sum() == 3 and (r["reason"] == R.MEDIAN_REJECTED).sum() >= 3
        want_x = check_host(el, er, sub, f"median subset {n}")
        assert np.array_equal(want_x, r["x_right"])


def test_host_entry_takes_65535_right_key_points_and_refuses_65536():
    sc = S.scene("120x160")
    el, er = extractors(sc)
    # 65535: the real right key points at the END of the list, behind copies of one that matches nobody: every winner has an index above 64000
    filler_k, filler_d = S.keypoint(80.0, 60.0, 0, sc.sf), np.random.default_rng(5).integers(0, 256, 32, dtype=np.uint8)
    n_fill = 65535 - len(sc.kr)
    big = sc.with_lists(sc.kl, np.concatenate([np.repeat(np.array([filler_k], O.KP_DTYPE), n_fill), sc.kr]), sc.dl,
                        np.concatenate([np.repeat(filler_d[None], n_fill, 0), sc.dr]))
    want_x = check_host(el, er, big, "65535 right key points")
    assert np.array_equal(want_x, oracle(sc)[0]) and (want_x >= 0).sum() >= 20
    # 65536: refused before any launch (the arrays only need the length)
    kr, dr = np.zeros(65536, O.KP_DTYPE), np.zeros((65536, 32), np.uint8)
    with pytest.raises(plp.PlpError) as e:
        el.stereo_compute(er, sc.kl, kr, sc.dl, dr, sc.fxb, sc.tb)
    assert e.value.status == plp.PLP_ERR_INVALID_ARG
    with pytest.raises(plp.PlpError) as e:
        el.stereo_compute(er, kr, sc.kr, dr, sc.dr, sc.fxb, sc.tb)
    assert e.value.status == plp.PLP_ERR_INVALID_ARG
    check_host(el, er, sc, "after the refusal")


# ------------------------------------------------------------------------------------------------ batched entry
B = 5
GARBAGE = 7.0


@functools.lru_cache(maxsize=None)
def ragged_frames(name):
    """five different frame pairs of one geometry, each with its own built lists: 0 left key points, 0 right key points, the full lists, 1 left key
    point, and 65 right key points in a single row"""
    scs = [S.scene(name, seed=f) for f in range(B)]
    out = []
    for f, sc in enumerate(scs):
        kl, kr, dl, dr = sc.kl, sc.kr, sc.dl, sc.dr
        if f == 0:
            kl, dl = kl[:0], dl[:0]
        elif f == 1:
            kr, dr = kr[:0], dr[:0]
        elif f == 3:
            j = int(np.nonzero(oracle(sc)[0] >= 0)[0][3])
            kl, dl = kl[j:j + 1], dl[j:j + 1]
        elif f == 4:
            kl, kr, dl, dr = S.single_row_lists(sc, seed=f)[0]
        out.append(sc.with_lists(kl, kr, dl, dr))
    return scs, out


def padded(full, sc, cap):
    """NULL counts: every frame holds exactly cap legal key points on both sides (its own lists repeated; an empty list takes the scene's)"""
    pick = lambda a, b: np.resize(a if len(a) else b, (cap,) + a.shape[1:])
    return sc.with_lists(pick(sc.kl, full.kl), pick(sc.kr, full.kr), pick(sc.dl, full.dl), pick(sc.dr, full.dr))


def run_batch(name, counts, stream, cap_slack, unaligned=False):
    import torch
    dev = torch.device("cuda:0")
    fulls, frames = ragged_frames(name)
    largest = max(max(len(sc.kl), len(sc.kr)) for sc in frames)
    cap = largest + cap_slack
    if not counts:
        frames = [padded(full, sc, cap) for full, sc in zip(fulls, frames)]
    sc0 = frames[0]
    H, W = sc0.rows, sc0.cols

    def upload(imgs):
        a = np.stack(imgs)
        if not unaligned:
            return torch.from_numpy(a).to(dev)
        big = torch.zeros((B, H, W + 5), dtype=torch.uint8, device=dev)          # base address odd, row step W + 5
        big[:, :, 1:W + 1] = torch.from_numpy(a).to(dev)
        d = big[:, :, 1:W + 1]
        assert d.data_ptr() % 4 != 0 and W % 4 != 0
        return d

    d_left, d_right = upload([sc.left for sc in frames]), upload([sc.right for sc in frames])

    def stage(lists, width):
        a = np.full((B, cap, width), 0xFF, np.uint8)                             # rows past a count: NaN coordinates, octave -1; never read
        for f, v in enumerate(lists):
            a[f, :len(v)] = np.ascontiguousarray(v).view(np.uint8).reshape(len(v), width)
        return torch.from_numpy(a).to(dev)

    t_kl, t_kr = stage([sc.kl for sc in frames], 28), stage([sc.kr for sc in frames], 28)
    t_dl, t_dr = stage([sc.dl for sc in frames], 32), stage([sc.dr for sc in frames], 32)
    t_cl = torch.tensor([len(sc.kl) for sc in frames], dtype=torch.int32, device=dev)
    t_cr = torch.tensor([len(sc.kr) for sc in frames], dtype=torch.int32, device=dev)
    xr = torch.full((B, cap), GARBAGE, dtype=torch.float32, device=dev); dep = torch.full((B, cap), GARBAGE, dtype=torch.float32, device=dev)
    el, er = plp.orb_extractor(sc0.K, sc0.scale, sc0.levels), plp.orb_extractor(sc0.K, sc0.scale, sc0.levels)
    ecap = 2 * sc0.K + 64
    e_k = [torch.zeros((B, ecap, 28), dtype=torch.uint8, device=dev) for _ in range(2)]
    e_d = [torch.zeros((B, ecap, 32), dtype=torch.uint8, device=dev) for _ in range(2)]
    e_c = [torch.zeros(B, dtype=torch.int32, device=dev) for _ in range(2)]
    cur = torch.cuda.current_stream(dev)
    st = cur if stream == "current" else torch.cuda.Stream(dev)
    st.wait_stream(cur)
    el.extract_batch(d_left, e_k[0], e_d[0], e_c[0], stream=st)
    er.extract_batch(d_right, e_k[1], e_d[1], e_c[1], stream=st)

    def call(cap=cap, nb=B, left=el, right=er):
        plp._check(plp.lib().plp_stereo_compute_batch_device(left._h, right._h, t_kl.data_ptr(), t_cl.data_ptr() if counts else None, t_kr.data_ptr(),
                                                             t_cr.data_ptr() if counts else None, t_dl.data_ptr(), t_dr.data_ptr(), cap, nb,
                                                             C.c_float(sc0.fxb), C.c_float(sc0.tb), xr.data_ptr(), dep.data_ptr(), C.c_void_p(st.cuda_stream)))

    return dict(frames=frames, cap=cap, call=call, st=st, xr=xr, dep=dep, el=el, er=er, keep=(d_left, d_right, e_k, e_d, e_c), torch=torch)


def check_batch(run):
    run["call"]()
    run["st"].synchronize()
    run["el"].last_batch_status(); run["er"].last_batch_status()
    xr, dep = run["xr"].cpu().numpy(), run["dep"].cpu().numpy()
    for f, sc in enumerate(run["frames"]):
        want_x, want_d = oracle(sc)                                             # each frame = the oracle on that frame alone
        n = len(sc.kl)
        assert np.array_equal(xr[f, :n], want_x) and np.array_equal(dep[f, :n], want_d), f
        assert (xr[f, n:] == -1).all() and (dep[f, n:] == -1).all(), f          # rows past the left count
    return xr


BATCH_CASES = [("160x208", True, "current", 0), ("160x208", True, "side", 37), ("160x208", False, "current", 37), ("160x208", False, "side", 0)]


@pytest.mark.parametrize("name,counts,stream,cap_slack", BATCH_CASES)
def test_batched_entry_ragged_frames_each_equal_the_oracle(name, counts, stream, cap_slack):
    run = run_batch(name, counts, stream, cap_slack)
    n_l, n_r = [len(sc.kl) for sc in run["frames"]], [len(sc.kr) for sc in run["frames"]]
    if counts:
        assert n_l[0] == 0 and n_r[1] == 0 and n_l[3] == 1 and n_r[4] == 65 and (max(n_l + n_r) == run["cap"]) == (cap_slack == 0)
    else:
        assert set(n_l + n_r) == {run["cap"]}
    xr = check_batch(run)
    assert sum(int((xr[f, :n_l[f]] >= 0).sum()) for f in range(B)) >= 60, "vacuous"
    assert len({sc.left.tobytes() for sc in run["frames"]}) == B                  # five different frames


def test_batched_entry_reads_the_level0_copy_of_unaligned_frames():
    """frames whose rows are not 4-byte aligned go through the extractor's aligned level-0 copy (tests/test_gpu_orb_passes.py); stereo must read the
    level 0 the extractor did, not the caller's view"""
    run = run_batch("161x211", True, "current", 37, unaligned=True)
    check_batch(run)
    for f, sc in enumerate(run["frames"]):
        assert np.array_equal(run["el"].image_pyramid(0, frame=f), sc.left) and np.array_equal(run["er"].image_pyramid(0, frame=f), sc.right)


def test_batched_entry_refusals_compute_nothing():
    run = run_batch("160x208", True, "current", 37)
    torch, sc0 = run["torch"], run["frames"][0]
    fresh = plp.orb_extractor(sc0.K, sc0.scale, sc0.levels)                       # has not run
    other = plp.orb_extractor(sc0.K, sc0.scale, sc0.levels)                       # ran on another geometry
    o = S.scene("161x211")
    d_o = torch.from_numpy(np.stack([o.left] * B)).to("cuda:0")
    ecap = 2 * sc0.K + 64
    ok_, od_, oc_ = (torch.zeros((B, ecap, 28), dtype=torch.uint8, device="cuda:0"), torch.zeros((B, ecap, 32), dtype=torch.uint8, device="cuda:0"),
                     torch.zeros(B, dtype=torch.int32, device="cuda:0"))
    other.extract_batch(d_o, ok_, od_, oc_)
    torch.cuda.synchronize()
    for kw in (dict(cap=0), dict(cap=65536), dict(nb=B + 1), dict(right=other), dict(left=other), dict(right=fresh), dict(left=fresh)):
        with pytest.raises(plp.PlpError) as e:
            run["call"](**kw)
        assert e.value.status == plp.PLP_ERR_INVALID_ARG, kw
        torch.cuda.synchronize()
        assert (run["xr"] == GARBAGE).all() and (run["dep"] == GARBAGE).all(), kw
    check_batch(run)                                                              # and the same arguments, unrefused, compute
