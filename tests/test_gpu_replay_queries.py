"""plp_replay_point_queries_device / plp_replay_line_queries_device (k_replay_point_queries, k_replay_line_queries) against a numpy reference written here:
np.float32 additions, 2 * shift formed in float first, shifts whose sums round.  Every output array is compared whole, over a sentinel-filled buffer
with a tail: what the kernels write for the slots at or above a frame's count is pinned as well as what they write below it, and nothing is written
behind an array.  Counts run below 0 and above cap (clamped), cap runs around the 256-lane block.  No tolerance: bytes."""
import numpy as np
import pytest
import torch

import oracle_lib as O
from plp import plp

pytestmark = pytest.mark.gpu

f32 = np.float32
TAIL, SENT = 64, 0xA5
SHIFT = (-3.3, 0.7)
CAPS, BS = (1, 255, 256, 257, 600), (1, 3)


def dev():
    return torch.device("cuda", 0)


def up(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev())


def counts_for(frames, cap, turn):
    """-3, 0, cap, cap + 9 and one in between, dealt round the frames from position `turn`: over five turns every frame meets every value"""
    vals = [cap + 9, -3, 0, cap, cap // 2]
    return np.array([vals[(f + turn) % 5] for f in range(frames)], np.int32)


def keypoints(rng, frames, cap):
    k = np.zeros((frames, cap), O.KP_DTYPE)                  # every slot looks alive, also those at or above its frame's count
    k["x"] = rng.uniform(0, 640, (frames, cap)); k["y"] = rng.uniform(0, 480, (frames, cap)); k["angle"] = rng.uniform(0, 360, (frames, cap))
    k["octave"] = rng.integers(0, 8, (frames, cap)); k["size"] = 31; k["response"] = rng.uniform(0, 1, (frames, cap)); k["class_id"] = -1
    return k


def keylines(rng, frames, cap):
    k = np.zeros((frames, cap), O.KL_DTYPE)
    for name in ("startPointX", "endPointX"):
        k[name] = rng.uniform(0, 640, (frames, cap))
    for name in ("startPointY", "endPointY"):
        k[name] = rng.uniform(0, 480, (frames, cap))
    k["octave"] = rng.integers(0, 3, (frames, cap)); k["angle"] = rng.uniform(-3, 3, (frames, cap)); k["lineLength"] = rng.uniform(10, 90, (frames, cap))
    return k


def shifted(x, y, sx, sy):
    return np.stack([np.asarray(x, f32) + sx, np.asarray(y, f32) + sy], -1)         # float32 + float32, one rounding each


def ref_points(kps, counts, halo, B, cap, shift):
    sx, sy = f32(shift[0]), f32(shift[1])
    sx2, sy2 = f32(f32(2) * sx), f32(f32(2) * sy)
    c = np.clip(counts, 0, cap)
    i = np.arange(cap)
    out = dict(q1_reproj=np.zeros((B, cap, 2), f32), q1_level=np.zeros((B, cap), np.int32), q1_angle=np.zeros((B, cap), f32), q1_counts=np.zeros(B, np.int32),
               q2_reproj=np.zeros((B, 2 * cap, 2), f32), q2_level=np.zeros((B, 2 * cap), np.int32), q2_valid=np.zeros((B, 2 * cap), np.uint8))
    for b in range(B):
        k1, k2 = kps[halo + b - 1], kps[halo + b - 2]
        out["q1_reproj"][b] = shifted(k1["x"], k1["y"], sx, sy); out["q1_level"][b] = k1["octave"]; out["q1_angle"][b] = k1["angle"]
        out["q1_counts"][b] = c[halo + b - 1]
        out["q2_reproj"][b, :cap] = shifted(k2["x"], k2["y"], sx2, sy2); out["q2_reproj"][b, cap:] = out["q1_reproj"][b]
        out["q2_level"][b, :cap] = k2["octave"]; out["q2_level"][b, cap:] = k1["octave"]
        out["q2_valid"][b, :cap] = i < c[halo + b - 2]; out["q2_valid"][b, cap:] = i < c[halo + b - 1]
    return out


def ref_lines(kl, counts, halo, B, cap, shift, q2, kps, kp_counts, kp_cap):
    sx, sy = f32(shift[0]), f32(shift[1])
    sx2, sy2 = f32(f32(2) * sx), f32(f32(2) * sy)
    c = np.clip(counts, 0, cap)
    i = np.arange(cap)
    out = dict(q_sp=np.zeros((B, cap, 2), f32), q_ep=np.zeros((B, cap, 2), f32), q_level=np.zeros((B, cap), np.int32), q_counts=np.zeros(B, np.int32))
    if q2:
        out.update(q2_sp=np.zeros((B, 2 * cap, 2), f32), q2_ep=np.zeros((B, 2 * cap, 2), f32), q2_level=np.zeros((B, 2 * cap), np.int32),
                   q2_valid=np.zeros((B, 2 * cap), np.uint8))
    if kps is not None:
        out["t_kp_octave"] = np.zeros((B, cap), np.int32)
    for b in range(B):
        k1 = kl[halo + b - 1]
        out["q_sp"][b] = shifted(k1["startPointX"], k1["startPointY"], sx, sy); out["q_ep"][b] = shifted(k1["endPointX"], k1["endPointY"], sx, sy)
        out["q_level"][b] = k1["octave"]; out["q_counts"][b] = c[halo + b - 1]
        if q2:
            k2 = kl[halo + b - 2]
            out["q2_sp"][b, :cap] = shifted(k2["startPointX"], k2["startPointY"], sx2, sy2); out["q2_sp"][b, cap:] = out["q_sp"][b]
            out["q2_ep"][b, :cap] = shifted(k2["endPointX"], k2["endPointY"], sx2, sy2); out["q2_ep"][b, cap:] = out["q_ep"][b]
            out["q2_level"][b, :cap] = k2["octave"]; out["q2_level"][b, cap:] = k1["octave"]
            out["q2_valid"][b, :cap] = i < c[halo + b - 2]; out["q2_valid"][b, cap:] = i < c[halo + b - 1]
        if kps is not None:
            nk = int(np.clip(kp_counts[halo + b], 0, kp_cap))
            m = min(nk, cap)
            out["t_kp_octave"][b, :m] = kps[halo + b, :m]["octave"]           # 0 where frame b has no key point with the line's index
    return out


def buffers(want):
    return {k: torch.full((v.nbytes + TAIL,), SENT, dtype=torch.uint8, device=dev()) for k, v in want.items()}


def assert_whole(got, want):
    torch.cuda.synchronize()
    for k, v in want.items():
        assert got[k].cpu().numpy().tobytes() == v.tobytes() + bytes([SENT]) * TAIL, k


def assert_untouched(got):
    torch.cuda.synchronize()
    for k, v in got.items():
        assert (v == SENT).all().item(), k


POINT_OUT = ("q1_reproj", "q1_level", "q1_angle", "q1_counts", "q2_reproj", "q2_level", "q2_valid")
LINE_OUT = ("q_sp", "q_ep", "q_level", "q_counts", "q2_sp", "q2_ep", "q2_level", "q2_valid")


def call_points(d_kps, d_counts, halo, B, cap, shift, out):
    p = lambda k: out[k].data_ptr() if out.get(k) is not None else None
    return plp.lib().plp_replay_point_queries_device(d_kps.data_ptr(), d_counts.data_ptr(), halo, B, cap, float(shift[0]), float(shift[1]),
                                                     *[p(k) for k in POINT_OUT], torch.cuda.current_stream(dev()).cuda_stream)


def call_lines(d_kl, d_counts, halo, B, cap, shift, out, d_kps=None, d_kp_counts=None, kp_cap=0):
    p = lambda k: out[k].data_ptr() if out.get(k) is not None else None
    q = lambda t: t.data_ptr() if t is not None else None
    return plp.lib().plp_replay_line_queries_device(d_kl.data_ptr(), d_counts.data_ptr(), halo, B, cap, float(shift[0]), float(shift[1]),
                                                    *[p(k) for k in LINE_OUT], q(d_kps), q(d_kp_counts), kp_cap, p("t_kp_octave"),
                                                    torch.cuda.current_stream(dev()).cuda_stream)


def test_the_shifts_round():
    """the sums are not exact, and 2 * shift in float is not the double product narrowed: the order of the operations shows in the bits"""
    x = np.arange(1, 600, dtype=f32) * f32(1.37)
    assert (x.astype(np.float64) + float(f32(SHIFT[0])) != (x + f32(SHIFT[0])).astype(np.float64)).any()
    two = x + f32(f32(2) * f32(SHIFT[0]))
    assert (two != (x + f32(SHIFT[0])) + f32(SHIFT[0])).any()                  # adding the shift twice is another number


@pytest.mark.parametrize("halo", (2, 3))
@pytest.mark.parametrize("B", BS)
@pytest.mark.parametrize("cap", CAPS)
def test_point_queries_equal_numpy(cap, B, halo):
    rng = np.random.default_rng(cap * 100 + B * 10 + halo)
    kps = keypoints(rng, halo + B, cap)
    d_kps = up(kps)
    for turn in range(5):
        counts = counts_for(halo + B, cap, turn)
        want = ref_points(kps, counts, halo, B, cap, SHIFT)
        got = buffers(want)
        assert call_points(d_kps, up(counts), halo, B, cap, SHIFT, got) == plp.PLP_OK
        assert_whole(got, want)
        assert want["q1_counts"].min() >= 0 and want["q1_counts"].max() <= cap


LINE_CASES = [(cap, B, halo, q2, kp) for cap in CAPS for B in BS for halo, q2 in ((1, False), (2, False), (2, True), (3, True)) for kp in (None, -5, 5)
              if kp is None or cap + kp > 0]


@pytest.mark.parametrize("cap,B,halo,q2,kp", LINE_CASES)
def test_line_queries_equal_numpy(cap, B, halo, q2, kp):
    rng = np.random.default_rng(cap * 1000 + B * 100 + halo * 10 + q2)
    kl = keylines(rng, halo + B, cap)
    d_kl = up(kl)
    kp_cap = 0 if kp is None else cap + kp
    kps = keypoints(rng, halo + B, kp_cap) if kp is not None else None
    d_kps = up(kps) if kps is not None else None
    for turn in range(5):
        counts = counts_for(halo + B, cap, turn)
        kp_counts = counts_for(halo + B, kp_cap, turn + 2) if kps is not None else None        # -3, 0, kp_cap // 2 (below most line indices), kp_cap, kp_cap + 9
        want = ref_lines(kl, counts, halo, B, cap, SHIFT, q2, kps, kp_counts, kp_cap)
        got = buffers(want)
        st = call_lines(d_kl, up(counts), halo, B, cap, SHIFT, got, d_kps, up(kp_counts) if kps is not None else None, kp_cap)
        assert st == plp.PLP_OK
        assert_whole(got, want)


def point_problem(halo=2, B=2, cap=9):
    rng = np.random.default_rng(3)
    kps = keypoints(rng, halo + B, cap)
    counts = counts_for(halo + B, cap, 0)
    return kps, counts, buffers(ref_points(kps, counts, halo, B, cap, SHIFT))


def test_point_queries_argument_checks_write_nothing():
    kps, counts, got = point_problem()
    d_kps, d_counts = up(kps), up(counts)
    for halo, B, cap in ((1, 2, 9), (0, 2, 9), (2, 0, 9), (2, 2, 0)):
        assert call_points(d_kps, d_counts, halo, B, cap, SHIFT, got) == plp.PLP_ERR_INVALID_ARG, (halo, B, cap)
    for k in POINT_OUT:
        assert call_points(d_kps, d_counts, 2, 2, 9, SHIFT, {**got, k: None}) == plp.PLP_ERR_INVALID_ARG, k
    assert_untouched(got)


def test_line_queries_argument_checks_write_nothing():
    halo, B, cap, kp_cap = 2, 2, 9, 7
    rng = np.random.default_rng(4)
    kl, kps = keylines(rng, halo + B, cap), keypoints(rng, halo + B, kp_cap)
    counts, kp_counts = counts_for(halo + B, cap, 0), counts_for(halo + B, kp_cap, 1)
    got = buffers(ref_lines(kl, counts, halo, B, cap, SHIFT, True, kps, kp_counts, kp_cap))
    d_kl, d_counts, d_kps, d_kp_counts = up(kl), up(counts), up(kps), up(kp_counts)
    bad = plp.PLP_ERR_INVALID_ARG
    no_q2 = {k: v for k, v in got.items() if not k.startswith("q2_")}
    assert call_lines(d_kl, d_counts, 0, B, cap, SHIFT, no_q2, d_kps, d_kp_counts, kp_cap) == bad               # halo too small without the landmark queries
    assert call_lines(d_kl, d_counts, 1, B, cap, SHIFT, got, d_kps, d_kp_counts, kp_cap) == bad                 # ... and with them
    q2_names = [k for k in LINE_OUT if k.startswith("q2_")]
    for k in q2_names:                                                                                          # a partial q2_* set: one missing, one alone
        assert call_lines(d_kl, d_counts, halo, B, cap, SHIFT, {**got, k: None}, d_kps, d_kp_counts, kp_cap) == bad, k
        assert call_lines(d_kl, d_counts, halo, B, cap, SHIFT, {**no_q2, k: got[k]}, d_kps, d_kp_counts, kp_cap) == bad, k
    assert call_lines(d_kl, d_counts, halo, B, cap, SHIFT, got, None, d_kp_counts, kp_cap) == bad               # t_kp_octave without its inputs
    assert call_lines(d_kl, d_counts, halo, B, cap, SHIFT, got, d_kps, None, kp_cap) == bad
    assert call_lines(d_kl, d_counts, halo, B, cap, SHIFT, got, d_kps, d_kp_counts, 0) == bad
    for k in ("q_sp", "q_ep", "q_level", "q_counts"):
        assert call_lines(d_kl, d_counts, halo, B, cap, SHIFT, {**got, k: None}, d_kps, d_kp_counts, kp_cap) == bad, k
    assert call_lines(d_kl, d_counts, halo, 0, cap, SHIFT, got, d_kps, d_kp_counts, kp_cap) == bad
    assert call_lines(d_kl, d_counts, halo, B, 0, SHIFT, got, d_kps, d_kp_counts, kp_cap) == bad
    assert_untouched(got)
