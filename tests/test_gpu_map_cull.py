"""module::local_map_cleaner on the device (plp_cull_keyframes_* / plp_cull_landmarks_*, csrc/map_cull_kernels.hip) against the object-level
restatement tests/map_cull_ref.py, on the scenes tests/test_map_cull_cpu.py holds the host build to: exact equality of every output over
sentinel-filled arrays.  The widths the kernels use are in the scenes: the workgroup of 256 lanes (key frames of 257 key points, fresh lists of
257 and 300 entries), the wave of 64 (63 .. 65 key points, lists that end mid-wave), the bitmap words of the removed set (F = 65 and 97), one
workgroup per entry of lists of 0, 1 and more than 64 entries."""
import numpy as np
import pytest

import map_cull_ref as R
import map_cull_scene as S
from plp import plp
from test_map_cull_cpu import equal, lm_results, results, sentinels

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mt():
    return plp.matcher()


def to_device(v, shift=False):
    """the array on the device; shift: its base one element past an allocation's"""
    import torch
    if v is None:
        return None
    a = np.ascontiguousarray(v)
    if a.dtype.fields is not None:
        a = a.view(np.uint8).reshape(a.shape + (-1,))
    elif a.dtype == np.uint32:
        a = a.view(np.int32)
    shape = a.shape
    t = torch.from_numpy(a.reshape(-1))
    if not shift:
        return t.cuda().reshape(shape)
    unit = 28 if shape[-1:] == (28,) and a.dtype == np.uint8 and len(shape) == 3 else 1
    buf = torch.zeros(t.numel() + 2 * unit, dtype=t.dtype, device="cuda")
    buf[unit:unit + t.numel()] = t.cuda()
    return buf[unit:unit + t.numel()].reshape(shape)


def dims_of(sc):
    return dict(F=sc["kf_lm"].shape[0], L=len(sc["obs_offsets"]) - 1, T=len(sc["obs_kf"]), cap=sc["kf_lm"].shape[1], kp_stride=sc["undist"].shape[1],
                G=len(sc["cur_kf"]), Cv=len(sc["covis"]))


def enqueue(mt, sc, want, shift=False, drop=(), drop_out=()):
    """plp_cull_keyframes_device on sentinel-filled device outputs, without the tables of `drop` and the outputs of `drop_out`; nothing is
    synchronised"""
    dev = {k: to_device(sc[k], shift) for k in S.KF_TABLES if k not in drop}
    out = {k: to_device(v, shift) for k, v in sentinels(want).items()}
    mt.cull_keyframes_device(dims_of(sc), dev, {k: v for k, v in out.items() if v.numel() and k not in drop_out}, origin_id=sc["origin_id"],
                             is_monocular=bool(sc["is_monocular"]))
    return out, dev


def fetch(out, want):
    import torch
    torch.cuda.synchronize()
    return {k: out[k].cpu().numpy().reshape(want[k].shape).view(want[k].dtype) for k in want}


@pytest.mark.parametrize("name", S.SCENES)
def test_device_equals_restatement(mt, name):
    """mono65 and stereo97 hold G > 1 problems with ragged lists, an empty list and one of a single entry"""
    sc = S.scene(name)
    want = R.expected_keyframes(results(name), sc)
    equal(fetch(enqueue(mt, sc, want)[0], want), want, name)


@pytest.mark.parametrize("name", S.SCENES)
def test_host_entry_equals_restatement(mt, name):
    sc = S.scene(name)
    want = R.expected_keyframes(results(name), sc)
    equal(mt.cull_keyframes(out=sentinels(want), **S.call_args(sc)), want, name)


def test_misaligned_bases(mt):
    """every base one element past an allocation's"""
    sc = S.scene("stereo97")
    want = R.expected_keyframes(results("stereo97"), sc)
    equal(fetch(enqueue(mt, sc, want, shift=True)[0], want), want, "shifted")


def test_padded_kp_stride(mt):
    """undist, x_right and depths in rows of cap + 7 key points; kf_lm keeps cap"""
    sc = S.scene("rgbd65")
    F, cap = sc["kf_lm"].shape
    pad = dict(sc)
    for k, fill in (("undist", 0), ("x_right", 5.0), ("depths", -3.0)):
        wide = np.full((F, cap + 7), fill, sc[k].dtype) if k != "undist" else np.zeros((F, cap + 7), sc[k].dtype)
        wide[:, :cap] = sc[k]
        pad[k] = wide
    want = R.expected_keyframes(results("rgbd65"), sc)
    equal(fetch(enqueue(mt, pad, want)[0], want), want, "padded")
    equal(mt.cull_keyframes(out=sentinels(want), **S.call_args(pad)), want, "padded, host entry")


def test_null_optionals_leave_optional_outputs_untouched(mt):
    """without kf_erased, and with the two optional outputs not given: their sentinel-filled arrays stay as they are"""
    sc = S.scene("mono97")
    want = R.expected_keyframes(results("mono97"), sc)
    out, _ = enqueue(mt, sc, want, drop=("kf_erased",), drop_out=("kf_removed", "lm_erased"))
    got = fetch(out, want)
    for k in ("kf_removed", "lm_erased"):
        assert (got[k] == R.SENTINEL[k]).all(), k
        want[k] = got[k]
    equal(got, want, "no optional outputs")
    nul = dict(S.scene("mono65"), x_right=None, kf_cannot_erase=None, lm_erased=None, kf_counts=None, lm_num_obs=None)
    nwant = R.expected_keyframes([R.remove_redundant_keyframes(nul, g) for g in range(len(nul["cur_kf"]))], nul)
    equal(fetch(enqueue(mt, nul, nwant)[0], nwant), nwant, "NULL tables")


def test_two_calls_back_to_back(mt):
    """the context's count buffer and removed sets serve both calls, the larger one first; one synchronisation at the end"""
    a, b = S.scene("stereo97"), S.scene("mono65")
    wa, wb = R.expected_keyframes(results("stereo97"), a), R.expected_keyframes(results("mono65"), b)
    oa, keep_a = enqueue(mt, a, wa)
    ob, keep_b = enqueue(mt, b, wb)
    oa2, keep_a2 = enqueue(mt, a, wa)
    equal(fetch(oa, wa), wa, "first call")
    equal(fetch(ob, wb), wb, "second call")
    equal(fetch(oa2, wa), wa, "third call")


def lm_enqueue(mt, sc, want, shift=False):
    dev = {k: to_device(sc[k], shift) for k in S.LM_TABLES}
    out = {k: to_device(v, shift) for k, v in sentinels(want).items()}
    mt.cull_landmarks_device(dict(R=len(sc["cur_kf_id"]), N=len(sc["fresh"]), L=len(sc["num_observed"])), dev, out)
    return out, dev


@pytest.mark.parametrize("name", list(S.LM_SCENES))
@pytest.mark.parametrize("shift", [False, True])
def test_landmark_states_and_compacted_lists(mt, name, shift):
    """lists of 0, 1, 70, 300 and 257 entries: the compacted list ends mid-wave, crosses the workgroup and ends one past it"""
    sc, want = S.lm_scene(name), lm_results(name)
    equal(fetch(lm_enqueue(mt, sc, want, shift)[0], want), want, name)
    if not shift:
        equal(mt.cull_landmarks(out=sentinels(want), **S.lm_call_args(sc)), want, name + ", host entry")


def test_mirror_class_on_the_device(mt):
    sc = S.scene("mono97")
    cl = plp.local_map_cleaner(is_monocular=True, mt=mt)
    cl.set_origin_keyframe_id(sc["origin_id"])
    assert cl.remove_redundant_keyframes(int(sc["cur_kf"][0]), sc["covis"], sc) == results("mono97")[0]["num_removed"]
    assert np.array_equal(cl.last["lm_erased"][0], results("mono97")[0]["lm_erased"])
