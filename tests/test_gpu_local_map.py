"""module::local_map_updater on the device (plp_local_map_device / _host, csrc/local_map_kernels.hip) against the restatement of DESIGN.md
section 5, D18 (tests/local_map_ref.py), on the scenes tests/test_local_map_cpu.py holds the host build to: exact equality of every output over
sentinel-filled arrays.  The widths the kernels use: the workgroup of 512 lanes of k_local_map_keyframes and k_local_map_compact (the stride of
the loops over key frames, frame slots and candidates: F = 130 and rows of at most 70 slots stay inside one pass of it, so the caps of 63 .. 70
slots sit around the wave of 64 instead, which is what the ballots and the children tiles work in), the 256 lanes of k_local_map_mark, and the
chunk of frames that shares one mark table.  The scenes in which a workgroup takes a second pass are those of tests/test_gpu_local_map_wide.py."""
import numpy as np
import pytest

import local_map_ref as R
import local_map_scene as S
from plp import plp
from test_local_map_cpu import EDGE, edge_caps, results, roomy, sentinels

pytestmark = pytest.mark.gpu
TABLES = ("kf_erased", "kf_covis", "kf_parent", "kf_children_offsets", "kf_children", "kf_lm", "kf_counts", "kf_lm_lines", "kf_kl_counts", "obs_offsets",
          "obs_kf", "lm_erased", "lm_erased_lines", "frm_lm", "frm_counts", "frm_lm_lines", "frm_kl_counts")


@pytest.fixture(scope="module")
def mt():
    return plp.matcher()


def frame_bytes(sc):
    rows = max(len(sc["obs_offsets"]) - 1, sc["LL"])
    return 4 * (rows + (rows + 31) // 32)


def dims_of(sc, k_cap, m_cap, ml_cap):
    lines = sc["kf_lm_lines"] is not None
    return dict(B=sc["frm_lm"].shape[0], F=len(sc["kf_parent"]), C=len(sc["kf_children"]), L=len(sc["obs_offsets"]) - 1, LL=sc["LL"], T=len(sc["obs_kf"]),
                cap=sc["cap"], lcap=sc["lcap"], fcap=sc["fcap"], flcap=sc["flcap"], frm_stride=sc["frm_lm"].shape[1],
                frm_stride_lines=sc["frm_lm_lines"].shape[1] if lines else 0, k_cap=k_cap, m_cap=m_cap, ml_cap=ml_cap)


def to_device(v, shift):
    """the array on the device; shift: its base one element past an allocation's (4 bytes for the i32 tables, 1 for the bytes)"""
    import torch
    if v is None:
        return None
    t = torch.from_numpy(np.ascontiguousarray(v).reshape(-1))
    if not shift:
        return t.cuda()
    buf = torch.zeros(t.numel() + 2, dtype=t.dtype, device="cuda")
    buf[1:1 + t.numel()] = t.cuda()
    return buf[1:1 + t.numel()]


def enqueue(mt, sc, k_cap, m_cap, ml_cap, want, shift=False, drop=(), stream=None, **kw):
    """plp_local_map_device on sentinel-filled device outputs; nothing is synchronised"""
    dev = {k: to_device(sc[k], shift) for k in TABLES if k not in drop}
    out = {k: to_device(v, shift) for k, v in sentinels(want).items()}
    mt.local_map_device(dims_of(sc, k_cap, m_cap, ml_cap), dev, {k: v for k, v in out.items() if v.numel() and k not in drop},
                        max_num_local_keyfrms=sc["max_kf"], stream=stream, **kw)
    return out, dev


def check_device(mt, name, k_cap, m_cap, ml_cap, **kw):
    import torch
    sc = S.scene(name)
    want = R.expected(results(name), k_cap, m_cap, ml_cap, sc["kf_lm_lines"] is not None)
    out, _ = enqueue(mt, sc, k_cap, m_cap, ml_cap, want, **kw)
    torch.cuda.synchronize()
    for k in want:
        got = out[k].cpu().numpy().reshape(want[k].shape)
        assert np.array_equal(got, want[k]), (name, k, np.argwhere(got != want[k])[:4].tolist())
    return want


@pytest.mark.parametrize("name", list(S.SCENES))
def test_device_equals_restatement(mt, name):
    check_device(mt, name, *roomy(name))


@pytest.mark.parametrize("name", list(S.SCENES))
def test_host_entry_equals_restatement(mt, name):
    sc = S.scene(name)
    kc, mc, mlc = roomy(name)
    want = R.expected(results(name), kc, mc, mlc, sc["kf_lm_lines"] is not None)
    got = mt.local_map(k_cap=kc, m_cap=mc, ml_cap=mlc, out=sentinels(want), **S.call_args(sc))
    for k in want:
        assert np.array_equal(got[k], want[k]), (name, k)


@pytest.mark.parametrize("frames", [1, 4])
def test_frames_split_into_chunks(mt, frames):
    """a mark table of one frame, and of four of the six: the last chunk is ragged"""
    sc = S.scene("f130")
    assert sc["frm_lm"].shape[0] == 6
    ws = 1 if frames == 1 else frames * frame_bytes(sc) + 5
    check_device(mt, "f130", *roomy("f130"), workspace_bytes=ws)
    kc, mc, mlc = roomy("f130")
    want = R.expected(results("f130"), kc, mc, mlc, True)
    got = mt.local_map(k_cap=kc, m_cap=mc, ml_cap=mlc, out=sentinels(want), workspace_bytes=ws, **S.call_args(sc))
    for k in want:
        assert np.array_equal(got[k], want[k]), k


def test_misaligned_bases_and_padded_stride(mt):
    """every base one element past an allocation's; f65's frame rows are three slots wider than fcap"""
    assert S.scene("f65")["frm_lm"].shape[1] == S.scene("f65")["fcap"] + 3
    check_device(mt, "f65", *roomy("f65"), shift=True)
    check_device(mt, "f130_mid", *roomy("f130_mid"), shift=True, workspace_bytes=2 * frame_bytes(S.scene("f130_mid")))


def test_null_optionals(mt):
    """no counts, no erased flags, no first_weight, no line side"""
    import torch
    sc = S.scene("f63_points")
    drop = ("kf_counts", "frm_counts", "kf_erased", "lm_erased", "first_weight")
    bare = dict(sc, kf_counts=None, frm_counts=None, kf_erased=None, lm_erased=None)
    kc, mc, mlc = roomy("f63_points")
    want = R.expected(R.run_scene(bare, sc["max_kf"]), kc, mc, mlc, False)
    out, _ = enqueue(mt, sc, kc, mc, mlc, want, drop=drop)
    torch.cuda.synchronize()
    for k in want:
        ref = sentinels(want)[k] if k == "first_weight" else want[k]
        assert np.array_equal(out[k].cpu().numpy().reshape(ref.shape), ref), k


@pytest.mark.parametrize("i", range(9))
def test_device_at_the_caps(mt, i):
    kc, mc, mlc, st = edge_caps()[i]
    want = check_device(mt, EDGE[0], kc, mc, mlc)
    assert want["status"][EDGE[1]] == st


def test_two_calls_in_a_row_on_one_context(mt):
    """different shapes back to back on one stream: the second call's mark table holds nothing of the first"""
    import torch
    outs = []
    for name in ("f130", "f63", "f130_mid", "f1"):
        sc = S.scene(name)
        want = R.expected(results(name), *roomy(name), sc["kf_lm_lines"] is not None)
        outs.append((name, want, enqueue(mt, sc, *roomy(name), want)))
    torch.cuda.synchronize()
    for name, want, (out, _) in outs:
        for k in want:
            assert np.array_equal(out[k].cpu().numpy().reshape(want[k].shape), want[k]), (name, k)


def test_refusals_write_nothing(mt):
    import torch
    sc = S.scene("f1")
    kc, mc, mlc = roomy("f1")
    want = R.expected(results("f1"), kc, mc, mlc, True)
    dev = {k: to_device(sc[k], False) for k in TABLES}
    out = {k: to_device(v, False) for k, v in sentinels(want).items()}

    def code(drop=(), **over):
        with pytest.raises(plp.PlpError) as e:
            mt.local_map_device({**dims_of(sc, kc, mc, mlc), **over}, {k: v for k, v in dev.items() if k not in drop},
                                {k: v for k, v in out.items() if k not in drop}, max_num_local_keyfrms=over.pop("max_kf", 60))
        return e.value.status
    for bad in (dict(B=-1), dict(F=-1), dict(T=-1), dict(cap=-1), dict(k_cap=-1), dict(m_cap=-1), dict(ml_cap=-1), dict(frm_stride=3)):
        assert code(**bad) == plp.PLP_ERR_INVALID_ARG, bad
    for drop in ("kf_covis", "kf_parent", "kf_children_offsets", "kf_lm", "obs_offsets", "obs_kf", "frm_lm", "status", "num_kf", "local_kf", "nearest_kf",
                 "num_lm", "local_lm", "held", "num_lines", "local_lines", "held_lines"):
        assert code(drop=(drop,)) == plp.PLP_ERR_INVALID_ARG, drop
    for bad in (dict(F=plp.LOCAL_MAP_MAX_KF + 1), dict(cap=plp.LOCAL_MAP_MAX_SLOTS + 1), dict(fcap=plp.LOCAL_MAP_MAX_SLOTS + 1, frm_stride=0),
                dict(lcap=plp.LOCAL_MAP_MAX_SLOTS + 1), dict(B=plp.LOCAL_MAP_MAX_FRAMES + 1), dict(k_cap=1 << 26, cap=64)):
        assert code(**bad) == plp.PLP_ERR_UNSUPPORTED, bad
    mt.local_map_device({**dims_of(sc, kc, mc, mlc), "B": 0}, dev, out)          # B == 0: PLP_OK, nothing written
    torch.cuda.synchronize()
    for k, v in sentinels(want).items():
        assert np.array_equal(out[k].cpu().numpy().reshape(v.shape), v), k
    with pytest.raises(plp.PlpError) as e:                                        # _host: the offsets are checked
        mt.local_map(k_cap=kc, m_cap=mc, ml_cap=mlc, **S.call_args(sc, kf_children_offsets=np.array([0, 3], np.int32)))
    assert e.value.status == plp.PLP_ERR_INVALID_ARG
