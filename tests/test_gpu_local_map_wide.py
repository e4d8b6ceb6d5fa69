"""module::local_map_updater on the device at the widths where a workgroup takes a second pass (csrc/local_map_kernels.hip: 512 lanes over the key
frames, a frame's slots and a key frame's candidates, 256 over the slots a block marks, 64 over a children run), on the wide scenes of
tests/local_map_scene.py.  The host build runs the same steps with a team of one lane, for which a pass is the whole loop, so what is carried
from pass to pass and from wave to wave is checked here alone: exact equality of every output with the restatement tests/local_map_ref.py over
sentinel-filled device arrays.  tests/test_local_map_wide_cpu.py shows that each scene reaches its second pass and that dropping it changes the
answer."""
import numpy as np
import pytest

import local_map_ref as R
import local_map_scene as S
from plp import plp
from test_gpu_local_map import check_device, enqueue, frame_bytes
from test_local_map_cpu import results, roomy, sentinels
from test_local_map_wide_cpu import wide_caps

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mt():
    return plp.matcher()


@pytest.mark.parametrize("name", list(S.WIDE_SCENES))
def test_device_equals_restatement(mt, name):
    check_device(mt, name, *roomy(name))


@pytest.mark.parametrize("i", range(9))
def test_device_at_the_caps(mt, i):
    """k_cap, m_cap and ml_cap at the true length - 1, at it and one past it, each more than 512 entries into its list"""
    name, kc, mc, mlc, st, n = wide_caps()[i]
    assert n - 1 > 512
    want = check_device(mt, name, kc, mc, mlc)
    assert want["status"][0] == st


@pytest.mark.parametrize("frames", [1, 4])
@pytest.mark.parametrize("name", ["deep_kf", "wide_f"])
def test_frames_split_into_chunks_at_misaligned_bases(mt, name, frames):
    """a mark table of one frame, and of four of the six; every base one element past an allocation's"""
    sc = S.scene(name)
    assert sc["frm_lm"].shape[0] == 6
    check_device(mt, name, *roomy(name), shift=True, workspace_bytes=1 if frames == 1 else frames * frame_bytes(sc) + 5)


@pytest.mark.parametrize("name", ["wide_f", "deep_lines", "hub"])
def test_host_entry_equals_restatement(mt, name):
    sc = S.scene(name)
    kc, mc, mlc = roomy(name)
    want = R.expected(results(name), kc, mc, mlc, True)
    got = mt.local_map(k_cap=kc, m_cap=mc, ml_cap=mlc, out=sentinels(want), **S.call_args(sc))
    for k in want:
        assert np.array_equal(got[k], want[k]), (name, k, np.argwhere(got[k] != want[k])[:4].tolist())


def test_null_optionals_at_width(mt):
    """no counts and no erased flags: every row runs to its cap, 600 frame slots and more first local key frames than with the flags"""
    import torch
    sc = S.scene("wide_f")
    drop = ("kf_counts", "frm_counts", "kf_erased", "lm_erased")
    bare = dict(sc, **{k: None for k in drop})
    res = R.run_scene(bare, sc["max_kf"])
    assert len(res[0]["first"]) > len(results("wide_f")[0]["first"]) > 512
    kc, mc, mlc = roomy("wide_f")
    want = R.expected(res, kc, mc, mlc, True)
    out, _ = enqueue(mt, sc, kc, mc, mlc, want, drop=drop)
    torch.cuda.synchronize()
    for k in want:
        got = out[k].cpu().numpy().reshape(want[k].shape)
        assert np.array_equal(got, want[k]), (k, np.argwhere(got != want[k])[:4].tolist())


def test_wide_and_small_calls_in_a_row_on_a_fresh_context():
    """wide, small and wide again on one stream of a context that has held nothing yet: each mark table is larger than the one before the small
    call, so the context's buffers regrow, and a call's table holds nothing of the call before it"""
    import torch
    mt = plp.matcher()
    order = ("deep_lines", "f1", "deep_kf", "f63", "wide_f", "cap_max_more", "hub")
    sizes = [frame_bytes(S.scene(n)) * S.scene(n)["frm_lm"].shape[0] for n in order]
    assert sizes[0] < sizes[2] and sizes[1] < sizes[0] and sizes[3] < sizes[2]
    outs = []
    for name in order:
        sc = S.scene(name)
        want = R.expected(results(name), *roomy(name), sc["kf_lm_lines"] is not None)
        outs.append((name, want, enqueue(mt, sc, *roomy(name), want)))
    torch.cuda.synchronize()
    for name, want, (out, _) in outs:
        for k in want:
            got = out[k].cpu().numpy().reshape(want[k].shape)
            assert np.array_equal(got, want[k]), (name, k, np.argwhere(got != want[k])[:4].tolist())
