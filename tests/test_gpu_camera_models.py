"""Post-extract step for the reference's three camera models (plp_post_extract_model_*): perspective equals the perspective-only entry
bit for bit; fisheye and equirectangular against the CPU restatement in tests/camera_models_ref.py (f64 tan / sin / cos of the device
are not glibc's: DESIGN.md section 5, D4)."""
import ctypes as C

import numpy as np
import pytest
from PIL import Image

import camera_models_ref as R
import oracle_lib as O
from plp import plp, synth

pytestmark = pytest.mark.gpu

# the five cameras of tests/test_gpu_post_extract.py (fx, fy, cx, cy, k1, k2, p1, p2, k3, focal_x_baseline)
CAMS = {
    "fr1": (517.306408, 516.469215, 318.643040, 255.313989, 0.262383, -0.953104, -0.005358, 0.002628, 1.163314, 40.0),
    "fr2": (520.908620, 521.007327, 325.141442, 249.701764, 0.231222, -0.784899, -0.003257, -0.000105, 0.917205, 40.0),
    "fr3": (535.4, 539.2, 320.1, 247.6, 0.0, 0.0, 0.0, 0.0, 0.0, 40.0),
    "kitti": (718.856, 718.856, 607.1928, 185.2157, 0.0, 0.0, 0.0, 0.0, 0.0, 386.1448),
    "wide": (300.0, 305.0, 322.0, 241.0, -0.35, 0.12, 0.001, -0.0007, -0.02, 30.0),
}
NAMES10 = ("fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2", "k3", "focal_x_baseline")
TUM_VI_MONO = {"Camera.model": "fisheye", "Camera.cols": 512, "Camera.rows": 512,
               "Camera.fx": 190.97847715128717, "Camera.fy": 190.9733070521226, "Camera.cx": 254.93170605935475, "Camera.cy": 256.8974428996504,
               "Camera.k1": 0.0034823894022493434, "Camera.k2": 0.0007150348452162257, "Camera.k3": -0.0020532361418706202,
               "Camera.k4": 0.00020293673591811182, "Camera.focal_x_baseline": 30.0}
# made up: 100 px focal length on 512 x 512 puts the corners at 3.6 rad (clamped to pi / 2), the super-wide branch of the bounds
WIDE_FISHEYE = {**TUM_VI_MONO, "Camera.fx": 100.0, "Camera.fy": 100.0, "Camera.cx": 256.0, "Camera.cy": 256.0}
# made up: strong negative k1, Newton on theta leaves the valid branch for about half of the image: OpenCV's (-1e6, -1e6) result
DIVERGENT_FISHEYE = {**TUM_VI_MONO, "Camera.fx": 150.0, "Camera.fy": 150.0, "Camera.cx": 256.0, "Camera.cy": 256.0,
                     "Camera.k1": -0.5, "Camera.k2": 0.1, "Camera.k3": 0.0, "Camera.k4": 0.0}
# made up: a long focal length keeps the four corners in view, the normal branch of the fisheye bounds (TUM-VI's corners are at 1.9 rad)
NARROW_FISHEYE = {**TUM_VI_MONO, "Camera.fx": 380.0, "Camera.fy": 380.0, "Camera.cx": 256.0, "Camera.cy": 256.0}
EQUIRECT = {"Camera.model": "equirectangular", "Camera.cols": 1920, "Camera.rows": 960}


def cam_c(v):
    c = plp.camera_c()
    for n, x in zip(NAMES10, v):
        setattr(c, n, float(x))
    return c


def cam_model_c(v, model=plp.CAMERA_PERSPECTIVE, cols=640, rows=480):
    c = plp.camera_model_c()
    c.model, c.cols, c.rows = model, cols, rows
    for n, x in zip(NAMES10, v):
        setattr(c, n, float(x))
    return c


def ref_cam(cm):
    return {"model": {0: "perspective", 1: "fisheye", 2: "equirectangular"}[cm.model], "cols": cm.cols, "rows": cm.rows,
            **{k: getattr(cm, k) for k in ("fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2", "k3", "k4")}}


def within_ulp(got, want, n=1):
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    return np.abs(got.astype(np.float64) - want.astype(np.float64)) <= n * np.spacing(np.abs(want)).astype(np.float64)


def lattice(cols, rows, n=17):
    xs, ys = np.linspace(0, cols - 1, n, dtype=np.float32), np.linspace(0, rows - 1, n, dtype=np.float32)
    X, Y = np.meshgrid(xs, ys)
    k = np.zeros(n * n + 2, plp.KP_DTYPE)
    k["x"][:n * n] = X.ravel(); k["y"][:n * n] = Y.ravel()
    k["x"][n * n:] = [(cols - 1) / 2, cols / 2]; k["y"][n * n:] = [(rows - 1) / 2, rows / 2]   # the centre
    k["octave"] = np.arange(len(k)) % 8; k["angle"] = np.arange(len(k)) * 1.5; k["size"] = 31; k["response"] = 5.0; k["class_id"] = 7
    return k


@pytest.mark.parametrize("name", list(CAMS))
def test_perspective_model_entry_equals_the_perspective_entry(name):
    v = CAMS[name]
    rng = np.random.default_rng(5)
    img = synth.replay(3, 1, 480, 640)[0]
    kps, _ = O.OrbOracle(1500).extract(img)
    extra = np.zeros(6, O.KP_DTYPE)
    extra["x"] = [0, 639, 0, 639, 320.25, 19.5]; extra["y"] = [0, 0, 479, 479, 240.75, 460.0]
    kps = np.concatenate([kps, extra])
    depth = rng.uniform(0.3, 8.0, (480, 640)).astype(np.float32)
    depth[rng.uniform(size=depth.shape) < 0.2] = 0.0
    kl = np.zeros(40, O.KL_DTYPE)
    kl["startPointX"] = rng.uniform(0, 639, 40); kl["startPointY"] = rng.uniform(0, 479, 40)
    kl["endPointX"] = rng.uniform(0, 639, 40); kl["endPointY"] = rng.uniform(0, 479, 40)
    pre = np.full((40, 2), -1, np.float32)
    mt = plp.matcher()
    want = mt.post_extract(cam_c(v), kps, depth, kl, pre, pre)
    got = mt.post_extract(cam_model_c(v), kps, depth, kl, pre, pre)
    assert set(got) == set(want)
    for key in want:
        assert np.array_equal(got[key].view(np.uint8), want[key].view(np.uint8)), key
    assert (got["kl_depths"] >= 0).any()


def check_fisheye(cm, kps, label):
    out = plp.matcher().post_extract(cm, kps)
    u, b = out["undist_keypts"], out["bearings"]
    wx, wy = R.fisheye_undistort(ref_cam(cm), kps["x"], kps["y"])
    ok = within_ulp(u["x"], wx) & within_ulp(u["y"], wy)
    assert ok.all(), (label, kps[~ok][:4], u[~ok][:4], wx[~ok][:4], wy[~ok][:4])
    bit = (u["x"] == wx) & (u["y"] == wy)
    print(f"{label}: {len(kps)} points, undistorted x and y bit-equal to the restatement for {bit.mean():.4%}")
    assert np.array_equal(b, R.pinhole_bearings(ref_cam(cm), u["x"], u["y"]))      # IEEE-only formula on the GPU's own points
    assert (u["response"] == 0).all() and (u["class_id"] == -1).all()
    for f in ("angle", "size", "octave"):
        assert np.array_equal(u[f], kps[f]), f
    return u, wx


def test_fisheye_tum_vi_mono():
    cm = plp.camera_model(TUM_VI_MONO)
    img = synth.canvas(11, 512, 512)
    kps, _ = O.OrbOracle(1000).extract(img)
    assert len(kps) > 500
    kps = np.concatenate([kps, lattice(512, 512)])
    kps[-1]["x"], kps[-1]["y"] = np.float32(cm.cx), np.float32(cm.cy)   # the principal point itself
    u, _ = check_fisheye(cm, kps, "TUM-VI mono")
    assert u["x"][-1] == np.float32(cm.cx) and u["y"][-1] == np.float32(cm.cy)
    # depth: frame.cc:1169-1194 does not depend on the model
    rng = np.random.default_rng(8)
    depth = rng.uniform(0.5, 5.0, (512, 512)).astype(np.float32)
    depth[rng.uniform(size=depth.shape) < 0.2] = 0.0
    d = plp.matcher().post_extract(cm, kps, depth)
    assert np.array_equal(d["undist_keypts"], u)
    dv = depth[kps["y"].astype(np.int32), kps["x"].astype(np.int32)]
    assert np.array_equal(d["depths"], np.where(dv > 0, dv, -1).astype(np.float32))
    want_xr = np.array([np.float32(float(x) - 30.0 / float(z)) if z > 0 else -1 for x, z in zip(u["x"], dv)], np.float32)
    assert np.array_equal(d["stereo_x_right"], want_xr)


def test_fisheye_clamped_corners_and_sentinel():
    cm = plp.camera_model(WIDE_FISHEYE)
    k = lattice(512, 512, 33)
    pw = np.hypot((k["x"] - 256.0) / 100.0, (k["y"] - 256.0) / 100.0)
    assert (pw > np.pi / 2).sum() > 300                      # the theta_d clamp is exercised
    u, wx = check_fisheye(cm, k, "wide fisheye")
    assert (u["x"] != R.SENTINEL).all()
    cm = plp.camera_model(DIVERGENT_FISHEYE)
    u, wx = check_fisheye(cm, k, "divergent fisheye")
    bad = wx == R.SENTINEL
    assert 100 < bad.sum() < len(k) - 100
    assert np.array_equal(u["x"] == R.SENTINEL, bad) and (u["y"][bad] == R.SENTINEL).all()


@pytest.mark.parametrize("idx", [1, 2])
def test_equirectangular_end_to_end_on_the_reference_images(golden_dir, idx):
    img = np.asarray(Image.open(golden_dir / f"equirect{idx}_1920x960.png"), dtype=np.uint8)
    assert img.shape == (960, 1920)
    rects = [[0.0, 1.0, 0.0, 0.1], [0.0, 1.0, 0.9, 1.0]]     # Feature.mask_rectangles: the top and bottom bands of a 360 frame
    gk, gd = plp.orb_extractor(2000, mask_rects=rects).extract(img)
    ok, od = O.OrbOracle(2000, mask_rects=rects).extract(img)
    assert len(gk) > 1500 and np.array_equal(gk, ok) and np.array_equal(gd, od)
    assert (gk["y"] >= 96).all() and (gk["y"] < 864).all()
    cm = plp.camera_model(EQUIRECT)
    out = plp.matcher().post_extract(cm, gk)
    assert out["undist_keypts"].tobytes() == gk.tobytes()                 # undist = dist, every field
    want = R.equirect_bearings(ref_cam(cm), gk["x"], gk["y"])
    err = np.abs(out["bearings"] - want)
    print(f"equirect{idx}: {len(gk)} key points, bearings bit-equal {np.mean(err == 0):.4%} of components, max |diff| {err.max():.3g}")
    assert err.max() <= 1e-15
    assert np.abs(np.linalg.norm(out["bearings"], axis=1) - 1).max() <= 1e-15


def test_equirectangular_bearings_over_the_whole_image():
    cm = plp.camera_model(EQUIRECT)
    k = lattice(1920, 960, 65)
    k = np.concatenate([k, lattice(1921, 961, 3)])            # the right and bottom borders themselves (x = 1920, y = 960)
    b = plp.matcher().post_extract(cm, k)["bearings"]
    want = R.equirect_bearings(ref_cam(cm), k["x"], k["y"])
    assert np.abs(b - want).max() <= 1e-15
    c = np.nonzero((k["x"] == 960) & (k["y"] == 480))[0]
    assert len(c) and b[c[0]].tolist() == [0.0, 0.0, 1.0]


def frames_for(model):
    if model == plp.CAMERA_PERSPECTIVE:
        return cam_model_c(CAMS["fr1"]), 640, 480
    if model == plp.CAMERA_FISHEYE:
        return plp.camera_model(TUM_VI_MONO), 512, 512
    return plp.camera_model(EQUIRECT), 1920, 960


@pytest.mark.parametrize("model", [plp.CAMERA_PERSPECTIVE, plp.CAMERA_FISHEYE, plp.CAMERA_EQUIRECTANGULAR])
def test_batched_device_path(model):
    import torch
    cm, cols, rows = frames_for(model)
    B, cap = 3, 700
    counts = np.array([cap - 5, 311, 0], np.int32)
    rng = np.random.default_rng(20 + model)
    k = np.zeros((B, cap), plp.KP_DTYPE)
    k["x"] = rng.uniform(0, cols - 1, (B, cap)); k["y"] = rng.uniform(0, rows - 1, (B, cap))
    k["size"] = 31; k["angle"] = rng.uniform(0, 360, (B, cap)); k["octave"] = rng.integers(0, 8, (B, cap))
    k["response"] = rng.uniform(0, 100, (B, cap)); k["class_id"] = rng.integers(-1, 5, (B, cap))
    with_depth = model != plp.CAMERA_EQUIRECTANGULAR
    depth = rng.uniform(0.5, 6.0, (B, rows, cols)).astype(np.float32)
    dev = torch.device("cuda", 0)
    d_k = torch.from_numpy(k.view(np.uint8).reshape(B, cap, 28)).to(dev); d_c = torch.from_numpy(counts).to(dev)
    d_depth = torch.from_numpy(depth).to(dev)
    d_u = torch.full((B, cap, 28), 0xAB, dtype=torch.uint8, device=dev)               # pre-filled: slots past a count stay as they are
    d_b = torch.full((B, cap, 3), 7.0, dtype=torch.float64, device=dev)
    d_x = torch.full((B, cap), 9.0, dtype=torch.float32, device=dev); d_z = torch.full((B, cap), 9.0, dtype=torch.float32, device=dev)
    mt = plp.matcher()
    torch.cuda.synchronize()
    plp._check(plp.lib().plp_post_extract_model_device(mt._h, C.byref(cm), d_k.data_ptr(), d_c.data_ptr(), cap, B,
                                                       d_depth.data_ptr() if with_depth else None, rows, cols, cols * 4, rows * cols * 4,
                                                       d_u.data_ptr(), d_b.data_ptr(), d_x.data_ptr() if with_depth else None,
                                                       d_z.data_ptr() if with_depth else None, None, None, 0, None, None, None))
    torch.cuda.synchronize()
    u, b, x, z = d_u.cpu().numpy(), d_b.cpu().numpy(), d_x.cpu().numpy(), d_z.cpu().numpy()
    for f in range(B):
        n = int(counts[f])
        want = plp.matcher().post_extract(cm, k[f, :n], depth[f] if with_depth else None)
        assert np.array_equal(u[f, :n].view(plp.KP_DTYPE).reshape(n), want["undist_keypts"])
        assert np.array_equal(b[f, :n], want["bearings"])
        if with_depth:
            assert np.array_equal(x[f, :n], want["stereo_x_right"]) and np.array_equal(z[f, :n], want["depths"])
        assert (u[f, n:] == 0xAB).all() and (b[f, n:] == 7.0).all() and (x[f, n:] == 9.0).all() and (z[f, n:] == 9.0).all()
    if not with_depth:
        assert (x == 9.0).all() and (z == 9.0).all()


def test_grid_of_every_model():
    mt = plp.matcher()

    def gpu_undistort(cm):
        def f(xs, ys):
            k = np.zeros(len(xs), plp.KP_DTYPE); k["x"] = xs; k["y"] = ys; k["size"] = 1.0
            u = mt.post_extract(cm, k)["undist_keypts"]
            return u["x"].copy(), u["y"].copy()
        return f

    def oracle_undistort(v):
        def f(xs, ys):
            k = np.zeros(len(xs), O.KP_DTYPE); k["x"] = xs; k["y"] = ys; k["size"] = 1.0
            u = O.post_extract(v, k)["undist_keypts"]
            return u["x"].copy(), u["y"].copy()
        return f

    fr1 = {"Camera.model": "perspective", "Camera.cols": 640, "Camera.rows": 480,
           **{f"Camera.{n}": x for n, x in zip(NAMES10, CAMS["fr1"])}}
    cases = [(EQUIRECT, None), (fr1, oracle_undistort(CAMS["fr1"])), (TUM_VI_MONO, None), (WIDE_FISHEYE, None), (NARROW_FISHEYE, None)]
    for node, ref_undistort in cases:
        cm = plp.camera_model(node)
        b = cm.img_bounds
        rc = ref_cam(cm)
        # the branch logic exactly, on the GPU's own undistorted corners; the whole restatement within 1 float ulp
        exact = R.image_bounds(rc, ref_undistort or gpu_undistort(cm))
        assert b.dtype == np.float32 and np.array_equal(b, exact), (node["Camera.model"], b, exact)
        full = R.image_bounds(rc, ref_undistort)
        assert within_ulp(b, full).all(), (b, full)
        g = cm.grid()
        assert (g.min_x, g.min_y, g.cols, g.rows) == (float(b[0]), float(b[2]), 64, 48)
        assert (g.inv_cell_width, g.inv_cell_height) == R.grid_cells(b)
    # both fisheye branches were taken: the top-left corner's incidence beyond pi / 2 (edge midpoints) and within it (corners)
    corner = lambda n: np.hypot(n["Camera.cx"] / n["Camera.fx"], n["Camera.cy"] / n["Camera.fy"])   # noqa: E731
    assert corner(TUM_VI_MONO) > np.pi / 2 and corner(WIDE_FISHEYE) > np.pi / 2 and corner(NARROW_FISHEYE) < np.pi / 2
    nb = plp.camera_model(NARROW_FISHEYE).img_bounds
    assert nb[0] < 0 < 512 < nb[1] and nb[2] < 0 < 512 < nb[3]


def test_validation():
    L = plp.lib()
    mt = plp.matcher()
    k = lattice(64, 48, 3)
    und = np.zeros(len(k), plp.KP_DTYPE); bear = np.zeros((len(k), 3)); xr = np.zeros(len(k), np.float32); dp = np.zeros(len(k), np.float32)
    depth = np.ones((48, 64), np.float32)
    P = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731

    def host(cm, kps=k, n=None, d=None, kl=None, n_kl=0):
        n = len(kps) if n is None else n
        kd = np.zeros((max(n_kl, 1), 2), np.float32)
        return L.plp_post_extract_model_host(mt._h, C.byref(cm), P(kps) if n else None, n, P(d) if d is not None else None, 48, 64, 64 * 4,
                                             P(und), P(bear), P(xr) if d is not None else None, P(dp) if d is not None else None,
                                             P(kl) if kl is not None else None, n_kl, P(kd) if n_kl else None, P(kd) if n_kl else None)

    def dev(cm, B=1):
        return L.plp_post_extract_model_device(mt._h, C.byref(cm), None, None, 0, B, None, 0, 0, 0, 0, None, None, None, None, None, None, 0,
                                               None, None, None)

    eq = cam_model_c((0,) * 10, plp.CAMERA_EQUIRECTANGULAR, 64, 48)
    for model in (3, -1):
        bad = cam_model_c(CAMS["fr1"], model)
        assert host(bad) == plp.PLP_ERR_INVALID_ARG and dev(bad) == plp.PLP_ERR_INVALID_ARG
    assert host(eq, d=depth) == plp.PLP_ERR_UNSUPPORTED
    kl = np.zeros(2, plp.KL_DTYPE)
    assert host(eq, d=None, kl=kl, n_kl=2) == plp.PLP_ERR_UNSUPPORTED
    assert L.plp_post_extract_model_device(mt._h, C.byref(eq), P(k), None, len(k), 1, P(depth), 48, 64, 256, 0, P(und), None, None, None,
                                           None, None, 0, None, None, None) == plp.PLP_ERR_UNSUPPORTED   # refused before any pointer is used
    for cols, rows in ((0, 48), (64, 0), (-5, 48)):
        assert host(cam_model_c((0,) * 10, plp.CAMERA_EQUIRECTANGULAR, cols, rows)) == plp.PLP_ERR_INVALID_ARG
    for model in (plp.CAMERA_PERSPECTIVE, plp.CAMERA_FISHEYE):
        v = list(CAMS["fr1"]); v[1] = 0.0
        assert host(cam_model_c(v, model)) == plp.PLP_ERR_INVALID_ARG and dev(cam_model_c(v, model)) == plp.PLP_ERR_INVALID_ARG
    fish = plp.camera_model(TUM_VI_MONO)
    assert host(fish, d=depth) == plp.PLP_OK               # depth with a fisheye camera is fine
    # nothing to do: PLP_OK, nothing written
    und[:] = np.frombuffer(b"\xcd" * und.nbytes, plp.KP_DTYPE); bear[:] = 3.0
    before = und.tobytes()
    for cm in (eq, fish, cam_model_c(CAMS["fr1"])):
        assert host(cm, n=0) == plp.PLP_OK and dev(cm) == plp.PLP_OK
        assert und.tobytes() == before and (bear == 3.0).all()
        assert len(mt.post_extract(cm, np.zeros(0, plp.KP_DTYPE))["undist_keypts"]) == 0
    with pytest.raises(plp.PlpError) as e:
        mt.post_extract(eq, k, depth)
    assert e.value.status == plp.PLP_ERR_UNSUPPORTED
