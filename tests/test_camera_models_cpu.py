"""Camera models of the post-extract step without a GPU: invariants of the CPU restatement (tests/camera_models_ref.py), the Python
mirror's parsing of the reference's Camera.* keys (camera_model) and the C ABI table."""
import ctypes
import math

import numpy as np
import pytest

import camera_models_ref as R
from plp import plp

# example/tum_vi/TUM_VI_mono.yaml of the reference (values quoted as data)
TUM_VI_MONO = {
    "Camera.name": "TUM VI monocular", "Camera.setup": "monocular", "Camera.model": "fisheye",
    "Camera.fx": 190.97847715128717, "Camera.fy": 190.9733070521226, "Camera.cx": 254.93170605935475, "Camera.cy": 256.8974428996504,
    "Camera.k1": 0.0034823894022493434, "Camera.k2": 0.0007150348452162257, "Camera.k3": -0.0020532361418706202, "Camera.k4": 0.00020293673591811182,
    "Camera.fps": 20, "Camera.cols": 512, "Camera.rows": 512, "Camera.color_order": "Gray",
}
EQUIRECT = {"Camera.name": "360 video", "Camera.setup": "monocular", "Camera.model": "equirectangular", "Camera.fps": 30.0,
            "Camera.cols": 1920, "Camera.rows": 960, "Camera.color_order": "RGB"}


def ref_cam(node):
    c = {"model": node["Camera.model"], "cols": node["Camera.cols"], "rows": node["Camera.rows"]}
    for k in ("fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2", "k3", "k4"):
        c[k] = float(node.get(f"Camera.{k}", 0.0))
    return c


def test_fisheye_without_distortion_is_the_equidistant_model():
    # k = 0 is not the identity for a fisheye camera: the distorted radius is f theta, the undistorted one f tan(theta)
    cam = dict(ref_cam(TUM_VI_MONO), k1=0.0, k2=0.0, k3=0.0, k4=0.0)
    rng = np.random.default_rng(3)
    ang, rad = rng.uniform(0, 2 * math.pi, 2000), rng.uniform(0, 1.5 * 190, 2000)     # incidence below 1.5 rad (the clamp is at pi / 2)
    x = (cam["cx"] + rad * np.cos(ang)).astype(np.float32); y = (cam["cy"] + rad * np.sin(ang)).astype(np.float32)
    ux, uy = R.fisheye_undistort(cam, x, y)
    fx, fy, cx, cy = (float(np.float32(cam[k])) for k in ("fx", "fy", "cx", "cy"))
    for i in range(len(x)):
        px, py = (float(x[i]) - cx) / fx, (float(y[i]) - cy) / fy
        th = math.hypot(px, py)
        s = math.tan(th) / th
        assert abs(float(ux[i]) - (cx + fx * px * s)) <= np.spacing(abs(ux[i])) and abs(float(uy[i]) - (cy + fy * py * s)) <= np.spacing(abs(uy[i]))
    # the principal point and points near it map to themselves up to float rounding
    ux, uy = R.fisheye_undistort(cam, np.float32([cam["cx"], cam["cx"] + 0.001]), np.float32([cam["cy"], cam["cy"] - 0.001]))
    assert ux[0] == np.float32(cam["cx"]) and uy[0] == np.float32(cam["cy"])
    assert abs(ux[1] - np.float32(cam["cx"] + 0.001)) <= np.spacing(ux[1]) and abs(uy[1] - np.float32(cam["cy"] - 0.001)) <= np.spacing(uy[1])


def test_fisheye_undistortion_inverts_the_forward_model():
    cam = ref_cam(TUM_VI_MONO)
    fx, fy, cx, cy = (float(np.float32(cam[k])) for k in ("fx", "fy", "cx", "cy"))
    k = [float(np.float32(cam[n])) for n in ("k1", "k2", "k3", "k4")]
    rng = np.random.default_rng(4)
    xu = rng.uniform(-200, 700, 1000); yu = rng.uniform(-200, 700, 1000)
    a, b = (xu - cx) / fx, (yu - cy) / fy
    r = np.hypot(a, b); th = np.arctan(r)
    thd = th * (1 + k[0] * th ** 2 + k[1] * th ** 4 + k[2] * th ** 6 + k[3] * th ** 8)
    xd = (cx + fx * a * thd / r).astype(np.float32); yd = (cy + fy * b * thd / r).astype(np.float32)
    ux, uy = R.fisheye_undistort(cam, xd, yd)
    assert np.abs(ux - xu).max() < 0.05 and np.abs(uy - yu).max() < 0.05      # float inputs magnified by the tangent towards the rim


def test_fisheye_sentinel_for_points_that_do_not_converge():
    cam = dict(ref_cam(TUM_VI_MONO), fx=150.0, fy=150.0, cx=256.0, cy=256.0, k1=-0.5, k2=0.1, k3=0.0, k4=0.0)
    xs = np.linspace(0, 511, 32, dtype=np.float32)
    X, Y = np.meshgrid(xs, xs)
    ux, uy = R.fisheye_undistort(cam, X.ravel(), Y.ravel())
    bad = ux == R.SENTINEL
    assert 0 < bad.sum() < bad.size and np.array_equal(bad, uy == R.SENTINEL)


def test_equirectangular_bearings():
    cam = ref_cam(EQUIRECT)
    b = R.equirect_bearings(cam, [960.0], [480.0])[0]
    assert b.tolist() == [0.0, 0.0, 1.0]                               # image centre: straight ahead
    b = R.equirect_bearings(cam, [0.0, 480.0, 960.0], [480.0, 480.0, 0.0])
    assert np.abs(b[0] - [0.0, 0.0, -1.0]).max() < 1e-15               # left border: behind
    assert np.abs(b[1] - [-1.0, 0.0, 0.0]).max() < 1e-15               # a quarter: to the left
    assert np.abs(b[2] - [0.0, -1.0, 0.0]).max() < 1e-15               # top row: up (y points down)
    rng = np.random.default_rng(5)
    b = R.equirect_bearings(cam, rng.uniform(0, 1920, 5000), rng.uniform(0, 960, 5000))
    assert np.abs(np.linalg.norm(b, axis=1) - 1).max() < 1e-15


def test_pinhole_bearings_have_unit_norm():
    cam = ref_cam(TUM_VI_MONO)
    rng = np.random.default_rng(6)
    b = R.pinhole_bearings(cam, rng.uniform(-500, 1000, 5000), rng.uniform(-500, 1000, 5000))
    assert np.abs(np.linalg.norm(b, axis=1) - 1).max() < 1e-15 and (b[:, 2] > 0).all()


def test_camera_model_parses_tum_vi_mono():
    cam = plp.camera_model(TUM_VI_MONO)
    assert (cam.model, cam.cols, cam.rows) == (plp.CAMERA_FISHEYE, 512, 512)
    for k in ("fx", "fy", "cx", "cy", "k1", "k2", "k3", "k4"):
        assert getattr(cam, k) == TUM_VI_MONO[f"Camera.{k}"], k
    assert cam.p1 == 0 and cam.p2 == 0 and cam.focal_x_baseline == 0.0
    # no distortion: the bounds are the image, without a GPU (fisheye.cc:102-107)
    flat = plp.camera_model({**TUM_VI_MONO, "Camera.k1": 0.0, "Camera.k2": 0.0, "Camera.k3": 0.0, "Camera.k4": 0.0})
    assert flat.img_bounds.dtype == np.float32 and flat.img_bounds.tolist() == [0.0, 512.0, 0.0, 512.0]


def test_camera_model_equirectangular_bounds_and_grid():
    cam = plp.camera_model(EQUIRECT)
    assert (cam.model, cam.cols, cam.rows, cam.fx, cam.fy) == (plp.CAMERA_EQUIRECTANGULAR, 1920, 960, 0.0, 0.0)
    assert cam.img_bounds.tolist() == [0.0, 1920.0, 0.0, 960.0] == R.image_bounds(ref_cam(EQUIRECT)).tolist()
    g = cam.grid()
    assert (g.min_x, g.min_y, g.cols, g.rows) == (0.0, 0.0, 64, 48)
    assert (g.inv_cell_width, g.inv_cell_height) == R.grid_cells(cam.img_bounds) == (64 / 1920, 48 / 960)


def test_camera_model_perspective_and_unknown_model():
    node = {"Camera.model": "perspective", "Camera.cols": 640, "Camera.rows": 480, "Camera.fx": 535.4, "Camera.fy": 539.2, "Camera.cx": 320.1,
            "Camera.cy": 247.6, "Camera.k1": 0.0, "Camera.k2": 0.0, "Camera.p1": 0.0, "Camera.p2": 0.0, "Camera.k3": 0.0, "Camera.focal_x_baseline": 40.0}
    cam = plp.camera_model(node)
    assert cam.model == plp.CAMERA_PERSPECTIVE and cam.focal_x_baseline == 40.0 and cam.k4 == 0.0
    assert cam.img_bounds.tolist() == [0.0, 640.0, 0.0, 480.0]
    g, want = cam.grid(), plp.make_grid(640, 480)
    assert (g.inv_cell_width, g.inv_cell_height) == (want.inv_cell_width, want.inv_cell_height)
    with pytest.raises(plp.PlpError):
        plp.camera_model({**node, "Camera.model": "pinhole"})


def test_ctypes_table_lists_the_model_entries():
    names = plp.api_symbols()
    assert "plp_post_extract_model_device" in names and "plp_post_extract_model_host" in names
    header = (plp.ROOT / "include" / "plp_front.h").read_text()
    assert "plp_post_extract_model_device(" in header and "plp_post_extract_model_host(" in header
    assert plp.camera_model_c.fx.offset == 16 and ctypes.sizeof(plp.camera_model_c) == 12 + 4 + 11 * 8     # int32 x 3, padding, 11 doubles
