"""ndtpso_map_curvature / ndtpso_map_curvature_batch / ndtpso_curvature_covariance without a device: the C-ABI's structures
against the header's defines, the symbols and their bindings, the contract's formulas (tests/curvature_ref.py) against
complex-step derivatives, the host-only covariance, and the replay tool in the host library's build."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np

import curvature_ref as cr
import np_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53


def _define(header, name):
    m = re.search(r"#define %s (\d+)\b" % name, header)
    assert m, name
    return int(m.group(1))


def test_struct_sizes_and_offsets_match_the_header():
    from ndtpso_slam_amd import capi
    header = open(os.path.join(ROOT, "include", "ndtpso_hip.h")).read()
    cv, job, bs, pc = capi.Curvature, capi.MapCurvatureJob, capi.CurvatureBatchStats, capi.PoseCovariance
    assert C.sizeof(cv) == _define(header, "NDTPSO_CURVATURE_BYTES") == 96
    assert cv.cost.offset == 0 and cv.gradient.offset == 8 and cv.hessian.offset == 32
    assert cv.n_points.offset == 80 and cv.n_hit.offset == 84 and cv.path.offset == 88
    assert capi.CURVATURE_DTYPE.itemsize == 96
    assert [capi.CURVATURE_DTYPE.fields[f][1] for f in ("cost", "gradient", "hessian", "n_points", "n_hit", "path")] == [0, 8, 32, 80, 84, 88]
    assert C.sizeof(job) == _define(header, "NDTPSO_MAP_CURVATURE_JOB_BYTES") == 48
    assert job.map.offset == 0 and job.new_points.offset == 8
    assert job.poses.offset == _define(header, "NDTPSO_MAP_CURVATURE_JOB_POSES_OFFSET") == 16
    assert job.n_poses.offset == 24
    assert job.rc.offset == _define(header, "NDTPSO_MAP_CURVATURE_JOB_RC_OFFSET") == 28
    assert job.out.offset == _define(header, "NDTPSO_MAP_CURVATURE_JOB_OUT_OFFSET") == 32
    assert job.route.offset == _define(header, "NDTPSO_MAP_CURVATURE_JOB_ROUTE_OFFSET") == 40
    assert C.sizeof(bs) == _define(header, "NDTPSO_CURVATURE_BATCH_STATS_BYTES") == 16
    assert [f for f, _ in bs._fields_] == ["launches", "waits", "single_jobs", "reserved"]
    assert C.sizeof(pc) == _define(header, "NDTPSO_POSE_COVARIANCE_BYTES") == 104
    assert pc.xy_major.offset == 72 and pc.xy_minor.offset == 80 and pc.xy_angle.offset == 88 and pc.definite.offset == 96
    assert capi.CURVATURE_MAX_POSES == _define(header, "NDTPSO_CURVATURE_MAX_POSES") == 65536
    # the header asserts the same sizes to a C and a C++ compiler
    for name in ("ndtpso_curvature", "ndtpso_map_curvature_job", "ndtpso_curvature_batch_stats", "ndtpso_pose_covariance"):
        assert "static_assert(sizeof(%s) == " % name in header
        assert "_Static_assert(sizeof(%s) == " % name in header


def test_symbols_are_exported_and_bound():
    from ndtpso_slam_amd import capi
    L = capi.load()
    for name, n_args in (("ndtpso_map_curvature", 5), ("ndtpso_map_curvature_batch", 4), ("ndtpso_curvature_covariance", 2)):
        assert name in capi.EXPORTS
        assert hasattr(L, name)
        fn = getattr(L, name)
        assert fn.argtypes is not None and len(fn.argtypes) == n_args
        assert fn.restype is C.c_int
    assert callable(capi.curvature_maps) and callable(capi.curvature_covariance) and callable(capi.ResidentMap.curvature)


def test_kernel_is_a_unit_of_its_own():
    units = open(os.path.join(ROOT, "ndtpso_slam_amd", "csrc", "hip_units.txt")).read().split()
    assert "ndtpso_map_curvature.hip" in units
    for f in ("ndtpso_map_curvature.hip", "ndtpso_map_curvature.h", "ndtpso_map_curvature.inc"):
        assert os.path.exists(os.path.join(ROOT, "ndtpso_slam_amd", "csrc", f))


# ---- the formulas, against complex-step derivatives -------------------------------------------------------------------

GRID = (20.0, 20.0, 1.0)


def _case():
    """a map of a few hundred points along the walls of a room (np_ref.build_cells) and a scan of it from elsewhere"""
    rng = np.random.default_rng(5)
    t = rng.uniform(-1, 1, 400)
    wall = rng.integers(0, 4, 400)
    pts = np.where((wall < 2)[:, None], np.stack([t * 7.0, np.where(wall == 0, -5.0, 5.0)], axis=1),
                   np.stack([np.where(wall == 2, -7.0, 7.0), t * 5.0], axis=1))
    pts = pts + rng.normal(0, 0.03, pts.shape)
    cells = cr.cells_of(np_ref.build_cells([tuple(p) for p in pts], *GRID))
    assert len(cells) > 20
    pose = np.array([0.21, -0.13, 0.07])
    # the scan: map points seen from `pose` (the inverse transform), every other one, with noise of its own
    c, s = math.cos(pose[2]), math.sin(pose[2])
    q = pts[::2] - pose[:2]
    scan = np.stack([q[:, 0] * c + q[:, 1] * s, -q[:, 0] * s + q[:, 1] * c], axis=1) + rng.normal(0, 0.02, q.shape)
    return cells, scan


def test_formulas_against_complex_step():
    cells, scan = _case()
    n = scan.shape[0]
    h = 1e-30
    for pose in (np.array([0.21, -0.13, 0.07]), np.array([0.5, 0.1, -0.2]), np.array([-0.3, 0.4, 7.0])):
        want, M, n_hit = cr.curvature(cells, GRID, scan, pose)
        assert n_hit > 20 and want[0] < -0.1      # (a case with something to differentiate)
        tol = cr.tolerance(n, M)
        grads = np.zeros((3, 3))
        for l in range(3):
            p = pose.astype(np.complex128)
            p[l] += 1j * h
            got, _, hit_c = cr.curvature(cells, GRID, scan, p)
            assert hit_c == n_hit                              # membership is the real part's
            # cost -> gradient
            d_cost = got[0].imag / h
            print("pose", pose, "d cost / d", l, d_cost, "analytic", want[1 + l], "tol", tol[1 + l])
            assert abs(d_cost - want[1 + l]) <= tol[1 + l]
            grads[l] = got[1:4].imag / h                       # gradient -> Hessian column l
        idx = {(0, 0): 4, (0, 1): 5, (0, 2): 6, (1, 1): 7, (1, 2): 8, (2, 2): 9}
        for (k, l), i in idx.items():
            for a, b in ((k, l), (l, k)):
                print("pose", pose, "hessian", a, b, grads[b][a], "analytic", want[i], "tol", tol[i])
                assert abs(grads[b][a] - want[i]) <= tol[i]


def test_zero_and_nan_terms_in_the_restatement():
    cells, scan = _case()
    want, M, n_hit = cr.curvature(cells, GRID, scan, np.array([0.21, -0.13, 0.07]))
    far, Mf, hit_f = cr.curvature(cells, GRID, scan, np.array([500.0, 0.0, 0.0]))
    assert hit_f == 0 and not far.any() and not Mf.any()
    # a term of exactly zero contributes exactly zero, whatever its g and h
    t = cr.point_terms(cells, GRID, scan, np.array([0.21, -0.13, 0.07]), math.cos(0.07), math.sin(0.07))
    e = np.exp(t["x"])
    first = int(np.flatnonzero(t["hit"])[0])
    e0 = e.copy()
    e0[first] = 0.0
    t["g"][first] = np.inf
    out, _, _ = cr.sums(t, e0)
    assert np.isfinite(out).all()
    e0[first] = np.nan
    out, _, _ = cr.sums(t, e0)
    assert np.isnan(out).all()


# ---- ndtpso_curvature_covariance: host only ---------------------------------------------------------------------------

def _rotation(rng):
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    return q


def _six(H):
    return [H[0, 0], H[0, 1], H[0, 2], H[1, 1], H[1, 2], H[2, 2]]


def test_covariance_of_a_definite_hessian():
    from ndtpso_slam_amd import capi
    rng = np.random.default_rng(11)
    for kappa in (1.0, 1e2, 1e5, 1e9):
        for _ in range(8):
            R = _rotation(rng)
            d = np.array([1.0, math.sqrt(kappa), kappa]) * rng.uniform(0.5, 2.0)
            H = R @ np.diag(d) @ R.T
            H = (H + H.T) / 2.0
            pc = capi.curvature_covariance({"hessian": _six(H)})
            assert pc["definite"]
            cov = pc["cov"]
            assert (cov == cov.T).all()
            err = np.abs(cov @ H - np.eye(3)).max()
            k_true = np.linalg.cond(H)
            print("kappa", kappa, "max |cov H - I|", err, "bound", 64 * U * k_true)
            assert err <= 64 * U * k_true


def test_covariance_axes_of_the_translational_block():
    from ndtpso_slam_amd import capi
    for angle in (0.0, 0.3, -1.2, 1.5, math.pi / 2):
        for major, minor in ((4.0, 1.0), (100.0, 0.01)):
            c, s = math.cos(angle), math.sin(angle)
            R2 = np.array([[c, -s], [s, c]])
            cov_xy = R2 @ np.diag([major, minor]) @ R2.T
            cov = np.zeros((3, 3))
            cov[:2, :2] = cov_xy
            cov[2, 2] = 0.5
            H = np.linalg.inv(cov)
            H = (H + H.T) / 2.0
            pc = capi.curvature_covariance({"hessian": _six(H)})
            assert pc["definite"]
            assert pc["xy_major"] >= pc["xy_minor"] > 0
            # (the test's own inverse and the library's each err by a few u kappa relative to the largest entry)
            tol = 256 * U * (max(major, 0.5) / min(minor, 0.5)) * major
            assert abs(pc["xy_major"] - major) <= tol and abs(pc["xy_minor"] - minor) <= tol
            assert -math.pi / 2 < pc["xy_angle"] <= math.pi / 2
            diff = (pc["xy_angle"] - angle + math.pi / 2) % math.pi - math.pi / 2       # axes are directions: modulo pi
            assert abs(diff) <= tol / (major - minor), (angle, pc["xy_angle"])


def test_covariance_refuses_what_is_not_definite():
    from ndtpso_slam_amd import capi
    nan = float("nan")
    cases = {"indefinite": [1.0, 0.0, 0.0, -1.0, 0.0, 1.0], "saddle off the diagonal": [1.0, 2.0, 0.0, 1.0, 0.0, 1.0],
             "singular": [1.0, 1.0, 0.0, 1.0, 0.0, 1.0], "zero": [0.0] * 6, "nan": [1.0, 0.0, nan, 1.0, 0.0, 1.0],
             "inf": [float("inf"), 0.0, 0.0, 1.0, 0.0, 1.0], "negative definite": [-1.0, 0.0, 0.0, -1.0, 0.0, -1.0]}
    for name, six in cases.items():
        pc = capi.curvature_covariance({"hessian": six})
        assert not pc["definite"], name
        assert not pc["cov"].any() and pc["xy_major"] == 0 and pc["xy_minor"] == 0 and pc["xy_angle"] == 0, name
    L = capi.load()
    out = capi.PoseCovariance()
    cv = capi.Curvature()
    assert L.ndtpso_curvature_covariance(None, C.byref(out)) == capi.E_ARG
    assert L.ndtpso_curvature_covariance(C.byref(cv), None) == capi.E_ARG


def test_curvature_check_builds():
    from ndtpso_slam_amd import build
    build.build_hip()
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "host"), "libndtpso_slam.so", "replay/curvature_check"],
                          stdout=subprocess.DEVNULL)
    exe = os.path.join(ROOT, "host", "replay", "curvature_check")
    assert os.access(exe, os.X_OK)
    assert subprocess.run([exe], stderr=subprocess.DEVNULL).returncode == 2       # usage: no arguments, nothing touched
    recipes = open(os.path.join(ROOT, "host", "Makefile")).read() + open(os.path.join(ROOT, "host", "CMakeLists.txt")).read()
    assert recipes.count("curvature_check") >= 4                                   # Makefile: all, rule, clean; CMake's tool list
