"""CPU side of ndtpso_map_align_batch (several ndtpso_map_align calls in one launch) and of its C++ face NDTFrame::alignBatch:
the export and its binding, the job struct's layout, argument checks that need no device, and -- through replay/node_fleet -- the
drop-in's failure semantics when there is no device at all (a failed alignment returns its guess, the update that follows is
refused, the process lives)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "host")


def test_export_and_binding():
    from ndtpso_slam_amd import capi
    L = capi.load()
    for name in ("ndtpso_map_align_batch", "ndtpso_exact_check_jobs"):
        assert name in capi.EXPORTS and hasattr(L, name), name
    assert callable(capi.align_maps) and callable(capi.Context.exact_check_jobs)


def test_job_struct_layout_matches_the_header():
    from ndtpso_slam_amd import capi
    src = open(os.path.join(ROOT, "include", "ndtpso_hip.h")).read()
    m = re.search(r"#define NDTPSO_MAP_ALIGN_JOB_BYTES (\d+)", src)
    assert m and "static_assert(sizeof(ndtpso_map_align_job) == NDTPSO_MAP_ALIGN_JOB_BYTES" in src
    assert C.sizeof(capi.MapAlignJob) == int(m.group(1))
    # out fields where the header puts them: pose behind the rand-table pointer, rc / route last
    assert capi.MapAlignJob.pose.offset == 80 and capi.MapAlignJob.stats.offset == 112 and capi.MapAlignJob.route.offset == 148


def test_argument_checks_need_no_device():
    from ndtpso_slam_amd import capi
    L = capi.load()
    cfg = capi.PSOConfig.make(50, 30)
    jobs = (capi.MapAlignJob * 2)()
    assert L.ndtpso_map_align_batch(None, jobs, 2, C.byref(cfg), capi.SCORE_EXACT) == capi.E_ARG
    assert L.ndtpso_map_align_batch(None, jobs, 0, C.byref(cfg), capi.SCORE_EXACT) == capi.E_ARG
    assert L.ndtpso_map_align_batch(None, None, 0, C.byref(cfg), capi.SCORE_F64) == capi.E_ARG
    assert L.ndtpso_exact_check_jobs(None, None) == capi.E_ARG


def _scan_file(path, n_scans):
    from ndtpso_slam_amd import synth
    s = np.linspace(0.0, 0.3, n_scans)
    poses = np.stack([2.0 + 1.2 * s, -1.0 + 0.8 * np.sin(1.5 * s), 0.3 + 0.25 * s], axis=1)
    ranges = synth.raycast(poses).astype(np.float32)
    with open(path, "wb") as f:
        np.array([n_scans, synth.N_BEAMS], dtype=np.int32).tofile(f)
        np.array([synth.ANGLE_MIN, synth.ANGLE_INC, synth.RANGE_MAX], dtype=np.float32).tofile(f)
        ranges.tofile(f)


def test_node_fleet_builds_and_survives_a_missing_device(tmp_path):
    from ndtpso_slam_amd import build as hip_build
    hip_build.build_hip()
    subprocess.check_call(["make", "-C", HOST, "-s"])
    exe = os.path.join(HOST, "replay", "node_fleet")
    assert os.path.exists(exe)
    out = subprocess.check_output(["nm", "-D", "--demangle", os.path.join(HOST, "libndtpso_slam.so")], text=True)
    assert "NDTFrame::alignBatch(" in out
    scans = tmp_path / "scans.bin"
    _scan_file(scans, 4)
    prefix = str(tmp_path / "fleet")
    env = {k: v for k, v in os.environ.items() if k not in ("NDTPSO_ABORT_ON_ERROR", "NODE_FLEET_SEQUENTIAL")}
    r = subprocess.run([exe, str(scans), "60", "0.5", "50", "30", "1", "3", prefix], text=True, capture_output=True,
                       env=dict(env, NDTPSO_DEVICE="99"), timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr[-2000:])          # it did not abort
    for robot in range(3):
        lines = open("%s.%d.poses" % (prefix, robot)).read().strip().splitlines()
        assert len(lines) == 4
        for k, line in enumerate(lines):
            f = line.split()
            assert int(f[0]) == k and [float(v) for v in f[1:]] == [0.0, 0.0, 0.0], line   # the initial guess, every time
    assert "align failed" in r.stderr and "update after a failed align" in r.stderr, r.stderr[-2000:]
    assert '"failed_alignments": 9' in r.stdout, r.stdout                          # 3 robots x 3 aligned scans
