"""ndtpso_map_curvature against what a caller did before it existed, and the batch against the single calls, in one process on one
box, alternating, so that the spread of either is known.

(a) One call for P poses against central differences through ResidentMap.cost: 19 poses per curvature (the pose, +-h per axis,
    and the four corners of each of the three axis pairs), step 1e-4 m / 1e-4 rad, in ONE ndtpso_map_cost call of 19 P poses
    (the best a caller could do).  Benchmark-shaped map: 1081 beams, 60 m frame, 0.5 m cells; P = 1, 64, 4096.  How far the
    finite differences are from the analytic values is recorded too (relative to the largest entry of each quantity).
(b) R = 4 / 16 / 64 ndtpso_map_curvature calls of one pose, one per robot against its own map, against ONE
    ndtpso_map_curvature_batch call; the batch's bytes are checked against the single calls' before anything is timed.
(c) host/replay/node_replay on a recorded sequence with and without a curvature() after every align() (NODE_REPLAY_CURVATURE,
    NODE_REPLAY_TIMING): the time per scan either way and the tool's own figure for the curvature call.

Ratios: of medians, with the 5th-95th percentile of the per-lap ratios.  Host clock around the C entries (ctypes, arguments made
once).

    python scripts/curvature_ab.py [--out profiles/curvature_ab.json] [--reps 15] [--warm 3]
"""
import argparse
import ctypes as C
import json
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MAP_POSES = [(-6.0, -2.0, 0.3), (-3.0, -1.0, 0.2), (0.0, 0.0, 0.0), (3.0, 1.0, -0.2), (6.0, 2.0, -0.4), (2.0, -3.0, 1.5)]
H = (1e-4, 1e-4, 1e-4)
PAIRS = ((0, 1), (0, 2), (1, 2))


def stencil(pose):
    """the 19 poses of a central-difference gradient and Hessian"""
    pose = np.asarray(pose, dtype=np.float64)
    out = [pose]
    for a in range(3):
        for sgn in (1.0, -1.0):
            p = pose.copy()
            p[a] += sgn * H[a]
            out.append(p)
    for a, b in PAIRS:
        for sa in (1.0, -1.0):
            for sb in (1.0, -1.0):
                p = pose.copy()
                p[a] += sa * H[a]
                p[b] += sb * H[b]
                out.append(p)
    return np.array(out)


def from_stencil(c):
    """gradient (3) and Hessian (xx, xy, xth, yy, yth, thth) from the 19 costs"""
    g = np.array([(c[1 + 2 * a] - c[2 + 2 * a]) / (2 * H[a]) for a in range(3)])
    diag = [(c[1 + 2 * a] - 2 * c[0] + c[2 + 2 * a]) / (H[a] * H[a]) for a in range(3)]
    off = {}
    for i, (a, b) in enumerate(PAIRS):
        pp, pm, mp, mm = c[7 + 4 * i:11 + 4 * i]
        off[(a, b)] = (pp - pm - mp + mm) / (4 * H[a] * H[b])
    return g, np.array([diag[0], off[(0, 1)], off[(0, 2)], diag[1], off[(1, 2)], diag[2]])


def summary(a, b):
    a, b = np.array(a), np.array(b)
    ratio = a / b
    return dict(a_ms=dict(median=float(np.median(a)), p5=float(np.percentile(a, 5)), p95=float(np.percentile(a, 95))),
                b_ms=dict(median=float(np.median(b)), p5=float(np.percentile(b, 5)), p95=float(np.percentile(b, 95))),
                a_over_b=dict(of_medians=float(np.median(a) / np.median(b)), p5=float(np.percentile(ratio, 5)),
                              p95=float(np.percentile(ratio, 95))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "curvature_ab.json"))
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warm", type=int, default=3)
    args = ap.parse_args()
    from ndtpso_slam_amd import capi, synth
    geom = capi.ScanGeom(synth.N_BEAMS, synth.ANGLE_MIN, synth.ANGLE_INC, synth.RANGE_MAX, 0.1)
    grid = capi.Grid(60, 60, 0.5)
    rng = np.random.default_rng(4)

    def scan_at(pose):
        clean = synth.raycast(np.asarray(pose, dtype=np.float64)[None, :])[0]
        return np.where(clean > 0, clean + rng.normal(0, 0.01, synth.N_BEAMS), 0.0).astype(np.float32)

    map_scans = [scan_at(p) for p in MAP_POSES]
    ctx = capi.Context(0)
    L = ctx._lib

    def robot(truth):
        m, s = capi.ResidentMap(ctx, grid, pool_bytes=16 << 20), capi.ResidentScan(ctx, synth.N_BEAMS)
        for k, pose in enumerate(MAP_POSES):
            s.load_scan(map_scans[k], geom, clip=grid)
            m.insert(s, np.asarray(pose, dtype=np.float64))
        m.build()
        s.load_scan(scan_at(truth), geom, clip=grid)
        return m, s

    dp = C.POINTER(C.c_double)
    # ---- (a) one call against central differences through the cost --------------------------------------------------------------
    truth = np.array([1.3, -0.7, 0.45])
    m, s = robot(truth)
    part_a = []
    for n_poses in (1, 64, 4096):
        poses = np.ascontiguousarray(truth + rng.uniform(-1, 1, (n_poses, 3)) * (0.05, 0.05, 0.005))
        poses[0] = truth
        sten = np.ascontiguousarray(np.concatenate([stencil(p) for p in poses]))
        rec = np.zeros(n_poses, dtype=capi.CURVATURE_DTYPE)
        costs = np.zeros(len(sten))

        def analytic():
            rc = L.ndtpso_map_curvature(m._h, s._h, poses.ctypes.data_as(dp), n_poses, C.cast(rec.ctypes.data, C.POINTER(capi.Curvature)))
            if rc != capi.OK:
                raise SystemExit("ndtpso_map_curvature: %d" % rc)

        def differences():
            rc = L.ndtpso_map_cost(m._h, s._h, sten.ctypes.data_as(dp), len(sten), capi.SCORE_F64, costs.ctypes.data_as(dp))
            if rc != capi.OK:
                raise SystemExit("ndtpso_map_cost: %d" % rc)

        analytic()
        differences()
        if rec["cost"].tobytes() != costs[::19].tobytes():
            raise SystemExit("the curvature's cost is not ndtpso_map_cost's")
        fd = [from_stencil(costs[19 * i:19 * i + 19]) for i in range(n_poses)]
        g_fd, h_fd = np.array([f[0] for f in fd]), np.array([f[1] for f in fd])
        g_err = np.abs(g_fd - rec["gradient"]).max(axis=1) / np.abs(rec["gradient"]).max(axis=1)
        h_err = np.abs(h_fd - rec["hessian"]).max(axis=1) / np.abs(rec["hessian"]).max(axis=1)
        t_fd, t_an = [], []
        for rep in range(args.warm + args.reps):
            t0 = time.perf_counter()
            differences()
            t1 = time.perf_counter()
            analytic()
            t2 = time.perf_counter()
            if rep >= args.warm:
                t_fd.append(1e3 * (t1 - t0))
                t_an.append(1e3 * (t2 - t1))
        row = dict(poses=n_poses, path=int(rec["path"][0]), n_hit_first=int(rec["n_hit"][0]),
                   a="central differences: one ndtpso_map_cost call of 19 poses per curvature", b="ndtpso_map_curvature",
                   finite_difference_error=dict(what="max |fd - analytic| over the entries / max |analytic| entry, per pose",
                                                gradient_median=float(np.median(g_err)), gradient_max=float(g_err.max()),
                                                hessian_median=float(np.median(h_err)), hessian_max=float(h_err.max())),
                   **summary(t_fd, t_an))
        part_a.append(row)
        print(json.dumps(row), flush=True)

    # ---- (b) R single calls against one batch call ------------------------------------------------------------------------------
    robots = []
    for r in range(64):
        tr = (-4.0 + 8.0 * (r % 8) / 7.0, -2.0 + 3.0 * (r // 8) / 7.0, -0.4 + 0.1 * (r % 9))
        robots.append(robot(tr) + (np.ascontiguousarray(tr, dtype=np.float64),))
    part_b = []
    for n_robots in (4, 16, 64):
        arr = (capi.MapCurvatureJob * n_robots)()
        single = np.zeros(n_robots, dtype=capi.CURVATURE_DTYPE)
        batch = np.zeros(n_robots, dtype=capi.CURVATURE_DTYPE)
        for k, (j, (rm, rs, tr)) in enumerate(zip(arr, robots)):
            j.map, j.new_points, j.n_poses = rm._h, rs._h, 1
            j.poses = tr.ctypes.data_as(dp)
            j.out = C.cast(batch.ctypes.data + 96 * k, C.POINTER(capi.Curvature))
        bs = capi.CurvatureBatchStats()

        def singles():
            for k, j in enumerate(arr):
                rc = L.ndtpso_map_curvature(j.map, j.new_points, j.poses, 1, C.cast(single.ctypes.data + 96 * k, C.POINTER(capi.Curvature)))
                if rc != capi.OK:
                    raise SystemExit("ndtpso_map_curvature: %d" % rc)

        def one_batch():
            rc = L.ndtpso_map_curvature_batch(ctx._h, arr, n_robots, C.byref(bs))
            if rc != capi.OK:
                raise SystemExit("ndtpso_map_curvature_batch: %d" % rc)

        singles()
        one_batch()
        if single.tobytes() != batch.tobytes():
            raise SystemExit("batch and single calls differ (R = %d)" % n_robots)
        t_s, t_b = [], []
        for rep in range(args.warm + args.reps):
            t0 = time.perf_counter()
            singles()
            t1 = time.perf_counter()
            one_batch()
            t2 = time.perf_counter()
            if rep >= args.warm:
                t_s.append(1e3 * (t1 - t0))
                t_b.append(1e3 * (t2 - t1))
        row = dict(robots=n_robots, equal=True, launches=int(bs.launches), waits=int(bs.waits), a="R ndtpso_map_curvature calls",
                   b="one ndtpso_map_curvature_batch call", **summary(t_s, t_b))
        part_b.append(row)
        print(json.dumps(row), flush=True)
    del robots, m, s
    ctx.close()

    # ---- (c) the node's sequence with and without a curvature() per scan ----------------------------------------------------------
    n_scans = 200
    t = np.linspace(0.0, 0.9, n_scans)
    path_poses = np.stack([2.0 + 1.2 * t, -1.0 + 0.8 * np.sin(1.5 * t), 0.3 + 0.25 * t], axis=1)
    clean = synth.raycast(path_poses)
    ranges = np.where(clean > 0, clean + rng.normal(0, 0.01, clean.shape), 0.0).astype(np.float32)
    part_c = None
    exe = os.path.join(ROOT, "host", "replay", "node_replay")
    if os.access(exe, os.X_OK):
        with tempfile.TemporaryDirectory() as tmp:
            scans = os.path.join(tmp, "scans.bin")
            with open(scans, "wb") as f:
                np.array([n_scans, synth.N_BEAMS], dtype=np.int32).tofile(f)
                np.array([synth.ANGLE_MIN, synth.ANGLE_INC, synth.RANGE_MAX], dtype=np.float32).tofile(f)
                ranges.tofile(f)
            ms = {"without": [], "with": []}
            call_us = []
            logs = {}
            for lap in range(5):
                for name in ("without", "with"):
                    env = dict(os.environ, NODE_REPLAY_TIMING="1", NODE_REPLAY_CURVATURE="1" if name == "with" else "0")
                    r = subprocess.run([exe, scans, "60", "0.5", "50", "30", "7"], env=env, text=True, capture_output=True, check=True)
                    logs[name] = r.stdout
                    ms[name].append(float(re.search(r"\(([0-9.]+) ms per scan\)", r.stderr).group(1)))
                    if name == "with":
                        call_us.append(float(re.search(r"curvature ([0-9.]+)", r.stderr).group(1)))
            part_c = dict(scans=n_scans, laps=5, same_poses=logs["with"] == logs["without"], curvature_call_us_median=float(np.median(call_us)),
                          a="node_replay with curvature() after every align(), ms per scan", b="node_replay, ms per scan",
                          added_us_per_scan_of_medians=1e3 * float(np.median(ms["with"]) - np.median(ms["without"])),
                          **summary(ms["with"], ms["without"]))
            print(json.dumps(part_c), flush=True)
    out = dict(what="ndtpso_map_curvature measured three ways, alternating in one process on one box, %d repetitions after %d warm-up laps "
                    "per point; a_over_b > 1: b is faster" % (args.reps, args.warm),
               one_call_against_central_differences=part_a, single_calls_against_batch=part_b, node_replay=part_c)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
