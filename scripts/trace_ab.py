"""ndtpso_map_trace against what a caller did before it existed, the batch against the single calls, the node's sequence with tracing
on and off, and the kernel's origin-cell aggregation against the plain lane-per-ray form -- alternating on one box, so that the
spread of either side is known.

(a) One trace of a 1081-beam scan in a 60 m frame at og_cell_size 0.25 and 0.05: ndtpso_map_trace followed by a wait for the
    stream (what a caller who wants the counters NOW pays; a node that only enqueues pays the host's share alone, recorded too),
    against host/replay/trace_check --host-trace's loop on the same kind of scan: download of the points + the same rule on one CPU
    thread (the tool's own per-scan figure, TRACE_CHECK_TIMING).  A lap is one run of the tool and, straight behind it, the
    device's side in a fresh process.
(b) R = 4 / 16 / 64 ndtpso_map_trace calls, one per robot into its own map, against ONE ndtpso_map_trace_batch call, each followed
    by one wait; the batch's counters are checked against the single calls' before anything is timed.
(c) host/replay/trace_check on a recorded sequence with setTraceOnUpdate on, off (--no-trace) and with --host-trace: ms per scan.
(d) (a)'s device side in child processes with NDTPSO_TRACE_AGGREGATE=1 (one add of a workgroup's rays to the origin's cell) and =0
    (every lane its own add), alternating; the counters of both are compared.

Ratios: of medians, with the 5th-95th percentile of the per-lap ratios.  Host clock around the C entries (ctypes, arguments made
once).  Every child process runs under a time limit; a failure ends the script.

    python scripts/trace_ab.py [--out profiles/trace_ab.json] [--reps 15] [--warm 3]
"""
import argparse
import ctypes as C
import hashlib
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

TRUTH = (1.3, -0.7, 0.45)
OGS = (0.25, 0.05)


def summary(a, b):
    a, b = np.array(a), np.array(b)
    ratio = a / b
    return dict(a_ms=dict(median=float(np.median(a)), p5=float(np.percentile(a, 5)), p95=float(np.percentile(a, 95))),
                b_ms=dict(median=float(np.median(b)), p5=float(np.percentile(b, 5)), p95=float(np.percentile(b, 95))),
                a_over_b=dict(of_medians=float(np.median(a) / np.median(b)), p5=float(np.percentile(ratio, 5)),
                              p95=float(np.percentile(ratio, 95))))


def setup():
    from ndtpso_slam_amd import capi, synth
    geom = capi.ScanGeom(synth.N_BEAMS, synth.ANGLE_MIN, synth.ANGLE_INC, synth.RANGE_MAX, 0.1)
    rng = np.random.default_rng(4)

    def scan_at(pose):
        clean = synth.raycast(np.asarray(pose, dtype=np.float64)[None, :])[0]
        return np.where(clean > 0, clean + rng.normal(0, 0.01, synth.N_BEAMS), 0.0).astype(np.float32)
    return capi, synth, geom, scan_at


def one_trace(reps, warm):
    """the child of (d), and (a)'s device side: per og_cell_size the times of trace + wait, of the trace call alone, and a digest"""
    capi, synth, geom, scan_at = setup()
    ctx = capi.Context(0)
    L = ctx._lib
    pose = np.ascontiguousarray(TRUTH, dtype=np.float64)
    dp = pose.ctypes.data_as(C.POINTER(C.c_double))
    out = {}
    for og in OGS:
        grid = capi.Grid(60, 60, 0.5)
        m = capi.ResidentMap(ctx, grid, og_cell_size=og, pool_bytes=16 << 20)
        s = capi.ResidentScan(ctx, synth.N_BEAMS)
        s.load_scan(scan_at(TRUTH), geom, clip=grid)
        both, call = [], []
        for rep in range(warm + reps):
            L.ndtpso_synchronize(ctx._h)
            t0 = time.perf_counter()
            rc = L.ndtpso_map_trace(m._h, s._h, dp)
            t1 = time.perf_counter()
            L.ndtpso_synchronize(ctx._h)
            t2 = time.perf_counter()
            if rc != capi.OK:
                raise SystemExit("ndtpso_map_trace: %d" % rc)
            if rep >= warm:
                both.append(1e3 * (t2 - t0))
                call.append(1e3 * (t1 - t0))
        m.clear()
        m.trace(s, TRUTH)
        hits, passes = m.trace_counts()
        info = m.trace_info()
        out[str(og)] = dict(trace_and_wait_ms=both, call_ms=call, n_rays=info["n_rays"], n_steps=info["n_steps"],
                            digest=hashlib.sha256(hits.tobytes() + passes.tobytes()).hexdigest())
    ctx.close()
    return out


def child(env_value, reps, warm):
    env = dict(os.environ, NDTPSO_TRACE_AGGREGATE=env_value)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one-trace", "--reps", str(reps), "--warm", str(warm)], env=env, text=True,
                       capture_output=True, check=True, timeout=300)
    return json.loads(r.stdout.splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "trace_ab.json"))
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--one-trace", action="store_true")
    args = ap.parse_args()
    if args.one_trace:
        print(json.dumps(one_trace(args.reps, args.warm)))
        return
    capi, synth, geom, scan_at = setup()

    # ---- the recorded sequence of (a)'s host side and of (c) -----------------------------------------------------------------------
    n_scans = 200
    t = np.linspace(0.0, 0.9, n_scans)
    path_poses = np.stack([2.0 + 1.2 * t, -1.0 + 0.8 * np.sin(1.5 * t), 0.3 + 0.25 * t], axis=1)
    clean = synth.raycast(path_poses)
    ranges = np.where(clean > 0, clean + np.random.default_rng(5).normal(0, 0.01, clean.shape), 0.0).astype(np.float32)
    exe = os.path.join(ROOT, "host", "replay", "trace_check")
    part_a, part_c = [], []
    with tempfile.TemporaryDirectory() as tmp:
        scans = os.path.join(tmp, "scans.bin")
        with open(scans, "wb") as f:
            np.array([n_scans, synth.N_BEAMS], dtype=np.int32).tofile(f)
            np.array([synth.ANGLE_MIN, synth.ANGLE_INC, synth.RANGE_MAX], dtype=np.float32).tofile(f)
            ranges.tofile(f)
        for og in OGS:
            ms = {"off": [], "on": [], "host": []}
            host_us, dev_ms, call_ms, logs = [], [], [], {}
            for lap in range(5):
                for name, flag in (("off", ["--no-trace"]), ("on", []), ("host", ["--host-trace"])):
                    r = subprocess.run([exe] + flag + [scans, "60", "0.5", str(og), "50", "30", "7", os.path.join(tmp, name)],
                                       env=dict(os.environ, TRACE_CHECK_TIMING="1"), text=True, capture_output=True, check=True, timeout=300)
                    logs[name] = r.stdout
                    ms[name].append(float(re.search(r"\(([0-9.]+) ms per scan\)", r.stderr).group(1)))
                    if name == "host":   # ... and the device's side of the same lap straight behind it, in a process of its own
                        host_us.append(float(re.search(r"host trace ([0-9.]+) us", r.stderr).group(1)))
                        d = child("1", args.reps, args.warm)[str(og)]
                        dev_ms.append(float(np.median(d["trace_and_wait_ms"])))
                        call_ms.append(float(np.median(d["call_ms"])))
            same_files = all(open(os.path.join(tmp, "on.0." + e), "rb").read() == open(os.path.join(tmp, "host.0." + e), "rb").read()
                             for e in ("hits", "passes", "nav"))
            host_ms = [u / 1e3 for u in host_us]
            row = dict(og_cell_size=og, n_rays=d["n_rays"], steps_per_ray=d["n_steps"] / max(d["n_rays"], 1), laps=len(host_ms),
                       a="trace_check --host-trace: download + one CPU thread, per scan (a lap: one run of %d scans)" % n_scans,
                       b="ndtpso_map_trace + wait for the stream (a lap: the median of %d calls in a fresh process)" % args.reps,
                       enqueue_alone_ms_median=float(np.median(call_ms)), **summary(host_ms, dev_ms))
            part_a.append(row)
            print(json.dumps(row), flush=True)
            row = dict(og_cell_size=og, scans=n_scans, laps=5, same_poses=logs["on"] == logs["off"] == logs["host"], same_files=same_files,
                       a="trace_check, setTraceOnUpdate on, ms per scan", b="trace_check --no-trace, ms per scan",
                       added_us_per_scan_of_medians=1e3 * float(np.median(ms["on"]) - np.median(ms["off"])),
                       host_trace_added_us_per_scan_of_medians=1e3 * float(np.median(ms["host"]) - np.median(ms["off"])),
                       scans_per_s=dict(on=1e3 / float(np.median(ms["on"])), off=1e3 / float(np.median(ms["off"])),
                                        host=1e3 / float(np.median(ms["host"]))),
                       **summary(ms["on"], ms["off"]))
            part_c.append(row)
            print(json.dumps(row), flush=True)

    # ---- (b) R single calls against one batch call ------------------------------------------------------------------------------
    ctx = capi.Context(0)
    L = ctx._lib
    grid = capi.Grid(60, 60, 1.0)   # (the map's own cells play no part in a trace: coarse ones keep 128 maps small)
    robots = []
    for r in range(64):
        tr = (-4.0 + 8.0 * (r % 8) / 7.0, -2.0 + 3.0 * (r // 8) / 7.0, -0.4 + 0.1 * (r % 9))
        m, m2 = (capi.ResidentMap(ctx, grid, og_cell_size=0.25, pool_bytes=1 << 20) for _ in range(2))
        s = capi.ResidentScan(ctx, synth.N_BEAMS)
        s.load_scan(scan_at(tr), geom, clip=grid)
        robots.append((m, m2, s, tr))
    part_b = []
    for n_robots in (4, 16, 64):
        arr = (capi.MapTraceJob * n_robots)()
        poses = [np.ascontiguousarray(tr, dtype=np.float64) for _, _, _, tr in robots[:n_robots]]
        for j, (m, m2, s, tr) in zip(arr, robots):
            j.map, j.points = m2._h, s._h
            j.pose[:] = list(tr)

        def singles():
            for (m, m2, s, tr), p in zip(robots[:n_robots], poses):
                rc = L.ndtpso_map_trace(m._h, s._h, p.ctypes.data_as(C.POINTER(C.c_double)))
                if rc != capi.OK:
                    raise SystemExit("ndtpso_map_trace: %d" % rc)
            L.ndtpso_synchronize(ctx._h)

        def one_batch():
            rc = L.ndtpso_map_trace_batch(ctx._h, arr, n_robots)
            if rc != capi.OK:
                raise SystemExit("ndtpso_map_trace_batch: %d" % rc)
            L.ndtpso_synchronize(ctx._h)

        for m, m2, s, tr in robots[:n_robots]:
            m.clear()
            m2.clear()
        singles()
        one_batch()
        for m, m2, s, tr in robots[:n_robots]:
            a, b = m.trace_counts(), m2.trace_counts()
            if not (np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])):
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
        row = dict(robots=n_robots, equal=True, a="R ndtpso_map_trace calls + one wait", b="one ndtpso_map_trace_batch call + one wait",
                   **summary(t_s, t_b))
        part_b.append(row)
        print(json.dumps(row), flush=True)
    del robots
    ctx.close()

    # ---- (d) the origin's cell: one add per workgroup against one per lane ------------------------------------------------------------
    laps = {"1": [], "0": []}
    for lap in range(4):
        for v in ("1", "0"):
            laps[v].append(child(v, args.reps, args.warm))
    part_d = []
    for og in OGS:
        plain = [x for lap in laps["0"] for x in lap[str(og)]["trace_and_wait_ms"]]
        agg = [x for lap in laps["1"] for x in lap[str(og)]["trace_and_wait_ms"]]
        same = len({lap[str(og)]["digest"] for v in laps for lap in laps[v]}) == 1
        row = dict(og_cell_size=og, same_counters=same, a="every lane adds its own pass to the origin's cell (NDTPSO_TRACE_AGGREGATE=0), trace + wait",
                   b="one add per workgroup (the default), trace + wait", **summary(plain, agg))
        part_d.append(row)
        print(json.dumps(row), flush=True)

    out = dict(what="ndtpso_map_trace measured four ways, alternating on one box, %d repetitions after %d warm-up laps per point; "
                    "a_over_b > 1: b is faster" % (args.reps, args.warm),
               one_trace_against_the_host_walk=part_a, single_calls_against_batch=part_b, live_sequence=part_c,
               origin_cell_aggregation=part_d)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
