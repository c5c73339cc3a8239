"""R robots in one process, two ways, alternated in ONE run on one device: `node_replicas R` (R host threads, a device context,
a stream and a launch per robot and scan) against `node_fleet R` (one host thread, the R alignments of a step in one launch:
NDTFrame::alignBatch -> ndtpso_map_align_batch).  Per R and program: aggregate scans per second and the p95 time per scan (replicas)
or per step (fleet), three repetitions each, with the spread between repetitions.  R = 1 also runs node_replay, which a fleet of
one must match (it takes the single-alignment path by construction).

    python scripts/fleet_ab.py [--out profiles/fleet_ab.json] [--scans 1010] [--robots 1,4,16,32,64] [--reps 3]

node_replicas asks the runtime for one hardware queue per replica, 4 at least and 16 at most (GPU_MAX_HW_QUEUES, unless the
environment already sets it); its children get exactly that here, whatever the environment of this script says, so that the
threads are measured at their own operating point.  node_fleet has one stream and runs with the environment as it is.
--replica-queues N overrides (0: leave the environment alone).

Every child process runs under its own time limit; the script stops at the first one that fails.
"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HOST = os.path.join(ROOT, "host", "replay")


def write_scans(path, n_scans):
    from ndtpso_slam_amd import synth
    rng = np.random.default_rng(4)
    s = np.linspace(0.0, 0.025 * n_scans, n_scans)            # the trajectory of the tests, 40 scans per unit of its parameter
    poses = np.stack([2.0 * np.cos(0.35 * s) + 1.0, 3.0 * np.sin(0.35 * s), 0.3 + 0.2 * s], axis=1)
    with open(path, "wb") as f:
        np.array([n_scans, synth.N_BEAMS], dtype=np.int32).tofile(f)
        np.array([synth.ANGLE_MIN, synth.ANGLE_INC, synth.RANGE_MAX], dtype=np.float32).tofile(f)
        for k in range(0, n_scans, 128):
            clean = synth.raycast(poses[k:k + 128])
            np.where(clean > 0, clean + rng.normal(0, 0.01, clean.shape), 0.0).astype(np.float32).tofile(f)


def run(cmd, env, limit):
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=limit)
    if r.returncode != 0:
        raise SystemExit("%s: exit %d\n%s" % (" ".join(cmd), r.returncode, r.stderr[-2000:]))
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fleet_ab.json"))
    ap.add_argument("--scans", type=int, default=1010)        # 10 warm-up scans, 1000 timed per robot
    ap.add_argument("--robots", default="1,4,16,32,64")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--limit", type=float, default=120.)      # seconds per child process
    ap.add_argument("--replica-queues", type=int, default=-1)  # -1: min(max(R, 4), 16), what node_replicas asks for
    args = ap.parse_args()
    env = {k: v for k, v in os.environ.items() if k not in ("NODE_FLEET_SEQUENTIAL", "NDTPSO_ABORT_ON_ERROR")}
    rows = []
    with tempfile.TemporaryDirectory() as tmp:
        scans = os.path.join(tmp, "scans.bin")
        write_scans(scans, args.scans)
        tail = [scans, "60", "0.5", "50", "30", "7"]
        for R in [int(v) for v in args.robots.split(",")]:
            for rep in range(args.reps):
                for prog in ("node_replicas", "node_fleet") + (("node_replay",) if R == 1 else ()):
                    if prog == "node_replay":
                        r = run([os.path.join(HOST, prog)] + tail, env, args.limit)
                        m = re.search(r"matching rate: ([0-9.]+) Hz \(([0-9.]+) ms per scan\)", r.stderr)
                        row = dict(program=prog, robots=1, rep=rep, aggregate_scans_per_s=float(m.group(1)), ms_mean=float(m.group(2)))
                    else:
                        child_env, queues = env, env.get("GPU_MAX_HW_QUEUES")
                        if prog == "node_replicas" and args.replica_queues != 0:
                            queues = str(args.replica_queues if args.replica_queues > 0 else min(max(R, 4), 16))
                            child_env = dict(env, GPU_MAX_HW_QUEUES=queues)
                        d = json.loads(run([os.path.join(HOST, prog)] + tail + [str(R)], child_env, args.limit).stdout.strip().splitlines()[-1])
                        if d["failed_alignments"] or d["device_errors"]:
                            raise SystemExit("%s %d: %r" % (prog, R, d))
                        per = "scan" if prog == "node_replicas" else "step"
                        row = dict(program=prog, robots=R, rep=rep, aggregate_scans_per_s=d["aggregate_scans_per_s"],
                                   ms_mean=d["ms_per_%s_mean" % per], ms_p95=d["ms_per_%s_p95" % per], ms_max=d["ms_per_%s_max" % per],
                                   cluster_timeouts=d["cluster_timeouts"], hw_queues=queues)
                    rows.append(row)
                    print(json.dumps(row), flush=True)
    summary = []
    for R in sorted({r["robots"] for r in rows}):
        s = dict(robots=R)
        for prog in ("node_replicas", "node_fleet", "node_replay"):
            v = [r["aggregate_scans_per_s"] for r in rows if r["robots"] == R and r["program"] == prog]
            if v:
                s[prog] = dict(scans_per_s_median=float(np.median(v)), scans_per_s_min=min(v), scans_per_s_max=max(v),
                               spread=(max(v) - min(v)) / float(np.median(v)),
                               ms_p95_median=float(np.median([r.get("ms_p95", 0.) for r in rows if r["robots"] == R and r["program"] == prog])))
        s["fleet_over_replicas"] = s["node_fleet"]["scans_per_s_median"] / s["node_replicas"]["scans_per_s_median"]
        summary.append(s)
    out = dict(what="node_replicas R (R host threads; per scan: ms per scan of one replica) against node_fleet R (one host thread, one "
                    "launch per step; per step: ms for the R scans of a step), alternated in one run on one MI355X, %d timed scans per "
                    "robot, 30 x 50 PSO, 60 m frame of 0.5 m cells, default (exact) score mode; hw_queues: GPU_MAX_HW_QUEUES of the child "
                    "(node_replicas: one per replica, 4 .. 16, as it asks for itself; null: the runtime's default)" % (args.scans - 10),
               summary=summary, runs=rows)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(summary))


if __name__ == "__main__":
    main()
