"""What batching the load and update phases of a fleet step buys, measured in ONE run on one device, the programs alternated:
`node_fleet R` with every phase batched (loadLaserBatch, alignBatch, updateBatch: the default), with the updates as R member calls
(NODE_FLEET_UPDATE=calls), with the loads as R member calls (NODE_FLEET_LOAD=calls), with both as calls (the step as it was when
only the alignments shared a launch), and `node_replicas R` (R host threads with a context and a stream each).  scripts/fleet_ab.py's
conventions: 1000 timed scans per robot, three repetitions, aggregate scans per second with the spread between repetitions, every
child under its own time limit, stop at the first failure.

    python scripts/fleet_update_ab.py [--out profiles/fleet_update_ab.json] [--scans 1010] [--robots 1,4,16,32,64] [--reps 3]
                                      [--queues N]

node_replicas' children get the hardware queues it asks for (one per replica, 4 .. 16), as in fleet_ab.py; --queues N puts
GPU_MAX_HW_QUEUES=N in front of EVERY child instead (N = 4: a process held to the runtime's default).

Accepted when, at every R >= 4, the fully batched fleet is faster than the both-as-calls fleet by more than the larger of the two
spreads, and at R = 1 within it: printed per R as `verdict`.
"""
import argparse
import json
import os
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fleet_ab  # noqa: E402

ROOT, HOST = fleet_ab.ROOT, fleet_ab.HOST
ARMS = [("fleet_batched", "node_fleet", {}),
        ("fleet_update_calls", "node_fleet", {"NODE_FLEET_UPDATE": "calls"}),
        ("fleet_load_calls", "node_fleet", {"NODE_FLEET_LOAD": "calls"}),
        ("fleet_both_calls", "node_fleet", {"NODE_FLEET_LOAD": "calls", "NODE_FLEET_UPDATE": "calls"}),
        ("replicas", "node_replicas", {})]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fleet_update_ab.json"))
    ap.add_argument("--scans", type=int, default=1010)        # 10 warm-up scans, 1000 timed per robot
    ap.add_argument("--robots", default="1,4,16,32,64")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--limit", type=float, default=120.)      # seconds per child process
    ap.add_argument("--queues", type=int, default=0)          # > 0: GPU_MAX_HW_QUEUES of every child
    args = ap.parse_args()
    env = {k: v for k, v in os.environ.items()
           if k not in ("NODE_FLEET_SEQUENTIAL", "NODE_FLEET_LOAD", "NODE_FLEET_UPDATE", "NDTPSO_ABORT_ON_ERROR")}
    if args.queues > 0:
        env["GPU_MAX_HW_QUEUES"] = str(args.queues)
    rows = []
    with tempfile.TemporaryDirectory() as tmp:
        scans = os.path.join(tmp, "scans.bin")
        fleet_ab.write_scans(scans, args.scans)
        tail = [scans, "60", "0.5", "50", "30", "7"]
        for R in [int(v) for v in args.robots.split(",")]:
            for rep in range(args.reps):
                for arm, prog, extra in ARMS:
                    child_env = dict(env, **extra)
                    if prog == "node_replicas" and args.queues <= 0:
                        child_env["GPU_MAX_HW_QUEUES"] = str(min(max(R, 4), 16))
                    d = json.loads(fleet_ab.run([os.path.join(HOST, prog)] + tail + [str(R)], child_env, args.limit).stdout.strip().splitlines()[-1])
                    if d["failed_alignments"] or d["device_errors"]:
                        raise SystemExit("%s %d: %r" % (arm, R, d))
                    per = "scan" if prog == "node_replicas" else "step"
                    row = dict(arm=arm, robots=R, rep=rep, aggregate_scans_per_s=d["aggregate_scans_per_s"], ms_mean=d["ms_per_%s_mean" % per],
                               ms_p95=d["ms_per_%s_p95" % per], cluster_timeouts=d["cluster_timeouts"],
                               hw_queues=child_env.get("GPU_MAX_HW_QUEUES"))
                    for k in ("host_ms_load_mean", "host_ms_align_mean", "host_ms_update_mean"):
                        if k in d:
                            row[k] = d[k]
                    rows.append(row)
                    print(json.dumps(row), flush=True)
    summary = []
    for R in sorted({r["robots"] for r in rows}):
        s = dict(robots=R)
        for arm, _, _ in ARMS:
            mine = [r for r in rows if r["robots"] == R and r["arm"] == arm]
            v = [r["aggregate_scans_per_s"] for r in mine]
            s[arm] = dict(scans_per_s_median=float(np.median(v)), scans_per_s_min=min(v), scans_per_s_max=max(v),
                          spread=(max(v) - min(v)) / float(np.median(v)))
            for k in ("host_ms_load_mean", "host_ms_align_mean", "host_ms_update_mean"):
                if k in mine[0]:
                    s[arm][k + "_median"] = float(np.median([r[k] for r in mine]))
        gain = s["fleet_batched"]["scans_per_s_median"] / s["fleet_both_calls"]["scans_per_s_median"] - 1.
        spread = max(s["fleet_batched"]["spread"], s["fleet_both_calls"]["spread"])
        s["batched_over_both_calls"] = 1. + gain
        s["batched_over_replicas"] = s["fleet_batched"]["scans_per_s_median"] / s["replicas"]["scans_per_s_median"]
        s["verdict"] = ("within the spread" if abs(gain) <= spread else "faster" if gain > 0 else "slower") + \
                       " (%+.1f %%, spread %.1f %%)" % (100. * gain, 100. * spread)
        summary.append(s)
    out = dict(what="node_fleet R with the load and update phases of a step batched, each as R member calls, both as calls (the step before "
                    "they were batched), and node_replicas R, alternated in one run on one MI355X; %d timed scans per robot, 30 x 50 PSO, "
                    "60 m frame of 0.5 m cells, default (exact) score mode; host_ms_*: mean host time per phase of a step (load and update "
                    "only enqueue); hw_queues: GPU_MAX_HW_QUEUES of the child (null: the runtime's default)" % (args.scans - 10),
               summary=summary, runs=rows)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(summary))


if __name__ == "__main__":
    main()
