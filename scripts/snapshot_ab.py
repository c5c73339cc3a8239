"""A resident map brought back from a blob against the only faithful way there was before: ResidentMap.snapshot +
ResidentMap.restore (ndtpso_map_snapshot / ndtpso_map_restore) against replaying the K scans the map absorbed -- a fresh map, K x
(insert + build).  Maps of K = 6, 100, 1000 and 10 000 scans of 1081 beams in the 60 m / 0.5 m frame (the scans are 64 views
along a loop through the synthetic room, taken in turn); the two ways alternate in one process after a warm-up of each size, a
host clock around the synchronous calls (Python binding included on both sides, the map's allocation on both sides).  Before
anything is timed the restored map, the replayed map and the original are checked equal: cells and every stored point bit for bit,
the restored map's own snapshot the blob byte for byte, the replayed map's the same counts.

    python scripts/snapshot_ab.py [--out profiles/snapshot_ab.json] [--reps 10] [--warm 2] [--sizes 6,100,1000,10000]
    python scripts/snapshot_ab.py --profile-pass 1000      # snapshot + restore only, for a kernel trace of their own:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o t -- python scripts/snapshot_ab.py --profile-pass 1000
    python scripts/snapshot_ab.py --kernel-stats DIR/.../t_kernel_stats.csv --kernel-stats-size 1000   # folded into the JSON
"""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N_VIEWS = 64
POOL = 512 << 20
KERNELS = ("k_snapshot_count", "k_snapshot_scan", "k_snapshot_gather", "k_restore_scatter", "k_map_pack")


def views():
    from ndtpso_slam_amd import synth
    rng = np.random.default_rng(4)
    t = np.linspace(0.0, 2 * np.pi, N_VIEWS, endpoint=False)
    poses = np.stack([3.0 * np.cos(t), 2.0 * np.sin(t), t + np.pi / 2], axis=1)
    clean = synth.raycast(poses)
    return poses, np.where(clean > 0, clean + rng.normal(0, 0.01, clean.shape), 0.0).astype(np.float32)


def kernel_stats(path):
    out = {}
    with open(path) as f:
        for row in csv.DictReader(f):
            for k in KERNELS:
                if k + "(" in row["Name"]:
                    out[k] = dict(calls=int(row["Calls"]), average_us=float(row["AverageNs"]) / 1e3, min_us=float(row["MinNs"]) / 1e3,
                                  max_us=float(row["MaxNs"]) / 1e3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "snapshot_ab.json"))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--sizes", default="6,100,1000,10000")
    ap.add_argument("--profile-pass", type=int, default=0, help="only snapshot + restore of a map of this many scans, 20 times")
    ap.add_argument("--kernel-stats", default=None, help="a rocprofv3 --stats CSV of a --profile-pass run, folded into --out")
    ap.add_argument("--kernel-stats-size", type=int, default=1000)
    args = ap.parse_args()
    if args.kernel_stats:
        with open(args.out) as f:
            out = json.load(f)
        out["kernels"] = dict(scans=args.kernel_stats_size, what="one rocprofv3 --kernel-trace --stats run of snapshot + restore alone "
                              "(--profile-pass), device time per launch", **kernel_stats(args.kernel_stats))
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
        return
    from ndtpso_slam_amd import capi, synth
    geom = capi.ScanGeom(synth.N_BEAMS, synth.ANGLE_MIN, synth.ANGLE_INC, synth.RANGE_MAX, 0.1)
    grid = capi.Grid(60, 60, 0.5)
    ctx = capi.Context(0)
    poses, ranges = views()
    scans = []
    for v in range(N_VIEWS):
        s = capi.ResidentScan(ctx, synth.N_BEAMS)
        s.load_scan(ranges[v], geom, clip=grid)
        scans.append(s)

    def replay(k_scans):
        m = capi.ResidentMap(ctx, grid, pool_bytes=POOL)
        for k in range(k_scans):
            m.insert(scans[k % N_VIEWS], poses[k % N_VIEWS])
            m.build()
        ctx.synchronize()
        return m

    def key(m):
        return [(c["index"], c["count"], c["built"], c["slot"], c["mean"].tobytes(), c["icov"].tobytes()) for c in m.cells()]

    if args.profile_pass:
        m = replay(args.profile_pass)
        for _ in range(20):
            capi.ResidentMap.restore(ctx, m.snapshot(), pool_bytes=POOL).close()
        return
    rows = []
    for k_scans in [int(v) for v in args.sizes.split(",")]:
        original = replay(k_scans)
        blob = original.snapshot()
        info = capi.snapshot_describe(blob)
        restored, replayed = capi.ResidentMap.restore(ctx, blob, pool_bytes=POOL), replay(k_scans)
        # (two maps accumulated apart hold the same cells, but the cells one insert creates enter created[] in the order its
        # threads' atomics land: their blobs may list the cells in another order.  A restored map keeps its blob's order.)
        for name, m in (("restored", restored), ("replayed", replayed)):
            if not (key(m) == key(original) and np.array_equal(m.points(), original.points())):
                raise SystemExit("the %s map of %d scans differs from the original" % (name, k_scans))
        if restored.snapshot() != blob or capi.snapshot_describe(replayed.snapshot()) != info:
            raise SystemExit("%d scans: the restored map's blob is not the blob, or the replayed map's holds other counts" % k_scans)
        restored.close()
        replayed.close()
        times = dict(replay=[], snapshot=[], restore=[], snapshot_restore=[])
        for rep in range(args.warm + args.reps):
            t0 = time.perf_counter()
            m = replay(k_scans)
            lap = dict(replay=time.perf_counter() - t0)
            m.close()
            t0 = time.perf_counter()
            b = original.snapshot()
            t1 = time.perf_counter()
            m = capi.ResidentMap.restore(ctx, b, pool_bytes=POOL)
            t2 = time.perf_counter()
            m.close()
            lap.update(snapshot=t1 - t0, restore=t2 - t1, snapshot_restore=t2 - t0)
            if rep >= args.warm:
                for k, v in lap.items():
                    times[k].append(1e3 * v)
        row = dict(scans=k_scans, equal=True, blob_bytes=len(blob),
                   info={k: info[k] for k in ("n_created", "n_built", "n_slots_used", "n_chunks", "n_points_stored")})
        for k, v in times.items():
            v = np.array(v)
            row[k + "_ms"] = dict(median=float(np.median(v)), p5=float(np.percentile(v, 5)), p95=float(np.percentile(v, 95)))
        r = np.array(times["replay"]) / np.array(times["snapshot_restore"])
        row["replay_over_snapshot_restore"] = dict(of_medians=float(np.median(times["replay"]) / np.median(times["snapshot_restore"])),
                                                   p5=float(np.percentile(r, 5)), p95=float(np.percentile(r, 95)))
        rows.append(row)
        print(json.dumps(row), flush=True)
        original.close()
    out = dict(what="ResidentMap.snapshot + ResidentMap.restore against a fresh map and K x (insert + build), maps of K scans of 1081 "
                    "beams (64 views along a loop, in turn), 60 m frame, 0.5 m cells, alternated in one process, %d repetitions after %d "
                    "warm-up laps per size; host clock around the synchronous calls, Python binding and the map's allocation included "
                    "on both sides; restored, replayed and original map checked equal (cells and points bit for bit, the restored map's snapshot the blob byte for byte) before timing"
                    % (args.reps, args.warm), rows=rows)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
