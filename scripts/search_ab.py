"""A pose lattice searched against one resident map: ResidentMap.search (ndtpso_map_search: the sweep and the selection on the
device) in its three score modes against the way a caller had to do it before -- capi.lattice_poses, every pose through
ResidentMap.cost(F64), argsort on the host.  One map of the benchmark's shape (1081 beams, 0.5 m cells, 60 m frame, 20 inserted
scans), lattices of about 1e4, 1e5 and 1e6 nodes; the two ways alternate in one process after a warm-up of each shape, a host
clock around the synchronous calls (Python binding included on both sides).  The results are checked equal before anything is
timed: the F64 and EXACT searches must return the caller's own best nodes, bit for bit.

    python scripts/search_ab.py [--out profiles/search_ab.json] [--reps 20] [--warm 3] [--top-k 8]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LATTICES = [  # (count, step): a 6.3 m x 6.3 m patch around the query's true pose, every heading
    ((22, 22, 20), (0.3, 0.3, 2 * np.pi / 20)),
    ((48, 48, 44), (0.134, 0.134, 2 * np.pi / 44)),
    ((100, 100, 100), (0.063, 0.063, 2 * np.pi / 100)),
]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "search_ab.json"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--top-k", type=int, default=8)
    ap.add_argument("--min-nodes", type=int, default=0, help="skip smaller lattices (a profiler pass wants one size)")
    ap.add_argument("--max-nodes", type=int, default=1 << 24, help="skip larger lattices")
    args = ap.parse_args()
    from ndtpso_slam_amd import capi, synth
    rng = np.random.default_rng(4)
    s = np.linspace(0.0, 3.0, 21)
    poses = np.stack([-4.0 + 2.4 * s, -1.0 + 0.8 * np.sin(1.5 * s), 0.3 + 0.25 * s], axis=1)
    clean = synth.raycast(poses)
    ranges = np.where(clean > 0, clean + rng.normal(0, 0.01, clean.shape), 0.0).astype(np.float32)
    geom = capi.ScanGeom(synth.N_BEAMS, synth.ANGLE_MIN, synth.ANGLE_INC, synth.RANGE_MAX, 0.1)
    grid = capi.Grid(60, 60, 0.5)
    ctx = capi.Context(0)
    rmap, scan = capi.ResidentMap(ctx, grid, pool_bytes=256 << 20), capi.ResidentScan(ctx, synth.N_BEAMS)
    for k in range(20):  # the map in world coordinates: every scan inserted where it was taken
        scan.load_scan(ranges[k], geom, clip=grid)
        rmap.insert(scan, poses[k])
    rmap.build()
    scan.load_scan(ranges[20], geom, clip=grid)
    truth = poses[20]
    modes = (("f64", capi.SCORE_F64), ("exact", capi.SCORE_EXACT), ("f32", capi.SCORE_F32))
    rows = []
    for count, step in LATTICES:
        nodes = count[0] * count[1] * count[2]
        if nodes > args.max_nodes or nodes < args.min_nodes:
            continue
        origin = (truth[0] - step[0] * (count[0] - 1) / 2, truth[1] - step[1] * (count[1] - 1) / 2, -np.pi)

        def callers_way():
            lattice = capi.lattice_poses(origin, step, count)
            costs = rmap.cost(scan, lattice, mode=capi.SCORE_F64)
            order = np.argsort(costs, kind="stable")[:args.top_k]
            return lattice[order], costs[order], order

        want = callers_way()
        stats = {}
        for name, mode in modes:
            got = rmap.search(scan, origin, step, count, args.top_k, mode=mode)
            stats[name] = got[3]
            if name != "f32" and not (got[2].tolist() == want[2].tolist() and got[1].tobytes() == want[1].tobytes() and
                                      got[0].tobytes() == want[0].tobytes()):
                raise SystemExit("search (%s) and the caller's way differ on %r: %r / %r" % (name, count, got[:3], want))
        times = {name: [] for name, _ in modes}
        times["callers_way"] = []
        for rep in range(args.warm + args.reps):
            t0 = time.perf_counter()
            callers_way()
            lap = {"callers_way": time.perf_counter() - t0}
            for name, mode in modes:
                t0 = time.perf_counter()
                rmap.search(scan, origin, step, count, args.top_k, mode=mode)
                lap[name] = time.perf_counter() - t0
            if rep >= args.warm:
                for k, v in lap.items():
                    times[k].append(1e3 * v)
        row = dict(count=list(count), nodes=nodes, top_k=args.top_k, equal=True, best_node=int(want[2][0]), best_cost=float(want[1][0]),
                   stats=stats)
        for k, v in times.items():
            v = np.array(v)
            row[k + "_ms"] = dict(median=float(np.median(v)), p5=float(np.percentile(v, 5)), p95=float(np.percentile(v, 95)))
        base = np.array(times["callers_way"])
        for name, _ in modes:
            r = base / np.array(times[name])
            row["callers_way_over_" + name] = dict(of_medians=float(np.median(base) / np.median(times[name])), p5=float(np.percentile(r, 5)),
                                                   p95=float(np.percentile(r, 95)))
        row["exact_over_f64"] = float(np.median(times["exact"]) / np.median(times["f64"]))
        rows.append(row)
        print(json.dumps(row), flush=True)
    out = dict(what="ResidentMap.search in three score modes against lattice_poses -> ResidentMap.cost(F64) -> argsort, one resident map "
                    "(20 inserted scans of 1081 beams, 60 m frame, 0.5 m cells), alternated in one process, %d repetitions after %d "
                    "warm-up laps per lattice; host clock around the synchronous calls, Python binding included on both sides; the F64 "
                    "and EXACT results checked bit for bit against the caller's way before timing" % (args.reps, args.warm), rows=rows)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
