"""R lattice searches, one per robot against its own resident map: R ndtpso_map_search calls one after the other against ONE
ndtpso_map_search_batch call, in the same process on the same maps, alternating, so that the spread of either is known.  R = 4,
16 and 64; lattices of 1296 nodes (the verified relocalization case), about 1e5 nodes, and as many as make the call's total 2^24
(the cap of a call); NDTPSO_SCORE_F64 and NDTPSO_SCORE_EXACT.  Maps of the verified case's shape (361 beams, 60 m frame, 0.5 m
cells, six inserted scans).  A host clock around the C entries themselves, called through ctypes with arguments made once (the
same on both sides: no result is converted while the clock runs).  The batch's hits are checked bit for bit against the single
calls' before anything is timed.

    python scripts/search_batch_ab.py [--out profiles/search_batch_ab.json] [--reps 15] [--warm 3] [--top-k 8]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N_BEAMS = 361
MAP_POSES = [(-6.0, -2.0, 0.3), (-3.0, -1.0, 0.2), (0.0, 0.0, 0.0), (3.0, 1.0, -0.2), (6.0, 2.0, -0.4), (2.0, -3.0, 1.5)]
ROBOTS = (4, 16, 64)
CAP = 1 << 24


def lattices(n_robots):
    """(name, count, step) -- a patch around the robot's pose, headings over 0.96 rad, as the verified case's 9 x 9 x 16"""
    side = int(np.sqrt(CAP // n_robots // 64))
    return [("1296", (9, 9, 16), (0.3, 0.3, 0.06)),
            ("1e5", (48, 48, 44), (0.05625, 0.05625, 0.96 / 44)),
            ("cap", (side, side, 64), (2.7 / side, 2.7 / side, 0.96 / 64))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "search_batch_ab.json"))
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--top-k", type=int, default=8)
    args = ap.parse_args()
    from ndtpso_slam_amd import capi, synth
    ainc = np.float32(4.712389 / float(N_BEAMS - 1))
    geom = capi.ScanGeom(N_BEAMS, synth.ANGLE_MIN, ainc, synth.RANGE_MAX, 0.1)
    grid = capi.Grid(60, 60, 0.5)
    rng = np.random.default_rng(4)

    def scan_at(pose):
        clean = synth.raycast(np.asarray(pose, dtype=np.float64)[None, :], N_BEAMS, synth.ANGLE_MIN, ainc)[0]
        return np.where(clean > 0, clean + rng.normal(0, 0.01, N_BEAMS), 0.0).astype(np.float32)

    map_scans = [scan_at(p) for p in MAP_POSES]
    ctx = capi.Context(0)
    L = ctx._lib
    robots = []
    for r in range(max(ROBOTS)):  # every robot its own map and its own query scan, taken somewhere else
        m, s = capi.ResidentMap(ctx, grid, pool_bytes=16 << 20), capi.ResidentScan(ctx, N_BEAMS)
        for k, pose in enumerate(MAP_POSES):
            s.load_scan(map_scans[k], geom, clip=grid)
            m.insert(s, np.asarray(pose, dtype=np.float64))
        m.build()
        truth = (-4.0 + 8.0 * (r % 8) / 7.0, -2.0 + 3.0 * (r // 8) / 7.0, -0.4 + 0.1 * (r % 9))
        s.load_scan(scan_at(truth), geom, clip=grid)
        robots.append((m, s, truth))
    modes = (("f64", capi.SCORE_F64), ("exact", capi.SCORE_EXACT))
    rows = []
    for n_robots in ROBOTS:
        for name, count, step in lattices(n_robots):
            nodes = count[0] * count[1] * count[2]
            arr = (capi.MapSearchJob * n_robots)()
            single_hits = [(capi.LatticeHit * args.top_k)() for _ in range(n_robots)]
            batch_hits = [(capi.LatticeHit * args.top_k)() for _ in range(n_robots)]
            for j, (m, s, truth) in zip(arr, robots):
                origin = [truth[a] - step[a] * (count[a] - 1) / 2 for a in range(3)]
                j.map, j.new_points = m._h, s._h
                j.lattice = capi.Lattice((C.c_double * 3)(*origin), (C.c_double * 3)(*step), (C.c_uint32 * 3)(*count), args.top_k)
            n_hits, st, bs = C.c_uint32(), capi.SearchStats(), capi.SearchBatchStats()

            def singles(mode):
                for j, hits in zip(arr, single_hits):
                    rc = L.ndtpso_map_search(j.map, j.new_points, C.byref(j.lattice), mode, hits, C.byref(n_hits), C.byref(st))
                    if rc != capi.OK:
                        raise SystemExit("ndtpso_map_search: %d" % rc)

            def batch(mode):
                for j, hits in zip(arr, batch_hits):
                    j.hits = hits
                rc = L.ndtpso_map_search_batch(ctx._h, arr, n_robots, mode, C.byref(bs))
                if rc != capi.OK:
                    raise SystemExit("ndtpso_map_search_batch: %d" % rc)

            row = dict(robots=n_robots, lattice=name, count=list(count), nodes=nodes, total_nodes=nodes * n_robots, top_k=args.top_k)
            for mode_name, mode in modes:
                singles(mode)
                batch(mode)
                for a, b in zip(single_hits, batch_hits):
                    if bytes(a) != bytes(b):
                        raise SystemExit("batch and single calls differ (%s, R = %d, %s)" % (mode_name, n_robots, name))
                fell = sorted({int(j.stats.fell_back) for j in arr})
                t_single, t_batch = [], []
                for rep in range(args.warm + args.reps):
                    t0 = time.perf_counter()
                    singles(mode)
                    t1 = time.perf_counter()
                    batch(mode)
                    t2 = time.perf_counter()
                    if rep >= args.warm:
                        t_single.append(1e3 * (t1 - t0))
                        t_batch.append(1e3 * (t2 - t1))
                t_single, t_batch = np.array(t_single), np.array(t_batch)
                ratio = t_single / t_batch
                row[mode_name] = dict(
                    equal=True, fell_back=fell, launches=int(bs.launches), waits=int(bs.waits), single_jobs=int(bs.single_jobs),
                    singles_ms=dict(median=float(np.median(t_single)), p5=float(np.percentile(t_single, 5)), p95=float(np.percentile(t_single, 95))),
                    batch_ms=dict(median=float(np.median(t_batch)), p5=float(np.percentile(t_batch, 5)), p95=float(np.percentile(t_batch, 95))),
                    singles_over_batch=dict(of_medians=float(np.median(t_single) / np.median(t_batch)), p5=float(np.percentile(ratio, 5)),
                                            p95=float(np.percentile(ratio, 95))))
            rows.append(row)
            print(json.dumps(row), flush=True)
    out = dict(what="R ndtpso_map_search calls against one ndtpso_map_search_batch call, R robots with maps and query scans of their own "
                    "(361 beams, 60 m frame, 0.5 m cells, six inserted scans), alternated in one process, %d repetitions after %d warm-up "
                    "laps per point; host clock around the C entries (ctypes, arguments made once); hits checked bit for bit before "
                    "timing; singles_over_batch > 1: the batch call is faster" % (args.reps, args.warm), rows=rows)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
