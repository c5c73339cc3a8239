"""Several start poses for one scan: M guesses against one resident map through capi.align_maps (one launch) against M calls of
ResidentMap.align, alternated, a host clock around calls that end in the result wait.  30 x 50 PSO, exact mode, 60 m frame of
0.5 m cells; the results of the two must be equal.

    python scripts/multistart_ab.py [--out profiles/multistart.json] [--m 8,32,128] [--reps 200]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "multistart.json"))
    ap.add_argument("--m", default="8,32,128")
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warm", type=int, default=5)
    args = ap.parse_args()
    from ndtpso_slam_amd import capi, synth
    rng = np.random.default_rng(4)
    s = np.linspace(0.0, 0.6, 5)
    poses = np.stack([2.0 + 1.2 * s, -1.0 + 0.8 * np.sin(1.5 * s), 0.3 + 0.25 * s], axis=1)
    clean = synth.raycast(poses)
    ranges = np.where(clean > 0, clean + rng.normal(0, 0.01, clean.shape), 0.0).astype(np.float32)
    geom = capi.ScanGeom(synth.N_BEAMS, synth.ANGLE_MIN, synth.ANGLE_INC, synth.RANGE_MAX, 0.1)
    grid, cfg, dev = capi.Grid(60, 60, 0.5), capi.PSOConfig.make(50, 30), (0.1, 0.1, 3.1415e-3)
    ctx = capi.Context(0)
    rmap, scan = capi.ResidentMap(ctx, grid, pool_bytes=64 << 20), capi.ResidentScan(ctx, synth.N_BEAMS)
    c0, s0 = np.cos(poses[0, 2]), np.sin(poses[0, 2])
    rel = [np.array([c0 * (p[0] - poses[0, 0]) + s0 * (p[1] - poses[0, 1]), -s0 * (p[0] - poses[0, 0]) + c0 * (p[1] - poses[0, 1]),
                     p[2] - poses[0, 2]]) for p in poses]
    for k in range(4):
        scan.load_scan(ranges[k], geom, clip=grid)
        rmap.insert(scan, rel[k])
    scan.load_scan(ranges[4], geom, clip=grid)
    rows = []
    for M in [int(v) for v in args.m.split(",")]:
        jobs = [(rmap, scan, rel[3] + np.array([0.05 * np.cos(j), 0.05 * np.sin(j), 0.002 * (j % 11 - 5)]), dev, 100 + j) for j in range(M)]
        t_batch, t_single, equal, route = [], [], True, None
        for rep in range(args.warm + args.reps):
            t0 = time.perf_counter()
            got = capi.align_maps(ctx, jobs, cfg, capi.SCORE_EXACT)
            t1 = time.perf_counter()
            one = [m.align(sc, g, d, cfg, seed=seed, mode=capi.SCORE_EXACT) for m, sc, g, d, seed in jobs]
            t2 = time.perf_counter()
            if rep == 0:
                equal = all(np.array_equal(got[0][j], one[j][0]) and got[1][j] == one[j][1] for j in range(M)) and bool((got[3] == 0).all())
                route = sorted({int(r) for r in got[4]})
            if rep >= args.warm:
                t_batch.append(1e3 * (t1 - t0))
                t_single.append(1e3 * (t2 - t1))
        b, o = np.array(t_batch), np.array(t_single)
        row = dict(guesses=M, equal=bool(equal), route=route, align_maps_ms_median=float(np.median(b)), align_maps_ms_p5=float(np.percentile(b, 5)),
                   align_maps_ms_p95=float(np.percentile(b, 95)), m_calls_ms_median=float(np.median(o)), m_calls_ms_p5=float(np.percentile(o, 5)),
                   m_calls_ms_p95=float(np.percentile(o, 95)), ratio_of_medians=float(np.median(o) / np.median(b)),
                   ratio_p5=float(np.percentile(o / b, 5)), ratio_p95=float(np.percentile(o / b, 95)))
        rows.append(row)
        print(json.dumps(row), flush=True)
        if not equal:
            raise SystemExit("align_maps and the single calls differ")
    out = dict(what="M start poses for one scan against one resident map (4 inserted scans, 60 m frame, 0.5 m cells), 30 x 50 PSO, exact "
                    "mode: capi.align_maps (one call) against M calls of ResidentMap.align, alternated, %d repetitions after %d warm-up; "
                    "host clock around the calls, Python binding included on both sides; ratio = time of the M calls / time of the one" %
                    (args.reps, args.warm), rows=rows)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
