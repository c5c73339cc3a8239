"""The verified relocalization case shared by tests/test_gpu_map_search.py and tests/test_gpu_relocalize.py: the project's
synthetic room seen by a 361-beam sensor, a 60 m / 0.5 m map of six scans, a query scan taken at (1.3, -0.7, 0.45) and a
9 x 9 x 16 lattice around it.  Scans are synth.raycast plus default_rng(seed).normal(0, 0.01) noise, float32, misses 0."""
import functools

import numpy as np

N_BEAMS = 361
FRAME_M = 60
CELL_SIDE = 0.5
MAP_POSES = [(-6.0, -2.0, 0.3), (-3.0, -1.0, 0.2), (0.0, 0.0, 0.0), (3.0, 1.0, -0.2), (6.0, 2.0, -0.4), (2.0, -3.0, 1.5)]
QUERY_SEED = 99
TRUTH = (1.3, -0.7, 0.45)
ORIGIN = (0.0, -2.0, 0.0)
STEP = (0.3, 0.3, 0.06)
COUNT = (9, 9, 16)
TOP_K = 8
TAU_PER_POINT = 7e-7      # tau(n) = 7e-7 * n_points (DESIGN 3.3's floor)


def angle_inc():
    return np.float32(4.712389 / float(N_BEAMS - 1))


def scan(seed, pose):
    from ndtpso_slam_amd import synth
    clean = synth.raycast(np.asarray(pose, dtype=np.float64)[None, :], N_BEAMS, synth.ANGLE_MIN, angle_inc())[0]
    noise = np.random.default_rng(seed).normal(0, 0.01, N_BEAMS)
    return np.where(clean > 0, clean + noise, 0.0).astype(np.float32)


@functools.lru_cache(maxsize=None)
def ranges():
    """(the six map scans [6, beams], the query scan [beams])"""
    return np.stack([scan(s, p) for s, p in enumerate(MAP_POSES)]), scan(QUERY_SEED, TRUTH)


def geom():
    from ndtpso_slam_amd import capi, synth
    return capi.ScanGeom(N_BEAMS, synth.ANGLE_MIN, angle_inc(), synth.RANGE_MAX, 0.1)


def device_case(ctx, cell_side=CELL_SIDE, frame=FRAME_M, poses=MAP_POSES, build=True):
    """(map, query scan) on the device"""
    from ndtpso_slam_amd import capi
    grid = capi.Grid(frame, frame, cell_side)
    m = capi.ResidentMap(ctx, grid, pool_bytes=64 << 20)
    s = capi.ResidentScan(ctx, N_BEAMS)
    maps, query = ranges()
    for k, pose in enumerate(poses):
        s.load_scan(maps[k], geom(), clip=grid)
        m.insert(s, np.asarray(pose, dtype=np.float64))
    if build:
        m.build()
    s.load_scan(query, geom(), clip=grid)
    return m, s


@functools.lru_cache(maxsize=None)
def oracle_case():
    """(oracle map frame, oracle query frame, the lattice's costs by the oracle's cost_function [nodes]); computed once"""
    from ndtpso_slam_amd import capi, synth
    from oracle import pyoracle
    maps, query = ranges()
    ref = pyoracle.Frame((0, 0, 0), FRAME_M, FRAME_M, CELL_SIDE)
    for k, pose in enumerate(MAP_POSES):
        f = pyoracle.Frame((0, 0, 0), FRAME_M, FRAME_M, float(FRAME_M))
        f.load_laser(maps[k], synth.ANGLE_MIN, angle_inc(), synth.RANGE_MAX)
        ref.update(pose, f)
    new = pyoracle.Frame((0, 0, 0), FRAME_M, FRAME_M, float(FRAME_M))
    new.load_laser(query, synth.ANGLE_MIN, angle_inc(), synth.RANGE_MAX)
    poses = capi.lattice_poses(ORIGIN, STEP, COUNT)
    costs = np.array([ref.cost(p, new) for p in poses])
    costs.setflags(write=False)
    return ref, new, costs


def brute(m, s, origin, step, count, top_k, capi):
    """what a caller does without ndtpso_map_search: every node's pose -> ResidentMap.cost(F64) -> stable argsort"""
    poses = capi.lattice_poses(origin, step, count)
    costs = m.cost(s, poses, mode=capi.SCORE_F64)
    order = np.argsort(costs, kind="stable")[:min(top_k, len(costs))]
    return poses, costs, order
