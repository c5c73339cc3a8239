#!/usr/bin/env python3
"""Records what ndtpso_align_pairs_describe answers over a grid of fused-pairs configurations (no device needed).

    python scripts/record_pairs_plans.py [OUT.npz]     (default: tests/golden/pairs_plans.npz)

The library is the one capi.load() finds: NDTPSO_LIB names another build, e.g. the one a host-side change is compared
against.  tests/test_pairs_plan_golden.py compares the library under test with the recorded file, field for field.
"""
import itertools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from ndtpso_slam_amd import capi, synth  # noqa: E402

BEAMS = (181, 361, 541, 721, 1081, 1441, 2048)
CELL_SIDES = (0.25, 0.3, 0.5, 1.0)
FRAMES = (60, 100)
POPULATIONS = (16, 30, 70, 300, 2048)
ITERATIONS = 50
N_PAIRS = (6, 512)
MODES = (capi.SCORE_F32, capi.SCORE_F64, capi.SCORE_EXACT)
KEY_NAMES = ("beams", "cell_side", "frame", "population", "n_pairs", "mode")
FIELDS = ("rc",) + tuple(k for k, _ in capi.PairsPlan._fields_)
DEFAULT_OUT = os.path.join(ROOT, "tests", "golden", "pairs_plans.npz")


def describe_all():
    """(keys [N, 6] float64, rows [N, len(FIELDS)] int64): every combination, in itertools.product order."""
    fov = float(synth.ANGLE_INC) * (synth.N_BEAMS - 1)   # synth's field of view, whatever the number of beams
    keys, rows = [], []
    for beams, cs, frame, pop, n_pairs, mode in itertools.product(BEAMS, CELL_SIDES, FRAMES, POPULATIONS, N_PAIRS, MODES):
        geom = capi.ScanGeom(beams, float(synth.ANGLE_MIN), fov / (beams - 1), float(synth.RANGE_MAX), 0.1)
        rc, plan = capi.align_pairs_describe(geom, capi.Grid(frame, frame, cs), capi.PSOConfig.make(ITERATIONS, pop), mode, n_pairs)
        keys.append((beams, cs, frame, pop, n_pairs, mode))
        rows.append((rc,) + tuple(int(plan[k]) for k in FIELDS[1:]))
    return np.array(keys, dtype=np.float64), np.array(rows, dtype=np.int64)


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else DEFAULT_OUT
    keys, rows = describe_all()
    np.savez_compressed(out, keys=keys, rows=rows, key_names=np.array(KEY_NAMES), fields=np.array(FIELDS))
    print("%s: %d configurations x %d fields, %d bytes" % (out, rows.shape[0], rows.shape[1], os.path.getsize(out)))


if __name__ == "__main__":
    main()
