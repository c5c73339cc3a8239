"""Regenerates tests/golden/map_snapshot_v1.bin and map_snapshot_v1.json: format 1 of the map snapshot (include/ndtpso_hip.h), pinned.

One 181-beam scan of the synthetic room in a 20 m frame of 1 m cells, inserted as loaded and built, no occupancy grid
(tests/snapshot_case.py: golden_map); the blob is ResidentMap.snapshot() of it and the JSON what capi.snapshot_describe says of
the blob.  Needs the GPU -- the blob is made by the kernels it pins:

    python tests/golden/make_golden_snapshot.py [output directory, default: this one]

A blob that differs from the committed one means the format or the device arithmetic of the map has changed: the first is a new
format version, not a new golden.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

import snapshot_case as snc  # noqa: E402
from ndtpso_slam_amd import capi  # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else HERE
    os.makedirs(out, exist_ok=True)
    ctx = capi.Context(0)
    m, _ = snc.golden_map(ctx)
    blob = m.snapshot()
    info = capi.snapshot_describe(blob)
    assert capi.ResidentMap.restore(ctx, blob, pool_bytes=1 << 20).snapshot() == blob
    with open(os.path.join(out, os.path.basename(snc.GOLDEN)), "wb") as f:
        f.write(blob)
    with open(os.path.join(out, os.path.basename(snc.GOLDEN_INFO)), "w") as f:
        json.dump(info, f, indent=1, sort_keys=True)
        f.write("\n")
    print(len(blob), "bytes", info)
    ctx.close()


if __name__ == "__main__":
    main()
