"""ndtpso_map_search without a device: the C-ABI's structures and symbol, capi.lattice_poses against the contract's formula,
and the replay tool of NDTFrame::relocalize in the host library's build."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_struct_sizes_match_the_header():
    from ndtpso_slam_amd import capi
    assert C.sizeof(capi.Lattice) == 64
    assert C.sizeof(capi.LatticeHit) == 40
    assert C.sizeof(capi.SearchStats) == 32
    header = open(os.path.join(ROOT, "include", "ndtpso_hip.h")).read()
    for name, size in (("NDTPSO_LATTICE_BYTES", 64), ("NDTPSO_LATTICE_HIT_BYTES", 40), ("NDTPSO_SEARCH_STATS_BYTES", 32)):
        assert "#define %s %d" % (name, size) in header
    assert capi.LatticeHit.cost.offset == 24 and capi.LatticeHit.index.offset == 32
    assert capi.Lattice.count.offset == 48 and capi.Lattice.top_k.offset == 60
    assert capi.SearchStats.fell_back.offset == 20


def test_symbol_is_exported():
    from ndtpso_slam_amd import capi
    L = capi.load()
    assert "ndtpso_map_search" in capi.EXPORTS
    assert hasattr(L, "ndtpso_map_search")
    assert L.ndtpso_map_search.argtypes is not None and len(L.ndtpso_map_search.argtypes) == 7


def test_lattice_poses_follow_the_formula_bit_for_bit():
    """origin + float(i) * step, one multiplication and one addition per component, on steps that are not representable; node
    (i, j, k) at index (k * ny + j) * nx + i"""
    from ndtpso_slam_amd import capi
    origin, step, count = (0.1, -2.0, 0.05), (0.3, 0.3, 0.06), (9, 7, 16)
    poses = capi.lattice_poses(origin, step, count)
    nx, ny, nth = count
    assert poses.shape == (nx * ny * nth, 3) and poses.dtype == np.float64
    for k in range(nth):
        for j in range(ny):
            for i in range(nx):
                want = [origin[0] + float(i) * step[0], origin[1] + float(j) * step[1], origin[2] + float(k) * step[2]]
                got = poses[(k * ny + j) * nx + i]
                assert got.tobytes() == np.array(want).tobytes(), (i, j, k, got, want)
    # (not a running sum: origin + step + step + ... differs from it in the last bits on these steps)
    walked = np.cumsum([0.1] + [0.3] * 8)
    assert not np.array_equal(walked, poses[:9, 0])
    # an axis of one node does not read its step
    one = capi.lattice_poses((1.0, 2.0, 3.0), (float("nan"), 0.3, float("inf")), (1, 2, 1))
    assert one.tolist() == [[1.0, 2.0, 3.0], [1.0, 2.3, 3.0]]


def test_relocalize_check_builds():
    from ndtpso_slam_amd import build
    build.build_hip()
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "host"), "libndtpso_slam.so", "replay/relocalize_check"],
                          stdout=subprocess.DEVNULL)
    exe = os.path.join(ROOT, "host", "replay", "relocalize_check")
    assert os.access(exe, os.X_OK)
    assert subprocess.run([exe]).returncode == 2       # usage: no arguments, nothing touched
