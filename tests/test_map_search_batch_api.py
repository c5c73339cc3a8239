"""ndtpso_map_search_batch without a device: the C-ABI's structures against the header's defines, the symbol and its binding, and
the replay tool of NDTFrame::relocalizeBatch in the host library's build."""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _define(header, name):
    m = re.search(r"#define %s (\d+)\b" % name, header)
    assert m, name
    return int(m.group(1))


def test_struct_sizes_and_offsets_match_the_header():
    from ndtpso_slam_amd import capi
    header = open(os.path.join(ROOT, "include", "ndtpso_hip.h")).read()
    job, bs = capi.MapSearchJob, capi.SearchBatchStats
    assert C.sizeof(job) == _define(header, "NDTPSO_MAP_SEARCH_JOB_BYTES") == 136
    assert C.sizeof(bs) == _define(header, "NDTPSO_SEARCH_BATCH_STATS_BYTES") == 16
    assert job.map.offset == 0 and job.new_points.offset == 8 and job.lattice.offset == 16
    assert C.sizeof(capi.Lattice) == _define(header, "NDTPSO_LATTICE_BYTES")
    assert job.hits.offset == _define(header, "NDTPSO_MAP_SEARCH_JOB_HITS_OFFSET") == 80
    assert job.n_hits.offset == 88
    assert job.rc.offset == _define(header, "NDTPSO_MAP_SEARCH_JOB_RC_OFFSET") == 92
    assert job.route.offset == 96
    assert job.stats.offset == _define(header, "NDTPSO_MAP_SEARCH_JOB_STATS_OFFSET") == 104
    assert C.sizeof(capi.SearchStats) == _define(header, "NDTPSO_SEARCH_STATS_BYTES")
    assert [f for f, _ in bs._fields_] == ["launches", "waits", "single_jobs", "reserved"]
    assert bs.waits.offset == 4 and bs.single_jobs.offset == 8
    # the header asserts the same sizes to a C and a C++ compiler
    assert "static_assert(sizeof(ndtpso_map_search_job) == NDTPSO_MAP_SEARCH_JOB_BYTES" in header
    assert "_Static_assert(sizeof(ndtpso_map_search_job) == NDTPSO_MAP_SEARCH_JOB_BYTES" in header


def test_symbol_is_exported_with_five_arguments():
    from ndtpso_slam_amd import capi
    L = capi.load()
    assert "ndtpso_map_search_batch" in capi.EXPORTS
    assert hasattr(L, "ndtpso_map_search_batch")
    assert L.ndtpso_map_search_batch.argtypes is not None and len(L.ndtpso_map_search_batch.argtypes) == 5
    assert L.ndtpso_map_search_batch.restype is C.c_int
    assert callable(capi.search_maps)


def test_job_kernels_are_a_unit_of_their_own():
    units = open(os.path.join(ROOT, "ndtpso_slam_amd", "csrc", "hip_units.txt")).read().split()
    assert "ndtpso_map_search_jobs.hip" in units and "ndtpso_map_search.hip" in units


def test_relocalize_fleet_check_builds():
    from ndtpso_slam_amd import build
    build.build_hip()
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "host"), "libndtpso_slam.so", "replay/relocalize_fleet_check"],
                          stdout=subprocess.DEVNULL)
    exe = os.path.join(ROOT, "host", "replay", "relocalize_fleet_check")
    assert os.access(exe, os.X_OK)
    assert subprocess.run([exe]).returncode == 2       # usage: no arguments, nothing touched
