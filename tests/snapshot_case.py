"""What the map-snapshot tests share (tests/test_gpu_map_snapshot.py, tests/test_map_snapshot_api.py, the golden's generator):
format 1's header as include/ndtpso_hip.h and ndtpso_map_snapshot.inc lay it out, the size bound of the contract, and the one
scan the pinned blob tests/golden/map_snapshot_v1.bin was made from."""
import os
import struct

import numpy as np

HEADER_BYTES = 320
# byte offsets of the header's fields (SnapHeader, ndtpso_map_snapshot.inc)
MAGIC, VERSION, HEADER_BYTES_AT, WINDOW_SIZE, MAX_POINTS_PER_CELL, CHUNK_POINTS, SIZEOF_CELL = 0, 8, 12, 16, 20, 24, 28
BYTES, CHECKSUM, SECTION_OFFSETS, HEADER_CHECKSUM = 32, 40, 208, 280
SECTIONS = ("created", "cells", "index", "win_sum", "win_cov", "win_count", "slot_len", "chunks", "og")

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "map_snapshot_v1.bin")
GOLDEN_INFO = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "map_snapshot_v1.json")
GOLDEN_BEAMS, GOLDEN_FRAME_M, GOLDEN_CELL_SIDE, GOLDEN_POSE, GOLDEN_SEED = 181, 20, 1.0, (1.0, -0.5, 0.2), 5


def fnv1a_words(data: bytes) -> int:
    """FNV-1a over little-endian 64-bit words"""
    h = 0xcbf29ce484222325
    for (w,) in struct.iter_unpack("<Q", data):
        h = ((h ^ w) * 0x100000001b3) & 0xFFFFFFFFFFFFFFFF
    return h


def section_offsets(blob: bytes) -> dict:
    off = struct.unpack_from("<9Q", blob, SECTION_OFFSETS)
    return dict(zip(SECTIONS, off))


def reseal(blob: bytes) -> bytes:
    """the header checksum computed again, as a writer of the altered header would have"""
    h = bytearray(blob[:HEADER_BYTES])
    body_sum = h[CHECKSUM:CHECKSUM + 8]
    h[CHECKSUM:CHECKSUM + 8] = bytes(8)
    h[HEADER_CHECKSUM:HEADER_CHECKSUM + 8] = bytes(8)
    s = fnv1a_words(bytes(h))
    h[CHECKSUM:CHECKSUM + 8] = body_sum
    h[HEADER_CHECKSUM:HEADER_CHECKSUM + 8] = struct.pack("<Q", s)
    return bytes(h) + blob[HEADER_BYTES:]


def with_u32(blob: bytes, at: int, value: int) -> bytes:
    b = bytearray(blob)
    struct.pack_into("<I", b, at, value)
    return reseal(bytes(b))


def size_bound(info: dict) -> int:
    """the contract's bound (include/ndtpso_hip.h)"""
    return 4096 + 192 * info["n_created"] + 80 * info["n_slots_used"] + 528 * info["n_chunks"] + 8 * info["og_box_entries"]


def golden_geom():
    from ndtpso_slam_amd import capi, synth
    return capi.ScanGeom(GOLDEN_BEAMS, synth.ANGLE_MIN, np.float32(4.712389 / float(GOLDEN_BEAMS - 1)), synth.RANGE_MAX, 0.1)


def golden_scan() -> np.ndarray:
    """the golden's one scan: synth.raycast from GOLDEN_POSE plus default_rng(GOLDEN_SEED).normal(0, 0.01), float32, misses 0"""
    from ndtpso_slam_amd import synth
    g = golden_geom()
    clean = synth.raycast(np.asarray(GOLDEN_POSE, dtype=np.float64)[None, :], GOLDEN_BEAMS, synth.ANGLE_MIN, g.angle_increment)[0]
    noise = np.random.default_rng(GOLDEN_SEED).normal(0, 0.01, GOLDEN_BEAMS)
    return np.where(clean > 0, clean + noise, 0.0).astype(np.float32)


def golden_map(ctx):
    """(the map the golden is a snapshot of, its scan on the device): one scan inserted as loaded, built"""
    from ndtpso_slam_amd import capi
    grid = capi.Grid(GOLDEN_FRAME_M, GOLDEN_FRAME_M, GOLDEN_CELL_SIDE)
    m = capi.ResidentMap(ctx, grid, pool_bytes=1 << 20)
    s = capi.ResidentScan(ctx, GOLDEN_BEAMS)
    s.load_scan(golden_scan(), golden_geom(), clip=grid)
    m.insert(s)
    m.build()
    return m, s
