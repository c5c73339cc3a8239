"""The contract of ndtpso_map_trace / ndtpso_map_get_nav_grid (include/ndtpso_hip.h) restated in plain Python and numpy fp64:
one function for a ray's cells, one for a scan's counters, one for the nav grid from occupancy() and the counters.  Python floats
are IEEE doubles and nothing here is fused, so every operation rounds as the header says.  cos and sin of the heading are passed
in: the device takes them from its own sincos (Context.device_math("sincos", ...))."""
import math

import numpy as np


def inside(q, hw, hh):
    return abs(q[0]) < hw and abs(q[1]) < hh


def ray_setup(o, e, hw, hh, cs):
    """(ix, iy, jx, jy, sx, sy, nx, ny, tx0, tdx, ty0, tdy) of a ray with both ends inside the frame"""
    fx0, fy0 = (o[0] + hw) / cs, (o[1] + hh) / cs
    fx1, fy1 = (e[0] + hw) / cs, (e[1] + hh) / cs
    ix, iy = int(math.floor(fx0)), int(math.floor(fy0))
    jx, jy = int(math.floor(fx1)), int(math.floor(fy1))
    dx, dy = fx1 - fx0, fy1 - fy0
    sx, sy = (1 if jx > ix else -1), (1 if jy > iy else -1)
    nx, ny = abs(jx - ix), abs(jy - iy)
    tdx = (1.0 / abs(dx)) if nx else math.inf
    tdy = (1.0 / abs(dy)) if ny else math.inf
    tx0 = ((((ix + 1) if sx > 0 else ix) - fx0) / dx) if nx else math.inf
    ty0 = ((((iy + 1) if sy > 0 else iy) - fy0) / dy) if ny else math.inf
    return ix, iy, jx, jy, sx, sy, nx, ny, tx0, tdx, ty0, tdy


def ray_cells(o, e, hw, hh, cs):
    """the cells (ox, oy) a ray from o to e visits, in order, the last one being the end's; None for a ray that is skipped (an
    origin or an end not strictly inside the frame)"""
    if not (inside(o, hw, hh) and inside(e, hw, hh)):
        return None
    ix, iy, jx, jy, sx, sy, nx, ny, tx0, tdx, ty0, tdy = ray_setup(o, e, hw, hh, cs)
    i = j = 0
    cells = [(ix, iy)]
    while i < nx or j < ny:
        if j == ny:
            step_x = True
        elif i == nx:
            step_x = False
        else:
            tx = tx0 + float(i) * tdx  # one multiplication, one addition
            ty = ty0 + float(j) * tdy
            step_x = tx <= ty          # a tie steps x first
        if step_x:
            i += 1
        else:
            j += 1
        cells.append((ix + sx * i, iy + sy * j))
    assert cells[-1] == (jx, jy)
    return cells


def end_points(xy, pose, cos_t, sin_t):
    """transform_point's rounding: rx = x c - y s, ry = x s + y c, then + t"""
    xy = np.asarray(xy, dtype=np.float64).reshape(-1, 2)
    rx = xy[:, 0] * cos_t - xy[:, 1] * sin_t
    ry = xy[:, 0] * sin_t + xy[:, 1] * cos_t
    return np.stack([rx + pose[0], ry + pose[1]], axis=1)


class Counters:
    """hits [h, w] uint32, passes [h, w] uint64 (entry [oy, ox] is og[ox + h * oy] of a square grid), extent and totals"""

    def __init__(self, width, height, og_cell_size):
        self.hw, self.hh, self.cs = width / 2., height / 2., float(og_cell_size)
        self.w, self.h = int(math.ceil(width / og_cell_size)), int(math.ceil(height / og_cell_size))
        assert self.w == self.h
        self.hits = np.zeros(self.w * self.h, dtype=np.uint32)
        self.passes = np.zeros(self.w * self.h, dtype=np.uint64)
        self.extent = [0xffffffff, 0, 0xffffffff, 0]
        self.n_rays = self.n_skipped = self.n_steps = 0

    def _at(self, c):
        at = c[0] + self.h * c[1]
        return at if at < self.hits.size else None   # (an entry beyond the grid is counted in the totals and not written)

    def trace(self, xy, pose, cos_t, sin_t):
        """one scan's rays: every visited cell but the last passes += 1, the last hits += 1"""
        o = (float(pose[0]), float(pose[1]))
        for e in end_points(xy, pose, cos_t, sin_t):
            cells = ray_cells(o, (float(e[0]), float(e[1])), self.hw, self.hh, self.cs)
            if cells is None:
                self.n_skipped += 1
                continue
            self.n_rays += 1
            self.n_steps += len(cells) - 1
            for c in cells[:-1]:
                if self._at(c) is not None:
                    self.passes[self._at(c)] += np.uint64(1)
            if self._at(cells[-1]) is not None:
                self.hits[self._at(cells[-1])] += np.uint32(1)
            xs, ys = (cells[0][0], cells[-1][0]), (cells[0][1], cells[-1][1])   # the staircase's bounding box is its ends'
            self.extent = [min(self.extent[0], *xs), max(self.extent[1], *xs), min(self.extent[2], *ys), max(self.extent[3], *ys)]
        return self

    def grids(self):
        return self.hits.reshape(self.h, self.w), self.passes.reshape(self.h, self.w)


def steps_of(xy, pose, cos_t, sin_t, width, height, og_cell_size):
    """(rays traced, rays skipped, sum of nx + ny) of a scan, vectorised: no per-step loop"""
    hw, hh, cs = width / 2., height / 2., float(og_cell_size)
    e = end_points(xy, pose, cos_t, sin_t)
    ok = (np.abs(e[:, 0]) < hw) & (np.abs(e[:, 1]) < hh) & (abs(pose[0]) < hw) & (abs(pose[1]) < hh)
    e = e[ok]
    ix, iy = math.floor((pose[0] + hw) / cs), math.floor((pose[1] + hh) / cs)
    jx, jy = np.floor((e[:, 0] + hw) / cs), np.floor((e[:, 1] + hh) / cs)
    return int(ok.sum()), int((~ok).sum()), int(np.abs(jx - ix).sum() + np.abs(jy - iy).sum())


def nav_grid(occupancy, hits, passes):
    """the three-state grid from ResidentMap.occupancy()'s bytes and the counters, all flat or all [h, w]: the reference's value
    where it is > 0, else -1 where nothing was counted, else (100 h + (h + p) / 2) / (h + p) in unsigned 64-bit arithmetic"""
    v = np.asarray(occupancy, dtype=np.int8)
    h = np.asarray(hits).astype(np.uint64).reshape(v.shape)
    p = np.asarray(passes).astype(np.uint64).reshape(v.shape)
    t = h + p
    ratio = (np.uint64(100) * h + t // np.uint64(2)) // np.maximum(t, np.uint64(1))
    out = np.where(t == 0, np.int8(-1), ratio.astype(np.int8))
    return np.where(v > 0, v, out).astype(np.int8)
