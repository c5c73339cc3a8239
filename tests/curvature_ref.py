"""Restatement of ndtpso_map_curvature's contract (include/ndtpso_hip.h) in numpy fp64, shared by tests/test_map_curvature_api.py
and tests/test_gpu_map_curvature.py: cost_function (core.cpp:26-48) with normalDistribution (ndtcell.cpp:70-78), differentiated
once and twice by the pose, point by point in the contract's operation order (numpy's elementwise operations do not fuse).

Membership comes from np_ref.cell_index and is held fixed: for a complex pose (complex-step derivatives) it is the real part's.
cos, sin and the exponential are passed in, so that on the GPU they are the device's own (ctx.device_math) and its last-bit
choices are not part of a comparison.

Besides every output the restatement returns its magnitude M: the same sum with every product replaced by its absolute value,
e.g. sum e (|h_kl| / 2 + |g_k| |g_l| / 4) with |g| and |h| themselves sums of absolute products.  The tolerance everywhere is
    |got - want| <= 2^-53 (n_points + 64) M
derived, not measured: a sum of n terms in any order errs by at most (n - 1) u sum |t|, and fewer than 64 roundings go into a
term, each relative to a product counted in M."""
import math

import numpy as np

import np_ref

U = 2.0 ** -53
NAMES = ("cost", "gx", "gy", "gth", "hxx", "hxy", "hxth", "hyy", "hyth", "hthth")


def cells_of(rows):
    """{index: (mean, icov)} of the built cells, from ResidentMap.cells() rows or np_ref.build_cells' dict"""
    if isinstance(rows, dict):
        return {k: (tuple(c["mean"]), tuple(c["icov"])) for k, c in rows.items() if c["built"]}
    return {int(r["index"]): (tuple(float(v) for v in r["mean"]), tuple(float(v) for v in r["icov"])) for r in rows if r["built"]}


def tolerance(n_points, M):
    return U * (n_points + 64) * np.asarray(M)


def _seq_sum(t):
    """the terms added one after the other"""
    t = np.asarray(t)
    return t.cumsum()[-1] if t.size else t.dtype.type(0)


def point_terms(cells, grid, xy, pose, c, s):
    """Per point of xy [n, 2] under `pose` with c, s = cos, sin of its heading: the mask of the points that land in a built cell,
    the exponent x = -Q / 2 (0 where the mask is off), and g [n, 3], h [n, 6], |g|, |h| as the contract defines them.
    grid = (width, height, cell_side)."""
    width, height, cs = grid
    xy = np.asarray(xy, dtype=np.float64).reshape(-1, 2)
    n = xy.shape[0]
    x, y = xy[:, 0], xy[:, 1]
    tx, ty = pose[0], pose[1]
    rx = x * c - y * s
    ry = x * s + y * c
    qx = rx + tx
    qy = ry + ty
    W, H = int(math.ceil(width / cs)), int(math.ceil(height / cs))
    hit = np.zeros(n, dtype=bool)
    mu = np.zeros((n, 2))
    A = np.zeros((n, 4))
    for i in range(n):
        k = np_ref.cell_index(float(np.real(qx[i])), float(np.real(qy[i])), width, height, cs)
        if k != -1 and k < W * H and k in cells:
            hit[i] = True
            mu[i], A[i] = cells[k]
    a00, a01, a10, a11 = A[:, 0], A[:, 1], A[:, 2], A[:, 3]
    d0 = qx - mu[:, 0]
    d1 = qy - mu[:, 1]
    r0 = d0 * a00 + d1 * a10
    r1 = d0 * a01 + d1 * a11
    Q = r0 * d0 + r1 * d1
    xarg = np.where(hit, -Q / 2.0, 0.0)
    b00, b01, b11 = 2.0 * a00, a01 + a10, 2.0 * a11
    v0 = b00 * d0 + b01 * d1
    v1 = b01 * d0 + b11 * d1
    g = np.stack([v0, v1, -ry * v0 + rx * v1], axis=1)
    h02 = -b00 * ry + b01 * rx
    h12 = -b01 * ry + b11 * rx
    h22 = ry * ry * b00 - 2.0 * rx * ry * b01 + rx * rx * b11 - (v0 * rx + v1 * ry)
    zero = np.zeros_like(h02)
    h = np.stack([b00 + zero, b01 + zero, h02, b11 + zero, h12, h22], axis=1)
    ab = np.abs
    B00, B01, B11 = 2.0 * ab(a00), ab(a01) + ab(a10), 2.0 * ab(a11)
    V0 = B00 * ab(d0) + B01 * ab(d1)
    V1 = B01 * ab(d0) + B11 * ab(d1)
    G = np.stack([V0, V1, ab(ry) * V0 + ab(rx) * V1], axis=1)
    H02 = B00 * ab(ry) + B01 * ab(rx)
    H12 = B01 * ab(ry) + B11 * ab(rx)
    H22 = ab(ry) ** 2 * B00 + 2.0 * ab(rx) * ab(ry) * B01 + ab(rx) ** 2 * B11 + (V0 * ab(rx) + V1 * ab(ry))
    Hm = np.stack([B00, B01, H02, B11, H12, H22], axis=1)
    return dict(hit=hit, x=xarg, g=g, h=h, G=G, H=Hm, n=n)


_KL = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))


def sums(t, e):
    """The ten sums and their magnitudes from point_terms' output and e = exp(t["x"]) per point.  A point outside the mask, or
    with e == 0, contributes exactly zero; a NaN e makes every sum NaN."""
    e = np.asarray(e)
    live = t["hit"] & ~(e == 0)
    e, g, h, G, Hm = e[live], t["g"][live], t["h"][live], t["G"][live], t["H"][live]
    ea = np.abs(e)
    out = np.zeros(10, dtype=e.dtype if e.size else np.float64)
    M = np.zeros(10)
    out[0] = -_seq_sum(e)
    M[0] = _seq_sum(ea)
    for k in range(3):
        out[1 + k] = _seq_sum(e * g[:, k] / 2.0)
        M[1 + k] = _seq_sum(ea * G[:, k] / 2.0)
    for i, (k, l) in enumerate(_KL):
        out[4 + i] = _seq_sum(e * (h[:, i] / 2.0 - g[:, k] * g[:, l] / 4.0))
        M[4 + i] = _seq_sum(ea * (Hm[:, i] / 2.0 + G[:, k] * G[:, l] / 4.0))
    return out, M, int(t["hit"].sum())


def curvature(cells, grid, xy, pose, c=None, s=None, exp=np.exp):
    """(the ten sums in NAMES' order, their magnitudes M, n_hit) at `pose` (real or complex); c, s default to numpy's cos / sin
    of the heading, `exp` maps the exponents to the terms e."""
    if c is None:
        c, s = np.cos(pose[2]), np.sin(pose[2])
    t = point_terms(cells, grid, xy, pose, c, s)
    return sums(t, exp(t["x"]))
