"""What the second-order conservative tests share: the mirror's inputs for a mesh pair, cell means of a smooth field by a fine
fan-subdivision quadrature, and the accuracy case (geodesic_mesh(8) and geodesic_mesh(16) onto vor1500).  Everything is computed once per
process and never modified."""
import functools

import numpy as np

import _mesh_conserve_ref as MR
import _mesh_to_mesh_cases as MC

ACCURACY_FREQS = (8, 16)
QUAD_LEVEL = 4          # every fan triangle is split into 4^4 = 256 triangles: a midpoint rule on cells 16 times finer than the cell


def field(xyz):
    """The smooth field of tests/test_patch_gpu.py, on [3][...] unit vectors."""
    x, y, z = xyz
    return np.sin(3 * x + 0.3) * np.cos(2 * y) + z ** 3 + 0.5 * x * z


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def cell_means(xyz, cnt, level=QUAD_LEVEL):
    """Mean of field() over every polygon (xyz [n][M][3], cnt [n]): each fan triangle (p_0, p_t, p_(t+1)) is split `level` times at its
    sides' spherical midpoints, the field is taken at every small triangle's normalised centroid and weighted with its spherical area."""
    n, M = xyz.shape[:2]
    num, den = np.zeros(n), np.zeros(n)
    for t in range(1, M - 1):
        on = np.flatnonzero(cnt > t + 1)
        if on.size == 0:
            break
        tri = np.stack([xyz[on, 0], xyz[on, t], xyz[on, t + 1]], axis=1)[:, None]          # [cells][1][3 corners][3]
        for _ in range(level):
            a, b, c = tri[:, :, 0], tri[:, :, 1], tri[:, :, 2]
            ab, bc, ca = _unit(a + b), _unit(b + c), _unit(c + a)
            tri = np.concatenate([np.stack(s, axis=2) for s in ((a, ab, ca), (ab, b, bc), (ca, bc, c), (ab, bc, ca))], axis=1)
        a, b, c = tri[:, :, 0], tri[:, :, 1], tri[:, :, 2]
        w = MR.tri_area(a, b, c)
        mid = _unit(a + b + c)
        f = field(np.moveaxis(mid, -1, 0))
        num[on] += (w * f).sum(axis=1)
        den[on] += w.sum(axis=1)
    return num / den


def neighbours_of(o, m):
    """patch_neighbours_mesh of a synthetic mesh, with the oracle's dual triangles."""
    from mpassit_amd import target_grid as tg
    tri, _ = o.dual_triangles(m.verticesOnCell, m.nVertices, MC.cell_xyz(o, m))
    return tg.patch_neighbours_mesh(m.verticesOnCell, tri)


_MIRROR = {}


def mirror(o, name, norm, first_order=False):
    """(rowptr, col, val, info) of the numpy mirror for pair `name` of tests/_mesh_to_mesh_cases.py on the REFERENCE's first-order pattern
    (tests/_mesh_conserve_ref.py): the CPU tests' input.  Cached."""
    from mpassit_amd import target_grid as tg
    key = (name, norm, first_order)
    if key not in _MIRROR:
        a = MR.answer(o, name)
        rp, col, _, _ = a.rows(norm)
        out = tg._conserve2nd_rows(rp, col, (a.ps[0], a.ps[1], MC.cell_xyz(o, a.src)), a.pd, neighbours_of(o, a.src), norm, first_order=first_order)
        for x in out[:3]:
            x.setflags(write=False)
        _MIRROR[key] = out
    return _MIRROR[key]


@functools.lru_cache(maxsize=None)
def accuracy_mesh(freq):
    from mpassit_amd import synth
    return synth.geodesic_mesh(freq)


_ACC = {}


def accuracy_case(o, freq):
    """The accuracy case at one source resolution: the reference Answer of geodesic_mesh(freq) -> vor1500, the source means and the true
    destination means of field() by quadrature.  Cached."""
    if freq not in _ACC:
        a = MR.Answer(o, accuracy_mesh(freq), MC.mesh("vor1500"))
        xs, xd = cell_means(*a.ps), cell_means(*a.pd)
        xs.setflags(write=False)
        xd.setflags(write=False)
        _ACC[freq] = (a, xs, xd)
    return _ACC[freq]


def rms_errors(rp1, col1, val1, rp2, col2, val2, areas, xs, xd):
    """(first-order RMS error, second-order RMS error, cells counted) of two DSTAREA patterns applied to the source means xs against the
    true destination means xd, over the destination cells whose sources are all fully covered.  areas = (area_s, area_d); a source is
    fully covered when its first-order column sum sum_j area_j w_je reaches its own area within 1e-9 of it."""
    area_s, area_d = areas
    n_dst = rp1.size - 1
    rows1 = np.repeat(np.arange(n_dst), np.diff(rp1))
    rows2 = np.repeat(np.arange(n_dst), np.diff(rp2))
    full = np.bincount(col1, weights=val1 * area_d[rows1], minlength=area_s.size) >= area_s * (1.0 - 1e-9)
    use = (np.bincount(rows1, weights=~full[col1], minlength=n_dst) == 0) & (np.diff(rp1) > 0)
    y1 = np.bincount(rows1, weights=val1 * xs[col1], minlength=n_dst)
    y2 = np.bincount(rows2, weights=val2 * xs[col2], minlength=n_dst)
    e1 = float(np.sqrt(np.mean((y1[use] - xd[use]) ** 2)))
    e2 = float(np.sqrt(np.mean((y2[use] - xd[use]) ** 2)))
    return e1, e2, int(use.sum())
