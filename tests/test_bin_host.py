"""The cell rule of the map match through a cell grid on the host (tests/bin_host.py): the numpy statement equals the g++ build of
coloc_amd/csrc/bin_math.h exactly, every window is at most 3 x 3 cells and holds every row that passes the gate (the g++ build of
proj_in_radius, tests/proj_host.py), and the table builder counts and orders the rows as it says."""
import numpy as np

import bin_host as bh
import guided_host as gh
import proj_host as ph

CAM = gh.CAM_EXACT                                         # ppx 320, ppy 240: W = 640, W / 64 = 10
RADII = [0.001, 2.0 ** -11, 2.0 ** -10, 0.37, 1.0, 3.0, 8.0, 9.99, 10.0, 10.01, 17.3, 40.0, 79.9]


def _ulps(v):
    v = np.asarray(v, dtype=np.float64)
    return np.concatenate([v, np.nextafter(v, np.inf), np.nextafter(v, -np.inf)])


def _adversarial(c):
    """float64 values: every cell border, one ulp either side, the ring, far outside, the zeros, the infinities, NaN"""
    borders = np.arange(-3, 68) * c
    special = np.array([0.0, -0.0, 1e30, -1e30, np.inf, -np.inf, np.nan, 64.0 * c, 65.0 * c, -c, 5e-324, -5e-324])
    return np.concatenate([_ulps(borders), special])


def test_grid_and_k_equal_the_gxx_build():
    rng = np.random.RandomState(1)
    for cam in (CAM, (500.0, 240.0, 320.0, 0, 0, 0), (500.0, 0.37, 0.11, 0, 0, 0), (500.0, 1e6, 3.0, 0, 0, 0)):
        for radius in RADII:
            g = bh.grid(cam, radius)
            assert g == bh.cxx_grid(cam, radius), (cam, radius)
            rw, W, c = g
            assert c >= rw and c >= W / 64.0 and (c == rw or c == W / 64.0)
            v = np.concatenate([_adversarial(c), rng.uniform(-3 * c, 68 * c, 4000), rng.normal(0, 1e3, 1000)])
            got, want = bh.k(v, c), bh.cxx_k(v, c)
            assert np.array_equal(got, want), (cam, radius)
            assert got.min() == 0 and got.max() == 65
    c = 10.0
    assert bh.k(np.array([0.0, -0.0, 9.999999999, 10.0, 639.99, 640.0, -1e-300, 1e30, -1e30, np.nan, np.inf, -np.inf]), c).tolist() == \
        [1, 1, 1, 2, 64, 65, 0, 65, 0, 0, 65, 0]


def _points(rng, c, n):
    """float32 points (n, 2): on cell borders, one float32 ulp either side, inside, in the ring, far outside, NaN"""
    b = (rng.randint(-2, 67, (n, 2)) * c).astype(np.float32)
    kind = rng.randint(0, 8, n)
    pts = np.where((kind == 0)[:, None], b, rng.uniform(-2 * c, 66 * c, (n, 2)).astype(np.float32))
    pts = np.where((kind == 1)[:, None], np.nextafter(b, np.float32(np.inf)), pts)
    pts = np.where((kind == 2)[:, None], np.nextafter(b, np.float32(-np.inf)), pts)
    pts = pts.astype(np.float32)
    far = np.array([[1e30, 5.0], [-1e30, -1e30], [3.0, 1e30], [np.inf, 7.0], [-0.0, 0.0], [np.nan, np.nan], [np.nan, 4.0]], dtype=np.float32)
    pts[:len(far)] = far[:n]
    return pts


def test_cells_and_windows_equal_the_gxx_build_and_windows_are_3_by_3():
    rng = np.random.RandomState(2)
    for radius in RADII:
        rw, W, c = bh.grid(CAM, radius)
        pts = _points(rng, c, 3000)
        cl = bh.cells(pts, c)
        assert np.array_equal(cl, bh.cxx_cells(pts, c)), radius
        assert (cl[np.isnan(pts).any(1)] == -1).all() and cl.max() < bh.CELLS and (cl[~np.isnan(pts).any(1)] >= 0).all()
        w = bh.windows(pts, rw, c)
        assert np.array_equal(w, bh.cxx_windows(pts, rw, c)), radius
        has = ~np.isnan(pts).any(1)
        assert (w[~has] == (1, 0, 1, 0)).all()
        nx, ny = w[has, 1] - w[has, 0], w[has, 3] - w[has, 2]
        assert nx.min() >= 0 and ny.min() >= 0 and nx.max() <= 2 and ny.max() <= 2, radius          # at most 3 x 3 cells
        assert w[has].min() >= 0 and w[has].max() <= 65
    assert (bh.k(np.array([np.nan]), 10.0) == 0).all()


def test_the_window_holds_every_candidate():
    """queries snapped onto cell borders (and a float32 ulp either side, in the ring, far outside), rows planted at radius (1 +- 1e-7)
    from them in sixteen directions, and projections of 1e30 and NaN among them: every row the g++ gate passes lies in the query's
    window.  Zero misses allowed."""
    rng = np.random.RandomState(3)
    radii = np.concatenate([[0.001, 79.9, 2.0 ** -10, 10.0, 8.0], np.exp(rng.uniform(np.log(0.001), np.log(79.9), 35))])
    ang = np.arange(16) * (np.pi / 8)
    dirs = np.column_stack([np.cos(ang), np.sin(ang)])
    queries = candidates = missed = 0
    for radius in radii:
        rw, W, c = bh.grid(CAM, radius)
        r2 = ph.r2_of(radius)
        q = _points(rng, c, 520)
        w = bh.windows(q, rw, c)
        for i in range(len(q)):
            scale = np.float64(np.float32(radius)) * (1.0 + rng.choice([-1e-7, 1e-7, 0.0, -1e-3], 16))
            rows = (q[i].astype(np.float64) + dirs * scale[:, None]).astype(np.float32)
            rows = np.concatenate([rows, q[i:i + 1], np.array([[1e30, 1e30], [np.nan, np.nan]], dtype=np.float32)])
            cand = ph.gate(q[i], rows, r2)
            if not cand.any():
                continue
            cl = bh.cells(rows[cand], c)
            kx, ky = cl % bh.AXIS, cl // bh.AXIS
            inside = (kx >= w[i, 0]) & (kx <= w[i, 1]) & (ky >= w[i, 2]) & (ky <= w[i, 3])
            candidates += int(cand.sum())
            missed += int((~inside).sum())
        queries += len(q)
    print("superset: %d queries, %d candidates, %d missed" % (queries, candidates, missed))
    assert queries >= 20000 and candidates > 50000
    assert missed == 0


def test_the_table_builder():
    rng = np.random.RandomState(4)
    rw, W, c = bh.grid(CAM, 3.0)
    proj = _points(rng, c, 1000)
    cell_start, cell_row = bh.table(proj, c)
    cl = bh.cells(proj, c)
    assert len(cell_start) == bh.CELLS + 1 and cell_start[0] == 0 and cell_start[-1] == (cl >= 0).sum() == len(cell_row)
    assert (np.diff(cell_start) >= 0).all()
    for cell in np.unique(cl[cl >= 0]):
        rows = cell_row[cell_start[cell]:cell_start[cell + 1]]
        assert np.array_equal(rows, np.nonzero(cl == cell)[0])
    assert set(cell_row.tolist()) == set(np.nonzero(cl >= 0)[0].tolist())
    # what a query visits: the rows of its window's cells, counted from the table
    q = _points(rng, c, 50)
    n = bh.visited(q, proj, rw, c)
    w = bh.windows(q, rw, c)
    kx, ky = cl % bh.AXIS, cl // bh.AXIS
    for i in range(len(q)):
        want = ((cl >= 0) & (kx >= w[i, 0]) & (kx <= w[i, 1]) & (ky >= w[i, 2]) & (ky <= w[i, 3])).sum()
        assert n[i] == want

