"""The leaf scan of a tiny scene (mega.hip / dscan.h: centre / half-extent box records) on the rays a slab test gets wrong first: origins
ON the scene's surfaces — and therefore on, or within rounding of, the faces of the leaf boxes that hold those surfaces — with directions
along an axis, with one or two components of exactly zero or of 1e-20 (below the scan's 1e-18 clamp), or lying in the surface's own plane.
Closest hits and occlusion through the scan must equal the BVH route (LJ_TUNE_MEGA=0) and the CPU oracle bit for bit: a box the scan
wrongly skips shows as a missing or farther hit."""
import os

import numpy as np
import pytest

import lajolla_public_amd as lj
from lajolla_public_amd import _abi
from helpers import Oracle, random_rays, scene_path

N_RAYS = 20000


class _wavefront:
    """LJ_TUNE_MEGA=0 for the duration: the library then traces tiny scenes with the general BVH kernels."""

    def __enter__(self):
        os.environ["LJ_TUNE_MEGA"] = "0"

    def __exit__(self, *a):
        os.environ.pop("LJ_TUNE_MEGA", None)


def _surface_frames(hs, hits):
    """Unit normal of the surface at each hit (triangles: of the float vertices' plane; spheres: the radius through the hit point)."""
    d = hs.desc
    n = np.zeros((len(hits), 3))
    for si in np.unique(hits["shape_id"]):
        sh = d.shapes[int(si)]
        rows = np.flatnonzero(hits["shape_id"] == si)
        if sh.kind == _abi.LJ_SHAPE_SPHERE:
            n[rows] = hits["_p"][rows] - np.array(sh.position[:])
        else:
            P = np.ctypeslib.as_array(d.positions, (d.n_vertices * 3,)).reshape(-1, 3)[sh.first_vertex:sh.first_vertex + sh.n_vertices]
            I = np.ctypeslib.as_array(d.indices, (d.n_triangles * 3,)).reshape(-1, 3)[sh.first_triangle:sh.first_triangle + sh.n_triangles]
            tri = P[I[hits["prim_id"][rows]]]
            n[rows] = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    return n / np.linalg.norm(n, axis=1, keepdims=True)


def edge_rays(hs, oracle, n=N_RAYS, seed=17):
    """`n` rays from hit points of random rays (the oracle's), a quarter each: along +-axis | one or two components exactly zero |
    one or two components of +-1e-20 | in the plane of the surface the origin lies on."""
    rng = np.random.default_rng(seed)
    seedrays = random_rays(hs, 4 * n, seed, oracle)
    h0 = oracle.intersect(seedrays)
    keep = np.flatnonzero(h0["shape_id"] >= 0)[:n]
    assert len(keep) == n
    p = (seedrays["org"][keep].astype(np.float64) + h0["t"][keep, None].astype(np.float64) * seedrays["dir"][keep]).astype(np.float32)
    hits = np.zeros(n, np.dtype([("shape_id", np.int32), ("prim_id", np.int32), ("_p", np.float64, 3)]))
    hits["shape_id"], hits["prim_id"], hits["_p"] = h0["shape_id"][keep], h0["prim_id"][keep], p
    nrm = _surface_frames(hs, hits)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    kind = np.arange(n) % 4
    # 0: along an axis
    axis, sign = rng.integers(0, 3, n), rng.choice([-1.0, 1.0], n)
    m = kind == 0
    d[m] = 0.0
    d[m, axis[m]] = sign[m]
    # 1 / 2: one or two of the components (never the largest) exactly zero / +-1e-20
    order = np.argsort(np.abs(d), axis=1)
    two = rng.random(n) < 0.5
    for k, value in ((1, 0.0), (2, 1e-20)):
        rows = np.flatnonzero(kind == k)
        d[rows, order[rows, 0]] = value * rng.choice([-1.0, 1.0], len(rows))
        rows2 = rows[two[rows]]
        d[rows2, order[rows2, 1]] = value * rng.choice([-1.0, 1.0], len(rows2))
    # 3: in the surface's plane
    m = kind == 3
    t = np.cross(nrm[m], d[m])
    d[m] = t / np.linalg.norm(t, axis=1, keepdims=True)
    return lj._rays_array(p, d, 0.0, np.inf)


_cache = {}


def _setup(name):
    """Per scene, once: the rays and what the oracle says about them (closest hits; occlusion of the bounded segments)."""
    if name not in _cache:
        hs = lj.parse_scene(scene_path(name))
        o = Oracle(hs)
        rays = edge_rays(hs, o)
        tb = o.tables()
        seg = rays.copy()
        seg["tnear"] = np.float32(tb["shadow_epsilon"])
        seg["tfar"] = (np.random.default_rng(5).random(len(rays)) * tb["bounds_radius"]).astype(np.float32)
        _cache[name] = dict(hs=hs, rays=rays, seg=seg, hits=o.intersect(rays), occ=o.occluded(seg))
    return _cache[name]


@pytest.mark.parametrize("name", ["cbox", "veach_mi"])
def test_oracle_alone_sees_both_outcomes_on_the_edge_rays(name):
    s = _setup(name)
    hit = (s["hits"]["shape_id"] >= 0).mean()
    print(f"{name}: oracle hit share {hit:.3f}, occluded share {s['occ'].mean():.3f}")
    assert 0.05 < hit < 0.95 and 0.05 < s["occ"].mean() < 0.95


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cbox", "veach_mi"])
def test_scan_on_surface_origins_and_degenerate_directions_equals_bvh_and_oracle(name):
    s = _setup(name)
    rays, seg = s["rays"], s["seg"]
    sc = lj.Scene(lj.Context(0), s["hs"])
    h_scan = lj.intersect(sc, rays["org"], rays["dir"], 0.0, np.inf)
    assert sc.stats().mega_launches == 1 and sc.stats().extend_launches == 0, "the query was not answered by the leaf scan"
    with _wavefront():
        h_bvh = lj.intersect(sc, rays["org"], rays["dir"], 0.0, np.inf)
        assert sc.stats().mega_launches == 0 and sc.stats().extend_launches == 1, "LJ_TUNE_MEGA=0 did not select the BVH traversal"
    for f in ("t", "u", "v", "shape_id", "prim_id"):
        assert np.array_equal(h_scan[f].view(np.uint32), s["hits"][f].view(np.uint32)), f"scan vs oracle: {f}"
        assert np.array_equal(h_scan[f].view(np.uint32), h_bvh[f].view(np.uint32)), f"scan vs BVH: {f}"
    occ_scan = lj.occluded(sc, seg["org"], seg["dir"], seg["tnear"], seg["tfar"])
    assert sc.stats().mega_launches == 1
    with _wavefront():
        occ_bvh = lj.occluded(sc, seg["org"], seg["dir"], seg["tnear"], seg["tfar"])
    assert np.array_equal(occ_scan, s["occ"]) and np.array_equal(occ_scan, occ_bvh)
    hit = (h_scan["shape_id"] >= 0).mean()
    assert 0.05 < hit < 0.95 and 0.05 < occ_scan.mean() < 0.95
