"""Scenes of the ray-marcher's shape tests (test_render_shapes_cpu.py / test_render_shapes_gpu.py): volumes whose outer shape is
neither cubic nor a multiple of the 8^3 leaf, and isosurfaces that the faces of the volume cut.

All scenes are fp32 ``[z][y][x]``.  The soft-sphere recipe is the one of ``test_oracle_iso._two_spheres``: the maximum over the spheres
of ``clip((rad - r) / 4 + 0.5, 0, 1)`` (iso 0.5 at radius ``rad``), values below the threshold set to 0; centres are (x, y, z).

    A  (41, 70, 99)    two spheres inside the box: three different, odd extents, one 128^3 node
    B  (150, 43, 77)   two spheres, 1 x 1 x 2 nodes (x, y, z): the node table's strides differ from the leaf table's
    C  (45, 83, 150)   six spheres, each cut by one face of the volume; 2 x 1 x 1 nodes; the active box is the whole volume
    D  (9, 17, 25)     uniform noise filling the box: every brick on the high sides is partial, every face has crossings
    D' (3, 40, 61)     a slab thinner than a leaf, noise in [:, 5:35, 7:55]
    E  (17, 150, 300)  five discs (spheres cut by both z faces) in 3 x 2 x 1 nodes of which node (1, 0, 0) is empty: the only node table
                       with two extents above 1 that differ.  On 1 x 1 x 2 and 2 x 1 x 1 every permutation of the node strides
                       addresses the same entry; here two swapped strides look up the empty node for an occupied one
"""
import functools

import numpy as np

SPHERES_A = [((24.0, 22.0, 18.0), 12.0), ((80.0, 52.0, 27.0), 7.0)]
SPHERES_B = [((20.0, 20.0, 30.0), 12.0), ((58.0, 26.0, 131.0), 9.0)]
SPHERES_C = [((0.0, 40.0, 20.0), 14.0), ((149.0, 30.0, 25.0), 12.0), ((70.0, 0.0, 22.0), 11.0), ((60.0, 82.0, 20.0), 13.0),
             ((100.0, 45.0, 0.0), 12.0), ((40.0, 50.0, 44.0), 10.0)]
SPHERES_E = [((30.0, 40.0, 8.0), 22.0), ((280.0, 30.0, 8.0), 13.0), ((100.0, 126.0, 8.0), 20.0), ((190.0, 139.0, 8.0), 8.0),
             ((281.0, 138.0, 8.0), 9.0)]


def soft_spheres(shape, spheres, threshold):
    nz, ny, nx = shape
    z, y, x = np.meshgrid(np.arange(nz, dtype=np.float32), np.arange(ny, dtype=np.float32), np.arange(nx, dtype=np.float32), indexing="ij")
    v = np.zeros(shape, np.float32)
    for (cx, cy, cz), rad in spheres:
        r = np.sqrt((x - cx) ** 2 + (y - cy) ** 2 + (z - cz) ** 2)
        v = np.maximum(v, np.clip((rad - r) / 4.0 + 0.5, 0.0, 1.0).astype(np.float32))
    v[v < threshold] = 0.0
    return v


def _frozen(v):
    v.setflags(write=False)          # computed once, shared by every test of a session
    return v


@functools.lru_cache(maxsize=None)
def scene_a():
    return _frozen(soft_spheres((41, 70, 99), SPHERES_A, 1e-3)), SPHERES_A


@functools.lru_cache(maxsize=None)
def scene_b():
    return _frozen(soft_spheres((150, 43, 77), SPHERES_B, 1e-3)), SPHERES_B


@functools.lru_cache(maxsize=None)
def scene_c():
    return _frozen(soft_spheres((45, 83, 150), SPHERES_C, 0.02))


@functools.lru_cache(maxsize=None)
def scene_c_padded():
    """Scene C with zeros up to the next multiple of 8 on every axis: the same bricks, none of them partial."""
    c = scene_c()
    v = np.zeros((48, 88, 152), np.float32)
    v[:c.shape[0], :c.shape[1], :c.shape[2]] = c
    return _frozen(v)


@functools.lru_cache(maxsize=None)
def scene_e():
    return _frozen(soft_spheres((17, 150, 300), SPHERES_E, 1e-3))


@functools.lru_cache(maxsize=None)
def scene_d():
    return _frozen(np.random.default_rng(9).random((9, 17, 25), dtype=np.float32))


@functools.lru_cache(maxsize=None)
def scene_d_thin():
    v = np.zeros((3, 40, 61), np.float32)
    v[:, 5:35, 7:55] = np.random.default_rng(3).random((3, 30, 48), dtype=np.float32)
    return _frozen(v)


def active_box_info(vol):
    """``scale`` / ``translation`` of the CPU semantics' world map (the longest edge of the active voxel box -> 1, centred) and the
    box of the occupied 8^3 bricks that ``semantics=gvdb`` normalises by, both from the data alone."""
    nz = np.argwhere(vol != 0)
    lo, hi = nz.min(0)[::-1].astype(float), nz.max(0)[::-1].astype(float)
    scale = 1.0 / (hi - lo).max()
    lo8, hi8 = (nz.min(0)[::-1] // 8) * 8, (nz.max(0)[::-1] // 8 + 1) * 8
    return {"scale": scale, "translation": list(-(lo + (hi - lo) / 2) * scale),
            "node_bbox_min": [int(v) for v in lo8], "node_bbox_max": [int(v) for v in hi8]}
