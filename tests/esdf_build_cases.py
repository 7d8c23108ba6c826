"""Cases of the ESDF build (vigo_build_esdf / vigo_esdf_from_voxels_host), named and seeded, shared by the CPU and the
GPU tests, and the two references: the all-pairs definition in numpy and the expression of synth.edt_esdf.

A case is (name, voxels uint8 [nx,ny,nz], plane, unknown_is_site, res).  Shapes: the minimum size, one bit into a second
word, exactly two words, a partial last word, and an axis of 300 (past a wave, a workgroup and any tile chunk) along z,
y and x; plus one 64^3 box world.  The build has ONE route for the y and x passes (global-memory scan,
csrc/vigo_esdf_build.hip), so no shape is there for a second one."""
import ctypes as C
import functools
import zlib

import numpy as np

from trajectory_planner_amd import _lib, synth

SMALL_SHAPES = [(2, 2, 2), (5, 7, 33), (3, 4, 64), (9, 70, 31), (2, 3, 300), (3, 300, 2), (300, 2, 3)]
CONTENTS = ["none", "all", "corners", "one_free", "slab_x", "slab_y", "slab_z", "checker", "rand02", "rand50", "rand98",
            "unknown_off", "unknown_on", "inflated_p0", "inflated_p2"]
WORLD_CASES = ["world64_p2", "world64_p0", "world64_p2_unknown"]
RANDOM_FILLS = ("rand02", "rand50", "rand98")


def _seed(name):
    return zlib.crc32(name.encode())


def _dilate1(m):
    """box dilation by one voxel (what the inflated plane is to the occupied one)"""
    out = m.copy()
    for ax in range(3):
        p = np.pad(out, [(1, 1) if a == ax else (0, 0) for a in range(3)])
        n = out.shape[ax]
        sl = lambda o: tuple(slice(o, o + n) if a == ax else slice(None) for a in range(3))
        out = p[sl(0)] | p[sl(1)] | p[sl(2)]
    return out


def small_case(shape, content):
    """-> (voxels, plane, unknown_is_site)"""
    nx, ny, nz = shape
    # (the two unknown_* cases share their voxels, and so do the two inflated_*: only the arguments differ)
    rng = np.random.default_rng(_seed(f"{nx}x{ny}x{nz}-{content.split('_')[0]}"))
    v = np.zeros(shape, dtype=np.uint8)
    plane, unk = 2, False
    if content == "none":
        pass
    elif content == "all":
        v[:] = 4
    elif content == "corners":
        for x in (0, nx - 1):
            for y in (0, ny - 1):
                for z in (0, nz - 1):
                    v[x, y, z] = 4
    elif content == "one_free":
        v[:] = 4
        v[tuple(int(rng.integers(0, n)) for n in shape)] = 0
    elif content.startswith("slab_"):
        ax = "xyz".index(content[-1])
        v[tuple(shape[ax] // 2 if a == ax else slice(None) for a in range(3))] = 4
    elif content == "checker":
        X, Y, Z = np.meshgrid(*[np.arange(n) for n in shape], indexing="ij")
        v[(X + Y + Z) % 2 == 0] = 4
    elif content in RANDOM_FILLS:
        v[rng.random(shape) < int(content[4:]) / 100.0] = 4
    elif content.startswith("unknown_"):
        r = rng.random(shape)
        v[r < 0.2] = 4
        v[(r >= 0.2) & (r < 0.4)] = 2            # disjoint from the occupied voxels
        unk = content == "unknown_on"
    elif content.startswith("inflated_"):
        occ = rng.random(shape) < 0.05
        v[occ] |= 4
        v[_dilate1(occ)] |= 1
        plane = 0 if content == "inflated_p0" else 2
    else:
        raise KeyError(content)
    return v, plane, unk


@functools.lru_cache(maxsize=None)
def world64():
    return synth.make_box_world(synth.SEED_BASE + 2, n=64, n_boxes=20, centre_range=2.5)


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (voxels, plane, unknown_is_site, res)"""
    if name in WORLD_CASES:
        w = world64()
        return w.voxels, (0 if "_p0" in name else 2), name.endswith("unknown"), float(w.res)
    dims, content = name.split("-")
    shape = tuple(int(t) for t in dims.split("x"))
    v, plane, unk = small_case(shape, content)
    return v, plane, unk, 0.1


SMALL_NAMES = [f"{s[0]}x{s[1]}x{s[2]}-{c}" for s in SMALL_SHAPES for c in CONTENTS]
ALL_NAMES = SMALL_NAMES + WORLD_CASES


def sites_of(vox, plane, unk):
    return (vox & ((1 << plane) | (2 if unk else 0))) != 0


def host_twin_raw(vox, plane, unk, res, out=None):
    """vigo_esdf_from_voxels_host -> (rc, lattice)"""
    vox = np.ascontiguousarray(vox, dtype=np.uint8)
    nx, ny, nz = vox.shape
    if out is None:
        out = np.empty(vox.shape, dtype=np.float32)
    rc = _lib.load().vigo_esdf_from_voxels_host(nx, ny, nz, vox.ctypes.data_as(C.c_void_p), int(plane), 1 if unk else 0,
                                                float(res), out.ctypes.data_as(C.c_void_p))
    return rc, out


@functools.lru_cache(maxsize=None)
def host_twin(name):
    """the host twin's lattice of a case, computed once and shared (read-only)"""
    vox, plane, unk, res = case(name)
    rc, out = host_twin_raw(vox, plane, unk, res)
    assert rc == 0, rc
    out.setflags(write=False)
    return out


def brute_d2(member):
    """All-pairs definition: min dx^2 + dy^2 + dz^2 from every voxel to a voxel of `member`; nx^2 + ny^2 + nz^2
    everywhere when the set is empty.  Every pair is evaluated, as |p|^2 + |m|^2 - 2 p.m in float32 (integers below
    2^24 throughout for these shapes: exact)."""
    shape = member.shape
    E = int(sum(n * n for n in shape))
    assert 4 * E < 1 << 24
    pts = np.argwhere(np.ones(shape, dtype=bool)).astype(np.float32)
    m = pts[member.ravel()]
    out = np.full(len(pts), E, dtype=np.int64)
    if len(m):
        mm = (m * m).sum(1)
        for c in range(0, len(pts), 1024):
            p = pts[c:c + 1024]
            d = (p * p).sum(1)[:, None] + mm[None, :] - np.float32(2.0) * (p @ m.T)
            out[c:c + 1024] = d.min(1).astype(np.int64)
    return out.reshape(shape)


def compose(d2_site, d2_free, res):
    return ((np.sqrt(d2_site.astype(np.float64)) - np.sqrt(d2_free.astype(np.float64))) * res).astype(np.float32)


def brute_lattice(vox, plane, unk, res):
    s = sites_of(vox, plane, unk)
    return compose(brute_d2(s), brute_d2(~s), res)


def edt_lattice(vox, plane, unk, res):
    """synth.edt_esdf's expression on the case's sites (scipy)"""
    from scipy import ndimage
    occ = sites_of(vox, plane, unk)
    d = (ndimage.distance_transform_edt(~occ) - ndimage.distance_transform_edt(occ)) * res
    return np.ascontiguousarray(d.astype(np.float32))


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))
